"""Oracle (test infrastructure): the goal-conditioned call of the frozen M3AE encoder, numpy float64, in the style of oracle/m3ae_np.py.

``MaskedMultimodalAutoencoder.forward_gc_representations(image, goal_image)`` (arp_dt/models/m3ae/model.py:498-525), which GCBC calls under
``stop_gradient`` where ARP-DT and BC call ``forward_representation`` (arp_dt/GCBC.py:462-468):

  * one sequence per (frame, goal) pair: class token, the frame's patches, the goal frame's patches (:502-522);
  * both patch blocks go through the same ``image_embedding`` and take the same ``get_2d_sincos_pos_embed`` and the same
    ``encoder_image_type_embedding`` (:505-517); the class token takes neither;
  * every padding mask is zero (:504, :511, :519): no key is masked;
  * the encoder is the same Transformer (blocks, then a LayerNorm over all tokens).

GCBC's policy is BC's (``diff BC.py GCBC.py``: an inlined copy of layers.py and the ``encode`` method), so the policy side is tests/bc_oracle.py as it is.
The data side, the hindsight goal row of arp_dt/data_procgen.py:186-189, is :func:`goal_row`.
"""
import numpy as np

from oracle import m3ae_np as M


def encode_tokens(P, cfg, x, key_mask=None):
    """The Transformer of m3ae/model.py:286-312 on a token sequence x [n, T, D] (float64): cfg.layers blocks, then the final LayerNorm.
    key_mask [T] bool (optional): keys that take part; the others get a score of -inf (the reference's padding mask)."""
    g = lambda k: np.asarray(P[k], np.float64)
    n, T, D = x.shape
    hd = D // cfg.heads
    for i in range(cfg.layers):
        p = f"encoder/Block_{i}/"
        y = M._ln(x, g(p + "LayerNorm_0/scale"), g(p + "LayerNorm_0/bias"))
        qkv = (y @ g(p + "Attention_0/Dense_0/kernel") + g(p + "Attention_0/Dense_0/bias")).reshape(n, T, 3, cfg.heads, hd)
        q, k, v = (qkv[:, :, j].transpose(0, 2, 1, 3) for j in range(3))
        s = q @ k.transpose(0, 1, 3, 2) * hd ** -0.5
        if key_mask is not None:
            s = np.where(np.asarray(key_mask, bool)[None, None, None, :], s, -np.inf)
        s = np.exp(s - s.max(-1, keepdims=True))
        s /= s.sum(-1, keepdims=True)
        y = (s @ v).transpose(0, 2, 1, 3).reshape(n, T, D)
        x = x + y @ g(p + "Attention_0/Dense_1/kernel") + g(p + "Attention_0/Dense_1/bias")
        y = M._ln(x, g(p + "LayerNorm_1/scale"), g(p + "LayerNorm_1/bias"))
        y = M._gelu_tanh(y @ g(p + "TransformerMLP_0/fc1/kernel") + g(p + "TransformerMLP_0/fc1/bias"))
        x = x + y @ g(p + "TransformerMLP_0/fc2/kernel") + g(p + "TransformerMLP_0/fc2/bias")
    return M._ln(x, g("encoder/LayerNorm_0/scale"), g("encoder/LayerNorm_0/bias"))


def embed_patches(P, cfg, images):
    """image_embedding(patchify(images)) + 2-D sincos position embedding + image type embedding -> [n, L, D]"""
    g = lambda k: np.asarray(P[k], np.float64)
    x = M.patchify(np.asarray(images, np.float64), cfg.patch)
    return x @ g("image_embedding/kernel") + g("image_embedding/bias") + M.sincos_2d(cfg.width, x.shape[1]) + g("encoder_image_type_embedding")[0]


def gc_tokens(P, cfg, images, goals):
    """the input sequence [n, 2 L + 1, D]: class token | frame patches | goal patches"""
    images, goals = np.asarray(images), np.asarray(goals)
    assert images.shape == goals.shape
    n = images.shape[0]
    cls = np.broadcast_to(np.asarray(P["cls_token"], np.float64), (n, 1, cfg.width))
    return np.concatenate([cls, embed_patches(P, cfg, images), embed_patches(P, cfg, goals)], axis=1)


def forward_gc_representations(P, cfg, images, goals):
    """images, goals: float [n, res, res, 3] (already normalised) -> [n, 2 L + 1, width] float64"""
    return encode_tokens(P, cfg, gc_tokens(P, cfg, images, goals))


def goal_row(rs, index, traj_end, n_rows):
    """data_procgen.py:187-189 for a processed row ``index`` whose trajectory ends (exclusively) at ``traj_end``: the row whose window is the goal frames"""
    return min(rs.choice(list(range(index, traj_end)), 1).item(), n_rows - 1)
