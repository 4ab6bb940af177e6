"""Oracle (test infrastructure): the image + text call of the frozen M3AE encoder, numpy float64, in the style of tests/gcbc_oracle.py.

``MaskedMultimodalAutoencoder.forward_representation(image, text, text_padding_mask)`` (arp_dt/models/m3ae/model.py:471-496), which InstructRL's
``BC.encode`` calls under ``stop_gradient`` (arp_dt/BC.py:283-321):

  * one sequence per frame: class token, the frame's patches (image_embedding + 2-D sincos + image type embedding), then the L instruction tokens:
    ``text_embedding[token] + get_1d_sincos_pos_embed(width, L) + encoder_text_type_embedding`` (:485-491);
  * the padding mask is zero for the class token and the patches and ``text_padding_mask`` for the text (:475, :483, :492); where it is > 0 the KEY's score is
    replaced by -1e7 in every softmax of every block (:247-250) -- exactly weight 0 after exp in float32 and float64 as long as one key is visible, and the
    class token always is.  Here the hidden keys get -inf (gcbc_oracle.encode_tokens' key_mask); tests/test_instructrl_oracle.py pins the two to 1e-12;
  * padded tokens are still QUERIES and still get output rows; the encoder is the same Transformer (blocks, then a LayerNorm over all tokens).
"""
import numpy as np

import gcbc_oracle as G
from oracle import m3ae_np as M


def text_rows(P, cfg, tokens):
    """tokens int [L] -> [L, D]: text_embedding + 1-D sincos position embedding + text type embedding"""
    tokens = np.asarray(tokens)
    L = tokens.shape[-1]
    emb = np.asarray(P["text_embedding/embedding"], np.float64)[tokens]
    return emb + M.sincos_1d(cfg.width, np.arange(L, dtype=np.float64)) + np.asarray(P["encoder_text_type_embedding"], np.float64)[0]


def forward_representation(P, cfg, images, tokens, mask):
    """images float [n, res, res, 3]; tokens int and mask (> 0 = padded) [L], shared by the frames, or [n, L] -> [n, 1 + P + L, width] float64"""
    images, tokens, mask = np.asarray(images), np.asarray(tokens), np.asarray(mask)
    n = images.shape[0]
    if tokens.ndim == 2:
        assert tokens.shape[0] == n and mask.shape == tokens.shape
        return np.concatenate([forward_representation(P, cfg, images[i:i + 1], tokens[i], mask[i]) for i in range(n)], axis=0)
    assert mask.shape == tokens.shape
    patches = G.embed_patches(P, cfg, images)
    cls = np.broadcast_to(np.asarray(P["cls_token"], np.float64), (n, 1, cfg.width))
    txt = np.broadcast_to(text_rows(P, cfg, tokens), (n, tokens.shape[0], cfg.width))
    x = np.concatenate([cls, patches, txt], axis=1)
    visible = np.concatenate([np.ones(1 + patches.shape[1], bool), ~(mask > 0)])
    return G.encode_tokens(P, cfg, x, key_mask=visible)
