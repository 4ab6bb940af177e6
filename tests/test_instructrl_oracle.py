"""Pins tests/instructrl_oracle.py (numpy float64, hidden keys at -inf) to a line-by-line torch restatement of the reference's own statements
(arp_dt/models/m3ae/model.py:471-496 forward_representation, :232-259 Attention.__call__ with padding_mask, :262-312 Block / Transformer), which replaces
a padded key's score by -1e7, not -inf.  No GPU."""
import numpy as np
import torch

import instructrl_oracle as I
from arp_amd import synth_policy as S
from oracle import m3ae_np as M

KW = dict(patch=16, width=128, layers=2, heads=2, img_res=64)


def _t(P, k):
    return torch.from_numpy(np.asarray(P[k], np.float64))


def _pos_1d(embed_dim, pos):
    """get_1d_sincos_pos_embed_from_grid (model.py:95-108)"""
    omega = torch.arange(embed_dim // 2, dtype=torch.float64)
    omega /= embed_dim / 2.0
    omega = 1.0 / 10000 ** omega
    out = torch.einsum("m,d->md", pos.reshape(-1), omega)
    return torch.cat([torch.sin(out), torch.cos(out)], dim=1)


def _pos_2d(embed_dim, length):
    """get_2d_sincos_pos_embed (model.py:118-136)"""
    gs = int(length ** 0.5)
    grid_h = torch.arange(gs, dtype=torch.float64)
    grid_w = torch.arange(gs, dtype=torch.float64)
    grid = torch.stack(torch.meshgrid(grid_w, grid_h, indexing="xy"), dim=0).reshape(2, 1, gs, gs)
    return torch.cat([_pos_1d(embed_dim // 2, grid[0]), _pos_1d(embed_dim // 2, grid[1])], dim=1)[None]


def _attention(P, p, cfg, inputs, padding_mask):
    """model.py:232-259"""
    batch, n, channels = inputs.shape
    scale = (cfg.width // cfg.heads) ** -0.5
    qkv = inputs @ _t(P, p + "Attention_0/Dense_0/kernel") + _t(P, p + "Attention_0/Dense_0/bias")
    qkv = qkv.reshape(batch, n, 3, cfg.heads, channels // cfg.heads).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    attention = (q @ k.transpose(-2, -1)) * scale
    if padding_mask is not None:
        pm = padding_mask[:, None, None, :].expand(attention.shape)
        attention = torch.where(pm > 0, torch.tensor(-1e7, dtype=torch.float64), attention)
    attention = torch.softmax(attention, dim=-1)
    x = (attention @ v).transpose(1, 2).reshape(batch, n, channels)
    return x @ _t(P, p + "Attention_0/Dense_1/kernel") + _t(P, p + "Attention_0/Dense_1/bias")


def _ln(P, p, x):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), _t(P, p + "/scale"), _t(P, p + "/bias"), eps=1e-6)


def _reference(P, cfg, image_patches, text, text_padding_mask):
    """model.py:471-496 on patchified frames, then the Transformer (:286-312)"""
    batch_size = image_patches.shape[0]
    cls_token = _t(P, "cls_token").expand(batch_size, 1, cfg.width)
    input_tensors = [cls_token]
    padding_masks = [torch.zeros((batch_size, 1), dtype=torch.float64)]
    image_x = (image_patches @ _t(P, "image_embedding/kernel") + _t(P, "image_embedding/bias")
               + _pos_2d(cfg.width, image_patches.shape[1]) + _t(P, "encoder_image_type_embedding"))
    input_tensors.append(image_x)
    padding_masks.append(torch.zeros((batch_size, image_patches.shape[1]), dtype=torch.float64))
    text_x = (_t(P, "text_embedding/embedding")[text]
              + _pos_1d(cfg.width, torch.arange(text.shape[1], dtype=torch.float64))[None] + _t(P, "encoder_text_type_embedding"))
    input_tensors.append(text_x)
    padding_masks.append(text_padding_mask)
    x = torch.cat(input_tensors, dim=1)
    padding_mask = torch.cat(padding_masks, dim=1)
    for i in range(cfg.layers):
        p = f"encoder/Block_{i}/"
        x = x + _attention(P, p, cfg, _ln(P, p + "LayerNorm_0", x), padding_mask)
        y = _ln(P, p + "LayerNorm_1", x)
        y = torch.nn.functional.gelu(y @ _t(P, p + "TransformerMLP_0/fc1/kernel") + _t(P, p + "TransformerMLP_0/fc1/bias"), approximate="tanh")
        x = x + y @ _t(P, p + "TransformerMLP_0/fc2/kernel") + _t(P, p + "TransformerMLP_0/fc2/bias")
    return _ln(P, "encoder/LayerNorm_0", x).numpy()


def test_oracle_is_the_reference_statements():
    cfg = M.EncConfig(**KW)
    P = S.add_m3ae_text_params(S.m3ae_params(cfg, seed=3), cfg, vocab=97, seed=3)
    frames = S.normalized_frames(3, cfg.img_res, seed=4).astype(np.float64)
    patches = torch.from_numpy(M.patchify(frames, cfg.patch))
    rng = np.random.default_rng(5)
    L = 13
    tok = rng.integers(0, 97, (3, L))
    masks = {"suffix": np.tile((np.arange(L) >= 5).astype(np.float64), (3, 1)), "none": np.zeros((3, L)), "all": np.ones((3, L)),
             "scattered": (rng.random((3, L)) < 0.5).astype(np.float64)}
    for name, mask in masks.items():
        want = _reference(P, cfg, patches, torch.from_numpy(tok), torch.from_numpy(mask))
        got = I.forward_representation(P, cfg, frames, tok, mask)
        assert got.shape == want.shape == (3, 1 + 16 + L, cfg.width)
        assert np.abs(got - want).max() < 1e-12, name
    # one instruction shared by the frames == the same instruction on every row
    shared = I.forward_representation(P, cfg, frames, tok[0], masks["suffix"][0])
    rows = I.forward_representation(P, cfg, frames, np.tile(tok[0], (3, 1)), masks["suffix"])
    assert np.abs(shared - rows).max() < 1e-12
    # the instruction matters, and a padded token's id does not reach any VISIBLE row... except its own (a padded token is still a query)
    other = tok.copy()
    other[:, 7] = (other[:, 7] + 1) % 97
    a = I.forward_representation(P, cfg, frames, tok, masks["suffix"])
    b = I.forward_representation(P, cfg, frames, other, masks["suffix"])
    keep = np.ones(1 + 16 + L, bool)
    keep[1 + 16 + 7] = False
    assert np.abs(a[:, keep] - b[:, keep]).max() < 1e-12 and np.abs(a[:, ~keep] - b[:, ~keep]).max() > 1e-3
    assert np.abs(a - I.forward_representation(P, cfg, frames, tok, masks["none"])).max() > 1e-3


def test_text_params_leave_the_image_tree_alone():
    cfg = M.EncConfig(**KW)
    P = S.m3ae_params(cfg, seed=3)
    Q = S.add_m3ae_text_params(P, cfg, vocab=97, seed=3)
    assert set(Q) - set(P) == {"text_embedding/embedding", "encoder_text_type_embedding"}
    assert Q["text_embedding/embedding"].shape == (97, cfg.width) and Q["encoder_text_type_embedding"].shape == (1, 1, cfg.width)
    again = S.m3ae_params(cfg, seed=3)
    assert all((P[k] == again[k]).all() and Q[k] is P[k] for k in P)
