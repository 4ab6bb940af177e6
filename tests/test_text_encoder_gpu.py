"""The image + text pass of the frozen M3AE encoder (arp_enc_forward_text, M3AEEncoder.forward_representation(images, text, text_padding_mask)) against
tests/instructrl_oracle.py in float64, on seeded weights (synth_policy.m3ae_params + add_m3ae_text_params, vocabulary 97).

Small geometry (patch 16, width 128, 2 layers, 2 heads, 64 x 64 frames, L = 13 with 5 valid tokens: 30 rows) is one key block of the masked attention
kernels and isolates the text rows, the mask words and the row bookkeeping; the same encoder at 256 x 256 with L = 77 and 9 valid tokens is InstructRL's
334 rows: 266 visible keys, key block 4 partly hidden, block 5 wholly hidden (skipped).  Bars: tests/test_gc_encoder_gpu.py's (f32 2e-5, f16 8e-3,
bf16 6e-2, f16x3 1e-4); at ViT-B/16 its real-geometry bars (f32 1e-4, f16 1e-2, bf16 8e-2)."""
import ctypes as C

import numpy as np
import pytest

import instructrl_oracle as I

pytestmark = pytest.mark.gpu
VOCAB = 97
SMALL = dict(patch=16, width=128, layers=2, heads=2, img_res=64)
LONG = dict(patch=16, width=128, layers=2, heads=2, img_res=256)
TEXT = {"N30": (SMALL, 13, 5), "N334": (LONG, 77, 9)}   # geometry, L, valid tokens
TOL = {"f32": 2e-5, "f16": 8e-3, "bf16": 6e-2, "f16x3": 1e-4}
_cache = {}


def _weights(kw, seed=3):
    key = ("w", tuple(sorted(kw.items())), seed)
    if key not in _cache:
        from arp_amd import m3ae, synth_policy as S
        from oracle import m3ae_np as M
        cfg, ocfg = m3ae.EncoderConfig(**kw), M.EncConfig(**kw)
        _cache[key] = (cfg, ocfg, S.add_m3ae_text_params(S.m3ae_params(ocfg, seed=seed), ocfg, vocab=VOCAB, seed=seed))
    return _cache[key]


def _instruction(L, valid, seed):
    """ids in [0, VOCAB) and the reference's padding mask: 1 behind the `valid` leading tokens"""
    tok = np.random.default_rng(seed).integers(0, VOCAB, L).astype(np.int32)
    return tok, (np.arange(L) >= valid).astype(np.float32)


def _case(name, n, what="suffix", seed=3):
    """(cfg, params, frames, tokens, mask, float64 reference), computed once"""
    key = (name, n, what, seed)
    if key not in _cache:
        from arp_amd import synth_policy as S
        kw, L, valid = TEXT[name]
        cfg, ocfg, P = _weights(kw, seed)
        x = S.normalized_frames(n, cfg.img_res, seed=seed + 1)
        tok, mask = _instruction(L, valid, seed + 2)
        if what == "all padding":       # the reference's empty instruction: every text key hidden
            mask = np.ones(L, np.float32)
        elif what == "no padding":
            mask = np.zeros(L, np.float32)
        elif what == "scattered":
            mask = (np.random.default_rng(seed + 3).random(L) < 0.5).astype(np.float32)
        elif what == "per row":         # two different instructions, alternating over the frames
            tok2, mask2 = _instruction(L, valid + 3, seed + 4)
            tok = np.stack([tok if i % 2 == 0 else tok2 for i in range(n)])
            mask = np.stack([mask if i % 2 == 0 else mask2 for i in range(n)])
        ref = I.forward_representation(P, ocfg, x, tok, mask)
        ref.setflags(write=False)
        _cache[key] = (cfg, P, x, tok, mask, ref)
    return _cache[key]


def test_geometries_are_the_ones_described(gpu_lib):
    cfg, _, _ = _weights(LONG)
    assert cfg.text_tokens(77) == 334 and _weights(SMALL)[0].text_tokens(13) == 30
    _, mask = _instruction(77, 9, 0)
    visible = 257 + int((mask <= 0).sum())
    assert visible == 266 and 4 * 64 < visible < 5 * 64 < 334   # block 4 partly hidden, block 5 (keys 320 .. 333) wholly hidden


@pytest.mark.parametrize("mode", ["f32", "f16", "bf16", "f16x3"])
@pytest.mark.parametrize("name", ["N30", "N334"])
def test_text_encoder_parity(gpu_lib, name, mode):
    """5 frames with max_frames = 2: the call is chunked 2 + 2 + 1"""
    from arp_amd import m3ae
    cfg, P, x, tok, mask, ref = _case(name, 5)
    enc = m3ae.M3AEEncoder(cfg, P, mode=mode, max_frames=2)
    assert gpu_lib.lib.arp_enc_text_tokens(enc._h, len(tok)) == cfg.text_tokens(len(tok)) == ref.shape[1]
    got = enc.forward_representation(x, tok, mask)
    enc.close()
    err = np.abs(got - ref).max()
    print(f"text encoder {name} {mode}: max err {err:.2e}")
    assert got.shape == ref.shape and err < TOL[mode], f"text encoder {mode} {name}: max err {err}"


@pytest.mark.parametrize("what", ["all padding", "no padding", "scattered", "per row"])
@pytest.mark.parametrize("name", ["N30", "N334"])
def test_text_encoder_masks_and_instructions(gpu_lib, name, what):
    from arp_amd import m3ae
    cfg, P, x, tok, mask, ref = _case(name, 3, what)
    for mode in ("f32", "f16"):
        enc = m3ae.M3AEEncoder(cfg, P, mode=mode, max_frames=2)
        got = enc.forward_representation(x, tok, mask)
        if what == "no padding":
            assert (got.view(np.uint32) == enc.forward_representation(x, tok).view(np.uint32)).all(), "text_padding_mask=None is not 'nothing padded'"
        enc.close()
        err = np.abs(got - ref).max()
        print(f"text encoder {name} {what} {mode}: max err {err:.2e}")
        assert err < TOL[mode], f"{name} {what} {mode}: max err {err}"


def test_shared_instruction_is_the_per_row_call_with_equal_rows(gpu_lib):
    """per_row = 0 and per_row = 1 with the same instruction on every row: the same bits"""
    from arp_amd import m3ae
    cfg, P, x, tok, mask, _ = _case("N334", 5)
    for mode in ("f32", "f16"):
        enc = m3ae.M3AEEncoder(cfg, P, mode=mode, max_frames=2)
        a = enc.forward_representation(x, tok, mask)
        b = enc.forward_representation(x, np.tile(tok, (5, 1)), np.tile(mask, (5, 1)))
        enc.close()
        assert (a.view(np.uint32) == b.view(np.uint32)).all(), mode


@pytest.mark.parametrize("mode", ["f16", "bf16", "f32"])
def test_text_encoder_chunking_and_part_streams_are_exact(gpu_lib, mode):
    """334 rows, a per-row instruction: the same bits for max_frames 2 and 5, and for one stream against two part streams"""
    from arp_amd import m3ae
    cfg, P, x, tok, mask, _ = _case("N334", 5, "per row")
    outs = []
    for mf, streams in ((2, None), (5, None), (5, (1, 0, 0)), (5, (2, 0, 1))):
        enc = m3ae.M3AEEncoder(cfg, P, mode=mode, max_frames=mf)
        if streams:
            enc.set_streams(streams[0], first_part_frames=streams[1], min_part_frames=streams[2])
        outs.append(enc.forward_representation(x, tok, mask))
        enc.close()
    for k in (1, 2, 3):
        assert (outs[0].view(np.uint32) == outs[k].view(np.uint32)).all(), f"{mode}: configuration {k} differs from max_frames = 2"


def test_latency_path_takes_the_mask(gpu_lib):
    """one frame, 334 rows, with arp_enc_set_latency(host_calls = 1): the skinny GEMMs around the same masked attention, within the mode's bar"""
    from arp_amd import m3ae
    cfg, P, x, tok, mask, ref = _case("N334", 5)
    for mode in ("f16", "bf16"):
        enc = m3ae.M3AEEncoder(cfg, P, mode=mode)
        enc.set_latency_rows(514, host_calls=True)
        got = enc.forward_representation(x[:1], tok, mask)
        enc.close()
        err = np.abs(got - ref[:1]).max()
        print(f"text encoder latency path {mode}: max err {err:.2e}")
        assert err < TOL[mode], f"{mode}: max err {err}"


def test_text_encoder_refusals(gpu_lib):
    from arp_amd import m3ae
    cfg, P, x, tok, mask, _ = _case("N30", 5)
    enc = m3ae.M3AEEncoder(cfg, P, mode="f16c", max_frames=2)
    with pytest.raises(gpu_lib.ArpError, match="f16c: no image \\+ text pass"):
        enc.forward_representation(x, tok, mask)
    enc.close()
    for missing in ("text_embedding/embedding", "encoder_text_type_embedding"):
        enc = m3ae.M3AEEncoder(cfg, {k: v for k, v in P.items() if k != missing}, mode="f32", max_frames=2)
        with pytest.raises(gpu_lib.ArpError, match="text weights were not loaded"):
            enc.forward_representation(x, tok, mask)
        enc.close()
    enc = m3ae.M3AEEncoder(cfg, P, mode="f32", max_frames=2)
    for bad in (VOCAB, -1):
        t = tok.copy()
        t[-1] = bad    # a padded position: ids are checked whatever the mask says
        with pytest.raises(gpu_lib.ArpError, match="outside the vocabulary"):
            enc.forward_representation(x, t, mask)
    with pytest.raises(ValueError):
        enc.forward_representation(x, tok, mask[:-1])
    enc.close()


@pytest.mark.parametrize("mode", ["f16", "f32", "f16x3"])
def test_plain_and_gc_passes_after_a_text_call_are_unchanged(gpu_lib, mode):
    """a handle that carries the text weights and has served a text call returns, for the other two calls, the bits of a fresh handle without them"""
    from arp_amd import m3ae, synth_policy as S
    cfg, P, x, tok, mask, _ = _case("N30", 5)
    g = S.normalized_frames(5, cfg.img_res, seed=11)
    fresh = m3ae.M3AEEncoder(cfg, {k: v for k, v in P.items() if "text" not in k}, mode=mode, max_frames=2)
    want, want_gc = fresh.forward_representation(x), fresh.forward_gc_representations(x, g)
    fresh.close()
    enc = m3ae.M3AEEncoder(cfg, P, mode=mode, max_frames=2)
    enc.forward_representation(x, tok, mask)
    got, got_gc = enc.forward_representation(x), enc.forward_gc_representations(x, g)
    enc.close()
    assert (got.view(np.uint32) == want.view(np.uint32)).all() and (got_gc.view(np.uint32) == want_gc.view(np.uint32)).all()


def test_text_encoder_real_geometry(gpu_lib):
    """one frame, ViT-B/16 at 256 x 256 with L = 77: 334 rows"""
    from arp_amd import m3ae, synth_policy as S
    from oracle import m3ae_np as M
    kw = dict(patch=16, width=768, layers=12, heads=12, img_res=256)
    cfg, ocfg = m3ae.EncoderConfig(**kw), M.EncConfig(**kw)
    P = S.add_m3ae_text_params(S.m3ae_params(ocfg, seed=0), ocfg, vocab=VOCAB, seed=0)
    x = S.normalized_frames(1, 256, seed=1)
    tok, mask = _instruction(77, 9, 2)
    ref = I.forward_representation(P, ocfg, x, tok, mask)
    assert cfg.text_tokens(77) == 334 == ref.shape[1]
    for mode, tol in (("f32", 1e-4), ("f16", 1e-2), ("bf16", 8e-2)):
        enc = m3ae.M3AEEncoder(cfg, P, mode=mode)
        got = enc.forward_representation(x, tok, mask)
        enc.close()
        err = np.abs(got - ref).max()
        print(f"text encoder ViT-B/16 334 rows {mode}: max err {err:.2e}")
        assert err < tol, f"{mode}: max err {err}"


def test_text_encoder_releases_what_it_took(gpu_lib):
    """after text calls (shared and per row, two part streams) and a destroy the live-resource counters are where they were"""
    import gc
    from arp_amd import m3ae

    def live():
        out = (C.c_int64 * 5)()
        gpu_lib.check(gpu_lib.lib.arp_debug_live(out))
        return list(out)
    gc.collect()
    cfg, P, x, tok, mask, _ = _case("N30", 5)
    before = live()
    enc = m3ae.M3AEEncoder(cfg, P, mode="f16", max_frames=2)
    enc.set_streams(2, min_part_frames=1)
    enc.forward_representation(x, tok, mask)
    enc.forward_representation(x, np.tile(tok, (5, 1)), np.tile(mask, (5, 1)))
    enc.close()
    assert live() == before
