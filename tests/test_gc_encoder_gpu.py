"""The goal-conditioned pass of the frozen M3AE encoder (arp_enc_forward_gc, M3AEEncoder.forward_gc_representations) against tests/gcbc_oracle.py in
float64, on seeded weights (synth_policy.m3ae_params).

Small geometry (patch 16, width 128, 2 layers, 2 heads, 64 x 64 frames: P = 16, 33 tokens) runs on the LDS-resident attention kernels and isolates
patch order, assembly and row bookkeeping; the same encoder at 208 x 208 (P = 169, 339 tokens) runs on the key-blocked kernels of csrc/attention_long.h.
Bars: tests/test_m3ae_gpu.py::test_encoder_parity's (f32 2e-5, f16 8e-3, bf16 6e-2), f16x3 1e-4; at ViT-B/16 and 256 x 256 (513 tokens)
test_full_size_encoder_parity's (f32 1e-4, f16 1e-2, bf16 8e-2)."""
import numpy as np
import pytest

import gcbc_oracle as G

pytestmark = pytest.mark.gpu
SMALL = dict(patch=16, width=128, layers=2, heads=2, img_res=64)
LONG = dict(patch=16, width=128, layers=2, heads=2, img_res=208)
TOL = {"f32": 2e-5, "f16": 8e-3, "bf16": 6e-2, "f16x3": 1e-4}
_cache = {}


def _case(kw, n, seed=3):
    """(cfg, ocfg, params, frames, goals, float64 reference), computed once per geometry"""
    key = (tuple(sorted(kw.items())), n, seed)
    if key not in _cache:
        from arp_amd import m3ae, synth_policy as S
        from oracle import m3ae_np as M
        cfg, ocfg = m3ae.EncoderConfig(**kw), M.EncConfig(**kw)
        P = S.m3ae_params(ocfg, seed=seed)
        x, g = S.normalized_frames(n, cfg.img_res, seed=seed + 1), S.normalized_frames(n, cfg.img_res, seed=seed + 2)
        ref = G.forward_gc_representations(P, ocfg, x, g)
        ref.setflags(write=False)
        _cache[key] = (cfg, ocfg, P, x, g, ref)
    return _cache[key]


@pytest.mark.parametrize("mode", ["f32", "f16", "bf16", "f16x3"])
@pytest.mark.parametrize("kw", [SMALL, LONG], ids=["N33", "N339"])
def test_gc_encoder_parity(gpu_lib, kw, mode):
    """5 pairs with max_frames = 2: the call is chunked 2 + 2 + 1"""
    from arp_amd import m3ae
    cfg, _, P, x, g, ref = _case(kw, 5)
    assert cfg.gc_tokens == 2 * (kw["img_res"] // 16) ** 2 + 1 == ref.shape[1]
    enc = m3ae.M3AEEncoder(cfg, P, mode=mode, max_frames=2)
    assert gpu_lib.lib.arp_enc_gc_tokens(enc._h) == cfg.gc_tokens
    got = enc.forward_gc_representations(x, g)
    enc.close()
    err = np.abs(got - ref).max()
    print(f"gc encoder N={cfg.gc_tokens} {mode}: max err {err:.2e}")
    assert got.shape == ref.shape and err < TOL[mode], f"gc encoder {mode} at {cfg.gc_tokens} tokens: max err {err}"


@pytest.mark.parametrize("kw", [SMALL, LONG], ids=["N33", "N339"])
def test_gc_encoder_f16c_is_refused(gpu_lib, kw):
    from arp_amd import m3ae
    cfg, _, P, x, g, _ = _case(kw, 5)
    enc = m3ae.M3AEEncoder(cfg, P, mode="f16c", max_frames=2)
    with pytest.raises(gpu_lib.ArpError, match="f16c: no goal-conditioned pass"):
        enc.forward_gc_representations(x, g)
    enc.close()


@pytest.mark.parametrize("mode", ["f16", "bf16", "f32"])
def test_gc_encoder_chunking_and_part_streams_are_exact(gpu_lib, mode):
    """339 tokens: the same bits for max_frames 2 and 5, and for one stream against two part streams"""
    from arp_amd import m3ae
    cfg, _, P, x, g, _ = _case(LONG, 5)
    outs = []
    for mf, streams in ((2, None), (5, None), (5, (1, 0, 0)), (5, (2, 0, 1))):
        enc = m3ae.M3AEEncoder(cfg, P, mode=mode, max_frames=mf)
        if streams:
            enc.set_streams(streams[0], first_part_frames=streams[1], min_part_frames=streams[2])
        outs.append(enc.forward_gc_representations(x, g))
        enc.close()
    for k in (1, 2, 3):
        assert (outs[0].view(np.uint32) == outs[k].view(np.uint32)).all(), f"{mode}: configuration {k} differs from max_frames = 2"


def test_gc_encoder_real_geometry(gpu_lib):
    """one pair, ViT-B/16 at 256 x 256: 513 tokens"""
    from arp_amd import m3ae
    cfg, _, P, x, g, ref = _case(dict(patch=16, width=768, layers=12, heads=12, img_res=256), 1, seed=0)
    assert cfg.gc_tokens == 513
    for mode, tol in (("f32", 1e-4), ("f16", 1e-2), ("bf16", 8e-2)):
        enc = m3ae.M3AEEncoder(cfg, P, mode=mode)
        got = enc.forward_gc_representations(x, g)
        enc.close()
        err = np.abs(got - ref).max()
        print(f"gc encoder ViT-B/16 513 tokens {mode}: max err {err:.2e}")
        assert err < tol, f"{mode}: max err {err}"


@pytest.mark.parametrize("mode", ["f16", "f32", "f16x3"])
def test_plain_pass_after_a_gc_call_is_unchanged(gpu_lib, mode):
    """forward_representation on a handle that has served a gc call returns the bits a fresh handle returns"""
    from arp_amd import m3ae
    cfg, _, P, x, g, _ = _case(LONG, 5)
    fresh = m3ae.M3AEEncoder(cfg, P, mode=mode, max_frames=2)
    want = fresh.forward_representation(x)
    fresh.close()
    enc = m3ae.M3AEEncoder(cfg, P, mode=mode, max_frames=2)
    enc.forward_gc_representations(x, g)
    got = enc.forward_representation(x)
    enc.close()
    assert (got.view(np.uint32) == want.view(np.uint32)).all()


def test_gc_encoder_releases_what_it_took(gpu_lib):
    """after a gc call and a destroy the live-resource counters are where they were"""
    import ctypes as C
    import gc
    from arp_amd import m3ae

    def live():
        out = (C.c_int64 * 5)()
        gpu_lib.check(gpu_lib.lib.arp_debug_live(out))
        return list(out)
    gc.collect()
    cfg, _, P, x, g, _ = _case(SMALL, 5)
    before = live()
    enc = m3ae.M3AEEncoder(cfg, P, mode="f16", max_frames=2)
    enc.set_streams(2, min_part_frames=1)
    enc.forward_gc_representations(x, g)
    enc.close()
    assert live() == before
