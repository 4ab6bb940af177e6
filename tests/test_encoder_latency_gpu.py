"""GPU tests of the M3AE encoder's latency path (arp_amd/csrc/arp_enc.hip: a call of at most arp_enc::lat_rows token rows on tower.h's skinny GEMMs with
split-K out_proj / c_proj): parity with fp64 at the bar the throughput path is held to, the row limit's cut, and that no existing caller changes a bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TINY_ENC = dict(patch=16, width=64, layers=2, heads=2, img_res=64)      # 17 tokens, head_dim 32 (VALU attention)
SMALL_ENC = dict(patch=16, width=128, layers=2, heads=2, img_res=64)    # head_dim 64 (MFMA attention)
TOL = {"f16": 8e-3, "bf16": 6e-2}  # tests/test_m3ae_gpu.py::test_encoder_parity

_REF = {}


def _case(kw):
    """(weights, frames, fp64 tokens of 3 frames), computed once per geometry"""
    key = kw["width"]
    if key not in _REF:
        from arp_amd import synth_policy as S
        from oracle import m3ae_np as M
        ocfg = M.EncConfig(**kw)
        P = S.m3ae_params(ocfg, seed=3)
        x = S.normalized_frames(3, kw["img_res"], seed=4)
        _REF[key] = (P, x, M.forward_representation(P, ocfg, x))
    return _REF[key]


def _reduce_launches(enc, x):
    """launches of the latency path's slab-reduce + LayerNorm kernel (site m3ae.out_reduce_ln_2) in one profiled call"""
    enc.profile(True)
    before = enc.profile_read().get("m3ae.out_reduce_ln_2", {"calls": 0})["calls"]
    enc.forward_representation(x)
    after = enc.profile_read().get("m3ae.out_reduce_ln_2", {"calls": 0})["calls"]
    enc.profile(False)
    return after - before


@pytest.mark.parametrize("kw", [TINY_ENC, SMALL_ENC])
@pytest.mark.parametrize("mode", ["f16", "bf16"])
def test_latency_path_parity_and_the_cut(gpu_lib, kw, mode):
    from arp_amd import m3ae
    P, x, ref = _case(kw)
    cfg = m3ae.EncoderConfig(**kw)
    enc = m3ae.M3AEEncoder(cfg, P, mode=mode)
    try:
        for n in (1, 2, 3):
            enc.set_latency_rows(0, host_calls=True)          # the path forced off: the control
            off = enc.forward_representation(x[:n])
            enc.set_latency_rows(1024, host_calls=True)
            lat = enc.forward_representation(x[:n])
            e_off, e_lat = np.abs(off - ref[:n]).max(), np.abs(lat - ref[:n]).max()
            print(f"m3ae {kw['width']} {mode} n {n}: latency path {e_lat:.2e}, throughput path {e_off:.2e}")
            assert e_lat < TOL[mode] and e_off < TOL[mode]
            assert _reduce_launches(enc, x[:n]) == kw["layers"]  # the path did run: one slab reduction behind every out_proj
            enc.set_latency_rows(n * cfg.tokens - 1, host_calls=True)   # a limit just below the call's rows: the throughput path
            assert np.array_equal(enc.forward_representation(x[:n]), off) and _reduce_launches(enc, x[:n]) == 0
            enc.set_latency_rows(n * cfg.tokens, host_calls=True)       # ... and exactly at them: the latency path
            assert np.array_equal(enc.forward_representation(x[:n]), lat)
            enc.set_latency_rows(1024, host_calls=False)       # host calls do not ask for the path: as ever
            assert np.array_equal(enc.forward_representation(x[:n]), off)
    finally:
        enc.close()


@pytest.mark.parametrize("mode", ["f16", "bf16"])
def test_existing_callers_are_untouched(gpu_lib, mode):
    """forward_representation on 8 frames and one encoder-inside train_step at TINY_ENC: bitwise equal with the knob at its default and with the latency path
    disabled."""
    from arp_amd import m3ae, synth_policy as S
    from arp_amd.train import PolicyConfig, PolicyTrainer
    P, _, _ = _case(TINY_ENC)
    ecfg = m3ae.EncoderConfig(**TINY_ENC)
    pcfg = PolicyConfig(emb=64, depth=2, heads=4, window=3, enc_tokens=ecfg.tokens, enc_dim=ecfg.width, lambda_ret=0.5)
    PP = S.policy_params(pcfg, seed=6)
    x8 = S.normalized_frames(8, ecfg.img_res, seed=9)
    rng = np.random.default_rng(7)
    frames = S.normalized_frames(pcfg.window, ecfg.img_res, seed=8).reshape(1, pcfg.window, ecfg.img_res, ecfg.img_res, 3)  # B = 1: 51 rows, under any limit
    act, rtg = rng.integers(0, pcfg.n_actions, (1, pcfg.window)).astype(np.int32), rng.random((1, pcfg.window, 1)).astype(np.float32)
    got = {}
    for name in ("default", "disabled"):
        enc = m3ae.M3AEEncoder(ecfg, P, mode=mode)
        if name == "disabled":
            enc.set_latency_rows(0)
        tr = PolicyTrainer(pcfg, mode="f16")
        tr.set_params(PP)
        tr.attach_encoder(enc)
        codes = enc.forward_representation(x8)
        one = enc.forward_representation(x8[:1])
        tr.set_batch_images(frames, act, rtg)
        aux = tr.train_step(1e-3)
        got[name] = (codes, one, aux["loss"], aux["grad_norm"], tr.get_params())
        tr.close(); enc.close()
    a, b = got["default"], got["disabled"]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]
    assert all(np.array_equal(a[4][k], b[4][k]) for k in a[4])
