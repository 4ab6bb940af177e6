"""GPU tests of the M3AE encoder's latency path for (frame, goal) pairs (arp_amd/csrc/arp_enc.hip: a goal-conditioned call of at most arp_enc::lat_rows token
rows IN TOTAL, pairs x (2 P + 1), on tower.h's skinny GEMMs with split-K out_proj / c_proj).  tests/test_encoder_latency_gpu.py for pairs: parity with fp64
(tests/gcbc_oracle.py) at the bar tests/test_gc_encoder_gpu.py holds the throughput path to, the row limit's cut, and that no existing caller changes a bit.

Geometries: 33-token pairs (LDS-resident attention; 1, 2 and 3 pairs), 339-token pairs (key-blocked attention, M = 339 is no multiple of 16) and one
513-row pair (img_res 256, one block: one row below the default limit of 514, the real geometry's row count)."""
import numpy as np
import pytest

import gcbc_oracle as G

pytestmark = pytest.mark.gpu

SMALL_ENC = dict(patch=16, width=128, layers=2, heads=2, img_res=64)
LONG_ENC = dict(patch=16, width=128, layers=2, heads=2, img_res=208)
ROWS513_ENC = dict(patch=16, width=128, layers=1, heads=2, img_res=256)
TOL = {"f16": 8e-3, "bf16": 6e-2}  # tests/test_gc_encoder_gpu.py::test_gc_encoder_parity

_REF = {}


def _case(kw, n):
    """(weights, frames, goals, fp64 tokens of n pairs), computed once per geometry"""
    key = (kw["img_res"], kw["layers"])
    if key not in _REF:
        from arp_amd import synth_policy as S
        from oracle import m3ae_np as M
        ocfg = M.EncConfig(**kw)
        P = S.m3ae_params(ocfg, seed=3)
        x, g = S.normalized_frames(n, kw["img_res"], seed=4), S.normalized_frames(n, kw["img_res"], seed=5)
        ref = G.forward_gc_representations(P, ocfg, x, g)
        ref.setflags(write=False)
        _REF[key] = (P, x, g, ref)
    return _REF[key]


def _reduce_launches(enc, x, g):
    """launches of the latency path's slab-reduce + LayerNorm kernel (site m3ae.out_reduce_ln_2) in one profiled call"""
    enc.profile(True)
    before = enc.profile_read().get("m3ae.out_reduce_ln_2", {"calls": 0})["calls"]
    enc.forward_gc_representations(x, g)
    after = enc.profile_read().get("m3ae.out_reduce_ln_2", {"calls": 0})["calls"]
    enc.profile(False)
    return after - before


@pytest.mark.parametrize("kw,pairs", [(SMALL_ENC, 3), (LONG_ENC, 1), (ROWS513_ENC, 1)], ids=["N33", "N339", "N513"])
@pytest.mark.parametrize("mode", ["f16", "bf16"])
def test_gc_latency_path_parity_and_the_cut(gpu_lib, kw, pairs, mode):
    from arp_amd import m3ae
    P, x, g, ref = _case(kw, pairs)
    cfg = m3ae.EncoderConfig(**kw)
    enc = m3ae.M3AEEncoder(cfg, P, mode=mode)
    try:
        for n in range(1, pairs + 1):
            rows = n * cfg.gc_tokens
            assert rows <= 1024
            enc.set_latency_rows(0, host_calls=True)          # the path forced off: the control
            off = enc.forward_gc_representations(x[:n], g[:n])
            enc.set_latency_rows(1024, host_calls=True)
            lat = enc.forward_gc_representations(x[:n], g[:n])
            e_off, e_lat = np.abs(off - ref[:n]).max(), np.abs(lat - ref[:n]).max()
            print(f"m3ae gc {cfg.gc_tokens} tokens {mode} n {n}: latency path {e_lat:.2e}, throughput path {e_off:.2e}")
            assert e_lat < TOL[mode] and e_off < TOL[mode]
            assert _reduce_launches(enc, x[:n], g[:n]) == kw["layers"]  # the path did run: one slab reduction behind every out_proj
            enc.set_latency_rows(rows - 1, host_calls=True)   # a limit just below the call's rows: the throughput path
            assert np.array_equal(enc.forward_gc_representations(x[:n], g[:n]), off) and _reduce_launches(enc, x[:n], g[:n]) == 0
            enc.set_latency_rows(rows, host_calls=True)       # ... and exactly at them: the latency path
            assert np.array_equal(enc.forward_gc_representations(x[:n], g[:n]), lat)
            enc.set_latency_rows(1024, host_calls=False)      # host calls do not ask for the path: as ever
            assert np.array_equal(enc.forward_gc_representations(x[:n], g[:n]), off)
    finally:
        enc.close()


def test_two_long_pairs_are_over_the_default_limit(gpu_lib):
    """339-token pairs with the knob at its default (514) and host calls asking for the path: one pair runs on it, two pairs (678 rows) do not"""
    from arp_amd import m3ae
    P, x, g, _ = _case(LONG_ENC, 1)
    x2, g2 = np.concatenate([x, g]), np.concatenate([g, x])
    enc = m3ae.M3AEEncoder(m3ae.EncoderConfig(**LONG_ENC), P, mode="f16")
    try:
        enc.set_latency_rows(514, host_calls=True)
        assert _reduce_launches(enc, x, g) == LONG_ENC["layers"] and _reduce_launches(enc, x2, g2) == 0
    finally:
        enc.close()


@pytest.mark.parametrize("mode", ["f16", "bf16"])
def test_existing_gc_callers_are_untouched(gpu_lib, mode):
    """forward_gc_representations on 3 pairs and one GCBC train_step with frames and goals in (B = 1: 99 rows, under any limit): bitwise equal with the knob at
    its default and with the latency path disabled."""
    from arp_amd import m3ae, synth_policy as S
    from arp_amd.train import PolicyConfig, PolicyTrainer
    P, x, g, _ = _case(SMALL_ENC, 3)
    ecfg = m3ae.EncoderConfig(**SMALL_ENC)
    pcfg = PolicyConfig(emb=64, depth=2, heads=4, window=3, enc_tokens=ecfg.gc_tokens, enc_dim=ecfg.width, model="GCBC")
    PP = S.policy_params(pcfg, seed=6)
    r = ecfg.img_res
    frames = S.normalized_frames(pcfg.window, r, seed=8).reshape(1, pcfg.window, r, r, 3)
    goals = S.normalized_frames(pcfg.window, r, seed=9).reshape(1, pcfg.window, r, r, 3)
    act = np.random.default_rng(7).integers(0, pcfg.n_actions, (1, pcfg.window)).astype(np.int32)
    got = {}
    for name in ("default", "disabled"):
        enc = m3ae.M3AEEncoder(ecfg, P, mode=mode)
        if name == "disabled":
            enc.set_latency_rows(0)
        tr = PolicyTrainer(pcfg, mode="f16")
        tr.set_params(PP)
        tr.attach_encoder(enc)
        codes = enc.forward_gc_representations(x, g)
        one = enc.forward_gc_representations(x[:1], g[:1])
        tr.set_batch_images(frames, act, goals=goals)
        aux = tr.train_step(1e-3)
        got[name] = (codes, one, aux["loss"], aux["grad_norm"], tr.get_params())
        tr.close(); enc.close()
    a, b = got["default"], got["disabled"]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]
    assert all(np.array_equal(a[4][k], b[4][k]) for k in a[4])
