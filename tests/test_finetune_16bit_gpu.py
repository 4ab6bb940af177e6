"""GPU: the fine-tune head's 16-bit step (arp_amd/csrc/arp_ft.hip in its f16 and bf16 modes) against fp64, tensor by tensor.

Two yardsticks per gradient tensor: the rounded-operand emulation (oracle/finetune_torch.py, `Rounding`: float64 with every operand rounded
where the kernels round it, the backward seeded x grad_scale) at tight bars, and the plain fp64 oracle at looser ones (the emulation and the
kernels must not share a mistake).  Then AdamW from a mid-training state (nonzero moments, step 10, weight decay) on the fused and the
unfused path against oracle.adamw_step, and the f16 mode's dropped-gradient counter on a backward that overflows binary16.

Per tensor the bars are a relative L2 error and the max error over all but 0.1 % of the entries (relative to the tensor's largest entry): a
ReLU pre-activation or a 16-bit rounding tie near a boundary moves a few entries by one term or one ulp; an indexing or reduction bug moves
the whole tensor.  The bars were set from MI355X measurements (commit message) with the margins stated next to them."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MID = dict(layers=3, width_v=128, width_t=64, embed=64, hidden=64, n_actions=15)
MODES = ("f16", "bf16")
# (relative L2, max over 99.9 % of entries) per gradient tensor and geometry, measured worst in the commit message.  Emulation, MID: f16
# 2.6e-4 / 4.0e-4, bf16 7e-5 / 9e-5; real geometry (ReLU ties of the adapters' 192 x 13312 H, the scalar residual-weight sums): f16 3.5e-3 /
# 2.5e-3, bf16 4.1e-3 / 4.1e-3 -> bars 2-4x above.  Plain fp64 (the operand rounding itself; bf16 text W1 0.10 / 0.19, cos 0.9947) -> 2-3x.
BAR_EMU = {("f16", "mid"): (1e-3, 1e-3), ("bf16", "mid"): (2e-4, 2e-4), ("f16", "full"): (1e-2, 5e-3), ("bf16", "full"): (1.2e-2, 1.2e-2)}
BAR_FP64 = {"f16": (0.1, 0.2), "bf16": (0.3, 0.6)}
COS_FP64 = {"f16": 0.999, "bf16": 0.99}
BAR_FWD = {"f16": 5e-5, "bf16": 1e-4}  # losses, scores (cosine units), logits: measured 5.3e-6 / 2.4e-5


def _cfgs(geom, **kw):
    from arp_amd import finetune as FT
    from oracle import finetune_torch as O
    fcfg = FT.FinetuneConfig(**(MID if geom == "mid" else {}), **kw)
    names = {f.name for f in dataclasses.fields(O.HeadConfig)}
    return fcfg, O.HeadConfig(**{k: v for k, v in dataclasses.asdict(fcfg).items() if k in names})


def _params(fcfg, seed):
    from arp_amd import finetune as FT
    P = FT.synth_params(fcfg, seed=seed)
    P["image_residual_weight"] = np.float32(0.4) * np.ones((), np.float32)  # both paths of the mix carry weight (the init's 4.0 gives 0.98 / 0.02)
    P["text_residual_weight"] = np.float32(-0.6) * np.ones((), np.float32)
    return P


def _batch(fcfg, B, seed):
    from arp_amd import finetune as FT
    b = FT.synth_batch(fcfg, B, seed=seed)
    if not fcfg.goal_conditioned:
        return b
    rng = np.random.Generator(np.random.PCG64(seed + 1000))  # image3, the goal frame, stands where the prompt stands
    return (np.concatenate([b[0], rng.standard_normal((1, B, fcfg.d_img), dtype=np.float32)]),
            np.concatenate([b[1], rng.standard_normal((1, B, fcfg.embed), dtype=np.float32)]), None, None, b[4], b[5])


def _get(tr, name, which):
    """one tensor (0 params, 1 grads, 2 / 3 AdamW moments): the full-size dicts would be another 1.9 GB of host memory each"""
    from arp_amd import _ffi
    a = np.empty(tr.shapes[name], np.float32)
    _ffi.check(_ffi.lib.arp_ft_get_tensor(tr._h, name.encode(), which, _ffi.as_ptr(a, C.c_float)))
    return a


def _errs(got, ref):
    """relative L2, max |error| over all but 0.1 % of the entries / max |ref|, cosine"""
    got, ref = np.asarray(got, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    d = np.abs(got - ref)
    k = int(0.999 * (d.size - 1))
    q = float(np.partition(d, k)[k]) / max(float(np.abs(ref).max()), 1e-30)
    nr, ng = float(np.linalg.norm(ref)), float(np.linalg.norm(got))
    return float(np.linalg.norm(d)) / max(nr, 1e-30), q, float(got @ ref) / max(nr * ng, 1e-30)


CASES = {  # geometry, B, config switches, environment
    "mid_b7": ("mid", 7, {}, {}),
    "mid_b5_no_vip": ("mid", 5, dict(use_vip=False), {}),
    "mid_b5_no_id": ("mid", 5, dict(use_id=False), {}),
    "mid_goal_b5": ("mid", 5, dict(goal_conditioned=True), {}),
    "mid_b7_nt": ("mid", 7, {}, {"ARP_FT_NN": "0"}),
    "full_b64": ("full", 64, {}, {}),      # the timed size: 192 image rows (m_fast), its split-K counts
    "full_b4": ("full", 4, {}, {}),        # 12 image rows: the other split-K routing of ft_gemm
    "full_b4_nt": ("full", 4, {}, {"ARP_FT_NN": "0"}),
}


@pytest.mark.parametrize("mode,case", [(m, c) for m in MODES for c in CASES if not (m == "bf16" and c == "full_b4_nt")])  # (suite time)
def test_16bit_head_matches_the_emulation_and_fp64(gpu_lib, monkeypatch, mode, case):
    """Loss, vip_loss, id_loss, scores and logits (arp_ft_forward), then every gradient tensor (arp_ft_backward) against the rounded-operand
    emulation and against plain fp64; on the cases without a switch also arp_ft_encode (the clip_ft labelling / online-reward path) on a
    ragged row count against the emulation's adapted features."""
    import torch
    from arp_amd import finetune as FT
    from oracle import finetune_torch as O
    geom, B, kw, env = CASES[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    fcfg, cfg = _cfgs(geom, **kw)
    P = _params(fcfg, seed=31)
    if geom == "full":
        # Hinv's pre-activations away from 0: at B x 1024 of them a few otherwise sit within f32-vs-f64 noise of the ReLU, and one flipped mask
        # entry moves that sample's whole dC row and every gradient behind it by ~1e-2 (measured).  MID keeps the random c1: the mask runs there.
        P["inverse_layer.layers.0.bias"] = P["inverse_layer.layers.0.bias"] + np.float32(0.5)
    batch = _batch(fcfg, B, seed=32)
    g_emu, aux_emu = O.grads(P, cfg, batch, operand=mode)
    tr = FT.FinetuneTrainer(fcfg, mode=mode)
    try:
        tr.set_params(P)
        tr.set_batch(*batch)
        out = tr.forward()
        bad = []
        # scores in cosine units (exp(logit_scale) <a, t>; goal_conditioned: distances of unit vectors), losses and logits relative to max(1, |ref|)
        unit = {"scores": 1.0 if fcfg.goal_conditioned else float(np.exp(fcfg.logit_scale))}
        for k in ("loss", "vip_loss", "id_loss", "scores", "logits"):
            e = float(np.abs(out[k] - aux_emu[k]).max() / unit.get(k, max(1.0, float(np.abs(aux_emu[k]).max()))))
            print(f"  {k}: max err vs emulation {e:.2e}")
            if not e < BAR_FWD[mode]:
                bad.append(("forward", k, e))
        tr.backward()
        for k in P:
            a = _get(tr, k, 1)
            r = g_emu[k]
            if not np.any(r):  # no gradient in this configuration (use_id off, goal_conditioned's text head): exactly zero
                assert not np.any(a), k
                continue
            l2, q, _ = _errs(a, r)
            if not (l2 < BAR_EMU[mode, geom][0] and q < BAR_EMU[mode, geom][1]):
                bad.append(("emulation", k, l2, q))
            print(f"  {k}: vs emulation rel L2 {l2:.2e}, q999 {q:.2e}")
        del g_emu
        g_ref, _ = O.grads(P, cfg, batch)
        for k in P:
            r = g_ref[k]
            if not np.any(r):
                continue
            l2, q, cos = _errs(_get(tr, k, 1), r)
            print(f"  {k}: vs fp64 rel L2 {l2:.2e}, q999 {q:.2e}, cos {cos:.7f}")
            if not (l2 < BAR_FP64[mode][0] and q < BAR_FP64[mode][1] and cos > COS_FP64[mode]):
                bad.append(("fp64", k, l2, q, cos))
        del g_ref
        assert not bad, bad
        if env or kw:
            return
        Pt = O.to_torch({k: v for k, v in P.items() if not k.startswith("inverse_layer")})
        for which, name in ((0, "image"), (1, "text")):
            inter = batch[0].reshape(-1, fcfg.d_img)[:5] if which == 0 else batch[2]
            final = batch[1].reshape(-1, fcfg.embed)[:5] if which == 0 else batch[3]
            got = tr.encode_image(inter, final) if which == 0 else tr.encode_text(inter, final)
            with torch.no_grad():
                args = (torch.as_tensor(inter, dtype=torch.float64), torch.as_tensor(final, dtype=torch.float64))
                emu = O._encode(Pt, name, *args, rq=O.Rounding(mode)).numpy()
                ref = O._encode(Pt, name, *args).numpy()
            e_emu, e_ref = float(np.abs(got - emu).max()), float(np.abs(got - ref).max())
            print(f"  encode {name} ({inter.shape[0]} rows): max err vs emulation {e_emu:.2e}, vs fp64 {e_ref:.2e}")
            # unit-norm rows: an absolute error; the bf16 fp64 bar is the operand rounding itself
            assert e_emu < 1e-4 and e_ref < (5e-4 if mode == "f16" else 3e-3), (name, e_emu, e_ref)  # measured 2.8e-5; 2.1e-4 / 8.9e-4
    finally:
        tr.close()


def _moments(G, seed):
    """a mid-training AdamW state built around this step's gradient: m ~ half the gradient plus noise of its RMS, v ~ (g^2 + RMS^2) x U(0.5, 2)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    M, V = {}, {}
    for k, g in G.items():
        g = np.where(np.isfinite(g), g, 0.0).astype(np.float32)
        s = np.float32(max(float(np.sqrt(np.mean(np.square(g, dtype=np.float64)))), 1e-6))
        M[k] = (0.5 * g + 0.5 * s * rng.standard_normal(g.shape, dtype=np.float32)).astype(np.float32)
        V[k] = ((g * g + s * s) * rng.uniform(0.5, 2.0, g.shape).astype(np.float32)).astype(np.float32)
    return M, V


def _rows(a):
    """at the real geometry the fp64 AdamW restatement runs on every 7th row (7 is prime to the GEMM tiles: every row residue of a tile is
    visited) plus the last one of each big weight; every tensor below 4 M entries is compared whole"""
    if a.size < (4 << 20):
        return a
    return np.concatenate([a[::7], a[-1:]])


def _check_adamw(tr, P, M, V, G, step, lr, wd, tag):
    """every tensor's parameter, m and v after one train_step against oracle.adamw_step from (P, M, V, G).  With moments present a wrong
    gradient scale, bias correction, eps or decay placement moves the update by O(lr); the bars are 1e-4 lr on p (plus 2 f32 ulp of |p|) and
    2e-6 of the tensor's largest m / v (the fused GEMM's gradient differs from the stored one by f32 round-off, ~1e-5 relative, and enters m
    with weight 0.1).  Measured worst: p 0.29 of its bar, m / v 1.5e-7."""
    from oracle import finetune_torch as O
    bad, worst = [], [0.0, 0.0, 0.0]
    for k in P:
        sl = {n: _rows(np.asarray(x[k]).reshape(tr.shapes[k])) for n, x in (("p", P), ("m", M), ("v", V), ("g", G))}
        p1, m1, v1 = (d[k] for d in O.adamw_step({k: sl["p"]}, {k: sl["m"]}, {k: sl["v"]}, {k: sl["g"].astype(np.float64)}, step, lr, wd))
        gp, gm, gv = (_rows(_get(tr, k, w)) for w in (0, 2, 3))
        assert np.isfinite(gp).all() and np.isfinite(gm).all() and np.isfinite(gv).all(), (tag, k)
        ep = float((np.abs(gp - p1) / (1e-4 * lr + 2.4e-7 * np.abs(p1))).max())
        em = float(np.abs(gm - m1).max() / max(np.abs(m1).max(), 1e-30))
        ev = float(np.abs(gv - v1).max() / max(np.abs(v1).max(), 1e-30))
        worst = [max(worst[0], ep), max(worst[1], em), max(worst[2], ev)]
        if not (ep < 1.0 and em < 2e-6 and ev < 2e-6):
            bad.append((k, ep, em, ev))
    print(f"  {tag}: worst p err / bar {worst[0]:.2e}, m {worst[1]:.2e}, v {worst[2]:.2e}")
    assert not bad, (tag, bad)


@pytest.mark.parametrize("geom,fuse", [("mid", "1"), ("full", "1"), ("full", "0")])
@pytest.mark.parametrize("mode", MODES)
def test_adamw_from_a_mid_training_state(gpu_lib, monkeypatch, mode, geom, fuse):
    """One train_step from parameters, nonzero moments, step 10 and weight decay 0.05, against oracle.adamw_step on the gradient arp_ft_backward
    stores for the same state and batch: the seven big weights (inside their weight-gradient GEMMs where ARP_FT_FUSE_ADAM is on at the real
    geometry, in ft_adamw_kernel otherwise), the biases and the three scalars.  MID's weights are too small for the fused epilogue: one path."""
    from arp_amd import _ffi, finetune as FT
    monkeypatch.setenv("ARP_FT_FUSE_ADAM", fuse)
    fcfg, _ = _cfgs(geom, weight_decay=0.05)
    P = _params(fcfg, seed=41)
    tr = FT.FinetuneTrainer(fcfg, mode=mode)
    try:
        tr.set_params(P)
        tr.set_batch(*_batch(fcfg, 64 if geom == "full" else 7, seed=42))
        tr.backward()
        G = {k: _get(tr, k, 1) for k in P}
        M, V = _moments(G, seed=43)
        tr.set_tensors(M, 2)
        tr.set_tensors(V, 3)
        tr.step = 10
        lr = 1e-3
        tr.train_step(lr)
        assert tr.step == 11 and tr.dropped_gradients == 0
        probe = np.empty(tr.shapes["image_intermediate_linear.weight"], np.float32)
        rc = _ffi.lib.arp_ft_get_tensor(tr._h, b"image_intermediate_linear.weight", 1, _ffi.as_ptr(probe, C.c_float))
        assert (rc != 0) == (geom == "full" and fuse == "1")  # the path under test is the one that ran: fused gradients are never stored
        _check_adamw(tr, P, M, V, G, 10, lr, 0.05, f"{mode} {geom} fuse={fuse}")
    finally:
        tr.close()


@pytest.mark.parametrize("geom,fuse", [("mid", "0"), ("full", "1"), ("full", "0")])
def test_f16_dropped_gradients_are_counted_and_treated_as_zero(gpu_lib, monkeypatch, geom, fuse):
    """A step whose gradients are non-finite on purpose.  The backward's own 16-bit copies cannot overflow to inf: transpose_mask_kernel
    saturates them at +-65504 in f16 (dHinv, dA, the masked dH, dU).  What reaches AdamW as inf / NaN is a forward past binary16's range:
    here the image adapter's first bias entry is 1e5, so fc1's stored H (a GEMM epilogue) holds inf -- an ordinary numeric overflow in a
    tensor -- the adapted features, the loss and every gradient turn NaN.  The step must count exactly the non-finite entries arp_ft_backward
    stores for the same state, keep parameters and moments finite, and equal oracle.adamw_step with those entries' gradients set to 0 -- in
    ft_adamw_kernel and in the fused GEMM epilogue."""
    from arp_amd import finetune as FT
    monkeypatch.setenv("ARP_FT_FUSE_ADAM", fuse)
    fcfg, _ = _cfgs(geom, weight_decay=0.05)
    P = _params(fcfg, seed=51)
    P["image_adapter.layers.0.bias"] = P["image_adapter.layers.0.bias"].copy()
    P["image_adapter.layers.0.bias"][0] = 1e5
    tr = FT.FinetuneTrainer(fcfg, mode="f16")
    try:
        tr.set_params(P)
        tr.set_batch(*_batch(fcfg, 8, seed=52))
        tr.backward()
        G, n_bad = {}, 0
        for k in P:
            g = _get(tr, k, 1)
            bad = ~np.isfinite(g)
            n_bad += int(bad.sum())
            G[k] = np.where(bad, np.float32(0), g)
        assert n_bad > 0
        assert tr.dropped_gradients == 0  # arp_ft_backward runs no AdamW
        M, V = _moments(G, seed=53)
        tr.set_tensors(M, 2)
        tr.set_tensors(V, 3)
        tr.step = 10
        tr.train_step(1e-3)
        dropped = tr.dropped_gradients
        print(f"  {geom} fuse={fuse}: {n_bad} non-finite gradient entries stored by arp_ft_backward, {dropped} dropped by the step")
        assert dropped == n_bad
        _check_adamw(tr, P, M, V, G, 10, 1e-3, 0.05, f"f16 dropped {geom} fuse={fuse}")
    finally:
        tr.close()
