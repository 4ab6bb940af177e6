"""GPU tests of the InstructRL baseline policy (PolicyConfig(model="BC"), arp_dt/BC.py) through the C ABI, against the fp64 oracle in
tests/bc_oracle.py: logits, losses and every gradient in the f32 parity mode, train trajectories, the fused kernel's two-token form against the
per-op path, causality of the action head, north_star's 1e-3 on the f16 logits at the real geometry (257 and 334 encoder tokens), the RCCL and
prefetch paths, and the reference's call surface (aux keys, greedy_action; no greedy_return, no image-only encoder)."""
import ctypes as C

import numpy as np
import pytest
import torch

import bc_oracle as BO

pytestmark = pytest.mark.gpu

TINY = dict(emb=64, depth=2, heads=4, window=3, enc_tokens=5, enc_dim=64)
SMALL = dict(emb=128, depth=2, heads=8, window=4, enc_tokens=9, enc_dim=128)


def _setup(kw, B, seed):
    from arp_amd import synth_policy as S
    from arp_amd.train import PolicyConfig
    cfg, ocfg = PolicyConfig(**kw, model="BC"), BO.PolicyConfig(**kw)
    P = S.policy_params(cfg, seed=seed)
    enc, act, _ = S.policy_batch(cfg, B, seed=seed + 1)
    Pt = {k: torch.from_numpy(v).double() for k, v in P.items()}
    tb = (torch.from_numpy(enc).double(), torch.from_numpy(act).long())
    return cfg, ocfg, P, (enc, act), Pt, tb


def _grad_errs(g, g_ref):
    return {k: float(np.abs(g[k] - g_ref[k].numpy()).max() / max(np.abs(g_ref[k].numpy()).max(), 1e-6)) for k in g_ref}


@pytest.mark.parametrize("kw,B", [(TINY, 4), (SMALL, 6), (TINY, 3)])
def test_f32_forward_and_gradients_match_oracle(gpu_lib, kw, B):
    from arp_amd.train import PolicyTrainer
    cfg, ocfg, P, (enc, act), Pt, tb = _setup(kw, B, 3)
    g_ref, _, ref = BO.grads(Pt, ocfg, *tb)
    tr = PolicyTrainer(cfg, mode="f32")
    assert set(tr.shapes) == set(BO.param_shapes(ocfg)) and all(tr.shapes[k] == v for k, v in BO.param_shapes(ocfg).items())
    tr.set_params(P)
    tr.set_batch(enc, act)  # no rtg: BC reads none
    out = tr.forward()
    assert set(out) == {"action_pred", "loss", "acc"}  # BC.py:181
    e = float(np.abs(out["action_pred"] - ref["action_pred"].numpy()).max())
    print(f"BC f32 logits err {e:.2e}")
    assert e <= 2e-5, e
    assert abs(out["loss"] - float(ref["loss"])) <= 1e-5 and abs(out["acc"] - float(ref["acc"])) <= 1e-5
    tr.backward()
    errs = _grad_errs(tr.get_grads(), g_ref)
    bad = {k: v for k, v in errs.items() if not v <= 1e-4}
    assert not bad, bad
    tr.close()


def test_f32_train_steps_match_oracle(gpu_lib):
    """3 steps with global-norm clipping active and a warm-up schedule from lr 0, as tests/test_policy_gpu.py runs ARP-DT's."""
    from arp_amd.train import PolicyTrainer
    cfg, ocfg, P, (enc, act), Pt, tb = _setup(dict(TINY, clip_norm=0.5), 4, 7)
    lr_fn = lambda t: 2e-3 * min(1.0, t / 2.0)
    tr = PolicyTrainer(cfg, mode="f32")
    tr.set_params(P)
    st = BO.init_state(Pt)
    for s in range(3):
        tr.set_batch(enc, act)
        aux = tr.train_step(lr_fn(tr.step))
        st, oaux = BO.train_step(st, ocfg, [tb], lr_fn)
        assert aux["train_state_step"] == s and aux["trans_loss"] == 0.0 and aux["return_loss"] == 0.0
        for k in ("loss", "weight_penalty", "weight_l2", "acc"):
            assert abs(aux[k] - oaux[k]) <= max(2e-5, 1e-6 * abs(oaux[k])), (s, k, aux[k], oaux[k])
        assert abs(aux["grad_norm"] - oaux["grad_norm"]) <= 1e-4
    got = tr.get_params()
    mean_err = float(np.mean([np.abs(got[k] - st["params"][k].numpy()).mean() for k in P]))
    # Adam's first steps are sign-like: an element whose gradient is ~0 may move by a fraction of lr either way (the ARP-DT test's reason for its 1e-4)
    max_err = max(float(np.abs(got[k] - st["params"][k].numpy()).max()) for k in P)
    print(f"BC 3-step trajectory: mean param err {mean_err:.2e}, max {max_err:.2e}")
    assert mean_err <= 2e-6 and max_err <= 1e-4
    tr.close()


@pytest.mark.parametrize("kw,B", [(TINY, 4), (SMALL, 6), (dict(TINY, window=8), 3)])  # window 8: 16 tokens, the fused kernel's last BC window
def test_fused_bc_kernel_matches_per_op_path(gpu_lib, kw, B, monkeypatch):
    from arp_amd.train import PolicyTrainer
    cfg, _, P, (enc, act), _, _ = _setup(kw, B, 11)
    res = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("ARP_DT_FUSED", fused)
        tr = PolicyTrainer(cfg, mode="f32")
        tr.set_params(P)
        tr.set_batch(enc, act)
        out = tr.forward()
        tr.backward()
        res[fused] = (out, tr.get_grads())
        tr.close()
    (o1, g1), (o0, g0) = res["1"], res["0"]
    assert np.abs(o1["action_pred"] - o0["action_pred"]).max() <= 1e-5
    assert abs(o1["loss"] - o0["loss"]) <= 1e-5 and abs(o1["acc"] - o0["acc"]) <= 1e-5
    bad = [(k, float(np.abs(g1[k] - g0[k]).max() / max(np.abs(g0[k]).max(), 1e-6))) for k in P]
    bad = [b for b in bad if not b[1] <= 5e-5]
    assert not bad, bad


def test_window_nine_runs_per_op_and_matches_oracle(gpu_lib):
    """2 x 9 = 18 tokens: past the fused kernel's 16-row tile, the per-op path's two-token form."""
    from arp_amd.train import PolicyTrainer
    cfg, ocfg, P, (enc, act), Pt, tb = _setup(dict(TINY, window=9), 3, 17)
    g_ref, _, ref = BO.grads(Pt, ocfg, *tb)
    tr = PolicyTrainer(cfg, mode="f32")
    tr.set_params(P)
    tr.set_batch(enc, act)
    assert np.abs(tr.forward()["action_pred"] - ref["action_pred"].numpy()).max() <= 2e-5
    tr.backward()
    errs = _grad_errs(tr.get_grads(), g_ref)
    bad = {k: v for k, v in errs.items() if not v <= 2e-4}
    assert not bad, bad
    tr.close()


@pytest.mark.parametrize("fused", ["1", "0"])
def test_action_head_is_causal_on_the_gpu(gpu_lib, fused, monkeypatch):
    """The logits at step t read the image-token row 2t: bitwise unchanged when action[t:] changes."""
    from arp_amd.train import PolicyTrainer
    monkeypatch.setenv("ARP_DT_FUSED", fused)
    cfg, _, P, (enc, act), _, _ = _setup(dict(TINY, window=4), 3, 19)
    tr = PolicyTrainer(cfg, mode="f32")
    tr.set_params(P)
    tr.set_batch(enc, act)
    base = tr.forward()["action_pred"]
    for t in range(cfg.window):
        a2 = act.copy()
        a2[:, t:] = (a2[:, t:] + 1 + t) % cfg.n_actions
        tr.set_batch(enc, a2)
        lg = tr.forward()["action_pred"]
        assert np.array_equal(lg[:, :t + 1], base[:, :t + 1]), t
        if t + 1 < cfg.window:  # ... and the later steps do see it
            assert np.abs(lg[:, t + 1:] - base[:, t + 1:]).max() > 0, t
    tr.close()


@pytest.mark.parametrize("enc_tokens", [257, 334])
def test_f16_real_geometry_logits_over_eight_seeds(gpu_lib, enc_tokens):
    """north_star's 1e-3 on the f16 logits at the real geometry (emb 128, depth 2, B = 32, window 4, 768-wide encodings): ARP-DT's 257 tokens,
    and the 334 of the reference's InstructRL encodings (image + instruction text, BC.py:286-321) -> image_text_input K = 256 512."""
    from arp_amd.train import PolicyTrainer
    kw = dict(enc_tokens=enc_tokens)
    tr = None
    errs = []
    for seed in range(8):
        cfg, ocfg, P, (enc, act), Pt, tb = _setup(kw, 32, 200 + 11 * seed)
        with torch.no_grad():
            ref = BO.forward(Pt, ocfg, *tb)["action_pred"].numpy()
        if tr is None:
            tr = PolicyTrainer(cfg, mode="f16")
        tr.set_params(P)
        tr.set_batch(enc, act)
        errs.append(float(np.abs(tr.forward()["action_pred"] - ref).max()))
    tr.close()
    print(f"BC f16, {enc_tokens} tokens, 8 seeds: logits max err {max(errs):.2e} (per seed {min(errs):.2e} .. {max(errs):.2e})")
    assert max(errs) <= 1e-3, errs


@pytest.mark.parametrize("mode", ["f32", "f16"])
def test_forced_comm_steps_equal_plain_steps(gpu_lib, monkeypatch, mode):
    """RCCL at world 1 with the comm path forced, overlapped (two buckets) and serial: bit-identical to the step without a communicator."""
    from arp_amd.train import PolicyTrainer
    cfg, _, P, (enc, act), _, _ = _setup(SMALL, 6, 21)
    res = {}
    for name, env in (("plain", None), ("serial", {"ARP_DT_FORCE_COMM": "1", "ARP_DT_OVERLAP": "0"}), ("overlap", {"ARP_DT_FORCE_COMM": "1", "ARP_DT_OVERLAP": "1"})):
        for k in ("ARP_DT_FORCE_COMM", "ARP_DT_OVERLAP"):
            monkeypatch.delenv(k, raising=False)
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
        tr = PolicyTrainer(cfg, mode=mode)
        tr.set_params(P)
        if env:
            tr.comm_init(PolicyTrainer.new_unique_id(), 1, 0)
            tr.broadcast_state()
        auxs = []
        for _ in range(5):  # eager, eager, capture, replay, replay of every staged graph
            tr.set_batch(enc, act)
            auxs.append(tr.train_step(1e-3))
        res[name] = (tr.get_params(), auxs, tr.get_grads())
        tr.close()
    for other in ("serial", "overlap"):
        for k in P:
            assert np.array_equal(res["plain"][0][k], res[other][0][k]), (other, k)
            assert np.array_equal(res["plain"][2][k], res[other][2][k]), (other, "grad", k)
        assert [a["loss"] for a in res["plain"][1]] == [a["loss"] for a in res[other][1]]


def test_prefetched_rtg_less_batches_equal_synchronous_upload(gpu_lib):
    """prefetch_to_device with BC batches (no "rtg" key): the same trajectory as set_batch, bit for bit; the aux keys are the reference's with
    trans_loss = return_loss = 0.0 (main_procgen.py:118-124,153-157)."""
    from arp_amd import synth_policy as S
    from arp_amd.train import AUX_KEYS, TrainState, create_train_step, create_val_step, prefetch_to_device
    cfg, ocfg, P, _, Pt, _ = _setup(SMALL, 4, 31)
    batches = []
    for i in range(6):
        enc, act, _ = S.policy_batch(cfg, 4, seed=40 + i)
        batches.append({"image": {"ob": enc}, "action": act})

    def run(prefetch):
        state = TrainState.create(cfg, P, mode="f32")
        fn, vfn = create_train_step(cfg, lambda s: 1e-3, cfg.weight_decay), create_val_step(cfg)
        rng, out = np.array([0, 42], np.uint32), []
        src = prefetch_to_device(iter(batches), 2, state.trainer) if prefetch else iter(batches)
        for b in src:
            state, aux, rng = fn(state, b, rng)
            out.append(aux)
        vaux, _ = vfn(state, batches[0], rng)
        p = state.params
        state.trainer.close()
        return out, p, vaux

    a, pa, va = run(False)
    b, pb, vb = run(True)
    assert [x["loss"] for x in a] == [x["loss"] for x in b] and all(np.array_equal(pa[k], pb[k]) for k in pa)
    assert set(AUX_KEYS) <= set(a[0]) and all(x["trans_loss"] == 0.0 and x["return_loss"] == 0.0 for x in a + b)
    assert va == vb and set(va) == {"loss", "trans_loss", "return_loss", "acc"} and va["trans_loss"] == 0.0 and va["return_loss"] == 0.0
    # the first step's aux against the oracle's loss_fn, and val_fn on the trained parameters
    _, oaux, _ = BO.grads(Pt, ocfg, torch.from_numpy(batches[0]["image"]["ob"]).double(), torch.from_numpy(batches[0]["action"]).long())
    assert abs(a[0]["loss"] - oaux["loss"]) <= 1e-5 and abs(a[0]["acc"] - oaux["acc"]) <= 1e-3
    ov = BO.val_aux({k: torch.from_numpy(v).double() for k, v in pa.items()}, ocfg, torch.from_numpy(batches[0]["image"]["ob"]).double(),
                    torch.from_numpy(batches[0]["action"]).long())
    assert abs(va["loss"] - ov["loss"]) <= 1e-5 and abs(va["acc"] - ov["acc"]) <= 1e-3


def test_greedy_action_and_what_bc_refuses(gpu_lib):
    """BC.greedy_action (BC.py:351-355) is the argmax of the last step's logits; BC has no greedy_return, and the image-only M3AE encoder cannot sit
    in front of it (the reference's InstructRL encoder also reads the instruction).  ARP-DT without rtg stays an error."""
    from arp_amd import _ffi
    from arp_amd import synth_policy as S
    from arp_amd.train import PolicyConfig, PolicyTrainer
    cfg, ocfg, P, (enc, act), Pt, tb = _setup(TINY, 2, 13)
    ref = BO.forward(Pt, ocfg, *tb)["action_pred"]
    tr = PolicyTrainer(cfg, mode="f32")
    tr.set_params(P)
    assert (tr.greedy_action(enc, act) == ref[:, -1].argmax(-1).numpy()).all()
    rtg = np.ones((2, cfg.window, 1), np.float32)
    assert (tr.greedy_action(enc, act, rtg) == ref[:, -1].argmax(-1).numpy()).all()  # a non-None rtg is ignored, as BC.encode does
    with pytest.raises(ValueError):
        tr.greedy_return(enc, act, rtg)
    with pytest.raises(_ffi.ArpError, match="model BC"):
        # refused on the model alone, before the encoder handle is read: any non-null pointer stands in for one here
        _ffi.check(_ffi.lib.arp_dt_attach_encoder(tr._h, tr._h))
    logits = np.empty((2, cfg.window, cfg.n_actions), np.float32)
    ret = np.empty((2, cfg.window, 1), np.float32)
    with pytest.raises(_ffi.ArpError, match="return_pred"):
        _ffi.check(_ffi.lib.arp_dt_forward(tr._h, _ffi.as_ptr(logits, C.c_float), _ffi.as_ptr(ret, C.c_float), None))
    tr.close()
    arp = PolicyTrainer(PolicyConfig(**TINY), mode="f32")
    arp.set_params(S.policy_params(PolicyConfig(**TINY), seed=13))
    with pytest.raises(_ffi.ArpError, match="rtg"):
        arp.set_batch(enc, act)
    arp.close()
