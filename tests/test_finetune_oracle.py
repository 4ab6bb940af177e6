"""CPU: the torch restatement of the fine-tune head (oracle/finetune_torch.py) against the fixture produced by running the
reference class itself under import stand-ins (tests/golden/make_golden_finetune.py)."""
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def load_golden(goal=False):
    from oracle import finetune_torch as O
    g = np.load(os.path.join(HERE, "golden", "finetune_tiny_goal.npz" if goal else "finetune_tiny.npz"))
    L, wv, wt, embed, hid, na = [int(v) for v in g["cfg"]]
    cfg = O.HeadConfig(layers=L, width_v=wv, width_t=wt, embed=embed, hidden=hid, n_actions=na, gamma=float(g["gamma"]),
                       logit_scale=float(g["logit_scale"]), goal_conditioned=goal)
    P = {k[6:]: g[k] for k in g.files if k.startswith("param:")}
    G = {k[5:]: g[k] for k in g.files if k.startswith("grad:")}
    batch = (g["img_inter"], g["img_final"], None if goal else g["txt_inter"], None if goal else g["txt_final"], g["r"], g["action"])
    return cfg, P, G, batch, g


def test_goal_conditioned_variant_matches_the_reference_class():
    """clip_multiscale_adapter.py:208-212,224-230 (goal_conditioned=True): fixture = the reference class itself with that switch on
    (make_golden_finetune.py --goal).  Loss, both components, every gradient; the text head's parameters get NO gradient."""
    from oracle import finetune_torch as O
    cfg, P, G, batch, g = load_golden(goal=True)
    assert int(g["goal_conditioned"]) == 1 and batch[0].shape[0] == 4
    got, aux = O.grads(P, cfg, batch)
    assert abs(aux["loss"] - float(g["loss"])) < 2e-5 and abs(aux["vip_loss"] - float(g["vip_loss"])) < 2e-5
    assert abs(float(P["lambda_id"]) * aux["id_loss"] - float(g["lambda_id_times_id_loss"])) < 2e-5
    for k in G:
        scale = max(np.abs(G[k]).max(), 1e-6)
        assert np.abs(got[k] - G[k]).max() / scale < 2e-4, k
    text_side = {k for k in P if k.startswith("text_")}
    assert text_side <= set(aux["no_grad"]) and all(not np.any(G[k]) for k in text_side)


def test_param_tree_matches_reference_state_dict():
    from oracle import finetune_torch as O
    cfg, P, _, _, _ = load_golden()
    shapes = O.param_shapes(cfg)
    assert set(shapes) == set(P)
    for k, s in shapes.items():
        assert tuple(P[k].shape) == tuple(s), k


def test_loss_and_components_match_reference():
    from oracle import finetune_torch as O
    cfg, P, _, batch, g = load_golden()
    _, aux = O.grads(P, cfg, batch)
    assert abs(aux["loss"] - float(g["loss"])) < 2e-5
    assert abs(aux["vip_loss"] - float(g["vip_loss"])) < 2e-5
    assert abs(float(P["lambda_id"]) * aux["id_loss"] - float(g["lambda_id_times_id_loss"])) < 2e-5


def test_gradients_match_reference_autograd():
    from oracle import finetune_torch as O
    cfg, P, G, batch, _ = load_golden()
    got, _ = O.grads(P, cfg, batch)
    for k in G:
        scale = max(np.abs(G[k]).max(), 1e-6)
        assert np.abs(got[k] - G[k]).max() / scale < 2e-4, k  # the reference ran in float32


def test_vip_exponent_broadcasts_to_a_matrix():
    """r is [B,1] and the scores [B]: the reference's mean runs over B*B terms (clip_multiscale_adapter.py:216-220)."""
    from oracle import finetune_torch as O
    cfg, P, _, batch, _ = load_golden()
    out = O.forward(O.to_torch(P), cfg, *[torch.as_tensor(b, dtype=torch.float64) for b in batch[:5]], torch.as_tensor(batch[5]))
    s = out["scores"].numpy()
    r = batch[4].astype(np.float64) - 1.0
    mat = np.exp(-(r[:, None] + cfg.gamma * s[2][None, :] - s[1][None, :]))
    vip = (1 - cfg.gamma) * -s[0].mean() + np.log(1e-8 + mat.mean())
    assert abs(vip - float(out["vip_loss"])) < 1e-10
    per_sample = np.exp(-(r + cfg.gamma * s[2] - s[1])).mean()
    assert abs(np.log(1e-8 + per_sample) - np.log(1e-8 + mat.mean())) > 1e-6  # a per-sample reading would differ


@pytest.mark.parametrize("use_id", [True, False])
def test_adamw_matches_torch(use_id):
    """incl. use_id_loss off: the inverse model and lambda_id then have .grad None and torch.optim.AdamW leaves them untouched
    (no decoupled decay either) -- ADVICE r1."""
    import dataclasses
    from oracle import finetune_torch as O
    cfg, P, _, batch, _ = load_golden()
    cfg = dataclasses.replace(cfg, use_id=use_id)
    Pt = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in P.items()}
    opt = torch.optim.AdamW(list(Pt.values()), lr=1e-3, weight_decay=0.01)
    for _ in range(3):
        opt.zero_grad()
        out = O.forward(Pt, cfg, *[torch.as_tensor(b, dtype=torch.float64) for b in batch[:5]], torch.as_tensor(batch[5]))
        out["loss"].backward()
        opt.step()
    got, _ = O.train_steps(P, cfg, [batch], 1e-3, 0.01, 3)
    for k in P:
        assert np.abs(got[k] - Pt[k].detach().numpy()).max() < 1e-9, k
    if not use_id:
        assert all(np.array_equal(got[k], np.asarray(P[k], np.float64)) for k in P if k.startswith("inverse_layer.") or k == "lambda_id")


# ---- the rounded-operand emulation of the 16-bit modes (Rounding) ----------------------------------------------------------------------
EMU_MID = dict(layers=3, width_v=128, width_t=64, embed=64, hidden=64, n_actions=15)


def _emu_case(goal=False, B=7, seed=3, **kw):
    from oracle import finetune_torch as O
    cfg = O.HeadConfig(**EMU_MID, goal_conditioned=goal, **kw)
    P = O.init_params(cfg, seed=seed)
    P["image_residual_weight"] = np.float32(0.4) * np.ones((), np.float32)
    P["text_residual_weight"] = np.float32(-0.6) * np.ones((), np.float32)
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    G = 4 if goal else 3
    batch = (rng.standard_normal((G, B, cfg.d_img)).astype(np.float32), rng.standard_normal((G, B, cfg.embed)).astype(np.float32),
             None if goal else rng.standard_normal((B, cfg.d_txt)).astype(np.float32), None if goal else rng.standard_normal((B, cfg.embed)).astype(np.float32),
             rng.integers(0, 2, B).astype(np.float32), rng.integers(0, cfg.n_actions, B))
    return cfg, P, batch


def test_emulation_off_is_the_plain_oracle():
    """operand=None runs the plain code; with every rounding point switched off (and the seed scale still applied) the emulation's own
    graph equals it to float64 round-off -- it restates the same head, only the roundings differ."""
    from oracle import finetune_torch as O
    cfg, P, batch = _emu_case()
    g0, a0 = O.grads(P, cfg, batch)
    g1, a1 = O.grads(P, cfg, batch, operand=None)
    assert a0["loss"] == a1["loss"] and all(np.array_equal(g0[k], g1[k]) for k in g0)
    for mode in ("f16", "bf16"):
        g2, a2 = O.grads(P, cfg, batch, operand=mode, skip=O.Rounding.POINTS)
        assert abs(a2["loss"] - a0["loss"]) < 1e-14 * abs(a0["loss"])
        for k in g0:
            assert np.abs(g2[k] - g0[k]).max() <= 1e-13 * max(np.abs(g0[k]).max(), 1e-300), (mode, k)


@pytest.mark.parametrize("mode", ["f16", "bf16"])
def test_every_rounding_point_fires(mode):
    """Each point produces values exactly representable in the operand type, and switching any ONE of them off changes the gradients."""
    from oracle import finetune_torch as O
    dt = {"f16": torch.float16, "bf16": torch.bfloat16}[mode]
    cfg, P, batch = _emu_case()
    trace = {}
    g, _ = O.grads(P, cfg, batch, operand=mode, trace=trace)
    assert set(trace) == set(O.Rounding.POINTS)
    for point, vals in trace.items():
        for v in vals:
            assert torch.equal(v, v.to(dt).to(v.dtype)), point
        assert any(bool((v != 0).any()) for v in vals), point
    for point in O.Rounding.POINTS:
        gp, _ = O.grads(P, cfg, batch, operand=mode, skip=(point,))
        assert max(float(np.abs(gp[k] - g[k]).max()) for k in g) > 0, point


@pytest.mark.parametrize("mode,lo,hi", [("f16", 1e-4, 1e-2), ("bf16", 1e-3, 1e-1)])
def test_emulation_differs_from_fp64_by_the_operand_rounding(mode, lo, hi):
    """MID geometry, B = 7: per-tensor relative L2 distance of the emulation from plain fp64.  Recorded: f16 1.9e-4 .. 3.2e-3, bf16
    5.0e-3 .. 3.1e-2; the gradients the GPU keeps in f32 end to end (c2, lambda_id) move only through the rounded forward: f16 1e-6,
    bf16 3e-5.  Every rounded tensor sits between lo and hi, the f32 ones below lo."""
    from oracle import finetune_torch as O
    cfg, P, batch = _emu_case()
    g0, a0 = O.grads(P, cfg, batch)
    g, a = O.grads(P, cfg, batch, operand=mode)
    assert 0 < abs(a["loss"] - a0["loss"]) < hi * abs(a0["loss"])
    for k in g0:
        rel = np.linalg.norm(g[k] - g0[k]) / np.linalg.norm(g0[k])
        if k in ("inverse_layer.layers.3.bias", "lambda_id"):  # f32 on the GPU: moved only through the rounded forward
            assert rel < lo, (k, rel)
        else:
            assert lo < rel < hi, (k, rel)


def test_emulation_keeps_the_configuration_switches():
    """goal_conditioned and use_vip / use_id run through the same rounded code: the text head gets no gradient without a text tower, the
    inverse model none without the id loss, and each case stays within the operand rounding of fp64."""
    from oracle import finetune_torch as O
    for goal, kw in ((True, {}), (False, dict(use_vip=False)), (False, dict(use_id=False))):
        cfg, P, batch = _emu_case(goal=goal, B=5, **kw)
        g0, a0 = O.grads(P, cfg, batch)
        g, a = O.grads(P, cfg, batch, operand="f16")
        assert set(a["no_grad"]) == set(a0["no_grad"])
        for k in g0:
            if k in a0["no_grad"]:
                assert not np.any(g[k]), k
            else:
                assert np.linalg.norm(g[k] - g0[k]) <= 5e-2 * np.linalg.norm(g0[k]), (goal, kw, k)  # recorded worst 3.8e-2: a residual-weight sum


def test_emulation_rounds_the_scaled_gradient():
    """The points round scale * value.  bfloat16 has f32's range: any power-of-two seed scale commutes with its roundings exactly.  binary16
    does not: unscaled, small gradient operands fall into its subnormals (why the f16 mode seeds x1024); scaled far past its range the
    16-bit copies saturate at +-65504 (transpose_mask_kernel) and the gradients stay finite but wrong."""
    from oracle import finetune_torch as O
    cfg, P, batch = _emu_case()
    g_bf, _ = O.grads(P, cfg, batch, operand="bf16")
    g_bf_big, _ = O.grads(P, cfg, batch, operand="bf16", grad_scale=2.0 ** 30)
    assert all(np.array_equal(g_bf[k], g_bf_big[k]) for k in g_bf)
    g, _ = O.grads(P, cfg, batch, operand="f16")
    g1, _ = O.grads(P, cfg, batch, operand="f16", grad_scale=1.0)
    assert any(not np.array_equal(g[k], g1[k]) for k in g)
    g_big, _ = O.grads(P, cfg, batch, operand="f16", grad_scale=2.0 ** 30)
    assert all(np.isfinite(v).all() for v in g_big.values())
    k = "image_adapter.layers.0.weight"
    assert np.linalg.norm(g_big[k] - g[k]) > 0.1 * np.linalg.norm(g[k])
