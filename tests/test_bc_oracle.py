"""CPU tests of the InstructRL baseline (PolicyConfig(model="BC"), arp_dt/BC.py): the fp64 oracle in tests/bc_oracle.py against an independent
numpy forward and finite differences, its parameter tree, the causality of its action head, and the all-reduce bucket plan of the BC handle."""
import numpy as np
import torch

import bc_oracle as BO
from oracle import arpdt_torch as O

CFG = BO.PolicyConfig(emb=32, depth=2, heads=2, window=3, enc_tokens=3, enc_dim=64)


def _setup(B=4, seed=1):
    from arp_amd import synth_policy as S
    from arp_amd.train import PolicyConfig
    cfg = PolicyConfig(**{k: getattr(CFG, k) for k in ("emb", "depth", "heads", "window", "enc_tokens", "enc_dim")}, model="BC")
    Pn = S.policy_params(cfg, seed=seed, dtype=np.float64)
    enc, act, _ = S.policy_batch(cfg, B, seed=seed + 1, dtype=np.float64)
    P = {k: torch.from_numpy(v) for k, v in Pn.items()}
    return Pn, P, (enc, act), (torch.from_numpy(enc), torch.from_numpy(act).long())


def test_param_tree_is_arpdt_minus_rtg_input_and_return_head():
    from arp_amd import synth_policy as S
    from arp_amd.train import PolicyConfig
    for kw in ({}, dict(emb=64, depth=3, heads=4, window=5, enc_tokens=334)):
        arp, bc = O.param_shapes(O.PolicyConfig(**kw)), BO.param_shapes(O.PolicyConfig(**kw))
        gone = set(arp) - set(bc)
        assert set(bc) <= set(arp) and all(bc[k] == arp[k] for k in bc)
        assert gone == {"rtg_input/kernel", "return_outputs_0/layers_0/kernel", "return_outputs_0/layers_0/bias", "return_outputs_0/layers_2/kernel"}
        assert S.policy_param_shapes(PolicyConfig(**kw, model="BC")) == bc
        assert S.policy_param_shapes(PolicyConfig(**kw)) == arp
    # the reference's InstructRL encodings: 1 + 256 + 77 = 334 tokens per frame (m3ae/model.py:471-496) -> image_text_input [256 512, 128]
    assert BO.param_shapes(O.PolicyConfig(enc_tokens=334))["image_text_input/kernel"] == (256_512, 128)
    assert BO.num_params(O.PolicyConfig()) == O.num_params(O.PolicyConfig()) - (128 + 128 * 128 + 128 + 128)


def test_policy_config_rejects_an_unknown_model():
    import pytest
    from arp_amd.train import PolicyConfig
    with pytest.raises(ValueError):
        PolicyConfig(model="GCBC")
    assert PolicyConfig().model == "ARPDT"


def test_torch_forward_matches_numpy_forward():
    Pn, P, (enc, act), tb = _setup()
    out = BO.forward(P, CFG, *tb)
    assert set(out) == {"action_pred", "loss", "acc"}  # BC.py:181
    lg = BO.forward_numpy(Pn, CFG, enc, act)
    assert np.abs(out["action_pred"].numpy() - lg).max() < 1e-12
    lp = torch.log_softmax(out["action_pred"], -1)
    ce = -lp.gather(-1, tb[1][..., None]).mean()
    assert abs(float(out["loss"]) - float(ce) / CFG.n_actions) < 1e-12  # CE over all B*T*n_actions elements (BC.py:358-365)


def test_autograd_matches_finite_differences():
    Pn, P, _, tb = _setup()
    g, aux, _ = BO.grads(P, CFG, *tb)
    assert aux["trans_loss"] == 0.0 and aux["return_loss"] == 0.0  # main_procgen.py:120-121: output.get(..., 0.0)
    rng = np.random.default_rng(0)
    for name, v in P.items():
        for _ in range(2):
            idx = tuple(int(rng.integers(0, s)) for s in v.shape)
            eps = 1e-6
            up, dn = dict(P), dict(P)
            a = v.clone(); a[idx] += eps; up[name] = a
            b = v.clone(); b[idx] -= eps; dn[name] = b
            fd = (float(BO.loss_and_aux(up, CFG, *tb)[0]) - float(BO.loss_and_aux(dn, CFG, *tb)[0])) / (2 * eps)
            assert abs(fd - float(g[name][idx])) < 1e-4 * max(abs(fd), 1e-3), (name, idx, fd, float(g[name][idx]))


def test_action_head_is_causal_in_the_action_tokens():
    """The head reads the image-token rows 0::2 (BC.py:166): the logits at step t see action[:t] and never action[t:]."""
    _, P, _, (enc, act) = _setup(B=2)
    T = CFG.window
    base = BO.forward(P, CFG, enc, act)["action_pred"]
    for t in range(T):
        a2 = act.clone()
        a2[:, t:] = (a2[:, t:] + 1) % CFG.n_actions
        lg = BO.forward(P, CFG, enc, a2)["action_pred"]
        assert torch.equal(lg[:, :t + 1], base[:, :t + 1]), t  # steps <= t do not move when action[t:] changes
        if t > 0:
            a3 = act.clone()
            a3[:, t - 1] = (a3[:, t - 1] + 1) % CFG.n_actions
            assert (BO.forward(P, CFG, enc, a3)["action_pred"][:, t] - base[:, t]).abs().max() > 1e-6, t


def test_train_step_semantics():
    _, P, _, tb = _setup()
    cfg = BO.PolicyConfig(**{**CFG.__dict__, "clip_norm": 0.1})
    st, aux = BO.train_step(BO.init_state(P), cfg, [tb], lambda t: 0.0)
    assert all(torch.equal(st["params"][k], P[k]) for k in P) and st["step"] == 1 and aux["train_state_step"] == 0
    st2, aux2 = BO.train_step(st, cfg, [tb], lambda t: 1e-2)
    assert aux2["grad_norm"] > cfg.clip_norm
    d = (st2["params"]["image_text_input/bias"] - P["image_text_input/bias"]).abs()
    assert float(d.max()) <= 1e-2 * 1.6 and float(d.max()) > 1e-3


def test_bucket_plan_tiles_the_bc_gradient_exactly_once():
    from arp_amd.train import PolicyConfig, bucket_plan
    pad = lambda n: (n + 3) // 4 * 4  # every tensor of the flat buffer starts on a multiple of 4 floats
    for kw in ({}, dict(enc_tokens=334), dict(use_adapter=False), dict(emb=64, depth=3, heads=4, window=8, enc_tokens=5, enc_dim=64)):
        cfg = PolicyConfig(**kw, model="BC")
        ranges, total = bucket_plan(cfg)
        shapes = BO.param_shapes(O.PolicyConfig(**kw))
        assert total == sum(pad(int(np.prod(s))) for s in shapes.values())
        cover = np.zeros(total, np.int32)
        for lo, hi in ranges:
            assert 0 <= lo <= hi <= total
            cover[lo:hi] += 1
        assert (cover == 1).all(), "the bucket ranges must tile [0, P) exactly once"
        assert ranges[0][1] - ranges[0][0] >= cfg.enc_tokens * cfg.enc_dim * cfg.emb
        _, total_arp = bucket_plan(PolicyConfig(**kw))
        E = cfg.emb
        assert total_arp - total == pad(E) + pad(E * E) + pad(E) + pad(E)  # rtg_input/kernel + the return head
