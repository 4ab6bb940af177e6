"""GPU tests of the rollout session with the FINE-TUNED reward on the device (arp_rollout_create_ft; RolloutSession(reward_model=<FinetunedClip>)): the
whole loop against the fp64 oracle reward of every frame (oracle/clip_torch.py towers on oracle/preprocess.py frames, oracle/finetune_torch.py head) and
rollout_oracle's return-to-go; refusals and ownership."""
import ctypes as C

import numpy as np
import pytest

from rollout_oracle import RolloutOracle
from test_ft_reward_gpu import TINY_HEAD, TOWER, _Setup, _live

pytestmark = pytest.mark.gpu

TINY_ENC = dict(patch=16, width=64, layers=2, heads=2, img_res=64)  # tests/test_rollout_gpu.py: 17 tokens
P3 = dict(emb=64, depth=2, heads=4, window=3, enc_tokens=17, enc_dim=64, lambda_ret=0.5)
REWARD_BAR = 2e-2  # tests/test_ft_reward_gpu.py: f32, label transform


def _frames(n, seed):
    from arp_amd import synth
    return synth.procgen_like_frames(n, 64, 64, seed=seed)


def _stack(pkw, model="ARPDT"):
    from arp_amd import m3ae, synth_policy as S
    from arp_amd.train import PolicyConfig, PolicyTrainer
    from oracle import m3ae_np as M
    kw = {k: v for k, v in pkw.items() if not (model == "BC" and k == "lambda_ret")}
    pcfg = PolicyConfig(**kw) if model == "ARPDT" else PolicyConfig(**kw, model=model)
    enc = m3ae.M3AEEncoder(m3ae.EncoderConfig(**TINY_ENC), S.m3ae_params(M.EncConfig(**TINY_ENC), seed=5), mode="f32")
    tr = PolicyTrainer(pcfg, mode="f32")
    tr.set_params(S.policy_params(pcfg, seed=6))
    if model == "ARPDT":
        tr.attach_encoder(enc)
    return enc, tr, pcfg


def test_whole_loop_with_the_finetuned_reward(gpu_lib):
    """8 steps, E = 2, f32, tiny towers + head on the session's 64 x 64 frames through the label transform: after every step the session's reward is within
    2e-2 of the fp64 oracle reward of that frame, and its return-to-go within (t + 1) 2e-2 / scale of rollout_oracle driven by the oracle rewards --
    plain, and with use_normalize / reward_min."""
    from arp_amd.rollout import RolloutSession
    s = _Setup(TOWER, TINY_HEAD, seed=371, keys=[("label", False)], frames=np.concatenate([_frames(2, 1400 + t) for t in range(8)]))
    enc, tr, pcfg = _stack(P3)
    m = s.model("f32").set_text(s.tok).set_prompt_reduce("mean")
    ref = s.logits[("label", False)].mean(axis=0).reshape(8, 2)
    E, T, scale = 2, pcfg.window, 100.0
    try:
        for norm, rmin in ((False, 0.0), (True, -1.75)):
            ses = RolloutSession(tr, reward_model=m, n_envs=E, return_to_go=100.0, scale=scale, use_normalize=norm, reward_min=rmin)
            orc = [RolloutOracle(T, 100.0, scale, reward_min=rmin, use_normalize=norm) for _ in range(E)]
            try:
                ses.reset()
                for t in range(8):
                    act = ses.step(s.frames[2 * t: 2 * t + 2])
                    assert act.shape == (E,) and np.all((0 <= act) & (act < pcfg.n_actions))
                    for e in range(E):
                        orc[e].apply_reward(ref[t, e])
                    rew, rtg = ses.read("reward"), ses.read("rtg")
                    want = np.asarray([o.rtg[0] for o in orc])
                    print(f"norm {norm} step {t}: reward {rew} oracle {ref[t]} rtg {rtg} oracle {want}")
                    assert np.abs(rew - ref[t]).max() < REWARD_BAR
                    assert np.abs(rtg - want).max() <= (t + 1) * REWARD_BAR / scale
            finally:
                ses.close()
    finally:
        m.close(); tr.close(); enc.close()


def test_refusals_and_ownership(gpu_lib):
    from arp_amd import finetune as FT
    from arp_amd.rollout import RolloutSession
    lib = gpu_lib
    s = _Setup(TOWER, TINY_HEAD, seed=371, n_frames=1, keys=[("label", False)])
    enc, tr, pcfg = _stack(P3)
    benc, btr, _ = _stack(P3, model="BC")
    m = s.model("f32").set_text(s.tok)
    fr = _frames(2, 1500)
    h = s.hcfg
    try:
        # every handle's lazily sized workspace at the session's shapes before the counters are read
        warm = RolloutSession(tr, reward_model=m, n_envs=2)
        warm.reset()
        for t in range(3):
            warm.step(fr)
        warm.close()
        before = _live(lib)
        with pytest.raises(lib.ArpError, match="model BC reads no return-to-go"):
            RolloutSession(btr, reward_model=m, n_envs=2, encoder=benc)
        other = FT.FinetuneTrainer(FT.FinetuneConfig(layers=h.layers, width_v=128, width_t=h.width_t, embed=h.embed, hidden=h.hidden, n_actions=h.n_actions), mode="f32")
        try:
            with pytest.raises(lib.ArpError, match="do not match"):
                RolloutSession(tr, reward_model=FT.FinetunedClip(m.towers, other), n_envs=2)
        finally:
            other.close()
        if lib.device_count() >= 2:  # head and towers on different devices
            other = FT.FinetuneTrainer(m.head.cfg, mode="f32", device=1)
            try:
                with pytest.raises(lib.ArpError, match="device"):
                    RolloutSession(tr, reward_model=FT.FinetunedClip(m.towers, other), n_envs=2)
            finally:
                other.close()
                lib.check(lib.lib.arp_set_device(0))
        assert _live(lib) == before  # a refused create holds nothing
        ses = RolloutSession(tr, reward_model=m, n_envs=2)
        ses.reset()
        with pytest.raises(lib.ArpError, match="owns a reward handle"):
            ses.step(fr, rewards=[0.0, 0.0])
        for t in range(3):  # the refusal came before any launch: the session goes on
            ses.step(_frames(2, 1510 + t))
        assert np.all(ses.read("len") == 3) and np.all(np.isfinite(ses.read("rtg"))) and np.all(ses.read("reward") != 0)
        ses.close()
        assert _live(lib) == before  # a session created with arp_rollout_create_ft, stepped and destroyed
        assert np.all(np.isfinite(m.reward(fr, transform="label")))  # the reward model stays usable
    finally:
        m.close(); btr.close(); benc.close(); tr.close(); enc.close()
