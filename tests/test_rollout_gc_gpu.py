"""GPU tests of the rollout session that carries one goal frame per environment (arp_rollout_create_gc / arp_rollout_reset_goal,
RolloutSession(..., goal_conditioned=True)): model GCBC through the session -- ring logic with goals, short windows against fp64, the session against the
host-driven way at 339-token pairs (the encoder's latency path) -- and the clip_goal_conditioned reward on the device for an ARP-DT policy.

Oracles: tests/gcbc_oracle.py (the encoder's goal-conditioned call, fp64), tests/bc_oracle.py (GCBC's policy is BC's), tests/rollout_oracle.py (the reference
loop's window handling), oracle/clip_np.py (the CLIP towers, fp64)."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import bc_oracle as BO
import gcbc_oracle as G
from conftest import TINY
from rollout_oracle import RolloutOracle, padded

pytestmark = pytest.mark.gpu

SMALL_ENC = dict(patch=16, width=128, layers=2, heads=2, img_res=64)    # 33-token pairs, LDS-resident attention
LONG_ENC = dict(patch=16, width=128, layers=2, heads=2, img_res=208)    # 339-token pairs, key-blocked attention; one pair is under the default row limit
TINY_ENC = dict(patch=16, width=64, layers=2, heads=2, img_res=64)      # the ARP-DT policy's plain encoder (tests/test_rollout_gpu.py): 17 tokens
P3 = dict(emb=64, depth=2, heads=4, window=3)
P4 = dict(emb=128, depth=2, heads=8, window=4)  # the fused policy kernel
ENC_TOL = {"f32": 2e-5, "f16": 8e-3}  # tests/test_gc_encoder_gpu.py::TOL
BC_LOGITS_BAR_F32 = 2e-5              # tests/test_bc_gpu.py: f32 BC logits against the fp64 oracle
GCBC_LOGITS_BAR_F16 = 1.5e-3          # tests/test_gcbc_gpu.py::test_gcbc_logits_against_float64: the toy-geometry f16 bar


def _frames(n, seed, res=64):
    from arp_amd import synth
    return synth.procgen_like_frames(n, res, res, seed=seed)


def _gcbc_stack(enc_kw, pkw, pmode, emode, seed=6):
    from arp_amd import m3ae, synth_policy as S
    from arp_amd.train import PolicyConfig, PolicyTrainer
    from oracle import m3ae_np as M
    ecfg, ocfg = m3ae.EncoderConfig(**enc_kw), M.EncConfig(**enc_kw)
    kw = dict(**pkw, enc_tokens=ecfg.gc_tokens, enc_dim=ecfg.width)
    pcfg = PolicyConfig(**kw, model="GCBC")
    EP, P = S.m3ae_params(ocfg, seed=5), S.policy_params(pcfg, seed=seed)
    enc = m3ae.M3AEEncoder(ecfg, EP, mode=emode)
    tr = PolicyTrainer(pcfg, mode=pmode)
    tr.set_params(P)
    tr.attach_encoder(enc)
    return enc, tr, pcfg, kw, ocfg, EP, P


def _arpdt_stack(pmode="f32", emode="f32"):
    from arp_amd import m3ae, synth_policy as S
    from arp_amd.train import PolicyConfig, PolicyTrainer
    from oracle import m3ae_np as M
    pcfg = PolicyConfig(**P3, enc_tokens=17, enc_dim=64, lambda_ret=0.5)
    enc = m3ae.M3AEEncoder(m3ae.EncoderConfig(**TINY_ENC), S.m3ae_params(M.EncConfig(**TINY_ENC), seed=5), mode=emode)
    tr = PolicyTrainer(pcfg, mode=pmode)
    tr.set_params(S.policy_params(pcfg, seed=6))
    tr.attach_encoder(enc)
    return enc, tr, pcfg


def _live(lib):
    out = (C.c_int64 * 5)()
    lib.check(lib.lib.arp_debug_live(out))
    return list(out)


def _gc_ref(EP, ocfg, frames_u8, goals_u8):
    from arp_amd import dataset
    return G.forward_gc_representations(EP, ocfg, dataset.bytes_to_float(frames_u8), dataset.bytes_to_float(goals_u8))


def test_refusals_and_ownership(gpu_lib):
    """What arp_rollout_create_gc accepts and refuses, what a goal-carrying session refuses, and the live-resource counters around all of it.  (On a tree
    without create_gc the first goal_conditioned session cannot be made: this test fails there.)"""
    from arp_amd import clip, finetune as FT, m3ae, synth, synth_policy as S
    from arp_amd.rollout import RolloutSession
    from arp_amd.train import PolicyConfig, PolicyTrainer
    from oracle import clip_np as CN
    lib = gpu_lib
    enc, tr, pcfg, kw, ocfg, EP, P = _gcbc_stack(SMALL_ENC, P3, "f32", "f32")
    aenc, atr, apcfg = _arpdt_stack()
    bc = PolicyTrainer(PolicyConfig(**kw, model="BC"), mode="f32")
    bc.set_params(S.policy_params(PolicyConfig(**kw, model="BC"), seed=6))
    lab = clip.ClipLabeller(clip.ClipConfig(**TINY), synth.clip_weights(CN.ClipConfig(**TINY), seed=11), mode="f32")  # no prompt set
    fr, goals = _frames(2, 700), _frames(2, 701)
    try:
        # every handle's lazily sized workspace at the sessions' shapes before the counters are read
        for t_, rm in ((tr, None), (atr, lab)):
            warm = RolloutSession(t_, reward_model=rm, n_envs=2, goal_conditioned=True)
            warm.reset(goals=goals)
            for _ in range(4):
                warm.step(fr)
            warm.close()
        gc.collect()
        before = _live(lib)
        with pytest.raises(lib.ArpError, match="goal frame per episode"):
            RolloutSession(tr, n_envs=1)  # the plain constructors keep refusing model GCBC
        with pytest.raises(lib.ArpError, match="model BC reads no goal frame"):
            RolloutSession(bc, n_envs=2, encoder=enc, goal_conditioned=True)
        with pytest.raises(lib.ArpError, match="pass a labelling handle"):
            RolloutSession(atr, n_envs=2, goal_conditioned=True)
        with pytest.raises(lib.ArpError, match="a reward handle is refused"):
            RolloutSession(tr, reward_model=lab, n_envs=2, goal_conditioned=True)
        with pytest.raises(lib.ArpError, match="fine-tuned goal reward stays with the host function"):
            RolloutSession(atr, reward_model=FT.FinetunedClip(lab, None), n_envs=2, goal_conditioned=True)
        h = C.c_void_p()
        assert lib.lib.arp_rollout_create_gc(tr._h, None, None, 2, 32, 64, 100.0, C.byref(h)) < 0 and "the attached encoder reads 64 x 64" in lib.last_error()
        assert _live(lib) == before  # a refused create holds nothing
        plain = RolloutSession(atr, n_envs=2)
        with pytest.raises(lib.ArpError, match="arp_rollout_create_gc"):
            plain.reset(goals=goals)
        with pytest.raises(lib.ArpError, match="goal exists on a session that carries goal frames"):
            plain.read("goal")
        plain.close()
        ses = RolloutSession(tr, n_envs=2, goal_conditioned=True)
        with pytest.raises(lib.ArpError, match="step before the first reset"):
            ses.step(fr)
        ses.reset()  # a plain reset installs no goal
        with pytest.raises(lib.ArpError, match="environment 0 has no goal frame yet"):
            ses.step(fr)
        ses.reset([1], goals=goals[1:])
        with pytest.raises(lib.ArpError, match="environment 0 has no goal frame yet"):
            ses.step(fr)
        with pytest.raises(ValueError):
            ses.reset([0], goals=goals[:1, :32])
        with pytest.raises(lib.ArpError, match="goal_feat exists on a session with the device goal reward"):
            ses.read("goal_feat")
        ses.reset([0], goals=goals[:1])
        with pytest.raises(lib.ArpError, match="rewards are refused"):
            ses.step(fr, rewards=[0.0, 0.0])
        for t in range(3):  # the refusals came before any launch: the session goes on
            ses.step(_frames(2, 710 + t))
        assert np.all(ses.read("len") == 3) and np.array_equal(ses.read("goal"), goals)
        ses.close()
        ses = RolloutSession(atr, reward_model=lab, n_envs=2, goal_conditioned=True)
        ses.reset(goals=goals)
        with pytest.raises(lib.ArpError, match="use_crop with the device goal reward is refused"):
            ses.step(fr, use_crop=True)
        with pytest.raises(lib.ArpError, match="owns a reward handle"):
            ses.step(fr, rewards=[0.0, 0.0])
        ses.step(fr)
        assert ses.read("goal_feat").shape == (2, TINY["embed"]) and np.all(np.isfinite(ses.read("rtg")))
        ses.close()
        assert _live(lib) == before  # sessions that were stepped, with and without a reward handle
        # the handles stay usable
        assert np.all(np.isfinite(enc.forward_gc_representations(np.zeros((1, 64, 64, 3), np.float32), np.zeros((1, 64, 64, 3), np.float32))))
        assert np.all(np.isfinite(lab.encode_image(fr)))
    finally:
        lab.close(); bc.close(); atr.close(); aenc.close(); tr.close(); enc.close()


@pytest.mark.parametrize("pkw,pmode,emode", [(P3, "f32", "f32"), (P4, "f16", "f16")])
def test_ring_logic_with_goals(gpu_lib, pkw, pmode, emode):
    """E = 3, every environment its own goal.  Environments 0 and 1 get theirs first: a step is then refused, naming environment 2, which gets its first goal
    after that.  2T + 2 steps; environment 2 is reset again (a plain reset: it keeps its goal) at step 2, environment 0 with a NEW goal at step T + 1.  After
    every step: the ring slot the session wrote is within the encoder's bar of gcbc_oracle on (frame_e, goal_e); the policy batch equals the reference's
    window of the session's own encodings, bitwise; a second GCBC trainer fed those arrays reproduces the session's logits bit for bit."""
    from arp_amd.rollout import RolloutSession
    from arp_amd.train import PolicyTrainer
    enc, tr, pcfg, kw, ocfg, EP, P = _gcbc_stack(SMALL_ENC, pkw, pmode, emode)
    other = PolicyTrainer(pcfg, mode=pmode)
    other.set_params(P)
    E, T = 3, pcfg.window
    goals = _frames(E + 1, 40)  # goals[3]: environment 0's second goal
    cur = [goals[0], goals[1], goals[2]]
    # (CPU) the goals tell the environments apart: swapping two environments' goals moves the tokens by more than 10 x the bar
    f0 = _frames(E, 100)
    swap = np.abs(_gc_ref(EP, ocfg, f0[:2], goals[:2]) - _gc_ref(EP, ocfg, f0[:2], goals[[1, 0]])).max()
    assert swap > 10 * ENC_TOL[emode], swap
    ses = RolloutSession(tr, n_envs=E, goal_conditioned=True)
    orc = [RolloutOracle(T) for _ in range(E)]
    errs = []
    try:
        ses.reset([0, 1], goals=goals[:2])
        with pytest.raises(gpu_lib.ArpError, match="environment 2 has no goal frame yet"):
            ses.step(f0)
        ses.reset([2], goals=goals[2:3])
        for t in range(2 * T + 2):
            if t == 2:
                ses.reset([2]); orc[2].reset()
            if t == T + 1:
                ses.reset([0], goals=goals[3:4]); orc[0].reset(); cur[0] = goals[3]
            assert np.array_equal(ses.read("goal"), np.stack(cur))
            head = int(ses.read("head")[0])
            fr = _frames(E, 100 + t)
            act = ses.step(fr)
            codes = ses.read("enc_ring")[head]  # this step's encodings, as the session holds them
            errs.append(float(np.abs(codes - _gc_ref(EP, ocfg, fr, np.stack(cur))).max()))
            assert errs[-1] < ENC_TOL[emode], (t, errs[-1])
            ew, aw, ln, lg = (ses.read(k) for k in ("enc_window", "action_window", "len", "logits"))
            for e in range(E):
                _, inputs = orc[e].step(codes[e], lambda inp: act[e])
                L, enc_w, act_w, _ = padded(inputs, T, codes[e].shape)
                assert min(int(ln[e]), T) == L
                assert np.array_equal(ew[e], enc_w) and np.array_equal(aw[e], act_w), (t, e)
                assert act[e] == lg[e, L - 1].argmax()
            other.set_batch(ew, aw)
            assert np.array_equal(other.forward()["action_pred"], lg), t
        print(f"GCBC session ring {pmode}/{emode} emb {pcfg.emb}: max encoding err {max(errs):.2e} (bar {ENC_TOL[emode]:.0e}), goal swap moves {swap:.2e}")
        # a later set_lut ingests the goals again: the next step's pairs are (frame, goal) through the NEW table on both sides
        from arp_amd import dataset
        lut2 = dataset.default_lut() * np.float32(0.5)
        ses.set_lut(lut2)
        head, fr = int(ses.read("head")[0]), _frames(E, 190)
        ses.step(fr)
        codes = ses.read("enc_ring")[head]
        new = G.forward_gc_representations(EP, ocfg, dataset.bytes_to_float(fr, lut2), dataset.bytes_to_float(np.stack(cur), lut2))
        stale = G.forward_gc_representations(EP, ocfg, dataset.bytes_to_float(fr, lut2), dataset.bytes_to_float(np.stack(cur)))
        assert np.abs(codes - new).max() < ENC_TOL[emode] and np.abs(new - stale).max() > 10 * ENC_TOL[emode]
    finally:
        ses.close(); other.close(); tr.close(); enc.close()


def test_short_windows_against_fp64(gpu_lib):
    """f32 policy and encoder, E = 1: for t < T - 1 the logits rows 0 .. L - 1 against bc_oracle on the UNPADDED length-L window (config window = L) of gcbc_oracle
    encodings of (frame_t, goal)."""
    from arp_amd.rollout import RolloutSession
    errs = []
    for pkw in (P3, P4):
        enc, tr, pcfg, kw, ocfg, EP, P = _gcbc_stack(SMALL_ENC, pkw, "f32", "f32")
        T = pcfg.window
        ses = RolloutSession(tr, n_envs=1, goal_conditioned=True)
        Pt = {k: torch.from_numpy(v).double() for k, v in P.items()}
        fr, goal = _frames(T - 1, 200), _frames(1, 201)
        try:
            ses.reset(goals=goal)
            for t in range(T - 1):
                ses.step(fr[t:t + 1])
                L = t + 1
                aw, lg = ses.read("action_window")[0, :L], ses.read("logits")[0]
                codes = _gc_ref(EP, ocfg, fr[:L], np.repeat(goal, L, axis=0))
                ref = BO.forward(Pt, BO.PolicyConfig(**{**kw, "window": L}), torch.from_numpy(codes)[None], torch.from_numpy(aw.astype(np.int64))[None])["action_pred"].numpy()[0]
                errs.append(float(np.abs(lg[:L] - ref).max()))
                print(f"GCBC short window emb {pcfg.emb} T {T} L {L}: max logit err {errs[-1]:.2e}")
        finally:
            ses.close(); tr.close(); enc.close()
    assert max(errs) <= BC_LOGITS_BAR_F32, errs


SEED_HOST, QUALIFY_HOST = 6, 6  # policy seed; fp64 decisions (of 2T = 6) whose top-two logit gap exceeds 2 x GCBC_LOGITS_BAR_F16, from a CPU run of the oracles


def test_session_against_the_host_driven_way(gpu_lib):
    """E = 1 at 339-token pairs (one pair: the encoder's latency path), f16, 2T steps.  The host-driven way: a second handle's greedy_action on the reference
    dict {"image": window, "goal": goal tiled over the window, "action": ...}, which encodes all T pairs again (throughput kernels); while the window is
    shorter than T its tail is padded and the logits row L - 1 is read.  Session and host-driven logits both within the f16 bar of fp64, and the actions
    equal fp64's wherever its top-two gap exceeds twice the bar."""
    from arp_amd import dataset
    from arp_amd.rollout import RolloutSession
    from arp_amd.train import PolicyTrainer
    enc, tr, pcfg, kw, ocfg, EP, P = _gcbc_stack(LONG_ENC, P3, "f16", "f16", seed=SEED_HOST)
    host = PolicyTrainer(pcfg, mode="f16")
    host.set_params(P)
    host.attach_encoder(enc)
    T, res = pcfg.window, LONG_ENC["img_res"]
    ses = RolloutSession(tr, n_envs=1, goal_conditioned=True)
    Pt = {k: torch.from_numpy(v).double() for k, v in P.items()}
    goal = _frames(1, 301, res)
    hist_f, hist_c, qualified = [], [], 0
    try:
        ses.reset(goals=goal)
        for t in range(2 * T):
            fr = _frames(1, 310 + t, res)
            enc.profile(True)   # (around the session's pass alone)
            act = ses.step(fr)
            enc.profile(False)
            L = min(t + 1, T)
            aw, lg = ses.read("action_window")[0], ses.read("logits")[0]
            hist_f = (hist_f + [dataset.bytes_to_float(fr[0])])[-T:]
            hist_c = (hist_c + [_gc_ref(EP, ocfg, fr, goal)[0]])[-T:]
            ref = BO.forward(Pt, BO.PolicyConfig(**{**kw, "window": L}), torch.from_numpy(np.stack(hist_c))[None],
                             torch.from_numpy(aw[:L].astype(np.int64))[None])["action_pred"].numpy()[0, L - 1]
            window = np.zeros((1, T, res, res, 3), np.float32)
            window[0, :L] = np.stack(hist_f)
            batch = {"image": {"ob": window}, "goal": {"ob": np.repeat(dataset.bytes_to_float(goal)[None], T, axis=1)}, "action": aw[None]}
            host_act = host.greedy_action(batch)
            host_lg = host.forward()["action_pred"][0, L - 1]
            e_ses, e_host = float(np.abs(lg[L - 1] - ref).max()), float(np.abs(host_lg - ref).max())
            top = np.sort(ref)[::-1]
            print(f"step {t} L {L}: session logits err {e_ses:.2e}, host-driven {e_host:.2e}, fp64 top-two gap {top[0] - top[1]:.2e}")
            assert e_ses <= GCBC_LOGITS_BAR_F16 and e_host <= GCBC_LOGITS_BAR_F16
            if top[0] - top[1] > 2 * GCBC_LOGITS_BAR_F16:
                qualified += 1
                assert act[0] == ref.argmax() and host_lg.argmax() == ref.argmax(), t
                if L == T:
                    assert host_act[0] == ref.argmax()
        assert enc.profile_read().get("m3ae.out_reduce_ln_2", {"calls": 0})["calls"] == 2 * T * LONG_ENC["layers"]  # the session's passes took the latency path
    finally:
        ses.close(); host.close(); tr.close(); enc.close()
    assert qualified >= (3 * 2 * T + 3) // 4 and qualified == QUALIFY_HOST, qualified


@pytest.mark.parametrize("mode", ["f32", "f16"])
def test_goal_reward_on_the_device(gpu_lib, mode):
    """ARP-DT session with a plain labelling handle (conftest's TINY CLIP, no prompt set), E = 2, 6 steps, environment 1 reset to a new goal at step 3; at step 4
    environment 0's frame IS its goal.  reward against fp64 -||f(frame) - f(goal)|| (oracle/clip_np on oracle/preprocess) within 2e-3 x the mean feature norm,
    the bar tests/test_clip_gpu.py::test_online_reward_family_full_vit_b16 holds the host function to; the return-to-go equals rollout_oracle's computed from
    the session's own rewards, bitwise, with use_normalize off and on."""
    from arp_amd import clip, synth
    from arp_amd.rollout import RolloutSession
    from oracle import clip_np as CN, preprocess as PP
    enc, tr, pcfg = _arpdt_stack()
    ocl = CN.ClipConfig(**TINY)
    Wt = synth.clip_weights(ocl, seed=11)
    Wd = CN.cast_weights(Wt, np.float64)
    feat = lambda x: CN.encode_image(Wd, ocl, PP.preprocess(x).astype(np.float64))
    lab = clip.ClipLabeller(clip.ClipConfig(**TINY), Wt, mode=mode)
    E, T, scale = 2, pcfg.window, 10.0
    goals = _frames(3, 50)  # goals[2]: environment 1's second goal
    gfeat = feat(goals)
    try:
        for norm, rmin in ((False, 0.0), (True, -1.75)):
            ses = RolloutSession(tr, reward_model=lab, n_envs=E, return_to_go=50.0, scale=scale, use_normalize=norm, reward_min=rmin, goal_conditioned=True)
            orc = [RolloutOracle(T, 50.0, scale, reward_min=rmin, use_normalize=norm) for _ in range(E)]
            cur = [0, 1]
            try:
                ses.reset(goals=goals[:2])
                for t in range(6):
                    if t == 3:
                        ses.reset([1], goals=goals[2:3]); orc[1].reset(); cur[1] = 2
                    fr = _frames(E, 520 + t)
                    if t == 4:
                        fr[0] = goals[0]
                    ses.step(fr)
                    f = feat(fr)
                    fn = np.linalg.norm(f, axis=1).mean()
                    ref = -np.linalg.norm(f - gfeat[cur], axis=1)
                    rew = ses.read("reward")
                    print(f"{mode} norm {norm} step {t}: reward {rew} fp64 {ref} bar {2e-3 * fn:.2e}")
                    assert np.abs(rew - ref).max() < 2e-3 * fn, (t, rew, ref)
                    for e in range(E):
                        orc[e].apply_reward(rew[e])
                    assert np.array_equal(ses.read("rtg"), np.asarray([o.rtg[0] for o in orc], np.float32)), t
                assert np.abs(ses.read("goal_feat") - gfeat[cur]).max() < 2e-3 * np.linalg.norm(gfeat, axis=1).mean()
                with pytest.raises(gpu_lib.ArpError, match="use_crop with the device goal reward is refused"):
                    ses.step(_frames(E, 530), use_crop=True)
            finally:
                ses.close()
    finally:
        lab.close(); tr.close(); enc.close()
