"""GPU tests of the device-resident rollout session (arp_amd/rollout.py::RolloutSession, arp_amd/csrc/arp_rollout.hip) against the literal restatement of
the reference loop's input handling (tests/rollout_oracle.py): ring logic bitwise, short windows against the fp64 oracles, the whole loop with a CLIP
reward, the reward variants, the decide kernel, and refusals / ownership.

Model BC refuses arp_dt_attach_encoder; its session is handed the encoder (RolloutSession(..., encoder=enc))."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from conftest import TINY
from rollout_oracle import RolloutOracle, padded

pytestmark = pytest.mark.gpu

TINY_ENC = dict(patch=16, width=64, layers=2, heads=2, img_res=64)  # 17 tokens
P3 = dict(emb=64, depth=2, heads=4, window=3, enc_tokens=17, enc_dim=64, lambda_ret=0.5)
P4 = dict(emb=128, depth=2, heads=8, window=4, enc_tokens=17, enc_dim=64, lambda_ret=0.5)  # the fused policy kernel
LOGITS_BAR_F32 = 1e-6   # test_m3ae_gpu.py::test_train_step_with_encoder_inside, f32 logits at this geometry
COS_TOL_F32 = 1e-4      # tests/test_clip_gpu.py: |reward error| / exp(logit_scale), f32


def _frames(n, seed):
    from arp_amd import synth
    return synth.procgen_like_frames(n, 64, 64, seed=seed)


def _stack(pkw, pmode, emode, seed=6):
    from arp_amd import m3ae, synth_policy as S
    from arp_amd.train import PolicyConfig, PolicyTrainer
    from oracle import m3ae_np as M
    ecfg, pcfg = m3ae.EncoderConfig(**TINY_ENC), PolicyConfig(**pkw)
    EP, P = S.m3ae_params(M.EncConfig(**TINY_ENC), seed=5), S.policy_params(pcfg, seed=seed)
    enc = m3ae.M3AEEncoder(ecfg, EP, mode=emode)
    tr = PolicyTrainer(pcfg, mode=pmode)
    tr.set_params(P)
    tr.attach_encoder(enc)
    return enc, tr, pcfg, EP, P


def _live(lib):
    out = (C.c_int64 * 5)()
    lib.check(lib.lib.arp_debug_live(out))
    return list(out)


@pytest.mark.parametrize("pkw,pmode,emode", [(P3, "f32", "f32"), (P4, "f16", "f16")])
def test_ring_logic_is_the_reference_window_bitwise(gpu_lib, pkw, pmode, emode):
    """E = 3, environments reset at steps 0, 0, 2, environment 0 again at step T + 1; 2T + 2 steps.  After every step the policy batch the session built equals
    the reference's window (L real steps at the front, zeros behind) of the session's own per-frame encodings, and a second trainer fed these arrays gives
    the session's logits bit for bit."""
    from arp_amd.rollout import RolloutSession
    from arp_amd.train import PolicyTrainer
    enc, tr, pcfg, EP, P = _stack(pkw, pmode, emode)
    other = PolicyTrainer(pcfg, mode=pmode)
    other.set_params(P)
    E, T = 3, pcfg.window
    ses = RolloutSession(tr, n_envs=E, return_to_go=80.0, scale=100.0)
    rng = np.random.default_rng(3)
    orc = [RolloutOracle(T, 80.0, 100.0) for _ in range(E)]
    orc[2].reset(rtg=0.0)  # never reset before step 2: the state a session is created with
    try:
        ses.reset([0, 1])
        for t in range(2 * T + 2):
            if t == 2:
                ses.reset([2]); orc[2].reset()
            if t == T + 1:
                ses.reset([0], rtg=0.25); orc[0].reset(rtg=0.25)
            head = int(ses.read("head")[0])
            rew = rng.standard_normal(E).astype(np.float32) * 3
            act = ses.step(_frames(E, 100 + t), rewards=rew)
            codes = ses.read("enc_ring")[head]  # this step's encodings, as the session holds them
            ew, aw, rw, ln, lg = (ses.read(k) for k in ("enc_window", "action_window", "rtg_window", "len", "logits"))
            for e in range(E):
                a, inputs = orc[e].step(codes[e], lambda inp: act[e])
                L, enc_w, act_w, rtg_w = padded(inputs, T, codes[e].shape)
                assert min(int(ln[e]), T) == L
                assert np.array_equal(ew[e], enc_w) and np.array_equal(aw[e], act_w) and np.array_equal(rw[e], rtg_w), (t, e)
                assert act[e] == lg[e, L - 1].argmax()
                orc[e].apply_reward(rew[e])
            assert np.array_equal(ses.read("rtg"), np.asarray([o.rtg[0] for o in orc], np.float32))
            other.set_batch(ew, aw, rw[..., None])
            assert np.array_equal(other.forward()["action_pred"], lg), t
    finally:
        ses.close(); other.close(); tr.close(); enc.close()


def test_short_windows_against_the_fp64_oracles(gpu_lib):
    """f32 policy and encoder: for t < T - 1 the logits row L - 1 against oracle/arpdt_torch.py on the UNPADDED length-L window (config window = L) behind
    oracle/m3ae_np.py encodings."""
    import torch
    from arp_amd import dataset
    from arp_amd.rollout import RolloutSession
    from oracle import arpdt_torch as O, m3ae_np as M
    errs = []
    for pkw in (P3, P4):
        enc, tr, pcfg, EP, P = _stack(pkw, "f32", "f32")
        T = pcfg.window
        ses = RolloutSession(tr, n_envs=1, return_to_go=60.0, scale=100.0)
        Pt = {k: torch.from_numpy(v).double() for k, v in P.items()}
        fr = _frames(T - 1, 200)
        try:
            ses.reset()
            for t in range(T - 1):
                ses.step(fr[t:t + 1], rewards=[1.5])
                L = t + 1
                aw, rw, lg = ses.read("action_window")[0, :L], ses.read("rtg_window")[0, :L], ses.read("logits")[0]
                codes = M.forward_representation(EP, M.EncConfig(**TINY_ENC), dataset.bytes_to_float(fr[:L]))
                ocfg = O.PolicyConfig(**{**{f.name: getattr(pcfg, f.name) for f in dataclasses.fields(O.PolicyConfig) if hasattr(pcfg, f.name)}, "window": L})
                ref = O.forward(Pt, ocfg, torch.from_numpy(np.asarray(codes, np.float64))[None], torch.from_numpy(aw.astype(np.int64))[None],
                                torch.from_numpy(rw.astype(np.float64))[None, :, None])["action_pred"].numpy()[0]
                errs.append(float(np.abs(lg[:L] - ref).max()))
                print(f"short window emb {pcfg.emb} T {T} L {L}: max logit err {errs[-1]:.2e}")
        finally:
            ses.close(); tr.close(); enc.close()
    assert max(errs) < LOGITS_BAR_F32, errs


@pytest.mark.parametrize("pkw,pmode,emode", [(P3, "f32", "f32"), (P4, "f16", "f16")])
def test_the_padded_tail_does_not_reach_the_real_positions(gpu_lib, pkw, pmode, emode):
    """The same frames through a session whose padded tail holds large finite junk (encodings, return-to-go, a non-zero action): logits at the real positions
    are bitwise those of the zero tail."""
    from arp_amd.rollout import RolloutSession
    enc, tr, pcfg, EP, P = _stack(pkw, pmode, emode)
    T = pcfg.window
    a, b = RolloutSession(tr, n_envs=2), RolloutSession(tr, n_envs=2)
    b._debug_set_tail(37.5, pcfg.n_actions - 1)
    try:
        a.reset(); b.reset()
        for t in range(T + 1):
            fr = _frames(2, 300 + t)
            aa, ab = a.step(fr, rewards=[0.5, 2.0]), None
            la, wa = a.read("logits"), a.read("enc_window")  # (read before b steps: both sessions fill the same batch slot of the policy handle)
            ab = b.step(fr, rewards=[0.5, 2.0])
            lb, wb = b.read("logits"), b.read("enc_window")
            L = min(t + 1, T)
            assert np.array_equal(la[:, :L], lb[:, :L]) and np.array_equal(aa, ab), t
            assert np.array_equal(wa[:, :L], wb[:, :L])
            if L < T:
                assert np.all(wb[:, L:] == 37.5) and np.all(wa[:, L:] == 0) and not np.array_equal(la[:, L:], lb[:, L:])
    finally:
        a.close(); b.close(); tr.close(); enc.close()


SEED_LOOP, QUALIFY_LOOP = 6, 20  # policy seed; decisions of the fp64 oracle whose top-two gap exceeds 2 x LOGITS_BAR_F32 (all 20; checked on the CPU)


def test_whole_loop_with_a_clip_reward(gpu_lib):
    """10 steps, E = 2, f32, a tiny CLIP as the reward model (64 x 64 frames resized by the labeller): actions and return-to-go after every step against
    rollout_oracle driven by fp64 policy logits (oracle/m3ae_np.py -> oracle/arpdt_torch.py) and ClipLabeller.label on the same frames."""
    import torch
    from arp_amd import clip, dataset, synth
    from arp_amd.rollout import RolloutSession
    from oracle import arpdt_torch as O, clip_np as CN, m3ae_np as M
    enc, tr, pcfg, EP, P = _stack(P3, "f32", "f32", seed=SEED_LOOP)
    ocl = CN.ClipConfig(**TINY)
    Wt = synth.clip_weights(ocl, seed=11)
    tok = synth.prompt_tokens(2, [7, 3], ctx=ocl.ctx, vocab=ocl.vocab, seed=13)
    lab = clip.ClipLabeller(clip.ClipConfig(**TINY), Wt, mode="f32").set_text(tok)
    clip_scale = float(np.exp(Wt["logit_scale"]))
    E, T, steps, scale = 2, pcfg.window, 10, 100.0
    ses = RolloutSession(tr, reward_model=lab, n_envs=E, return_to_go=100.0, scale=scale)
    Pt = {k: torch.from_numpy(v).double() for k, v in P.items()}
    fields = {f.name: getattr(pcfg, f.name) for f in dataclasses.fields(O.PolicyConfig) if hasattr(pcfg, f.name)}
    gaps = []

    def policy_fn(inputs):
        L = inputs["action"].shape[1]
        out = O.forward(Pt, O.PolicyConfig(**{**fields, "window": L}), torch.from_numpy(np.asarray(inputs["image"], np.float64)),
                        torch.from_numpy(inputs["action"].astype(np.int64)), torch.from_numpy(inputs["rtg"].astype(np.float64)))["action_pred"].numpy()[0, L - 1]
        top = np.sort(out)[::-1]
        gaps.append(float(top[0] - top[1]))
        return int(out.argmax())
    orc = [RolloutOracle(T, 100.0, scale) for _ in range(E)]
    qualified = 0
    try:
        ses.reset()
        for t in range(steps):
            fr = _frames(E, 400 + t)
            r = lab.label(fr)
            act = ses.step(fr)
            codes = M.forward_representation(EP, M.EncConfig(**TINY_ENC), dataset.bytes_to_float(fr))
            for e in range(E):
                a, _ = orc[e].step(codes[e], policy_fn)
                if gaps[-1] > 2 * LOGITS_BAR_F32:
                    qualified += 1
                    assert act[e] == a, (t, e, gaps[-1])
                orc[e].apply_reward(r[e])
            got, ref = ses.read("rtg"), np.asarray([o.rtg[0] for o in orc])
            bar = (t + 1) * COS_TOL_F32 * clip_scale / scale
            print(f"step {t}: rtg {got} oracle {ref} bar {bar:.2e} reward {ses.read('reward')} label {r}")
            assert np.abs(got - ref).max() <= bar
    finally:
        ses.close(); lab.close(); tr.close(); enc.close()
    assert qualified >= 8 and qualified == QUALIFY_LOOP, qualified


def test_reward_variants(gpu_lib):
    from arp_amd.rollout import RolloutSession
    from arp_amd.train import PolicyConfig, PolicyTrainer
    enc, tr, pcfg, EP, P = _stack(P3, "f32", "f32")
    rng = np.random.default_rng(9)
    try:
        for norm, rmin in ((False, 0.0), (True, -1.75)):
            ses = RolloutSession(tr, n_envs=2, return_to_go=50.0, scale=10.0, use_normalize=norm, reward_min=rmin)
            orc = [RolloutOracle(pcfg.window, 50.0, 10.0, reward_min=rmin, use_normalize=norm) for _ in range(2)]
            ses.reset()
            for t in range(5):
                rew = (rng.standard_normal(2) * 4).astype(np.float32)
                ses.step(_frames(2, 500 + t), rewards=rew)
                for e in range(2):
                    orc[e].apply_reward(rew[e])
                assert np.array_equal(ses.read("rtg"), np.asarray([o.rtg[0] for o in orc], np.float32)) and np.array_equal(ses.read("reward"), rew)
            ses.close()
        ses = RolloutSession(tr, n_envs=2, return_to_go=50.0, scale=10.0)  # no reward source: the return-to-go stays constant
        ses.reset()
        for t in range(4):
            ses.step(_frames(2, 600 + t))
            assert np.array_equal(ses.read("rtg"), np.full(2, 5.0, np.float32)) and np.array_equal(ses.read("rtg_window")[:, :min(t + 1, 3)], np.full((2, min(t + 1, 3)), 5.0, np.float32))
        ses.close()
    finally:
        tr.close(); enc.close()


BC_LOGITS_BAR_F32 = 2e-5  # tests/test_bc_gpu.py::test_f32_forward_and_gradients_match_oracle: f32 BC logits against the fp64 oracle


@pytest.mark.parametrize("pkw", [P3, P4])
def test_bc_policy_runs_through_the_session(gpu_lib, pkw):
    """PolicyConfig(model="BC"): 6 steps, E = 2, f32.  The windows are the reference's (rollout_oracle on the session's own encodings, bitwise; no
    return-to-go), the logits at the real positions are those of tests/bc_oracle.py on the UNPADDED window behind oracle/m3ae_np.py encodings, the action is
    the argmax of row L - 1, and every reward option is refused."""
    import torch
    import bc_oracle as BO
    from arp_amd import clip, dataset, m3ae, synth, synth_policy as S
    from arp_amd.rollout import RolloutSession
    from arp_amd.train import PolicyConfig, PolicyTrainer
    from oracle import clip_np as CN, m3ae_np as M
    lib = gpu_lib
    kw = {k: v for k, v in pkw.items() if k != "lambda_ret"}
    pcfg = PolicyConfig(**kw, model="BC")
    P = S.policy_params(pcfg, seed=6)
    EP = S.m3ae_params(M.EncConfig(**TINY_ENC), seed=5)
    enc = m3ae.M3AEEncoder(m3ae.EncoderConfig(**TINY_ENC), EP, mode="f32")
    tr = PolicyTrainer(pcfg, mode="f32")
    tr.set_params(P)
    with pytest.raises(lib.ArpError):
        tr.attach_encoder(enc)  # the handle's refusal stands
    Pt = {k: torch.from_numpy(v).double() for k, v in P.items()}
    E, T = 2, pcfg.window
    ocl = CN.ClipConfig(**TINY)
    lab = clip.ClipLabeller(clip.ClipConfig(**TINY), synth.clip_weights(ocl, seed=11), mode="f32").set_text(synth.prompt_tokens(1, 5, ctx=ocl.ctx, vocab=ocl.vocab, seed=2))
    errs = []
    try:
        before = _live(lib)
        with pytest.raises(lib.ArpError, match="pass one to arp_rollout_create_with_encoder"):
            RolloutSession(tr, n_envs=E)
        with pytest.raises(lib.ArpError, match="a reward handle is refused"):
            RolloutSession(tr, reward_model=lab, n_envs=E, encoder=enc)
        with pytest.raises(lib.ArpError, match="set_reward_norm is refused"):
            RolloutSession(tr, n_envs=E, encoder=enc, use_normalize=True, reward_min=-1.0)
        assert _live(lib) == before
        ses = RolloutSession(tr, n_envs=E, encoder=enc)
        orc = [RolloutOracle(T) for _ in range(E)]
        ses.reset()
        for t in range(6):
            fr = _frames(E, 800 + t)
            head = int(ses.read("head")[0])
            act = ses.step(fr)
            codes = ses.read("enc_ring")[head]
            ew, aw, lg = ses.read("enc_window"), ses.read("action_window"), ses.read("logits")
            ref_codes = M.forward_representation(EP, M.EncConfig(**TINY_ENC), dataset.bytes_to_float(fr))
            for e in range(E):
                _, inputs = orc[e].step(codes[e], lambda inp: act[e])
                L, enc_w, act_w, _ = padded(inputs, T, codes[e].shape)
                assert np.array_equal(ew[e], enc_w) and np.array_equal(aw[e], act_w) and act[e] == lg[e, L - 1].argmax(), (t, e)
                hist = getattr(orc[e], "ref_hist", []) + [ref_codes[e]]
                orc[e].ref_hist = hist[-T:]
                ref = BO.forward(Pt, BO.PolicyConfig(**{**kw, "window": L}), torch.from_numpy(np.asarray(orc[e].ref_hist, np.float64))[None],
                                 torch.from_numpy(act_w[:L].astype(np.int64))[None])["action_pred"].numpy()[0]
                errs.append(float(np.abs(lg[e, :L] - ref).max()))
        print(f"BC session emb {pcfg.emb} window {T}: max logit err over 6 steps {max(errs):.2e}")
        assert max(errs) <= BC_LOGITS_BAR_F32, errs
        with pytest.raises(lib.ArpError, match="rewards are refused"):
            ses.step(_frames(E, 900), rewards=[0.0, 0.0])
        with pytest.raises(lib.ArpError, match="set_reward_norm is refused"):
            ses.set_reward_norm(True, 0.5)
        with pytest.raises(lib.ArpError, match="no return-to-go"):
            ses.read("rtg_window")
        ses.step(_frames(E, 901))  # the refusals came before any launch: the session goes on
        ses.close()
    finally:
        lab.close(); tr.close(); enc.close()


def _decide(lib, logits, lens):
    lg = np.require(np.asarray(logits, np.float32), requirements="C")
    E, T, NA = lg.shape
    ln = np.require(np.asarray(lens, np.int32), requirements="C")
    out = np.full(E, -1, np.int32)
    lib.check(lib.lib.arp_op_rollout_decide(lib.as_ptr(lg, C.c_float), lib.as_ptr(ln, C.c_int32), E, T, NA, lib.as_ptr(out, C.c_int32)))
    return out


def test_op_rollout_decide(gpu_lib):
    rng = np.random.default_rng(1)
    E, T, NA = 70, 4, 15  # more than one block of 64 environments
    lg = rng.standard_normal((E, T, NA)).astype(np.float32)
    lens = rng.integers(1, T + 1, E)
    lens[:4] = [1, 2, 3, 4]
    for e in range(E):  # the other rows hold a larger decoy
        for j in range(T):
            if j != lens[e] - 1:
                lg[e, j, (e + j) % NA] = 100.0
    lg[0, 0, [3, 7, 9]] = 50.0                       # ties -> the lowest index
    lg[1, 1] = 0.0; lg[1, 1, 4] = -0.0              # -0.0 against 0.0: the first
    lg[2, 2] = -0.0; lg[2, 2, 5] = 0.0
    lg[3, 3, 6] = np.nan; lg[3, 3, 11] = np.nan; lg[3, 3, 2] = 1e30   # the first NaN wins
    lg[4, lens[4] - 1, 0] = np.nan
    lg[5, lens[5] - 1] = -np.inf
    want = np.asarray([lg[e, lens[e] - 1].argmax() for e in range(E)], np.int32)
    assert want[0] == 3 and want[1] == 0 and want[2] == 0 and want[3] == 6 and want[4] == 0 and want[5] == 0
    assert np.array_equal(_decide(gpu_lib, lg, lens), want)
    one = rng.standard_normal((3, 2, 1)).astype(np.float32)
    assert np.array_equal(_decide(gpu_lib, one, [1, 2, 2]), np.zeros(3, np.int32))  # n_actions = 1
    with pytest.raises(gpu_lib.ArpError, match="window lengths"):
        _decide(gpu_lib, one, [0, 1, 1])


def test_refusals_and_ownership(gpu_lib):
    from arp_amd import clip, m3ae, synth, synth_policy as S
    from arp_amd.rollout import RolloutSession
    from arp_amd.train import PolicyConfig, PolicyTrainer
    from oracle import clip_np as CN
    lib = gpu_lib
    enc, tr, pcfg, EP, P = _stack(P3, "f32", "f32")
    ocl = CN.ClipConfig(**TINY)
    lab = clip.ClipLabeller(clip.ClipConfig(**TINY), synth.clip_weights(ocl, seed=11), mode="f32").set_text(synth.prompt_tokens(1, 5, ctx=ocl.ctx, vocab=ocl.vocab, seed=2))
    bare = PolicyTrainer(pcfg, mode="f32")
    bare.set_params(P)
    fr = _frames(2, 700)
    # every handle's lazily sized workspace at the session's shapes (2 frames, B = 2) before the counters are read
    warm = RolloutSession(tr, reward_model=lab, n_envs=2)
    warm.reset()
    for t in range(4):
        warm.step(fr)
    warm.close()
    lab.label(fr)
    try:
        before = _live(lib)
        h = C.c_void_p()
        assert lib.lib.arp_rollout_create(tr._h, None, 2, 32, 64, 100.0, C.byref(h)) < 0 and "the attached encoder reads 64 x 64" in lib.last_error()
        assert lib.lib.arp_rollout_create(tr._h, None, 0, 64, 64, 100.0, C.byref(h)) < 0 and "n_envs" in lib.last_error()
        with pytest.raises(lib.ArpError, match="no frozen encoder attached"):
            RolloutSession(bare, n_envs=1)
        assert _live(lib) == before  # a refused create holds nothing
        ses = RolloutSession(tr, reward_model=lab, n_envs=2)
        with pytest.raises(lib.ArpError, match="step before the first reset"):
            ses.step(fr)
        with pytest.raises(lib.ArpError, match="env_id 2 out of range"):
            ses.reset([0, 2])
        with pytest.raises(lib.ArpError, match="env_id -1 out of range"):
            ses.reset([-1])
        with pytest.raises(lib.ArpError, match="owns a reward handle"):
            ses.reset(); ses.step(fr, rewards=[0.0, 0.0])
        with pytest.raises(ValueError):
            ses.step(fr[:, :32])
        for t in range(3):
            ses.step(_frames(2, 710 + t))
        assert np.all(ses.read("len") == 3) and np.all(np.isfinite(ses.read("rtg")))
        ses.close()
        assert _live(lib) == before  # a session that was stepped, with a reward handle
        # the policy, encoder and CLIP handles stay usable
        codes = enc.forward_representation(np.zeros((3, 64, 64, 3), np.float32))[None]
        tr.set_batch(codes, np.zeros((1, 3), np.int32), np.zeros((1, 3, 1), np.float32))
        assert np.all(np.isfinite(tr.forward()["action_pred"])) and np.all(np.isfinite(lab.label(fr)))
    finally:
        bare.close(); lab.close(); tr.close(); enc.close()
