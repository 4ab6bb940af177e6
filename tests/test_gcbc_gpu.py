"""Model GCBC (arp_dt/GCBC.py) through the policy step: BC's policy behind the frozen encoder's goal-conditioned call.

GCBC == BC bit for bit with encodings in; frames + goals in == the encoder's own gc output fed as encodings (as
tests/test_m3ae_gpu.py::test_train_step_with_encoder_inside compares the ARP-DT pair, 1e-6); logits against float64 (tests/bc_oracle.py on
tests/gcbc_oracle.py's encodings: f32 at tests/test_bc_gpu.py's 2e-5, f16 at the toy-geometry bar of tests/test_policy_gpu.py, 1.5e-3); the reference's batch
dict {"image", "goal", "action"} through create_train_step and greedy_action; what the model refuses; and the live-resource counters."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import bc_oracle as BO
import gcbc_oracle as G

pytestmark = pytest.mark.gpu
SMALL_ENC = dict(patch=16, width=128, layers=2, heads=2, img_res=64)    # P = 16: 33 tokens per pair
LONG_ENC = dict(patch=16, width=128, layers=2, heads=2, img_res=208)    # P = 169: 339 tokens, the key-blocked attention


def _pair(enc_kw, window, B, seed=5):
    from arp_amd import m3ae, synth_policy as S
    from arp_amd.train import PolicyConfig
    from oracle import m3ae_np as M
    ecfg, ocfg = m3ae.EncoderConfig(**enc_kw), M.EncConfig(**enc_kw)
    kw = dict(emb=64, depth=2, heads=4, window=window, enc_tokens=ecfg.gc_tokens, enc_dim=ecfg.width)
    pcfg = PolicyConfig(**kw, model="GCBC")
    EP, P = S.m3ae_params(ocfg, seed=seed), S.policy_params(pcfg, seed=seed + 1)
    r = ecfg.img_res
    frames = S.normalized_frames(B * window, r, seed=seed + 2).reshape(B, window, r, r, 3)
    goals = S.normalized_frames(B * window, r, seed=seed + 3).reshape(B, window, r, r, 3)
    act = np.random.default_rng(seed).integers(0, pcfg.n_actions, (B, window)).astype(np.int32)
    return ecfg, ocfg, kw, pcfg, EP, P, frames, goals, act


def test_gcbc_is_bc_with_encodings_in(gpu_lib):
    """same parameters, same encodings: forward, one train step and the parameters after it, bit for bit"""
    from arp_amd import synth_policy as S
    from arp_amd.train import PolicyConfig, PolicyTrainer
    kw = dict(emb=64, depth=2, heads=4, window=3, enc_tokens=33, enc_dim=128)
    for mode in ("f32", "f16"):
        res = []
        for model in ("BC", "GCBC"):
            cfg = PolicyConfig(**kw, model=model)
            P = S.policy_params(PolicyConfig(**kw, model="BC"), seed=3)
            enc, act, _ = S.policy_batch(cfg, 3, seed=4)
            tr = PolicyTrainer(cfg, mode=mode)
            assert set(tr.shapes) == set(BO.param_shapes(BO.PolicyConfig(**kw)))
            tr.set_params(P)
            tr.set_batch(enc, act)
            out = tr.forward()
            assert set(out) == {"action_pred", "loss", "acc"}
            aux = tr.train_step(1e-3)
            res.append((out, aux, tr.get_params()))
            tr.close()
        (oa, xa, pa), (ob, xb, pb) = res
        assert (oa["action_pred"].view(np.uint32) == ob["action_pred"].view(np.uint32)).all() and oa["loss"] == ob["loss"] and oa["acc"] == ob["acc"]
        assert xa == xb, (xa, xb)
        assert all((pa[k].view(np.uint32) == pb[k].view(np.uint32)).all() for k in pa)


@pytest.mark.parametrize("enc_kw,window,B", [(SMALL_ENC, 3, 3), (LONG_ENC, 2, 2)], ids=["N33", "N339"])
def test_frames_and_goals_in_equal_encodings_in(gpu_lib, enc_kw, window, B):
    from arp_amd import m3ae
    from arp_amd.train import PolicyTrainer
    ecfg, _, _, pcfg, EP, P, frames, goals, act = _pair(enc_kw, window, B)
    r = ecfg.img_res
    enc = m3ae.M3AEEncoder(ecfg, EP, mode="f32")
    codes = enc.forward_gc_representations(frames.reshape(-1, r, r, 3), goals.reshape(-1, r, r, 3)).reshape(B, window, ecfg.gc_tokens, ecfg.width)
    a = PolicyTrainer(pcfg, mode="f32"); a.set_params(P); a.set_batch(codes, act)
    b = PolicyTrainer(pcfg, mode="f32"); b.set_params(P); b.attach_encoder(enc); b.set_batch_images(frames, act, goals=goals)
    fa, fb = a.forward(), b.forward()
    assert np.abs(fa["action_pred"] - fb["action_pred"]).max() < 1e-6
    xa, xb = a.train_step(1e-3), b.train_step(1e-3)
    assert abs(xa["loss"] - xb["loss"]) < 1e-6 and abs(xa["grad_norm"] - xb["grad_norm"]) < 1e-6
    pa, pb = a.get_params(), b.get_params()
    assert max(np.abs(pa[k] - pb[k]).max() for k in pa) < 1e-6
    a.close(); b.close(); enc.close()


@pytest.mark.parametrize("mode,tol", [("f32", 2e-5), ("f16", 1.5e-3)])
def test_gcbc_logits_against_float64(gpu_lib, mode, tol):
    """frames + goals in, against bc_oracle.forward on the gc oracle's encodings (f16: the f16 policy behind the f16 encoder).
    The f32 bar is tests/test_bc_gpu.py's (2e-5).  The f16 bar departs from the issue's wording: it names "tests/test_bc_gpu.py's toy-geometry bar", and that
    file has no f16 bar at a toy geometry (its only f16 bar is 1e-3 at the real one).  The bar used is the project's f16 bar for toy geometries,
    tests/test_policy_gpu.py::test_forward_parity's 1.5e-3 (64 .. 128-term contractions average the operand roundings less than the real geometry's) -- set
    before the first run, which read 1.13e-3."""
    from arp_amd import m3ae
    from arp_amd.train import PolicyTrainer
    ecfg, ocfg, kw, pcfg, EP, P, frames, goals, act = _pair(SMALL_ENC, 3, 3)
    r = ecfg.img_res
    codes = G.forward_gc_representations(EP, ocfg, frames.reshape(-1, r, r, 3), goals.reshape(-1, r, r, 3)).reshape(3, 3, ecfg.gc_tokens, ecfg.width)
    ref = BO.forward({k: torch.from_numpy(v).double() for k, v in P.items()}, BO.PolicyConfig(**kw), torch.from_numpy(codes), torch.from_numpy(act).long())
    enc = m3ae.M3AEEncoder(ecfg, EP, mode=mode)
    tr = PolicyTrainer(pcfg, mode=mode)
    tr.set_params(P); tr.attach_encoder(enc); tr.set_batch_images(frames, act, goals=goals)
    out = tr.forward()
    e = float(np.abs(out["action_pred"] - ref["action_pred"].numpy()).max())
    print(f"GCBC {mode} logits err {e:.2e}")
    assert e <= tol, e
    if mode == "f32":
        assert abs(out["loss"] - float(ref["loss"])) <= 1e-5
    tr.close(); enc.close()


def test_reference_batch_dict_through_the_step_functions(gpu_lib):
    """{"image": {...}, "goal": {...}, "action": ...} through create_train_step and greedy_action reproduces the explicit calls"""
    from arp_amd import m3ae
    from arp_amd.train import PolicyTrainer, TrainState, create_train_step
    ecfg, _, _, pcfg, EP, P, frames, goals, act = _pair(SMALL_ENC, 3, 3)
    enc = m3ae.M3AEEncoder(ecfg, EP, mode="f32")
    batch = {"image": {"ob": frames}, "goal": {"ob": goals}, "action": act}
    a = PolicyTrainer(pcfg, mode="f32"); a.set_params(P); a.attach_encoder(enc)
    a.set_batch_images(frames, act, goals=goals)
    want_action = a.forward()["action_pred"][:, -1, :].argmax(-1)
    want = a.train_step(1e-3)
    pa = a.get_params()
    b = PolicyTrainer(pcfg, mode="f32"); b.set_params(P); b.attach_encoder(enc)
    assert (b.greedy_action(batch) == want_action).all()
    fn = create_train_step(pcfg, lambda s: 1e-3, pcfg.weight_decay)
    _, aux, _ = fn(TrainState(b), batch, None)
    assert aux["loss"] == want["loss"] and aux["grad_norm"] == want["grad_norm"]
    pb = b.get_params()
    assert all((pa[k].view(np.uint32) == pb[k].view(np.uint32)).all() for k in pa)
    a.close(); b.close(); enc.close()


def test_what_gcbc_refuses(gpu_lib):
    from arp_amd import m3ae, rollout
    from arp_amd.train import PolicyConfig, PolicyTrainer
    ecfg, _, kw, pcfg, EP, P, frames, goals, act = _pair(SMALL_ENC, 3, 3)
    enc = m3ae.M3AEEncoder(ecfg, EP, mode="f32")
    Err = gpu_lib.ArpError
    with pytest.raises(ValueError, match="2 P \\+ 1"):
        PolicyConfig(**{**kw, "enc_tokens": ecfg.tokens}, model="GCBC")   # P + 1 = 17 is no pair's token count
    wrong = PolicyTrainer(PolicyConfig(**{**kw, "enc_tokens": 19}, model="GCBC"), mode="f32")   # a pair of 3 x 3 grids; this encoder's pairs are 33 tokens
    with pytest.raises(Err, match="encoder geometry does not match"):
        wrong.attach_encoder(enc)
    wrong.close()
    bc = PolicyTrainer(PolicyConfig(**kw, model="BC"), mode="f32")
    with pytest.raises(Err, match="model BC takes encodings"):
        bc.attach_encoder(enc)
    bc.close()
    tr = PolicyTrainer(pcfg, mode="f32"); tr.set_params(P); tr.attach_encoder(enc)
    with pytest.raises(Err, match="goal batches exist in the synchronous slot only"):
        tr.upload_async(0, frames, act, images=True, goals=goals)
    with pytest.raises(Err, match="synchronous slot only"):
        tr.upload_async(0, frames, act, images=True)
    with pytest.raises(Err, match="no encode-ahead"):
        tr.encode_ahead(2)
    with pytest.raises(Err, match="goal frame per episode"):
        rollout.RolloutSession(tr, n_envs=1)
    with pytest.raises(Err, match="needs goals="):
        tr.set_batch_images(frames, act, np.zeros((3, 3, 1), np.float32))
    rc = gpu_lib.lib.arp_dt_set_batch_images(tr._h, frames.ctypes.data_as(C.POINTER(C.c_float)), act.ctypes.data_as(C.POINTER(C.c_int32)),
                                             np.zeros(9, np.float32).ctypes.data_as(C.POINTER(C.c_float)), 3)
    assert rc != 0 and "arp_dt_set_batch_images_goal" in gpu_lib.last_error()
    tr.set_batch_images(frames, act, goals=goals)   # and the handle still works
    assert np.isfinite(tr.forward()["loss"])
    tr.close(); enc.close()


def test_gcbc_handles_release_what_they_took(gpu_lib):
    from arp_amd import m3ae
    from arp_amd.train import PolicyTrainer

    def live():
        out = (C.c_int64 * 5)()
        gpu_lib.check(gpu_lib.lib.arp_debug_live(out))
        return list(out)
    ecfg, _, _, pcfg, EP, P, frames, goals, act = _pair(SMALL_ENC, 3, 3)
    gc.collect()
    before = live()
    enc = m3ae.M3AEEncoder(ecfg, EP, mode="f16")
    tr = PolicyTrainer(pcfg, mode="f16"); tr.set_params(P); tr.attach_encoder(enc)
    tr.set_batch_images(frames, act, goals=goals)
    tr.train_step(1e-3)
    tr.close(); enc.close()
    assert live() == before
