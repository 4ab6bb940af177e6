"""InstructRL (PolicyConfig(model="BC")) with frames in: the frozen M3AE encoder's image + text pass inside the policy step
(arp_dt_attach_text_encoder, PolicyTrainer.attach_encoder(enc, instruct=...)), through the one stager every batch kind goes through.

Small geometry: the encoder of tests/test_text_encoder_gpu.py (patch 16, width 128, 2 layers, 2 heads, 64 x 64 frames) with L = 13 and 5 valid tokens:
30 encoder tokens per frame.  A BC trainer fed enc.forward_representation(frames, text, mask) as encodings is the yardstick for the trainer that encodes
the frames itself; tests/bc_oracle.py on tests/instructrl_oracle.py's float64 encodings is the yardstick for the 16-bit logits.

The rollout session with the instruction (arp_rollout_create_text, RolloutSession(instruct=...)) is checked against the host-driven greedy_action on the
same windows."""
import numpy as np
import pytest
import torch

import bc_oracle as BO
import instructrl_oracle as I
from test_dataset_gpu import BATCHES, T, _data
from test_text_encoder_gpu import SMALL, VOCAB, _instruction

pytestmark = pytest.mark.gpu
L, VALID = 13, 5


def _setup(window=3, B=3, seed=5):
    from arp_amd import m3ae, synth_policy as S
    from arp_amd.train import PolicyConfig
    from oracle import m3ae_np as M
    ecfg, ocfg = m3ae.EncoderConfig(**SMALL), M.EncConfig(**SMALL)
    kw = dict(emb=64, depth=2, heads=4, window=window, enc_tokens=ecfg.text_tokens(L), enc_dim=ecfg.width)
    pcfg = PolicyConfig(**kw, model="BC")
    EP = S.add_m3ae_text_params(S.m3ae_params(ocfg, seed=seed), ocfg, vocab=VOCAB, seed=seed)
    P = S.policy_params(pcfg, seed=seed + 1)
    r = ecfg.img_res
    frames = S.normalized_frames(B * window, r, seed=seed + 2).reshape(B, window, r, r, 3)
    act = np.random.default_rng(seed).integers(0, pcfg.n_actions, (B, window)).astype(np.int32)
    tok, mask = _instruction(L, VALID, seed + 3)
    return ecfg, ocfg, kw, pcfg, EP, P, frames, act, tok, mask


def test_frames_in_equal_encodings_in(gpu_lib):
    """f32: logits within 1e-6, and the same three-step trajectory (loss, gradient norm, parameters) at tests/test_gcbc_gpu.py's 1e-6"""
    from arp_amd import m3ae
    from arp_amd.train import PolicyTrainer
    ecfg, _, _, pcfg, EP, P, frames, act, tok, mask = _setup()
    B, W, r = frames.shape[0], frames.shape[1], ecfg.img_res
    enc = m3ae.M3AEEncoder(ecfg, EP, mode="f32")
    codes = enc.forward_representation(frames.reshape(-1, r, r, 3), tok, mask).reshape(B, W, ecfg.text_tokens(L), ecfg.width)
    a = PolicyTrainer(pcfg, mode="f32"); a.set_params(P)
    b = PolicyTrainer(pcfg, mode="f32"); b.set_params(P); b.attach_encoder(enc, instruct=tok, text_padding_mask=mask)
    a.set_batch(codes, act); b.set_batch_images(frames, act)
    fa, fb = a.forward(), b.forward()
    assert np.abs(fa["action_pred"] - fb["action_pred"]).max() < 1e-6
    for _ in range(3):
        a.set_batch(codes, act); b.set_batch_images(frames, act)
        xa, xb = a.train_step(1e-3), b.train_step(1e-3)
        assert abs(xa["loss"] - xb["loss"]) < 1e-6 and abs(xa["grad_norm"] - xb["grad_norm"]) < 1e-6
    pa, pb = a.get_params(), b.get_params()
    assert max(np.abs(pa[k] - pb[k]).max() for k in pa) < 1e-6
    # the instruction is what the step encodes with: another one gives other logits
    other = PolicyTrainer(pcfg, mode="f32"); other.set_params(P); other.attach_encoder(enc, instruct=(tok + 1) % VOCAB, text_padding_mask=mask)
    other.set_batch_images(frames, act)
    assert np.abs(other.forward()["action_pred"] - fa["action_pred"]).max() > 1e-4
    a.close(); b.close(); other.close(); enc.close()


@pytest.mark.parametrize("mode,tol", [("f32", 2e-5), ("f16", 1.5e-3), ("bf16", 3e-2)])
def test_logits_against_float64(gpu_lib, mode, tol):
    """frames in, against bc_oracle.forward on the float64 encodings of tests/instructrl_oracle.py.  Bars: tests/test_gcbc_gpu.py's for its equivalent
    (f32 2e-5, f16 1.5e-3); bf16 is not in that file: tests/test_policy_gpu.py::test_forward_parity's 3e-2, the project's bf16 bar for toy geometries."""
    from arp_amd import m3ae
    from arp_amd.train import PolicyTrainer
    ecfg, ocfg, kw, pcfg, EP, P, frames, act, tok, mask = _setup()
    r = ecfg.img_res
    codes = I.forward_representation(EP, ocfg, frames.reshape(-1, r, r, 3), tok, mask).reshape(3, 3, ecfg.text_tokens(L), ecfg.width)
    ref = BO.forward({k: torch.from_numpy(v).double() for k, v in P.items()}, BO.PolicyConfig(**kw), torch.from_numpy(codes), torch.from_numpy(act).long())
    enc = m3ae.M3AEEncoder(ecfg, EP, mode=mode)
    tr = PolicyTrainer(pcfg, mode=mode)
    tr.set_params(P); tr.attach_encoder(enc, instruct=tok[None], text_padding_mask=mask[None]); tr.set_batch_images(frames, act)
    out = tr.forward()
    e = float(np.abs(out["action_pred"] - ref["action_pred"].numpy()).max())
    print(f"InstructRL frames in, {mode}: logits err {e:.2e}")
    assert e <= tol, e
    tr.close(); enc.close()


@pytest.mark.parametrize("mode", ["f32", "f16"])
def test_prefetched_frames_equal_the_synchronous_slot_bitwise(gpu_lib, monkeypatch, mode):
    """prefetch_to_device (frames into slots 0 / 1) with encode-ahead asked for -- the text pass of the next batch beside the current step -- and with
    its default for these batches (off), against set_batch_images, 5 steps"""
    from arp_amd import m3ae, synth_policy as S
    from arp_amd.train import TrainState, create_train_step, prefetch_to_device
    ecfg, _, _, pcfg, EP, P, _, _, tok, mask = _setup()
    rng = np.random.default_rng(9)
    r = ecfg.img_res
    batches = [{"image": {"ob": S.normalized_frames(4 * pcfg.window, r, seed=20 + i).reshape(4, pcfg.window, r, r, 3)},
                "action": rng.integers(0, pcfg.n_actions, (4, pcfg.window)).astype(np.int32),
                "instruct": np.tile(tok, (4, 1)), "text_padding_mask": np.tile(mask, (4, 1))} for i in range(5)]
    out = {}
    for name in ("sync", "prefetch", "prefetch default"):
        if name == "prefetch":
            monkeypatch.setenv("ARP_DT_ENCODE_AHEAD", "1")
        else:
            monkeypatch.delenv("ARP_DT_ENCODE_AHEAD", raising=False)
        enc = m3ae.M3AEEncoder(ecfg, EP, mode=mode)
        state = TrainState.create(pcfg, P, mode=mode)
        state.trainer.attach_encoder(enc, instruct=tok, text_padding_mask=mask)
        fn = create_train_step(pcfg, lambda step: 1e-3, pcfg.weight_decay)
        losses = []
        if name == "sync":
            for b in batches:
                state.trainer.set_batch_images(b["image"]["ob"], b["action"])
                losses.append(state.trainer.train_step(1e-3)["loss"])
        else:
            for b in prefetch_to_device(iter(batches), 2, state.trainer):
                state, aux, _ = fn(state, b, None)
                losses.append(aux["loss"])
        out[name] = (losses, state.trainer.get_params())
        state.trainer.close(); enc.close()
    assert out["sync"][0] == out["prefetch"][0] == out["prefetch default"][0] and all(np.isfinite(v) for v in out["sync"][0])
    for name in ("prefetch", "prefetch default"):
        assert all(np.array_equal(out["sync"][1][k], out[name][1][k]) for k in out["sync"][1]), name


def test_index_batches_of_frames_equal_host_batches_bitwise(gpu_lib):
    """a DeviceDataset's frames, gathered on the GPU and encoded with the text pass, against host-built batches of the same rows"""
    from arp_amd import dataset, m3ae
    from arp_amd.dataset import ProcgenDataset
    from arp_amd.train import TrainState, create_train_step, prefetch_to_device
    ecfg, _, _, pcfg, EP, P, _, _, tok, mask = _setup(window=T)
    arrays = {k: v for k, v in _data(64)[0].items() if "reward" not in k}
    pd = ProcgenDataset(arrays, T, env_name="coinrun", use_vl=False)  # no return-to-go: model BC reads none
    lut = dataset.default_lut()
    out = {}
    for feed in ("host", "index"):
        enc = m3ae.M3AEEncoder(ecfg, EP, mode="f32")
        state = TrainState.create(pcfg, P, mode="f32")
        tr = state.trainer
        tr.attach_encoder(enc, instruct=tok, text_padding_mask=mask)
        losses = []
        if feed == "host":
            for idx in BATCHES[:3]:
                items = [pd[int(i)] for i in idx]
                fr = np.stack([it["image"]["ob"] for it in items])
                img = np.stack([lut[c][fr[..., c]] for c in range(3)], axis=-1)
                tr.set_batch_images(img, np.stack([it["action"] for it in items]).astype(np.int32))
                losses.append(tr.train_step(1e-3)["loss"])
        else:
            ds = dataset.DeviceDataset.load(pd)
            tr.attach_dataset(ds)
            fn = create_train_step(pcfg, lambda step: 1e-3, pcfg.weight_decay)
            for b in prefetch_to_device(({"index": np.asarray(i, np.int64)} for i in BATCHES[:3]), 2, tr):
                state, aux, _ = fn(state, b, None)
                losses.append(aux["loss"])
        out[feed] = (losses, tr.get_params())
        tr.close()
        if feed == "index":
            ds.close()
        enc.close()
    assert out["host"][0] == out["index"][0] and len(out["host"][0]) == 3
    assert all(np.array_equal(out["host"][1][k], out["index"][1][k]) for k in P)


def test_batch_dict_instruction_is_checked(gpu_lib):
    """the step functions and greedy_action accept "instruct" / "text_padding_mask" rows that repeat the attached instruction and refuse a differing row"""
    from arp_amd import m3ae
    from arp_amd._ffi import ArpError
    from arp_amd.train import PolicyTrainer, TrainState, create_train_step, create_val_step
    ecfg, _, _, pcfg, EP, P, frames, act, tok, mask = _setup()
    enc = m3ae.M3AEEncoder(ecfg, EP, mode="f32")
    a = PolicyTrainer(pcfg, mode="f32"); a.set_params(P); a.attach_encoder(enc, instruct=tok, text_padding_mask=mask)
    a.set_batch_images(frames, act)
    want_action = a.forward()["action_pred"][:, -1, :].argmax(-1)
    want = a.train_step(1e-3)
    b = PolicyTrainer(pcfg, mode="f32"); b.set_params(P); b.attach_encoder(enc, instruct=np.tile(tok, (3, 1)), text_padding_mask=np.tile(mask, (3, 1)))
    batch = {"image": {"ob": frames}, "action": act, "instruct": np.tile(tok, (3, 1)), "text_padding_mask": np.tile(mask, (3, 1))}
    assert (b.greedy_action(batch) == want_action).all()
    vaux, _ = create_val_step(pcfg)(TrainState(b), batch, None)
    assert np.isfinite(vaux["loss"])
    _, aux, _ = create_train_step(pcfg, lambda s: 1e-3, pcfg.weight_decay)(TrainState(b), batch, None)
    assert aux["loss"] == want["loss"] and aux["grad_norm"] == want["grad_norm"]
    bad = dict(batch, instruct=batch["instruct"].copy())
    bad["instruct"][1, 2] = (bad["instruct"][1, 2] + 1) % VOCAB
    with pytest.raises(ArpError, match="BC.py:290-291"):
        b.greedy_action(bad)
    other = dict(batch, instruct=(batch["instruct"] + 1) % VOCAB)   # equal rows, but not the attached instruction
    with pytest.raises(ArpError, match="differ from the instruction attached"):
        create_train_step(pcfg, lambda s: 1e-3, pcfg.weight_decay)(TrainState(b), other, None)
    with pytest.raises(ArpError, match="BC.py:290-291"):
        PolicyTrainer(pcfg, mode="f32").attach_encoder(enc, instruct=bad["instruct"])
    assert (b.greedy_action(batch) == b.greedy_action(batch)).all()   # the handle is still usable
    a.close(); b.close(); enc.close()


def test_which_handles_take_which_encoder(gpu_lib):
    """arp_dt_attach_encoder still refuses the BC handle; the new entry refuses an ARP-DT handle, a GCBC handle, a wrong enc_tokens, an encoder without the text
    weights and a token id outside the vocabulary"""
    import ctypes as C
    from arp_amd import _ffi, m3ae
    from arp_amd.train import PolicyConfig, PolicyTrainer
    ecfg, _, kw, pcfg, EP, P, frames, act, tok, mask = _setup()
    enc = m3ae.M3AEEncoder(ecfg, EP, mode="f32")
    tr = PolicyTrainer(pcfg, mode="f32")
    with pytest.raises(_ffi.ArpError, match="model BC takes encodings"):
        tr.attach_encoder(enc)
    with pytest.raises(_ffi.ArpError, match="model BC"):
        _ffi.check(_ffi.lib.arp_dt_attach_encoder(tr._h, tr._h))   # on the model alone, as tests/test_bc_gpu.py pins it
    for other in (PolicyConfig(**kw), PolicyConfig(**dict(kw, enc_tokens=ecfg.gc_tokens), model="GCBC")):
        o = PolicyTrainer(other, mode="f32")
        with pytest.raises(_ffi.ArpError, match="belongs to model BC"):
            o.attach_encoder(enc, instruct=tok, text_padding_mask=mask)
        o.close()
    wrong = PolicyTrainer(PolicyConfig(**dict(kw, enc_tokens=ecfg.tokens), model="BC"), mode="f32")
    with pytest.raises(_ffi.ArpError, match="enc_tokens must be 1 \\+ P \\+ L"):
        wrong.attach_encoder(enc, instruct=tok, text_padding_mask=mask)
    wrong.close()
    with pytest.raises(_ffi.ArpError, match="outside the vocabulary"):
        tr.attach_encoder(enc, instruct=np.full(L, VOCAB), text_padding_mask=mask)
    bare = m3ae.M3AEEncoder(ecfg, {k: v for k, v in EP.items() if "text" not in k}, mode="f32")
    with pytest.raises(_ffi.ArpError, match="text weights were not loaded"):
        tr.attach_encoder(bare, instruct=tok, text_padding_mask=mask)
    bare.close()
    with pytest.raises(_ffi.ArpError, match="no encoder attached"):   # nothing above stuck
        tr.set_batch_images(frames, act)
    tr.set_params(P); tr.attach_encoder(enc, instruct=tok, text_padding_mask=mask); tr.set_batch_images(frames, act)
    assert np.isfinite(tr.forward()["loss"])
    tr.close(); enc.close()


def test_handles_release_what_they_took(gpu_lib):
    import ctypes as C
    import gc
    from arp_amd import m3ae
    from arp_amd.train import PolicyTrainer

    def live():
        out = (C.c_int64 * 5)()
        gpu_lib.check(gpu_lib.lib.arp_debug_live(out))
        return list(out)
    ecfg, _, _, pcfg, EP, P, frames, act, tok, mask = _setup()
    gc.collect()
    before = live()
    enc = m3ae.M3AEEncoder(ecfg, EP, mode="f16")
    tr = PolicyTrainer(pcfg, mode="f16"); tr.set_params(P); tr.attach_encoder(enc, instruct=tok, text_padding_mask=mask)
    tr.set_batch_images(frames, act)
    tr.train_step(1e-3)
    tr.attach_encoder(enc, instruct=(tok + 1) % VOCAB, text_padding_mask=mask)   # a re-attach replaces the instruction
    tr.set_batch_images(frames, act)
    tr.train_step(1e-3)
    tr.close(); enc.close()
    assert live() == before


ROLLOUT_BAR = {"f32": 1e-6, "f16": 1.5e-3}   # tests/test_rollout_gpu.py's f32 logits bar; tests/test_rollout_gc_gpu.py's f16 bar


@pytest.mark.parametrize("mode", ["f32", "f16"])
def test_rollout_session_with_the_instruction(gpu_lib, mode):
    """2 environments, 6 steps, environment 1 reset before step 3.  The host-driven way: a second handle with the same instruction attached stages each
    environment's window of frames (zeros behind the L real steps) with the session's action window and runs the policy's forward, which encodes all T
    frames again; the session encoded one new frame per environment and step.  Logits rows L - 1 within the mode's bar, and the same actions wherever
    the host-driven top-two gap exceeds twice the bar (f16: the session's pass of 2 x 30 rows runs on the latency path, another summation order)."""
    from arp_amd import dataset, m3ae, synth
    from arp_amd.rollout import RolloutSession
    from arp_amd.train import PolicyTrainer
    ecfg, _, _, pcfg, EP, P, _, _, tok, mask = _setup()
    E, T, r, bar = 2, pcfg.window, ecfg.img_res, ROLLOUT_BAR[mode]
    enc = m3ae.M3AEEncoder(ecfg, EP, mode=mode)
    tr = PolicyTrainer(pcfg, mode=mode); tr.set_params(P)
    host = PolicyTrainer(pcfg, mode=mode); host.set_params(P); host.attach_encoder(enc, instruct=tok, text_padding_mask=mask)
    with pytest.raises(gpu_lib.ArpError, match="pass one to arp_rollout_create_with_encoder|no encoder"):
        RolloutSession(tr, n_envs=E, instruct=(tok, mask))           # nothing attached, nothing lent
    ses = RolloutSession(tr, n_envs=E, encoder=enc, instruct=(tok, mask))   # lent; the handle `tr` itself carries no encoder
    hist = [[] for _ in range(E)]
    worst, decided = 0.0, 0
    try:
        ses.reset()
        for t in range(6):
            if t == 3:
                ses.reset(env_ids=[1])
                hist[1] = []
            fr = synth.procgen_like_frames(E, r, r, seed=700 + t)
            act = ses.step(fr)
            aw, lg = ses.read("action_window"), ses.read("logits")
            window = np.zeros((E, T, r, r, 3), np.float32)
            Ls = []
            for e in range(E):
                hist[e] = (hist[e] + [dataset.bytes_to_float(fr[e])])[-T:]
                Ls.append(len(hist[e]))
                window[e, :Ls[e]] = np.stack(hist[e])
            host.set_batch_images(window, aw)
            hl = host.forward()["action_pred"]
            for e in range(E):
                L = Ls[e]
                err = float(np.abs(lg[e, L - 1] - hl[e, L - 1]).max())
                worst = max(worst, err)
                top = np.sort(hl[e, L - 1])[::-1]
                assert err <= bar, (t, e, err)
                assert act[e] == lg[e, L - 1].argmax()
                if top[0] - top[1] > 2 * bar:
                    decided += 1
                    assert act[e] == hl[e, L - 1].argmax(), (t, e)
        print(f"InstructRL session {mode}: max logit difference session / host-driven {worst:.2e}, {decided} of 12 decisions compared")
        assert decided >= 6
        assert Ls == [T, 3]
    finally:
        ses.close(); host.close(); tr.close(); enc.close()
    # the policy's own encoder, when it carries one, serves the session too; ARP-DT and GCBC policies are refused
    from arp_amd.train import PolicyConfig
    enc = m3ae.M3AEEncoder(ecfg, EP, mode=mode)
    own = PolicyTrainer(pcfg, mode=mode); own.set_params(P); own.attach_encoder(enc, instruct=tok, text_padding_mask=mask)
    ses = RolloutSession(own, n_envs=1, instruct=(tok, mask))
    ses.reset()
    assert ses.step(synth.procgen_like_frames(1, r, r, seed=1)).shape == (1,)
    ses.close()
    arp = PolicyTrainer(PolicyConfig(emb=64, depth=2, heads=4, window=3, enc_tokens=pcfg.enc_tokens, enc_dim=pcfg.enc_dim), mode=mode)
    with pytest.raises(gpu_lib.ArpError, match="belongs to model BC"):
        RolloutSession(arp, n_envs=1, encoder=enc, instruct=(tok, mask))
    arp.close(); own.close(); enc.close()
