"""Model GCBC trained from the device-resident set (arp_amd/csrc/arp_ds.hip's pair gather, arp_dt_*_index_pairs*, prefetch_to_device with encode-ahead).

Every comparison is bitwise: the gather is a table look-up that the host path repeats through the same table, and the goal-conditioned encoder pass is the
same kernels on the same bytes, on another stream.  The set is tests/test_dataset_gpu.py's (24 rows, trajectories starting at rows 0, 1, 3 and 10)."""
import ctypes as C
import gc
import itertools

import numpy as np
import pytest

import dataset_oracle as O
from test_dataset_gpu import LENS, _data
from test_gcbc_gpu import LONG_ENC, SMALL_ENC

pytestmark = pytest.mark.gpu

T, B = 3, 4
# (row, goal row), chosen by hand: a one-row trajectory; a trajectory shorter than the window with its last row / the row itself as the goal; first row to
# last row; a row as its own goal; the file's last row (from its trajectory's first row, and from itself); a goal in ANOTHER trajectory (bounds are checked,
# not the hindsight rule); a repeated pair
PAIRS = [(0, 0), (1, 2), (1, 1), (3, 9), (5, 5), (10, 23), (23, 23), (4, 20), (3, 9), (3, 9)]
VAL = (np.asarray([0, 23, 1, 5], np.int64), np.asarray([0, 23, 2, 9], np.int64))  # the validation / greedy batch: fixed goals (no draw from the stream's generator)
SEED, GOAL_SEED = 3, 7

_CACHE = {}


def _literal_goals(arrays, g, lut, window):
    fr = np.stack([arrays["ob"][int(r)][-window:] for r in g])
    return np.stack([lut[c][fr[..., c]] for c in range(3)], axis=-1)


@pytest.mark.parametrize("hw,lut_seed", [(64, None), (64, 5), (32, None)])
def test_pair_gather_equals_the_literal_windows_bitwise(gpu_lib, hw, lut_seed):
    from arp_amd import dataset
    arrays, pd, _, _ = _data(hw)
    lut = dataset.default_lut() if lut_seed is None else np.random.default_rng(lut_seed).standard_normal((3, 256)).astype(np.float32)
    ds = dataset.DeviceDataset.load(pd, lut=None if lut_seed is None else lut, chunk_rows=7)
    try:
        batches = [(np.asarray([p[0] for p in PAIRS]), np.asarray([p[1] for p in PAIRS]))]
        if hw == 64 and lut_seed is None:  # 400 pairs x window 3 = 1 200 frames per half: a block walks more than one tile of a frame
            rng = np.random.default_rng(2)
            batches.append((rng.integers(0, 24, 400), rng.integers(0, 24, 400)))
        for idx, g in batches:
            got, plain = ds.gather(idx, goal_index=g), ds.gather(idx)
            assert set(got) == {"image", "goal", "action"}
            want = _literal_goals(arrays, g, lut, T)
            assert got["goal"].shape == want.shape and np.array_equal(got["goal"], want)
            assert np.array_equal(got["image"], plain["image"]) and np.array_equal(got["action"], plain["action"])
            assert np.array_equal(got["image"], _literal_goals(arrays, idx, lut, T))
    finally:
        ds.close()


def _goal_pd(hw, window):
    from arp_amd.dataset import ProcgenDataset
    return ProcgenDataset(dict(_arrays(hw)), window, env_name="coinrun", goal_rng=np.random.RandomState(GOAL_SEED))


def _arrays(hw):
    if ("arrays", hw) not in _CACHE:
        _CACHE[("arrays", hw)] = _data(hw)[0] if hw in (32, 64) else O.recorder_arrays(LENS, hw=hw, seed=11)
    return _CACHE[("arrays", hw)]


def _host_batch(pd, idx, lut, goal_index=None):
    """The batch the host path builds: ProcgenDataset.__getitem__ per row, in order (one goal draw per item), frames and goals through the table.
    goal_index: these goal rows instead of drawn ones."""
    from arp_amd.dataset import bytes_to_float
    if goal_index is None:
        items = [pd[int(i)] for i in idx]
        goal = np.stack([it["goal"]["ob"] for it in items])
    else:
        items = [{"image": {"ob": pd.last_frames(pd.window_rows(int(i)))}, "action": pd.action[pd.window_rows(int(i))]} for i in idx]
        goal = np.stack([pd.last_frames(pd.window_rows(int(g))) for g in goal_index])
    img = np.stack([it["image"]["ob"] for it in items])
    return {"image": {"ob": bytes_to_float(img, lut)}, "goal": {"ob": bytes_to_float(goal, lut)},
            "action": np.stack([it["action"] for it in items]).astype(np.int32)}


def _run(feed, pmode, emode, enc_kw=SMALL_ENC, window=T, batch=B, steps=5):
    """`steps` train steps, with a validation step and a greedy action on the VAL pairs after step 3 (where there are 5).  feed: "host" (set_batch_images(goals=)
    of host-built batches, goals drawn by ProcgenDataset(goal_rng=RandomState(7)): the reference trajectory), "index" (pair batches of
    index_batches(goal_rng=RandomState(7)) through prefetch_to_device) or "sync" (the same pair batches through set_batch_index_pairs, no prefetcher).
    Returns (losses, val aux, greedy action, parameters)."""
    from arp_amd import dataset, m3ae, synth_policy as S
    from arp_amd.train import PolicyConfig, TrainState, create_train_step, create_val_step, prefetch_to_device
    from oracle import m3ae_np as M
    hw = enc_kw["img_res"]
    pd = _goal_pd(hw, window)
    lut = dataset.default_lut()
    ecfg = m3ae.EncoderConfig(**enc_kw)
    pcfg = PolicyConfig(emb=64, depth=2, heads=4, window=window, enc_tokens=ecfg.gc_tokens, enc_dim=ecfg.width, model="GCBC")
    enc = m3ae.M3AEEncoder(ecfg, S.m3ae_params(M.EncConfig(**enc_kw), seed=5), mode=emode)
    state = TrainState.create(pcfg, S.policy_params(pcfg, seed=6), mode=pmode)
    tr = state.trainer
    tr.attach_encoder(enc)
    fn, vfn = create_train_step(pcfg, lambda step: 1e-3, pcfg.weight_decay), create_val_step(pcfg)
    ds = None
    losses, val, ga = [], None, None
    try:
        if feed == "host":
            plain = itertools.islice(dataset.index_batches(len(pd), batch, SEED, process_index=pd.process_index), steps)
            for i, b in enumerate(plain):
                hb = _host_batch(pd, b["index"], lut)
                tr.set_batch_images(hb["image"]["ob"], hb["action"], goals=hb["goal"]["ob"])
                losses.append(tr.train_step(1e-3)["loss"])
                if i == 2 and steps == 5:
                    v = _host_batch(pd, VAL[0], lut, goal_index=VAL[1])
                    val, _ = vfn(TrainState(tr), v, None)
                    ga = tr.greedy_action(v)
        else:
            ds = dataset.DeviceDataset.load(pd)
            tr.attach_dataset(ds)
            stream = itertools.islice(ds.index_batches(batch, SEED, goal_rng=np.random.RandomState(GOAL_SEED)), steps)
            for i, b in enumerate(prefetch_to_device(stream, 2, tr) if feed == "index" else stream):
                state, aux, _ = fn(state, b, None)
                losses.append(aux["loss"])
                if i == 2 and steps == 5:
                    v = {"index": VAL[0], "goal_index": VAL[1]}
                    val, _ = vfn(state, v, None)
                    ga = tr.greedy_action(v)
        return losses, val, ga, tr.get_params()
    finally:
        tr.close()
        if ds is not None:
            ds.close()
        enc.close()


def _cached(feed, pmode, emode):
    key = (feed, pmode, emode)
    if key not in _CACHE:
        _CACHE[key] = _run(feed, pmode, emode)
    return _CACHE[key]


def _same(a, b, steps=5):
    assert a[0] == b[0], (a[0], b[0])
    assert all(np.isfinite(v) for v in a[0]) and len(a[0]) == steps
    if steps == 5:
        assert a[1] == b[1] and np.array_equal(a[2], b[2]) and a[2].shape == (B,)
    assert all(np.array_equal(a[3][k], b[3][k]) for k in a[3])


@pytest.mark.parametrize("pmode,emode", [("f32", "f32"), ("f16", "f16")])
def test_index_pairs_equal_the_host_goal_batches_bitwise(gpu_lib, monkeypatch, pmode, emode):
    monkeypatch.delenv("ARP_DT_ENCODE_AHEAD", raising=False)  # encode-ahead on (the default)
    monkeypatch.delenv("ARP_DT_ENC_EAGER", raising=False)
    _same(_cached("index", pmode, emode), _cached("host", pmode, emode))


def test_gc_encode_ahead_on_equals_off_bitwise(gpu_lib, monkeypatch):
    monkeypatch.delenv("ARP_DT_ENCODE_AHEAD", raising=False)
    monkeypatch.delenv("ARP_DT_ENC_EAGER", raising=False)
    on = _cached("index", "f16", "f16")
    sync = _run("sync", "f16", "f16")
    monkeypatch.setenv("ARP_DT_ENCODE_AHEAD", "0")
    off = _run("index", "f16", "f16")
    _same(off, on)
    _same(sync, on)


def test_long_pairs_prefetched_equal_the_synchronous_slot_bitwise(gpu_lib, monkeypatch):
    """339 tokens per pair: the key-blocked attention runs on the encoder stream beside the policy part of the step before."""
    monkeypatch.delenv("ARP_DT_ENCODE_AHEAD", raising=False)
    monkeypatch.delenv("ARP_DT_ENC_EAGER", raising=False)
    kw = dict(enc_kw=LONG_ENC, window=2, batch=2, steps=3)
    ahead = _run("index", "f16", "f16", **kw)
    _same(ahead, _run("sync", "f16", "f16", **kw), steps=3)
    _same(ahead, _run("host", "f16", "f16", **kw), steps=3)


def test_pair_refusals_leave_the_handles_usable(gpu_lib):
    from arp_amd import dataset, m3ae, synth_policy as S
    from arp_amd._ffi import ArpError
    from arp_amd.train import PolicyConfig, PolicyTrainer
    from oracle import m3ae_np as M
    pd = _data(64)[1]
    n = pd.n_rows
    ds = dataset.DeviceDataset.load(pd)
    ecfg = m3ae.EncoderConfig(**SMALL_ENC)
    enc = m3ae.M3AEEncoder(ecfg, S.m3ae_params(M.EncConfig(**SMALL_ENC), seed=5), mode="f32")
    kw = dict(emb=64, depth=2, heads=4, window=T, enc_dim=ecfg.width)
    pcfg = PolicyConfig(**kw, enc_tokens=ecfg.gc_tokens, model="GCBC")
    ok_i, ok_g = [0, 5, 23, 11], [0, 9, 23, 20]
    i64 = lambda a: np.asarray(a, np.int64).ctypes.data_as(C.POINTER(C.c_int64))  # noqa: E731

    tr = PolicyTrainer(pcfg, mode="f32")
    tr.set_params(S.policy_params(pcfg, seed=6))
    # pairs without an encoder: the trainer refuses to attach frames, and the library refuses the call itself
    with pytest.raises(ArpError, match="encoder"):
        tr.attach_dataset(ds)
    assert gpu_lib.lib.arp_dt_set_batch_index_pairs(tr._h, ds._h, i64(ok_i), i64(ok_g), 4) != 0 and "no encoder attached" in gpu_lib.last_error()
    assert gpu_lib.lib.arp_dt_upload_batch_index_pairs_async(tr._h, 0, ds._h, i64(ok_i), i64(ok_g), 4) != 0 and "no encoder attached" in gpu_lib.last_error()
    tr.attach_encoder(enc)
    # a GCBC encodings cache
    with pytest.raises(ArpError, match="not a per-row quantity"):
        tr.attach_dataset(ds, use_encodings=True)
    tr.attach_dataset(ds)
    tr.set_batch_index_pairs(ok_i, ok_g)
    loss = tr.forward()["loss"]
    assert np.isfinite(loss)
    # a goal index equal to n_rows, a negative one; a bad row index still says what it said
    for bad in ([0, n, 1, 2], [0, -1, 1, 2]):
        with pytest.raises(ArpError, match=r"goal index .* \(batch position 1\) is outside"):
            tr.set_batch_index_pairs(ok_i, bad)
        with pytest.raises(ArpError, match=r"goal index .* \(batch position 1\) is outside"):
            tr.upload_index_pairs_async(0, ok_i, bad)
        with pytest.raises(ArpError, match=r"index .* \(batch position 1\) is outside") as e:
            tr.upload_index_pairs_async(0, bad, ok_g)
        assert "goal index" not in str(e.value)
    with pytest.raises(ArpError, match="one goal row per row"):
        tr.set_batch_index_pairs(ok_i, ok_g[:3])
    assert tr.forward()["loss"] == loss  # the staged batch is still selected
    # a plain index batch on a GCBC handle: it names no goals (and the refusal names the call that does)
    with pytest.raises(ArpError, match="arp_dt_set_batch_index_pairs"):
        tr.set_batch_indices(ok_i)
    with pytest.raises(ArpError, match="arp_dt_upload_batch_index_pairs_async"):
        tr.upload_indices_async(0, ok_i)
    # encode-ahead of the synchronous slot: its step encodes it (the text tests/test_gcbc_gpu.py pins); of an empty prefetch slot
    with pytest.raises(ArpError, match="no encode-ahead"):
        tr.encode_ahead(2)
    with pytest.raises(ArpError, match="holds no frames"):
        tr.encode_ahead(1)
    # slot 0 is still fillable, encodes ahead, and holds the batch the synchronous slot held
    assert tr.upload_index_pairs_async(0, ok_i, ok_g) is True
    tr.encode_ahead(0)
    tr.select(0)
    assert tr.forward()["loss"] == loss
    assert np.isfinite(tr.train_step(1e-3)["loss"])
    tr.close()

    # pairs on an ARP-DT handle
    acfg = PolicyConfig(**kw, enc_tokens=ecfg.tokens, lambda_ret=0.5)
    a = PolicyTrainer(acfg, mode="f32")
    a.set_params(S.policy_params(acfg, seed=6))
    a.attach_encoder(enc)
    a.attach_dataset(ds)
    with pytest.raises(ArpError, match="goal indices belong to model GCBC"):
        a.set_batch_index_pairs(ok_i, ok_g)
    with pytest.raises(ArpError, match="goal indices belong to model GCBC"):
        a.upload_index_pairs_async(0, ok_i, ok_g)
    a.set_batch_indices(ok_i)
    assert np.isfinite(a.forward()["loss"])
    a.upload_indices_async(0, ok_i)
    a.select(0)
    assert np.isfinite(a.forward()["loss"])
    a.close(); ds.close(); enc.close()


def test_gc_prefetch_releases_what_it_took(gpu_lib, monkeypatch):
    monkeypatch.delenv("ARP_DT_ENCODE_AHEAD", raising=False)
    monkeypatch.delenv("ARP_DT_ENC_EAGER", raising=False)

    def live():
        out = (C.c_int64 * 5)()
        gpu_lib.check(gpu_lib.lib.arp_debug_live(out))
        return list(out)
    _arrays(64)
    gc.collect()
    before = live()
    losses = _run("index", "f16", "f16", steps=3)[0]
    assert len(losses) == 3
    gc.collect()
    assert live() == before
