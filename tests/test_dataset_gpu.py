"""GPU tests of the device-resident demonstration set (arp_amd/dataset.py::DeviceDataset, arp_amd/csrc/arp_ds.hip): the gathers against the literal
reading of the stacked rows (tests/dataset_oracle.py), bitwise; train trajectories fed by index batches against the same trajectories fed by the host-built
batches of ProcgenDataset.__getitem__, bitwise (frames through the encoder inside the step, cached encodings, model BC on supplied encodings); and every
refusal the host-side checks make, each followed by a valid call that works."""
import numpy as np
import pytest

import dataset_oracle as O

pytestmark = pytest.mark.gpu

TINY_ENC = dict(patch=16, width=64, layers=2, heads=2, img_res=64)  # 17 tokens
LENS = [1, 2, 7, 14]  # 24 rows; window 3: a trajectory shorter than the window, one of its length - 1, two longer
T, B = 3, 4
POLICY = dict(emb=64, depth=2, heads=4, window=T, enc_tokens=17, enc_dim=64, lambda_ret=0.5)
# 5 batches: row 0, the last row, every trajectory's first rows, a repeated index; the rest spread over the long trajectories
BATCHES = [[0, 23, 1, 2], [3, 4, 5, 5], [10, 11, 12, 9], [23, 23, 0, 17], [8, 20, 13, 6]]

_CACHE = {}


def _data(hw=64):
    if hw not in _CACHE:
        from arp_amd.dataset import ProcgenDataset
        arrays = O.recorder_arrays(LENS, hw=hw, seed=11)
        pd = ProcgenDataset(dict(arrays), T, env_name="coinrun")
        rtgs, _, _, _, scale = O.preprocess_rtgs(arrays["ob_clip_reward"], arrays["done"], "coinrun", False)
        _CACHE[hw] = (arrays, pd, rtgs, scale)
    return _CACHE[hw]


def _literal(arrays, rtgs, scale, idx, lut):
    """The batch the reference reads for these rows (the stacked rows themselves), frames through the byte -> float table."""
    items = [O.getitem(arrays, int(i), T, rtgs, scale) for i in idx]
    fr = np.stack([it["image"]["ob"] for it in items])
    img = np.stack([lut[c][fr[..., c]] for c in range(3)], axis=-1)
    return img, np.stack([it["action"] for it in items]).astype(np.int32), np.stack([it["rtg"]["ob"] for it in items]).astype(np.float32)


@pytest.mark.parametrize("hw,lut_seed", [(64, None), (64, 5), (32, None)])
def test_gather_equals_the_literal_windows_bitwise(gpu_lib, hw, lut_seed):
    from arp_amd import dataset
    arrays, pd, rtgs, scale = _data(hw)
    lut = dataset.default_lut() if lut_seed is None else np.random.default_rng(lut_seed).standard_normal((3, 256)).astype(np.float32)
    ds = dataset.DeviceDataset.load(pd, lut=None if lut_seed is None else lut, chunk_rows=7)  # 7: chunks that end inside trajectories
    try:
        assert ds.nbytes >= 24 * hw * hw * 3
        # 400 rows x window 3 = 1 200 frames: past the size at which a block of the frame gather walks more than one tile of a frame
        many = [np.random.default_rng(1).integers(0, 24, 400).tolist()] if hw == 64 and lut_seed is None else []
        for idx in BATCHES + [[0, 1, 2, 3, 4, 10, 11, 12, 23, 23, 9, 0]] + many:
            got = ds.gather(idx)
            img, act, rtg = _literal(arrays, rtgs, scale, idx, lut)
            assert got["image"].shape == img.shape and np.array_equal(got["image"], img)
            assert np.array_equal(got["action"], act) and np.array_equal(got["rtg"], rtg)
    finally:
        ds.close()


def _host_batch(pd, idx, lut):
    """The batch the host path builds: ProcgenDataset.__getitem__ per row, frames through the table (what a data loader's collate would do)."""
    items = [pd[int(i)] for i in idx]
    fr = np.stack([it["image"]["ob"] for it in items])
    img = np.stack([lut[c][fr[..., c]] for c in range(3)], axis=-1)
    return {"image": {"ob": img}, "action": np.stack([it["action"] for it in items]).astype(np.int32),
            "rtg": {"ob": np.stack([it["rtg"]["ob"] for it in items])}}


def _run(feed, pmode, emode):
    """5 train steps, with a validation step and a greedy action on batch 0 after step 3.  feed: "host" (set_batch_images of host-built batches: the
    reference trajectory), "index" (index batches through prefetch_to_device, frames gathered on the GPU, encode-ahead on) or "cached" (index batches on
    cached encodings).  Returns (losses, val aux, greedy action, parameters)."""
    from arp_amd import dataset, m3ae, synth_policy as S
    from arp_amd.train import PolicyConfig, TrainState, create_train_step, create_val_step, prefetch_to_device
    from oracle import m3ae_np as M
    arrays, pd, rtgs, scale = _data(64)
    lut = dataset.default_lut()
    ecfg, pcfg = m3ae.EncoderConfig(**TINY_ENC), PolicyConfig(**POLICY)
    enc = m3ae.M3AEEncoder(ecfg, S.m3ae_params(M.EncConfig(**TINY_ENC), seed=5), mode=emode)
    state = TrainState.create(pcfg, S.policy_params(pcfg, seed=6), mode=pmode)
    tr = state.trainer
    tr.attach_encoder(enc)
    fn, vfn = create_train_step(pcfg, lambda step: 1e-3, pcfg.weight_decay), create_val_step(pcfg)
    ds = None
    losses, val, ga = [], None, None
    try:
        if feed == "host":
            for i, idx in enumerate(BATCHES):
                b = _host_batch(pd, idx, lut)
                tr.set_batch_images(b["image"]["ob"], b["action"], b["rtg"]["ob"])
                losses.append(tr.train_step(1e-3)["loss"])
                if i == 2:
                    b0 = _host_batch(pd, BATCHES[0], lut)
                    val, _ = vfn(TrainState(tr), b0, None)
                    ga = tr.greedy_action(b0["image"]["ob"], b0["action"], b0["rtg"]["ob"])
        else:
            ds = dataset.DeviceDataset.load(pd)
            if feed == "cached":
                ds.cache_encodings(enc, chunk=5)  # 24 rows in chunks of 5: no chunk is a batch of the trajectory
            tr.attach_dataset(ds, use_encodings=feed == "cached")
            it = ({"index": np.asarray(idx, np.int64)} for idx in BATCHES)
            for i, b in enumerate(prefetch_to_device(it, 2, tr)):
                state, aux, _ = fn(state, b, None)
                losses.append(aux["loss"])
                if i == 2:
                    val, _ = vfn(state, {"index": np.asarray(BATCHES[0], np.int64)}, None)
                    ga = tr.greedy_action({"index": np.asarray(BATCHES[0], np.int64)})
        return losses, val, ga, tr.get_params()
    finally:
        tr.close()
        if ds is not None:
            ds.close()
        enc.close()


def _reference(pmode, emode):
    key = ("host", pmode, emode)
    if key not in _CACHE:
        _CACHE[key] = _run("host", pmode, emode)
    return _CACHE[key]


def _same(a, b):
    assert a[0] == b[0], (a[0], b[0])
    assert a[1] == b[1] and np.array_equal(a[2], b[2]) and a[2].shape == (B,)
    assert all(np.array_equal(a[3][k], b[3][k]) for k in a[3])
    assert all(np.isfinite(v) for v in a[0]) and len(a[0]) == 5


@pytest.mark.parametrize("pmode,emode", [("f32", "f32"), ("f16", "f16")])
def test_index_batches_of_frames_equal_the_host_batches_bitwise(gpu_lib, pmode, emode):
    _same(_run("index", pmode, emode), _reference(pmode, emode))


@pytest.mark.parametrize("pmode,emode", [("f32", "f32"), ("f16", "f16")])
def test_cached_encodings_equal_the_encoder_inside_trajectory_bitwise(gpu_lib, pmode, emode):
    """The frozen encoder's output for a frame does not depend on the batch it is encoded in: encoded once, 5 rows at a time, and gathered per step, the
    trajectory equals the one that encodes every batch (12 frames) inside its step."""
    _same(_run("cached", pmode, emode), _reference(pmode, emode))


def test_bc_trains_from_supplied_encodings_by_index(gpu_lib):
    """Model BC takes encodings (and refuses the image-only encoder): set_encodings + index batches equal set_batch on the host-gathered encodings."""
    from arp_amd import dataset, synth_policy as S
    from arp_amd.dataset import ProcgenDataset
    from arp_amd.train import PolicyConfig, TrainState, create_train_step, prefetch_to_device
    arrays = {k: v for k, v in _data(64)[0].items() if "reward" not in k}
    pd = ProcgenDataset(arrays, T, env_name="coinrun", use_vl=False)  # no return-to-go
    cfg = PolicyConfig(**dict(POLICY, enc_tokens=9), model="BC")
    P = S.policy_params(cfg, seed=3)
    E = np.random.default_rng(4).standard_normal((24, 9, 64)).astype(np.float32)
    out = {}
    for feed in ("host", "index"):
        state = TrainState.create(cfg, P, mode="f32")
        tr = state.trainer
        losses = []
        if feed == "host":
            for idx in BATCHES[:3]:
                j = np.stack([pd.window_rows(i) for i in idx])
                tr.set_batch(E[j], np.stack([pd[i]["action"] for i in idx]))
                losses.append(tr.train_step(1e-3)["loss"])
        else:
            ds = dataset.DeviceDataset.load(pd)
            ds.set_encodings(iter([E[:10], E[10:]]))
            tr.attach_dataset(ds, use_encodings=True)
            fn = create_train_step(cfg, lambda step: 1e-3, cfg.weight_decay)
            for b in prefetch_to_device(({"index": np.asarray(i, np.int64)} for i in BATCHES[:3]), 2, tr):
                state, aux, _ = fn(state, b, None)
                losses.append(aux["loss"])
            assert "rtg" not in ds.gather(BATCHES[0], frames=False)
            ds.close()
        out[feed] = (losses, tr.get_params())
        tr.close()
    assert out["host"][0] == out["index"][0] and len(out["host"][0]) == 3
    assert all(np.array_equal(out["host"][1][k], out["index"][1][k]) for k in P)


def test_refusals_leave_the_handles_usable(gpu_lib):
    from arp_amd import dataset, m3ae, synth_policy as S
    from arp_amd._ffi import ArpError
    from arp_amd.train import PolicyConfig, PolicyTrainer, prefetch_to_device
    from oracle import m3ae_np as M
    arrays, pd, rtgs, scale = _data(64)
    n = pd.n_rows
    frames = np.ascontiguousarray(arrays["ob"][:, -1])
    rtg = (pd.rtg / np.float32(pd.scale)).astype(np.float32)
    ok = [0, 5, 23, 11]
    want = _literal(arrays, rtgs, scale, ok, dataset.default_lut())

    def good(g):
        assert np.array_equal(g["image"], want[0]) and np.array_equal(g["action"], want[1]) and np.array_equal(g["rtg"], want[2])

    # a set built by hand: labels not set, frames only partly uploaded
    raw = dataset.DeviceDataset(n, 64)
    raw.window_size = T
    raw.set_lut(dataset.default_lut())
    raw.upload_frames(0, frames[:10])
    with pytest.raises(ArpError, match="frame rows were uploaded"):
        raw.gather(ok)
    raw.upload_frames(10, frames[10:])
    with pytest.raises(ArpError, match="labels are not set"):
        raw.gather(ok)
    with pytest.raises(ArpError, match="action id"):
        raw.set_labels(pd.action, rtg, pd.traj_start, int(pd.action.max()))  # one action id too few
    with pytest.raises(ArpError, match="traj_start"):
        raw.set_labels(pd.action, rtg, np.minimum(pd.traj_start + 1, n - 1), 15)  # a start behind its own row
    raw.set_labels(pd.action, rtg, pd.traj_start, 15)
    good(raw.gather(ok))
    for bad, what in (([0, n, 1, 2], "outside"), ([0, -1, 1, 2], "outside")):  # an index equal to n_rows, a negative index
        with pytest.raises(ArpError, match=what):
            raw.gather(bad)
        good(raw.gather(ok))
    with pytest.raises(ArpError, match="window"):
        raw.gather(ok, window=65)
    with pytest.raises(ArpError, match="multiple of 16"):
        dataset.DeviceDataset(4, 10)  # 10 * 10 * 3 = 300 bytes per frame
    good(raw.gather(ok))

    ecfg, pcfg = m3ae.EncoderConfig(**TINY_ENC), PolicyConfig(**POLICY)
    enc = m3ae.M3AEEncoder(ecfg, S.m3ae_params(M.EncConfig(**TINY_ENC), seed=5), mode="f32")
    tr = PolicyTrainer(pcfg, mode="f32")
    tr.set_params(S.policy_params(pcfg, seed=6))
    with pytest.raises(ArpError, match="attach_dataset"):
        tr.set_batch_indices(ok)
    with pytest.raises(ArpError, match="encoder"):
        tr.attach_dataset(raw)  # frames need the encoder inside the step
    tr.attach_encoder(enc)
    wide = PolicyTrainer(PolicyConfig(**dict(POLICY, window=4)), mode="f32")
    with pytest.raises(ArpError, match="window"):  # the wrong window
        wide.attach_dataset(raw, use_encodings=True)
    wide.close()
    tr.attach_dataset(raw)
    for bad in ([0, n, 1, 2], [0, -3, 1, 2]):
        with pytest.raises(ArpError, match="outside"):
            tr.set_batch_indices(bad)
        with pytest.raises(ArpError, match="outside"):
            tr.upload_indices_async(0, bad)
    tr.set_batch_indices(ok)
    loss = tr.forward()["loss"]
    assert np.isfinite(loss)
    # use_encodings without a cache; a cache of another geometry
    tr.attach_dataset(raw, use_encodings=True)
    with pytest.raises(ArpError, match="holds no encodings"):
        tr.set_batch_indices(ok)
    raw.set_encodings(np.zeros((n, 5, 64), np.float32))
    with pytest.raises(ArpError, match="per frame"):
        tr.set_batch_indices(ok)
    # frames of another size than the encoder reads
    small = dataset.DeviceDataset.load(_data(32)[1])
    tr.attach_dataset(small)
    with pytest.raises(ArpError, match="pixels square"):
        tr.set_batch_indices(ok)
    with pytest.raises(ArpError, match="pixels square"):
        small.cache_encodings(enc)
    small.close()
    # cache_encodings under a live prefetcher
    tr.attach_dataset(raw)
    g = prefetch_to_device(({"index": np.asarray(ok, np.int64)} for _ in range(3)), 2, tr)
    first = next(g)
    with pytest.raises(ArpError, match="prefetcher"):
        raw.cache_encodings(enc)
    tr.select(first.slot)
    assert tr.forward()["loss"] == loss  # the prefetched slot holds the same batch the synchronous slot did
    first.done()
    g.close()
    raw.cache_encodings(enc)
    tr.attach_dataset(raw, use_encodings=True)
    tr.set_batch_indices(ok)
    assert tr.forward()["loss"] == loss  # cached encodings of the same frames
    tr.close(); raw.close(); enc.close()
