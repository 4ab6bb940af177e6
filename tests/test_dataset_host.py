"""Host side of the demonstration set (arp_amd/dataset.py) against the literal reading of recorder-stacked rows and the line-cited restatement of the
reference's return-to-go preprocessing (tests/dataset_oracle.py).  No GPU."""
import numpy as np
import pytest

import dataset_oracle as O

LENS = [1, 2, 5, 9, 3]  # window 4: the clamp engages at 0, 1, 2 and 3 positions, and one trajectory is shorter than the window
T = 4


def _stores(tmp_path, arrays, env_name="coinrun", name="data"):
    """The same arrays as an H5 store and as a dict store."""
    from arp_amd import h5store
    p = str(tmp_path / f"{name}.hdf5")
    O.write_h5(p, arrays, env_name)
    return {"h5": h5store.H5Store(p, "r"), "dict": dict(arrays)}


@pytest.mark.parametrize("kind", ["h5", "dict"])
def test_getitem_is_the_literal_window_bitwise(tmp_path, kind):
    from arp_amd.dataset import ProcgenDataset
    arrays = O.recorder_arrays(LENS, seed=1)
    store = _stores(tmp_path, arrays)[kind]
    ds = ProcgenDataset(store, T, env_name="coinrun")
    rtgs, _, _, _, scale = O.preprocess_rtgs(arrays["ob_clip_reward"], arrays["done"], "coinrun", False)
    assert len(ds) == sum(LENS)
    clamped = set()
    for i in range(len(ds)):
        got, lit, ref = ds[i], ds.literal_item(i), O.getitem(arrays, i, T, rtgs, scale)
        for other in (lit, ref):
            assert np.array_equal(got["image"]["ob"], other["image"]["ob"]) and got["image"]["ob"].dtype == np.uint8
            assert np.array_equal(got["action"], other["action"])
        assert np.array_equal(got["rtg"]["ob"], ref["rtg"]["ob"]) and got["rtg"]["ob"].shape == (T, 1) and got["rtg"]["ob"].dtype == ref["rtg"]["ob"].dtype
        clamped.add(max(0, int(ds.traj_start[i]) - (i - T + 1)))  # window positions in front of the trajectory's first row
    assert clamped == {0, 1, 2, 3}
    assert ds.verify(8, seed=3)
    assert ds.get_traj_idx() == [int(v) for v in O.get_traj_idx(arrays["done"])]
    assert np.array_equal(ds.index_to_traj(), O.index_to_traj(arrays["done"]))


@pytest.mark.parametrize("kind", ["h5", "dict"])
def test_verify_fails_on_rows_that_are_not_recorder_stacked(tmp_path, kind):
    from arp_amd import _ffi, dataset
    arrays = O.recorder_arrays(LENS, seed=2)
    bad = {k: v.copy() for k, v in arrays.items()}
    row = sum(LENS) - 1  # the last row (always sampled): its older frames shuffled
    bad["ob"][row, F_OLD] = bad["ob"][row, F_OLD][::-1]
    store = _stores(tmp_path, bad)[kind]
    ds = dataset.ProcgenDataset(store, T, env_name="coinrun")
    assert not ds.verify(4, seed=0)
    with pytest.raises(_ffi.ArpError, match="recorder-stacked"):  # refused before anything touches a GPU
        dataset.DeviceDataset.load(ds)
    assert dataset.ProcgenDataset(_stores(tmp_path, arrays, name="good")[kind], T, env_name="coinrun").verify(4, seed=0)


F_OLD = slice(O.F - T, O.F - 1)  # the window's older frames of a stacked row


def test_num_frames_must_exceed_the_window(tmp_path):
    from arp_amd.dataset import ProcgenDataset
    arrays = O.recorder_arrays(LENS, seed=1)
    with pytest.raises(ValueError, match="stacked frames"):  # data_procgen.py:81-85
        ProcgenDataset(dict(arrays), O.F)
    assert ProcgenDataset(dict(arrays), O.F - 1, env_name="coinrun").window_size == O.F - 1


@pytest.mark.parametrize("use_normalize", [False, True])
@pytest.mark.parametrize("env_name", ["coinrun", "maze_aisc"])
@pytest.mark.parametrize("reward_name", ["ob_clip_reward", "ob_clip_pos_reward"])
def test_rtg_statistics_equal_the_restated_preprocessing(env_name, use_normalize, reward_name):
    from arp_amd.dataset import ProcgenDataset
    arrays = O.recorder_arrays([3, 11, 7, 20, 1, 6], seed=4, reward_name=reward_name)
    ds = ProcgenDataset(dict(arrays), T, env_name=env_name, use_normalize=use_normalize)
    rtgs, rmin, rmax, rtg0, scale = O.preprocess_rtgs(arrays[reward_name], arrays["done"], env_name, use_normalize)
    assert ds.reward_key == reward_name
    assert ds.reward_min == rmin and ds.reward_max == rmax and ds.return_to_go == rtg0 and ds.scale == scale
    assert np.array_equal(ds.rtg, rtgs[:, -1]) and ds.rtg.dtype == np.float32
    for i in (0, 2, 3, 5, 13, len(ds) - 1):
        assert np.array_equal(ds[i]["rtg"]["ob"], O.getitem(arrays, i, T, rtgs, scale)["rtg"]["ob"])


def test_reward_key_choice():
    from arp_amd.dataset import ProcgenDataset
    a = O.recorder_arrays(LENS, seed=5)
    both = dict(a, ob_clip_pos_reward=a["ob_clip_reward"] * 2, other=a["ob_clip_reward"] + 1)
    assert ProcgenDataset(both, T, env_name="coinrun").reward_key == "ob_clip_reward"  # the writer's name first
    assert ProcgenDataset(both, T, env_name="coinrun", reward_key="other").reward_key == "other"
    with pytest.raises(KeyError):
        ProcgenDataset({k: v for k, v in a.items() if "reward" not in k}, T, env_name="coinrun")
    bc = ProcgenDataset({k: v for k, v in a.items() if "reward" not in k}, T, env_name="coinrun", use_vl=False)  # BC reads no return-to-go
    assert bc.rtg is None and bc[3]["rtg"] == {}


@pytest.mark.parametrize("v", [0, 4, 5, 49, 50, 99, 100, 499, 500, -30, -70])
def test_compute_scale(v):
    from arp_amd.dataset import compute_scale
    assert compute_scale(v) == O.compute_scale(v) and compute_scale(float(v)) == O.compute_scale(float(v))


def test_len_and_process_index():
    from arp_amd.dataset import ProcgenDataset
    a = dict(O.recorder_arrays(LENS, seed=6))
    n = sum(LENS)
    assert len(ProcgenDataset(a, T, env_name="coinrun")) == n
    d = ProcgenDataset(a, T, env_name="coinrun", start_index=3)
    assert len(d) == n - 3 and d.process_index(0) == 3 and d.process_index(n - 3) == 3  # :176-178: modulo the length, then the offset
    assert np.array_equal(d[2]["image"]["ob"], a["ob"][5][-T:])
    d = ProcgenDataset(a, T, env_name="coinrun", max_length=7)
    assert len(d) == 7 and d.process_index(9) == 2
    d = ProcgenDataset(a, T, env_name="coinrun", start_index=2, max_length=100)
    assert len(d) == n - 2
    d = ProcgenDataset(a, T, env_name="coinrun", num_subset=3)  # :109-111: the first 3 trajectories of the training split
    assert len(d) == 1 + 2 + 5
    assert len(ProcgenDataset(a, T, env_name="coinrun", num_subset=3, split="val")) == n


def test_index_batches():
    from arp_amd.dataset import index_batches
    from arp_amd.train import shard_batch
    n, B = 20, 6
    a = [b["index"] for b in index_batches(n, B, seed=7, epochs=2)]
    b = [b["index"] for b in index_batches(n, B, seed=7, epochs=2)]
    c = [b["index"] for b in index_batches(n, B, seed=8, epochs=2)]
    assert len(a) == 6 and all(x.dtype == np.int64 and x.shape == (B,) for x in a)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and not all(np.array_equal(x, y) for x, y in zip(a, c))
    for ep in (a[:3], a[3:]):  # drop_last: 18 distinct rows of the epoch's permutation
        flat = np.concatenate(ep)
        assert len(set(flat.tolist())) == 18 and flat.min() >= 0 and flat.max() < n
    assert not np.array_equal(np.concatenate(a[:3]), np.concatenate(a[3:]))  # a fresh permutation per epoch
    full = [b["index"] for b in index_batches(n, B, seed=7, epochs=1, drop_last=False)]
    assert [len(x) for x in full] == [6, 6, 6, 2] and sorted(np.concatenate(full).tolist()) == list(range(n))
    assert np.array_equal(np.concatenate(full)[:18], np.concatenate(a[:3]))
    # world 2: every rank draws the same global batch; shard_batch cuts the two contiguous halves
    for rank in (0, 1):
        g = next(index_batches(n, B, seed=7, rank=rank, world=2))
        assert np.array_equal(g["index"], a[0])
        assert np.array_equal(shard_batch(g, rank, 2)["index"], a[0][rank * 3 : rank * 3 + 3])
    with pytest.raises(ValueError):
        next(index_batches(n, 5, seed=0, world=2))
    mapped = next(index_batches(n, B, seed=7, process_index=lambda i: i + 100))
    assert np.array_equal(mapped["index"], a[0] + 100)


def test_default_lut_is_byte_to_float_then_normalize():
    from arp_amd import dataset
    lut = dataset.default_lut()
    assert lut.shape == (3, 256) and lut.dtype == np.float32
    u = np.arange(256, dtype=np.uint8)
    for c, (m, s) in enumerate(zip(dataset.NORM_MEAN, dataset.NORM_STD)):
        want = (u.astype(np.float32) / np.float32(255) - np.float32(m)) / np.float32(s)  # ByteToFloat, Normalize (main_procgen.py:241,259-261)
        assert np.array_equal(lut[c], want)
    fr = np.random.default_rng(0).integers(0, 256, (2, 5, 5, 3), dtype=np.uint8)
    f = dataset.bytes_to_float(fr)
    assert f.dtype == np.float32 and all(np.array_equal(f[..., c], lut[c][fr[..., c]]) for c in range(3))
