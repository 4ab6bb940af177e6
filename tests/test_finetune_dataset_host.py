"""arp_amd.finetune_data.ProcgenActionDataset against what the reference class read and returned (tests/golden/finetune_dataset.npz, written by
tests/golden/make_golden_finetune_dataset.py from the reference class itself).  No GPU.  Every comparison is exact: integers."""
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(__file__), "golden", "finetune_dataset.npz")
STACK = 2


def _store(done, act):
    """The generator's set rebuilt from the recorded ``done`` / ``act``: row i's last frame holds i in every byte."""
    n = done.shape[0]
    ends = np.nonzero(done[:, -1])[0] + 1
    b = np.concatenate([[0], ends])
    start = b[np.searchsorted(b, np.arange(n), side="right") - 1]
    src = np.maximum(np.arange(n)[:, None] - np.arange(STACK - 1, -1, -1)[None, :], start[:, None])
    ob = np.broadcast_to(src[:, :, None, None, None].astype(np.uint8), (n, STACK, 2, 2, 3)).copy()
    return {"ob": ob, "act": act, "done": done}


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _open(gold, name, **kw):
    from arp_amd.finetune_data import ProcgenActionDataset
    ratio = float(gold[f"{name}/start_offset_ratio"])
    return ProcgenActionDataset(_store(gold[f"{name}/done"], gold[f"{name}/act"]), start_index=int(gold[f"{name}/start_index"]),
                                max_length=int(gold[f"{name}/max_length"]), start_offset_ratio=None if np.isnan(ratio) else ratio, env_name="coinrun", **kw)


NAMES = ["tail", "tail_start3", "tail_ratio", "tail_max7", "closed"]


def test_fixture_holds_the_sets_the_issue_names(gold):
    assert list(gold["names"]) == NAMES
    assert gold["tail/done"].shape[0] == 13 and list(np.nonzero(gold["tail/done"][:, -1])[0] + 1) == [1, 3, 8, 11]
    assert list(gold["closed/traj_idx"])[-1] == gold["closed/done"].shape[0]  # no tail rows
    assert int(gold["tail_start3/start_index"]) == 3 and int(gold["tail_max7/max_length"]) == 7 and float(gold["tail_ratio/start_offset_ratio"]) == 0.4
    # the quirk rows are where the sort matters: row i moves behind trajectory 0's last row
    assert gold["tail/rows"][11].tolist() == [0, 0, 0, 11] and gold["tail/r"][11] == 0
    # a length-1 trajectory: four equal rows, r = 1; a length-2 trajectory: r = 1 at both rows
    assert gold["tail/rows"][0].tolist() == [0, 0, 0, 0] and gold["tail/r"][:3].tolist() == [1, 1, 1]


@pytest.mark.parametrize("name", NAMES)
def test_len_traj_idx_process_index(gold, name):
    ds = _open(gold, name)
    assert len(ds) == int(gold[f"{name}/len"])
    assert ds.get_traj_idx() == [int(v) for v in gold[f"{name}/traj_idx"]]
    assert [ds.process_index(i) for i in range(len(ds))] == gold[f"{name}/process_index"].tolist()
    assert ds.num_actions == int(gold[f"{name}/num_actions"])
    assert ds.env_name == str(gold[f"{name}/env_name"])
    assert ds.instruct == str(gold["prompt"])


@pytest.mark.parametrize("name", NAMES)
def test_items_equal_the_reference(gold, name):
    ds = _open(gold, name, tokens=np.full((1, 77), 7, np.int32))
    rows, r, action = gold[f"{name}/rows"], gold[f"{name}/r"], gold[f"{name}/action"]
    for i in range(len(ds)):
        assert ds.quad(i) == rows[i].tolist()
        item = ds[i]
        assert sorted(item) == ["action", "image0", "image1", "image2", "image3", "instruct", "r"]
        for g in range(4):
            fr = item[f"image{g}"]["ob"]
            assert fr.dtype == np.uint8 and fr.shape == (2, 2, 3) and (fr == rows[i, g]).all()
        assert item["r"].shape == (1,) and item["r"].dtype.kind == "i" and int(item["r"][0]) == int(r[i])
        assert int(item["action"]) == int(action[i])
        assert item["instruct"].shape == (1, 77)
    assert "instruct" not in _open(gold, name)[0]  # no tokens, no tokenizer: no BPE vocabulary ships with the package


@pytest.mark.parametrize("name", NAMES)
def test_quads_vectorised(gold, name):
    ds = _open(gold, name)
    q, r, arow = ds.quads(range(len(ds)))
    assert q.dtype == np.int32 and r.dtype == np.int32 and arow.dtype == np.int32
    assert q.shape == (len(ds), 4) and r.shape == (len(ds),) and arow.shape == (len(ds),)
    assert np.array_equal(q, gold[f"{name}/rows"])
    assert np.array_equal(r, gold[f"{name}/r"])
    assert np.array_equal(arow, q[:, 0])
    assert np.array_equal(ds.action[arow].astype(np.int64), gold[f"{name}/action"].astype(np.int64))
    # processed rows in: the same quads
    q2, r2, a2 = ds.quads_of_rows(gold[f"{name}/process_index"])
    assert np.array_equal(q2, q) and np.array_equal(r2, r) and np.array_equal(a2, arow)


@pytest.mark.parametrize("name", NAMES)
def test_bounds_reproduce_every_quad(gold, name):
    ds = _open(gold, name)
    first, last = ds.bounds()
    assert first.dtype == np.int32 and last.dtype == np.int32 and first.shape == (ds.n_rows,) and last.shape == (ds.n_rows,)
    assert (0 <= first).all() and (first <= last).all() and (last < ds.n_rows).all()
    i = gold[f"{name}/process_index"].astype(np.int64)
    four = np.sort(np.stack([first[i], i, np.minimum(i + 1, last[i]), last[i]], axis=1), axis=1)
    assert np.array_equal(four, gold[f"{name}/rows"])
    assert np.array_equal((four[:, 2] == four[:, 3]).astype(np.int32), gold[f"{name}/r"])


def test_quirk_rows_are_outside_their_bounds(gold):
    ds = _open(gold, "tail")
    first, last = ds.bounds()
    assert first[11:].tolist() == [0, 0] and last[11:].tolist() == [0, 0]  # trajectory 0's interval, which does not contain rows 11 and 12
    assert ds.idx_to_traj.tolist() == [0, 1, 1, 2, 2, 2, 2, 2, 3, 3, 3, 0, 0]


def test_two_image_keys_on_the_host(gold):
    from arp_amd.finetune_data import ProcgenActionDataset
    s = _store(gold["tail/done"], gold["tail/act"])
    s["ob2"] = 255 - s["ob"]
    item = ProcgenActionDataset(s, image_key="ob, ob2", env_name="coinrun")[4]
    q = gold["tail/rows"][4]
    for g in range(4):
        assert (item[f"image{g}"]["ob"] == q[g]).all() and (item[f"image{g}"]["ob2"] == 255 - q[g]).all()


def test_env_name_suffixes_and_attribute(gold):
    from arp_amd.finetune_data import ProcgenActionDataset

    class Store(dict):
        attrs = {"env_name": b"maze"}

    s = Store(_store(gold["closed/done"], gold["closed/act"]))
    assert ProcgenActionDataset(s).env_name == "maze"
    ds = ProcgenActionDataset(s, env_type="aisc")
    assert ds.env_name == "maze_aisc" and ds.instruct == "navigate a maze to collect the yellow cheese."


def test_no_done_flag_raises_as_the_reference(gold):
    from arp_amd.finetune_data import ProcgenActionDataset
    assert str(gold["nodone/raises"]) == "IndexError"
    done = np.zeros((4, STACK), np.uint8)
    ds = ProcgenActionDataset(_store(done, np.zeros((4, STACK), np.int64)), env_name="coinrun")
    with pytest.raises(IndexError):
        ds[0]
    with pytest.raises(IndexError):
        ds.quads([0])
    with pytest.raises(IndexError):
        ds.bounds()
    s = _store(done, np.zeros((4, STACK), np.int64))
    del s["done"]
    with pytest.raises(KeyError):  # no `done` dataset at all: the reference's h5_file["done"]
        ProcgenActionDataset(s, env_name="coinrun")
