"""arp_amd/train.py::classify_batch -- the one place that decides what kind of batch a dict is -- on the dict shapes the reference's loader
(main_procgen.py:693-701) and the device-resident set's index_batches produce.  Needs no GPU."""
import itertools

import numpy as np
import pytest

B, T, TOK, DIM, HW = 2, 3, 5, 8, 16


def _host_batch(image, goal=True, rtg_views=("ob",)):
    """generate_batch's dict: per-image-key dicts, and the keys this project never reads beside them"""
    rs = np.random.RandomState(1)
    return {"image": {"ob": image}, "goal": {"ob": rs.rand(B, T, HW, HW, 3).astype(np.float32)} if goal else None, "state": None,
            "action": rs.randint(0, 15, (B, T)), "rtg": {k: (10.0 * rs.randn(B, T, 1)).astype(np.float32) for k in rtg_views},
            "instruct": None, "text_padding_mask": None}


FRAMES = np.random.RandomState(2).rand(B, T, HW, HW, 3).astype(np.float32)
ENCODINGS = np.random.RandomState(3).randn(B, T, TOK, DIM).astype(np.float32)


def _index_streams():
    from arp_amd import dataset
    plain = next(dataset.index_batches(24, B, 3))
    pairs = next(dataset.index_batches(24, B, 3, goal_row=lambda i: min(i + 1, 23)))
    return plain, pairs


@pytest.mark.parametrize("kind, encoder, gcbc", [("encodings", False, False), ("encodings", True, False), ("frames", True, False), ("frames+goals", True, True),
                                                 ("index", True, False), ("index_pairs", True, True)])
def test_each_kind_is_recognised_and_carries_its_arrays(kind, encoder, gcbc):
    from arp_amd.train import classify_batch
    plain, pairs = _index_streams()
    batch = {"encodings": _host_batch(ENCODINGS), "frames": _host_batch(FRAMES), "frames+goals": _host_batch(FRAMES), "index": plain, "index_pairs": pairs}[kind]
    b = classify_batch(batch, encoder=encoder, gcbc=gcbc)
    assert b.kind == kind
    if kind.startswith("index"):
        assert np.array_equal(b.index, batch["index"]) and b.image is None and b.action is None and b.rtg is None and b.goals is None
        assert (b.goal_index is None) if kind == "index" else np.array_equal(b.goal_index, batch["goal_index"])
        return
    assert b.image is batch["image"]["ob"] and np.array_equal(b.action, batch["action"]) and b.index is None and b.goal_index is None
    assert np.array_equal(b.rtg, batch["rtg"]["ob"])
    assert (b.goals is batch["goal"]["ob"]) if kind == "frames+goals" else b.goals is None


def test_goal_is_read_by_gcbc_alone_and_only_beside_frames():
    from arp_amd.train import classify_batch
    assert classify_batch(_host_batch(FRAMES), encoder=True, gcbc=False).kind == "frames"       # the loader puts "goal" in every batch
    assert classify_batch(_host_batch(FRAMES), encoder=True, gcbc=False).goals is None
    assert classify_batch(_host_batch(FRAMES, goal=False), encoder=True, gcbc=True).kind == "frames"  # "goal": None -- staging refuses it, not the classifier
    b = classify_batch(_host_batch(ENCODINGS), encoder=True, gcbc=True)  # GCBC on encodings of pairs: nothing left to pair
    assert b.kind == "encodings" and b.goals is None


def test_five_dimensional_arrays_are_frames_only_behind_an_encoder():
    from arp_amd.train import classify_batch
    for gcbc in (False, True):
        b = classify_batch(_host_batch(FRAMES), encoder=False, gcbc=gcbc)
        assert b.kind == "encodings" and b.image is not None and b.goals is None
    five_d = np.zeros((B, T, HW, HW, 4), np.float32)  # five axes, but no RGB last axis
    assert classify_batch(_host_batch(five_d), encoder=True, gcbc=False).kind == "encodings"


def test_rtg_is_the_view_mean_with_symlog_applied_once():
    from arp_amd.train import classify_batch, symlog
    batch = _host_batch(ENCODINGS, rtg_views=("ob", "ob2"))
    views = np.stack([batch["rtg"]["ob"], batch["rtg"]["ob2"]])
    keep = {k: v.copy() for k, v in batch["rtg"].items()}
    plain = classify_batch(batch, encoder=False, gcbc=False).rtg
    logged = classify_batch(batch, encoder=False, gcbc=False, use_symlog=True).rtg
    assert np.array_equal(plain, views.mean(0))
    want = (np.sign(views) * np.log1p(np.abs(views))).mean(0)
    assert np.array_equal(logged, want) and not np.array_equal(logged, symlog(want))  # once: each view, then the mean -- not again on the result
    assert np.abs(views).max() > 3 and not np.allclose(logged, plain)                   # (the data tells the two apart)
    assert all(np.array_equal(batch["rtg"][k], keep[k]) for k in keep)                  # the caller's arrays are left alone
    no_rtg = {k: v for k, v in _host_batch(ENCODINGS).items() if k != "rtg"}            # model BC's batch
    assert classify_batch(no_rtg, encoder=False, gcbc=False, use_symlog=True).rtg is None


def test_an_index_dict_with_a_stray_key_is_no_index_batch():
    from arp_amd.train import classify_batch
    plain, pairs = _index_streams()
    for stray in ({**plain, "action": np.zeros((B, T), np.int64)}, {**pairs, "action": np.zeros((B, T), np.int64)}, {"goal_index": pairs["goal_index"]}):
        with pytest.raises(KeyError):  # read as the reference's dict, which it is not: no "image"
            classify_batch(stray, encoder=True, gcbc=True)
    b = classify_batch({**_host_batch(ENCODINGS), "index": plain["index"]}, encoder=True, gcbc=False)
    assert b.kind == "encodings" and b.index is None


def test_index_streams_classify_batch_after_batch():
    from arp_amd import dataset
    from arp_amd.train import classify_batch, shard_batch
    for p in itertools.islice(dataset.index_batches(24, 4, 5, goal_row=lambda i: i), 3):
        for r in range(2):  # cut to a rank first, as the step functions and the prefetcher do
            b = classify_batch(shard_batch(p, r, 2), encoder=True, gcbc=True)
            assert b.kind == "index_pairs" and np.array_equal(b.index, p["index"][2 * r: 2 * r + 2]) and np.array_equal(b.goal_index, b.index)
