"""The (row, goal row) pair stream of model GCBC's device-resident feed (arp_amd/dataset.py::index_batches with a goal draw): needs no GPU."""
import itertools

import numpy as np

import dataset_oracle as O

LENS = [1, 2, 7, 14]  # tests/test_dataset_gpu.py's set: 24 rows, trajectories starting at rows 0, 1, 3 and 10
ENDS = np.repeat([1, 3, 10, 24], LENS)  # one past the last row of each row's trajectory
T, B = 3, 4


def _pairs(seed, goal_seed, n_batches=12):
    from arp_amd import dataset
    pd = dataset.ProcgenDataset(dict(O.recorder_arrays(LENS, hw=16, seed=11)), T, env_name="coinrun")
    rng = np.random.RandomState(goal_seed)
    it = dataset.index_batches(len(pd), B, seed, process_index=pd.process_index, goal_row=lambda i: pd.goal_row(i, rng))
    return pd, list(itertools.islice(it, n_batches))  # 12 batches of 4 over 24 rows: two epochs


def test_pair_stream_is_deterministic_in_both_seeds():
    same = lambda a, b: all(np.array_equal(x["index"], y["index"]) and np.array_equal(x["goal_index"], y["goal_index"]) for x, y in zip(a, b))  # noqa: E731
    a, b = _pairs(3, 7)[1], _pairs(3, 7)[1]
    assert len(a) == 12 and same(a, b)
    assert not same(a, _pairs(3, 8)[1])  # another goal seed: other goals ...
    assert all(np.array_equal(x["index"], y["index"]) for x, y in zip(a, _pairs(3, 8)[1]))  # ... for the same rows
    assert not all(np.array_equal(x["index"], y["index"]) for x, y in zip(a, _pairs(4, 7)[1]))


def test_pair_stream_keeps_the_plain_index_stream_and_its_keys():
    from arp_amd import dataset
    from arp_amd.train import is_index_batch, is_index_pair_batch
    pd, pairs = _pairs(3, 7)
    plain = list(itertools.islice(dataset.index_batches(len(pd), B, 3, process_index=pd.process_index), 12))
    for p, q in zip(pairs, plain):
        assert set(q) == {"index"} and set(p) == {"index", "goal_index"}
        assert np.array_equal(p["index"], q["index"]) and p["goal_index"].dtype == np.int64 and p["goal_index"].shape == (B,)
        assert is_index_pair_batch(p) and not is_index_batch(p)
        assert is_index_batch(q) and not is_index_pair_batch(q)
    assert not is_index_pair_batch({"index": 0, "goal_index": 0, "action": 0}) and not is_index_pair_batch({"goal_index": 0})


def test_goals_follow_the_hindsight_rule_in_sequential_order():
    from arp_amd import dataset
    pd, pairs = _pairs(3, 7)
    seen = set()
    for p in pairs:
        for i, g in zip(p["index"], p["goal_index"]):
            assert i <= g < ENDS[i], (i, g)
            seen.add(int(g) - int(i))
    assert len(seen) > 3  # drawn, not a constant offset
    # one draw per batch position, in batch order: what a sequential [pd[i] for i in index] consumes from the same generator
    seq = dataset.ProcgenDataset(dict(O.recorder_arrays(LENS, hw=16, seed=11)), T, env_name="coinrun", goal_rng=np.random.RandomState(7))
    for p in pairs:
        for i, g in zip(p["index"], p["goal_index"]):
            want = seq.last_frames(seq.window_rows(int(g)))
            assert np.array_equal(seq[int(i)]["goal"]["ob"], want)


def test_shard_batch_cuts_both_arrays_at_the_same_place():
    from arp_amd.train import is_index_pair_batch, shard_batch
    _, pairs = _pairs(3, 7, n_batches=2)
    for p in pairs:
        parts = [shard_batch(p, r, 2) for r in range(2)]
        assert all(is_index_pair_batch(q) for q in parts)
        for r, q in enumerate(parts):
            assert np.array_equal(q["index"], p["index"][2 * r : 2 * r + 2]) and np.array_equal(q["goal_index"], p["goal_index"][2 * r : 2 * r + 2])
