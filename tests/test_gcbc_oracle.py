"""tests/gcbc_oracle.py pinned (no GPU): the goal-conditioned encoder oracle against oracle/m3ae_np.py, its frame / goal symmetry, and the seeded
hindsight-goal draw against a literal transcription of arp_dt/data_procgen.py:187-189."""
import numpy as np

import gcbc_oracle as G
from arp_amd import synth_policy as S
from oracle import m3ae_np as M

KW = dict(patch=16, width=64, layers=2, heads=2, img_res=64)


def _setup(n=3):
    cfg = M.EncConfig(**KW)
    P = S.m3ae_params(cfg, seed=5)
    return cfg, P, S.normalized_frames(n, cfg.img_res, seed=6), S.normalized_frames(n, cfg.img_res, seed=7)


def test_shared_blocks_reduce_to_the_plain_oracle():
    """the block function on the plain token sequence IS forward_representation (1e-12); and with the goal columns key-masked, rows 0..L of the gc
    sequence are forward_representation's rows"""
    cfg, P, x, goal = _setup()
    ref = M.forward_representation(P, cfg, x)
    L = cfg.tokens - 1
    cls = np.broadcast_to(np.asarray(P["cls_token"], np.float64), (x.shape[0], 1, cfg.width))
    plain = G.encode_tokens(P, cfg, np.concatenate([cls, G.embed_patches(P, cfg, x)], axis=1))
    assert plain.shape == ref.shape and np.abs(plain - ref).max() < 1e-12
    mask = np.arange(2 * L + 1) <= L
    masked = G.encode_tokens(P, cfg, G.gc_tokens(P, cfg, x, goal), key_mask=mask)
    assert np.abs(masked[:, :L + 1] - ref).max() < 1e-12


def test_swapping_frame_and_goal_swaps_the_patch_blocks():
    """both patch blocks carry the same position and type embedding and no key is masked: attention is permutation-equivariant"""
    cfg, P, x, goal = _setup()
    L = cfg.tokens - 1
    a = G.forward_gc_representations(P, cfg, x, goal)
    b = G.forward_gc_representations(P, cfg, goal, x)
    assert a.shape == (x.shape[0], 2 * L + 1, cfg.width)
    assert np.abs(a[:, 0] - b[:, 0]).max() < 1e-12
    assert np.abs(a[:, 1:L + 1] - b[:, L + 1:]).max() < 1e-12 and np.abs(a[:, L + 1:] - b[:, 1:L + 1]).max() < 1e-12
    assert np.abs(a[:, 1:L + 1] - a[:, L + 1:]).max() > 1e-3   # and the two blocks are not the same thing


def _synthetic_set(n_rows=60, stack=4, res=8, ends=(17, 41, 59)):
    """three finished trajectories (the last done flag on the last row), recorder-stacked rows"""
    rng = np.random.default_rng(0)
    last = rng.integers(0, 255, (n_rows, res, res, 3), dtype=np.uint8)
    done = np.zeros(n_rows, bool)
    done[list(ends)] = True
    start = np.zeros(n_rows, np.int64)
    s = 0
    for i in range(n_rows):
        start[i] = s
        if done[i]:
            s = i + 1
    src = np.maximum(np.arange(n_rows)[:, None] - np.arange(stack - 1, -1, -1)[None, :], start[:, None])
    act = rng.integers(0, 15, n_rows)
    return {"ob": last[src], "done": np.repeat(done[:, None], stack, 1), "act": act[src]}


def test_seeded_goal_rows_are_the_reference_draws():
    """200 indices: ProcgenDataset.goal_row and gcbc_oracle.goal_row against the three lines of data_procgen.py written out with numpy's global generator"""
    from arp_amd.dataset import ProcgenDataset
    store = _synthetic_set()
    ds = ProcgenDataset(store, 3, use_vl=False, goal_rng=np.random.RandomState(11))
    h5_file_traj_idx, idx_to_traj, n_rows = ds.h5_file_traj_idx, ds.idx_to_traj, store["ob"].shape[0]
    idx = np.random.default_rng(1).integers(0, n_rows, 200)
    idx[:3] = (n_rows - 1, 17, 0)   # the last row (the only candidate is the row the clamp names), a trajectory's last row, the first row
    np.random.seed(11)
    want = []
    for index in idx:
        subsequent_indices = list(range(index, h5_file_traj_idx[idx_to_traj[index] + 1]))
        goal_indices = np.random.choice(subsequent_indices, 1).item()
        want.append(min(goal_indices, store["ob"].shape[0] - 1))
    got = [ds.goal_row(int(i)) for i in idx]
    rs = np.random.RandomState(11)
    oracle = [G.goal_row(rs, int(i), h5_file_traj_idx[idx_to_traj[i] + 1], n_rows) for i in idx]
    assert got == want == oracle
    assert want[0] == n_rows - 1 and want[1] == 17 and all(i <= g < h5_file_traj_idx[idx_to_traj[i] + 1] for i, g in zip(idx, want))
    # an item carries the goal row's window under "goal"
    ds3 = ProcgenDataset(store, 3, use_vl=False, goal_rng=np.random.RandomState(5))
    g = np.random.RandomState(5).choice(list(range(20, 42)), 1).item()
    assert np.array_equal(ds3[20]["goal"]["ob"], ds3.last_frames(ds3.window_rows(g))) and ds3[20]["goal"]["ob"].shape == ds3[20]["image"]["ob"].shape


def test_goal_row_clamp_bites_when_the_frames_end_before_the_flags():
    """The clamp of data_procgen.py:189 is to the IMAGE dataset's last row, while the trajectory ends come from the done flags.  In a whole file both have the
    same length and the clamp never moves a draw (the test above); it bites when "ob" holds fewer rows than "done" -- here the last two rows' frames are
    missing -- and a draw lands behind the last frame row.  A goal_row without the clamp fails this test."""
    from arp_amd.dataset import ProcgenDataset
    store = _synthetic_set()
    store["ob"] = store["ob"][:-2]
    n_ob = store["ob"].shape[0]
    ds = ProcgenDataset(store, 3, use_vl=False, goal_rng=np.random.RandomState(3))
    h5_file_traj_idx, idx_to_traj = ds.h5_file_traj_idx, ds.idx_to_traj
    assert h5_file_traj_idx[-1] == 60 and n_ob == 58
    idx = np.random.default_rng(2).integers(42, n_ob, 80)   # rows of the last trajectory, whose end (60) lies behind the last frame row (57)
    np.random.seed(3)
    want, raw = [], []
    for index in idx:
        subsequent_indices = list(range(index, h5_file_traj_idx[idx_to_traj[index] + 1]))
        goal_indices = np.random.choice(subsequent_indices, 1).item()
        raw.append(goal_indices)
        want.append(min(goal_indices, store["ob"].shape[0] - 1))
    rs = np.random.RandomState(3)
    assert [ds.goal_row(int(i)) for i in idx] == want == [G.goal_row(rs, int(i), h5_file_traj_idx[idx_to_traj[i] + 1], n_ob) for i in idx]
    assert max(raw) >= n_ob and max(want) == n_ob - 1, "no draw landed behind the last frame row: the clamp was not exercised"
