"""Oracle (test infrastructure) of the demonstration set: the reference's ProcgenDataset (/root/reference/arp_dt/data_procgen.py) read LITERALLY --
the stacked rows themselves, ``ob[i][-T:]`` -- plus a line-cited restatement of ``preprocess_rtgs`` (:132-174) and ``compute_scale``
(arp_dt/utils.py:453-463).  Imports nothing from arp_amd/dataset.py; builds the recorder-style stores the tests read.
"""
from collections import deque

import numpy as np

F = 8  # trajectory_recorder.py's num_frames (and config.num_frames, data_procgen.py:23)


def stack(x):
    """stack_frames (data/PPG/trajectory_recorder.py:103-112) over one trajectory: row i = the last F items up to i, the first one left-padded."""
    idx = np.clip(np.arange(len(x))[:, None] + np.arange(-F + 1, 1)[None, :], 0, None)
    return x[idx]


def recorder_arrays(lens, hw=16, seed=0, n_actions=15, reward_name="ob_clip_reward"):
    """Stacked ``ob`` / ``act`` / ``done`` / reward arrays of trajectories of the given lengths, as the recorder and the labelling pass write them."""
    rng = np.random.default_rng(seed)
    ob, act, done, rew = [], [], [], []
    for L in lens:
        fr = rng.integers(0, 256, (L, hw, hw, 3), dtype=np.uint8)
        a = rng.integers(0, n_actions, L).astype(np.int64)
        r = (rng.random(L) * 60 - 5).astype(np.float32)
        d = np.zeros(L, np.float32)
        d[-1] = 1
        ob.append(stack(fr)); act.append(stack(a)); done.append(stack(d)); rew.append(stack(r))
    return {"ob": np.concatenate(ob), "act": np.concatenate(act), "done": np.concatenate(done), reward_name: np.concatenate(rew)}


def write_h5(path, arrays, env_name="coinrun"):
    """The arrays as a recorder-style file: gzip chunks of one row."""
    from arp_amd import h5store
    with h5store.H5Store(path, "w") as f:
        f.attrs["env_name"] = env_name
        for k, v in arrays.items():
            f.create_dataset(k, data=v, compression="gzip", chunks=(1,) + v.shape[1:], maxshape=(None,) + v.shape[1:])


def get_traj_idx(done):
    """data_procgen.py:118-121"""
    idx = list(np.nonzero(done[:, -1])[0] + 1)
    idx.insert(0, 0)
    return idx


def index_to_traj(done):
    """data_procgen.py:123-130"""
    b = get_traj_idx(done)
    out = np.zeros_like(done[:, -1], dtype=np.int32)
    for i in range(len(b) - 1):
        out[list(range(b[i], b[i + 1]))] = i
    return out


def compute_scale(return_to_go):
    """arp_dt/utils.py:453-463"""
    if return_to_go >= 0:
        max_digit = int(str(int(return_to_go))[0])  # :455
    else:
        max_digit = int(str(int(return_to_go))[1])  # :457
    if return_to_go >= 0:
        n = len(str(int(return_to_go))) - 1 if max_digit < 5 else len(str(int(return_to_go)))  # :460
    else:
        n = len(str(int(return_to_go))) - 2 if max_digit < 5 else len(str(int(return_to_go))) - 1  # :462
    return pow(10, n)


def preprocess_rtgs(reward_stacked, done, env_name, use_normalize, num_frames=F):
    """data_procgen.py:132-174 for one image key.  Returns (stacked rtgs [n, num_frames], reward_min, reward_max, return_to_go, scale)."""
    def discount_cumsum(x, gamma):  # :133-138
        out = np.zeros_like(x)
        out[-1] = x[-1]
        for t in reversed(range(x.shape[0] - 1)):
            out[t] = x[t] + gamma * out[t + 1]
        return out

    reward = reward_stacked[:, -1].astype(np.float32)  # :141
    reward_min, reward_max = np.min(reward), np.max(reward)  # :144-145
    modified = reward - reward_min if use_normalize else reward  # :147-150
    b = get_traj_idx(done)
    rtgs = []
    for idx in range(len(b) - 1):  # :155-164
        st = deque([], maxlen=num_frames)
        rows = list(range(b[idx], b[idx + 1]))
        cs = discount_cumsum(modified[rows], gamma=1.0)
        for i in range(len(rows)):
            if i == 0:
                st.extend([cs[i]] * num_frames)
            else:
                st.append(cs[i])
            rtgs.append(np.stack(st))
    if "coinrun" in env_name:  # :168-171 (the statistic runs over the list of stacked rows)
        return_to_go = np.max([rtgs]) // 100 * 100
    else:
        return_to_go = np.quantile([rtgs], 0.9) // 100 * 100
    scale = compute_scale(return_to_go)  # :172
    return np.asarray(rtgs), reward_min, reward_max, return_to_go, scale


def getitem(arrays, i, T, rtgs=None, scale=None, key="ob"):
    """data_procgen.py:180-213 for one image key, without goal / state / instruction: the stacked rows read literally."""
    res = {"image": {key: np.asarray(arrays[key][i])[-T:]}, "rtg": {}, "action": np.asarray(arrays["act"][i])[-T:]}  # :184,207
    if rtgs is not None:
        res["rtg"][key] = rtgs[i][-T:][..., None] / scale  # :200
    return res
