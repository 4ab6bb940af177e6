"""The demonstration set of the policy trainer: the reference's ``ProcgenDataset`` on the host, and its mirror in HBM.

Mirrors /root/reference/arp_dt/data_procgen.py:58-213 (the deterministic parts):
  * :class:`ProcgenDataset` -- ``get_traj_idx`` / ``index_to_traj`` (:118-130), ``__len__`` (:108-116), ``process_index`` (:176-178),
    ``preprocess_rtgs`` (:132-174) with ``compute_scale`` (arp_dt/utils.py:453-463), ``__getitem__`` (:180-213) for one image key:
    ``{"image": {key: uint8 [T, H, W, 3]}, "rtg": {key: f32 [T, 1]}, "action": [T]}``.
  * :class:`DeviceDataset` -- the same set resident on the GPU; a batch is ``{"index": int64[B]}`` and HIP kernels assemble the
    window batch straight into one of the trainer's batch slots (``PolicyTrainer.attach_dataset``): no frame crosses PCIe after the load.

The window rule.  The recorder builds every row with ``stack_frames`` (data/PPG/trajectory_recorder.py:103-112): row ``i`` holds the last
``num_frames`` items of its trajectory, the first one left-padded, so ``ob[i, -1]`` is the only frame row ``i`` adds and

    ob[i][-T:][t] == ob[j(t), -1],   j(t) = max(i - (T - 1 - t), s[i]),   t = 0..T-1,   s[i] = first row of i's trajectory

(likewise ``act`` and the stacked returns-to-go).  ``__getitem__`` is built from the per-row values by that rule; ``literal_item`` reads the
stacked rows themselves and ``verify`` compares the two on sampled rows -- ``DeviceDataset.load`` refuses a file that fails it.

Goal frames (model GCBC).  The hindsight goal of row ``i`` is one RNG draw over the rows from ``i`` to the end of its trajectory
(``ProcgenDataset.goal_row``, data_procgen.py:186-189) and its frames are ``ob[g][-T:]``: the window of row ``g`` under the same rule.  The draw stays on
the host -- ``DeviceDataset.index_batches(goal_rng=...)`` yields ``{"index", "goal_index"}`` pair batches, drawn in the order a sequential host loader
draws -- and one gather launch fills a slot's frames and goal frames from the set in HBM (``PolicyTrainer.set_batch_index_pairs`` /
``upload_index_pairs_async``).  A pair's encoding is not a per-row quantity: there is no encodings cache for it.

Not here: ``use_task_reward``, ``state``, several image keys, the BERT tokenizer, ``random_start``.  There is no CPU fallback for the device side:
the gathers are in libarp_hip.so.
"""
import ctypes as C
import os
import weakref

import numpy as np

from . import _ffi
from ._ffi import ArpError, check, lib

# main_procgen.py:259-261 (and :291-292): augmax.Normalize behind augmax.ByteToFloat
NORM_MEAN = (0.5762, 0.5503, 0.5213)
NORM_STD = (0.3207, 0.3169, 0.3307)


def default_lut():
    """f32 [3, 256]: ``ByteToFloat`` (``x / 255``) then ``Normalize(mean, std)`` (main_procgen.py:241,259-261) of every byte value per channel, in
    f32 numpy.  The frame gather writes exactly ``lut[c][u]``, and :func:`bytes_to_float` is the host path through the same table."""
    u = np.arange(256, dtype=np.float32) / np.float32(255)
    mean, std = np.asarray(NORM_MEAN, np.float32), np.asarray(NORM_STD, np.float32)
    return np.ascontiguousarray(((u[None, :] - mean[:, None]) / std[:, None]).astype(np.float32))


def bytes_to_float(frames_u8, lut=None):
    """uint8 ``[..., 3]`` -> f32 through the table: ``lut[c][u]`` per channel (what the device gather writes)."""
    lut = default_lut() if lut is None else np.asarray(lut, np.float32)
    f = np.asarray(frames_u8)
    if f.dtype != np.uint8 or f.shape[-1] != 3:
        raise ValueError("frames must be uint8 [..., 3]")
    return np.stack([lut[c][f[..., c]] for c in range(3)], axis=-1)


def compute_scale(return_to_go):
    """arp_dt/utils.py:453-463: a power of ten from the leading digit and the digit count of ``int(return_to_go)``."""
    s = str(int(return_to_go))
    neg = not (return_to_go >= 0)
    max_digit = int(s[1]) if neg else int(s[0])
    digits = len(s) - 1 if neg else len(s)
    n = digits - 1 if max_digit < 5 else digits
    return pow(10, n)


def _discount_cumsum(x, gamma):
    out = np.zeros_like(x)
    out[-1] = x[-1]
    for t in reversed(range(x.shape[0] - 1)):
        out[t] = x[t] + gamma * out[t + 1]
    return out


class ProcgenDataset:
    """The reference class's deterministic core over an :class:`arp_amd.h5store.H5Store`, a path to one, or a plain dict of arrays."""

    def __init__(self, store_or_path, window_size, image_key="ob", vl_type="clip", *, env_name=None, use_vl=True, use_normalize=False,
                 start_index=0, max_length=int(1e9), num_subset=-1, split="train", num_frames=None, reward_key=None, goal_rng=None):
        # goal_rng: a numpy.random.RandomState -> items carry the hindsight goal of data_procgen.py:186-189 under "goal" (GCBC's batch dict)
        self.goal_rng = goal_rng
        self._own = False
        if isinstance(store_or_path, (str, os.PathLike)):
            from . import h5store
            store_or_path = h5store.H5Store(os.fspath(store_or_path), "r")
            self._own = True
        self.store = store_or_path
        if ", " in image_key:
            raise ValueError("one image key (several are out of scope here)")
        self.image_key, self.vl_type, self.split = image_key, vl_type, split
        self.start_index, self.max_length, self.num_subset = int(start_index), int(max_length), int(num_subset)
        self.use_vl, self.use_normalize = bool(use_vl), bool(use_normalize)
        ob = self.store[image_key]
        self.n_rows = int(ob.shape[0])
        self.file_num_frames = int(ob.shape[1])
        self.frame_shape = tuple(int(v) for v in ob.shape[2:])
        if not self.file_num_frames > int(window_size):  # data_procgen.py:81-85
            raise ValueError(f"this file have {self.file_num_frames} stacked frames <= window_size {window_size}")
        self.window_size = int(window_size)
        self.num_frames = int(num_frames) if num_frames is not None else self.file_num_frames  # config.num_frames: the depth of the stacked returns
        if env_name is None:
            attrs = getattr(self.store, "attrs", None)
            env_name = attrs.get("env_name", "") if attrs is not None else ""
            env_name = env_name.decode() if isinstance(env_name, bytes) else str(env_name)
        self.env_name = env_name
        self.random_start_offset = 0
        done_last = np.asarray(self.store["done"][:, -1])
        self.h5_file_traj_idx = self.get_traj_idx(done_last)
        self.idx_to_traj = self.index_to_traj(done_last)
        # per-row values: s[j] (rows behind the last done flag form an unfinished trajectory of their own), a[j], R[j]
        bounds = np.asarray(self.h5_file_traj_idx, np.int64)
        self.traj_start = bounds[np.searchsorted(bounds, np.arange(self.n_rows), side="right") - 1].astype(np.int32)
        self.action = np.ascontiguousarray(np.asarray(self.store["act"][:, -1])).astype(np.int32)
        self.reward_key = None
        self.rtg = None
        if self.use_vl:
            self.reward_key = self._find_reward_key(reward_key)
            self.rtg = self.preprocess_rtgs()

    # -- data_procgen.py:118-130 ---------------------------------------------------------------------------------------------------
    def get_traj_idx(self, done_last=None):
        done_last = np.asarray(self.store["done"][:, -1]) if done_last is None else done_last
        return [0] + [int(v) for v in np.nonzero(done_last)[0] + 1]

    def index_to_traj(self, done_last=None):
        b = self.get_traj_idx(done_last)
        out = np.zeros(self.n_rows, np.int32)
        for t in range(len(b) - 1):
            out[b[t] : b[t + 1]] = t
        return out

    # -- data_procgen.py:108-116, 176-178 ------------------------------------------------------------------------------------------
    def __len__(self):
        if self.split == "train" and self.num_subset != -1:
            return self.h5_file_traj_idx[self.num_subset]
        return min(self.n_rows - self.start_index, self.max_length)

    def process_index(self, index):
        index = (index + self.random_start_offset) % len(self)
        return index + self.start_index

    # -- data_procgen.py:132-174 ---------------------------------------------------------------------------------------------------
    def _find_reward_key(self, reward_key):
        if reward_key is not None:
            if reward_key not in self.store:
                raise KeyError(f"reward dataset {reward_key!r} is not in the store")
            return reward_key
        # the writer here emits "{key}_{vl_type}_reward" (arp_amd/label_reward.py); the reference READER asks for "..._pos_reward"
        for name in (f"{self.image_key}_{self.vl_type}_reward", f"{self.image_key}_{self.vl_type}_pos_reward"):
            if name in self.store:
                return name
        raise KeyError(f"no reward dataset: neither {self.image_key}_{self.vl_type}_reward nor {self.image_key}_{self.vl_type}_pos_reward")

    def preprocess_rtgs(self):
        """Per-row return-to-go R[j] (f32, NOT yet divided by the scale); sets reward_min / reward_max / return_to_go / scale."""
        reward = np.asarray(self.store[self.reward_key][:, -1]).astype(np.float32)
        self.reward_min, self.reward_max = np.min(reward), np.max(reward)
        modified = reward - self.reward_min if self.use_normalize else reward
        R = np.zeros(self.n_rows, np.float32)
        b = self.h5_file_traj_idx
        spans = list(zip(b[:-1], b[1:]))
        for lo, hi in spans:
            R[lo:hi] = _discount_cumsum(modified[lo:hi], 1.0)
        # the reference takes the statistic over the STACKED array [n, num_frames] (:156-171): the maximum is the per-row one, the quantile is not
        # (a row's stack repeats the trajectory's first value while it is being filled), so the stack is rebuilt for it
        n_done = b[-1]
        if n_done == 0:
            raise ValueError("no finished trajectory (no done flag): the reference has no return-to-go to take a statistic of")
        if "coinrun" in self.env_name:
            self.return_to_go = np.max(R[:n_done]) // 100 * 100
        else:
            rows = np.arange(n_done)
            src = np.maximum(rows[:, None] - np.arange(self.num_frames - 1, -1, -1)[None, :], self.traj_start[:n_done, None])
            self.return_to_go = np.quantile(R[src][None], 0.9) // 100 * 100
        self.scale = compute_scale(self.return_to_go)
        if n_done < self.n_rows:  # an unfinished trajectory at the end: the reference raises IndexError on these rows; here they carry their own partial sums
            R[n_done:] = _discount_cumsum(modified[n_done:], 1.0)
        return R

    # -- data_procgen.py:180-213 ---------------------------------------------------------------------------------------------------
    def window_rows(self, i):
        """Source rows j(t) of the window of (processed) row i."""
        T = self.window_size
        return np.maximum(i - (T - 1 - np.arange(T)), int(self.traj_start[i]))

    def last_frames(self, rows):
        """``ob[rows, -1]`` for sorted-or-not row numbers (one chunk read per row on an H5 store)."""
        ob = self.store[self.image_key]
        rows = np.asarray(rows, np.int64)
        if hasattr(ob, "read_last_frames_spans"):
            out = np.empty((len(rows),) + self.frame_shape, np.uint8)
            for k, j in enumerate(rows):
                out[k] = ob[int(j), -1] if not ob.fast_path_ok() else ob.read_last_frames_spans([(int(j), int(j) + 1)], stacked=False)[0]
            return out
        return np.stack([np.asarray(ob[int(j)][-1]) for j in rows])

    # -- data_procgen.py:186-189 ---------------------------------------------------------------------------------------------------
    def goal_row(self, i, rng=None):
        """The hindsight goal of (processed) row i: one draw of ``goal_rng.choice`` over the rows from i to the end of i's trajectory -- the reference's own
        call, so a RandomState seeded like its global generator gives its sequence -- clamped to the last row.  The goal frames are that row's window.
        ``rng``: draw from this generator instead of the dataset's own (``DeviceDataset.index_batches(goal_rng=...)``)."""
        rng = self.goal_rng if rng is None else rng
        if rng is None:
            raise ValueError("no goal_rng: construct the dataset with goal_rng=numpy.random.RandomState(seed)")
        b = self.h5_file_traj_idx
        t = int(self.idx_to_traj[i])
        end = b[t + 1] if t + 1 < len(b) and b[t] <= i < b[t + 1] else self.n_rows  # (rows behind the last done flag: their unfinished trajectory)
        return min(rng.choice(list(range(i, end)), 1).item(), self.n_rows - 1)

    def _labels(self, index, j):
        res = {"image": {}, "rtg": {}}
        if self.use_vl:
            res["rtg"][self.image_key] = (self.rtg[j][..., None] / self.scale).astype(np.float32)
        res["action"] = self.action[j]
        return res

    def __getitem__(self, index):
        i = self.process_index(int(index))
        j = self.window_rows(i)
        res = self._labels(i, j)
        res["image"][self.image_key] = self.last_frames(j)
        if self.goal_rng is not None:
            res["goal"] = {self.image_key: self.last_frames(self.window_rows(self.goal_row(i)))}
        return res

    def literal_item(self, index):
        """The reference's literal reads: ``ob[i][-T:]``, ``act[i][-T:]`` of the stacked rows themselves (the return-to-go is not stored stacked:
        it is the same per-row array through the window rule, as the reference's own stack of it is)."""
        i = self.process_index(int(index))
        T = self.window_size
        res = self._labels(i, self.window_rows(i))
        res["image"][self.image_key] = np.asarray(self.store[self.image_key][i])[-T:]
        res["action"] = np.asarray(self.store["act"][i])[-T:].astype(np.int32)
        return res

    def verify(self, k=8, seed=0):
        """Compare ``k`` sampled rows (plus the first and the last) read literally against the window rule; True when every one agrees bitwise."""
        n = len(self)
        if n <= 0:
            return True
        pick = np.random.default_rng(seed).choice(n, size=min(int(k), n), replace=False)
        for i in sorted(set(int(v) for v in pick) | {0, n - 1}):
            a, b = self[i], self.literal_item(i)
            if not (np.array_equal(a["image"][self.image_key], b["image"][self.image_key]) and np.array_equal(a["action"], b["action"])):
                return False
        return True

    def close(self):
        if self._own:
            self.store.close()
            self._own = False


class DeviceDataset:
    """The demonstration set resident in HBM (``arp_ds`` of libarp_hip.so): one uint8 frame, action, return-to-go and trajectory start per row,
    optionally one encoding per row.  Rows are FILE rows: an index batch holds processed indices (``ProcgenDataset.process_index``)."""

    def __init__(self, n_rows, res, device=0):
        _ffi.require_gpu()
        h = C.c_void_p()
        check(lib.arp_ds_create(int(n_rows), int(res), int(device), C.byref(h)))
        self._h = h
        self.n_rows, self.res, self.device = int(n_rows), int(res), int(device)
        self.dataset = None
        self.window_size = None
        self.encoder_mode = None
        self._trainers = weakref.WeakSet()

    @classmethod
    def load(cls, dataset, device=0, lut=None, chunk_rows=1024, verify_rows=8):
        """Read every row's last frame (``read_last_frames_spans``: one inflate per ``num_frames`` rows), upload chunk by chunk -- the next chunk is
        read while the copy of this one runs --, set the labels.  Refuses a file whose stacked rows do not follow the window rule."""
        from .finetune_data import ProcgenActionDataset
        action_set = isinstance(dataset, ProcgenActionDataset)  # the fine-tune step's set: frames and actions only, and it reads `[-1]` of a row, never a window
        if action_set and len(dataset.image_keys) != 1:
            raise ArpError("the device-resident set holds one image_key (several work on the host side only)")
        if not action_set and not dataset.verify(verify_rows, seed=0):
            raise ArpError("this file's rows are not recorder-stacked (ob[i][-T:] differs from the frames of rows max(i - k, trajectory start)): "
                           "a device-resident dataset would train on other windows than the reference reads")
        H, W, ch = dataset.frame_shape
        if H != W or ch != 3:
            raise ArpError(f"frames must be square RGB, not {dataset.frame_shape}")
        self = cls(dataset.n_rows, H, device)
        try:
            self.dataset, self.window_size = dataset, dataset.window_size
            self.set_lut(default_lut() if lut is None else lut)
            from concurrent.futures import ThreadPoolExecutor
            ob = dataset.store[dataset.image_keys[0] if action_set else dataset.image_key]
            bounds = list(dataset.h5_file_traj_idx)
            if bounds[-1] < dataset.n_rows:
                bounds.append(dataset.n_rows)

            def read(r0):
                r1 = min(r0 + int(chunk_rows), dataset.n_rows)
                if hasattr(ob, "read_last_frames_spans"):  # spans of ONE trajectory each
                    cuts = [r0] + [b for b in bounds if r0 < b < r1] + [r1]
                    return r0, ob.read_last_frames_spans(list(zip(cuts[:-1], cuts[1:])))
                return r0, np.ascontiguousarray(np.asarray(ob[r0:r1])[:, -1])

            with ThreadPoolExecutor(1) as pool:
                nxt = pool.submit(read, 0)
                while nxt is not None:
                    r0, fr = nxt.result()
                    nxt = pool.submit(read, r0 + len(fr)) if r0 + len(fr) < dataset.n_rows else None
                    self.upload_frames(r0, fr)
            # the scale is divided in here, as __getitem__ does; the fine-tune step's set carries no return-to-go
            rtg = (dataset.rtg / np.float32(dataset.scale)).astype(np.float32) if not action_set and dataset.use_vl else None
            self.set_labels(dataset.action, rtg, dataset.traj_start, int(dataset.action.max()) + 1 if len(dataset.action) else 1)
        except BaseException:
            self.close()
            raise
        return self

    # -- contents ---------------------------------------------------------------------------------------------------------------------
    def upload_frames(self, row0, frames_u8):
        f = np.require(np.asarray(frames_u8), dtype=np.uint8, requirements="C")
        if f.ndim != 4 or f.shape[1:] != (self.res, self.res, 3):
            raise ValueError(f"frames must be uint8 [n, {self.res}, {self.res}, 3], not {f.shape}")
        check(lib.arp_ds_upload_frames(self._h, int(row0), f.shape[0], _ffi.as_ptr(f, C.c_uint8)))

    def set_labels(self, action, rtg, traj_start, n_actions):
        a = np.require(np.asarray(action, dtype=np.int32), requirements="C")
        s = np.require(np.asarray(traj_start, dtype=np.int32), requirements="C")
        r = None if rtg is None else np.require(np.asarray(rtg, dtype=np.float32), requirements="C")
        if a.shape != (self.n_rows,) or s.shape != (self.n_rows,) or (r is not None and r.shape != (self.n_rows,)):
            raise ValueError(f"labels must have one value per row ({self.n_rows})")
        check(lib.arp_ds_set_labels(self._h, _ffi.as_ptr(a, C.c_int32), None if r is None else _ffi.as_ptr(r, C.c_float), _ffi.as_ptr(s, C.c_int32),
                                    int(n_actions)))

    def set_quad_bounds(self, first, last):
        """The per-row trajectory interval the fine-tune step's four frames are taken from (``ProcgenActionDataset.bounds()``)."""
        f = np.require(np.asarray(first, dtype=np.int32), requirements="C")
        l = np.require(np.asarray(last, dtype=np.int32), requirements="C")
        if f.shape != (self.n_rows,) or l.shape != (self.n_rows,):
            raise ValueError(f"quad bounds must have one value per row ({self.n_rows})")
        check(lib.arp_ds_set_quad_bounds(self._h, _ffi.as_ptr(f, C.c_int32), _ffi.as_ptr(l, C.c_int32)))

    def quads(self, idx, groups=4):
        """Debug read-back of the quad kernel: ``(rows int32 [groups, B] group-major, r f32 [B], action int32 [B])`` of the processed indices ``idx``."""
        idx = np.require(np.asarray(idx, dtype=np.int64).reshape(-1), requirements="C")
        B, G = len(idx), int(groups)
        rows, r, act = np.empty((max(G, 0), B), np.int32), np.empty(B, np.float32), np.empty(B, np.int32)
        check(lib.arp_ds_quads_debug(self._h, _ffi.as_ptr(idx, C.c_int64), B, G, _ffi.as_ptr(rows, C.c_int32), _ffi.as_ptr(r, C.c_float),
                                     _ffi.as_ptr(act, C.c_int32)))
        return rows, r, act

    def set_lut(self, lut):
        t = np.require(np.asarray(lut, dtype=np.float32), requirements="C")
        if t.shape != (3, 256):
            raise ValueError("lut must be f32 [3, 256]")
        check(lib.arp_ds_set_lut(self._h, _ffi.as_ptr(t, C.c_float)))
        self.lut = t.copy()

    def _refuse_beside_prefetch(self, what):
        for tr in list(self._trainers):
            if getattr(tr, "_prefetch_owner", None) is not None:
                raise ArpError(f"{what} while a prefetcher of an attached trainer is live: the encoder's workspace (and the slots' encodings) are in use; "
                               "finish or drop the prefetcher first")

    def cache_encodings(self, encoder, chunk=128):
        """Encode every frame once with the frozen encoder (``arp_ds_encode``); index batches with ``use_encodings=True`` then gather encodings and the step
        is the encodings-in step.  Sound because the encoder's output for a frame does not depend on the batch it is encoded in (DESIGN, "device-resident
        dataset": shown bitwise by tests/test_dataset_gpu.py)."""
        self._refuse_beside_prefetch("cache_encodings")
        check(lib.arp_ds_encode(self._h, encoder._h, int(min(chunk, getattr(encoder, "max_frames", chunk)))))
        self.encoder_mode = getattr(encoder, "mode", None)

    def set_encodings(self, encodings):
        """Encodings the user supplies: one array ``[n_rows, tokens, dim]`` or an iterable of consecutive chunks ``[n, tokens, dim]``."""
        self._refuse_beside_prefetch("set_encodings")
        chunks = [encodings] if isinstance(encodings, np.ndarray) else encodings
        row0 = 0
        for ch in chunks:
            e = np.require(np.asarray(ch, dtype=np.float32), requirements="C")
            if e.ndim != 3:
                raise ValueError("encodings must be [n, tokens, dim]")
            if row0 == 0:
                check(lib.arp_ds_alloc_encodings(self._h, e.shape[1], e.shape[2]))
                shape = e.shape[1:]
            if e.shape[1:] != shape:
                raise ValueError(f"encoding chunks must all be [n, {shape[0]}, {shape[1]}]")
            check(lib.arp_ds_upload_encodings(self._h, row0, e.shape[0], _ffi.as_ptr(e, C.c_float)))
            row0 += e.shape[0]
        if row0 != self.n_rows:
            raise ArpError(f"set_encodings: {row0} rows given, the dataset has {self.n_rows}")

    def gather(self, idx, window=None, frames=True, goal_index=None):
        """Debug read-back: ``{"image": f32 [B, T, res, res, 3], "action": int32 [B, T], "rtg": f32 [B, T, 1] (if the set holds one)}`` of the batch
        the row indices name.  ``goal_index`` (model GCBC's pair batch): ``"goal"`` beside ``"image"`` -- the windows of the goal rows, through the pair
        gather -- and no ``"rtg"`` (GCBC reads none)."""
        idx = np.require(np.asarray(idx, dtype=np.int64).reshape(-1), requirements="C")
        T = int(self.window_size if window is None else window)
        B = len(idx)
        if T <= 0 or B == 0:
            raise ArpError("gather: window must be positive and idx non-empty")
        img = np.empty((B, T, self.res, self.res, 3), np.float32) if frames else None
        act = np.empty((B, T), np.int32)
        if goal_index is not None:
            gidx = np.require(np.asarray(goal_index, dtype=np.int64).reshape(-1), requirements="C")
            if len(gidx) != B:
                raise ArpError(f"gather: {B} indices, {len(gidx)} goal indices")
            goal = np.empty((B, T, self.res, self.res, 3), np.float32) if frames else None
            check(lib.arp_ds_gather_pairs_debug(self._h, _ffi.as_ptr(idx, C.c_int64), _ffi.as_ptr(gidx, C.c_int64), B, T,
                                                None if img is None else _ffi.as_ptr(img, C.c_float), None if goal is None else _ffi.as_ptr(goal, C.c_float),
                                                _ffi.as_ptr(act, C.c_int32)))
            return {"action": act, "image": img, "goal": goal} if frames else {"action": act}
        has_rtg = self.dataset is None or self.dataset.use_vl
        rtg = np.empty((B, T, 1), np.float32) if has_rtg else None
        check(lib.arp_ds_gather_debug(self._h, _ffi.as_ptr(idx, C.c_int64), B, T, None if img is None else _ffi.as_ptr(img, C.c_float),
                                      _ffi.as_ptr(act, C.c_int32), None if rtg is None else _ffi.as_ptr(rtg, C.c_float)))
        out = {"action": act}
        if img is not None:
            out["image"] = img
        if rtg is not None:
            out["rtg"] = rtg
        return out

    @property
    def nbytes(self):
        return int(lib.arp_ds_nbytes(self._h)) if self._h else 0

    def index_batches(self, batch_size, seed, epochs=None, drop_last=True, rank=0, world=1, goal_rng=None):
        """Yields ``{"index": int64[B_global]}``: per epoch one fresh ``numpy.random.default_rng`` permutation of ``range(len(dataset))``, mapped through
        ``process_index``, cut into global batches.  NOT torch's ``DataLoader`` stream: same distribution (a uniform shuffle without replacement per
        epoch), other numbers.  ``rank`` / ``world`` only check divisibility: every rank draws the same global batch and ``shard_batch`` (what the step
        functions and ``prefetch_to_device`` apply) cuts this rank's contiguous part, exactly as for a host batch.

        ``goal_rng`` (a ``numpy.random.RandomState``; model GCBC): yields ``{"index": int64[B], "goal_index": int64[B]}`` -- one ``dataset.goal_row`` draw
        per batch position, in batch order, which is the order in which a sequential ``[dataset[i] for i in index]`` consumes the same generator: the same
        seed names the same goals on both feeds.  The index stream itself is the one without ``goal_rng``."""
        goal_row = None
        if goal_rng is not None:
            if self.dataset is None:
                raise ArpError("index_batches(goal_rng=...): the hindsight draw needs the trajectory bounds of a loaded ProcgenDataset (DeviceDataset.load)")
            goal_row = lambda i: self.dataset.goal_row(i, goal_rng)  # noqa: E731
        return index_batches(len(self.dataset) if self.dataset is not None else self.n_rows, batch_size, seed, epochs=epochs, drop_last=drop_last,
                             rank=rank, world=world, process_index=self.dataset.process_index if self.dataset is not None else None, goal_row=goal_row)

    def close(self):
        if getattr(self, "_h", None):
            lib.arp_ds_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def index_batches(n, batch_size, seed, epochs=None, drop_last=True, rank=0, world=1, process_index=None, goal_row=None):
    """The index stream of :meth:`DeviceDataset.index_batches` (needs no GPU).  ``goal_row``: a callable (processed row -> goal row), called once per batch
    position in batch order as each batch is drawn; its rows go out under ``"goal_index"``."""
    B = int(batch_size)
    if B <= 0 or B % int(world) or not (0 <= int(rank) < int(world)):
        raise ValueError(f"global batch of {B} does not divide over {world} ranks (rank {rank})")
    if n < B and drop_last:
        raise ValueError(f"{n} rows give no full batch of {B}")
    rng = np.random.default_rng(seed)
    epoch = 0
    while epochs is None or epoch < epochs:
        perm = rng.permutation(n).astype(np.int64)
        if process_index is not None:
            perm = np.asarray([process_index(int(i)) for i in perm], np.int64)
        stop = n - n % B if drop_last else n
        for lo in range(0, stop, B):
            if goal_row is None:
                yield {"index": perm[lo : lo + B]}
            else:
                yield {"index": perm[lo : lo + B], "goal_index": np.asarray([goal_row(int(i)) for i in perm[lo : lo + B]], np.int64)}
        epoch += 1
