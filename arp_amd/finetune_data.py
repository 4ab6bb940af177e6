"""The demonstration set of the CLIP-adapter fine-tune step: the reference's ``ProcgenActionDataset`` on the host.

Mirrors finetune_module/action_finetune_data_procgen.py:47-169 (the deterministic parts): ``__len__`` (:87-91), ``get_traj_idx`` (:93-96),
``get_idx_to_traj`` (:98-105), ``process_index`` (:107-109), ``__getitem__`` (:134-165), ``num_actions`` (:167-169).

The four rows.  A sample is four frames of one trajectory -- its first row, row ``i``, row ``i + 1`` clamped to the last row, the last row --
SORTED (:144), ``r = int(rows[2] == rows[3])`` (:162) and the action at the smallest row (:164).  Every frame is ``h5_file[key][row][-1]``: the one
frame row ``row`` adds to the recorder's stack (arp_amd/dataset.py, "the window rule"), which is what :class:`arp_amd.dataset.DeviceDataset` keeps in
HBM -- :meth:`ProcgenActionDataset.quads` names the rows, :meth:`bounds` is the table the device side computes them from.

The quirk, kept.  ``idx_to_traj`` starts as 0 everywhere and is filled for the rows in front of the last ``done`` flag only, so every row behind it
belongs to trajectory 0.  Such a row ``i`` gets ``[first_0, i, min(i + 1, last_0), last_0]`` with ``i > last_0``: the sort moves ``i`` to the end, the
third and fourth rows differ (``r = 0``), and the action is trajectory 0's first.  A file without a single ``done`` flag has no trajectory 0 to point
at: the reference raises IndexError there, and so does this class.

Not here: ``random_start`` draws its offset with an unseeded generator as the reference does (pass ``start_offset_ratio`` for a reproducible one),
kornia's ColorJitter (the augmentation sits in the model, not in the dataset), the gcsfs path.  ``instruct`` needs ``tokens=`` or ``tokenizer=``: no
BPE vocabulary ships with this package (as in arp_amd.label_reward).
"""
import os

import numpy as np

from .data import get_clip_instruct


class ProcgenActionDataset:
    """The reference class's deterministic core over an :class:`arp_amd.h5store.H5Store`, a path to one, or a plain mapping of arrays."""

    def __init__(self, store_or_path, image_key="ob", start_index=0, max_length=int(1e9), random_start=False, start_offset_ratio=None, env_name=None,
                 env_type="none", *, action_dim=15, tokens=None, tokenizer=None):
        self._own = False
        path = ""
        if isinstance(store_or_path, (str, os.PathLike)):
            from . import h5store
            path = os.fspath(store_or_path)
            store_or_path = h5store.H5Store(path, "r")
            self._own = True
        self.store = store_or_path
        self.image_key = image_key
        self.image_keys = image_key.split(", ")  # (:156)
        self.start_index, self.max_length = int(start_index), int(max_length)
        self.action_dim = int(action_dim)
        ob = self.store["ob"]  # (__len__ reads "ob" whatever the image key is, :89)
        self.n_rows = int(ob.shape[0])
        first = self.store[self.image_keys[0]]
        self.frame_shape = tuple(int(v) for v in first.shape[2:])
        self.window_size = 1  # a row is read for its last frame only
        if env_name is None:
            attrs = getattr(self.store, "attrs", None)
            env_name = attrs.get("env_name", "") if attrs is not None else ""
            env_name = env_name.decode() if isinstance(env_name, bytes) else str(env_name)
        if env_type != "none":  # (:64-67)
            env_name = f"{env_name}_{env_type}"
        if "mugen" in path:
            env_name += "_mugen"
        self.env_name = env_name
        self.instruct = get_clip_instruct(env_name)
        self._tokens = None if tokens is None else np.asarray(tokens)
        self._tokenizer = tokenizer
        if random_start:  # (:69-74)
            self.random_start_offset = int(np.random.default_rng().choice(len(self)))
        elif start_offset_ratio is not None:
            self.random_start_offset = int(len(self) * start_offset_ratio) % len(self)
        else:
            self.random_start_offset = 0
        done_last = np.asarray(self.store["done"][:, -1])
        self.h5_file_traj_idx = self.get_traj_idx(done_last)
        self.idx_to_traj = self.get_idx_to_traj(done_last)
        self.action = np.ascontiguousarray(np.asarray(self.store["act"][:, -1]))
        # what DeviceDataset.set_labels wants beside the actions: the start of each row's trajectory by the RECORDER's rule (rows behind the last done
        # flag form a trajectory of their own) -- the window rule's table, not the quirked one the quads come from
        b = np.asarray(self.h5_file_traj_idx, np.int64)
        self.traj_start = b[np.searchsorted(b, np.arange(self.n_rows), side="right") - 1].astype(np.int32)

    # -- :87-109 ---------------------------------------------------------------------------------------------------------------------
    def __len__(self):
        return min(self.n_rows - self.start_index, self.max_length)

    def get_traj_idx(self, done_last=None):
        done_last = np.asarray(self.store["done"][:, -1]) if done_last is None else done_last
        return [0] + [int(v) for v in np.nonzero(done_last)[0] + 1]

    def get_idx_to_traj(self, done_last=None):
        """int32 [n_done_rows]: the trajectory of every row in front of the last ``done`` flag, 0 for every row behind it (the reference's initial value)."""
        done_last = np.asarray(self.store["done"][:, -1]) if done_last is None else done_last
        b = np.asarray(self.get_traj_idx(done_last), np.int64)
        rows = np.arange(done_last.shape[0])
        t = np.searchsorted(b, rows, side="right") - 1
        return np.where(rows < b[-1], t, 0).astype(np.int32)

    def process_index(self, index):
        index = (index + self.random_start_offset) % len(self)
        return index + self.start_index

    @property
    def num_actions(self):
        return self.action_dim

    # -- the four rows (:136-144, 162, 164) -----------------------------------------------------------------------------------------------
    def bounds(self):
        """``(first int32 [n_rows], last int32 [n_rows])``: the interval of the trajectory ``idx_to_traj`` gives each row, quirk rows included (theirs
        is trajectory 0's, which does not contain them).  What ``DeviceDataset.set_quad_bounds`` takes."""
        b = np.asarray(self.h5_file_traj_idx, np.int64)
        if len(b) < 2:
            raise IndexError("list index out of range: no done flag in the file, so no trajectory has an end (the reference fails the same way)")
        t = self.idx_to_traj.astype(np.int64)
        return b[t].astype(np.int32), (b[t + 1] - 1).astype(np.int32)

    def quads_of_rows(self, rows):
        """:meth:`quads` for rows that are already processed (file rows: what an index batch of ``arp_amd.dataset.index_batches`` holds)."""
        first, last = self.bounds()
        i = np.asarray(rows, np.int64).reshape(-1)
        f, l = first[i].astype(np.int64), last[i].astype(np.int64)
        q = np.sort(np.stack([f, i, np.minimum(i + 1, l), l], axis=1), axis=1).astype(np.int32)
        return q, (q[:, 2] == q[:, 3]).astype(np.int32), np.ascontiguousarray(q[:, 0])

    def quads(self, indices):
        """``(rows int32 [B, 4] sorted, r int32 [B], action_row int32 [B])`` of dataset indices (``process_index`` is applied, as ``__getitem__`` does)."""
        idx = np.asarray(indices, np.int64).reshape(-1)
        return self.quads_of_rows((idx + self.random_start_offset) % len(self) + self.start_index)

    def quad(self, index):
        i = self.process_index(int(index))
        t = int(self.idx_to_traj[i])
        first, last = self.h5_file_traj_idx[t], self.h5_file_traj_idx[t + 1] - 1  # (IndexError without a done flag, as the reference)
        return sorted([first, i, min(i + 1, last), last])

    def last_frames(self, key, rows):
        """``store[key][rows, -1]`` (one chunk read per row on an H5 store)."""
        ob = self.store[key]
        out = []
        for j in rows:
            if hasattr(ob, "read_last_frames_spans") and ob.fast_path_ok():
                out.append(ob.read_last_frames_spans([(int(j), int(j) + 1)], stacked=False)[0])
            else:
                out.append(np.asarray(ob[int(j)][-1]))
        return out

    def __getitem__(self, index):
        q = self.quad(index)
        res = {f"image{g}": {} for g in range(4)}
        for key in self.image_keys:
            for g, fr in enumerate(self.last_frames(key, q)):
                res[f"image{g}"][key] = fr
        res["r"] = np.array([int(q[-2] == q[-1])])
        if self._tokens is not None:
            res["instruct"] = self._tokens
        elif self._tokenizer is not None:
            res["instruct"] = self._tokenizer(self.instruct)
        res["action"] = self.action[q[0]]
        return res

    def close(self):
        if self._own:
            self.store.close()
            self._own = False
