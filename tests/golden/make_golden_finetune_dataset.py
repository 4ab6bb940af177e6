"""Generates tests/golden/finetune_dataset.npz (run in the build container; never on the GPU box).

    python tests/golden/make_golden_finetune_dataset.py [reference checkout]

What pins what: which four rows a sample reads, its ``r`` and its ``action`` come from the REFERENCE CLASS ITSELF --
finetune_module/action_finetune_data_procgen.py::ProcgenActionDataset -- executed here with its missing imports replaced by stand-ins:
  * `h5py`           -> `File(path)` returns an in-memory mapping of numpy arrays with `.attrs` (the sets below, registered by path);
  * `clip`           -> `tokenize` records the prompt it was given and returns a marker array;
  * `gcsfs`          -> an empty module (only a gs:// path touches it);
  * `ml_collections` -> `ConfigDict` is an attribute bag with `update` / `copy_and_resolve_references`;
  * `arp_dt.data_procgen` -> `get_clip_instruct` is arp_amd.data's table (the prompt is recorded, not judged on).
None of the stand-ins decides anything the class under test is judged on: trajectory bounds, the index mapping, the four rows, their sort, `r` and the
action row are the reference's own code.  Frames are 2 x 2 x 3 bytes that all hold their row's number, so the frames an item returns name the rows read.

Only what the class read and returned goes into the fixture, beside the `done` / `act` arrays it was given.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"

STACK = 2
FILES = {}
PROMPTS = []


class _Mem(dict):
    def __init__(self, arrays, attrs):
        super().__init__(arrays)
        self.attrs = attrs


class _Bag:
    def __init__(self, d=None):
        for k, v in (d.__dict__ if isinstance(d, _Bag) else dict(d or {})).items():
            setattr(self, k, v)

    def update(self, other):
        self.__dict__.update(other.__dict__)

    def copy_and_resolve_references(self):
        return _Bag(self)


def _install_stand_ins():
    sys.path.insert(0, ROOT)
    from arp_amd.data import get_clip_instruct

    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    def tokenize(text):
        PROMPTS.append(text)
        return np.full((1, 77), 7, np.int32)

    mod("h5py", File=lambda path, mode="r": FILES[path])
    mod("clip", tokenize=tokenize)
    mod("gcsfs")
    mod("ml_collections", ConfigDict=_Bag)
    pkg = mod("arp_dt")
    pkg.__path__ = []
    pkg.data_procgen = mod("arp_dt.data_procgen", get_clip_instruct=get_clip_instruct)
    sys.path.insert(0, REF)


def make_set(lengths, tail, seed, done_flags=True):
    """Recorder-stacked rows: ob [n, STACK, 2, 2, 3] (row i's last frame holds i in every byte), act [n, STACK], done [n, STACK]."""
    n = sum(lengths) + tail
    start = np.zeros(n, np.int64)
    done_last = np.zeros(n, np.uint8)
    lo = 0
    for ln in list(lengths) + ([tail] if tail else []):
        start[lo: lo + ln] = lo
        lo += ln
    if done_flags:
        done_last[np.cumsum(lengths) - 1] = 1
    rng = np.random.default_rng(seed)
    act_last = rng.integers(0, 15, n).astype(np.int64)
    src = np.maximum(np.arange(n)[:, None] - np.arange(STACK - 1, -1, -1)[None, :], start[:, None])  # the window rule
    ob = np.broadcast_to(src[:, :, None, None, None].astype(np.uint8), (n, STACK, 2, 2, 3)).copy()
    done = np.zeros((n, STACK), np.uint8)
    done[:, -1] = done_last
    return {"ob": ob, "act": act_last[src], "done": done}


def record(name, arrays, out, **kw):
    from finetune_module.action_finetune_data_procgen import ProcgenActionDataset
    path = f"mem/{name}/data_train.hdf5"
    FILES[path] = _Mem(arrays, {"env_name": "coinrun"})
    update = {"path": "mem", "start_index": kw.get("start_index", 0), "max_length": kw.get("max_length", int(1e9))}
    ds = ProcgenActionDataset(update, dataset_name=name, start_offset_ratio=kw.get("start_offset_ratio"))
    n = len(ds)
    rows = np.zeros((n, 4), np.int32)
    r = np.zeros(n, np.int32)
    action = np.zeros(n, np.int32)
    pidx = np.zeros(n, np.int32)
    for i in range(n):
        item = ds[i]
        for g in range(4):
            fr = item[f"image{g}"]["ob"]
            assert fr.shape == (2, 2, 3) and (fr == fr.flat[0]).all()
            rows[i, g] = int(fr.flat[0])
        assert item["r"].shape == (1,)
        r[i] = int(item["r"][0])
        action[i] = int(item["action"])
        pidx[i] = ds.process_index(i)
    out[f"{name}/done"] = arrays["done"]
    out[f"{name}/act"] = arrays["act"]
    out[f"{name}/start_index"] = np.int64(kw.get("start_index", 0))
    out[f"{name}/max_length"] = np.int64(kw.get("max_length", int(1e9)))
    out[f"{name}/start_offset_ratio"] = np.float64(kw.get("start_offset_ratio", np.nan) if kw.get("start_offset_ratio") is not None else np.nan)
    out[f"{name}/len"] = np.int64(n)
    out[f"{name}/traj_idx"] = np.asarray(ds.get_traj_idx(), np.int64)
    out[f"{name}/process_index"] = pidx
    out[f"{name}/rows"] = rows
    out[f"{name}/r"] = r
    out[f"{name}/action"] = action
    out[f"{name}/num_actions"] = np.int64(ds.num_actions)
    out[f"{name}/env_name"] = np.asarray(ds.env_name)


def main():
    _install_stand_ins()
    from finetune_module.action_finetune_data_procgen import ProcgenActionDataset
    out = {}
    tail = make_set([1, 2, 5, 3], 2, seed=0)
    record("tail", tail, out)
    record("tail_start3", tail, out, start_index=3)
    record("tail_ratio", tail, out, start_offset_ratio=0.4)
    record("tail_max7", tail, out, max_length=7)
    record("closed", make_set([3, 1, 4], 0, seed=1), out)
    out["names"] = np.asarray(["tail", "tail_start3", "tail_ratio", "tail_max7", "closed"])
    out["prompt"] = np.asarray(PROMPTS[0])
    assert all(p == PROMPTS[0] for p in PROMPTS)
    # a file without a single done flag: which exception the class raises, and where
    FILES["mem/nodone/data_train.hdf5"] = _Mem(make_set([4], 0, seed=2, done_flags=False), {"env_name": "coinrun"})
    ds = ProcgenActionDataset({"path": "mem"}, dataset_name="nodone")
    try:
        ds[0]
        raised = ""
    except Exception as e:  # noqa: BLE001
        raised = type(e).__name__
    out["nodone/raises"] = np.asarray(raised)
    np.savez_compressed(os.path.join(HERE, "finetune_dataset.npz"), **out)
    print("wrote finetune_dataset.npz:", {k: out[k + "/rows"].tolist() for k in ("tail",)}, "no done ->", raised)


if __name__ == "__main__":
    main()
