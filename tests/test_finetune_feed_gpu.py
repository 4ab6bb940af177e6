"""The fine-tune step fed from the device-resident demonstration set (arp_ft_feed_*, arp_amd.finetune.FinetuneFeed).

Every comparison here is EXACT: both sides run the same kernels on the same bytes -- the quad kernel against numpy integers, the transform from rows against the
transform of the gathered frames (one pinned arithmetic, arp_amd/csrc/preprocess.h), the feed against a batch the host builds from the same rows and hands
to the same towers and the same head.  No tolerance anywhere."""
import ctypes as C
import gc
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "finetune_dataset.npz")
TOWER = dict(patch=32, width=64, layers=2, heads=2, embed=64, img_res=224, txt_width=64, txt_layers=2, txt_heads=2, ctx=77, vocab=512)
HEAD = dict(layers=2, width_v=64, width_t=64, embed=64, hidden=64)
F32, BF16, F16 = 0, 1, 2
FILL = 0xA5


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _live(lib):
    out = (C.c_int64 * 5)()
    lib.check(lib.lib.arp_debug_live(out))
    return list(out)


# ---- the 13-row set: trajectory lengths [1, 2, 5, 3] and two rows behind the last done flag -------------------------------------------------------------------
_SET = {}


def _action_dataset(res=256):
    """(ProcgenActionDataset over an in-memory recorder-stacked store, its frames uint8 [13, res, res, 3]); built once."""
    if res in _SET:
        return _SET[res]
    from arp_amd import synth
    from arp_amd.finetune_data import ProcgenActionDataset
    g = np.load(GOLD)
    done, act = g["tail/done"], g["tail/act"]
    n = done.shape[0]
    frames = synth.procgen_like_frames(n, res, res, seed=700)
    b = np.concatenate([[0], np.nonzero(done[:, -1])[0] + 1])
    start = b[np.searchsorted(b, np.arange(n), side="right") - 1]
    src = np.maximum(np.arange(n)[:, None] - np.arange(done.shape[1] - 1, -1, -1)[None, :], start[:, None])
    ds = ProcgenActionDataset({"ob": frames[src], "act": act, "done": done}, env_name="coinrun")
    frames.setflags(write=False)
    _SET[res] = (ds, frames)
    return _SET[res]


def _device_dataset(ads):
    from arp_amd.dataset import DeviceDataset
    return DeviceDataset.load(ads)


# ---- 1. the quad kernel -------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G", [3, 4])
def test_quad_kernel_equals_the_host_rule(gpu_lib, G):
    ads, _ = _action_dataset(16)
    dds = _device_dataset(ads)
    dds.set_quad_bounds(*ads.bounds())
    idx = np.random.default_rng(5).permutation(13).astype(np.int64)  # every row once, shuffled
    q, r, arow = ads.quads_of_rows(idx)
    B = len(idx)
    # read-back buffers one element longer, sentinel-filled: the call copies back exactly its outputs (and checks a guard word behind each on the device)
    rows = np.full(G * B + 1, -77, np.int32)
    rr = np.full(B + 1, -77.0, np.float32)
    act = np.full(B + 1, -77, np.int32)
    gpu_lib.check(gpu_lib.lib.arp_ds_quads_debug(dds._h, _p(idx, C.c_int64), B, G, _p(rows, C.c_int32), _p(rr, C.c_float), _p(act, C.c_int32)))
    assert np.array_equal(rows[:-1].reshape(G, B), q[:, :G].T)          # group-major
    assert np.array_equal(rr[:-1], r.astype(np.float32))                # r from all four rows, whatever G is
    assert np.array_equal(act[:-1], ads.action[arow].astype(np.int32))  # the action at the smallest row
    assert rows[-1] == -77 and rr[-1] == -77.0 and act[-1] == -77
    # the wrapper, and one row fewer
    rows2, r2, act2 = dds.quads(idx[:-1], groups=G)
    assert np.array_equal(rows2, q[:-1, :G].T) and np.array_equal(r2, r[:-1].astype(np.float32)) and np.array_equal(act2, ads.action[arow[:-1]].astype(np.int32))
    # the quirk rows went through the sort
    k = int(np.nonzero(idx == 11)[0][0])
    assert q[k].tolist() == [0, 0, 0, 11] and rr[k] == 0.0
    # refused on the host
    bad = np.array([0, 13], np.int64)
    assert gpu_lib.lib.arp_ds_quads_debug(dds._h, _p(bad, C.c_int64), 2, G, _p(rows, C.c_int32), _p(rr, C.c_float), _p(act, C.c_int32)) != 0
    assert "outside [0, 13)" in gpu_lib.last_error()
    assert gpu_lib.lib.arp_ds_quads_debug(dds._h, _p(idx, C.c_int64), B, 5, _p(rows, C.c_int32), _p(rr, C.c_float), _p(act, C.c_int32)) != 0
    f, l = ads.bounds()
    l2 = l.copy(); l2[3] = 13
    assert gpu_lib.lib.arp_ds_set_quad_bounds(dds._h, _p(f, C.c_int32), _p(l2, C.c_int32)) != 0 and "row 3" in gpu_lib.last_error()
    dds.close()


# ---- 2. the transform from rows -------------------------------------------------------------------------------------------------------------------------------

GEOMETRIES = [(256, 256, 0), (256, 256, 1), (72, 100, 0), (72, 100, 1), (224, 224, 0)]
ROWS = np.array([2, 0, 2, 3, 1], np.int32)  # a repeat, out of order


@pytest.mark.parametrize("H,W,crop", GEOMETRIES, ids=[f"{h}x{w}{'-crop' if c else ''}" for h, w, c in GEOMETRIES])
def test_transform_from_rows_equals_transform_of_gathered_frames(gpu_lib, H, W, crop):
    lib = gpu_lib.lib
    R = 224
    st = np.random.default_rng(H * 1000 + W).integers(0, 256, (4, H, W, 3), dtype=np.uint8)
    picked = st[ROWS]
    if crop:  # the centre crop of side W // 2 (label_reward.py:15-36), in numpy
        cs = W // 2
        y0, x0 = int((H - cs) / 2), int((W - cs) / 2)
        picked = picked[:, y0:y0 + cs, x0:x0 + cs]
    picked = np.ascontiguousarray(picked)
    n = len(ROWS)
    for patch in (16, 32):
        for mode in (F32, BF16, F16):
            nbytes = n * 3 * R * R * (4 if mode == F32 else 2)
            want = np.full(nbytes, FILL, np.uint8)
            got = np.full(nbytes, FILL, np.uint8)
            gpu_lib.check(lib.arp_op_preprocess_bilinear(_p(picked, C.c_uint8), n, picked.shape[1], picked.shape[2], R, patch, mode, _p(want, C.c_void_p)))
            gpu_lib.check(lib.arp_op_preprocess_bilinear_rows(_p(st, C.c_uint8), 4, _p(ROWS, C.c_int32), n, H, W, crop, R, patch, mode, _p(got, C.c_void_p)))
            diff = np.nonzero(want != got)[0]
            assert diff.size == 0, f"{H}x{W} crop {crop} patch {patch} mode {mode}: {diff.size} bytes differ, first at {diff[0]}"


def test_transform_from_rows_refusals(gpu_lib):
    lib = gpu_lib.lib
    st = np.zeros((4, 64, 64, 3), np.uint8)
    out = np.full(2 * 3 * 224 * 224 * 4, FILL, np.uint8)
    for bad in ([0, 4], [-1, 0]):
        rows = np.array(bad, np.int32)
        assert lib.arp_op_preprocess_bilinear_rows(_p(st, C.c_uint8), 4, _p(rows, C.c_int32), 2, 64, 64, 0, 224, 16, F32, _p(out, C.c_void_p)) != 0
        assert "outside the set" in gpu_lib.last_error() and (out == FILL).all()
    rows = np.array([0, 1], np.int32)
    for H, W in ((224, 100), (100, 224)):
        fr = np.zeros((4, H, W, 3), np.uint8)
        assert lib.arp_op_preprocess_bilinear_rows(_p(fr, C.c_uint8), 4, _p(rows, C.c_int32), 2, H, W, 0, 224, 16, F32, _p(out, C.c_void_p)) != 0
        assert "exactly one side at 224" in gpu_lib.last_error() and (out == FILL).all()


# ---- 3 .. 6: the feed -------------------------------------------------------------------------------------------------------------------------------------------

def _towers(mode, max_batch=1024):
    from arp_amd import clip, synth
    from oracle import clip_np
    return clip.ClipLabeller(clip.ClipConfig(**TOWER), synth.clip_weights(clip_np.ClipConfig(**TOWER), seed=81), mode=mode, max_batch=max_batch)


def _head(mode, goal=False, seed=91):
    from arp_amd import finetune as FT
    cfg = FT.FinetuneConfig(goal_conditioned=goal, **HEAD)
    tr = FT.FinetuneTrainer(cfg, mode=mode)
    tr.set_params(FT.synth_params(cfg, seed=seed))
    return tr


def _tokens():
    from arp_amd import synth
    return synth.prompt_tokens(1, 6, ctx=TOWER["ctx"], vocab=TOWER["vocab"], seed=90)


class HostFeed:
    """The host-built feed the issue defines: frames gathered in numpy by `quads`, group-major; ONE arp_clip_encode_image_multiscale_dev pass of the G B
    frames; the single prompt's encode_text_multiscale rows tiled B times; set_batch_device."""

    def __init__(self, lib, tr, towers, ads, frames, tokens):
        self.lib, self.tr, self.towers, self.ads, self.frames = lib, tr, towers, ads, frames
        self.G = 4 if tr.cfg.goal_conditioned else 3
        self.text = None if tokens is None else towers.encode_text_multiscale(tokens)

    def stage(self, idx):
        from arp_amd.clip import DeviceBuffer
        q, r, arow = self.ads.quads_of_rows(idx)
        B = len(idx)
        fr = np.ascontiguousarray(self.frames[q[:, :self.G].T.reshape(-1)])
        bufs = list(self.tr.feature_buffers(B))
        self.lib.check(self.lib.lib.arp_clip_encode_image_multiscale_dev(self.towers._h, _p(fr, C.c_uint8), len(fr), fr.shape[1], fr.shape[2], bufs[0].ptr, bufs[1].ptr))
        if self.text is not None:
            bufs[2].upload(np.tile(self.text[0], (B, 1)))
            bufs[3].upload(np.tile(self.text[1], (B, 1)))
        self.tr.set_batch_device(bufs, r.astype(np.float32), self.ads.action[arow].astype(np.int32))
        for b in bufs:
            b.free()

    def train_step(self, idx, lr):
        self.stage(idx)
        return self.tr.train_step(lr)

    def forward(self, idx):
        self.stage(idx)
        return self.tr.forward()


BATCHES = {3: [[11, 4, 0], [2, 12, 7], [9, 1, 5]],                                        # quirk rows, a length-1 trajectory, trajectory ends
           8: [[11, 4, 0, 2, 12, 7, 9, 1], [3, 5, 6, 8, 10, 0, 11, 2], [12, 1, 7, 4, 3, 9, 10, 6]]}


@pytest.mark.parametrize("B", [3, 8], ids=["B3-latency-rows", "B8-throughput-rows"])
@pytest.mark.parametrize("goal", [False, True], ids=["plain", "goal"])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_feed_equals_host_built_feed(gpu_lib, mode, goal, B):
    """Two AdamW steps and a forward: every aux value, every parameter tensor, scores and logits, bit for bit."""
    from arp_amd import finetune as FT
    ads, frames = _action_dataset()
    towers = _towers(mode)
    dds = _device_dataset(ads)
    tok = None if goal else _tokens()
    a, b = _head(mode, goal), _head(mode, goal)
    host = HostFeed(gpu_lib, a, towers, ads, frames, tok)
    feed = FT.FinetuneFeed(b, towers, dds, ads, tokens=tok)
    idx = [np.asarray(v, np.int64) for v in BATCHES[B]]
    for k in range(2):
        want, got = host.train_step(idx[k], 1e-3), feed.train_step(idx[k], 1e-3)
        assert want == got, f"step {k}: {want} != {got}"
    Pa, Pb = a.get_params(), b.get_params()
    for name in Pa:
        assert np.array_equal(Pa[name], Pb[name]), name
    fa, fb = host.forward(idx[2]), feed.eval_step(idx[2])
    assert np.array_equal(fa["scores"], fb["scores"]) and np.array_equal(fa["logits"], fb["logits"])
    assert all(fa[k] == fb[k] for k in FT.AUX_KEYS)
    feed.close(); a.close(); b.close(); dds.close(); towers.close()


def test_stage_ahead_equals_synchronous(gpu_lib):
    """Six steps through run() -- each slot reused three times -- against six train_step calls on the same index stream."""
    from arp_amd import finetune as FT
    from arp_amd.dataset import index_batches
    ads, _ = _action_dataset()
    towers = _towers("f32")
    dds = _device_dataset(ads)
    tok = _tokens()
    a, b = _head("f32"), _head("f32")
    fa, fb = FT.FinetuneFeed(a, towers, dds, ads, tokens=tok), FT.FinetuneFeed(b, towers, dds, ads, tokens=tok)
    stream = index_batches(len(ads), 3, seed=4, process_index=ads.process_index)
    batches = [next(stream)["index"] for _ in range(6)]
    sync = [fa.train_step(i, 1e-3) for i in batches]
    ahead = list(fb.run(iter({"index": i} for i in batches), 1e-3))
    assert len(ahead) == 6 and sync == ahead
    Pa, Pb = a.get_params(), b.get_params()
    assert all(np.array_equal(Pa[k], Pb[k]) for k in Pa)
    fa.close(); fb.close(); a.close(); b.close(); dds.close(); towers.close()


def test_eval_step_is_the_forward_and_moves_no_parameter(gpu_lib):
    from arp_amd import finetune as FT
    ads, frames = _action_dataset()
    towers = _towers("f32")
    dds = _device_dataset(ads)
    tok = _tokens()
    a, b = _head("f32"), _head("f32")
    host, feed = HostFeed(gpu_lib, a, towers, ads, frames, tok), FT.FinetuneFeed(b, towers, dds, ads, tokens=tok)
    idx = np.asarray(BATCHES[3][1], np.int64)
    before = b.get_params()
    want, got = host.forward(idx), feed.eval_step(idx)
    assert np.array_equal(want["scores"], got["scores"]) and np.array_equal(want["logits"], got["logits"]) and all(want[k] == got[k] for k in FT.AUX_KEYS)
    after = b.get_params()
    assert all(np.array_equal(before[k], after[k]) for k in before) and b.step == 0
    feed.close(); a.close(); b.close(); dds.close(); towers.close()


def test_refusals_and_ownership(gpu_lib):
    from arp_amd import finetune as FT
    from arp_amd._ffi import ArpError
    from arp_amd.dataset import DeviceDataset
    lib = gpu_lib.lib
    ads, frames = _action_dataset()
    tok = _tokens()
    gc.collect()
    live0 = _live(gpu_lib)
    towers, small = _towers("f32"), _towers("f32", max_batch=8)
    dds = _device_dataset(ads)
    dds.set_quad_bounds(*ads.bounds())  # (the set's own two tables: FinetuneFeed(...) sets them again in place)
    plain, goal, ref = _head("f32"), _head("f32", goal=True), _head("f32")
    live1 = _live(gpu_lib)

    with pytest.raises(ArpError, match="goal_conditioned head reads no prompt"):
        FT.FinetuneFeed(goal, towers, dds, ads, tokens=tok)
    with pytest.raises(ArpError, match="pass its tokens"):
        FT.FinetuneFeed(plain, towers, dds, ads, tokens=None)
    assert _live(gpu_lib) == live1  # a refused attach keeps nothing

    feed = FT.FinetuneFeed(plain, towers, dds, ads, tokens=tok)
    good = np.asarray(BATCHES[3][0], np.int64)
    with pytest.raises(ArpError, match=r"index 13 \(batch position 1\) is outside \[0, 13\)"):
        feed.stage(0, [0, 13, 2])
    with pytest.raises(ArpError, match="outside"):
        feed.stage(0, [0, -1, 2])
    with pytest.raises(ArpError, match="holds no staged batch"):
        feed.step_async(1, 1e-3)                 # stepped before it is staged (the refused stagings above left nothing behind either)
    with pytest.raises(ArpError, match="holds no staged batch"):
        feed.step_async(0, 1e-3)
    with pytest.raises(ArpError, match="slots 0 and 1"):
        feed.stage(2, good)

    # G B > max_batch: 3 x 3 frames into towers created with max_batch = 8
    tight = FT.FinetuneFeed(goal, small, dds, ads)
    with pytest.raises(ArpError, match="max_batch 8"):
        tight.stage(0, good)                     # 4 x 3 = 12 frames
    tight.stage(0, good[:2])                     # 8 frames fit
    tight.step_async(0, 1e-3)
    assert np.isfinite(tight.collect()["loss"])
    tight.close()

    # sets that lack something: no labels / no quad bounds / a row not uploaded.  (Attached through the C ABI: FinetuneFeed sets the bounds itself.)
    first, last = ads.bounds()
    idx = np.ascontiguousarray(good)

    def staged_error(ds):
        gpu_lib.check(lib.arp_ft_feed_detach(goal._h))
        gpu_lib.check(lib.arp_ft_feed_attach(goal._h, towers._h, ds._h, None))
        rc = lib.arp_ft_feed_stage_async(goal._h, 0, _p(idx, C.c_int64), len(idx))
        err = gpu_lib.last_error()
        gpu_lib.check(lib.arp_ft_feed_detach(goal._h))
        assert rc != 0
        return err

    nolab = DeviceDataset(13, 256); nolab.upload_frames(0, frames); nolab.set_quad_bounds(first, last)
    assert "labels are not set" in staged_error(nolab)
    noquad = DeviceDataset(13, 256); noquad.upload_frames(0, frames); noquad.set_labels(ads.action, None, ads.traj_start, 15)
    assert "quad bounds are not set" in staged_error(noquad)
    short = DeviceDataset(13, 256); short.upload_frames(0, frames[:12]); short.set_labels(ads.action, None, ads.traj_start, 15); short.set_quad_bounds(first, last)
    assert "only 12 of 13 frame rows" in staged_error(short)
    for d in (nolab, noquad, short):
        d.close()

    # a staged slot is taken by ONE step
    feed.stage(0, good)
    feed.step_async(0, 1e-3)
    with pytest.raises(ArpError, match="holds no staged batch"):
        feed.step_async(0, 1e-3)
    got = feed.collect()
    # ... and the feed still works, and computed what a feed that met no refusal computes
    clean = FT.FinetuneFeed(ref, towers, dds, ads, tokens=tok)
    assert clean.train_step(good, 1e-3) == got
    nxt = np.asarray(BATCHES[3][1], np.int64)
    assert feed.train_step(nxt, 1e-3) == clean.train_step(nxt, 1e-3)

    feed.close(); clean.close()
    live2 = _live(gpu_lib)
    # close() gives back everything FinetuneFeed(...) took: on handles whose own workspaces are warm (the steps above grew the head's and the towers'),
    # a feed that is attached, steps and closes leaves every counter where it was before FinetuneFeed(...)
    again = FT.FinetuneFeed(plain, towers, dds, ads, tokens=tok)
    again.train_step(good, 1e-3)
    again.close()
    assert _live(gpu_lib) == live2
    plain.close(); goal.close(); ref.close(); dds.close(); towers.close(); small.close()
    gc.collect()
    assert _live(gpu_lib) == live0
