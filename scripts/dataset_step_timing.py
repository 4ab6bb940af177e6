"""Step time of the policy trainer fed from a device-resident demonstration set (arp_amd.dataset.DeviceDataset) beside today's feeds, at the real
geometry: B = 32, window 4, 256 x 256 frames, policy mode f16 with the f16c encoder, synthetic frames, one GPU, one trainer.

Four arms, each `--steps` synchronous train steps (train_step_fn incl. the aux read-back) behind `--lead` untimed ones, wall clock per step:
  a_host_frames     host float frames [B, T, 256, 256, 3] through prefetch_to_device (101 MB over PCIe per step): today's path, the comparison for b
  b_index_frames    index batches through prefetch_to_device, frames gathered on the GPU, the encoder inside the step
  c_index_cached    index batches through prefetch_to_device on cached encodings: the encodings-in step plus one gather
  d_resident        encodings resident in the synchronous slot (bench.py --path policy's figure): the floor for c

The arms are warmed up, then timed in alternation over `--rounds` rounds; medians and ranges go into one JSON line.  Beside them: the gather launches on
their own (device events around the synchronous slot's gathers, arp_dt_profile), the frame gather against its traffic bound, whether the cached-encodings
trajectory equals the encoder-inside one bitwise in this encoder mode, and -- with `--load-rows N` -- the load time of an N-row recorder-style file split
into file read, upload and cache_encodings.

    python scripts/dataset_step_timing.py [--steps 20] [--lead 8] [--rounds 5] [--rows 1024] [--load-rows 8192] [--hbm-gbs 4000]
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

F = 8  # the recorder's num_frames


def synthetic_set(rows, traj_len, seed):
    """Per-row frames / actions / returns / trajectory starts of `rows` rows in trajectories of `traj_len`."""
    import numpy as np

    from arp_amd import synth
    rng = np.random.default_rng(seed)
    frames = synth.procgen_like_frames(rows, seed=seed)
    start = (np.arange(rows) // traj_len * traj_len).astype(np.int32)
    return frames, rng.integers(0, 15, rows).astype(np.int32), rng.random(rows).astype(np.float32), start


def write_recorder_file(path, frames, action, start, reward):
    """The set as the recorder + the labelling pass write it: rows stacked F deep, gzip chunks of one row (level 1: the file is scaffolding here)."""
    import numpy as np

    from arp_amd import h5store
    n = len(frames)
    src = np.maximum(np.arange(n)[:, None] - np.arange(F - 1, -1, -1)[None, :], start[:, None])
    done = np.zeros(n, np.float32)
    done[np.r_[start[1:] != start[:-1], True]] = 1
    with h5store.H5Store(path, "w") as f:
        f.attrs["env_name"] = "coinrun"
        ob = f.create_dataset("ob", shape=(n, F) + frames.shape[1:], dtype=np.uint8, compression="gzip", compression_opts=1, chunks=(1, F) + frames.shape[1:])
        for r0 in range(0, n, 64):
            ob[r0 : r0 + 64] = frames[src[r0 : r0 + 64]]
        for k, v in (("act", action.astype(np.int64)), ("done", done), ("ob_clip_reward", reward)):
            f.create_dataset(k, data=v[src], compression="gzip", chunks=(1, F))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--lead", type=int, default=8, help="untimed steps in front of every timed block (a chain captured for frames is captured again for encodings)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rows", type=int, default=1024, help="rows of the synthetic set the steps draw from")
    ap.add_argument("--load-rows", type=int, default=0, help="also time the load of a recorder-style file of this many rows (0: skip)")
    ap.add_argument("--hbm-gbs", type=float, default=4000.0, help="the HBM rate the traffic bounds are taken at, GB/s")
    ap.add_argument("--encoder-mode", default="f16c")
    a = ap.parse_args()
    import torch  # noqa: F401  -- before arp_amd: one HIP runtime per process (arp_amd/_ffi.py)
    import numpy as np

    from arp_amd import _ffi, dataset, m3ae, synth_policy as S
    from arp_amd.train import PolicyConfig, TrainState, create_train_step, prefetch_to_device
    _ffi.require_gpu()
    cfg, ecfg = PolicyConfig(lambda_ret=0.01), m3ae.EncoderConfig()
    B, T, lr = a.batch, cfg.window, 5e-4
    enc = m3ae.M3AEEncoder(ecfg, S.m3ae_params(ecfg, seed=0), mode=a.encoder_mode, max_frames=B * T)
    state = TrainState.create(cfg, S.policy_params(cfg, seed=0), mode="f16")
    tr = state.trainer
    tr.attach_encoder(enc)
    fn = create_train_step(cfg, lambda step: lr, cfg.weight_decay)

    frames, action, rtg, start = synthetic_set(a.rows, 64, seed=1)
    ds = dataset.DeviceDataset(a.rows, ecfg.img_res)
    ds.window_size = T
    ds.set_lut(dataset.default_lut())
    t0 = time.perf_counter()
    ds.upload_frames(0, frames)
    upload_s = time.perf_counter() - t0
    ds.set_labels(action, rtg, start, 15)
    t0 = time.perf_counter()
    ds.cache_encodings(enc)
    cache_s = time.perf_counter() - t0
    rng = np.random.default_rng(2)
    index = [rng.integers(0, a.rows, B).astype(np.int64) for _ in range(4)]

    def host_batch(idx):
        j = np.maximum(idx[:, None] - (T - 1 - np.arange(T))[None, :], start[idx][:, None])
        return {"image": {"ob": dataset.bytes_to_float(frames[j])}, "action": action[j], "rtg": {"ob": rtg[j][..., None]}}

    host = [host_batch(i) for i in index[:2]]

    def run(arm, steps, lead, collect=None):
        """ms per step of one arm; collect: a list that receives the losses of the timed steps"""
        nonlocal state
        n = steps + lead
        if arm == "d_resident":
            tr.attach_dataset(ds, use_encodings=True)
            tr.set_batch_indices(index[0])
            t_s = None
            for k in range(n):
                if k == lead:
                    t_s = time.perf_counter()
                aux = tr.train_step(lr)
                if collect is not None and k >= lead:
                    collect.append(aux["loss"])
            return (time.perf_counter() - t_s) / steps * 1e3
        if arm == "a_host_frames":
            src = (host[k & 1] for k in range(n))
        else:
            tr.attach_dataset(ds, use_encodings=arm == "c_index_cached")
            src = ({"index": index[k & 1]} for k in range(n))
        t_s = None
        for k, b in enumerate(prefetch_to_device(src, 2, tr)):
            if k == lead:
                t_s = time.perf_counter()
            state, aux, _ = fn(state, b, None)
            if collect is not None and k >= lead:
                collect.append(aux["loss"])
        return (time.perf_counter() - t_s) / steps * 1e3

    arms = ("a_host_frames", "b_index_frames", "c_index_cached", "d_resident")
    # does this encoder mode give a frame the same encoding in every batch?  the same steps from the same state, frames in against cached encodings
    P0, same = tr.get_params(), {}
    for arm in ("a_host_frames", "b_index_frames", "c_index_cached"):
        tr.set_params(P0)
        for which in (2, 3):
            tr.set_tensors({k: np.zeros_like(v) for k, v in P0.items()}, which)
        tr.step = 0
        same[arm] = []
        run(arm, 4, 0, same[arm])
    for arm in arms:  # warm-up
        run(arm, 4, a.lead)
    times = {n: [] for n in arms}
    for _ in range(a.rounds):
        for arm in arms:
            times[arm].append(run(arm, a.steps, a.lead))

    # the gather launches on their own: device events around the synchronous slot's gathers
    gathers = {}
    for use_enc, site in ((False, "ds.gather_frames"), (True, "ds.gather_encodings")):
        tr.attach_dataset(ds, use_encodings=use_enc)
        for k in range(3):
            tr.set_batch_indices(index[k & 1])
        tr.profile(True)
        tr.profile_reset()
        for k in range(20):
            tr.set_batch_indices(index[k & 3])
        p = tr.profile_read()[site]
        tr.profile(False)
        gathers[site] = p["ms"] / p["calls"] * 1e3
    fb = ecfg.img_res * ecfg.img_res * 3
    frame_bytes, enc_bytes = B * T * fb * 5, 2 * B * T * ecfg.tokens * ecfg.width * 4

    out = {"metric": "ms per policy train step (train_step_fn incl. aux read-back), f16 policy", "encoder_mode": a.encoder_mode, "batch": B, "window": T,
           "rows": a.rows, "steps": a.steps, "lead": a.lead, "rounds": a.rounds}
    for n, v in times.items():
        out[n] = {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    spread = max(times["a_host_frames"]) - min(times["a_host_frames"])
    out["b_minus_a_ms"] = round(out["b_index_frames"]["median_ms"] - out["a_host_frames"]["median_ms"], 4)
    out["a_spread_ms"] = round(spread, 4)
    out["c_minus_d_us"] = round((out["c_index_cached"]["median_ms"] - out["d_resident"]["median_ms"]) * 1e3, 1)
    out["gather_frames_us"] = round(gathers["ds.gather_frames"], 1)
    out["gather_encodings_us"] = round(gathers["ds.gather_encodings"], 1)
    out["hbm_gbs_assumed"] = a.hbm_gbs
    out["gather_frames_bound_us"] = round(frame_bytes / a.hbm_gbs / 1e3, 1)
    out["gather_frames_over_bound"] = round(gathers["ds.gather_frames"] / (frame_bytes / a.hbm_gbs / 1e3), 2)
    out["gather_encodings_bound_us"] = round(enc_bytes / a.hbm_gbs / 1e3, 1)
    out["gather_encodings_over_bound"] = round(gathers["ds.gather_encodings"] / (enc_bytes / a.hbm_gbs / 1e3), 2)
    out["index_frames_equal_host_frames_bitwise"] = same["a_host_frames"] == same["b_index_frames"]
    out["cached_equal_encoder_inside_bitwise"] = same["b_index_frames"] == same["c_index_cached"]
    out["set"] = {"rows": a.rows, "upload_s": round(upload_s, 3), "cache_encodings_s": round(cache_s, 3), "hbm_mb": round(ds.nbytes / 1e6, 1)}
    tr.close()
    ds.close()

    if a.load_rows > 0:  # the load of a file, split: file read (the last frame of every row), upload, cache_encodings
        fr, act, r, st = synthetic_set(a.load_rows, 64, seed=3)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "data_train.hdf5")
            write_recorder_file(path, fr, act, st, r)
            del fr
            t0 = time.perf_counter()
            pd = dataset.ProcgenDataset(path, T)
            ob = pd.store["ob"]
            b = list(pd.h5_file_traj_idx)
            host_frames = ob.read_last_frames_spans(list(zip(b[:-1], b[1:])))
            read_s = time.perf_counter() - t0
            del host_frames
            t0 = time.perf_counter()
            big = dataset.DeviceDataset.load(pd)
            load_s = time.perf_counter() - t0  # (read and upload overlapped, chunk by chunk, + verify + labels)
            t0 = time.perf_counter()
            big.cache_encodings(enc)
            big_cache_s = time.perf_counter() - t0
            out["load"] = {"rows": a.load_rows, "file_mb": round(os.path.getsize(path) / 1e6, 1), "file_read_s": round(read_s, 3),
                           "load_read_overlapped_with_upload_s": round(load_s, 3), "cache_encodings_s": round(big_cache_s, 3),
                           "hbm_mb": round(big.nbytes / 1e6, 1)}
            big.close()
            pd.close()
    enc.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
