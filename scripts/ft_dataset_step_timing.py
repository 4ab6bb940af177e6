"""Step time of the CLIP-adapter fine-tune step fed from the device-resident demonstration set beside the host-built batches, at the real geometry:
ViT-B/16 towers, the 476 M-parameter head, B = 64 samples x 3 frames of 256 x 256, a seeded synthetic set of `--rows` rows in trajectories of 64, one GPU,
one process, one head.

Three arms, each `--steps` steps with the losses read back every step, behind `--lead` untimed ones, every step timed on the wall clock:
  a_host_built  towers.encode_multiscale_to(3B host frames, B prompts) + set_batch_device + train_step: the feed before this one (README's frames-in row).  The
                two 3B-frame batches it alternates are assembled BEFORE the clock starts: the arm pays the upload, the B-prompt text pass and the three host
                synchronisations, not the host's gather of 192 frames
  b_feed_sync   FinetuneFeed.train_step: indices in; quad kernel, transform from the resident rows, vision tower, head -- two streams, ordered by events
  c_feed_run    FinetuneFeed.run: the same with batch k + 1 staged before step k's losses are waited for

The arms are warmed up, then timed in alternation over `--rounds` rounds.  Per arm: the median over the rounds of each round's median step, and the spread
(max - min) of the round medians.  The one decision the figures carry: `run` keeps its stage-ahead only if c is below b by more than the larger of their two
spreads.  Beside them the transform-from-rows launch on its own (device events of the towers' profiler around preprocess_bilinear_rows).  Its 192 source
frames (37.7 MB) and its output sit in the 256 MiB Infinity Cache across such a loop: the figure is a launch time, NOT an HBM rate.

Writes profiles/ft_dataset_step_timing.txt and prints it.

    python scripts/ft_dataset_step_timing.py [--steps 200] [--lead 8] [--rounds 5] [--rows 2048] [--mode f16]
"""
import argparse
import datetime
import json
import os
import socket
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--lead", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--mode", default="f16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ft_dataset_step_timing.txt"))
    a = ap.parse_args()
    import torch  # noqa: F401  -- before arp_amd: one HIP runtime per process (arp_amd/_ffi.py)
    import numpy as np

    from arp_amd import _ffi, clip, dataset, synth
    from arp_amd import finetune as FT
    from arp_amd.finetune_data import ProcgenActionDataset
    _ffi.require_gpu()
    B, lr, L = a.batch, 1e-4, 64
    ccfg = clip.MODELS["ViT-B/16"]
    towers = clip.ClipLabeller(ccfg, synth.clip_weights(ccfg, seed=0), mode=a.mode, max_batch=3 * B)
    hcfg = FT.FinetuneConfig()
    tr = FT.FinetuneTrainer(hcfg, mode=a.mode)
    tr.set_params(FT.synth_params(hcfg, seed=0))

    rng = np.random.default_rng(1)
    frames = synth.procgen_like_frames(a.rows, seed=1)
    act = rng.integers(0, 15, a.rows).astype(np.int32)
    done = np.zeros(a.rows, np.uint8)
    done[L - 1::L] = 1
    # a one-frame "stack": the set reads ob[row][-1] only
    ads = ProcgenActionDataset({"ob": frames[:, None], "act": act[:, None], "done": done[:, None]}, env_name="coinrun")
    ds = dataset.DeviceDataset.load(ads)
    tokens = synth.prompt_tokens(1, 8, seed=203)
    feed = FT.FinetuneFeed(tr, towers, ds, ads, tokens=tokens)

    def index_stream(n, seed):
        it = dataset.index_batches(len(ads), B, seed, process_index=ads.process_index)
        return [next(it)["index"] for _ in range(n)]

    host = []
    for idx in index_stream(2, 5):
        q, r, arow = ads.quads_of_rows(idx)
        host.append((np.ascontiguousarray(frames[q[:, :3].T.reshape(-1)]), r.astype(np.float32), act[arow]))
    tokens_b = np.tile(tokens, (B, 1))
    fbufs = tr.feature_buffers(B)

    def run(arm, steps, lead):
        """the wall-clock ms of each of `steps` steps of one arm behind `lead` untimed ones"""
        n, ms = steps + lead, []
        if arm == "a_host_built":
            for k in range(n):
                t0 = time.perf_counter()
                fr, r, action = host[k & 1]
                towers.encode_multiscale_to(fr, tokens_b, fbufs)
                tr.set_batch_device(fbufs, r, action)
                tr.train_step(lr)
                ms.append((time.perf_counter() - t0) * 1e3)
        elif arm == "b_feed_sync":
            for idx in index_stream(n, 7):
                t0 = time.perf_counter()
                feed.train_step(idx, lr)
                ms.append((time.perf_counter() - t0) * 1e3)
        else:
            t0 = time.perf_counter()
            for _ in feed.run(index_stream(n, 7), lr):
                t1 = time.perf_counter()
                ms.append((t1 - t0) * 1e3)
                t0 = t1
        return ms[lead:]

    arms = ("a_host_built", "b_feed_sync", "c_feed_run")
    for arm in arms:  # warm-up: allocations, the first launches
        run(arm, 4, a.lead)
    med = {n: [] for n in arms}
    for _ in range(a.rounds):
        for arm in arms:
            med[arm].append(float(np.median(run(arm, a.steps, a.lead))))

    # the transform-from-rows launch on its own: the towers' profiler brackets it with device events
    towers.profile(True)
    towers.profile_reset()
    for idx in index_stream(20, 9):
        feed.train_step(idx, lr)
    site = towers.profile_read()["preprocess_bilinear_rows"]
    towers.profile(False)
    rows_us = site["ms"] / site["calls"] * 1e3
    esz = 4 if a.mode == "f32" else 2
    mb_in, mb_out = 3 * B * 256 * 256 * 3 / 1e6, 3 * B * 3 * 224 * 224 * esz / 1e6
    feed.close()
    for b in fbufs:
        b.free()
    tr.close()
    ds.close()
    towers.close()

    out = {"metric": f"ms per fine-tune step (losses read back), ViT-B/16 towers + {tr.n_params / 1e6:.0f} M-parameter head, {a.mode}", "batch": B, "rows": a.rows,
           "steps": a.steps, "lead": a.lead, "rounds": a.rounds}
    for n, v in med.items():
        out[n] = {"median_ms": round(float(np.median(v)), 4), "spread_ms": round(max(v) - min(v), 4), "round_medians_ms": [round(x, 4) for x in v]}
    base = out["a_host_built"]["median_ms"]
    for n in arms[1:]:
        out[n]["minus_a_ms"] = round(out[n]["median_ms"] - base, 4)
    gain = out["b_feed_sync"]["median_ms"] - out["c_feed_run"]["median_ms"]
    bar = max(out["b_feed_sync"]["spread_ms"], out["c_feed_run"]["spread_ms"])
    out["stage_ahead_gain_ms"] = round(gain, 4)
    out["stage_ahead_gain_exceeds_larger_spread"] = bool(gain > bar)
    out["transform_rows_us"] = round(rows_us, 1)
    out["transform_rows_mb_read"] = round(mb_in, 1)
    out["transform_rows_mb_written"] = round(mb_out, 1)

    lines = [f"box {socket.gethostname()}  date {datetime.datetime.now().isoformat(timespec='seconds')}",
             f"fine-tune step, ViT-B/16 towers + {tr.n_params / 1e6:.0f} M-parameter head, {a.mode}, B = {B} x 3 frames of 256 x 256, {a.rows}-row synthetic set; "
             f"{a.rounds} alternating rounds of {a.steps} steps behind {a.lead} untimed; per arm: median of the round medians, spread (max - min) of the round medians"]
    for n in arms:
        r = out[n]
        lines.append(f"{n:13s} {r['median_ms']:.3f} ms (spread {r['spread_ms']:.3f})" + (f"  {r['minus_a_ms']:+.3f} ms against a_host_built" if "minus_a_ms" in r else ""))
    lines.append(f"stage-ahead: c is {gain:.3f} ms below b, the larger spread is {bar:.3f} ms -> " +
                 ("run() keeps staging batch k + 1 before it waits for step k" if gain > bar else "NOT beyond the spread: run() should stage synchronously"))
    lines.append(f"transform from rows alone (device events, 20 launches): {rows_us:.1f} us for {mb_in:.1f} MB read + {mb_out:.1f} MB written -- a loop whose "
                 "buffers sit in the 256 MiB Infinity Cache: a launch time, not an HBM rate")
    text = "\n".join(lines) + "\n" + json.dumps(out) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
