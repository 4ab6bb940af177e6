"""Step time of a GCBC trainer fed from the device-resident demonstration set beside the host-built goal batches, at the real geometry: ViT-B/16 at
256 x 256 (513 tokens per (frame, goal) pair), the 26.9 M-parameter policy, f16 policy + f16 encoder, B = 32, window 4, a seeded synthetic set of
`--rows` rows in trajectories of 64, one GPU, one trainer.

Four arms, each `--steps` synchronous train steps (the aux read-back included) behind `--lead` untimed ones, every step timed on the wall clock:
  a_host_goals      set_batch_images(frames, action, goals=) on the synchronous slot, 2 x 100.7 MB of f32 over PCIe per step: the only GCBC feed before the
                    pair gather, and the baseline.  The two host batches it alternates are built BEFORE the clock starts: the arm pays the upload, not the
                    host's assembly of 256 windows (which a data loader would overlap, or not)
  b_sync_pairs      set_batch_index_pairs: (row, goal row) pairs gathered on the GPU into the synchronous slot, the step encodes at its head
  c_prefetch        pair batches through prefetch_to_device, ARP_DT_ENCODE_AHEAD=0: the gather of batch i + 1 runs beside step i
  d_prefetch_ahead  the same with encode-ahead: the goal-conditioned encoder pass of batch i + 1 runs beside step i's policy part

The arms are warmed up, then timed in alternation over `--rounds` rounds.  Per arm: the median over the rounds of each round's median step, and the spread
(max - min) of the round medians.  Beside them the pair gather on its own (device events around the synchronous slot's gather, arp_dt_profile) against
its traffic (2 x B x T frames: 1 byte read, 4 written per value).  The one decision the figures carry: encode-ahead stays prefetch_to_device's default
for pair batches only if d is lower than c by more than the larger of their two spreads.

Writes profiles/gcbc_dataset_step_timing.txt and prints it.

    python scripts/gcbc_dataset_step_timing.py [--steps 200] [--lead 8] [--rounds 5] [--rows 2048]
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
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gcbc_dataset_step_timing.txt"))
    a = ap.parse_args()
    import torch  # noqa: F401  -- before arp_amd: one HIP runtime per process (arp_amd/_ffi.py)
    import numpy as np

    from arp_amd import _ffi, dataset, m3ae, synth, synth_policy as S
    from arp_amd.train import PolicyConfig, TrainState, create_train_step, prefetch_to_device
    from oracle import m3ae_np as M
    _ffi.require_gpu()
    ecfg = m3ae.EncoderConfig()
    cfg = PolicyConfig(model="GCBC", enc_tokens=ecfg.gc_tokens)
    B, T, lr, L = a.batch, cfg.window, 5e-4, 64
    enc = m3ae.M3AEEncoder(ecfg, S.m3ae_params(M.EncConfig(), seed=0), mode="f16", max_frames=B * T)
    state = TrainState.create(cfg, S.policy_params(cfg, seed=0), mode="f16")
    tr = state.trainer
    tr.attach_encoder(enc)
    fn = create_train_step(cfg, lambda step: lr, cfg.weight_decay)

    rng = np.random.default_rng(1)
    frames = synth.procgen_like_frames(a.rows, seed=1)
    action = rng.integers(0, 15, a.rows).astype(np.int32)
    start = (np.arange(a.rows) // L * L).astype(np.int32)
    ds = dataset.DeviceDataset(a.rows, ecfg.img_res)
    ds.window_size = T
    ds.set_lut(dataset.default_lut())
    ds.upload_frames(0, frames)
    ds.set_labels(action, None, start, 15)
    tr.attach_dataset(ds)

    def pair_stream(n, seed):
        """n pair batches: the index stream of DeviceDataset.index_batches, the hindsight draw over [i, end of i's trajectory)"""
        g = np.random.RandomState(seed)
        it = dataset.index_batches(a.rows, B, seed, goal_row=lambda i: int(g.randint(i, min(int(start[i]) + L, a.rows))))
        return (next(it) for _ in range(n))

    def windows(rows):
        return np.maximum(rows[:, None] - (T - 1 - np.arange(T))[None, :], start[rows][:, None])

    host = []
    for p in pair_stream(2, 5):
        host.append((dataset.bytes_to_float(frames[windows(p["index"])]), action[windows(p["index"])], dataset.bytes_to_float(frames[windows(p["goal_index"])])))

    def run(arm, steps, lead):
        """the wall-clock ms of each of `steps` steps of one arm behind `lead` untimed ones"""
        nonlocal state
        n, ms = steps + lead, []
        os.environ["ARP_DT_ENCODE_AHEAD"] = "1" if arm == "d_prefetch_ahead" else "0"
        if arm == "a_host_goals":
            for k in range(n):
                t0 = time.perf_counter()
                fr, act, go = host[k & 1]
                tr.set_batch_images(fr, act, goals=go)
                tr.train_step(lr)
                ms.append((time.perf_counter() - t0) * 1e3)
            return ms[lead:]
        src = pair_stream(n, 7)
        it = iter(src if arm == "b_sync_pairs" else prefetch_to_device(src, 2, tr))
        for k in range(n):
            t0 = time.perf_counter()
            state, _, _ = fn(state, next(it), None)
            ms.append((time.perf_counter() - t0) * 1e3)
        for _ in it:  # (lets the prefetcher finish and hand its slots back)
            pass
        return ms[lead:]

    arms = ("a_host_goals", "b_sync_pairs", "c_prefetch", "d_prefetch_ahead")
    for arm in arms:  # warm-up: allocations, the first launches, the captured chains
        run(arm, 4, a.lead)
    med = {n: [] for n in arms}
    for _ in range(a.rounds):
        for arm in arms:
            med[arm].append(float(np.median(run(arm, a.steps, a.lead))))

    # the pair gather on its own: device events around the synchronous slot's gather
    pairs = list(pair_stream(4, 9))
    for p in pairs[:3]:
        tr.set_batch_index_pairs(p["index"], p["goal_index"])
    tr.profile(True)
    tr.profile_reset()
    for k in range(20):
        tr.set_batch_index_pairs(pairs[k & 3]["index"], pairs[k & 3]["goal_index"])
    site = tr.profile_read()["ds.gather_pairs"]
    tr.profile(False)
    gather_us = site["ms"] / site["calls"] * 1e3
    values = 2 * B * T * ecfg.img_res * ecfg.img_res * 3
    tr.close()
    ds.close()
    enc.close()

    out = {"metric": "ms per GCBC train step (aux read-back included), f16 policy + f16 encoder", "batch": B, "window": T, "rows": a.rows, "steps": a.steps,
           "lead": a.lead, "rounds": a.rounds}
    for n, v in med.items():
        out[n] = {"median_ms": round(float(np.median(v)), 4), "spread_ms": round(max(v) - min(v), 4), "round_medians_ms": [round(x, 4) for x in v]}
    base = out["a_host_goals"]["median_ms"]
    for n in arms[1:]:
        out[n]["minus_a_ms"] = round(out[n]["median_ms"] - base, 4)
    gain = out["c_prefetch"]["median_ms"] - out["d_prefetch_ahead"]["median_ms"]
    bar = max(out["c_prefetch"]["spread_ms"], out["d_prefetch_ahead"]["spread_ms"])
    out["encode_ahead_gain_ms"] = round(gain, 4)
    out["encode_ahead_gain_exceeds_larger_spread"] = bool(gain > bar)
    out["pair_gather_us"] = round(gather_us, 1)
    out["pair_gather_mb_read"] = round(values / 1e6, 1)
    out["pair_gather_mb_written"] = round(values * 4 / 1e6, 1)
    out["pair_gather_gbs"] = round(values * 5 / gather_us / 1e3, 1)

    lines = [f"box {socket.gethostname()}  date {datetime.datetime.now().isoformat(timespec='seconds')}",
             f"GCBC train step, ViT-B/16 at 256 x 256 (513 tokens per pair), f16 policy + f16 encoder, B = {B}, window {T}, {a.rows}-row synthetic set; "
             f"{a.rounds} alternating rounds of {a.steps} steps behind {a.lead} untimed; per arm: median of the round medians, spread (max - min) of the round medians"]
    for n in arms:
        r = out[n]
        lines.append(f"{n:17s} {r['median_ms']:.3f} ms (spread {r['spread_ms']:.3f})" + (f"  {r['minus_a_ms']:+.3f} ms against a_host_goals" if "minus_a_ms" in r else ""))
    lines.append(f"encode-ahead: d is {gain:.3f} ms below c, the larger spread is {bar:.3f} ms -> " +
                 ("encode-ahead stays the default for pair batches" if gain > bar else "NOT beyond the spread: encode-ahead should be off for pair batches"))
    lines.append(f"pair gather alone (one launch for both halves + the labels, device events): {gather_us:.1f} us for {values / 1e6:.1f} MB read + "
                 f"{values * 4 / 1e6:.1f} MB written = {out['pair_gather_gbs']:.0f} GB/s")
    text = "\n".join(lines) + "\n" + json.dumps(out) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
