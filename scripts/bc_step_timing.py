"""Step time of the InstructRL baseline (PolicyConfig(model="BC")) beside ARP-DT's, encodings in, B = 32, window 4, f16 (the default mode), on one GPU.

Three configurations, each a trainer of its own with its batch resident in HBM:
  arpdt_257  ARP-DT, 257 encoder tokens (bench.py --path policy's step)
  bc_257     BC at the same encodings: two tokens per time step, no return head -- strictly less work than arpdt_257
  bc_334     BC at the reference's InstructRL encodings, 1 + 256 + 77 = 334 tokens (image + instruction text): the adapter and image_text_input grow 1.30x

Every configuration is warmed up first (its step graphs captured); then the three are timed in alternation, `--rounds` times `--steps` steps each,
with device events recorded on the trainer's stream around each block.  Prints one JSON line: the median and the range of ms per step per configuration.

    python scripts/bc_step_timing.py [--steps 20] [--warmup 10] [--rounds 5]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    a = ap.parse_args()
    import torch  # noqa: F401  -- before arp_amd: one HIP runtime per process (arp_amd/_ffi.py)
    import numpy as np

    from arp_amd import _ffi, clip, synth_policy as S
    from arp_amd.train import PolicyConfig, PolicyTrainer
    _ffi.require_gpu()
    cfgs = {"arpdt_257": PolicyConfig(lambda_ret=0.01), "bc_257": PolicyConfig(model="BC"), "bc_334": PolicyConfig(model="BC", enc_tokens=334)}
    trainers = {}
    for name, cfg in cfgs.items():
        tr = PolicyTrainer(cfg, mode="f16")
        tr.set_params(S.policy_params(cfg, seed=0))
        enc, act, rtg = S.policy_batch(cfg, a.batch, seed=100)
        tr.set_batch(enc, act, rtg)  # (BC ignores the rtg)
        for _ in range(a.warmup):
            tr.train_step_async(5e-4)
        tr.sync()
        trainers[name] = tr
    times = {n: [] for n in cfgs}
    e0, e1 = clip.Event(), clip.Event()
    for _ in range(a.rounds):
        for name, tr in trainers.items():
            tr.record(e0)
            for _ in range(a.steps):
                tr.train_step_async(5e-4)
            tr.record(e1)
            times[name].append(clip.elapsed_ms(e0, e1) / a.steps)  # (synchronises on e1)
    for tr in trainers.values():
        tr.close()
    out = {"metric": "ms per policy train step, encodings in, f16", "batch": a.batch, "window": 4, "steps": a.steps, "rounds": a.rounds, "warmup": a.warmup}
    for n, v in times.items():
        out[n] = {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
