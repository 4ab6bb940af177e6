"""The goal-conditioned pass of the frozen M3AE encoder beside the plain pass, and one GCBC train step beside the ARP-DT frames-in step, on one GPU.

Encoder (ViT-B/16 at 256 x 256, f16 and bf16, seeded weights and frames), timed with the encoder's own site profiler (device events around every site):
  gc_128     forward_gc_representations of 128 (frame, goal) pairs: 513 tokens per pair, 65 664 token rows, on the key-blocked attention
  plain_256  forward_representation of 256 frames: 257 tokens per frame, 65 792 token rows -- code the tree has had all along: the comparator
The two passes run the same patch rows and the same GEMM rows within 0.2 % and differ in the `m3ae.attn` site alone, where the gc pass does
513^2 / (2 * 257^2) = 1.99x the MACs.  One part stream (set_streams(1)), so that a pass's site times add up to its device time.  Both passes are warmed
up; then `--rounds` alternating rounds of `--passes` passes each (about 0.2 s of device work per window); the medians, and the range, over the rounds of the whole-pass time (the sum of the sites) and of the
`m3ae.attn` site, and their ratios, are reported.

Policy step (B = 32, window 4, f16 policy + f16 encoder, the synchronous slot, no encode-ahead): a GCBC step on frames + goals beside the ARP-DT step on
frames, wall clock per step over `--steps` steps, alternating rounds, medians and ranges.

Writes profiles/gc_encoder_timing.txt (the box, the date, the medians and ranges) and prints it.

    python scripts/gc_encoder_timing.py [--rounds 5] [--passes 10] [--steps 20] [--pairs 128]
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


def _sites(enc):
    return {k: v["ms"] for k, v in enc.profile_read().items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--passes", type=int, default=10, help="encoder passes per timed window")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=128)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gc_encoder_timing.txt"))
    a = ap.parse_args()
    import torch  # noqa: F401  -- before arp_amd: one HIP runtime per process (arp_amd/_ffi.py)
    import numpy as np

    from arp_amd import _ffi, m3ae, synth_policy as S
    from arp_amd.train import PolicyConfig, PolicyTrainer
    from oracle import m3ae_np as M
    _ffi.require_gpu()
    ecfg = m3ae.EncoderConfig()
    EP = S.m3ae_params(M.EncConfig(), seed=0)
    n = a.pairs
    # a few distinct frames, tiled: the kernels' time does not depend on the values, and 2 n full-size frames need not be synthesised one by one
    base = S.normalized_frames(8, ecfg.img_res, seed=1)
    frames = np.ascontiguousarray(np.tile(base, (2 * n // 8 + 1, 1, 1, 1))[:2 * n])
    lines = [f"box {socket.gethostname()}  date {datetime.datetime.now().isoformat(timespec='seconds')}",
             f"encoder ViT-B/16 at 256 x 256; gc pass of {n} pairs (513 tokens) against a plain pass of {2 * n} frames (257 tokens); {a.rounds} alternating rounds of {a.passes} passes each, per pass: median [min .. max] over the rounds; one part stream"]
    result = {}
    for mode in ("f16", "bf16"):
        enc = m3ae.M3AEEncoder(ecfg, EP, mode=mode, max_frames=128)
        enc.set_streams(1)
        enc.forward_gc_representations(frames[:n], frames[n:])   # warm-up (allocations, first launches)
        enc.forward_representation(frames)
        enc.profile(True)
        tot = {"gc": [], "plain": []}
        att = {"gc": [], "plain": []}
        for _ in range(a.rounds):
            for name in ("gc", "plain"):
                before = _sites(enc)
                for _ in range(a.passes):
                    if name == "gc":
                        enc.forward_gc_representations(frames[:n], frames[n:])
                    else:
                        enc.forward_representation(frames)
                after = _sites(enc)
                d = {k: (after[k] - before.get(k, 0.0)) / a.passes for k in after}
                tot[name].append(sum(d.values()))
                att[name].append(d.get("m3ae.attn", 0.0))
        enc.close()
        r = {f"{k}_{w}_ms": float(np.median(v)) for w, src in (("pass", tot), ("attn", att)) for k, v in src.items()}
        r.update({f"{k}_{w}_range_ms": [float(min(v)), float(max(v))] for w, src in (("pass", tot), ("attn", att)) for k, v in src.items()})
        rng = lambda key: "[{:.3f} .. {:.3f}]".format(*r[key])
        r["pass_ratio"] = r["gc_pass_ms"] / r["plain_pass_ms"]
        r["attn_ratio"] = r["gc_attn_ms"] / r["plain_attn_ms"] if r["plain_attn_ms"] > 0 else float("nan")
        r["attn_time_per_mac_ratio"] = r["attn_ratio"] / (513.0 ** 2 * n / (257.0 ** 2 * 2 * n))
        result[mode] = r
        lines.append(f"{mode}: whole pass gc {r['gc_pass_ms']:.3f} ms {rng('gc_pass_range_ms')}, plain {r['plain_pass_ms']:.3f} ms {rng('plain_pass_range_ms')}, "
                     f"ratio {r['pass_ratio']:.3f};  m3ae.attn gc {r['gc_attn_ms']:.3f} ms {rng('gc_attn_range_ms')}, "
                     f"plain {r['plain_attn_ms']:.3f} ms {rng('plain_attn_range_ms')}, ratio {r['attn_ratio']:.3f} at 1.99x the MACs (time per MAC {r['attn_time_per_mac_ratio']:.2f}x the N = 257 instance's)")
    # ---- one train step: GCBC on frames + goals, ARP-DT on frames, the same run
    B, T, res = a.batch, 4, ecfg.img_res
    enc = m3ae.M3AEEncoder(ecfg, EP, mode="f16", max_frames=128)
    fr = frames[:B * T].reshape(B, T, res, res, 3)
    go = frames[B * T:2 * B * T].reshape(B, T, res, res, 3)
    act = np.random.default_rng(2).integers(0, 15, (B, T)).astype(np.int32)
    rtg = np.random.default_rng(3).random((B, T, 1)).astype(np.float32)
    gcfg, acfg = PolicyConfig(model="GCBC", enc_tokens=ecfg.gc_tokens), PolicyConfig(lambda_ret=0.01)
    g = PolicyTrainer(gcfg, mode="f16"); g.set_params(S.policy_params(gcfg, seed=0)); g.attach_encoder(enc); g.set_batch_images(fr, act, goals=go)
    p = PolicyTrainer(acfg, mode="f16"); p.set_params(S.policy_params(acfg, seed=0)); p.attach_encoder(enc); p.set_batch_images(fr, act, rtg)
    for tr in (g, p):
        for _ in range(3):
            tr.train_step(5e-4)
    step = {"gcbc": [], "arpdt": []}
    for _ in range(a.rounds):
        for name, tr in (("gcbc", g), ("arpdt", p)):
            t0 = time.perf_counter()
            for _ in range(a.steps):
                tr.train_step(5e-4)   # (returns the step's aux: synchronous)
            step[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
    g.close(); p.close(); enc.close()
    result["step"] = {k + "_ms": float(np.median(v)) for k, v in step.items()}
    result["step"].update({k + "_range_ms": [float(min(v)), float(max(v))] for k, v in step.items()})
    lines.append(f"train step, B = {B}, window {T}, f16 policy + f16 encoder, synchronous slot, no encode-ahead: GCBC (frames + goals, {B * T} pairs) "
                 f"{result['step']['gcbc_ms']:.3f} ms [{result['step']['gcbc_range_ms'][0]:.3f} .. {result['step']['gcbc_range_ms'][1]:.3f}], "
                 f"ARP-DT (frames, {B * T} frames) {result['step']['arpdt_ms']:.3f} ms [{result['step']['arpdt_range_ms'][0]:.3f} .. {result['step']['arpdt_range_ms'][1]:.3f}]")
    text = "\n".join(lines) + "\n" + json.dumps(result) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
