"""The image + text pass of the frozen M3AE encoder (InstructRL's encoder call) beside the plain pass, what the masked attention's block skip buys, and
one InstructRL (BC) train step with frames in beside the ARP-DT frames-in step, on one GPU.  Method of scripts/gc_encoder_timing.py: one box, one process,
ViT-B/16 at 256 x 256, seeded weights and frames, `--rounds` alternating rounds, medians with the range of the round medians.

(1) Encoder pass, f16 and bf16, the encoder's own site profiler (device events around every site), one part stream so that the sites add up:
      text_12   forward_representation(frames, text, mask) of 256 frames, L = 77 with 12 valid tokens: 334 rows per frame, 269 visible keys -- 5 of the 6
                key blocks of 64 executed (block 5 wholly hidden, skipped), block 4 partly hidden
      plain     forward_representation(frames) of 256 frames: 257 rows per frame -- the comparator, code the tree has had all along
    Derived, for comparison only: 334 / 257 = 1.30x the rows; nominal attention MACs 334^2 / 257^2 = 1.69x.
(2) Block skip: text_77, the same pass with all 77 tokens valid (6 of 6 key blocks executed).  text_77 - text_12 in `m3ae.attn` is what the skip buys.
(3) Train step, B = 32, window 4, f16 policy + f16 encoder, wall clock per step: InstructRL on frames with the instruction attached -- the synchronous slot
    (the step encodes its own batch at its head), host batches through prefetch_to_device without encode-ahead (ARP_DT_ENCODE_AHEAD=0) and with it --
    beside ARP-DT's synchronous-slot step on frames in the same run.  The rule the figures carry: encode-ahead stays prefetch_to_device's default for
    these batches only if it is lower than the arm without it by more than the larger spread of the two.
(4) Rollout, f16 + f16: RolloutSession(instruct=...).step at 1 / 2 / 3 environments (one new frame per environment encoded, 334 rows each) against the
    host-driven way (greedy_action on the window's T frames, all encoded again); at one environment the encoder's latency path on (row limit 514) / off.
    The rule: text calls of a session take the latency path by default only if it is lower by more than the larger spread.

Not measured here: bf16 steps and rollouts, a second box, real BERT / M3AE weights, a real episode.

Writes profiles/instructrl_timing.txt (or --out) and prints it.

    python scripts/instructrl_timing.py [--rounds 5] [--passes 5] [--steps 20] [--frames 256]
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
L, VOCAB = 77, 30522


def _sites(enc):
    return {k: v["ms"] for k, v in enc.profile_read().items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--passes", type=int, default=5, help="encoder passes per timed window")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rollout-steps", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "instructrl_timing.txt"))
    a = ap.parse_args()
    import torch  # noqa: F401  -- before arp_amd: one HIP runtime per process (arp_amd/_ffi.py)
    import numpy as np

    from arp_amd import _ffi, m3ae, synth_policy as S
    from arp_amd.rollout import RolloutSession
    from arp_amd.train import PolicyConfig, PolicyTrainer, TrainState, create_train_step, prefetch_to_device
    from oracle import m3ae_np as M
    _ffi.require_gpu()
    ecfg = m3ae.EncoderConfig()
    EP = S.add_m3ae_text_params(S.m3ae_params(M.EncConfig(), seed=0), M.EncConfig(), vocab=VOCAB, seed=0)
    n = a.frames
    base = S.normalized_frames(8, ecfg.img_res, seed=1)   # a few distinct frames, tiled: the kernels' time does not depend on the values
    frames = np.ascontiguousarray(np.tile(base, (n // 8 + 1, 1, 1, 1))[:n])
    tok = np.random.default_rng(2).integers(0, VOCAB, L).astype(np.int32)
    masks = {"text_12": (np.arange(L) >= 12).astype(np.float32), "text_77": np.zeros(L, np.float32)}
    lines = [f"box {socket.gethostname()}  date {datetime.datetime.now().isoformat(timespec='seconds')}",
             f"encoder ViT-B/16 at 256 x 256, {n} frames per pass; text pass L = {L} (334 rows per frame) with 12 and with 77 valid tokens against the plain pass "
             f"(257 rows); {a.rounds} alternating rounds of {a.passes} passes each, per pass: median [min .. max] over the rounds; one part stream"]
    result = {}
    names = ("text_12", "text_77", "plain")
    for mode in ("f16", "bf16"):
        enc = m3ae.M3AEEncoder(ecfg, EP, mode=mode, max_frames=128)
        enc.set_streams(1)
        run = {"plain": lambda: enc.forward_representation(frames)}
        for k, m in masks.items():
            run[k] = (lambda m: lambda: enc.forward_representation(frames, tok, m))(m)
        for k in names:
            run[k]()   # warm-up (allocations, first launches)
        enc.profile(True)
        tot, att = {k: [] for k in names}, {k: [] for k in names}
        for _ in range(a.rounds):
            for k in names:
                before = _sites(enc)
                for _ in range(a.passes):
                    run[k]()
                after = _sites(enc)
                d = {s: (after[s] - before.get(s, 0.0)) / a.passes for s in after}
                tot[k].append(sum(d.values()))
                att[k].append(d.get("m3ae.attn", 0.0))
        enc.close()
        r = {}
        for w, src in (("pass", tot), ("attn", att)):
            for k, v in src.items():
                r[f"{k}_{w}_ms"] = float(np.median(v))
                r[f"{k}_{w}_range_ms"] = [float(min(v)), float(max(v))]
        r["pass_ratio_text12_plain"] = r["text_12_pass_ms"] / r["plain_pass_ms"]
        r["attn_ratio_text12_plain"] = r["text_12_attn_ms"] / r["plain_attn_ms"]
        r["block_skip_attn_ms"] = r["text_77_attn_ms"] - r["text_12_attn_ms"]
        result[mode] = r
        f = lambda k: "{:.3f} ms [{:.3f} .. {:.3f}]".format(r[k + "_ms"], *r[k + "_range_ms"])
        lines.append(f"{mode}: whole pass text_12 {f('text_12_pass')}, text_77 {f('text_77_pass')}, plain {f('plain_pass')}, text_12 / plain {r['pass_ratio_text12_plain']:.3f} "
                     f"(1.30x the rows);  m3ae.attn text_12 {f('text_12_attn')}, text_77 {f('text_77_attn')}, plain {f('plain_attn')}, text_12 / plain "
                     f"{r['attn_ratio_text12_plain']:.3f} (1.69x the nominal MACs, 5 of 6 key blocks executed);  block skip: text_77 - text_12 = {r['block_skip_attn_ms']:.3f} ms of m3ae.attn per pass")
    # ---- (3) one train step: InstructRL on frames with the instruction, ARP-DT on frames, the same run
    B, T, res = a.batch, 4, ecfg.img_res
    enc = m3ae.M3AEEncoder(ecfg, EP, mode="f16", max_frames=128)
    fr = np.ascontiguousarray(np.tile(base, (B * T // 8 + 1, 1, 1, 1))[:B * T]).reshape(B, T, res, res, 3)
    act = np.random.default_rng(2).integers(0, 15, (B, T)).astype(np.int32)
    rtg = np.random.default_rng(3).random((B, T, 1)).astype(np.float32)
    bcfg, acfg = PolicyConfig(model="BC", enc_tokens=ecfg.text_tokens(L)), PolicyConfig(lambda_ret=0.01)
    b = PolicyTrainer(bcfg, mode="f16"); b.set_params(S.policy_params(bcfg, seed=0)); b.attach_encoder(enc, instruct=tok, text_padding_mask=masks["text_12"])
    b.set_batch_images(fr, act)
    p = PolicyTrainer(acfg, mode="f16"); p.set_params(S.policy_params(acfg, seed=0)); p.attach_encoder(enc); p.set_batch_images(fr, act, rtg)
    for tr in (b, p):
        for _ in range(3):
            tr.train_step(5e-4)
    step = {"instructrl": [], "arpdt": []}
    for _ in range(a.rounds):
        for name, tr in (("instructrl", b), ("arpdt", p)):
            t0 = time.perf_counter()
            for _ in range(a.steps):
                tr.train_step(5e-4)   # (returns the step's aux: synchronous)
            step[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
    # the prefetched arms: the same host batch over and over through prefetch_to_device (101 MB of frames over PCIe per step), encode-ahead off / on
    fn = create_train_step(bcfg, lambda s_: 5e-4, bcfg.weight_decay)
    batch = {"image": {"ob": fr}, "action": act, "instruct": tok[None], "text_padding_mask": masks["text_12"][None]}
    for name in ("prefetch_no_ahead", "prefetch_ahead"):
        step[name] = []
    for rnd in range(a.rounds + 1):   # round 0: warm-up of both arms
        for name, flag in (("prefetch_no_ahead", "0"), ("prefetch_ahead", "1")):
            os.environ["ARP_DT_ENCODE_AHEAD"] = flag
            state, t0, k = TrainState(b), None, 0
            for dev_batch in prefetch_to_device((batch for _ in range(a.steps + 2)), 2, b):
                if k == 2:
                    t0 = time.perf_counter()   # (the first two steps fill the pipeline)
                state, _, _ = fn(state, dev_batch, None)
                k += 1
            if rnd:
                step[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
    os.environ.pop("ARP_DT_ENCODE_AHEAD", None)
    b.close(); p.close()
    # ---- (4) the rollout session with the instruction against the host-driven way
    from arp_amd import dataset, synth
    pool = synth.procgen_like_frames(3 * 32, seed=7).reshape(32, 3, res, res, 3)
    rb = PolicyTrainer(bcfg, mode="f16"); rb.set_params(S.policy_params(bcfg, seed=0)); rb.attach_encoder(enc, instruct=tok, text_padding_mask=masks["text_12"])
    roll = {}

    def timed(f, n):
        ts = np.empty(n)
        for i in range(n):
            t0 = time.perf_counter()
            f(i)
            ts[i] = time.perf_counter() - t0
        return float(np.median(ts * 1e3))
    for E in (1, 2, 3):
        ses = RolloutSession(rb, n_envs=E, instruct=(tok, masks["text_12"]))
        ses.reset()
        st = {"win": [np.ascontiguousarray(pool[0, :E])] * T, "act": [np.zeros(E, np.int32)] * T}

        def step_s(k):
            ses.step(np.ascontiguousarray(pool[k % 32, :E]))

        def step_h(k):
            st["win"] = st["win"][1:] + [np.ascontiguousarray(pool[k % 32, :E])]
            acts = st["act"][1:] + [np.zeros(E, np.int32)]
            got = rb.greedy_action({"image": {"ob": dataset.bytes_to_float(np.stack(st["win"], axis=1))}, "action": np.stack(acts, axis=1)})
            st["act"] = st["act"][1:] + [got.astype(np.int32)]
        arms = {"host": (step_h, 514), "on": (step_s, 514)}
        if E == 1:
            arms["off"] = (step_s, 0)
        got = {k: [] for k in arms}
        for rnd in range(a.rounds + 1):   # round 0: warm-up
            for k, (f, rows) in arms.items():
                enc.set_latency_rows(rows)
                timed(f, 3)
                m = timed(f, a.rollout_steps)
                if rnd:
                    got[k].append(m)
        enc.set_latency_rows(m3ae.LATENCY_ROWS_DEFAULT)
        ses.close()
        roll[E] = {k: {"median_ms": float(np.median(v)), "spread_ms": float(max(v) - min(v))} for k, v in got.items()}
    rb.close(); enc.close()
    result["rollout"] = roll
    result["step"] = {k + "_ms": float(np.median(v)) for k, v in step.items()}
    result["step"].update({k + "_range_ms": [float(min(v)), float(max(v))] for k, v in step.items()})
    s = result["step"]
    lines.append(f"train step, B = {B}, window {T}, f16 policy + f16 encoder, synchronous slot: InstructRL (frames + the instruction, {B * T} frames x 334 rows) "
                 f"{s['instructrl_ms']:.3f} ms [{s['instructrl_range_ms'][0]:.3f} .. {s['instructrl_range_ms'][1]:.3f}], "
                 f"ARP-DT (frames, {B * T} frames x 257 rows) {s['arpdt_ms']:.3f} ms [{s['arpdt_range_ms'][0]:.3f} .. {s['arpdt_range_ms'][1]:.3f}]")
    gain = s["prefetch_no_ahead_ms"] - s["prefetch_ahead_ms"]
    bar = max(s[k + "_range_ms"][1] - s[k + "_range_ms"][0] for k in ("prefetch_no_ahead", "prefetch_ahead"))
    result["step"]["encode_ahead_gain_ms"], result["step"]["encode_ahead_wins"] = gain, bool(gain > bar)
    lines.append(f"  InstructRL prefetched (host batches, 101 MB of frames per step): without encode-ahead {s['prefetch_no_ahead_ms']:.3f} ms "
                 f"[{s['prefetch_no_ahead_range_ms'][0]:.3f} .. {s['prefetch_no_ahead_range_ms'][1]:.3f}], with encode-ahead {s['prefetch_ahead_ms']:.3f} ms "
                 f"[{s['prefetch_ahead_range_ms'][0]:.3f} .. {s['prefetch_ahead_range_ms'][1]:.3f}]: lower by {gain:+.3f} ms against the larger spread {bar:.3f}: "
                 f"encode-ahead {'STAYS' if gain > bar else 'does NOT earn'} the default for these batches")
    for E, r in roll.items():
        line = (f"rollout E={E} ({E * 334} encoder rows per session step), f16 + f16, {a.rounds} rounds x {a.rollout_steps} steps, median ms per step (spread of the round medians): "
                f"host-driven greedy_action {r['host']['median_ms']:.3f} ({r['host']['spread_ms']:.3f}) | session {r['on']['median_ms']:.3f} ({r['on']['spread_ms']:.3f}) | "
                f"{r['host']['median_ms'] / r['on']['median_ms']:.2f}x")
        if "off" in r:
            g, br = r["off"]["median_ms"] - r["on"]["median_ms"], max(r["on"]["spread_ms"], r["off"]["spread_ms"])
            result["rollout"][E]["latency_path_wins"] = bool(g > br)
            line += (f" | session with the latency path off {r['off']['median_ms']:.3f} ({r['off']['spread_ms']:.3f}): off - on {g:+.3f} ms against the larger spread {br:.3f}: "
                     f"the latency path {'WINS' if g > br else 'does NOT win'} at one frame + instruction (334 rows)")
        lines.append(line)
    lines.append("not measured: bf16 steps and rollouts, a second box, real BERT / M3AE weights, a real episode")
    text = "\n".join(lines) + "\n" + json.dumps(result) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
