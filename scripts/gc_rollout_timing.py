"""Wall clock of one rollout environment step with goal frames at the real geometry -- ViT-B/16 M3AE encoder at 256 x 256 (513 token rows per (frame, goal)
pair), the 26.9 M-parameter policy (window 4), f16 -- in one process, on seeded weights and frames; the protocol of scripts/rollout_step_timing.py.

  part gcbc    model GCBC at E = 1, 2 and 3 environments:
    arm (a)    the host-driven way: the host keeps the last four frames and calls PolicyTrainer.greedy_action({"image": window, "goal": the goal tiled over
               the window, "action": ...}), which encodes all 4 E pairs of the window again.
    arm (on)   RolloutSession(goal_conditioned=True).step(frame) with the encoder's row limit at 514: one new pair per environment; at E = 1 (513 rows) the
               pass runs on the latency path, at E = 2, 3 (1026, 1539 rows: over the skinny kernel's 1024-row domain) on the throughput kernels.
    arm (off)  E = 1 only: the same with the latency path disabled (arp_enc_set_latency rows = 0).  (on) against (off) is what the path is worth for a pair.
  part reward  the ARP-DT policy (257-token frames) with the clip_goal_conditioned reward of a ViT-B/16 CLIP, E = 1, 2 and 3:
    arm (a)    RolloutSession(reward_model=None).step(frame, rewards=[get_torch_clip_goal_conditioned_reward(clip, frame_e, goal_e) ...]): the host function
               runs frame AND goal through the towers at every step, one call per environment.
    arm (b)    RolloutSession(reward_model=clip, goal_conditioned=True).step(frame): the goals' features are computed at the reset; a step runs the E new
               frames through the towers beside the policy and a kernel writes -||f - g||.

Every shape is warmed up, then the arms alternate in `--rounds` rounds of `--steps` steps; a host clock wraps the calls, all of which end in a
synchronisation.  Medians per step over all timed steps, and per arm the spread of the round medians (max - min).  An untimed pass before the rounds gives the
largest difference between the arms' results for the same decisions (logits, rewards).

    python scripts/gc_rollout_timing.py [--parts gcbc,reward] [--steps 200] [--rounds 5] [--out profiles/gc_rollout_timing.txt] [--append]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="gcbc,reward")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--envs", default="1,2,3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gc_rollout_timing.txt"))
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it (one part per process)")
    a = ap.parse_args()
    import torch  # noqa: F401  -- before arp_amd: one HIP runtime per process (arp_amd/_ffi.py)
    import numpy as np

    from arp_amd import _ffi, clip, dataset, m3ae, synth, synth_policy as S
    from arp_amd.label_reward import get_torch_clip_goal_conditioned_reward
    from arp_amd.rollout import RolloutSession
    from arp_amd.train import PolicyConfig, PolicyTrainer
    _ffi.require_gpu()
    ecfg = m3ae.EncoderConfig()
    EP = S.m3ae_params(ecfg, seed=0)
    n_frames = 64
    pool = synth.procgen_like_frames(3 * n_frames, seed=7).reshape(n_frames, 3, 256, 256, 3)
    goals = synth.procgen_like_frames(3, seed=8)
    envs = [int(v) for v in a.envs.split(",")]
    lines, results = [], {}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn, k0, n):
        ts = np.empty(n)
        for i in range(n):
            t0 = time.perf_counter()
            fn(k0 + i)
            ts[i] = time.perf_counter() - t0
        return ts * 1e3

    def rounds_of(arms, before):
        """arms: name -> step function of the frame index; before(name) makes the arm current.  Returns name -> {median, round medians, spread}."""
        got = {name: [] for name in arms}
        for name, fn in arms.items():  # warm-up of every shape
            before(name)
            timed(fn, 0, a.warmup)
        for r in range(a.rounds):
            for name, fn in arms.items():
                before(name)
                timed(fn, 0, 3)  # (the arm's captured chains are current again)
                got[name].append(timed(fn, r * a.steps, a.steps))
        out = {}
        for name, rs in got.items():
            med = [float(np.median(x)) for x in rs]
            out[name] = {"median_ms": float(np.median(np.concatenate(rs))), "round_medians_ms": [round(m, 4) for m in med], "spread_ms": max(med) - min(med)}
        return out

    say(f"gc_rollout_timing ({a.parts}): {a.rounds} rounds x {a.steps} steps per arm, warm-up {a.warmup} steps per shape; ms per environment step (wall clock, each call ends in a sync)")
    if "gcbc" in a.parts.split(","):
        cfg = PolicyConfig(model="GCBC", enc_tokens=ecfg.gc_tokens)
        T = cfg.window
        enc = m3ae.M3AEEncoder(ecfg, EP, mode="f16")
        tr = PolicyTrainer(cfg, mode="f16")
        tr.set_params(S.policy_params(cfg, seed=0))
        tr.attach_encoder(enc)
        results["gcbc"] = []
        for E in envs:
            ses = RolloutSession(tr, n_envs=E, goal_conditioned=True)
            goal32 = np.repeat(dataset.bytes_to_float(goals[:E])[:, None], T, axis=1)  # the goal tiled over the window
            state = {"win": None, "act": None}

            def frames_at(k):
                return np.ascontiguousarray(pool[k % n_frames, :E])

            def step_a(k):
                state["win"] = state["win"][1:] + [frames_at(k)]
                acts = state["act"][1:] + [np.zeros(E, np.int32)]
                batch = {"image": {"ob": dataset.bytes_to_float(np.stack(state["win"], axis=1))}, "goal": {"ob": goal32}, "action": np.stack(acts, axis=1)}
                act = tr.greedy_action(batch)
                state["act"] = state["act"][1:] + [act.astype(np.int32)]

            def step_s(k):
                ses.step(frames_at(k))

            # the largest logit difference between the two ways of computing the same decision (the host-driven call is given the session's action history)
            ses.reset(goals=goals[:E]); enc.set_latency_rows(514)
            hist, diff, n_cmp = [], 0.0, 0
            for k in range(n_frames // 4 + T - 1):
                hist = (hist + [frames_at(k)])[-T:]
                ses.step(hist[-1])
                if len(hist) == T:
                    lb, aw = ses.read("logits")[:, -1], ses.read("action_window")
                    tr.set_batch_images(dataset.bytes_to_float(np.stack(hist, axis=1)), aw, goals=goal32)
                    diff = max(diff, float(np.abs(tr.forward()["action_pred"][:, -1] - lb).max()))
                    n_cmp += 1
            state["win"], state["act"] = [frames_at(0)] * T, [np.zeros(E, np.int32)] * T  # (timing only: the window is full from the start)
            ses.reset()
            arms = {"a": step_a, "on": step_s}
            if E == 1:
                arms["off"] = step_s
            res = rounds_of(arms, lambda name: enc.set_latency_rows(0 if name == "off" else 514))
            enc.set_latency_rows(m3ae.LATENCY_ROWS_DEFAULT)
            res.update({"E": E, "rows_per_step": E * ecfg.gc_tokens, "max_logit_diff_a_vs_on": diff, "logit_comparisons": n_cmp})
            line = (f"GCBC E={E} ({E * ecfg.gc_tokens} encoder rows per session step): (a) host-driven greedy_action {res['a']['median_ms']:.3f} ms (spread {res['a']['spread_ms']:.3f}) | "
                    f"(on) session, row limit 514 {res['on']['median_ms']:.3f} ms (spread {res['on']['spread_ms']:.3f}) | a/on {res['a']['median_ms'] / res['on']['median_ms']:.2f}x")
            if E == 1:
                gain, bar = res["off"]["median_ms"] - res["on"]["median_ms"], max(res["on"]["spread_ms"], res["off"]["spread_ms"])
                res["latency_path_wins"] = bool(gain > bar)
                line += (f" | (off) session, latency path off {res['off']['median_ms']:.3f} ms (spread {res['off']['spread_ms']:.3f}) | off - on {gain:+.3f} ms against the larger "
                         f"spread {bar:.3f}: the latency path {'WINS' if gain > bar else 'does NOT win'} at one pair")
            say(line + f" | max logit diff a vs on {diff:.2e} over {n_cmp} decisions of an untimed pass")
            results["gcbc"].append(res)
            ses.close()
        tr.close(); enc.close()
    if "reward" in a.parts.split(","):
        cfg = PolicyConfig(lambda_ret=0.01)
        scale = 100.0
        ccfg = clip.ClipConfig(patch=16)
        lab = clip.ClipLabeller(ccfg, synth.clip_weights(ccfg, seed=1), mode="f16", max_batch=64, n_streams=1)  # (no prompt set: the goal reward reads images only)
        enc = m3ae.M3AEEncoder(ecfg, EP, mode="f16")
        tr = PolicyTrainer(cfg, mode="f16")
        tr.set_params(S.policy_params(cfg, seed=0))
        tr.attach_encoder(enc)
        results["reward"] = []
        for E in envs:
            host = RolloutSession(tr, n_envs=E, return_to_go=100.0, scale=scale)
            dev = RolloutSession(tr, reward_model=lab, n_envs=E, return_to_go=100.0, scale=scale, goal_conditioned=True)

            def frames_at(k):
                return np.ascontiguousarray(pool[k % n_frames, :E])

            def step_a(k):
                fr = frames_at(k)
                host.step(fr, rewards=[get_torch_clip_goal_conditioned_reward(lab, fr[e], goals[e]) for e in range(E)])

            def step_b(k):
                dev.step(frames_at(k))

            host.reset(); dev.reset(goals=goals[:E])
            diff = 0.0
            for k in range(n_frames // 4):
                fr = frames_at(k)
                dev.step(fr)
                want = np.asarray([get_torch_clip_goal_conditioned_reward(lab, fr[e], goals[e]) for e in range(E)])
                diff = max(diff, float(np.abs(dev.read("reward") - want).max()))
            host.reset(); dev.reset()
            res = rounds_of({"a": step_a, "b": step_b}, lambda name: None)
            res.update({"E": E, "max_reward_diff_a_vs_b": diff})
            res["b_below_a_by_more_than_the_larger_spread"] = bool(res["a"]["median_ms"] - res["b"]["median_ms"] > max(res["a"]["spread_ms"], res["b"]["spread_ms"]))
            say(f"goal reward E={E}: (a) session + host get_torch_clip_goal_conditioned_reward {res['a']['median_ms']:.3f} ms (spread {res['a']['spread_ms']:.3f}) | (b) session, goal "
                f"reward on the device {res['b']['median_ms']:.3f} ms (spread {res['b']['spread_ms']:.3f}) | a/b {res['a']['median_ms'] / res['b']['median_ms']:.2f}x | max reward diff a vs b "
                f"{diff:.2e} over {n_frames // 4} steps of an untimed pass")
            results["reward"].append(res)
            host.close(); dev.close()
        tr.close(); enc.close(); lab.close()
    say(json.dumps({"gc_rollout_timing": results}))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
