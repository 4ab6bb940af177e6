"""Wall clock of one rollout environment step at the real geometry -- ViT-B/16 M3AE encoder at 256 x 256, the 26.9 M-parameter policy (window 4), a
ViT-B/16 CLIP reward -- the parent's host-driven way against the device-resident session (arp_amd.rollout.RolloutSession), in one process, on
synthetic weights and frames.  f16 policy; the encoder in f16, then in bf16; E = 1, 2 and 3 environments (257, 514, 771 encoder rows per step).

  arm (a)  the host keeps the last four frames: dataset.bytes_to_float -> PolicyTrainer.greedy_action(window [E, 4, 256, 256, 3] f32) ->
           get_torch_clip_reward(frame) -> return-to-go decremented on the host.  Four frames encoded and 3.1 MB uploaded per environment and step.
  arm (b)  session.step(frame) as the product runs it: one uint8 frame per environment up, the encoder on the new frames only -- on its latency path up
           to the default row limit (514 rows = two frames), on the throughput kernels above it --, one host wait.
  arm (b1) arm (b) with the row limit forced to 1024 (the latency path at every E here): differs from (b) at E = 3 only.
  arm (b0) arm (b) with the encoder's latency path disabled (arp_enc_set_latency rows = 0): what the path itself is worth.

Every shape is warmed up (the policy's forward chain and the labeller's single-frame pass are captured on their third call), then the arms alternate in
`--rounds` rounds of `--steps` steps; a host clock wraps the calls, all of which end in a synchronisation.  Medians per step over all timed steps, and per
arm the spread of the round medians (max - min).  Also: the largest logit difference between arm (a)'s and arm (b)'s computation of the same
decisions, in an untimed pass of its own over every frame the timed rounds use (the frame pool, once round: pool + window - 1 steps, one comparison per
step with a full window; the same frames, actions and returns-to-go on both sides).

    python scripts/rollout_step_timing.py [--steps 200] [--rounds 5] [--out profiles/rollout_step_timing.txt]
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
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--envs", default="1,2,3")
    ap.add_argument("--encoder-modes", default="f16,bf16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_step_timing.txt"))
    a = ap.parse_args()
    import torch  # noqa: F401  -- before arp_amd: one HIP runtime per process (arp_amd/_ffi.py)
    import numpy as np

    from arp_amd import _ffi, clip, dataset, m3ae, synth, synth_policy as S
    from arp_amd.label_reward import get_torch_clip_reward
    from arp_amd.rollout import RolloutSession
    from arp_amd.train import PolicyConfig, PolicyTrainer
    _ffi.require_gpu()
    cfg, ecfg = PolicyConfig(lambda_ret=0.01), m3ae.EncoderConfig()
    T, scale = cfg.window, 100.0
    ccfg = clip.ClipConfig(patch=16)
    lab = clip.ClipLabeller(ccfg, synth.clip_weights(ccfg, seed=1), mode="f16", max_batch=64, n_streams=1).set_text(synth.prompt_tokens(1, 8, seed=2))
    EP, PP = S.m3ae_params(ecfg, seed=0), S.policy_params(cfg, seed=0)
    n_frames = 64
    pool = synth.procgen_like_frames(3 * n_frames, seed=7).reshape(n_frames, 3, 256, 256, 3)
    lines, results = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"rollout_step_timing: {a.rounds} rounds x {a.steps} steps per arm, warm-up {a.warmup} steps per shape; ms per environment step (wall clock, each call ends in a sync)")
    for emode in a.encoder_modes.split(","):
        enc = m3ae.M3AEEncoder(ecfg, EP, mode=emode)
        tr = PolicyTrainer(cfg, mode="f16")
        tr.set_params(PP)
        tr.attach_encoder(enc)
        for E in [int(v) for v in a.envs.split(",")]:
            ses = RolloutSession(tr, reward_model=lab, n_envs=E, return_to_go=100.0, scale=scale)
            state = {"k": 0, "win": None, "rtg_hist": None, "rtg": None, "act": None, "diff": 0.0}

            def frames_at(k):
                return np.ascontiguousarray(pool[k % n_frames, :E])

            def reset_a():
                state["win"] = [frames_at(0)] * T  # (timing only: the window is full from the start)
                state["rtg"] = np.full(E, 100.0 / scale, np.float32)
                state["rtg_hist"] = [state["rtg"].copy()] * T
                state["act"] = [np.zeros(E, np.int32)] * T

            def step_a(k):
                fr = frames_at(k)
                state["win"] = state["win"][1:] + [fr]
                state["rtg_hist"] = state["rtg_hist"][1:] + [state["rtg"].copy()]
                acts = state["act"][1:] + [np.zeros(E, np.int32)]
                window = dataset.bytes_to_float(np.stack(state["win"], axis=1))
                act = tr.greedy_action(window, np.stack(acts, axis=1), np.stack(state["rtg_hist"], axis=1)[..., None])
                state["act"] = state["act"][1:] + [act.astype(np.int32)]
                r = get_torch_clip_reward(lab, fr)
                state["rtg"] = state["rtg"] - r / np.float32(scale)
                return act

            def run(arm, k0, n):
                ts = np.empty(n)
                for i in range(n):
                    t0 = time.perf_counter()
                    if arm == "a":
                        step_a(k0 + i)
                    else:
                        ses.step(frames_at(k0 + i))
                    ts[i] = time.perf_counter() - t0
                return ts * 1e3

            # The largest logit difference between the arms' ways of computing the same decision: behind every session step with a full window the parent's
            # call (host window of f32 frames through greedy_action's path: four frames encoded on the throughput kernels) is given the session's own action
            # and return-to-go history, so that the two differ in nothing but how the logits are computed.
            ses.reset(); enc.set_latency_rows(m3ae.LATENCY_ROWS_DEFAULT)
            hist, n_cmp = [], 0
            for k in range(n_frames + T - 1):
                hist = (hist + [frames_at(k)])[-T:]
                ses.step(hist[-1])
                if len(hist) == T:
                    lb, aw, rw = ses.read("logits")[:, -1], ses.read("action_window"), ses.read("rtg_window")
                    tr.set_batch_images(dataset.bytes_to_float(np.stack(hist, axis=1)), aw, rw[..., None])
                    state["diff"] = max(state["diff"], float(np.abs(tr.forward()["action_pred"][:, -1] - lb).max()))
                    n_cmp += 1
            reset_a(); ses.reset()
            arms = {"a": [], "b": [], "b1": [], "b0": []}
            limit = {"a": m3ae.LATENCY_ROWS_DEFAULT, "b": m3ae.LATENCY_ROWS_DEFAULT, "b1": 1024, "b0": 0}
            for arm in arms:  # warm-up of every shape
                enc.set_latency_rows(limit[arm])
                run("a" if arm == "a" else "b", 0, a.warmup)
            for r in range(a.rounds):
                for arm in arms:
                    enc.set_latency_rows(limit[arm])
                    run("a" if arm == "a" else "b", 0, 3)  # (the arm's captured chains are current again)
                    arms[arm].append(run("a" if arm == "a" else "b", r * a.steps, a.steps))
            enc.set_latency_rows(m3ae.LATENCY_ROWS_DEFAULT)
            res = {"encoder": emode, "E": E, "max_logit_diff_a_vs_b": state["diff"], "logit_comparisons": n_cmp}
            for arm, rounds in arms.items():
                med = [float(np.median(x)) for x in rounds]
                res[arm] = {"median_ms": float(np.median(np.concatenate(rounds))), "round_medians_ms": [round(m, 4) for m in med], "spread_ms": max(med) - min(med)}
            res["b_below_a_by_more_than_a_spread"] = bool(res["a"]["median_ms"] - res["b"]["median_ms"] > res["a"]["spread_ms"])
            results.append(res)
            say(f"encoder {emode} E={E}: (a) host window {res['a']['median_ms']:.3f} ms (spread {res['a']['spread_ms']:.3f}) | (b) session, default limit {res['b']['median_ms']:.3f} ms "
                f"(spread {res['b']['spread_ms']:.3f}) | (b1) session, limit forced to 1024 {res['b1']['median_ms']:.3f} ms (spread {res['b1']['spread_ms']:.3f}) | (b0) session, latency path off {res['b0']['median_ms']:.3f} ms (spread {res['b0']['spread_ms']:.3f}) | "
                f"a/b {res['a']['median_ms'] / res['b']['median_ms']:.2f}x | max logit diff a vs b {state['diff']:.2e} over {n_cmp} decisions of an untimed pass | timing condition {'met' if res['b_below_a_by_more_than_a_spread'] else 'NOT met'}")
            ses.close()
        tr.close(); enc.close()
    lab.close()
    say(json.dumps({"rollout_step_timing": results}))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
