"""Wall clock of the fine-tuned CLIP reward (model_type = "clip_ft") at the real geometry -- ViT-B/16 towers plus the 476 M-parameter multi-scale adapter
head, f16, synthetic weights and frames -- the host-driven path against the device-resident one (arp_ft_reward_*), in one process on one machine.

  1. one frame in, one reward out (label transform): get_torch_clip_adapter_reward on a FinetunedClip with resident = False (three host round trips:
     towers -> host, host -> training forward -> host, numpy dot product) against the same call with resident = True.
  1b. the same resident call at one and at three frames with the head's three products on the weight-streaming rows kernel against the existing split-K GEMMs.
  2. RolloutSession.step at 1, 2 and 3 environments: reward_model = <FinetunedClip> (the reward beside the policy, on the device) against a session given
     rewards = get_torch_clip_adapter_reward per environment (the only way available before).
  3. labelling 1 024 frames of 256 x 256 through the fine-tune transform: FinetunedClip.label with resident = False against resident = True, frames / s.

Protocol of scripts/rollout_step_timing.py: every shape is warmed up, then the arms alternate in `--rounds` rounds of `--steps` calls; a host clock wraps the
calls, all of which end in a synchronisation.  Medians over all timed calls, and per arm the spread of the round medians (max - min).  Nothing is gated.

    python scripts/ft_reward_timing.py [--steps 200] [--rounds 5] [--out profiles/ft_reward_timing.txt]
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
    ap.add_argument("--label-frames", type=int, default=1024)
    ap.add_argument("--label-calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ft_reward_timing.txt"))
    a = ap.parse_args()
    import torch  # noqa: F401  -- before arp_amd: one HIP runtime per process (arp_amd/_ffi.py)
    import numpy as np

    from arp_amd import _ffi, clip, finetune as FT, m3ae, synth, synth_policy as S
    from arp_amd.label_reward import get_torch_clip_adapter_reward
    from arp_amd.rollout import RolloutSession
    from arp_amd.train import PolicyConfig, PolicyTrainer
    _ffi.require_gpu()
    ccfg = clip.ClipConfig(patch=16)
    hcfg = FT.FinetuneConfig()
    sd = {**{"clip_model." + k: v for k, v in synth.clip_weights(ccfg, seed=1).items()}, **FT.synth_params(hcfg, seed=2)}
    m = FT.FinetunedClip.from_state_dict(sd, mode="f16", model=ccfg).set_text(synth.prompt_tokens(1, 8, seed=3))
    del sd
    n_pool = 64
    pool = synth.procgen_like_frames(3 * n_pool, seed=7).reshape(n_pool, 3, 256, 256, 3)
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

    def compare(arms, steps, warmup):
        """arms: {name: fn(k)}; alternating rounds; -> {name: {median_ms, round_medians_ms, spread_ms}}"""
        got = {k: [] for k in arms}
        for fn in arms.values():
            timed(fn, 0, warmup)
        for r in range(a.rounds):
            for name, fn in arms.items():
                timed(fn, 0, 3)
                got[name].append(timed(fn, r * steps, steps))
        out = {}
        for name, rounds in got.items():
            med = [float(np.median(x)) for x in rounds]
            out[name] = {"median_ms": float(np.median(np.concatenate(rounds))), "round_medians_ms": [round(v, 4) for v in med], "spread_ms": max(med) - min(med)}
        return out

    say(f"ft_reward_timing: ViT-B/16 towers + {m.head.n_params / 1e6:.0f} M-parameter head, f16; {a.rounds} rounds x {a.steps} calls per arm, warm-up {a.warmup}; "
        "wall clock, every call ends in a synchronisation")

    # 1. one frame in, one reward out
    def one(resident):
        def fn(k):
            m.resident = resident
            return get_torch_clip_adapter_reward(m, pool[k % n_pool, 0])
        return fn
    r_host, r_res = one(False)(5), one(True)(5)
    res = compare({"host": one(False), "resident": one(True)}, a.steps, a.warmup)
    res["reward_host_vs_resident"] = [float(r_host[0]), float(r_res[0])]
    results["one_frame"] = res
    say(f"one frame, label transform: host path {res['host']['median_ms']:.3f} ms (spread {res['host']['spread_ms']:.3f}) | resident {res['resident']['median_ms']:.3f} ms "
        f"(spread {res['resident']['spread_ms']:.3f}) | {res['host']['median_ms'] / res['resident']['median_ms']:.2f}x | the same frame's reward: {r_host[0]:.4f} / {r_res[0]:.4f}")

    # 1b. the stop rule's A/B inside the resident path: the head's three products on the weight-streaming rows kernel (csrc/ftrows.h) against the training
    # GEMMs (split-K 128 x 128 tiles + reduce), at one frame and at three.  The kernel ships if its median at one frame is lower by more than the spread of
    # the round medians and it is not higher at three.
    def rows(on, k_frames):
        def fn(k):
            m.set_rows_kernel(on)
            return m.reward(pool[k % n_pool, :k_frames], transform="label")
        return fn
    results["rows_kernel_ab"] = []
    for nf in (1, 3):
        d = float(np.abs(rows(True, nf)(3) - rows(False, nf)(3)).max())
        res = compare({"split_k_gemms": rows(False, nf), "rows_kernel": rows(True, nf)}, a.steps, a.warmup)
        res.update(frames=nf, max_reward_diff=d)
        results["rows_kernel_ab"].append(res)
        say(f"resident path, {nf} frame(s), head on the existing split-K GEMMs {res['split_k_gemms']['median_ms']:.4f} ms (spread {res['split_k_gemms']['spread_ms']:.4f}) | "
            f"on the rows kernel {res['rows_kernel']['median_ms']:.4f} ms (spread {res['rows_kernel']['spread_ms']:.4f}) | max |reward difference| {d:.3e}")
    m.set_rows_kernel(True)
    st = m.reward_stats()
    say(f"captured chains: {st['captured']} captured, {st['replayed']} replays, {st['launched']} calls launched one by one, {st['rows_products']} products on the rows kernel")

    # 2. the rollout step
    cfg, ecfg = PolicyConfig(lambda_ret=0.01), m3ae.EncoderConfig()
    enc = m3ae.M3AEEncoder(ecfg, S.m3ae_params(ecfg, seed=0), mode="f16")
    tr = PolicyTrainer(cfg, mode="f16")
    tr.set_params(S.policy_params(cfg, seed=0))
    tr.attach_encoder(enc)
    results["rollout_step"] = []
    for E in [int(v) for v in a.envs.split(",")]:
        m.resident = False
        dev, host = RolloutSession(tr, reward_model=m, n_envs=E), RolloutSession(tr, n_envs=E)
        dev.reset(); host.reset()

        def step_dev(k):
            dev.step(np.ascontiguousarray(pool[k % n_pool, :E]))

        def step_host(k):
            fr = np.ascontiguousarray(pool[k % n_pool, :E])
            host.step(fr, rewards=np.concatenate([get_torch_clip_adapter_reward(m, fr[e]) for e in range(E)]))
        res = compare({"rewards_from_host": step_host, "reward_model": step_dev}, a.steps, a.warmup)
        res["E"] = E
        results["rollout_step"].append(res)
        say(f"RolloutSession.step E={E}: rewards= from the host {res['rewards_from_host']['median_ms']:.3f} ms (spread {res['rewards_from_host']['spread_ms']:.3f}) | "
            f"reward_model=<FinetunedClip> {res['reward_model']['median_ms']:.3f} ms (spread {res['reward_model']['spread_ms']:.3f}) | "
            f"{res['rewards_from_host']['median_ms'] / res['reward_model']['median_ms']:.2f}x")
        dev.close(); host.close()
    tr.close(); enc.close()

    # 3. labelling
    n = a.label_frames
    frames = np.ascontiguousarray(np.resize(pool.reshape(-1, 256, 256, 3), (n, 256, 256, 3)))

    def lab(resident):
        def fn(k):
            m.resident = resident
            return m.label(frames)
        return fn
    d = float(np.abs(lab(False)(0) - lab(True)(0)).max())
    res = compare({"host": lab(False), "resident": lab(True)}, a.label_calls, 1)
    for k in ("host", "resident"):
        res[k]["frames_per_s"] = n / (res[k]["median_ms"] * 1e-3)
    res["max_reward_diff"] = d
    results["labelling"] = res
    say(f"labelling {n} frames of 256 x 256, fine-tune transform: host path {res['host']['frames_per_s']:.0f} frames/s ({res['host']['median_ms']:.1f} ms per call, spread "
        f"{res['host']['spread_ms']:.1f}) | resident {res['resident']['frames_per_s']:.0f} frames/s ({res['resident']['median_ms']:.1f} ms, spread {res['resident']['spread_ms']:.1f}) | "
        f"max |reward difference| {d:.3e}")
    m.close()
    say(json.dumps({"ft_reward_timing": results}))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
