"""CPU tests of arp_amd.rollout: the window plan against the reference's deque, batch_rollout's accounting, and the header / binding agreement of the
session's C ABI."""
import os
import re

import numpy as np
import pytest

from rollout_oracle import RolloutOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("T", [1, 3, 4])
def test_window_plan_agrees_with_the_reference_deque(T):
    from arp_amd.rollout import window_plan
    o = RolloutOracle(T)
    for t in range(3 * T + 1):
        _, inputs = o.step(np.full(2, t, np.float32), lambda inp: (t * 7) % 15)
        L, offs = window_plan(t, T)
        assert L == inputs["action"].shape[1] == min(t + 1, T)
        assert [t - d for d in offs] == [int(v) for v in inputs["image"][0, :, 0]]
        # earlier steps carry the action taken, the current one action 0
        assert [int(a) for a in inputs["action"][0]] == [((t - d) * 7) % 15 for d in offs[:-1]] + [0]
    with pytest.raises(ValueError):
        window_plan(-1, T)


class _Cfg:
    rand_seed = 11


class FakeEnv:
    """Scripted: episode k gives rewards[k][t] and is done after len(rewards[k]) steps."""
    config = _Cfg()

    def __init__(self, rewards):
        self.rewards, self.seeds, self.actions, self.ep, self.t = rewards, [], [], -1, 0

    def _obs(self):
        return {"image": {"ob": np.full((4, 4, 3), (self.ep * 16 + self.t) % 256, np.uint8)}}

    def reset(self, seed):
        self.seeds.append(seed)
        self.ep += 1
        self.t = 0
        return self._obs()

    def step(self, action):
        self.actions.append(int(action))
        r = self.rewards[self.ep][self.t]
        self.t += 1
        done = self.t >= len(self.rewards[self.ep])
        return self._obs(), np.full(1, r, np.float32), np.full(1, int(done), np.int32), {"episode_len": self.t, "vid": None}


class StubSession:
    def __init__(self):
        self.resets, self.frames = 0, []

    def reset(self):
        self.resets += 1

    def step(self, frames):
        assert frames.dtype == np.uint8 and frames.shape == (1, 4, 4, 3)
        self.frames.append(int(frames[0, 0, 0, 0]))
        return np.asarray([len(self.frames) % 15], np.int32)


def test_batch_rollout_reproduces_the_reference_accounting():
    from arp_amd.rollout import batch_rollout
    rewards = [[1.0, 0.5, 2.0], [0.25, 4.0], [3.0, 1.0, 1.0, 1.0, 1.0]]
    env, ses = FakeEnv(rewards), StubSession()
    m = batch_rollout(env, ses, episode_length=4, num_episodes=3, transform_action_fn=lambda a: int(a) + 100)
    # episode 2 is cut by episode_length = 4 before its done: its first four rewards count, its length does not (:170-172 adds it only on done)
    assert env.seeds == [11, 12, 13] and ses.resets == 3
    assert np.allclose(m["return"], (3.5 + 4.25 + 6.0) / 3) and m["return"].dtype == np.float32
    assert np.allclose(m["episode_length"], (3 + 2) / 3)
    assert len(env.actions) == 3 + 2 + 4 and all(a >= 100 for a in env.actions)  # stops on done; the transformed action reaches the env
    assert ses.frames == [0, 1, 2, 16, 17, 32, 33, 34, 35]  # the frame of reset first, then each step's next_obs


def test_batch_rollout_masks_rewards_after_done():
    """reward * (1 - done_prev): with a two-lane `done` the loop runs until both are done and a finished lane stops counting."""
    from arp_amd.rollout import batch_rollout

    class TwoLane(FakeEnv):
        def step(self, action):
            self.t += 1
            return self._obs(), np.asarray([1.0, 1.0], np.float32), np.asarray([self.t >= 2, self.t >= 4], np.int32), {"episode_len": self.t, "vid": None}
    m = batch_rollout(TwoLane([[0.0]]), StubSession(), episode_length=10, num_episodes=1)
    assert np.array_equal(m["return"], np.asarray([2.0, 4.0], np.float32)) and float(m["episode_length"][0]) == 4.0


def test_header_and_binding_agree_on_the_rollout_symbols():
    from arp_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "arp_hip.h")).read()
    declared = set(re.findall(r"\b(arp_(?:rollout_\w+|op_rollout_\w+|enc_set_latency))\s*\(", hdr))
    bound = {n for n in _ffi.SIGNATURES if n.startswith(("arp_rollout_", "arp_op_rollout_")) or n == "arp_enc_set_latency"}
    assert declared == bound and {"arp_rollout_create", "arp_rollout_destroy", "arp_rollout_reset", "arp_rollout_set_lut", "arp_rollout_set_reward_norm",
                                  "arp_rollout_step", "arp_rollout_read", "arp_op_rollout_decide"} <= bound
    for n in bound:  # argument counts
        args = re.search(r"\b" + n + r"\s*\(([^;]*?)\)\s*;", hdr, re.S).group(1)
        args = re.sub(r"/\*.*?\*/", "", args, flags=re.S)
        assert len([a for a in args.split(",") if a.strip()]) == len(_ffi.SIGNATURES[n][1]), n
