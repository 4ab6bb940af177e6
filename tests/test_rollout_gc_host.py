"""CPU tests of the goal-carrying rollout session's host side: batch_rollout hands episode ``ep`` its goal frame at that episode's reset and nowhere else
(the reference reads it once per episode, envs/rollout_procgen.py:94), and the binding declares the new entry points with the header's signatures."""
import ctypes as C
import os
import re

import numpy as np

from test_rollout_host import FakeEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class GoalStubSession:
    """records (what reset was given, how many steps had been taken by then)"""

    def __init__(self):
        self.resets, self.steps = [], 0

    def reset(self, env_ids=None, rtg=None, goals=None):
        assert env_ids is None and rtg is None
        self.resets.append((None if goals is None else np.array(goals), self.steps))

    def step(self, frames):
        assert frames.dtype == np.uint8 and frames.shape == (1, 4, 4, 3)
        self.steps += 1
        return np.asarray([self.steps % 15], np.int32)


def _goal(ep):
    return np.full((4, 4, 3), 200 + ep, np.uint8)


def test_batch_rollout_hands_each_episode_its_goal_at_its_reset():
    from arp_amd.rollout import batch_rollout
    rewards = [[1.0, 0.5, 2.0], [0.25, 4.0], [3.0, 1.0, 1.0, 1.0, 1.0]]
    asked = []

    def goal_fn(ep):
        asked.append(ep)
        return _goal(ep)
    for goals in ([_goal(ep) for ep in range(3)], np.stack([_goal(ep) for ep in range(3)]), goal_fn):
        env, ses = FakeEnv(rewards), GoalStubSession()
        m = batch_rollout(env, ses, episode_length=4, num_episodes=3, goals=goals)
        assert len(ses.resets) == 3 and [n for _, n in ses.resets] == [0, 3, 5]  # one reset per episode, before its first step
        for ep, (g, _) in enumerate(ses.resets):
            assert g.dtype == np.uint8 and g.shape == (1, 4, 4, 3) and np.array_equal(g[0], _goal(ep))
        assert ses.steps == 3 + 2 + 4 and np.allclose(m["return"], (3.5 + 4.25 + 6.0) / 3)  # the accounting is the plain loop's
    assert asked == [0, 1, 2]  # the callable is asked once per episode, in order
    # without goals the session's reset is called bare, as ever
    env, ses = FakeEnv(rewards), GoalStubSession()
    batch_rollout(env, ses, episode_length=4, num_episodes=2)
    assert [g for g, _ in ses.resets] == [None, None]


def test_binding_declares_the_new_entry_points_with_the_header_signatures():
    from arp_amd import _ffi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "arp_hip.h")).read(), flags=re.S)
    vp, i, f = C.c_void_p, C.c_int32, C.c_float
    p = C.POINTER
    ctype = {"arp_dt*": vp, "arp_enc*": vp, "arp_clip*": vp, "arp_rollout*": vp, "arp_rollout**": p(vp), "int": i, "float": f, "const int32_t*": p(C.c_int32),
             "const float*": p(f), "const uint8_t*": p(C.c_uint8)}
    want = {
        "arp_rollout_create_gc": ["arp_dt*", "arp_enc*", "arp_clip*", "int", "int", "int", "float", "arp_rollout**"],
        "arp_rollout_reset_goal": ["arp_rollout*", "const int32_t*", "int", "const float*", "const uint8_t*"],
        # (frames and features are DEVICE pointers: the binding passes them as void*)
        "arp_clip_encode_image_dev_async": ["arp_clip*", "const uint8_t*", "int", "int", "int", "int", "int", "float*"],
    }
    for name, types in want.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, name
        declared = [" ".join(a.split()[:-1]) for a in m.group(1).split(",")]  # drop the parameter names
        assert declared == types, (name, declared)
        res, args = _ffi.SIGNATURES[name]
        assert res is i and len(args) == len(types), name
        if name == "arp_clip_encode_image_dev_async":
            assert args == [vp, vp, i, i, i, i, i, vp]
        else:
            assert args == [ctype[t] for t in types], name
