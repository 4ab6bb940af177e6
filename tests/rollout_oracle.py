"""A literal numpy restatement of the rollout loop's input handling: ``prepare_input`` / ``update_input`` / ``trim_fn``
(/root/reference/arp_dt/envs/rollout_procgen.py:46-82) and the return-to-go update (:152-155), for ONE environment.  No GPU, no library.

The policy is a callable ``policy_fn(inputs) -> action`` that sees the reference's ``inputs`` dict: ``image`` [1, L, ...], ``action`` [1, L],
``rtg`` [1, L, 1] with ``L = min(t + 1, window)`` -- unpadded, the current step last, carrying action 0.
"""
import copy

import numpy as np


def _concat(x, y):
    return np.concatenate([x, y], axis=1)


class RolloutOracle:
    def __init__(self, window_size, return_to_go=100.0, scale=100.0, reward_min=0.0, use_normalize=False):
        self.window_size, self.scale, self.reward_min, self.use_normalize = int(window_size), np.float32(scale), np.float32(reward_min), bool(use_normalize)
        self.rtg0 = np.float32(return_to_go) / np.float32(scale)
        self.reset()

    def reset(self, rtg=None):
        self.rtg = np.full(1, self.rtg0 if rtg is None else rtg, dtype=np.float32)  # :90
        self.all_inputs = {}

    def _trim(self, x):
        return x[:, -self.window_size:, ...]

    def _batch(self, d):
        return {k: np.asarray(v)[None, None, ...] for k, v in d.items()}

    def prepare_input(self, image, rtg):  # :57-70
        inputs = self._batch({"image": image, "action": np.zeros(1, dtype=np.int32), "rtg": rtg})
        inputs["action"] = inputs["action"].squeeze(-1)
        if len(self.all_inputs) != 0:
            prev = copy.deepcopy(self.all_inputs)
            inputs = {k: self._trim(_concat(prev[k], inputs[k])) for k in inputs}
        return inputs

    def update_input(self, image, action, rtg):  # :72-82
        inputs = self._batch({"image": image, "action": np.asarray(action, np.int32), "rtg": rtg})
        if len(self.all_inputs) == 0:
            self.all_inputs = inputs
        else:
            self.all_inputs = {k: self._trim(_concat(self.all_inputs[k], inputs[k])) for k in inputs}

    def step(self, image, policy_fn):
        """One pass of :123-126: returns (action, the inputs the policy saw)."""
        inputs = self.prepare_input(image, self.rtg)
        action = int(policy_fn(inputs))
        self.update_input(image, action, self.rtg)
        return action, inputs

    def apply_reward(self, clip_reward):  # :152-155 (a new array: the windows keep the value they were built with)
        r = np.float32(clip_reward)
        if self.use_normalize:
            self.rtg = self.rtg - (r - self.reward_min) / self.scale
        else:
            self.rtg = self.rtg - r / self.scale


def padded(inputs, T, tokens_shape):
    """The reference's unpadded window as the session lays it out: L real steps at the front, zeros behind."""
    L = inputs["action"].shape[1]
    enc = np.zeros((T,) + tuple(tokens_shape), np.float32)
    act = np.zeros(T, np.int32)
    rtg = np.zeros(T, np.float32)
    enc[:L] = inputs["image"][0]
    act[:L] = inputs["action"][0]
    rtg[:L] = inputs["rtg"][0].reshape(L)
    return L, enc, act, rtg
