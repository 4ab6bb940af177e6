"""Argument handling of the device-resident fine-tuned reward that needs no device (arp_amd/finetune.py::FinetunedClip, arp_amd/rollout.py::RolloutSession)."""
import types

import numpy as np
import pytest


def test_finetuned_clip_refuses_unknown_strings_and_bad_frames():
    from arp_amd.finetune import FinetunedClip
    m = FinetunedClip(None, None)
    assert m.resident is False and FinetunedClip(None, None, resident=True).resident is True
    fr = np.zeros((2, 8, 8, 3), np.uint8)
    with pytest.raises(ValueError, match="transform"):
        m.reward(fr, transform="bicubic")
    with pytest.raises(ValueError, match="transform"):
        m.reward_device_async(None, 2, 8, 8, None, transform="pil")
    with pytest.raises(ValueError, match="set_prompt_reduce"):
        m.set_prompt_reduce("median")
    with pytest.raises(ValueError, match="uint8"):
        m.reward(fr.astype(np.float32))
    with pytest.raises(ValueError, match="uint8"):
        m.reward(np.zeros((2, 8, 8), np.uint8)[None, None])
    assert sorted(FinetunedClip.TRANSFORMS) == ["finetune", "label"] and sorted(FinetunedClip.REDUCES) == ["first", "mean"]


def test_rollout_session_refuses_an_unknown_reward_model():
    from arp_amd.rollout import RolloutSession
    with pytest.raises(ValueError, match="reward_model"):
        RolloutSession(types.SimpleNamespace(cfg=types.SimpleNamespace()), reward_model="clip_ft")


def test_the_new_entry_points_are_bound():
    from arp_amd import _ffi
    for name in ("arp_ft_reward_set_text", "arp_ft_reward_set_reduce", "arp_ft_reward_dev_async", "arp_ft_reward", "arp_rollout_create_ft", "arp_op_ft_reward"):
        assert name in _ffi.SIGNATURES and hasattr(_ffi.lib, name)
