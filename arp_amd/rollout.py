"""The rollout loop on MI355X: a session that keeps an episode's state in HBM.

Reference: ``batch_rollout`` (/root/reference/arp_dt/envs/rollout_procgen.py:24-182), driven by ``create_test_step``
(arp_dt/main_procgen.py:171-229).  Per environment step the reference encodes the whole window again, uploads the frame a second
time for the CLIP reward and decrements the return-to-go on the host.  :class:`RolloutSession` (``arp_rollout_*`` in
include/arp_hip.h) takes one uint8 frame per environment and returns one greedy action, with one host synchronisation per
step: the frozen encoder runs on the NEW frames only, the last ``window`` encodings / actions / returns-to-go live in a ring in
HBM, the CLIP reward of the same device frames runs beside the policy on the reward handle's stream, and a kernel takes it off
the return-to-go.

:func:`window_plan` and :func:`batch_rollout` are pure numpy (no GPU, no library call of their own).
"""
import ctypes as C

import numpy as np


def window_plan(steps_since_reset, T):
    """What a step whose environment has taken ``steps_since_reset`` steps since its reset (this one not counted) feeds the policy:
    ``(L, offsets)`` with ``L = min(steps_since_reset + 1, T)`` real time steps and, in time order, how many steps back from the
    current one each lies (``offsets[j] = L - 1 - j``; the ring slot is ``(head - offsets[j]) mod T``).  Positions ``L .. T - 1`` of
    the policy's batch are padding.  ``prepare_input`` / ``trim_fn``, rollout_procgen.py:46-70."""
    if steps_since_reset < 0 or T < 1:
        raise ValueError("window_plan: steps_since_reset >= 0 and T >= 1")
    L = min(int(steps_since_reset) + 1, int(T))
    return L, [L - 1 - j for j in range(L)]


class RolloutSession:
    """``n_envs`` independent environments behind one ARP-DT policy with its frozen encoder attached (``trainer.attach_encoder``).

    ``reward_model``: an :class:`arp_amd.clip.ClipLabeller` with its prompts set (its ``prompt_reduce`` and the step's ``use_crop``
    apply), or an :class:`arp_amd.finetune.FinetunedClip` with its prompts set (the fine-tuned reward through the label transform,
    ``get_torch_clip_adapter_reward``; its ``set_prompt_reduce`` and the step's ``use_crop`` apply) -- the reward of every frame is then
    computed on the device and never read by the host; ``None``: pass ``rewards=`` to :meth:`step` (computed by the caller with any of
    ``VL_REWARD_FNS``: the goal-conditioned variants), or nothing, and the return-to-go stays constant.  ``return_to_go / scale`` is every episode's first return-to-go (rollout_procgen.py:90).
    ``encoder``: the encoder to use instead of the trainer's attached one.  Model BC (``PolicyConfig(model="BC")``) runs this way -- it refuses
    ``attach_encoder`` and keeps refusing it, the session borrows the encoder for its own passes: two tokens per step, no return-to-go ring, and a reward
    model, ``use_normalize`` / ``reward_min`` and ``rewards=`` are refused by the library.
    ``goal_conditioned=True`` (``arp_rollout_create_gc``): the session keeps one goal frame per environment in HBM, handed over with ``reset(goals=...)``
    (the reference fixes it per episode, rollout_procgen.py:94).  With a GCBC trainer a step encodes the new (frame, goal) pairs; with an ARP-DT trainer and a
    plain :class:`arp_amd.clip.ClipLabeller` (no prompts needed) the reward is ``clip_goal_conditioned``, ``-||f(frame) - f(goal)||`` on the device, the goal's
    feature computed once per reset; ``use_crop`` is then refused.  Without the flag a GCBC trainer is refused, as ever.
    ``instruct=(tokens, text_padding_mask)`` (``arp_rollout_create_text``): model BC as the reference rolls it out -- InstructRL, with the game's instruction
    (int ids ``[L]`` or ``[1, L]``, mask > 0 = padded, or None).  A step encodes the new frames with the encoder's image + text pass; the encoder is
    ``encoder``, or the one the trainer carries from ``attach_encoder(enc, instruct=...)``, and must hold the text weights.
    """

    def __init__(self, trainer, reward_model=None, n_envs=1, return_to_go=100.0, scale=100.0, reward_min=0.0, use_normalize=False, lut=None, encoder=None,
                 goal_conditioned=False, instruct=None):
        from . import _ffi, dataset
        from .finetune import FinetunedClip
        self._ffi = _ffi
        finetuned = isinstance(reward_model, FinetunedClip)
        if reward_model is not None and not finetuned and not hasattr(reward_model, "_h"):
            raise ValueError(f"reward_model: a ClipLabeller, a FinetunedClip or None, not {type(reward_model).__name__}")
        enc = encoder if encoder is not None else getattr(trainer, "_encoder", None)
        if getattr(trainer.cfg, "use_symlog", False):
            raise _ffi.ArpError("use_symlog: the session embeds rtg / scale, not its symlog")
        res = enc.cfg.img_res if enc is not None else 0
        h = C.c_void_p()
        rm = reward_model._h if reward_model is not None and not finetuned else None
        self.goal_conditioned = bool(goal_conditioned)
        if instruct is not None:
            from .train import _one_instruction
            if goal_conditioned or reward_model is not None:
                raise _ffi.ArpError("rollout: instruct= is model BC's session: no goal frames, no reward model (BC reads no return-to-go)")
            tok, mask = _one_instruction(*instruct) if isinstance(instruct, (tuple, list)) else _one_instruction(instruct)
            _ffi.check(_ffi.lib.arp_rollout_create_text(trainer._h, encoder._h if encoder is not None else None, int(n_envs), res, res,
                                                        _ffi.as_ptr(tok, C.c_int32), _ffi.as_ptr(mask, C.c_float), len(tok), C.byref(h)))
        elif goal_conditioned:
            if finetuned:
                raise _ffi.ArpError("rollout: create_gc takes a plain labelling handle: the fine-tuned goal reward stays with the host function")
            _ffi.check(_ffi.lib.arp_rollout_create_gc(trainer._h, encoder._h if encoder is not None else None, rm, int(n_envs), res, res, float(scale), C.byref(h)))
        elif finetuned:  # the fine-tuned reward: its towers and its head (both kept alive through reward_model below)
            if reward_model._resident_text_error:
                raise _ffi.ArpError(reward_model._resident_text_error)
            _ffi.check(_ffi.lib.arp_rollout_create_ft(trainer._h, encoder._h if encoder is not None else None, reward_model.towers._h,
                                                      reward_model.head._h, int(n_envs), res, res, float(scale), C.byref(h)))
        elif encoder is not None:
            _ffi.check(_ffi.lib.arp_rollout_create_with_encoder(trainer._h, encoder._h, rm, int(n_envs), res, res, float(scale), C.byref(h)))
        else:
            _ffi.check(_ffi.lib.arp_rollout_create(trainer._h, rm, int(n_envs), res, res, float(scale), C.byref(h)))
        self._h = h
        self.trainer, self.reward_model, self.encoder = trainer, reward_model, enc  # (kept alive: the session holds their handles)
        self.n_envs, self.res, self.window, self.n_actions = int(n_envs), res, trainer.cfg.window, trainer.cfg.n_actions
        self.tokens, self.dim = trainer.cfg.enc_tokens, trainer.cfg.enc_dim
        self.return_to_go, self.scale = float(return_to_go), float(scale)
        self.set_lut(dataset.default_lut() if lut is None else lut)
        try:
            if use_normalize or reward_min:
                self.set_reward_norm(use_normalize, reward_min)
        except Exception:
            self.close()
            raise

    def set_lut(self, lut):
        t = np.require(np.asarray(lut, np.float32).reshape(3, 256), requirements="C")
        self._ffi.check(self._ffi.lib.arp_rollout_set_lut(self._h, self._ffi.as_ptr(t, C.c_float)))

    def set_reward_norm(self, use_normalize, reward_min):
        self._ffi.check(self._ffi.lib.arp_rollout_set_reward_norm(self._h, int(bool(use_normalize)), float(reward_min)))

    def reset(self, env_ids=None, rtg=None, goals=None):
        """Start an episode in ``env_ids`` (default: all).  ``rtg``: the first return-to-go, already divided by ``scale`` (scalar or one per listed
        environment; default ``return_to_go / scale``).  ``goals`` (a ``goal_conditioned`` session): the listed environments' goal frames, uint8
        ``[n, H, W, 3]`` (``[H, W, 3]`` for one); without it an environment keeps the goal it has."""
        ids = np.arange(self.n_envs, dtype=np.int32) if env_ids is None else np.require(np.asarray(env_ids, np.int32).reshape(-1), requirements="C")
        r = np.full(len(ids), self.return_to_go / self.scale if rtg is None else 0.0, np.float32)
        if rtg is not None:
            r[:] = np.asarray(rtg, np.float32).reshape(-1)
        if goals is not None:
            g = np.asarray(goals)
            if g.dtype != np.uint8:
                raise ValueError("goals must be uint8")
            g = np.require(g.reshape(-1, *g.shape[-3:]), requirements="C")
            if g.shape != (len(ids), self.res, self.res, 3):
                raise ValueError(f"goals {g.shape}, expected {(len(ids), self.res, self.res, 3)}")
            self._ffi.check(self._ffi.lib.arp_rollout_reset_goal(self._h, self._ffi.as_ptr(ids, C.c_int32), len(ids), self._ffi.as_ptr(r, C.c_float),
                                                                 self._ffi.as_ptr(g, C.c_uint8)))
            return
        self._ffi.check(self._ffi.lib.arp_rollout_reset(self._h, self._ffi.as_ptr(ids, C.c_int32), len(ids), self._ffi.as_ptr(r, C.c_float)))

    def step(self, frames_u8, rewards=None, use_crop=False):
        """uint8 frames ``[E, H, W, 3]`` (or ``[H, W, 3]`` with one environment) -> greedy actions int32 ``[E]``."""
        f = np.asarray(frames_u8)
        if f.dtype != np.uint8:
            raise ValueError("frames must be uint8")
        f = np.require(f.reshape(-1, *f.shape[-3:]), requirements="C")
        if f.shape != (self.n_envs, self.res, self.res, 3):
            raise ValueError(f"frames {f.shape}, expected {(self.n_envs, self.res, self.res, 3)}")
        rp = None
        if rewards is not None:
            rewards = np.require(np.asarray(rewards, np.float32).reshape(-1), requirements="C")
            if rewards.size != self.n_envs:
                raise ValueError("rewards: one per environment")
            rp = self._ffi.as_ptr(rewards, C.c_float)
        out = np.empty(self.n_envs, np.int32)
        self._ffi.check(self._ffi.lib.arp_rollout_step(self._h, self._ffi.as_ptr(f, C.c_uint8), rp, int(bool(use_crop)), self._ffi.as_ptr(out, C.c_int32)))
        return out

    def read(self, what):
        """Test / logging accessor (synchronises): see ``arp_rollout_read``."""
        E, T = self.n_envs, self.window
        shape, dt = {"enc_window": ((E, T, self.tokens, self.dim), np.float32), "action_window": ((E, T), np.int32), "rtg_window": ((E, T), np.float32),
                     "len": ((E,), np.int32), "rtg": ((E,), np.float32), "reward": ((E,), np.float32), "logits": ((E, T, self.n_actions), np.float32),
                     "enc_ring": ((T, E, self.tokens, self.dim), np.float32), "head": ((1,), np.int32), "goal": ((E, self.res, self.res, 3), np.uint8),
                     "goal_feat": ((E, getattr(getattr(self.reward_model, "cfg", None), "embed", 0)), np.float32)}[what]
        out = np.empty(shape, dt)
        self._ffi.check(self._ffi.lib.arp_rollout_read(self._h, what.encode(), out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def _debug_set_tail(self, value, action=0):
        self._ffi.check(self._ffi.lib.arp_rollout_debug_set_tail(self._h, float(value), int(action)))

    def close(self):
        if getattr(self, "_h", None):
            self._ffi.lib.arp_rollout_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def batch_rollout(env, session, episode_length, num_episodes, transform_action_fn=None, log_interval=None, goals=None):
    """The reference loop (rollout_procgen.py:84-182) around a one-environment session; returns its ``metric`` dict
    (``return``, ``episode_length``; :178-181).  numpy only.

    ``env``: any object with the reference wrapper's ``reset(seed)`` and ``step(action) -> (obs, reward, done, info)``, ``obs["image"][key]``
    uint8 ``[H, W, 3]`` (the first image key is the one the session sees), ``info["episode_len"]`` on the last step, and ``config.rand_seed``
    (0 when absent).  ``session``: ``reset()`` and ``step(frame) -> [action]``.  Episode ``ep`` starts with ``env.reset(rand_seed + ep)``; the
    environment reward is counted as ``reward * (1 - done_prev)``; an episode stops at the first ``done``.

    One difference from the reference: it hands ``update_input`` the TRANSFORMED action (:125-126), so that is what later windows carry; the session's
    action ring keeps the greedy action itself and only ``env.step`` sees ``transform_action_fn(action)``.  The two agree for the identity transform the
    reference runs with, and for no other.

    ``goals`` (a goal-conditioned session): a sequence indexed by episode or a callable ``goals(ep)`` giving episode ``ep``'s goal frame, uint8 ``[H, W, 3]``;
    it is handed to ``session.reset(goals=...)`` at that episode's reset and nowhere else, where the reference reads
    ``eval_hdf5["ob"][eval_traj_idx[ep + 1] - 1, -1]`` (:94) and re-attaches it to every observation (:108,130).

    Out of scope (no Procgen in this project): ``eval_data_path`` replay with saved states, videos, state recording, several
    image keys.  The vision-language reward and the return-to-go are the session's business (:class:`RolloutSession`).
    """
    import logging
    seed0 = int(getattr(getattr(env, "config", None), "rand_seed", 0))
    reward, ep_lens = np.zeros(1, np.float32), np.zeros(1, np.float32)
    info = {}
    for ep in range(num_episodes):
        if goals is None:
            session.reset()
        else:
            session.reset(goals=np.asarray(goals(ep) if callable(goals) else goals[ep], np.uint8)[None])
        done = np.zeros(1, np.int32)
        next_obs = None
        for t in range(episode_length):
            done_prev = done
            obs = env.reset(seed0 + ep) if t == 0 else next_obs
            frame = next(iter(obs["image"].values()))
            action = np.asarray(session.step(np.asarray(frame, np.uint8)[None]))[0]
            if transform_action_fn is not None:
                action = transform_action_fn(action)
            next_obs, _reward, done, info = env.step(action)
            reward = reward + np.asarray(_reward, np.float32) * (1 - done_prev)
            done = np.logical_or(np.asarray(done), done_prev).astype(np.int32)
            if log_interval and t % log_interval == 0:
                logging.info("step: %d done: %s reward: %s", t, done, reward)
            if np.all(done):
                ep_lens = ep_lens + np.float32(info["episode_len"])
                break
    return {"return": reward.astype(np.float32) / num_episodes, "episode_length": ep_lens.astype(np.float32) / num_episodes}
