"""Path (2): the ARP-DT policy train step on MI355X, behind the reference's call surface.

Mirrors /root/reference/arp_dt/main_procgen.py:
  * ``create_train_step(model, learning_rate, weight_decay) -> train_step_fn`` (:104-141)
  * ``train_step_fn(state, batch, rng) -> (new_state, aux, next_rng)`` with the reference's ``aux`` keys
    (``loss, acc, trans_loss, return_loss, weight_penalty, weight_l2, train_state_step, learning_rate``)
  * ``create_val_step(model) -> val_step_fn(state, batch, rng) -> (aux, next_rng)`` (:144-169)
  * ``prefetch_to_device(iterator, 2, ...)`` (:703): batch i+1 uploads while step i runs
  * ``sync_state_fn`` (:94-101) = :meth:`PolicyTrainer.broadcast_state`
and ARPDT.__call__ (arp_dt/ARPDT.py:152-236) = :meth:`PolicyTrainer.forward`.

``model`` is the policy configuration (the reference passes an ``ARPDT`` flax module built from
``FLAGS.model``; jax/flax do not exist here, so a :class:`PolicyConfig` or a dict of the same fields
stands in).  ``state`` is a :class:`TrainState` wrapping the device-resident parameters, Adam moments and
step counter; like the reference's donated state it is consumed by the call and the returned one must be
used.  ``batch`` keeps the reference's keys: ``batch["image"]`` holds, per image key, the frozen encoder
output ``[B, T, tokens, dim]`` (the boundary of this round: BASELINE.json configs[3] feeds pre-computed
encodings), ``batch["action"]`` int ``[B, T]``, ``batch["rtg"]`` per key ``[B, T, 1]`` (none for ``PolicyConfig(model="BC")``);
``PolicyConfig(model="GCBC")`` with the frozen encoder attached reads ``batch["image"]`` and ``batch["goal"]`` frames and no rtg
(or, with a device-resident dataset attached, ``{"index", "goal_index"}``: rows and goal rows, gathered on the GPU).
All compute is in libarp_hip.so; there is no CPU fallback.
"""
import ctypes as C
import json
import os
from dataclasses import asdict, dataclass

import numpy as np

from . import _ffi
from ._ffi import MODE_BF16, MODE_F16, MODE_F32, check, lib

AUX_KEYS = ("loss", "acc", "trans_loss", "return_loss", "weight_penalty", "weight_l2", "train_state_step", "learning_rate")


@dataclass(frozen=True)
class PolicyConfig:
    """ARPDT.get_default_config fields that shape the shipped policy (arp_dt/ARPDT.py:27-66)."""
    emb: int = 128
    depth: int = 2
    heads: int = 8
    mlp_ratio: int = 4
    n_actions: int = 15
    window: int = 4
    enc_tokens: int = 257
    enc_dim: int = 768
    use_adapter: bool = True
    lambda_ret: float = 1.0
    use_symlog: bool = False  # config.use_symlog (ARPDT.py:55): symlog of every return-to-go view before their mean
    alibi_bias: bool = False  # config.alibi_bias (ARPDT.py:88, layers.py:74-78): slope_h * key index on the attention scores; off as shipped
    weight_decay: float = 5e-5
    clip_norm: float = 10.0
    b1: float = 0.9
    b2: float = 0.999
    eps: float = 1e-8
    # main_procgen.py:406-427: "ARPDT" (use_vl=True), or "BC" -- the InstructRL baseline (use_vl=False, vl_type="BC": arp_dt/BC.py), the same transformer
    # on two tokens per time step [image, action], no return-to-go input, no return head, the cross-entropy alone; or "GCBC" -- the goal-conditioned
    # baseline (main_procgen.py:413-414, arp_dt/GCBC.py): BC's policy behind the frozen encoder's goal-conditioned call on (frame, goal) pairs
    # (enc_tokens = EncoderConfig.gc_tokens).  Unlike BC it accepts attach_encoder, and then takes batch["image"] + batch["goal"] frames.
    model: str = "ARPDT"

    def __post_init__(self):
        if self.model not in _ffi.DT_MODELS:
            raise ValueError(f"PolicyConfig.model must be one of {sorted(_ffi.DT_MODELS)}, not {self.model!r}")
        if self.model == "GCBC":
            # forward_gc_representations emits class token + the frame's P patches + the goal's P patches, P a square patch grid (513 at 256 x 256, patch 16).
            # The default enc_tokens (257: ARP-DT's P + 1) is not such a count: a GCBC configuration has to name its own (EncoderConfig.gc_tokens).
            p2 = self.enc_tokens - 1
            g = int(round((p2 // 2) ** 0.5)) if p2 > 0 else 0
            if p2 <= 0 or p2 % 2 or g * g != p2 // 2:
                raise ValueError(f"PolicyConfig(model='GCBC'): enc_tokens must be 2 P + 1 with P a square patch grid (EncoderConfig.gc_tokens, 513 at 256 x 256), "
                                 f"not {self.enc_tokens}")


def _dt_cfg(cfg, mode, device):
    """The C configuration (arp_dt_cfg) of a policy configuration."""
    return _ffi.DtCfg(cfg.emb, cfg.depth, cfg.heads, cfg.mlp_ratio, cfg.n_actions, cfg.window, cfg.enc_tokens, cfg.enc_dim, int(cfg.use_adapter), mode,
                      device, 1, 0, cfg.lambda_ret, cfg.weight_decay, cfg.clip_norm, cfg.b1, cfg.b2, cfg.eps, int(getattr(cfg, "alibi_bias", False)),
                      _ffi.DT_MODELS[getattr(cfg, "model", "ARPDT")])


class PolicyTrainer:
    """Owns one GPU's copy of the policy: parameters, Adam state, activations, RCCL communicator."""

    def __init__(self, cfg, mode="f16", device=0, adapter_corrections=None):
        """mode: GEMM operand type of the adapter path -- "f16" (default: the 16-bit mode that meets north_star's 1e-3 on the
        logits), "bf16" (8 significand bits: ~1e-2) or "f32" (f32-input MFMA, the parity mode).
        adapter_corrections (f16 only): the adapter's forward products with their operand roundings corrected on the fp4 MFMA
        (arp_dt_set_adapter_corrections) -- what the encoder-inside step (row N1, encoder mode "f16c") pairs with."""
        _ffi.require_gpu()
        self.cfg = cfg
        c = _dt_cfg(cfg, {"bf16": MODE_BF16, "f16": MODE_F16, "f32": MODE_F32}[mode], device)
        self.bc = getattr(cfg, "model", "ARPDT") in ("BC", "GCBC")  # GCBC is BC everywhere inside the step
        self.gcbc = getattr(cfg, "model", "ARPDT") == "GCBC"
        h = C.c_void_p()
        check(lib.arp_dt_create(C.byref(c), C.byref(h)))
        self._h = h
        self._B = 0                    # windows in the batch the next forward / step reads
        self._inflight = {}            # slot -> (arrays of an upload, kept alive until the slot is refilled, ..., B)
        self._encoder = None           # attach_encoder
        self._dataset, self._ds_use_enc = None, False  # attach_dataset
        self._prefetch_owner = None    # prefetch_to_device: the live prefetcher that owns slots 0 / 1
        # None: the library's default -- ON in f16 mode where the corrected products exist (enc_dim a multiple of 256, >= 512), since round 6
        if adapter_corrections is not None:
            check(lib.arp_dt_set_adapter_corrections(h, int(bool(adapter_corrections))))
        self.world, self.rank = 1, 0
        self.shapes = {}
        n = C.c_int32()
        tot = C.c_int64()
        check(lib.arp_dt_num_params(h, C.byref(tot), C.byref(n)))
        self.num_params = tot.value
        buf = C.create_string_buffer(256)
        shape = (C.c_int64 * 4)()
        nd = C.c_int32()
        for i in range(n.value):
            check(lib.arp_dt_param_info(h, i, buf, 256, shape, C.byref(nd)))
            self.shapes[buf.value.decode()] = tuple(shape[d] for d in range(nd.value))

    def close(self):
        if getattr(self, "_h", None):
            lib.arp_dt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- tensors (Flax tree path -> array, Flax layout) ---------------------------------------------
    def set_tensors(self, tree, which=0):
        for name, val in tree.items():
            a = np.require(np.asarray(val, dtype=np.float32), requirements="C")
            if tuple(a.shape) != self.shapes[name]:
                raise ValueError(f"{name}: shape {a.shape}, expected {self.shapes[name]}")
            check(lib.arp_dt_set_tensor(self._h, name.encode(), which, _ffi.as_ptr(a, C.c_float)))

    def get_tensors(self, which=0, names=None):
        out = {}
        for name in (names or self.shapes):
            a = np.empty(self.shapes[name], np.float32)
            check(lib.arp_dt_get_tensor(self._h, name.encode(), which, _ffi.as_ptr(a, C.c_float)))
            out[name] = a
        return out

    set_params = set_tensors

    def get_params(self):
        return self.get_tensors(0)

    def get_grads(self):
        return self.get_tensors(1)

    @property
    def step(self):
        s = C.c_int64()
        check(lib.arp_dt_get_step(self._h, C.byref(s)))
        return s.value

    @step.setter
    def step(self, v):
        check(lib.arp_dt_set_step(self._h, int(v)))

    # -- compute --------------------------------------------------------------------------------------
    def _rtg(self, rtg, B, T):
        """(array, pointer) of the return-to-go: None / NULL for model BC, which reads none (BC.encode); for ARP-DT a missing rtg reaches the
        library as NULL and is refused there."""
        if self.bc or rtg is None:
            return None, None
        rtg = np.require(np.asarray(rtg, dtype=np.float32), requirements="C")
        if rtg.size != B * T:
            raise ValueError(f"batch shapes: rtg {rtg.shape}, expected {B * T} values")
        return rtg, _ffi.as_ptr(rtg, C.c_float)

    # -- batches: the synchronous slot, and two prefetch slots -- the reference's prefetch_to_device(..., 2) (main_procgen.py:703) ---------
    def _stage_host(self, slot, enc, action, rtg, images=False):
        """Host arrays -- encodings, or with ``images`` frames -- into the synchronous slot (``slot`` None) or into prefetch slot 0 / 1."""
        enc = np.require(np.asarray(enc, dtype=np.float32), requirements="C")
        action = np.require(np.asarray(action, dtype=np.int32), requirements="C")
        B, T = action.shape
        if T != self.cfg.window or (not images and enc.shape != (B, T, self.cfg.enc_tokens, self.cfg.enc_dim)):
            raise ValueError(f"batch shapes: enc {enc.shape}, action {action.shape}")
        rtg, rp = self._rtg(rtg, B, T)
        args = (_ffi.as_ptr(enc, C.c_float), _ffi.as_ptr(action, C.c_int32), rp, B)
        if slot is None:
            check(lib.arp_dt_set_batch(self._h, *args))
            self._B = B
        else:
            fn = lib.arp_dt_upload_batch_images_async if images else lib.arp_dt_upload_batch_async
            check(fn(self._h, slot, *args))
            self._inflight[slot] = (enc, action, rtg, B)

    def set_batch(self, enc, action, rtg=None):
        self._stage_host(None, enc, action, rtg)

    def upload_async(self, slot, enc, action, rtg=None, images=False, goals=None):
        """Enqueue the host -> device copy of a batch into slot 0 / 1 on the handle's copy stream.  Safe to call from another
        thread while :meth:`train_step` runs on the other slot.  The arrays must stay alive until :meth:`select` (kept here).
        ``goals``: refused -- goal batches (model GCBC) exist in the synchronous slot only (:meth:`set_batch_images`)."""
        if goals is not None:
            raise _ffi.ArpError("goal batches exist in the synchronous slot only: set_batch_images(images, action, goals=goals) (no prefetch slot, no encode_ahead)")
        self._stage_host(int(slot), enc, action, rtg, images)

    def encode_ahead(self, slot):
        """Enqueue the frozen encoder's pass for the frames in batch slot ``slot`` now, on the encoder's own stream, so that it runs beside the current step's
        policy part (``arp_dt_encode_ahead``); the step that reads the slot then waits for it instead of encoding at its head."""
        check(lib.arp_dt_encode_ahead(self._h, int(slot)))

    def select(self, slot):
        """The next forward / val_step / train_step reads batch slot ``slot`` (ordered behind its upload on the GPU)."""
        check(lib.arp_dt_select_batch(self._h, int(slot)))
        self._B = self._inflight[int(slot)][3]

    def val_step(self):
        """val_step_fn's aux (main_procgen.py:144-169): forward only, rank mean of loss / trans_loss / return_loss / acc*100."""
        m = np.empty(4, np.float32)
        check(lib.arp_dt_val_step(self._h, _ffi.as_ptr(m, C.c_float)))
        return {"loss": float(m[0]), "trans_loss": float(m[1]), "return_loss": float(m[2]), "acc": float(m[3])}

    def attach_encoder(self, encoder, instruct=None, text_padding_mask=None):
        """Put the frozen M3AE encoder (arp_amd.m3ae.M3AEEncoder) inside the step: the boundary then is the
        reference's own -- batch["image"] holds frames, not encodings (ARPDT.py:413-462).  Model BC (InstructRL) needs ``instruct``: its encoder call reads
        the instruction's text tokens beside the frame (BC.py:286-321), so without one the image-only encoder is refused.  ``instruct``: int token ids
        ``[L]``, ``[1, L]`` or ``[B, L]`` with all rows equal, ``text_padding_mask`` likewise (> 0 = padded; default: nothing padded) -- ONE instruction, the
        game's, stored on the handle (``arp_dt_attach_text_encoder``); ``cfg.enc_tokens`` must be the encoder's ``text_tokens(L)`` and the encoder must carry
        the text weights.  Every frames batch of the handle is then encoded with the text pass.  Accepted without ``instruct`` for model GCBC, whose
        encoder call reads frames and goal frames alone (GCBC.py:462-468): ``cfg.enc_tokens`` must be the encoder's ``gc_tokens``."""
        if instruct is None:
            if text_padding_mask is not None:
                raise ValueError("text_padding_mask without instruct")
            check(lib.arp_dt_attach_encoder(self._h, encoder._h))
            self._encoder = encoder
            return
        tok, mask = _one_instruction(instruct, text_padding_mask)
        check(lib.arp_dt_attach_text_encoder(self._h, encoder._h, _ffi.as_ptr(tok, C.c_int32), _ffi.as_ptr(mask, C.c_float), len(tok)))
        self._encoder, self._instruct = encoder, (tok, mask)

    def check_instruction(self, batch):
        """A BC batch dict may carry the reference's keys ``"instruct"`` and ``"text_padding_mask"`` (main_procgen.py:547-553): with an instruction attached
        they must repeat it on every row -- the encoder pass uses the attached one."""
        _check_instruction(getattr(self, "_instruct", None), batch)

    # -- batches named by row indices of a device-resident dataset (arp_amd.dataset.DeviceDataset) -----------------------------------
    def attach_dataset(self, ds, use_encodings=False):
        """After this call ``_stage``, ``prefetch_to_device``, ``create_train_step`` / ``create_val_step``'s step functions, ``greedy_action`` and
        ``greedy_return`` accept a batch dict whose only key is ``"index"`` (int64 row indices): HIP gather kernels build the window batch in the batch slot
        from the set in HBM.  ``use_encodings=False``: frames, through the attached encoder inside the step; ``True``: the set's cached encodings -- the
        encodings-in step (the only way model BC trains from a file: it takes encodings).  Model GCBC attaches frames only, and its batch dict has the
        keys ``"index"`` and ``"goal_index"`` (:func:`is_index_pair_batch`): frames and goal frames are gathered by one launch, and ``prefetch_to_device``
        runs the goal-conditioned encoder pass of the next batch beside the current step."""
        if getattr(ds, "window_size", None) is not None and ds.window_size != self.cfg.window:
            raise _ffi.ArpError(f"the dataset's window is {ds.window_size}, the handle's is {self.cfg.window}")
        if self.cfg.use_symlog:
            raise _ffi.ArpError("use_symlog: the set holds rtg / scale, not its symlog (load the set with symlog'd returns through set_labels instead)")
        if self.gcbc and use_encodings:
            raise _ffi.ArpError("model GCBC: attach_dataset(use_encodings=True) has nothing to gather -- the encoder reads (frame, goal) pairs and the goal is "
                                "drawn per sample, so a pair's encoding is not a per-row quantity and there is nothing to cache; attach the frames "
                                '(use_encodings=False) and feed {"index", "goal_index"} batches')
        if not use_encodings and self._encoder is None:
            raise _ffi.ArpError("attach_dataset(use_encodings=False) gathers frames: attach the frozen encoder first (attach_encoder)")
        self._dataset, self._ds_use_enc = ds, bool(use_encodings)
        ds._trainers.add(self)

    def _stage_indices(self, slot, index, goal_index=None):
        """Rows (and, model GCBC, goal rows) of the attached dataset into the synchronous slot (``slot`` None) or into prefetch slot 0 / 1, gathered on the
        GPU.  Returns whether the slot now holds frames."""
        ds = self._dataset
        if ds is None:
            raise _ffi.ArpError('a batch of row indices ({"index": ...}) needs attach_dataset first')
        idx = np.require(np.asarray(index, dtype=np.int64).reshape(-1), requirements="C")
        pairs, B = goal_index is not None, len(idx)
        if pairs:
            gidx = np.require(np.asarray(goal_index, dtype=np.int64).reshape(-1), requirements="C")
            if len(gidx) != B:
                raise _ffi.ArpError(f"a pair batch names one goal row per row: {B} indices, {len(gidx)} goal indices")
            args = (ds._h, _ffi.as_ptr(idx, C.c_int64), _ffi.as_ptr(gidx, C.c_int64), B)
        else:
            args = (ds._h, _ffi.as_ptr(idx, C.c_int64), B, int(self._ds_use_enc))
        if slot is None:
            check((lib.arp_dt_set_batch_index_pairs if pairs else lib.arp_dt_set_batch_indices)(self._h, *args))
            self._B = B
        else:
            check((lib.arp_dt_upload_batch_index_pairs_async if pairs else lib.arp_dt_upload_batch_indices_async)(self._h, slot, *args))
            self._inflight[slot] = (None, None, None, B)
        return pairs or not self._ds_use_enc

    def set_batch_indices(self, index):
        self._stage_indices(None, index)

    def upload_indices_async(self, slot, index):
        """:meth:`upload_async` for a batch of row indices: the gathers run on the handle's copy stream.  Returns whether the slot now holds frames."""
        return self._stage_indices(int(slot), index)

    # -- model GCBC: (row, goal row) pairs of the attached dataset ---------------------------------------------------------------------
    def set_batch_index_pairs(self, index, goal_index):
        """Frames of the windows of ``index`` and goal frames of the windows of ``goal_index``, gathered on the GPU into the synchronous slot
        (``arp_dt_set_batch_index_pairs``); the step then encodes the pairs at its head, as after ``set_batch_images(..., goals=)``."""
        self._stage_indices(None, index, goal_index)

    def upload_index_pairs_async(self, slot, index, goal_index):
        """:meth:`upload_indices_async` for a pair batch: one gather launch on the handle's copy stream fills the slot's frames and goal frames.  Returns
        True (the slot holds frames: :meth:`encode_ahead` may follow)."""
        return self._stage_indices(int(slot), index, goal_index)

    def set_batch_images(self, images, action, rtg=None, goals=None):
        """Frames ``[B, T, H, W, 3]`` in front of the attached encoder.  ``goals`` (model GCBC): the hindsight goal frames, same shape; the step then encodes
        (frame, goal) pairs (``arp_dt_set_batch_images_goal``) and reads no return-to-go."""
        if goals is None and self.gcbc:
            raise _ffi.ArpError("model GCBC encodes (frame, goal) pairs: set_batch_images needs goals=")
        if goals is None and rtg is None and not self.bc:
            raise ValueError("rtg is None (only model BC and a goal batch of model GCBC take no return-to-go)")
        images = np.require(np.asarray(images, dtype=np.float32), requirements="C")
        action = np.require(np.asarray(action, dtype=np.int32), requirements="C")
        B, T = action.shape
        if goals is not None:
            goals = np.require(np.asarray(goals, dtype=np.float32), requirements="C")
            if images.ndim != 5 or images.shape[:2] != (B, T) or goals.shape != images.shape or T != self.cfg.window:
                raise ValueError(f"batch shapes: images {images.shape}, goals {goals.shape}, action {action.shape}")
            check(lib.arp_dt_set_batch_images_goal(self._h, _ffi.as_ptr(images, C.c_float), _ffi.as_ptr(goals, C.c_float), _ffi.as_ptr(action, C.c_int32), B))
        else:
            if images.shape[:2] != (B, T) or T != self.cfg.window:
                raise ValueError(f"batch shapes: images {images.shape}, action {action.shape}")
            rtg, rp = self._rtg(rtg, B, T)  # (model BC: None / NULL)
            check(lib.arp_dt_set_batch_images(self._h, _ffi.as_ptr(images, C.c_float), _ffi.as_ptr(action, C.c_int32), rp, B))
        self._B = B

    def classify(self, batch, use_symlog=None):
        """:func:`classify_batch` with this trainer's facts (and, model BC with an instruction attached, :meth:`check_instruction`)."""
        _check_instruction(getattr(self, "_instruct", None), batch)
        return classify_batch(batch, encoder=self._encoder is not None, gcbc=self.gcbc, use_symlog=self.cfg.use_symlog if use_symlog is None else use_symlog)

    def stage_batch(self, b, slot=None):
        """Put a classified batch (:func:`classify_batch`) in front of the policy step: synchronously (``slot`` None: the next forward / step reads it), or
        asynchronously into prefetch slot 0 / 1, to be read after :meth:`select`.  Returns whether the slot now holds frames (:meth:`encode_ahead` may follow)."""
        if b.kind in ("index", "index_pairs"):
            return self._stage_indices(slot if slot is None else int(slot), b.index, b.goal_index)
        frames = b.kind != "encodings"
        if slot is not None:
            self.upload_async(slot, b.image, b.action, b.rtg, images=frames, goals=b.goals)
        elif frames:
            self.set_batch_images(b.image, b.action, b.rtg, goals=b.goals)
        else:
            self.set_batch(b.image, b.action, b.rtg)
        return frames

    def forward(self):
        """ARPDT.__call__ (ARPDT.py:152-236) on the staged batch; model BC: BC.__call__ (BC.py:135-181), {action_pred, loss, acc}."""
        B, T, NA = self._B, self.cfg.window, self.cfg.n_actions
        logits = np.empty((B, T, NA), np.float32)
        if self.bc:
            m = np.empty(4, np.float32)
            check(lib.arp_dt_forward(self._h, _ffi.as_ptr(logits, C.c_float), None, _ffi.as_ptr(m, C.c_float)))
            return {"action_pred": logits, "loss": float(m[0]), "acc": float(m[1])}
        ret = np.empty((B, T, 1), np.float32)
        m = np.empty(4, np.float32)
        check(lib.arp_dt_forward(self._h, _ffi.as_ptr(logits, C.c_float), _ffi.as_ptr(ret, C.c_float), _ffi.as_ptr(m, C.c_float)))
        return {"action_pred": logits, "return_pred": ret, "loss": float(m[0]), "acc": float(m[1]), "trans_loss": float(m[2]),
                "return_loss": float(m[3])}

    def backward(self):
        check(lib.arp_dt_backward(self._h))

    def _set_batch_any(self, enc, action=None, rtg=None):
        """Stage synchronously what :meth:`greedy_action` / :meth:`greedy_return` are given: a batch dict of any kind (:func:`classify_batch`), or the arrays
        of one -- encodings [B, T, tokens, dim] or, with a frozen encoder attached, normalised frames [B, T, H, W, 3] (row N1: what the rollout loop has)."""
        if isinstance(enc, dict):
            self.stage_batch(self.classify(enc))
        else:  # (arrays are staged as given: the caller has prepared the return-to-go)
            self.stage_batch(self.classify({"image": enc, "action": action, "rtg": rtg}, use_symlog=False))

    def greedy_action(self, enc, action=None, rtg=None):
        """ARPDT.greedy_action (ARPDT.py:488-492): argmax of the LAST time step's action logits."""
        self._set_batch_any(enc, action, rtg)
        return self.forward()["action_pred"][:, -1, :].argmax(-1)

    def greedy_return(self, enc, action=None, rtg=None):
        """ARPDT.greedy_return (ARPDT.py:494-495): symexp(return_pred) (utils.py symexp = sign(x)(exp|x| - 1)).  BC has none."""
        if self.bc:
            raise ValueError("model BC has no return head: greedy_return exists for ARP-DT only (BC.py defines greedy_action alone)")
        self._set_batch_any(enc, action, rtg)
        r = self.forward()["return_pred"]
        return np.sign(r) * (np.exp(np.abs(r)) - 1.0)

    def train_step(self, lr):
        aux = np.empty(9, np.float32)
        check(lib.arp_dt_train_step(self._h, float(lr), _ffi.as_ptr(aux, C.c_float)))
        d = {k: float(aux[i]) for i, k in enumerate(AUX_KEYS)}
        d["train_state_step"] = int(aux[6])
        d["grad_norm"] = float(aux[8])
        return d

    def train_step_async(self, lr):
        check(lib.arp_dt_train_step_async(self._h, float(lr)))

    def sync(self):
        check(lib.arp_dt_sync(self._h))

    def record(self, event):
        check(lib.arp_dt_event_record(self._h, event.ptr))

    # -- data parallelism (one process per GPU, RCCL over xGMI) ---------------------------------------
    @staticmethod
    def new_unique_id():
        buf = C.create_string_buffer(128)
        check(lib.arp_dt_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, unique_id, world, rank):
        check(lib.arp_dt_comm_init(self._h, C.create_string_buffer(unique_id, 128), world, rank))
        self.world, self.rank = world, rank

    def broadcast_state(self):
        """sync_state_fn (main_procgen.py:94-101)."""
        check(lib.arp_dt_broadcast_state(self._h))

    def comm_info(self):
        """what the RCCL communicator says about itself: nranks (ncclCommCount), rank (ncclCommUserRank), device, RCCL version code"""
        v = (C.c_int32 * 5)()
        check(lib.arp_dt_comm_info(self._h, v))
        return {"nranks": v[0], "rank": v[1], "device": v[2], "rccl_version": v[3], "has_comm": bool(v[4])}

    def comm_selfcheck(self):
        """all-reduce(sum) of ``rank + 1`` through the step's communicator: world (world + 1) / 2 on every rank"""
        d = C.c_double()
        check(lib.arp_dt_comm_selfcheck(self._h, C.byref(d)))
        return d.value

    def profile(self, on=True):
        check(lib.arp_dt_profile_enable(self._h, int(on)))

    def profile_reset(self):
        check(lib.arp_dt_profile_reset(self._h))

    def profile_read(self):
        buf = C.create_string_buffer(1 << 16)
        check(lib.arp_dt_profile_json(self._h, buf, len(buf)))
        return json.loads(buf.value.decode())


class TrainState:
    """The reference's flax ``TrainState`` (params + optax state + step), resident on the GPU."""

    def __init__(self, trainer):
        self.trainer = trainer
        self._live = True

    @classmethod
    def create(cls, model, params, mode="f16", device=0, adapter_corrections=None):
        cfg = model if isinstance(model, PolicyConfig) else PolicyConfig(**dict(model))
        tr = PolicyTrainer(cfg, mode=mode, device=device, adapter_corrections=adapter_corrections)
        tr.set_params(params)
        return cls(tr)

    @property
    def step(self):
        return self.trainer.step

    @property
    def params(self):
        return self.trainer.get_params()


def symlog(x):
    """``sign(x) * log(1 + |x|)`` (arp_dt/utils.py:445-446)."""
    x = np.asarray(x, np.float32)
    return np.sign(x) * np.log1p(np.abs(x))


def is_index_batch(batch):
    """A batch that names rows of an attached device-resident dataset: a dict whose only key is ``"index"``."""
    return isinstance(batch, dict) and set(batch) == {"index"}


def _one_instruction(instruct, text_padding_mask=None):
    """(tokens int32 [L], mask f32 [L]) of ``instruct`` given as ``[L]``, ``[1, L]`` or ``[B, L]`` with all rows equal (the mask likewise; None: nothing padded).
    Rows that differ are refused: BC.py:290-291 tiles the instructions with ``jnp.tile(text, (T, 1))``, which pairs frame row i of the ``[B * T]`` frames with
    instruction ``i mod B``, not ``i // T`` -- with differing rows the reference itself feeds frames the wrong instruction, so only one instruction per
    batch is meaningful."""
    tok = np.asarray(_first_view(instruct))
    mask = np.zeros(tok.shape, np.float32) if text_padding_mask is None else np.asarray(_first_view(text_padding_mask), np.float32)
    if tok.ndim not in (1, 2) or mask.shape != tok.shape or tok.shape[-1] < 1:
        raise ValueError(f"instruct must be int [L], [1, L] or [B, L] and text_padding_mask of its shape: {tok.shape}, {mask.shape}")
    if tok.ndim == 2:
        if (tok != tok[:1]).any() or ((mask > 0) != (mask[:1] > 0)).any():
            raise _ffi.ArpError("instruct rows differ: one instruction per batch (BC.py:290-291 tiles them with jnp.tile(text, (T, 1)), pairing frame row i with "
                                "instruction i mod B, not i // T, so the reference itself is only meaningful with one)")
        tok, mask = tok[0], mask[0]
    return np.require(tok.astype(np.int32), requirements="C"), np.require(mask.astype(np.float32), requirements="C")


def _check_instruction(attached, batch):
    """:meth:`PolicyTrainer.check_instruction`: ``attached`` is the (tokens, mask) of attach_encoder(instruct=...), or None"""
    if attached is None or not isinstance(batch, dict) or batch.get("instruct") is None:
        return
    tok, mask = _one_instruction(batch["instruct"], batch.get("text_padding_mask"))
    if tok.shape != attached[0].shape or (tok != attached[0]).any() or ((mask > 0) != (attached[1] > 0)).any():
        raise _ffi.ArpError('batch["instruct"] / batch["text_padding_mask"] differ from the instruction attached with attach_encoder(instruct=...): a handle '
                            "trains one game, one instruction")


def is_index_pair_batch(batch):
    """Model GCBC's batch from the device-resident dataset: a dict with the keys ``"index"`` and ``"goal_index"`` exactly
    (``DeviceDataset.index_batches(goal_rng=...)``)."""
    return isinstance(batch, dict) and set(batch) == {"index", "goal_index"}


def _first_view(v):
    """the array of a per-image-key dict (one image key here), or the array itself"""
    return np.asarray(next(iter(v.values())) if isinstance(v, dict) else v)


def _batch_arrays(batch, use_symlog=False):
    """(encodings, actions, return-to-go) of a reference batch dict.  ``batch["rtg"]`` holds one array per image view; the model
    embeds -- and regresses onto -- their MEAN, each view passed through symlog first when ``config.use_symlog``
    (arp_dt/ARPDT.py:251-258,281-293).  Both uses see the same array, so the transform is applied here, once, on the host."""
    image = batch["image"]
    enc = next(iter(image.values())) if isinstance(image, dict) else image
    rtg = batch.get("rtg")
    if rtg is None:  # (a BC batch: BC.encode reads no return-to-go)
        return np.asarray(enc), np.asarray(batch["action"]), None
    views = [np.asarray(v, np.float32) for v in rtg.values()] if isinstance(rtg, dict) else [np.asarray(rtg, np.float32)]
    if use_symlog:
        views = [symlog(v) for v in views]
    rtg = np.mean(np.stack(views), axis=0) if isinstance(rtg, dict) else views[0]
    return np.asarray(enc), np.asarray(batch["action"]), np.asarray(rtg)


@dataclass
class ClassifiedBatch:
    """What :func:`classify_batch` makes of a host batch: its kind and the arrays that kind carries (the others stay None)."""
    kind: str                 # "encodings" | "frames" | "frames+goals" | "index" | "index_pairs"
    image: object = None      # encodings [B, T, tokens, dim], or frames [B, T, H, W, 3]
    goals: object = None      # "frames+goals": the goal frames, the frames' shape
    action: object = None
    rtg: object = None        # the mean over the views, symlog'd first under use_symlog; None where the batch holds none
    index: object = None      # "index" / "index_pairs": rows of the attached dataset
    goal_index: object = None  # "index_pairs": the goal row of every row


def classify_batch(batch, *, encoder, gcbc, use_symlog=False):
    """The one place that answers "what kind of batch is this?", for a batch dict already cut to this rank (:func:`shard_batch`).  ``encoder``: a frozen
    encoder is attached; ``gcbc``: the model is GCBC.  Needs no GPU.

    * exactly ``{"index", "goal_index"}`` / exactly ``{"index"}``: rows of the attached device-resident dataset (``DeviceDataset.index_batches``);
    * otherwise the reference's batch dict (:func:`_batch_arrays`): ``batch["image"]`` holds frames when an encoder is attached and the array is
      ``[B, T, H, W, 3]``, else encodings; ``batch["goal"]`` -- the reference's dataset puts it in every batch -- is read by model GCBC alone, beside frames."""
    if is_index_pair_batch(batch):
        return ClassifiedBatch("index_pairs", index=batch["index"], goal_index=batch["goal_index"])
    if is_index_batch(batch):
        return ClassifiedBatch("index", index=batch["index"])
    image, action, rtg = _batch_arrays(batch, use_symlog)
    if not (encoder and image.ndim == 5 and image.shape[-1] == 3):
        return ClassifiedBatch("encodings", image=image, action=action, rtg=rtg)
    if gcbc and batch.get("goal") is not None:
        return ClassifiedBatch("frames+goals", image=image, goals=_first_view(batch["goal"]), action=action, rtg=rtg)
    return ClassifiedBatch("frames", image=image, action=action, rtg=rtg)


def shard_batch(batch, rank, world, device_axis=False):
    """This rank's part of a global batch: ``generate_batch``'s ``x.reshape(n_devices, -1, *x.shape[1:])[rank]``
    (main_procgen.py:645-683) -- contiguous, equal parts of the leading axis, every leaf of the (nested) batch dict alike;
    ``None`` leaves stay ``None``.  ``device_axis=True``: the batch already carries the reference's leading ``[n_devices, ...]``
    axis (what its pmapped train_step_fn receives) and the rank's slice is ``x[rank]``."""
    if world == 1 and not device_axis:
        return batch

    def cut(x):
        x = np.asarray(x)
        if device_axis:
            if x.shape[0] != world:
                raise ValueError(f"leading device axis is {x.shape[0]}, expected {world}")
            return x[rank]
        if x.shape[0] % world:
            raise ValueError(f"global batch of {x.shape[0]} does not divide over {world} ranks")
        per = x.shape[0] // world
        return x[rank * per : (rank + 1) * per]

    def walk(v):
        if v is None:
            return None
        if isinstance(v, dict):
            return {k: walk(x) for k, x in v.items()}
        return cut(v)

    return walk(batch)


def torch_object_broadcast(dist):
    """``bcast`` for :class:`DataParallel` on an initialised ``torch.distributed`` group (gloo control plane)."""

    def bcast(obj, src=0):
        box = [obj]
        dist.broadcast_object_list(box, src=src)
        return box[0]

    return bcast


class DataParallel:
    """One process per GPU around a :class:`PolicyTrainer` -- the reference's ``pmap`` over devices (main_procgen.py:94-141):

    * the RCCL unique id is made on rank 0 and handed to every rank over the control plane (``bcast``);
    * ``sync_state_fn`` (``:94-101``): every rank takes rank 0's parameters, Adam moments and step counter, once, at start;
    * a step = this rank's shard of the global batch (:func:`shard_batch`) through forward/backward, ONE all-reduce(sum) of
      the flat gradient + one of the loss scalars inside the library (``pmean``, ``:132``; the 1/world is folded into the
      update), then the identical clip + Adam update on every rank.  No other collective."""

    def __init__(self, trainer, rank, world, bcast):
        if not (0 <= rank < world):
            raise ValueError(f"rank {rank} outside world {world}")
        self.trainer, self.rank, self.world = trainer, int(rank), int(world)
        uid = trainer.new_unique_id() if rank == 0 else None
        uid = bcast(uid, 0)
        if not isinstance(uid, (bytes, bytearray)) or len(uid) != 128:
            raise ValueError("the control plane did not deliver rank 0's 128-byte RCCL unique id")
        trainer.comm_init(bytes(uid), self.world, self.rank)
        trainer.broadcast_state()

    def certify(self):
        return certify_collective(self.trainer, self.rank, self.world)

    def set_global_batch(self, batch, device_axis=False):
        self.trainer.set_batch(*_batch_arrays(shard_batch(batch, self.rank, self.world, device_axis), self.trainer.cfg.use_symlog))

    def train_step(self, batch, lr, device_axis=False):
        """aux is the rank-averaged aux of the reference's pmean: identical on every rank."""
        self.set_global_batch(batch, device_axis)
        return self.trainer.train_step(lr)


def certify_collective(trainer, rank, world):
    """What a multi-GPU bench line prints about its communicator: the rank count and user rank RCCL itself reports
    (``ncclCommCount`` / ``ncclCommUserRank``, not the environment's), and one all-reduce(sum) of ``rank + 1`` through it -- every rank
    must read world (world + 1) / 2.  ``ok`` is False when any of the three disagrees with (rank, world)."""
    info = trainer.comm_info()
    got = trainer.comm_selfcheck()
    want = world * (world + 1) / 2.0
    ok = info["nranks"] == world and info["rank"] == rank and got == want and (world == 1 or info["has_comm"])
    return dict(info, allreduce_selfcheck=got, expected=want, ok=bool(ok),
                NCCL_ALGO=os.environ.get("NCCL_ALGO"), NCCL_PROTO=os.environ.get("NCCL_PROTO"))


def bucket_plan(cfg):
    """Flat-gradient ranges ``[(lo, hi)] * 4`` of the data-parallel step's two all-reduce buckets (bucket 1 = ranges 0, 1:
    image_text_input's kernel + everything the transformer owns, launched while the adapter's backward still runs; bucket 2 =
    ranges 2, 3) and the flat parameter count.  Needs no GPU."""
    c = _dt_cfg(cfg, MODE_F16, 0)
    r = (C.c_int64 * 8)()
    tot = C.c_int64()
    check(lib.arp_dt_bucket_plan(C.byref(c), r, C.byref(tot)))
    return [(r[2 * i], r[2 * i + 1]) for i in range(4)], tot.value


def _threefry2x32(key, x0, x1):
    """Threefry-2x32, 20 rounds (Salmon et al. 2011) on uint32 arrays: the block cipher behind jax.random's default PRNG."""
    rot = ((13, 15, 26, 6), (17, 29, 16, 24))
    k0, k1 = np.uint32(key[0]), np.uint32(key[1])
    ks = (k0, k1, np.uint32(k0 ^ k1 ^ np.uint32(0x1BD11BDA)))
    x0 = (x0 + ks[0]).astype(np.uint32)
    x1 = (x1 + ks[1]).astype(np.uint32)
    for i in range(5):
        for r in rot[i % 2]:
            x0 = (x0 + x1).astype(np.uint32)
            x1 = ((x1 << np.uint32(r)) | (x1 >> np.uint32(32 - r))).astype(np.uint32)
            x1 = x1 ^ x0
        x0 = (x0 + ks[(i + 1) % 3]).astype(np.uint32)
        x1 = (x1 + ks[(i + 2) % 3] + np.uint32(i + 1)).astype(np.uint32)
    return x0, x1


def split_rng(rng):
    """``next_rng, split_rng = jax.random.split(rng)`` (main_procgen.py:130,163) for a raw threefry key ``uint32[2]`` (or a stack
    ``[..., 2]`` of them, the pmapped ``sharded_rng``), computed as jax's original (non-partitionable) split does: counts
    ``0..3`` enciphered pairwise under the key.  Anything else (None, an int seed, an opaque object) is carried through: the
    shipped configuration has dropout 0, so the step never draws from it."""
    a = np.asarray(rng) if isinstance(rng, (np.ndarray, list, tuple)) else None
    if a is None or a.dtype.kind not in "ui" or a.ndim < 1 or a.shape[-1] != 2:
        return rng, rng
    a = a.astype(np.uint32)
    if a.ndim > 1:
        parts = [split_rng(k) for k in a.reshape(-1, 2)]
        return (np.stack([p[0] for p in parts]).reshape(a.shape), np.stack([p[1] for p in parts]).reshape(a.shape))
    with np.errstate(over="ignore"):
        y0, y1 = _threefry2x32(a, np.array([0, 1], np.uint32), np.array([2, 3], np.uint32))
    out = np.concatenate([y0, y1]).reshape(2, 2)
    return out[0], out[1]


class DeviceBatch:
    """A batch resident in (or on its way into) one of the trainer's two device slots: what :func:`prefetch_to_device` yields
    and what ``train_step_fn`` / ``val_step_fn`` accept where the reference passes a device-put batch."""

    def __init__(self, trainer, slot, release):
        self.trainer, self.slot, self._release = trainer, slot, release

    def done(self):
        """The step that read this batch has been synchronised (its aux was read back): the slot may be refilled."""
        if self._release is not None:
            self._release()
            self._release = None


_SLOT_OWNER_LOCK = __import__("threading").Lock()


def prefetch_to_device(iterator, size, trainer, *, rank=0, world=1, device_axis=False):
    """``flax.jax_utils.prefetch_to_device(iterator, size, devices)`` as the reference uses it (main_procgen.py:703,706: size 2):
    host batches (the reference's batch dicts) are uploaded into the trainer's two device slots by a background thread -- the
    ctypes call releases the GIL, the copy runs on the handle's copy stream -- while the main thread is inside ``train_step_fn``
    on the other slot.  Yields :class:`DeviceBatch`.  ``size`` > 2 is clamped: the library keeps two slots.

    The two device slots belong to the TRAINER, and one prefetcher at a time owns them.  The reference opens ``train_iter`` and
    ``val_iter`` side by side on the same state (main_procgen.py:703-708); here the prefetcher that starts first owns the slots and a
    second one opened while it is live yields prepared HOST batches instead -- ``train_step_fn`` / ``val_step_fn`` stage those through the
    handle's third, synchronous slot -- so a validation upload can never land in a slot that holds an uploaded-but-unconsumed training
    batch, and neither iterator can starve the other of slots."""
    import queue
    import threading
    import warnings

    # Ownership is decided HERE, when the prefetcher is created -- not at the first next() (this used to be a generator function: whichever
    # iterator was pulled first won, so a validation iterator pulled before the training one silently demoted the training loop).
    with _SLOT_OWNER_LOCK:
        owner = trainer._prefetch_owner is None
        if owner:
            token = object()
            trainer._prefetch_owner = token
    if not owner:
        warnings.warn("prefetch_to_device: another prefetcher owns this trainer's two device slots; this one yields host batches (staged "
                      "synchronously by the step functions)", RuntimeWarning, stacklevel=2)
        return (batch for batch in iterator)  # no device slots for this one: the host-side preparation only

    free = queue.Queue()
    for s in range(min(max(int(size), 1), 2)):
        free.put(s)
    ready = queue.Queue()
    stop = threading.Event()

    def worker():
        try:
            for batch in iterator:
                slot = free.get()
                if stop.is_set():
                    return
                part = shard_batch(batch, rank, world, device_axis)
                images = trainer.stage_batch(trainer.classify(part), slot)
                # (model BC with its instruction attached: off unless asked for -- measured 0.61 ms lower than the arm without it, inside that arm's 1.30 ms
                #  spread of round medians: profiles/instructrl_timing.txt; ARP_DT_ENCODE_AHEAD=1 turns it on)
                ahead_default = "0" if getattr(trainer, "_instruct", None) is not None else "1"
                if images and os.environ.get("ARP_DT_ENCODE_AHEAD", ahead_default) != "0" and os.environ.get("ARP_DT_ENC_EAGER", "1") != "0":
                    trainer.encode_ahead(slot)  # the frozen encoder's pass for this batch runs beside the step that is reading the OTHER slot
                ready.put(DeviceBatch(trainer, slot, lambda s=slot: free.put(s)))
            ready.put(None)
        except BaseException as e:  # surfaces in the consumer
            ready.put(e)

    th = threading.Thread(target=worker, daemon=True)

    def release():
        stop.set()
        free.put(0)  # wake a worker blocked on a free slot
        if th.is_alive():
            th.join(timeout=30)  # an upload in flight finishes before the slots change hands
        if th.is_alive():
            # the worker is still inside an upload: the slots are NOT free -- keep the ownership (a new prefetcher is demoted to host staging) and say so
            raise RuntimeError("prefetch_to_device: the upload thread did not stop within 30 s; the device slots stay owned by this prefetcher")
        with _SLOT_OWNER_LOCK:
            if trainer._prefetch_owner is token:
                trainer._prefetch_owner = None

    def gen():
        th.start()
        try:
            while True:
                item = ready.get()
                if item is None:
                    return
                if isinstance(item, BaseException):
                    raise item
                yield item
        finally:
            release()

    g = gen()
    # a prefetcher that is created and dropped without ever being pulled must give the slots back too
    import weakref
    weakref.finalize(g, lambda: (None if th.is_alive() else _release_if_unstarted(trainer, token)))
    return g


def _release_if_unstarted(trainer, token):
    with _SLOT_OWNER_LOCK:
        if trainer._prefetch_owner is token:
            trainer._prefetch_owner = None


def _stage(tr, batch, rank, world, device_axis):
    """Put ``batch`` (a host batch dict, or a DeviceBatch from prefetch_to_device) in front of the next step."""
    if isinstance(batch, DeviceBatch):
        tr.select(batch.slot)
        return batch
    part = shard_batch(batch, rank, world, device_axis)
    tr.stage_batch(tr.classify(part))
    return None


def create_val_step(model, *, rank=0, world=1, device_axis=False):
    """main_procgen.py:144-169: ``val_step_fn(state, batch, rng) -> (aux, next_rng)`` -- forward only (``deterministic=True``),
    aux = the rank mean of ``loss, trans_loss, return_loss, acc * 100``; the state is NOT consumed (no ``donate_argnums``)."""

    def val_step_fn(state, batch, rng):
        tr = state.trainer
        if world > 1 and getattr(tr, "world", 1) != world:
            raise ValueError("world > 1: wrap the state's trainer in DataParallel (RCCL communicator + state sync) first")
        dev = _stage(tr, batch, rank, world, device_axis)
        aux = tr.val_step()
        if dev is not None:
            dev.done()
        return aux, split_rng(rng)[0]

    return val_step_fn


def create_train_step(model, learning_rate, weight_decay, *, rank=0, world=1, device_axis=False):
    """main_procgen.py:104-141.  ``learning_rate`` is the schedule ``step -> lr`` (``:135``).  With ``world > 1`` (one process
    per GPU, the state's trainer wrapped by :class:`DataParallel` beforehand) every call steps on this rank's shard of the
    global batch it is given."""
    cfg = model if isinstance(model, PolicyConfig) else PolicyConfig(**dict(model))
    if abs(cfg.weight_decay - weight_decay) > 1e-12:
        cfg = PolicyConfig(**{**asdict(cfg), "weight_decay": float(weight_decay)})

    def train_step_fn(state, batch, rng):
        if not state._live:
            raise RuntimeError("this TrainState was donated to a previous train_step_fn call (donate_argnums=0)")
        tr = state.trainer
        if abs(tr.cfg.weight_decay - cfg.weight_decay) > 1e-12:
            raise ValueError("state was created with a different weight_decay than create_train_step")
        if world > 1 and getattr(tr, "world", 1) != world:
            raise ValueError("world > 1: wrap the state's trainer in DataParallel (RCCL communicator + state sync) first")
        dev = _stage(tr, batch, rank, world, device_axis)  # a host batch dict (synchronous upload) or a prefetched DeviceBatch
        aux = tr.train_step(learning_rate(tr.step))
        if dev is not None:
            dev.done()
        state._live = False
        # next_rng of jax.random.split(rng) (main_procgen.py:130) when rng is a raw threefry key; dropout is 0 in the shipped
        # configuration, so the step itself never draws from the split key
        return TrainState(tr), aux, split_rng(rng)[0]

    return train_step_fn
