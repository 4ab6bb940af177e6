"""The frozen M3AE image encoder on MI355X.

Mirrors ``MaskedMultimodalAutoencoder.forward_representation`` for the image-only call ARP-DT makes
(/root/reference/arp_dt/models/m3ae/model.py:471-496, called at arp_dt/ARPDT.py:451-458 under
``stop_gradient``): float frames ``[n, 256, 256, 3]`` (already normalised) -> ``[n, 257, 768]``.
Weights are the Flax parameter tree flattened with '/' (what ``load_m3ae_model_vars`` returns under
``["params"]``).  All compute is in libarp_hip.so (same kernels as the CLIP image tower).
"""
import ctypes as C
import json
from dataclasses import dataclass

import numpy as np

from . import _ffi
from ._ffi import MODE_BF16, MODE_F16, MODE_F16C, MODE_F16X3, MODE_F32, check, lib


@dataclass(frozen=True)
class EncoderConfig:
    """get_transformer_by_config("base") (m3ae/model.py:935-941) at 256x256, patch 16."""
    patch: int = 16
    width: int = 768
    layers: int = 12
    heads: int = 12
    mlp_ratio: int = 4
    img_res: int = 256

    @property
    def tokens(self):
        return (self.img_res // self.patch) ** 2 + 1

    @property
    def gc_tokens(self):
        """tokens of one (frame, goal) pair in :meth:`M3AEEncoder.forward_gc_representations`: class token + both frames' patches"""
        return 2 * (self.img_res // self.patch) ** 2 + 1

    def text_tokens(self, L):
        """tokens of one frame with an instruction of ``L`` tokens (:meth:`M3AEEncoder.forward_representation` with ``text``): class token + patches + L"""
        return self.tokens + int(L)


def flops_per_frame(cfg):
    n, d = cfg.tokens, cfg.width
    macs = (n - 1) * cfg.patch * cfg.patch * 3 * d + cfg.layers * (n * (4 * d * d + 2 * cfg.mlp_ratio * d * d) + cfg.heads * 2 * n * n * (d // cfg.heads))
    return 2 * macs


LATENCY_ROWS_DEFAULT = 514  # arp_enc::lat_rows as the library sets it: two frames at 257 tokens


class M3AEEncoder:
    def __init__(self, cfg, params, mode="bf16", device=0, max_frames=128, attn_impl=0):
        """mode: "f16" / "bf16" (16-bit GEMM operands: throughput modes with a stated error), "f32" (f32-input MFMA: the parity mode) or
        "f16x3" (every GEMM operand an (hi, lo) pair of binary16 values, three 16-bit MFMAs per product, attention / LayerNorm in f32: f32-level error at
        about twice the f32 mode's speed)."""
        _ffi.require_gpu()
        self.cfg, self.mode, self.max_frames = cfg, mode, int(max_frames) if max_frames > 0 else 128
        c = _ffi.EncCfg(cfg.patch, cfg.width, cfg.layers, cfg.heads, cfg.mlp_ratio, cfg.img_res, {"bf16": MODE_BF16, "f16": MODE_F16, "f32": MODE_F32, "f16x3": MODE_F16X3, "f16c": MODE_F16C}[mode],
                        device, max_frames, attn_impl)
        h = C.c_void_p()
        check(lib.arp_enc_create(C.byref(c), C.byref(h)))
        self._h = h
        for name, val in params.items():
            a = np.require(np.asarray(val, dtype=np.float32), requirements="C")
            shape = (C.c_int64 * max(a.ndim, 1))(*a.shape)
            check(lib.arp_enc_load_weight(h, name.encode(), _ffi.as_ptr(a, C.c_float), shape, a.ndim))
        check(lib.arp_enc_finalize_weights(h))

    def forward_representation(self, images, text=None, text_padding_mask=None):
        """Without ``text``: the image-only call, ``[n, tokens, width]``.  With ``text`` (InstructRL's call, arp_dt/BC.py:283-321): int token ids ``[L]`` (one
        instruction for every frame) or ``[n, L]``, ``text_padding_mask`` of the same shape with > 0 = padded (default: nothing padded) ->
        ``[n, 1 + P + L, width]``; padded text keys are out of every softmax.  Needs the two text weights in ``params``
        (``synth_policy.add_m3ae_text_params`` for seeded ones).  Modes f32 / f16 / bf16 / f16x3; f16c raises."""
        x = np.require(np.asarray(images, dtype=np.float32), requirements="C")
        if x.ndim != 4 or x.shape[1:] != (self.cfg.img_res, self.cfg.img_res, 3):
            raise ValueError(f"images must be float [n, {self.cfg.img_res}, {self.cfg.img_res}, 3]")
        if text is None:
            if text_padding_mask is not None:
                raise ValueError("text_padding_mask without text")
            out = np.empty((x.shape[0], self.cfg.tokens, self.cfg.width), np.float32)
            check(lib.arp_enc_forward(self._h, _ffi.as_ptr(x, C.c_float), x.shape[0], _ffi.as_ptr(out, C.c_float)))
            return out
        tok = np.require(np.asarray(text, dtype=np.int32), requirements="C")
        if tok.ndim not in (1, 2) or tok.shape[-1] < 1 or (tok.ndim == 2 and tok.shape[0] != x.shape[0]):
            raise ValueError("text must be int [L] or [n, L]")
        mask = np.zeros(tok.shape, np.float32) if text_padding_mask is None else np.require(np.asarray(text_padding_mask, dtype=np.float32), requirements="C")
        if mask.shape != tok.shape:
            raise ValueError("text_padding_mask must have the shape of text")
        L = tok.shape[-1]
        out = np.empty((x.shape[0], self.cfg.text_tokens(L), self.cfg.width), np.float32)
        check(lib.arp_enc_forward_text(self._h, _ffi.as_ptr(x, C.c_float), x.shape[0], _ffi.as_ptr(tok, C.c_int32), _ffi.as_ptr(mask, C.c_float), L,
                                       int(tok.ndim == 2), _ffi.as_ptr(out, C.c_float)))
        return out

    def forward_gc_representations(self, images, goals):
        """``forward_gc_representations`` (m3ae/model.py:498-525, GCBC's encoder call): float frames and goal frames ``[n, res, res, 3]`` ->
        ``[n, gc_tokens, width]``; row 0 the class token, rows ``1..P`` the frame's patches, rows ``P+1..2P`` the goal's.  ``max_frames`` counts pairs.
        Modes f32 / f16 / bf16 / f16x3; f16c raises."""
        x = np.require(np.asarray(images, dtype=np.float32), requirements="C")
        g = np.require(np.asarray(goals, dtype=np.float32), requirements="C")
        if x.ndim != 4 or x.shape[1:] != (self.cfg.img_res, self.cfg.img_res, 3) or g.shape != x.shape:
            raise ValueError(f"images and goals must both be float [n, {self.cfg.img_res}, {self.cfg.img_res}, 3]")
        out = np.empty((x.shape[0], self.cfg.gc_tokens, self.cfg.width), np.float32)
        check(lib.arp_enc_forward_gc(self._h, _ffi.as_ptr(x, C.c_float), _ffi.as_ptr(g, C.c_float), x.shape[0], _ffi.as_ptr(out, C.c_float)))
        return out

    def set_streams(self, n_streams=2, first_part_frames=0, min_part_frames=0):
        """Part streams of a call (``arp_enc_set_streams``): contiguous parts of the frames on HIP streams of their own; same encodings for every setting."""
        check(lib.arp_enc_set_streams(self._h, int(n_streams), int(first_part_frames), int(min_part_frames)))

    def set_latency_rows(self, rows, host_calls=None):
        """The latency path's row limit (``arp_enc_set_latency``): a call of at most ``rows`` token rows in total (frames x tokens; f16 / bf16) runs the skinny
        GEMMs instead of the throughput tiles.  A rollout session's per-step pass takes the path by default; ``host_calls=True`` makes
        :meth:`forward_representation` and :meth:`forward_gc_representations` take it too.  A goal-conditioned call counts ``pairs x gc_tokens`` rows.
        ``rows=0`` turns it off for every caller."""
        check(lib.arp_enc_set_latency(self._h, int(rows), -1 if host_calls is None else int(bool(host_calls))))

    def profile(self, on=True):
        check(lib.arp_enc_profile_enable(self._h, int(on)))

    def profile_read(self):
        buf = C.create_string_buffer(1 << 16)
        check(lib.arp_enc_profile_json(self._h, buf, len(buf)))
        return json.loads(buf.value.decode())

    def close(self):
        if getattr(self, "_h", None):
            lib.arp_enc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
