"""Every handle and every test entry point gives back exactly what it took: device bytes, device buffers, streams, events and pinned host bytes.

The library's owners (arp_amd/csrc/runtime.h: DevBuf, PinBuf, Stream, Event) count every acquire and release in process-wide counters that
arp_debug_live reads.  Every case below reads them before and after and asserts EQUALITY of all five -- a condition, not a measurement: the counter
is the library's own, so other people's jobs on the device (which move its free memory) do not move it.  The cases are the paths whose buffers the
hand-written release lists of the destroy functions had lost (the policy handle's alibi / colpart0 / dres_part, the fine-tune handle's dropped), the
second-stream siblings of the labelling handle and what they share with their primary, and the early returns of the test entry points."""
import contextlib
import ctypes as C
import functools
import gc

import numpy as np
import pytest

from conftest import TINY as CLIP_TINY
from test_m3ae_gpu import TINY_ENC
from test_policy_gpu import SMALL, TINY

pytestmark = pytest.mark.gpu

NAMES = ("device bytes", "device buffers", "streams", "events", "pinned bytes")
FT_SMALLEST = dict(layers=2, width_v=64, width_t=64, embed=64, hidden=64)  # tests/test_finetune_gpu.py


def _live(lib):
    out = (C.c_int64 * 5)()
    lib.check(lib.lib.arp_debug_live(out))
    return dict(zip(NAMES, out))


@contextlib.contextmanager
def _unchanged(lib, what):
    gc.collect()  # (a handle an earlier test dropped without close() goes now, not in the middle of this one)
    before = _live(lib)
    yield before
    gc.collect()
    after = _live(lib)
    assert after == before, f"{what}: live resources before {before}, after {after}"


def _policy(kw, B, seed, mode):
    from arp_amd import synth_policy as S
    from arp_amd.train import PolicyConfig, PolicyTrainer
    cfg = PolicyConfig(**kw)
    tr = PolicyTrainer(cfg, mode=mode)
    tr.set_params(S.policy_params(cfg, seed=seed))
    return cfg, tr, S.policy_batch(cfg, B, seed=seed + 1)


def test_policy_handle_with_alibi_bias(gpu_lib):
    with _unchanged(gpu_lib, "policy handle, alibi_bias"):
        cfg, tr, batch = _policy(dict(TINY, alibi_bias=True), 4, 1, "f32")
        tr.set_batch(*batch)
        assert np.isfinite(tr.train_step(1e-3)["loss"])
        tr.close()


def test_policy_handle_on_the_fused_tn_path(gpu_lib):
    """SMALL in f16: the fused-dY + TN backward (colpart0, dres_part); three steps, so that the captured chain exists when the handle goes"""
    with _unchanged(gpu_lib, "policy handle, fused + TN path"):
        cfg, tr, batch = _policy(SMALL, 6, 21, "f16")
        for _ in range(3):
            tr.set_batch(*batch)
            assert np.isfinite(tr.train_step(1e-3)["loss"])
        tr.close()


def test_policy_handle_with_encoder_index_batches_and_encode_ahead(gpu_lib):
    """SMALL with the encodings' geometry taken from the attached encoder (17 tokens of width 64), as every encoder-inside test sizes its policy"""
    from arp_amd import dataset, m3ae, synth_policy as S
    from oracle import m3ae_np as M
    with _unchanged(gpu_lib, "policy handle + encoder + dataset"):
        ecfg = m3ae.EncoderConfig(**TINY_ENC)
        enc = m3ae.M3AEEncoder(ecfg, S.m3ae_params(M.EncConfig(**TINY_ENC), seed=5), mode="f16")
        cfg, tr, _ = _policy(dict(SMALL, enc_tokens=ecfg.tokens, enc_dim=ecfg.width), 1, 6, "f16")
        tr.attach_encoder(enc)
        rng = np.random.default_rng(3)
        ds = dataset.DeviceDataset(8, ecfg.img_res)
        ds.window_size = cfg.window
        ds.set_lut(dataset.default_lut())
        ds.upload_frames(0, rng.integers(0, 256, (8, ecfg.img_res, ecfg.img_res, 3), dtype=np.uint8))
        ds.set_labels(rng.integers(0, cfg.n_actions, 8), rng.random(8), np.zeros(8, np.int32), cfg.n_actions)
        tr.attach_dataset(ds)
        tr.upload_indices_async(0, [0, 3, 7, 5])
        tr.encode_ahead(0)
        tr.select(0)
        assert np.isfinite(tr.train_step(1e-3)["loss"])
        tr.close(); ds.close(); enc.close()


def test_finetune_handle_f16(gpu_lib):
    from arp_amd import finetune as FT
    with _unchanged(gpu_lib, "fine-tune handle, f16"):
        cfg = FT.FinetuneConfig(**FT_SMALLEST)
        tr = FT.FinetuneTrainer(cfg, mode="f16")
        tr.set_params(FT.synth_params(cfg, seed=1))
        tr.set_batch(*FT.synth_batch(cfg, 4, seed=2))
        assert np.isfinite(tr.train_step(1e-3)["loss"])
        assert tr.dropped_gradients == 0
        tr.close()


@functools.lru_cache(maxsize=None)
def _clip_inputs():
    from arp_amd import synth
    from oracle import clip_np
    ocfg = clip_np.ClipConfig(**CLIP_TINY)
    toks = [synth.prompt_tokens(n, 5, ctx=ocfg.ctx, vocab=ocfg.vocab, seed=4 + n) for n in (1, 2, 5)]
    return synth.clip_weights(ocfg, seed=3), synth.procgen_like_frames(256, 64, 64, seed=5), toks


def test_clip_handle_with_a_sibling(gpu_lib):
    """Two streams: 256 frames make a sibling, the copy stream and the fork / join / copy events; one frame takes the pinned buffers and the captured
    pass; a prompt set that grows re-allocates the primary's text features, which the sibling must read where they now are."""
    from arp_amd import clip
    Wt, frames, toks = _clip_inputs()
    with _unchanged(gpu_lib, "labelling handle, two streams") as before:
        m = clip.ClipLabeller(clip.ClipConfig(**CLIP_TINY), Wt, mode="bf16", n_streams=2).set_text(toks[0])
        first = m.label(frames)
        now = _live(gpu_lib)
        assert now["streams"] - before["streams"] == 3 and now["events"] - before["events"] >= 3, now  # primary + sibling + copy stream
        one = m.label(frames[:1])
        assert np.isfinite(one).all() and _live(gpu_lib)["pinned bytes"] > before["pinned bytes"]
        m.set_text(toks[1])
        m.set_text(toks[2])
        second = m.label(frames)
        fresh = clip.ClipLabeller(clip.ClipConfig(**CLIP_TINY), Wt, mode="bf16", n_streams=1).set_text(toks[2])
        want = fresh.label(frames)
        fresh.close()
        assert (second == want).all(), "the sibling labelled against other text features than the primary's current ones"
        assert not (second == first).all()
        m.close()


def _refused_gemm_bwd(lib, what):
    from test_backward_gemms_gpu import F32, REFUSALS, _run_bwd
    _, kind, mode, S, M, N, K, pa, pb, ldo = next(c for c in REFUSALS if c[0] == what)
    rows_a, cols_a = (M, K) if what.startswith("nn") else (K, M)
    A, B = np.ones((rows_a, cols_a + pa), np.float32), np.ones((K, N + pb), np.float32)
    return _run_bwd(lib, kind, mode, F32, S, A, cols_a + pa, B, N + pb, None, ldo, M, N, K, 1.0, False)[0]


def _refused_attention_form(lib):
    from test_attention_forms_gpu import E4M3, F16, _attn, _random_qkv
    return _attn(lib, F16, 0, _random_qkv(2, 160, 128, 1), 2, 160, 128, 2, 0, form=E4M3, scale=16.0)[0]  # 160 tokens: no MFMA instance, e4m3 refused


def _refused_qkv_attention(lib):
    from test_attention_forms_gpu import F16, _fused, _fused_random
    A, W, bias, _ = _fused_random(2, 65, 128, 1, F16, 1, 0)  # 65 tokens: one past the kernel's frame
    return _fused(lib, F16, A, W, bias, 2, 65, 128, 1, 0)[0]


@pytest.mark.parametrize("family,call", [
    ("arp_op_gemm_bwd, TN", lambda lib: _refused_gemm_bwd(lib, "tn: K % 64")),
    ("arp_op_gemm_bwd, NN", lambda lib: _refused_gemm_bwd(lib, "nn: K % 64")),
    ("arp_op_attention_forms", _refused_attention_form),
    ("arp_op_qkv_attention", _refused_qkv_attention),
], ids=lambda v: v if isinstance(v, str) else "")
def test_a_refused_entry_point_call_gives_everything_back(gpu_lib, family, call):
    """the launcher refuses AFTER the entry has uploaded its operands: the early return must free them"""
    with _unchanged(gpu_lib, family):
        assert call(gpu_lib) != 0 and gpu_lib.last_error(), family


def _cycle_clip():
    from arp_amd import clip
    Wt, _, toks = _clip_inputs()
    clip.ClipLabeller(clip.ClipConfig(**CLIP_TINY), Wt, mode="f16").set_text(toks[0]).close()


def _cycle_encoder():
    from arp_amd import m3ae, synth_policy as S
    from oracle import m3ae_np as M
    m3ae.M3AEEncoder(m3ae.EncoderConfig(**TINY_ENC), S.m3ae_params(M.EncConfig(**TINY_ENC), seed=5), mode="f16").close()


def _cycle_policy():
    _policy(TINY, 1, 1, "f16")[1].close()


def _cycle_finetune():
    from arp_amd import finetune as FT
    FT.FinetuneTrainer(FT.FinetuneConfig(**FT_SMALLEST), mode="f16").close()


def _cycle_dataset():
    from arp_amd import dataset
    dataset.DeviceDataset(8, 64).close()


@pytest.mark.parametrize("cycle", [_cycle_clip, _cycle_encoder, _cycle_policy, _cycle_finetune, _cycle_dataset], ids=lambda f: f.__name__[7:])
def test_two_create_close_cycles_in_a_row(gpu_lib, cycle):
    with _unchanged(gpu_lib, cycle.__name__) as before:
        cycle()
        gc.collect()
        after_first = _live(gpu_lib)
        cycle()
        gc.collect()
        assert _live(gpu_lib) == after_first == before, (before, after_first, _live(gpu_lib))
