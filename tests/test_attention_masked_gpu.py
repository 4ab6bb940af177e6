"""The key-masked instances of the key-blocked attention kernels (csrc/attention_long.h: attn_long_masked_kernel<f16 | bf16>, attn_long_f32_kernel<.., true>)
through arp_op_attention_masked -- so through tower.h::launch_attention -- on sentinel-prefilled byte buffers, with the checks of
tests/test_attention_forms_gpu.py.  A mask is one bit per key (1 = visible) in 32-bit words, per sample with a word stride, stride 0 = one mask for the call.

(a) EXACTLY SOLVABLE inputs (test_attention_forms_gpu.py's docstring; test_attention_long_gpu.py's for why the online softmax keeps them exact), built here so
that a sample's heads share one group assignment -- the mask is per sample, not per head.  The mask hides, in every second group of even size, the half
of its members with the lowest key indices: never key 0 (alone in its group), never a whole group.  A hidden key scores -inf, weight exactly 0, so a row
is the mean over the VISIBLE members of its group: bit equality where that count is a power of two, the 1.5-ulp interval of the one division elsewhere.
(b) RANDOM inputs against float64 (hidden keys at -inf) at tests/test_ops_gpu.py::test_attention's bars, under three masks -- a suffix mask that hides the
last key block wholly and the one before it partly, keys 64 .. 127 hidden (an interior block the kernel skips), a scattered mask -- each shared by the call,
and two of them as different per-sample masks.
(c) ALL-VISIBLE mask: the unmasked kernels' bits.  f32: at every length (impl 1, attn_valu_kernel, below 289 keys: attn_long_f32_kernel gives its bits);
16-bit: from 289 keys on, where the unmasked launcher takes the key-blocked kernel too (below, the unmasked kernel is attn_mfma_kernel, another algorithm).
(d) f32: a visible query row has the bits the unmasked f32 kernel gives it on the sequence with the hidden K / V rows removed.
(e) nq < N leaves the other rows' fill; the query split on / off gives the same bits.
(f) Refusals: key 0 hidden, causal, the other output forms, 1025 keys, head_dim 32 -- an error string, every output byte untouched.

Geometry: D = 128, 2 heads, B = 2 (B = 1 at 1023 and 1024 keys)."""
import ctypes as C

import numpy as np
import pytest

from lowbits import BF16, F16
from test_attention_forms_gpu import (E4M3, F16C, F32, H64, PLAIN, SPLIT3, _attn, _buffer, _check_plain_exact, _check_plain_random, _fp, _is_fill, _is_pow2,
                                      _random_qkv, _rnd, _v16)
from test_attention_long_gpu import _group_sizes_long

gpu = pytest.mark.gpu
LENGTHS = [34, 65, 129, 289, 320, 334, 513, 1023, 1024]
D0, HEADS0 = 128, 2
UNIT = {F32: 4, F16: 2, BF16: 2}
MODES = (F16, BF16, F32)


def _b_of(N):
    return 1 if N >= 1023 else 2


def _pack(vis):
    """vis bool [S, N] -> uint32 [S, (N + 31) // 32]: key k in bit k & 31 of word k >> 5"""
    S, N = vis.shape
    per = (N + 31) // 32
    bits = np.zeros((S, per * 32), np.uint64)
    bits[:, :N] = vis
    return (bits.reshape(S, per, 32) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def _attn_m(lib, mode, qkv, B, N, D, heads, vis, nq=0, causal=0, form=PLAIN, pad=3):
    """vis bool [1, N] (one mask, stride 0) or [B, N] (per sample) -> (rc, bytes [B * N + pad, row_bytes])"""
    words = np.ascontiguousarray(_pack(vis))
    stride = 0 if vis.shape[0] == 1 else words.shape[1]
    row_bytes, unit = {PLAIN: (D * UNIT[mode], UNIT[mode]), E4M3: (D, 1), F16C: (3 * D, 2), SPLIT3: (6 * D, 2)}[form]
    buf = _buffer(B * N + pad, row_bytes, unit)
    rc = lib.lib.arp_op_attention_masked(mode, _fp(qkv), buf.ctypes.data, buf.nbytes, B, N, D, heads, causal, nq, form,
                                         words.ctypes.data_as(C.POINTER(C.c_uint32)), words.size, stride)
    return rc, buf


def _ref_masked(qkv, B, N, D, heads, vis):
    """float64 softmax attention with the hidden keys at -inf; vis bool [B or 1, N]"""
    hd = D // heads
    q, k, v = np.split(qkv.astype(np.float64).reshape(B, N, 3 * D), 3, axis=-1)
    sh = lambda a: a.reshape(B, N, heads, hd).transpose(0, 2, 1, 3)
    q, k, v = sh(q), sh(k), sh(v)
    s = (q @ k.transpose(0, 1, 3, 2)) * hd ** -0.5
    s = np.where(np.broadcast_to(vis, (B, N))[:, None, None, :], s, -np.inf)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    return (p @ v).transpose(0, 2, 1, 3).reshape(B * N, D)


# ---- (a): the exactly solvable inputs, one group assignment per sample ----------------------------------------------------------------------------

def _exact_masked(B, N, D, heads, mode, seed):
    """-> (qkv f32 [B * N, 3 D], a [B, N] group of every token, vis [B, N]).  q = k = 4 H[perm_h[a]], every head with its own Hadamard rows; key 0 alone in
    its group (size 1: never hidden); key N - 1, the key pad keys alias, in a largest group on odd samples"""
    rng = np.random.default_rng(seed)
    sizes = _group_sizes_long(N)
    ids = np.repeat(np.arange(len(sizes)), sizes)
    a = np.empty((B, N), np.int64)
    vis = np.ones((B, N), bool)
    qkv = np.zeros((B, N, 3, heads, 64))
    for b in range(B):
        t = rng.permutation(ids)
        z = int(np.flatnonzero(t == 0)[0])   # group 0 has size 1
        t[z], t[0] = t[0], t[z]
        if b % 2 and N > 2:
            z = int(np.flatnonzero(t[1:] == int(np.argmax(sizes)))[0]) + 1
            t[z], t[N - 1] = t[N - 1], t[z]
        a[b] = t
        even = [gi for gi, s in enumerate(sizes) if s % 2 == 0]
        for gi in even[::2]:
            members = np.flatnonzero(t == gi)   # ascending key indices
            vis[b, members[:len(members) // 2]] = False
        for h in range(heads):
            rows = rng.permutation(64)[t]
            qkv[b, :, 0, h] = qkv[b, :, 1, h] = 4.0 * H64[rows]
    qkv[:, :, 2] = _v16((B, N, heads, 64), mode, rng)
    assert D == heads * 64 and vis[:, 0].all()
    return np.ascontiguousarray(qkv.reshape(B * N, 3 * D), np.float32), a, vis


def _expect_masked(qkv, a, vis, B, N, D, heads):
    """-> (mean [B * N, D] float64, exact [B * N, D] bool, share of rows with a power-of-two visible count)"""
    v = qkv.reshape(B, N, 3, heads, 64)[:, :, 2].astype(np.float64)
    mem = (a[:, :, None] == a[:, None, :]) & vis[:, None, :]   # [B, query, key]
    m = mem.sum(-1)
    assert (m >= 1).all(), "a whole group is hidden"
    mean = np.einsum("bij,bjhd->bihd", mem.astype(np.float64), v) / m[:, :, None, None]
    p2 = _is_pow2(m)
    return mean.reshape(B * N, D), np.repeat(p2.reshape(B * N, 1), D, axis=1), float(p2.mean())


def test_masked_exact_inputs():
    """no GPU: at every length at least 0.75 of the rows have a power-of-two visible count; key 0 is visible, no group is wholly hidden, some key is hidden
    from 65 keys on; the float64 masked softmax is the mean over the visible members to 1e-12; the inputs are 16-bit numbers"""
    for N in LENGTHS:
        B = _b_of(N)
        for mode in (F16, BF16):
            qkv, a, vis = _exact_masked(B, N, D0, HEADS0, mode, 7000 * N)
            assert (_rnd(mode)(qkv) == qkv).all()
            mean, exact, share = _expect_masked(qkv, a, vis, B, N, D0, HEADS0)
            assert share >= 0.75, (N, share)
            assert vis[:, 0].all() and (N < 65 or not vis.all())
            assert np.abs(_ref_masked(qkv, B, N, D0, HEADS0, vis) - mean).max() < 1e-12, N
            assert (mean[exact].astype(np.float32).astype(np.float64) == mean[exact]).all()


def test_pack_is_the_documented_word_format():
    vis = np.zeros((2, 70), bool)
    vis[0, [0, 31, 32, 69]] = True
    vis[1, 5] = True
    w = _pack(vis)
    assert w.shape == (2, 3) and w.dtype == np.uint32
    assert w[0].tolist() == [0x80000001, 1, 1 << 5] and w[1].tolist() == [1 << 5, 0, 0]


# ---- the masks of (b) ------------------------------------------------------------------------------------------------------------------------------

def _mask_suffix(N):
    """the last 64-key block wholly hidden, the one before it hidden from its key 40 on (one block only: hidden from key 20 on)"""
    nkb = (N + 63) // 64
    vis = np.zeros(N, bool)
    vis[:64 * (nkb - 2) + 40 if nkb >= 2 else 20] = True
    return vis


def _mask_interior(N):
    """keys 64 .. 127 hidden: a whole interior block (up to 64 keys: the upper 32 keys of the only block)"""
    vis = np.ones(N, bool)
    vis[64:128] = False
    if N <= 64:
        vis[32:] = False
    return vis


def _mask_scattered(N, seed):
    vis = np.random.default_rng(seed).random(N) < 0.5
    vis[0] = True
    return vis


def test_masks_cover_the_block_cases():
    """no GPU: the suffix mask hides the last block wholly and the one before it partly; the interior mask hides block 1 wholly where it exists"""
    for N in LENGTHS:
        nkb = (N + 63) // 64
        s, i = _mask_suffix(N), _mask_interior(N)
        assert s[0] and i[0] and _mask_scattered(N, N)[0]
        if nkb >= 2:
            assert not s[64 * (nkb - 1):].any()
            prev = s[64 * (nkb - 2):64 * (nkb - 1)]
            assert prev.any() and not prev.all()
            assert not i[64:128].any() and i[:64].all()


# ---- GPU --------------------------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("N", LENGTHS)
def test_masked_attention_exact_inputs(gpu_lib, N):
    """(a), per-sample masks"""
    B, D, heads = _b_of(N), D0, HEADS0
    for mode in MODES:
        qkv, a, vis = _exact_masked(B, N, D, heads, BF16 if mode == BF16 else F16, 7000 * N)
        mean, exact, _ = _expect_masked(qkv, a, vis, B, N, D, heads)
        rc, buf = _attn_m(gpu_lib, mode, qkv, B, N, D, heads, vis)
        gpu_lib.check(rc)
        _check_plain_exact(buf, B * N, mode, mean, exact, f"N={N} mode={mode} (a)")


@gpu
@pytest.mark.parametrize("N", LENGTHS)
def test_masked_attention_random_inputs(gpu_lib, N):
    """(b): three shared masks, then two of them as different per-sample masks"""
    B, D, heads = _b_of(N), D0, HEADS0
    r = _random_qkv(B, N, D, N * 17)
    masks = {"suffix": _mask_suffix(N)[None], "interior": _mask_interior(N)[None], "scattered": _mask_scattered(N, N)[None]}
    if B == 2:
        masks["per sample"] = np.stack([_mask_suffix(N), _mask_scattered(N, N + 1)])
        masks["per sample 2"] = np.stack([_mask_scattered(N, N + 2), _mask_interior(N)])
    for mode in MODES:
        x = _rnd(mode)(r)
        for name, vis in masks.items():
            rc, buf = _attn_m(gpu_lib, mode, r, B, N, D, heads, vis)
            gpu_lib.check(rc)
            _check_plain_random(buf, B * N, mode, _ref_masked(x, B, N, D, heads, vis), f"N={N} mode={mode} mask={name} (b)")


@gpu
@pytest.mark.parametrize("N", LENGTHS)
def test_all_visible_mask_gives_the_unmasked_bits(gpu_lib, N):
    """(c)"""
    B, D, heads = _b_of(N), D0, HEADS0
    r = _random_qkv(B, N, D, N * 19)
    vis = np.ones((1, N), bool)
    for mode in MODES:
        rc, got = _attn_m(gpu_lib, mode, r, B, N, D, heads, vis)
        gpu_lib.check(rc)
        if mode == F32 or N >= 289:
            rc, want = _attn(gpu_lib, mode, 0 if N >= 289 else 1, r, B, N, D, heads, 0)
            gpu_lib.check(rc)
            assert (got == want).all(), f"N={N} mode={mode}: an all-visible mask changes the bits"
        else:   # no unmasked key-blocked launch below 289 keys in the 16-bit modes
            _check_plain_random(got, B * N, mode, _ref_masked(_rnd(mode)(r), B, N, D, heads, vis), f"N={N} mode={mode} all visible")
        rc, per = _attn_m(gpu_lib, mode, r, B, N, D, heads, np.ones((B, N), bool))
        gpu_lib.check(rc)
        assert (per == got).all(), f"N={N} mode={mode}: the per-sample stride changes the bits"


@gpu
@pytest.mark.parametrize("N", [129, 334, 513])
def test_f32_masked_rows_are_the_compacted_sequence_bits(gpu_lib, N):
    """(d): per sample, the visible rows of the masked run == the unmasked f32 kernel on the visible rows alone (impl 1 = attn_valu_kernel below 289 keys)"""
    B, D, heads = 2, D0, HEADS0
    r = _random_qkv(B, N, D, N * 23)
    vis = np.stack([_mask_suffix(N), _mask_scattered(N, N + 3)])
    rc, got = _attn_m(gpu_lib, F32, r, B, N, D, heads, vis)
    gpu_lib.check(rc)
    for b in range(B):
        keep = np.flatnonzero(vis[b])
        n2 = len(keep)
        sub = np.ascontiguousarray(r[b * N + keep])
        rc, want = _attn(gpu_lib, F32, 0 if n2 >= 289 else 1, sub, 1, n2, D, heads, 0)
        gpu_lib.check(rc)
        assert (got[b * N + keep] == want[:n2]).all(), f"N={N} sample {b}: visible rows differ from the compacted sequence ({n2} keys)"


@gpu
def test_masked_nq_and_query_split(gpu_lib):
    """(e): nq in {1, 17, N - 1} at 334 keys leaves rows >= nq and the pad rows alone; sample 0 alone (tiles dealt over gridDim.y) and as sample 0 of 64
    (no split) has the same bits"""
    B, N, D, heads = 2, 334, D0, HEADS0
    r = _random_qkv(B, N, D, 5)
    vis = np.stack([_mask_suffix(N), _mask_scattered(N, 9)])
    for mode in MODES:
        rc, full = _attn_m(gpu_lib, mode, r, B, N, D, heads, vis)
        gpu_lib.check(rc)
        for nq in (1, 17, N - 1):
            rc, part = _attn_m(gpu_lib, mode, r, B, N, D, heads, vis, nq=nq)
            gpu_lib.check(rc)
            rows = np.arange(B * N) % N < nq
            assert (part[:B * N][rows] == full[:B * N][rows]).all(), f"mode={mode} nq={nq}: rows < nq differ from the nq = N run"
            assert _is_fill(part[:B * N][~rows], UNIT[mode]) and _is_fill(part[B * N:], UNIT[mode]), f"mode={mode} nq={nq}: a row >= nq was written"
    big = _random_qkv(64, N, D, 6)
    shared = _mask_suffix(N)[None]
    for mode in (F16, BF16):
        rc1, one = _attn_m(gpu_lib, mode, np.ascontiguousarray(big[:N]), 1, N, D, heads, shared)
        rc64, all64 = _attn_m(gpu_lib, mode, big, 64, N, D, heads, shared)
        gpu_lib.check(rc1); gpu_lib.check(rc64)
        assert (one[:N] == all64[:N]).all(), f"mode={mode}: sample 0 differs between the split and the unsplit launch"
        assert _is_fill(all64[64 * N:], 2)


@gpu
def test_masked_attention_refusals(gpu_lib):
    """(f)"""
    D, heads, N = D0, HEADS0, 334
    x = _random_qkv(2, N, D, 1)
    ok = _mask_suffix(N)[None]
    hidden0 = np.stack([_mask_suffix(N), _mask_suffix(N)])
    hidden0[1, 0] = False
    for mode in MODES:
        u = UNIT[mode]
        rc, buf = _attn_m(gpu_lib, mode, x, 2, N, D, heads, hidden0)
        assert rc != 0 and "key 0 is hidden" in gpu_lib.last_error() and "sample 1" in gpu_lib.last_error() and _is_fill(buf, u), f"key 0, mode {mode}"
        rc, buf = _attn_m(gpu_lib, mode, x, 2, N, D, heads, ok, causal=1)
        assert rc != 0 and "causal" in gpu_lib.last_error() and _is_fill(buf, u), f"causal, mode {mode}"
        x5 = _random_qkv(1, 1025, D, 2)
        rc, buf = _attn_m(gpu_lib, mode, x5, 1, 1025, D, heads, np.ones((1, 1025), bool))
        assert rc != 0 and "too long" in gpu_lib.last_error() and _is_fill(buf, u), f"1025 keys, mode {mode}"
        x32 = _random_qkv(2, N, 64, 3)
        rc, buf = _attn_m(gpu_lib, mode, x32, 2, N, 64, 2, ok)
        assert rc != 0 and "head_dim 64" in gpu_lib.last_error() and _is_fill(buf, u), f"head_dim 32, mode {mode}"
    for mode, form, unit in ((F16, E4M3, 1), (BF16, E4M3, 1), (F16, F16C, 2), (F32, SPLIT3, 2)):
        rc, buf = _attn_m(gpu_lib, mode, x, 2, N, D, heads, ok, form=form)
        assert rc != 0 and "plain output only" in gpu_lib.last_error() and _is_fill(buf, unit), f"form {form}, mode {mode}"
