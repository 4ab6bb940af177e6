"""Every attention kernel, instance and output form the product launches, op by op, against float64 (arp_op_attention_forms: everything
tower.h::launch_attention takes; arp_op_qkv_attention: the fused QKV + attention kernel).  Outputs are raw byte buffers pre-filled with a sentinel, so a
row, a segment or a pad row the kernel must leave alone is seen to be left alone.  Both references are plain numpy in float64 and never call the library.

(a) EXACTLY SOLVABLE inputs.  Per (sample, head) token j belongs to a group g(j); its q and k slices are both 4 H[g(j)], H the 64 x 64 Hadamard matrix.  A
score is 1024 inside a group and 0 across groups; after the 1/8 scale a non-member's weight is e^-128 of a member's: 0 in f32, binary16 and bf16, while
a member's is exactly 1.  V holds 16-bit values of magnitude in [0.5, 2), so an output row is the plain mean of the V rows of the VISIBLE members of its
group: sums of a few 16-bit values (exact in f32) and one division by the member count m.  Where m is a power of two the f32 result is exact and the
check is equality of bits; elsewhere any output is accepted that encodes an f32 value within 1.5 f32 ulps of the exact mean (sum * (1.0f / m) and sum / m
with correctly rounded f32 operations both lie inside).  A wrong key slot, pad key, lane, nibble order or segment offset moves a row to another group's
mean: O(1), not a tolerance.  At least half of all (row, head) pairs are held to bit equality; that share is asserted from the inputs alone.

(b) RANDOM inputs against float64 on the rounded operands with the tolerances tests/test_ops_gpu.py::test_attention asserts for the same kernels
(max error 1e-5 f32, 3.5e-3 binary16, 2.5e-2 bf16, mean 2e-3 bf16): a softmax with many non-trivial weights, which (a) cannot give.

The module's two input-builder tests need no GPU and are not marked; every other test carries the gpu mark.

One place where the kernel's documented behaviour, not a blanket rule, is asserted: attn_mfma_kernel's instances of at most 64 tokens compile one
[hi | x4 | dx4] store and write dx4 whatever bit 4 of outc says (attention.h: the second form made them spill); there the dx4 segment under bit 4 must
equal the segment written without it.  Above 64 tokens the dx4 bytes must still hold the caller's fill."""
import ctypes as C

import numpy as np
import pytest

from lowbits import BF16, F16, _bits16, _e4m3_bits, _e4m3_values, _quant_fp4, _unpack_nibbles, _val16
from test_ops_gpu import _attn_ref

gpu = pytest.mark.gpu
F32 = 0
PLAIN, E4M3, F16C, SPLIT3 = 0, 1, 2, 3
FILL = {2: 0x7E5A, 4: 0x7FC0DEAD, 1: 0x7F}   # a binary16 NaN (7e37 in bf16), an f32 NaN, the e4m3 NaN: never a result here
TOL = {F32: 1e-5, BF16: 2.5e-2, F16: 3.5e-3}  # tests/test_ops_gpu.py::test_attention
SWEEP = [1, 2, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 95, 96, 97, 112, 127, 128, 129, 160, 192, 193, 208, 223, 224, 225, 256, 257, 272, 273, 287, 288,
         289, 300]


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _mfma16_has(N):
    """tower.h::launch_attention's switch: the 16-bit MFMA kernel exists for 2, 4, 6, 8, 14 and 18 key tiles"""
    return ((N + 31) // 32) * 2 in (2, 4, 6, 8, 14, 18)


# ---- (a): the exactly solvable inputs ---------------------------------------------------------------------------------------------------------

def _hadamard64():
    h = np.ones((1, 1))
    while h.shape[0] < 64:
        h = np.block([[h, h], [h, -h]])
    return h


H64 = _hadamard64()


def _group_sizes(N):
    """sizes 1, 2, 4, 3, 2, 5 first, then a cycle heavy in powers of two (so that m is 1, 2, 4 or 8 for most rows, causal or not); at most 64 groups"""
    sizes, left = [], N
    cycle = [2, 4, 1, 4, 2, 8, 3] if N <= 100 else [4, 8, 4, 4, 8, 4, 6]
    for s in [1, 2, 4, 3, 2, 5] + cycle * 64:
        if left == 0:
            break
        sizes.append(min(s, left))
        left -= sizes[-1]
    assert len(sizes) <= 64 and sum(sizes) == N
    return sizes


def _groups(B, N, heads, rng):
    """g[b, h, j]: the Hadamard row of token j.  Members of a group are scattered over the sequence (different 16-key tiles, the last tile beside the pad
    keys); key N - 1, the key pad keys alias, is alone in its group on even heads and in the largest group on odd heads."""
    sizes = _group_sizes(N)
    ids = np.repeat(np.arange(len(sizes)), sizes)
    g = np.empty((B, heads, N), np.int64)
    for b in range(B):
        for h in range(heads):
            a = rng.permutation(ids)
            want = 0 if h % 2 == 0 else int(np.argmax(sizes))   # group 0 has size 1
            t = int(np.flatnonzero(a == want)[0])
            a[t], a[N - 1] = a[N - 1], a[t]
            g[b, h] = rng.permutation(64)[a]
    return g


def _v16(shape, mode, rng):
    """random 16-bit values of magnitude in [0.5, 2): 11 significand bits (binary16; also the f32 kernels' V), 8 for bf16"""
    bits = 7 if mode == BF16 else 10
    mag = (1.0 + rng.integers(0, 1 << bits, shape) / float(1 << bits)) * np.where(rng.random(shape) < 0.5, 0.5, 1.0)
    return mag * np.where(rng.random(shape) < 0.5, -1.0, 1.0)


def _exact_qkv(B, N, D, heads, mode, seed, big_head=False):
    rng = np.random.default_rng(seed)
    g = _groups(B, N, heads, rng)
    qkv = np.zeros((B, N, 3, heads, 64))
    qkv[:, :, 0] = qkv[:, :, 1] = 4.0 * H64[g].transpose(0, 2, 1, 3)
    qkv[:, :, 2] = _v16((B, N, heads, 64), mode, rng)
    if big_head:
        qkv[0, :, 2, heads - 1] *= 32.0   # V up to 64: 16 x that saturates e4m3
    assert D == heads * 64
    return np.ascontiguousarray(qkv.reshape(B * N, 3 * D), np.float32), g


def _exact_expect(v, g, causal):
    """v [B, N, heads, 64] float64, g [B, heads, N] -> (mean [B * N, heads * 64], m [B * N, heads]): the mean of the visible members' V rows"""
    B, N, heads, _ = v.shape
    mem = g[:, :, :, None] == g[:, :, None, :]
    if causal:
        mem &= np.tril(np.ones((N, N), bool))
    m = mem.sum(-1)                                                          # [B, heads, N]
    s = np.einsum("bhij,bjhd->bihd", mem.astype(np.float64), v)              # exact: few terms, multiples of 2^-11
    mean = s / m.transpose(0, 2, 1)[..., None]
    return mean.reshape(B * N, heads * 64), m.transpose(0, 2, 1).reshape(B * N, heads)


def _is_pow2(m):
    return (m & (m - 1)) == 0


def _expect_of(qkv, g, B, N, D, heads, causal):
    v = qkv.reshape(B, N, 3, heads, 64)[:, :, 2].astype(np.float64)
    mean, m = _exact_expect(v, g, causal)
    share = float(np.isin(m, (1, 2, 4, 8)).mean())
    assert share >= 0.5, f"only {share:.2f} of the (row, head) pairs have m in 1, 2, 4, 8"
    return mean, np.repeat(_is_pow2(m), 64, axis=1)


def _cands(mean, exact):
    """f32 values an output element may be: the mean itself where `exact`, else every f32 within 1.5 ulps (of the mean's binade) of it -> (c [5, ...], ok)"""
    f = mean.astype(np.float32)
    c, up, dn = [f], f, f
    for _ in range(2):
        up, dn = np.nextafter(up, np.float32(np.inf)), np.nextafter(dn, np.float32(-np.inf))
        c += [up, dn]
    c = np.stack(c)
    ulp = np.where(mean == 0, 0.0, np.ldexp(1.0, np.frexp(mean)[1] - 24))
    ok = np.abs(c.astype(np.float64) - mean) <= 1.5 * ulp
    ok[1:] &= ~exact
    ok[0] &= ~exact | (f.astype(np.float64) == mean)
    return c, ok


def _assert_member(got, enc, mean, exact, what, keep=None):
    """got == enc(c) for one of the admissible f32 values c (`keep`: a further mask over the candidates)"""
    c, ok = _cands(mean, exact)
    if keep is not None:
        ok = ok & keep(c)
    hit = np.zeros(got.shape, bool)
    for k in range(c.shape[0]):
        hit |= ok[k] & (enc(c[k]) == got)
    if not hit.all():
        r, col = np.argwhere(~hit)[0]
        raise AssertionError(f"{what}: {int((~hit).sum())} of {hit.size} elements are not the exact mean (first: row {r} column {col}, stored "
                             f"{got[r, col]!r}, wanted {enc(c[0])[r, col]!r}, exact row {bool(exact[r, col])}; rows hit: {np.unique(np.argwhere(~hit)[:, 0])[:12]})")


# ---- running the two entries -------------------------------------------------------------------------------------------------------------------

def _buffer(rows, row_bytes, unit):
    return np.full(rows * row_bytes // unit, FILL[unit], {1: np.uint8, 2: np.uint16, 4: np.uint32}[unit]).view(np.uint8).reshape(rows, row_bytes)


def _attn(lib, mode, impl, qkv, B, N, D, heads, causal, nq=0, form=PLAIN, scale=0.0, outc=0, pad=3):
    """-> (rc, bytes [B * N + pad, row_bytes]); the pad rows lie inside the buffer the entry uploads and downloads"""
    row_bytes, unit = {PLAIN: (D * (4 if mode == F32 else 2), 4 if mode == F32 else 2), E4M3: (D, 1), F16C: (3 * D, 2), SPLIT3: (6 * D, 2)}[form]
    buf = _buffer(B * N + pad, row_bytes, unit)
    rc = lib.lib.arp_op_attention_forms(mode, impl, _fp(qkv), buf.ctypes.data, buf.nbytes, B, N, D, heads, causal, nq, form, scale, outc)
    return rc, buf


def _fused(lib, mode, A, W, bias, B, N, K, heads, causal, nq=0, pad=3):
    D = heads * 64
    buf = _buffer(B * N + pad, 2 * D, 2)
    rc = lib.lib.arp_op_qkv_attention(mode, _fp(A), _fp(W), _fp(bias), buf.ctypes.data, buf.nbytes, B, N, K, heads, causal, nq)
    return rc, buf


def _is_fill(part, unit):
    part = np.ascontiguousarray(part)
    return part.size == 0 or (part.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[unit]) == FILL[unit]).all()


def _rnd(mode):
    from conftest import bf16_round
    return {F32: lambda x: x, BF16: bf16_round, F16: lambda x: x.astype(np.float16).astype(np.float32)}[mode]


def _words(buf, mode):
    return buf.view(np.uint32 if mode == F32 else np.uint16)


def _values(buf, mode):
    return buf.view(np.float32).astype(np.float64) if mode == F32 else _val16(buf.view(np.uint16), mode)


def _enc_plain(mode):
    return (lambda c: c.view(np.uint32)) if mode == F32 else (lambda c: _bits16(c, mode))


def _check_plain_exact(buf, rows, mode, mean, exact, what):
    _assert_member(_words(buf[:rows], mode), _enc_plain(mode), mean, exact, what)
    assert _is_fill(buf[rows:], 4 if mode == F32 else 2), f"{what}: rows past B * N were written"


def _check_plain_random(buf, rows, mode, ref, what):
    err = np.abs(_values(buf[:rows], mode) - ref)
    print(f"{what}: max err {err.max():.3e} mean {err.mean():.3e}")
    assert err.max() < TOL[mode], f"{what}: max err {err.max()}"
    if mode == BF16:
        assert err.mean() < 2e-3, f"{what}: mean err {err.mean()}"
    assert _is_fill(buf[rows:], 4 if mode == F32 else 2), f"{what}: rows past B * N were written"


def _check_f16c(buf, plain, rows, N, D, outc, what, mean=None, exact=None):
    """[hi | x4 | dx4] rows against the same kernel's plain binary16 output (and, on exact inputs, dx4 against the exact mean)"""
    hi = buf[:rows, :2 * D].view(np.uint16)
    assert (hi == plain[:rows].view(np.uint16)).all(), f"{what}: the hi segment differs from the plain run's output"
    hv = _val16(hi, F16)
    x4 = _unpack_nibbles(buf[:rows, 2 * D:2 * D + D // 2])   # values: the convert keeps the sign of what rounds to zero, and code 8 is -0 = 0
    assert (x4 == _quant_fp4(2.0 * hv)).all(), f"{what}: x4 is not fp4(2 hi), nibble by nibble"
    dx = buf[:rows, 2 * D + D // 2:]
    if (outc & 4) and N > 64:
        assert _is_fill(dx, 2), f"{what}: bit 4 of outc set, yet the dx4 segment was written"
    elif mean is not None:
        _assert_member(_unpack_nibbles(dx), lambda c: _quant_fp4((c.astype(np.float64) - hv) * 2.0 ** 13), mean, exact, what + " dx4",
                       keep=lambda c: _bits16(c, F16) == hi)
    else:   # random inputs: |v - hi| <= half an ulp of hi, so |dx4| <= fp4(2^12 ulp(hi))
        half = 0.5 * np.maximum(np.ldexp(1.0, np.frexp(hv)[1] - 11), 2.0 ** -24)
        assert (np.abs(_unpack_nibbles(dx)) <= _quant_fp4(half * 2.0 ** 13)).all(), f"{what}: a dx4 code exceeds the rounding it corrects"
    assert _is_fill(buf[rows:], 2), f"{what}: rows past B * N were written"


def _check_e4m3_exact(buf, rows, mean, exact, what):
    from oracle.clip_np import quant_e4m3
    _assert_member(buf[:rows], lambda c: _e4m3_bits(quant_e4m3(16.0 * c.astype(np.float64))), mean, exact, what)
    assert _is_fill(buf[rows:], 1), f"{what}: rows past B * N were written"


def _check_split3(buf, plain32, rows, D, what):
    """(hi, lo, hi) binary16 rows against the same kernel's plain f32 output, bit for bit"""
    out = plain32[:rows].view(np.float32).astype(np.float64)
    hi = out.astype(np.float16)
    lo = (out - hi.astype(np.float64)).astype(np.float16)
    w = buf[:rows].view(np.uint16)
    assert (w[:, :D] == hi.view(np.uint16)).all(), f"{what}: hi != rn16(out)"
    assert (w[:, D:2 * D] == lo.view(np.uint16)).all(), f"{what}: lo != rn16(out - hi)"
    assert (w[:, 2 * D:] == w[:, :D]).all(), f"{what}: the third segment is not hi"
    assert _is_fill(buf[rows:], 2), f"{what}: rows past B * N were written"


def _random_qkv(B, N, D, seed):
    return (np.random.default_rng(seed).standard_normal((B * N, 3 * D)) * 1.5).astype(np.float32)


# ---- the builder itself (no GPU) ---------------------------------------------------------------------------------------------------------------

def test_exact_inputs_softmax_is_the_group_mean():
    """On the exact inputs the float64 softmax attention equals the mean over the visible members of the query's group to 1e-12, and exp(-128) is 0 in f32"""
    assert np.exp(np.float32(-128.0)).astype(np.float32) == 0.0 and np.float32(np.exp(-128.0)) == 0.0
    assert (H64 @ H64.T == 64 * np.eye(64)).all()
    for N in (1, 5, 33, 77, 197, 257, 288):
        for causal in (0, 1):
            for mode in (F16, BF16):
                qkv, g = _exact_qkv(2, N, 128, 2, mode, N + causal)
                assert (_rnd(mode)(qkv) == qkv).all(), "the inputs are not representable in the operand type"
                mean, exact = _expect_of(qkv, g, 2, N, 128, 2, causal)
                assert np.abs(_attn_ref(qkv, 2, N, 128, 2, causal) - mean).max() < 1e-12, (N, causal)
                assert (mean[exact].astype(np.float32).astype(np.float64) == mean[exact]).all(), "a power-of-two mean is not an f32 number"


def test_exact_inputs_cover_the_cases():
    """From the inputs alone: at every length of the sweep at least half of the (row, head) pairs have m in {1, 2, 4, 8}, causal or not; group sizes 1, 2, 3, 4
    and larger occur; members of one group sit in different 16-key tiles; key N - 1 is alone on even heads and in the largest group on odd heads; the
    fused kernel's inputs project to q = k = 4 H[g], v = t + c exactly."""
    for N in SWEEP + list(range(1, 65)):
        qkv, g = _exact_qkv(2, N, 128, 2, F16, N)
        for causal in (0, 1):
            _expect_of(qkv, g, 2, N, 128, 2, causal)   # asserts the share
        sizes = np.array([(g[0, h] == g[0, h, N - 1]).sum() for h in range(2)])
        if N >= 17:
            cnt = np.bincount(np.unique(g[0, 0], return_counts=True)[1])
            assert all(cnt[s] > 0 for s in (1, 2, 3, 4)) and len(cnt) > 5
            assert sizes[0] == 1 and sizes[1] == max(_group_sizes(N))
        if N >= 64:
            big = np.flatnonzero(g[0, 1] == g[0, 1, N - 1])
            assert len(set(big // 16)) > 1
    for mode in (F16, BF16):
        A, W, bias, g = _fused_exact(3, 50, 128, 2, mode, 1)
        proj = A.astype(np.float64) @ W.astype(np.float64).T + bias
        q, k, _ = np.split(proj.reshape(3, 50, 3, 2, 64), 3, axis=2)
        assert (np.abs(q) == 4).all() and (q == k).all()
        assert (np.einsum("bihd,bjhd->bhij", q[:, :, 0], k[:, :, 0]) == 1024 * (g[:, :, :, None] == g[:, :, None, :])).all()


# ---- the 16-bit MFMA kernel, the VALU kernel behind it, every form -----------------------------------------------------------------------------

B0, D0, HEADS0 = 2, 128, 2


@gpu
@pytest.mark.parametrize("N", SWEEP)
def test_attention_16bit_every_length(gpu_lib, N):
    """attn_mfma_kernel<T, NT> (NT = 2, 4, 6, 8, 14, 18) on either side of every instance boundary and 16-key tile edge, causal and not; the lengths without
    an instance (129-192, 225-256, 289 on) take attn_valu_kernel: the plain form must still be right, the e4m3 and [hi | x4 | dx4] forms are refused and
    the buffer keeps its fill."""
    B, D, heads, rows = B0, D0, HEADS0, B0 * N
    for causal in (0, 1):
        for mode in (F16, BF16):
            what = f"N={N} causal={causal} mode={mode}"
            qkv, g = _exact_qkv(B, N, D, heads, mode, 1000 * N + causal)
            mean, exact = _expect_of(qkv, g, B, N, D, heads, causal)
            rc, plain = _attn(gpu_lib, mode, 0, qkv, B, N, D, heads, causal)
            gpu_lib.check(rc)
            _check_plain_exact(plain, rows, mode, mean, exact, what + " plain (a)")
            qb, gb = _exact_qkv(B, N, D, heads, mode, 1000 * N + causal + 7, big_head=True)
            rc, b8 = _attn(gpu_lib, mode, 0, qb, B, N, D, heads, causal, form=E4M3, scale=16.0)
            if _mfma16_has(N):
                gpu_lib.check(rc)
                m8, e8 = _expect_of(qb, gb, B, N, D, heads, causal)
                assert np.abs(16.0 * m8).max() > 448.0
                _check_e4m3_exact(b8, rows, m8, e8, what + " e4m3 (a)")
            else:
                assert rc != 0 and "MFMA kernel only" in gpu_lib.last_error() and _is_fill(b8, 1), what + ": e4m3 without an MFMA instance"
            r = _random_qkv(B, N, D, N * 13 + D + causal)
            ref = _attn_ref(_rnd(mode)(r), B, N, D, heads, causal)
            rc, rplain = _attn(gpu_lib, mode, 0, r, B, N, D, heads, causal)
            gpu_lib.check(rc)
            _check_plain_random(rplain, rows, mode, ref, what + " plain (b)")
            if _mfma16_has(N):
                rc, r8 = _attn(gpu_lib, mode, 0, r, B, N, D, heads, causal, form=E4M3, scale=16.0)
                gpu_lib.check(rc)
                # the kernel's f32 value lies within TOL of ref (the bar above); e4m3 rounds it by at most half a step -- one whole step of 16 ref's binade allows for a binade edge
                v8 = np.abs(16.0 * ref)
                step = np.ldexp(1.0, np.clip(np.frexp(np.maximum(v8, 2.0 ** -9))[1] - 1, -6, 8) - 3)
                assert (np.abs(_e4m3_values(r8[:rows]) - 16.0 * ref) <= 16.0 * TOL[mode] + step).all(), what + " e4m3 (b)"
                assert _is_fill(r8[rows:], 1)
            if mode != F16:
                continue
            full = {}
            for outc in (1, 2, 5, 6):
                rc, bc = _attn(gpu_lib, F16, 0, qkv, B, N, D, heads, causal, form=F16C, outc=outc)
                rc2, rcb = _attn(gpu_lib, F16, 0, r, B, N, D, heads, causal, form=F16C, outc=outc)
                if not _mfma16_has(N):
                    assert rc != 0 and rc2 != 0 and "MFMA kernel only" in gpu_lib.last_error() and _is_fill(bc, 2) and _is_fill(rcb, 2), what + f": outc={outc} without an MFMA instance"
                    continue
                gpu_lib.check(rc); gpu_lib.check(rc2)
                _check_f16c(bc, plain, rows, N, D, outc, what + f" outc={outc} (a)", mean, exact)
                _check_f16c(rcb, rplain, rows, N, D, outc, what + f" outc={outc} (b)")
                full[outc] = (bc, rcb)
            if full:
                for k in (0, 1):
                    assert (full[1][k] == full[2][k]).all() and (full[5][k] == full[6][k]).all(), what + ": outc 1 and 2 give different bytes"
                    if N <= 64:   # the instances of <= 64 tokens write dx4 whatever bit 4 says (see the module docstring): then it must be the right one
                        assert (full[5][k] == full[1][k]).all(), what + ": bit 4 changed the bytes of a <= 64-token instance"


@gpu
@pytest.mark.parametrize("N", SWEEP)
def test_attention_f32_every_length(gpu_lib, N):
    """attn_f32_mfma_kernel (impl 0; 1, 4, 5, 13, 17, 18 tiles) and attn_x3_kernel (impl 3) in both output forms; past 288 tokens launch_attention
    sends the plain form through attn_valu_kernel (2 N 64 f32 of LDS: up to 320 tokens) and refuses (hi, lo, hi)."""
    B, D, heads, rows = B0, D0, HEADS0, B0 * N
    for causal in (0, 1):
        qkv, g = _exact_qkv(B, N, D, heads, F16, 2000 * N + causal)
        mean, exact = _expect_of(qkv, g, B, N, D, heads, causal)
        r = _random_qkv(B, N, D, N * 7 + causal)
        ref = _attn_ref(r, B, N, D, heads, causal)
        for impl in (0, 3):
            what = f"N={N} causal={causal} impl={impl}"
            for x, kind in ((qkv, "a"), (r, "b")):
                rc, plain = _attn(gpu_lib, F32, impl, x, B, N, D, heads, causal)
                gpu_lib.check(rc)
                if kind == "a":
                    _check_plain_exact(plain, rows, F32, mean, exact, what + " plain (a)")
                else:
                    _check_plain_random(plain, rows, F32, ref, what + " plain (b)")
                rc, b3 = _attn(gpu_lib, F32, impl, x, B, N, D, heads, causal, form=SPLIT3)
                if N <= 288:
                    gpu_lib.check(rc)
                    _check_split3(b3, plain, rows, D, what + f" (hi, lo, hi) ({kind})")
                else:
                    assert rc != 0 and "f32-MFMA kernel only" in gpu_lib.last_error() and _is_fill(b3, 2), what + ": (hi, lo, hi) past 288 tokens"


@gpu
@pytest.mark.parametrize("N", [1, 5, 33, 64, 65, 77, 129, 197, 257, 300])
def test_attention_valu_kernel(gpu_lib, N):
    """attn_valu_kernel asked for by name (impl 1), all three operand types; no other output form exists on it"""
    B, D, heads, rows = B0, D0, HEADS0, B0 * N
    for causal in (0, 1):
        for mode in (F32, BF16, F16):
            what = f"N={N} causal={causal} mode={mode} impl=1"
            qkv, g = _exact_qkv(B, N, D, heads, BF16 if mode == BF16 else F16, 3000 * N + causal)
            mean, exact = _expect_of(qkv, g, B, N, D, heads, causal)
            rc, plain = _attn(gpu_lib, mode, 1, qkv, B, N, D, heads, causal)
            gpu_lib.check(rc)
            _check_plain_exact(plain, rows, mode, mean, exact, what + " (a)")
            r = _random_qkv(B, N, D, N * 3 + causal)
            rc, plain = _attn(gpu_lib, mode, 1, r, B, N, D, heads, causal)
            gpu_lib.check(rc)
            _check_plain_random(plain, rows, mode, _attn_ref(_rnd(mode)(r), B, N, D, heads, causal), what + " (b)")
            form, kw = {F32: (SPLIT3, {}), BF16: (E4M3, dict(scale=16.0)), F16: (F16C, dict(outc=1))}[mode]
            rc, b = _attn(gpu_lib, mode, 1, r, B, N, D, heads, causal, form=form, **kw)
            assert rc != 0 and _is_fill(b, 1 if form == E4M3 else 2), what + f": form {form} on the VALU kernel"


@gpu
@pytest.mark.parametrize("N", [197, 257])
def test_attention_query_split_on_and_off(gpu_lib, N):
    """gridDim.y > 1 when B * heads < 128 and there are more than 4 query blocks: B = 1 (split) against B = 70 (not), the rows of sample 0 identical"""
    D, heads = D0, HEADS0
    for mode, form, kw in ((F16, PLAIN, {}), (BF16, PLAIN, {}), (F16, F16C, dict(outc=2)), (F16, F16C, dict(outc=5)), (BF16, E4M3, dict(scale=16.0))):
        for kind in "ab":
            big = _exact_qkv(70, N, D, heads, mode, N)[0] if kind == "a" else _random_qkv(70, N, D, N)
            rc1, one = _attn(gpu_lib, mode, 0, np.ascontiguousarray(big[:N]), 1, N, D, heads, 0, form=form, **kw)
            rc70, all70 = _attn(gpu_lib, mode, 0, big, 70, N, D, heads, 0, form=form, **kw)
            gpu_lib.check(rc1); gpu_lib.check(rc70)
            assert (one[:N] == all70[:N]).all(), f"N={N} mode={mode} form={form} ({kind}): sample 0 differs between the split and the unsplit launch"
        if form == PLAIN:   # and the split launch is right
            qkv, g = _exact_qkv(1, N, D, heads, mode, N + 1)
            mean, exact = _expect_of(qkv, g, 1, N, D, heads, 0)
            rc, plain = _attn(gpu_lib, mode, 0, qkv, 1, N, D, heads, 0)
            gpu_lib.check(rc)
            _check_plain_exact(plain, N, mode, mean, exact, f"N={N} mode={mode} B=1 (a)")


NQ_RUNS = [  # mode, impl, form, kwargs, fill unit
    (F16, 0, PLAIN, {}, 2), (BF16, 0, PLAIN, {}, 2), (F16, 0, F16C, dict(outc=1), 2), (F16, 0, F16C, dict(outc=2), 2), (F16, 0, F16C, dict(outc=5), 2),
    (F16, 0, F16C, dict(outc=6), 2), (F16, 0, E4M3, dict(scale=16.0), 1), (BF16, 0, E4M3, dict(scale=16.0), 1),
    (F32, 0, PLAIN, {}, 4), (F32, 0, SPLIT3, {}, 2), (F32, 3, PLAIN, {}, 4), (F32, 3, SPLIT3, {}, 2),
    (F32, 1, PLAIN, {}, 4), (F16, 1, PLAIN, {}, 2), (BF16, 1, PLAIN, {}, 2),
]


@gpu
@pytest.mark.parametrize("N", [50, 130, 257])
def test_attention_nq_leaves_the_other_rows_alone(gpu_lib, N):
    """nq < N (the class-token-only last block) on every kernel and form: rows < nq bit-equal to the nq = N run, rows >= nq (every segment) still the fill.
    (130 and 257 tokens: attn_x3_kernel's cooperative tail on and off as nq moves; the 16-bit MFMA kernel has an instance at each of the three lengths.)"""
    B, D, heads = B0, D0, HEADS0
    for mode, impl, form, kw, unit in NQ_RUNS:
        if form in (E4M3, F16C) and not _mfma16_has(N):
            continue   # (130 tokens is here for the f32 kernels: these forms exist at lengths with a 16-bit MFMA instance only)
        for causal in (0, 1):
            x = _exact_qkv(B, N, D, heads, BF16 if mode == BF16 else F16, N + causal)[0] if causal else _random_qkv(B, N, D, N)
            rc, full = _attn(gpu_lib, mode, impl, x, B, N, D, heads, causal, form=form, **kw)
            gpu_lib.check(rc)
            for nq in (1, 16, 17, N - 1):
                what = f"N={N} nq={nq} mode={mode} impl={impl} form={form} {kw} causal={causal}"
                rc, part = _attn(gpu_lib, mode, impl, x, B, N, D, heads, causal, nq=nq, form=form, **kw)
                gpu_lib.check(rc)
                rows = np.arange(B * N) % N < nq
                no_dx = form == F16C and (kw["outc"] & 4)
                w = 2 * D + D // 2 if no_dx else part.shape[1]
                assert (part[:B * N][rows][:, :w] == full[:B * N][rows][:, :w]).all(), what + ": rows < nq differ from the nq = N run"
                assert _is_fill(part[:B * N][~rows], unit) and _is_fill(part[B * N:], unit), what + ": a row >= nq was written"


@gpu
def test_attention_f16c_rows_at_the_encoder_geometry(gpu_lib):
    """[hi | x4 | dx4] rows as the f16c encoder launches them twelve times per step: 257 tokens, width 768, 12 heads, outc = 1, 2, 1|4, 2|4.  With outc & 3 == 2
    the entry permutes V's columns inside each head as the encoder's weight loader does; the row that comes out is the unpermuted one."""
    B, N, D, heads = 3, 257, 768, 12
    qkv, g = _exact_qkv(B, N, D, heads, F16, 5)
    mean, exact = _expect_of(qkv, g, B, N, D, heads, 0)
    r = _random_qkv(B, N, D, 6)
    rc, plain = _attn(gpu_lib, F16, 0, qkv, B, N, D, heads, 0)
    gpu_lib.check(rc)
    _check_plain_exact(plain, B * N, F16, mean, exact, "encoder geometry plain (a)")
    rc, rplain = _attn(gpu_lib, F16, 0, r, B, N, D, heads, 0)
    gpu_lib.check(rc)
    _check_plain_random(rplain, B * N, F16, _attn_ref(_rnd(F16)(r), B, N, D, heads, 0), "encoder geometry plain (b)")
    got = {}
    for outc in (1, 2, 5, 6):
        rc, a = _attn(gpu_lib, F16, 0, qkv, B, N, D, heads, 0, form=F16C, outc=outc)
        gpu_lib.check(rc)
        _check_f16c(a, plain, B * N, N, D, outc, f"encoder geometry outc={outc} (a)", mean, exact)
        rc, b = _attn(gpu_lib, F16, 0, r, B, N, D, heads, 0, form=F16C, outc=outc)
        gpu_lib.check(rc)
        _check_f16c(b, rplain, B * N, N, D, outc, f"encoder geometry outc={outc} (b)")
        got[outc] = (a, b)
    for k in (0, 1):
        assert (got[1][k] == got[2][k]).all() and (got[5][k] == got[6][k]).all()


# ---- the fused QKV + attention kernel ----------------------------------------------------------------------------------------------------------

def _signed_perm(rng, scale=1.0):
    p = np.zeros((64, 64))
    p[np.arange(64), rng.permutation(64)] = np.where(rng.random(64) < 0.5, -scale, scale)
    return p


def _fused_exact(B, N, K, heads, mode, seed):
    """The exact inputs one step back, so that the projection is exact too (K >= 128).  Activation row j = [H[g(j)] | t_j | u_j]: t_j 64 random 16-bit
    values, u_j K - 128 more that meet zero weights only.  Head h: W_q = W_k = [4 P_h | 0 | 0], W_v = [0 | S_h | 0] with P_h, S_h signed permutation
    matrices of its own (a signed permutation keeps H's rows orthogonal, and a head that took another head's q or k weights would see scores that are
    neither 0 nor 1024); bias 0 for q and k, a 16-bit vector c_h for v.  Every product has one non-zero term: q = k = 4 P_h H[g(j)], v = S_h t_j + c_h
    exactly in f32, which the kernel then rounds to the operand type -- as the reference does.  All heads of a sample share its groups."""
    rng = np.random.default_rng(seed)
    D = heads * 64
    g1 = _groups(B, N, 1, rng)
    g = np.repeat(g1, heads, axis=1)
    A = np.zeros((B, N, K))
    A[:, :, :64] = H64[g1[:, 0]]
    A[:, :, 64:] = _v16((B, N, K - 64), mode, rng)
    W = np.zeros((3, heads, 64, K))
    bias = np.zeros((3, heads, 64))
    for h in range(heads):
        W[0, h, :, :64] = W[1, h, :, :64] = _signed_perm(rng, 4.0)
        W[2, h, :, 64:128] = _signed_perm(rng)
        bias[2, h] = _v16(64, mode, rng)
    f32 = lambda a, *s: np.ascontiguousarray(a.reshape(*s), np.float32)
    return f32(A, B * N, K), f32(W, 3 * D, K), f32(bias, 3 * D), g


def _fused_expect(A, W, bias, g, B, N, heads, mode, causal):
    D = heads * 64
    proj = A.astype(np.float64) @ W.astype(np.float64).T + bias          # exact: one non-zero term per product
    v = _val16(_bits16(proj[:, 2 * D:], mode), mode).reshape(B, N, heads, 64)
    mean, m = _exact_expect(v, g, causal)
    share = float(np.isin(m, (1, 2, 4, 8)).mean())
    assert share >= 0.5, f"only {share:.2f} of the (row, head) pairs have m in 1, 2, 4, 8"
    return mean, np.repeat(_is_pow2(m), 64, axis=1)


def _fused_random(B, N, K, heads, mode, seed, causal):
    """Random operands for which the projection is EXACT in f32, so that "q | k | v rounded to the operand type" is one well-defined set of numbers for the
    kernel and the reference alike: A on the grid 2^-3 within +-4, W and the bias on the grid 2^-10, |W| <= 192 / K -- every product is a multiple of 2^-13
    and a row's sum stays below 2^10, 23 bits.  (Rounded from an f32 sum that merely approximates the fp64 one, ~2e-4 of the bf16 q | k | v values fall on
    the other side of a rounding boundary, and one such V element under a peaked softmax is an output error of a whole bf16 ulp that neither side made.)
    The scales give q | k | v the standard deviation 1.5 of test_ops_gpu.py::test_attention's inputs, which its tolerances belong to."""
    rng = np.random.default_rng(seed)
    D = heads * 64
    A = (np.clip(np.round(rng.standard_normal((B * N, K)) * 8.0), -32, 32) / 8.0).astype(np.float32)
    wmax = np.floor(192.0 / K * 1024.0)
    W = (np.clip(np.round(rng.standard_normal((3 * D, K)) * np.sqrt(2.0 / K) * 1024.0), -wmax, wmax) / 1024.0).astype(np.float32)
    bias = (np.round(rng.standard_normal(3 * D) * 0.5 * 1024.0) / 1024.0).astype(np.float32)
    rnd = _rnd(mode)
    proj = rnd(A).astype(np.float64) @ rnd(W).astype(np.float64).T + bias
    assert (proj.astype(np.float32).astype(np.float64) == proj).all()
    ref = _attn_ref(_val16(_bits16(proj, mode), mode), B, N, D, heads, causal)   # q | k | v rounded to the operand type, as the kernel rounds them
    return A, W, bias, ref


def _check_fused(lib, mode, B, N, K, heads, causal, nq, seed, kinds, pad=3):
    what = f"fused mode={mode} B={B} N={N} K={K} heads={heads} causal={causal} nq={nq}"
    rows = np.arange(B * N) % N < (nq or N)
    for kind in kinds:
        if kind == "a":
            A, W, bias, g = _fused_exact(B, N, K, heads, mode, seed)
            mean, exact = _fused_expect(A, W, bias, g, B, N, heads, mode, causal)
        else:
            A, W, bias, ref = _fused_random(B, N, K, heads, mode, seed, causal)
        rc, buf = _fused(lib, mode, A, W, bias, B, N, K, heads, causal, nq, pad)
        lib.check(rc)
        out = buf[:B * N]
        if kind == "a":
            _assert_member(out[rows].view(np.uint16), _enc_plain(mode), mean[rows], exact[rows], what + " (a)")
        else:
            err = np.abs(_val16(out[rows].view(np.uint16), mode) - ref[rows])
            print(f"{what} (b): max err {err.max():.3e} mean {err.mean():.3e}")
            assert err.max() < TOL[mode] and (mode != BF16 or err.mean() < 2e-3), what + f" (b): max err {err.max()} mean {err.mean()}"
        assert _is_fill(out[~rows], 2), what + ": a row >= nq was written"
        assert _is_fill(buf[B * N:], 2), what + ": rows past B * N were written"


@gpu
@pytest.mark.parametrize("N", range(1, 65))
def test_fused_qkv_attention_every_length(gpu_lib, N):
    """qkv_attn_kernel at every length it accepts, causal and not: one full frame tile and a one-frame tile.  Below 32 tokens the pad keys of a frame
    are the NEXT frame's rows in LDS; on the exact inputs a pad key let through joins some group of the query's head at full weight."""
    for causal in (0, 1):
        for mode in (F16, BF16):
            _check_fused(gpu_lib, mode, 256 // N + 1, N, 128, 1, causal, 0, N * 2 + causal, "ab")


@gpu
@pytest.mark.parametrize("heads", [1, 2, 12])
@pytest.mark.parametrize("K", [64, 128, 768])
def test_fused_qkv_attention_shapes(gpu_lib, K, heads):
    """50 tokens (ViT-B/32) over the K loop's lengths (one K-tile, two, twelve), head counts, frame counts around the 5-frame tile, all rows or the class row"""
    for B in (1, 4, 5, 6, 37):
        for nq in (1, 50):
            for mode, causal in ((F16, 0), (BF16, 0), (F16, 1)):
                _check_fused(gpu_lib, mode, B, 50, K, heads, causal, nq, K + heads + B, "b" if K == 64 else "ab")


@gpu
def test_fused_qkv_attention_tile_walk(gpu_lib):
    """More frame tiles than one L2 group and a ragged last group: 87 frames = 18 tiles of 5 (the last one of 2 frames) in groups of 8, 8 and 2, 3 heads"""
    for mode in (F16, BF16):
        _check_fused(gpu_lib, mode, 87, 50, 128, 3, 0, 0, 87, "ab", pad=40)


@gpu
def test_fused_qkv_attention_refusals(gpu_lib):
    for N, K in ((65, 128), (50, 96)):
        A, W, bias, _ = _fused_random(2, N, K, 1, F16, 1, 0)
        rc, buf = _fused(gpu_lib, F16, A, W, bias, 2, N, K, 1, 0)
        assert rc != 0 and "unsupported shape" in gpu_lib.last_error() and _is_fill(buf, 2), f"N={N} K={K}"
