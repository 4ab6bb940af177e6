"""The key-blocked attention kernels (csrc/attention_long.h: attn_long_kernel<f16 | bf16>, attn_long_f32_kernel) for 289 .. 1024 keys at head_dim 64,
through arp_op_attention_forms -- so through tower.h::launch_attention -- on sentinel-prefilled byte buffers, with the builders and checks of
tests/test_attention_forms_gpu.py.

(a) EXACTLY SOLVABLE inputs (that module's docstring): a score is 1024 inside a group and 0 across groups, so softmax is the mean of the visible members'
V rows.  Under the ONLINE softmax of a key-blocked kernel this stays exact: while no member of the query's group has been seen the running maximum is 0
and every key so far carries weight 1; at the first block with a member the maximum moves to 128 (1024 / 8) and the rescale factor e^-128 is 0 in f32, which
wipes the accumulated sum and row; from then on a rescale factor is exactly 1, members weigh exactly 1 and non-members exactly 0.  Bit equality where the
member count is a power of two, the 1.5-ulp interval of the one division elsewhere.
(b) RANDOM inputs against float64 at tests/test_ops_gpu.py::test_attention's bars (1e-5 f32, 3.5e-3 binary16, 2.5e-2 bf16 and its 2e-3 mean).

Lengths: the issue's list plus 64 j - 1, 64 j, 64 j + 1 for the 16-bit kernel's key block of 64 (the f32 kernel's block is 128, a subset).  B = 2, D = 128,
2 heads; B = 1 at 1023 and 1024."""
import numpy as np
import pytest

from lowbits import BF16, F16
from test_attention_forms_gpu import (E4M3, F16C, F32, H64, SPLIT3, _attn, _check_plain_exact, _check_plain_random, _exact_expect, _is_fill, _is_pow2,
                                      _random_qkv, _rnd, _v16)
from test_ops_gpu import _attn_ref

gpu = pytest.mark.gpu
KB = 64
LENGTHS = sorted(set([289, 290, 303, 304, 305, 319, 320, 321, 384, 385, 512, 513, 514, 544, 545, 1023, 1024]) |
                 {KB * j + d for j in range(5, 17) for d in (-1, 0, 1) if 289 <= KB * j + d <= 1024})
D0, HEADS0 = 128, 2
UNIT = {F32: 4, F16: 2, BF16: 2}


def _b_of(N):
    return 1 if N >= 1023 else 2


# test_attention_forms_gpu.py's builder stops at 333 tokens (64 Hadamard rows, its group sizes); restated here with larger groups.  Sizes 1, 2, 4, 3, 2, 5
# first, then a cycle of 16, 32, 16, 8, 32, 16, 12: at most 64 groups up to 1024 tokens, and without a causal mask over 80 % of the rows have a power-of-two
# member count.  Sums of at most 32 values that are multiples of 2^-11 below 2 are exact in f32.
def _group_sizes_long(N):
    sizes, left = [], N
    for s in [1, 2, 4, 3, 2, 5] + [16, 32, 16, 8, 32, 16, 12] * 9:
        if left == 0:
            break
        sizes.append(min(s, left))
        left -= sizes[-1]
    assert len(sizes) <= 64 and sum(sizes) == N
    return sizes


def _exact_qkv(B, N, D, heads, mode, seed):
    """q = k = 4 H[g(j)], V random 16-bit values; members of a group scattered over the sequence (so over the key blocks); key N - 1, the key pad keys alias,
    alone in its group on even heads and in a largest group on odd heads"""
    rng = np.random.default_rng(seed)
    sizes = _group_sizes_long(N)
    ids = np.repeat(np.arange(len(sizes)), sizes)
    g = np.empty((B, heads, N), np.int64)
    for b in range(B):
        for h in range(heads):
            a = rng.permutation(ids)
            want = 0 if h % 2 == 0 else int(np.argmax(sizes))
            t = int(np.flatnonzero(a == want)[0])
            a[t], a[N - 1] = a[N - 1], a[t]
            g[b, h] = rng.permutation(64)[a]
    qkv = np.zeros((B, N, 3, heads, 64))
    qkv[:, :, 0] = qkv[:, :, 1] = 4.0 * H64[g].transpose(0, 2, 1, 3)
    qkv[:, :, 2] = _v16((B, N, heads, 64), mode, rng)
    assert D == heads * 64
    return np.ascontiguousarray(qkv.reshape(B * N, 3 * D), np.float32), g


def _expect_of(qkv, g, B, N, D, heads, causal):
    v = qkv.reshape(B, N, 3, heads, 64)[:, :, 2].astype(np.float64)
    mean, m = _exact_expect(v, g, causal)
    share = float(_is_pow2(m).mean())
    # (under the causal mask the k-th member of a group sees k members: 5 of 16 and 6 of 32 counts are powers of two, so about a quarter of the rows)
    assert share >= (0.25 if causal else 0.8), f"only {share:.2f} of the (row, head) pairs have a power-of-two member count"
    return mean, np.repeat(_is_pow2(m), 64, axis=1)


def test_exact_inputs_at_long_lengths():
    """no GPU: on the restated inputs the float64 softmax attention is the mean over the visible members to 1e-12, the inputs are 16-bit numbers, and
    a group's members lie in more than one 64-key block"""
    for N in (289, 513, 1024):
        for causal in (0, 1):
            for mode in (F16, BF16):
                qkv, g = _exact_qkv(1, N, 128, 2, mode, N + causal)
                assert (_rnd(mode)(qkv) == qkv).all()
                mean, exact = _expect_of(qkv, g, 1, N, 128, 2, causal)
                assert np.abs(_attn_ref(qkv, 1, N, 128, 2, causal) - mean).max() < 1e-12, (N, causal)
                assert (mean[exact].astype(np.float32).astype(np.float64) == mean[exact]).all()
        big = np.flatnonzero(g[0, 1] == g[0, 1, N - 1])
        assert len(set(big // KB)) > 1


def test_lengths_cover_every_key_block_edge():
    """no GPU: the sweep holds the issue's lengths and both sides of every multiple of the key block in range"""
    for j in range(5, 17):
        for d in (-1, 0, 1):
            n = KB * j + d
            assert n > 1024 or n in LENGTHS
    assert {289, 290, 303, 304, 305, 513, 514, 544, 545, 1023, 1024} <= set(LENGTHS)


@gpu
@pytest.mark.parametrize("N", LENGTHS)
def test_long_attention_every_length(gpu_lib, N):
    B, D, heads = _b_of(N), D0, HEADS0
    rows = B * N
    for causal in (0, 1):
        r = _random_qkv(B, N, D, N * 11 + causal)
        for mode in (F16, BF16, F32):
            what = f"N={N} causal={causal} mode={mode}"
            qkv, g = _exact_qkv(B, N, D, heads, BF16 if mode == BF16 else F16, 4000 * N + causal)
            mean, exact = _expect_of(qkv, g, B, N, D, heads, causal)
            rc, plain = _attn(gpu_lib, mode, 0, qkv, B, N, D, heads, causal)
            gpu_lib.check(rc)
            _check_plain_exact(plain, rows, mode, mean, exact, what + " (a)")
            rc, rplain = _attn(gpu_lib, mode, 0, r, B, N, D, heads, causal)
            gpu_lib.check(rc)
            _check_plain_random(rplain, rows, mode, _attn_ref(_rnd(mode)(r), B, N, D, heads, causal), what + " (b)")


@gpu
def test_long_attention_nq_leaves_the_other_rows_alone(gpu_lib):
    """nq in {1, 16, 17, N - 1} at 513 keys: rows < nq are the nq = N run's bits, rows >= nq and the pad rows behind the last row keep the fill"""
    B, N, D, heads = 2, 513, D0, HEADS0
    for mode in (F16, BF16, F32):
        for causal in (0, 1):
            x = _exact_qkv(B, N, D, heads, BF16 if mode == BF16 else F16, N + causal)[0] if causal else _random_qkv(B, N, D, N)
            rc, full = _attn(gpu_lib, mode, 0, x, B, N, D, heads, causal)
            gpu_lib.check(rc)
            for nq in (1, 16, 17, N - 1):
                what = f"N={N} nq={nq} mode={mode} causal={causal}"
                rc, part = _attn(gpu_lib, mode, 0, x, B, N, D, heads, causal, nq=nq)
                gpu_lib.check(rc)
                rows = np.arange(B * N) % N < nq
                assert (part[:B * N][rows] == full[:B * N][rows]).all(), what + ": rows < nq differ from the nq = N run"
                assert _is_fill(part[:B * N][~rows], UNIT[mode]) and _is_fill(part[B * N:], UNIT[mode]), what + ": a row >= nq was written"


@gpu
def test_long_attention_query_split_on_and_off(gpu_lib):
    """B * heads = 2 deals the 64-query tiles over gridDim.y; 64 samples x 2 heads = 128 does not.  Sample 0's rows: the same bits."""
    N, D, heads = 289, D0, HEADS0
    for mode in (F16, BF16):
        for kind in "ab":
            for causal in (0, 1):
                big = _exact_qkv(64, N, D, heads, mode, N + causal)[0] if kind == "a" else _random_qkv(64, N, D, N + causal)
                rc1, one = _attn(gpu_lib, mode, 0, np.ascontiguousarray(big[:N]), 1, N, D, heads, causal)
                rc64, all64 = _attn(gpu_lib, mode, 0, big, 64, N, D, heads, causal)
                gpu_lib.check(rc1); gpu_lib.check(rc64)
                assert (one[:N] == all64[:N]).all(), f"mode={mode} ({kind}) causal={causal}: sample 0 differs between the split and the unsplit launch"
                if kind == "b":
                    _check_plain_random(all64, 64 * N, mode, _attn_ref(_rnd(mode)(big), 64, N, D, heads, causal), f"B=64 mode={mode} causal={causal}")


@gpu
def test_long_attention_repeatable_and_independent_of_placement(gpu_lib):
    """two launches give the same bits; a sample's rows are the same bits alone (B = 1) and as sample 1 of B = 2"""
    D, heads = D0, HEADS0
    for N in (339, 513):
        for mode in (F16, BF16, F32):
            for causal in (0, 1):
                x = _random_qkv(2, N, D, N + 5 * causal)
                rc, a = _attn(gpu_lib, mode, 0, x, 2, N, D, heads, causal)
                gpu_lib.check(rc)
                rc, b = _attn(gpu_lib, mode, 0, x, 2, N, D, heads, causal)
                gpu_lib.check(rc)
                assert (a == b).all(), f"N={N} mode={mode} causal={causal}: two launches differ"
                rc, one = _attn(gpu_lib, mode, 0, np.ascontiguousarray(x[N:]), 1, N, D, heads, causal)
                gpu_lib.check(rc)
                assert (one[:N] == a[N:2 * N]).all(), f"N={N} mode={mode} causal={causal}: sample 1 of B = 2 differs from the same sample alone"


@gpu
def test_long_attention_refusals(gpu_lib):
    """1025 keys, the e4m3 and [hi | x4 | dx4] forms, and (hi, lo, hi) past 288 keys: an error string, every output byte untouched"""
    D, heads = D0, HEADS0
    x = _random_qkv(1, 1025, D, 1)
    for mode in (F16, BF16, F32):
        rc, buf = _attn(gpu_lib, mode, 0, x, 1, 1025, D, heads, 0)
        assert rc != 0 and "too long" in gpu_lib.last_error() and _is_fill(buf, UNIT[mode]), f"1025 keys, mode {mode}"
    x = _random_qkv(2, 513, D, 2)
    for outc in (1, 2, 5, 6):
        rc, buf = _attn(gpu_lib, F16, 0, x, 2, 513, D, heads, 0, form=F16C, outc=outc)
        assert rc != 0 and "MFMA kernel only" in gpu_lib.last_error() and _is_fill(buf, 2), f"outc={outc}"
    for mode in (F16, BF16):
        rc, buf = _attn(gpu_lib, mode, 0, x, 2, 513, D, heads, 0, form=E4M3, scale=16.0)
        assert rc != 0 and "MFMA kernel only" in gpu_lib.last_error() and _is_fill(buf, 1), f"e4m3, mode {mode}"
    for impl in (0, 3):
        rc, buf = _attn(gpu_lib, F32, impl, x, 2, 513, D, heads, 0, form=SPLIT3)
        assert rc != 0 and "f32-MFMA kernel only" in gpu_lib.last_error() and _is_fill(buf, 2), f"(hi, lo, hi), impl {impl}"


@gpu
@pytest.mark.parametrize("N", [257, 288])
def test_dispatch_below_289_still_runs(gpu_lib, N):
    """the LDS-resident kernels keep their lengths: 257 and 288 keys still run and match float64 (their bits are the existing tests' business)"""
    B, D, heads = 2, D0, HEADS0
    for causal in (0, 1):
        r = _random_qkv(B, N, D, N + causal)
        for mode in (F16, BF16, F32):
            rc, buf = _attn(gpu_lib, mode, 0, r, B, N, D, heads, causal)
            gpu_lib.check(rc)
            _check_plain_random(buf, B * N, mode, _attn_ref(_rnd(mode)(r), B, N, D, heads, causal), f"N={N} mode={mode} causal={causal}")


@gpu
def test_f16x3_attention_request_past_288_keys_is_the_f32_kernel(gpu_lib):
    """impl 3 (the f16x3 encoder mode's attention) has no instance past 288 keys and takes the exact-f32 kernel: the same bits as impl 0"""
    B, N, D, heads = 2, 339, D0, HEADS0
    r = _random_qkv(B, N, D, 9)
    rc0, a = _attn(gpu_lib, F32, 0, r, B, N, D, heads, 0)
    rc3, b = _attn(gpu_lib, F32, 3, r, B, N, D, heads, 0)
    gpu_lib.check(rc0); gpu_lib.check(rc3)
    assert (a == b).all()
    _check_plain_random(b, B * N, F32, _attn_ref(r, B, N, D, heads, 0), "impl 3 at 339 keys")


@gpu
@pytest.mark.parametrize("N", [289, 320])
def test_f32_long_kernel_gives_the_valu_kernel_its_bits(gpu_lib, N):
    """f32 sequences of 289 .. 320 keys ran on attn_valu_kernel (impl 1 still asks for it by name) and now take attn_long_f32_kernel (impl 0): the same
    operations in the same order per query, so the same bits -- causal and not, all rows and nq = 17"""
    B, D, heads = 2, D0, HEADS0
    for causal in (0, 1):
        r = _random_qkv(B, N, D, 31 * N + causal)
        for nq in (0, 17):
            rc0, a = _attn(gpu_lib, F32, 0, r, B, N, D, heads, causal, nq=nq)
            rc1, b = _attn(gpu_lib, F32, 1, r, B, N, D, heads, causal, nq=nq)
            gpu_lib.check(rc0); gpu_lib.check(rc1)
            assert (a == b).all(), f"N={N} causal={causal} nq={nq}: attn_long_f32_kernel and attn_valu_kernel differ"
