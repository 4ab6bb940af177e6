"""The backward products of the two trainers, one kernel at a time against float64: the split-K reduce that finishes every one of them
(dtops.h: the narrow and the 4-wide kernel, three output types, bias / tanh / ReLU / residual / strided output / alpha), the NN dX kernel of the
fine-tune head (gemm_tn.hip::gemm_nn_kernel: ragged M, separate operand strides, slabs + reduce into a strided, possibly 16-bit output) and
the TN weight-gradient kernels with the operand strides the policy step passes (ldb = the [hi | x4 | dx4] row stride).

Operands are pre-rounded to the operand type on the host, so the only device rounding is the output's.  Every output buffer, the guard rows
behind the last slab and the columns N..ldo are prefilled with FILL, exact in f32 / bf16 / binary16 and far outside every result: an element
that is still FILL was not written, and a guard element that is anything else was.  Every case asserts (1) values within a derived tolerance,
(2) everything finite, (3) guards bit-for-bit as the host left them, (4) a second call returns the same bits (all reductions are fixed-order).

Tolerances (u = 2^-24, the unit roundoff of f32):
  * n exact f32 terms summed in any order: |err| <= n u sum|terms| to first order.  The reduce: S u |alpha| sum_s |part_s| + u |value| (the
    multiplication by alpha).  The GEMMs: the project's per-element form 2e-6 alpha (|A| |B|) + 1e-6 (tests/test_ops_gpu.py::test_gemm_tn).
  * ReLU and tanh are 1-Lipschitz: the bound of their input carries through.  A bias or residual addition adds one rounding, u |result|.
  * a 16-bit output adds 1.01 ulp16 |ref| (test_ops_gpu.py::_ulp16), plus 2^-25 absolute for binary16 (its subnormal spacing is 2^-24).
  * the device tanhf's own error is the one measured number: see TANHF_MEASURED_ULP.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from lowbits import BF16, F16, _bits16, _val16

pytestmark = pytest.mark.gpu

F32 = 0
ACT_NONE, ACT_RELU, ACT_TANH = 0, 2, 3
TN128, TN256, NN = 0, 1, 2
FILL = np.float32(-4096.0)
GUARD_ROWS = 128       # arp_op_gemm_bwd's slab buffer: ksplit * M * N + 128 * N floats
PAD = 16384.0          # operand padding columns: finite in both 16-bit types; one of them in a product moves it by thousands
U = 2.0 ** -24
ULP16 = {BF16: 2.0 ** -8, F16: 2.0 ** -11}   # half a unit in the last place, relative (test_ops_gpu.py::_ulp16)
ALPHA = float(np.float32(0.3))               # not a power of two: the multiplication rounds

# The device tanhf against np.tanh in float64, in units in the last place of the f32 result, over the pre-activations of every bias + tanh
# case below (4 269 values in [-5.86, 5.75]): measured maximum 1.179 ulp on an MI355X (ROCm 7.0).  Allowed: twice that, 2.36 ulp (the cap is 16).
TANHF_MEASURED_ULP = 1.18
TANHF_ALLOWED_ULP = min(2.0 * TANHF_MEASURED_ULP, 16.0)


def _fp(a):
    assert a.dtype == np.float32 and a.flags.c_contiguous
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _rnd(x, t):
    """values -> the nearest value of type t (f32 / bf16 / binary16), as float32"""
    x = np.asarray(x, np.float32)
    return x if t == F32 else _val16(_bits16(x, t), t).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _untouched(a):
    return (_bits(a) == _bits(FILL)).all()


def _out_tol(ref, tol, out_type):
    """adds the output's own rounding to a bound on the f32 value"""
    if out_type == F32:
        return tol
    return tol + 1.01 * ULP16[out_type] * np.abs(ref) + (2.0 ** -25 if out_type == F16 else 0.0)


def _check_out(out, ref, tol, N, what):
    """the four-way check's first three parts on an [M, ld] output whose first N columns were to be written"""
    assert np.isfinite(out).all(), what
    assert _untouched(out[:, N:]), f"{what}: columns N..ldo were written"
    got = out[:, :N].astype(np.float64)
    assert np.abs(ref).max() < 2048 and not (got == float(FILL)).any(), f"{what}: an element was not written"
    bad = np.abs(got - ref) > tol
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} outside the bound, worst {float((np.abs(got - ref) / tol).max()):.3g} x tol at {np.argwhere(bad)[0]}"


# ---- the split-K reduce --------------------------------------------------------------------------------------------------------------------

NARROW_S = [1, 2, 3, 4, 5, 12, 13, 16, 17, 31, 33, 63]        # thread groups 0..3, `k + 12 < S` stepping 16
WIDE_S = [64, 65, 79, 80, 112, 113, 128, 129, 257]             # groups 0..15, `k + 48 < S` stepping 64
FORMS = {  # name: (bias, act, resid, strided, alpha)
    "bias_tanh": (True, ACT_TANH, False, False, 1.0),      # image_text_input's forward
    "bias_relu": (True, ACT_RELU, False, False, 1.0),      # ft_gemm's fc1
    "resid_ldo": (False, ACT_NONE, True, True, 1.0),       # ft_gemm_nn into a strided view
    "alpha": (False, ACT_NONE, False, False, ALPHA),       # tn_gemm
}


def _reduce_kernel(M, N, ldo, S):
    """dtops.h::launch_splitk_reduce's choice"""
    return "wide" if (M * N) % 4 == 0 and N % 4 == 0 and ldo % 4 == 0 and S >= 64 else "narrow"


def _reduce_cases():
    cases = []  # (M, N, ldo, S, form)
    for form, (_, _, _, strided, _) in FORMS.items():
        cases += [(9, 20, 24 if strided else 0, S, form) for S in NARROW_S + WIDE_S]   # MN = 180: a partial last block in both kernels
        cases.append((7, 15, 17 if strided else 0, 80, form))                          # N % 4: many slabs through the narrow kernel
        cases.append((8, 16, 17, 80, form))                                            # ldo % 4: narrow again
        cases += [(8, 16, 20, S, form) for S in (80, 257)]                             # wide and strided
    return cases


REDUCE_CASES = _reduce_cases()
_seen = {(_reduce_kernel(M, N, ldo, S), form) for M, N, ldo, S, form in REDUCE_CASES}
assert _seen == {(k, f) for k in ("narrow", "wide") for f in FORMS}, _seen   # every form on both kernels (the output types are crossed below)
assert {S for M, N, ldo, S, _ in REDUCE_CASES if _reduce_kernel(M, N, ldo, S) == "narrow"} >= set(NARROW_S) | {80}
assert {S for M, N, ldo, S, _ in REDUCE_CASES if _reduce_kernel(M, N, ldo, S) == "wide"} == set(WIDE_S)
assert _reduce_kernel(9, 20, 0, 63) == "narrow" and _reduce_kernel(8, 16, 20, 80) == "wide" and _reduce_kernel(8, 16, 17, 80) == "narrow"


@functools.lru_cache(maxsize=None)
def _reduce_problem(M, N, ldo, S, form):
    """inputs, the float64 result and the bound on the f32 value in front of the output's rounding; slabs partly cancelling: random signs,
    magnitudes spread over 2^6, scaled so that the sum stays O(1) (a tanh is not saturated) -- one slab dropped or counted twice moves an
    element by 2^-4 .. 2^2 / sqrt(S), against an f32 bound of about S^1.5 2^-24: seventeen times the bound at the least (S = 257, the
    smallest magnitude), over a hundred times at the median magnitude"""
    use_b, act, use_r, _, alpha = FORMS[form]
    rng = np.random.default_rng([M, N, ldo, S, sorted(FORMS).index(form)])
    part = (rng.choice([-1.0, 1.0], (S, M, N)) * 2.0 ** rng.uniform(-3, 3, (S, M, N)) * 0.5 / np.sqrt(S)).astype(np.float32)
    bias = (0.5 * rng.standard_normal(N)).astype(np.float32) if use_b else None
    ld = ldo if ldo else N
    resid = np.full((M, ld), PAD, np.float32) if use_r else None   # (its columns N..ldo must not be read into a result either)
    if use_r:
        resid[:, :N] = rng.standard_normal((M, N)).astype(np.float32)
    p64 = part.astype(np.float64)
    v = alpha * p64.sum(0)
    tol = S * U * abs(alpha) * np.abs(p64).sum(0) + U * np.abs(v)
    pre = None
    if use_b:
        v = v + bias
        tol = tol + U * np.abs(v)
    if act == ACT_RELU:
        v = np.maximum(v, 0.0)
    elif act == ACT_TANH:
        pre = v
        v = np.tanh(v)
        tol = tol + TANHF_ALLOWED_ULP * np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)
    if use_r:
        v = v + resid[:, :N]
        tol = tol + U * np.abs(v)
    for a in (part, bias, resid):
        if a is not None:
            a.setflags(write=False)
    return part, bias, resid, alpha, act, v, tol, pre


def _run_reduce(lib, out_type, part, bias, act, resid, ldo, alpha):
    S, M, N = part.shape
    out = np.full((M, ldo if ldo else N), FILL, np.float32)
    rc = lib.lib.arp_op_splitk_reduce(out_type, _fp(part), S, M, N, _fp(bias) if bias is not None else None, act,
                                      _fp(resid) if resid is not None else None, _fp(out), ldo, alpha)
    lib.check(rc)
    return out


@pytest.mark.parametrize("out_type", [F32, BF16, F16])
@pytest.mark.parametrize("case", REDUCE_CASES, ids=lambda c: "%dx%d-ldo%d-S%d-%s" % c)
def test_splitk_reduce(gpu_lib, case, out_type):
    M, N, ldo, S, form = case
    part, bias, resid, alpha, act, ref, tol, _ = _reduce_problem(*case)
    out = _run_reduce(gpu_lib, out_type, part, bias, act, resid, ldo, alpha)
    _check_out(out, ref, _out_tol(ref, tol, out_type), N, f"{_reduce_kernel(M, N, ldo, S)} reduce {case} -> type {out_type}")
    again = _run_reduce(gpu_lib, out_type, part, bias, act, resid, ldo, alpha)
    assert (_bits(again) == _bits(out)).all(), "a second launch differs"


def test_device_tanhf_error_is_what_the_bound_allows(gpu_lib):
    """The one measured constant: the device tanhf on the pre-activations of every tanh case (a one-slab reduce with alpha = 1 and no bias
    stores tanhf(part) itself) against np.tanh in float64, in f32 units in the last place."""
    pre = np.concatenate([_reduce_problem(*c)[7].ravel() for c in REDUCE_CASES if c[4] == "bias_tanh"]).astype(np.float32)
    out = _run_reduce(gpu_lib, F32, pre.reshape(1, 1, -1), None, ACT_TANH, None, 0, 1.0)[0]
    want = np.tanh(pre.astype(np.float64))
    ulps = np.abs(out - want) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    print(f"device tanhf: max {ulps.max():.3f} ulp over {pre.size} values in [{pre.min():.2f}, {pre.max():.2f}] (allowed {TANHF_ALLOWED_ULP})")
    assert ulps.max() <= TANHF_ALLOWED_ULP


# ---- the backward GEMMs ------------------------------------------------------------------------------------------------------------------

def _strided(a, ld):
    """[rows, cols] -> [rows, ld] with the padding columns filled with PAD"""
    out = np.full((a.shape[0], ld), PAD, np.float32)
    out[:, :a.shape[1]] = a
    return out


def _slices(K, S, bk):
    """the kernels' K-slices: ceil(tiles / S) K-tiles of bk rows each, the last one shorter (possibly empty)"""
    nk = K // bk
    per = -(-nk // S)
    return [(min(s * per, nk) * bk, min((s + 1) * per, nk) * bk) for s in range(S)]


def _run_bwd(lib, kind, mode, out_type, S, A, lda, B, ldb, resid, ldo, M, N, K, alpha, with_slabs):
    out = np.full((M, ldo if ldo else N), FILL, np.float32)
    slabs = np.full(S * M * N + GUARD_ROWS * N, FILL, np.float32) if with_slabs else None
    rc = lib.lib.arp_op_gemm_bwd(kind, mode, out_type, S, _fp(A), lda, _fp(B), ldb, _fp(resid) if resid is not None else None, _fp(out), ldo,
                                 _fp(slabs) if with_slabs else None, M, N, K, alpha)
    return rc, out, slabs


def _check_slabs(slabs, S, M, N, slab_ref, slab_mag, what):
    """the raw slabs against the float64 product of their own K-slice, their sum against the whole product, and the guard rows behind the
    last slab -- the only deterministic witness of a row stored past M: a stray row of slab s otherwise lands in slab s + 1"""
    assert np.isfinite(slabs).all(), what
    assert _untouched(slabs[S * M * N:]), f"{what}: the guard rows behind the last slab were written"
    got = slabs[:S * M * N].reshape(S, M, N).astype(np.float64)
    assert not (got == float(FILL)).any(), f"{what}: a slab element was not written"
    tol = 2e-6 * slab_mag + 1e-6
    assert (np.abs(got - slab_ref) <= tol).all(), f"{what}: slab error {float((np.abs(got - slab_ref) / tol).max()):.3g} x tol"
    tol = 2e-6 * slab_mag.sum(0) + 1e-6
    assert (np.abs(got.sum(0) - slab_ref.sum(0)) <= tol).all(), f"{what}: slab sum error {float((np.abs(got.sum(0) - slab_ref.sum(0)) / tol).max()):.3g} x tol"


NN_CASES = [  # M, N, K, S: rows below / at / one past / across the 128-row tile, one to three column tiles, even and ragged K-slices (none empty)
    (1, 128, 64, 1), (5, 256, 128, 2), (127, 128, 128, 1), (128, 128, 192, 3), (129, 256, 64, 1),
    (200, 384, 704, 3),     # slices of 4 / 4 / 3 K-tiles
    (300, 128, 1344, 5),    # slices of 5 / 5 / 5 / 5 / 1 K-tiles
]
NN_FORMS = {  # name: (operand padding (lda - K, ldb - N), 16-bit output, resid, ldo - N, alpha)
    "dense-f32": ((0, 0), False, False, 0, 1.0),
    "strided-f32-resid-ldo": ((8, 72), False, True, 4, 1.0),
    "strided-16-resid-ldo": ((24, 264), True, True, 8, 1.0),
    "dense-16-alpha": ((0, 0), True, False, 0, ALPHA),
    "strided-16": ((8, 8), True, False, 0, 1.0),
}
assert all(all(hi > lo for lo, hi in _slices(K, S, 64)) for _, _, K, S in NN_CASES)


@functools.lru_cache(maxsize=None)
def _nn_problem(case, mode):
    M, N, K, S = case
    rng = np.random.default_rng([M, N, K, S, mode])
    A = _rnd(rng.standard_normal((M, K)), mode)
    B = _rnd(rng.standard_normal((K, N)) * 0.25, mode)
    resid = rng.standard_normal((M, N)).astype(np.float32)
    a64, b64 = A.astype(np.float64), B.astype(np.float64)
    slab_ref = np.stack([a64[:, lo:hi] @ b64[lo:hi] for lo, hi in _slices(K, S, 64)])
    slab_mag = np.stack([np.abs(a64[:, lo:hi]) @ np.abs(b64[lo:hi]) for lo, hi in _slices(K, S, 64)])
    for a in (A, B, resid, slab_ref, slab_mag):
        a.setflags(write=False)
    return A, B, resid, slab_ref, slab_mag


@pytest.mark.parametrize("form", list(NN_FORMS))
@pytest.mark.parametrize("mode", [BF16, F16])
@pytest.mark.parametrize("case", NN_CASES, ids=lambda c: "%dx%dx%d-S%d" % c)
def test_gemm_nn(gpu_lib, case, mode, form):
    """dX = alpha * dY . W (+ resid) on a weight as it lies in memory, the way arp_ft.hip::ft_gemm_nn runs it: slabs [S][M][N], then the reduce
    into a strided f32 or 16-bit output."""
    M, N, K, S = case
    (pa, pb), out16, use_r, po, alpha = NN_FORMS[form]
    A, B, resid, slab_ref, slab_mag = _nn_problem(case, mode)
    lda, ldb, ldo, out_type = K + pa, N + pb, (N + po if po else 0), (mode if out16 else F32)
    As, Bs = _strided(A, lda), _strided(B, ldb)
    rs = _strided(resid, N + po) if use_r else None
    what = f"gemm_nn {case} mode {mode} {form}"
    rc, out, slabs = _run_bwd(gpu_lib, NN, mode, out_type, S, As, lda, Bs, ldb, rs, ldo, M, N, K, alpha, True)
    gpu_lib.check(rc)
    _check_slabs(slabs, S, M, N, slab_ref, slab_mag, what)
    v = alpha * slab_ref.sum(0)
    mag = slab_mag.sum(0)
    tol = 2e-6 * alpha * mag + 1e-6 + S * U * alpha * np.abs(slab_ref).sum(0) + U * np.abs(v)
    if use_r:
        v = v + resid
        tol = tol + U * np.abs(v)
    _check_out(out, v, _out_tol(v, tol, out_type), N, what)
    rc, out2, slabs2 = _run_bwd(gpu_lib, NN, mode, out_type, S, As, lda, Bs, ldb, rs, ldo, M, N, K, alpha, True)
    assert rc == 0 and (_bits(out2) == _bits(out)).all() and (_bits(slabs2) == _bits(slabs)).all(), f"{what}: a second call differs"


TN_STRIDED_CASES = [  # M, N, K, S, kind: one per kernel form, from test_ops_gpu.py::test_gemm_tn
    (256, 384, 704, 3, TN128), (256, 512, 704, 1, TN256), (768, 768, 2112, 16, TN256),   # (the last: per-XCD slice placement)
]


@pytest.mark.parametrize("mode", [BF16, F16])
@pytest.mark.parametrize("case", TN_STRIDED_CASES, ids=lambda c: "%dx%dx%d-S%d-kind%d" % c)
def test_gemm_tn_with_operand_strides(gpu_lib, case, mode):
    """dW = alpha * A^T B with lda = M + 8 and ldb = N + 264 -- the policy step passes ldb = the [hi | x4 | dx4] row stride of its adapter operands --
    the padding columns filled with PAD; the direct form (alpha in the kernel) and slabs + reduce (alpha there), as arp_dt.hip::tn_gemm."""
    M, N, K, S, kind = case
    rng = np.random.default_rng([M, N, K, S, kind, mode])
    A = _rnd(rng.standard_normal((K, M)), mode)
    B = _rnd(rng.standard_normal((K, N)) * 0.25, mode)
    lda, ldb, ldo, alpha = M + 8, N + 264, N + 4, 0.5
    As, Bs = _strided(A, lda), _strided(B, ldb)
    a64, b64 = A.astype(np.float64), B.astype(np.float64)
    what = f"gemm_tn {case} mode {mode}"
    rc, out, slabs = _run_bwd(gpu_lib, kind, mode, F32, S, As, lda, Bs, ldb, None, ldo, M, N, K, alpha, S > 1)
    gpu_lib.check(rc)
    sl = _slices(K, S, 32 if kind == TN256 else 64)
    slab_ref = np.stack([a64[lo:hi].T @ b64[lo:hi] for lo, hi in sl])
    slab_mag = np.stack([np.abs(a64[lo:hi]).T @ np.abs(b64[lo:hi]) for lo, hi in sl])
    if S > 1:
        _check_slabs(slabs, S, M, N, slab_ref, slab_mag, what)
    v = alpha * slab_ref.sum(0)
    tol = 2e-6 * alpha * slab_mag.sum(0) + 1e-6
    if S > 1:
        tol = tol + S * U * alpha * np.abs(slab_ref).sum(0) + U * np.abs(v)
    _check_out(out, v, tol, N, what)
    rc, out2, slabs2 = _run_bwd(gpu_lib, kind, mode, F32, S, As, lda, Bs, ldb, None, ldo, M, N, K, alpha, S > 1)
    assert rc == 0 and (_bits(out2) == _bits(out)).all() and (S == 1 or (_bits(slabs2) == _bits(slabs)).all()), f"{what}: a second call differs"


REFUSALS = [  # what, kind, mode, S, M, N, K, lda - rows' width, ldb - N, ldo
    ("tn: N % 128", TN128, F16, 1, 128, 192, 64, 0, 0, 0),
    ("tn: M % 128", TN128, F16, 1, 192, 128, 64, 0, 0, 0),
    ("tn: K % 64", TN128, F16, 1, 128, 128, 96, 0, 0, 0),
    ("tn: lda % 8", TN128, F16, 1, 128, 128, 64, 4, 0, 0),
    ("tn: ldb % 8", TN128, F16, 1, 128, 128, 64, 0, 4, 0),
    ("tn: ldo % 4 on the direct path", TN128, F16, 1, 128, 128, 64, 0, 0, 130),
    ("tn: a 32-bit operand mode", TN128, F32, 1, 128, 128, 64, 0, 0, 0),
    ("tn256: M % 256", TN256, BF16, 1, 384, 256, 64, 0, 0, 0),
    ("tn256: N % 256", TN256, BF16, 1, 256, 384, 64, 0, 0, 0),
    ("tn256: a 32-bit operand mode", TN256, F32, 1, 256, 256, 64, 0, 0, 0),
    ("nn: N % 128", NN, F16, 1, 40, 192, 64, 0, 0, 0),
    ("nn: K % 64", NN, F16, 1, 40, 128, 96, 0, 0, 0),
    ("nn: lda % 8", NN, F16, 1, 40, 128, 64, 4, 0, 0),
    ("nn: ldb % 8", NN, F16, 1, 40, 128, 64, 0, 4, 0),
    ("nn: a 32-bit operand mode", NN, F32, 1, 40, 128, 64, 0, 0, 0),
]


@pytest.mark.parametrize("case", REFUSALS, ids=lambda c: c[0])
def test_launchers_refuse_what_they_cannot_run(gpu_lib, case):
    """one call per stated requirement of launch_gemm_tn / launch_gemm_nn: non-zero, and `out` comes back from the device as it went up"""
    what, kind, mode, S, M, N, K, pa, pb, ldo = case
    rows_a, cols_a = (M, K) if kind == NN else (K, M)
    A = np.ones((rows_a, cols_a + pa), np.float32)
    B = np.ones((K, N + pb), np.float32)
    rc, out, _ = _run_bwd(gpu_lib, kind, mode, F32, S, A, cols_a + pa, B, N + pb, None, ldo, M, N, K, 1.0, False)
    assert rc != 0 and gpu_lib.last_error(), what
    assert _untouched(out), what
