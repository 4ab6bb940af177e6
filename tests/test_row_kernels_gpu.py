"""The towers' row kernels (csrc/rowops.h, tower.h) and the operand converters (dtops.h, arp_enc.hip), op by op, against float64, in every output form the
product instantiates.  Each entry point runs the product's own launch helper; every output is a byte buffer this module fills with a pattern first, so a
pad column, a segment or a row the kernel must leave alone is seen to be left alone.  The references are plain numpy and never call the library.

ACCEPTANCE RULE of a LayerNorm element (i, j), v its float64 value on the f32 inputs, u = 2^-24:

    delta_ij = 16 u (|xhat_ij w_j| + |b_j| + a_i |w_j|),   a_i = mean_j |x_ij| / sqrt(var_i + eps)

the worst case of the kernel's own f32 arithmetic: at most 16 additions on the longest path of either reduction (2 inside a float4, 8 float4 per lane, 6
shuffle levels), then subtract, two multiplies and an add.  f32 output: |out - v| <= delta.  Narrow outputs (bf16, binary16, e4m3): the stored code is one
the format's round-to-nearest-even, saturating quantiser q (lowbits.quantize, monotone) gives for SOME value of [v - delta, v + delta]:
q(v - delta) <= dec(out) <= q(v + delta) -- no exempt share, no relative slack; saturation and subnormals are q's.  [hi | lo | hi]: hi by the narrow rule,
third segment bitwise the first, |hi + lo - v| <= delta + 2^-11 |lo| + 2^-25.  [hi | x4 (| dx4)]: hi by the narrow rule, x4 == fp4(2 hi) exactly from the
kernel's own hi, fp4((v - delta - hi) 2^13) <= dx4 <= fp4((v + delta - hi) 2^13); in the [hi | x4] form the dx4 bytes keep the fill.

Sums (row_stats, the assemble kernel's strip 0, reward, l2_normalize): (L + 1) u sum |terms|, L the additions on the longest path, stated at each test.
Kernels that only move or round data or add once (text_embed, m3ae_assemble, rows_gather, extract_hi, the operand copies, convert_f16c*, split3) are held to
bit equality.

Largest |out - v| / delta measured on an MI355X over every LayerNorm case of this module (the bar is 1.0; the tests print theirs, `pytest -s`): f32 form
0.175; ln_pre rows of the two assembly kernels 0.173; hi + lo of the [hi | lo | hi] form 0.275 of its own bound.  A numpy f32 restatement of the kernel with
pairwise sums reaches 0.17 / 0.18 / 0.28 on the same inputs.  Every narrow code was inside q of the interval."""
import ctypes as C

import numpy as np
import pytest

from lowbits import BF16, F16, _bits16, _e4m3_values, _GRID, _unpack_codes, _unpack_nibbles, _val16, fp4_codes_signed, quantize

pytestmark = pytest.mark.gpu

RATIOS = {}   # form -> largest |out - v| / delta this run has seen (test_zz_report_ratios prints it)

U = 2.0 ** -24
F32_, BF16_, F16_, E4M3_, SPLIT3_, F16C_, F16C2_ = range(7)   # ARP_LN_OUT_*
FORM_NAME = ["f32", "bf16", "f16", "e4m3", "split3", "f16c", "f16c2"]
ESZ = [4, 2, 2, 1, 2, 2, 2]
NARROW = {BF16_: "bf16", F16_: "f16", E4M3_: "e4m3"}
LNPRE, LAT_LN1, LAT_STATS = 0, 1, 2
FILL = 0x5A
WIDTHS = [4, 64, 68, 256, 260, 512, 516, 768, 772, 1024, 1028, 1280, 2044, 2048]
WIDTHS_C = [256, 512, 768, 1024, 1280, 2048]                  # f16c forms: D % 256 (gemm_c's rule)
WIDTHS_3 = [d for d in WIDTHS if (3 * d) % 64 == 0]           # [hi | lo | hi]: the K = 3 D binary16 product wants K % 64
ONE_PER_NV = [68, 260, 516, 772, 1028]                        # ARP_NV_DISPATCH: 1, 2, 3, 4, 8 float4 per lane, each with a ragged last group
ONE_PER_NV_C = [256, 512, 768, 1024, 1280]


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _filled(nbytes):
    return np.full(nbytes, FILL, np.uint8)


def _widths_of(form):
    return WIDTHS_C if form in (F16C_, F16C2_) else WIDTHS_3 if form == SPLIT3_ else WIDTHS


def _row_elems(form, D):
    return 3 * D if form == SPLIT3_ else 3 * D // 2 if form in (F16C_, F16C2_) else D


# ---- inputs and the float64 reference ---------------------------------------------------------------------------------------------------------

def _ln_inputs(D, form, nrows=9, base=2000):
    """(base: seed offset -- 2000 is the first multiple of 1000 at which the three coverage conditions test_layernorm_dense asserts on the float64
    reference hold at every width >= 256.)
    x = 3 N(0, 1) + 1 as tests/test_ops_gpu.py::test_layernorm; row 1 shifted by +24 (cancellation in the mean), row 2 with one 1e3 outlier (a normalised
    value of about sqrt(D)), row 3 scaled by 1e-3 (eps matters); w = 1 + 0.1 N, b = N, times 32 in the e4m3 form as the product pre-scales them"""
    rng = np.random.default_rng(base + D)
    x = (rng.standard_normal((nrows, D)) * 3 + 1).astype(np.float32)
    if nrows > 3:
        x[1] += np.float32(24)
        x[2, D // 3] = np.float32(1e3)
        x[3] *= np.float32(1e-3)
    w = (1 + 0.1 * rng.standard_normal(D)).astype(np.float32)
    b = rng.standard_normal(D).astype(np.float32)
    if form == E4M3_:
        w, b = w * np.float32(32), b * np.float32(32)
    return x, w, b


def _ln_ref(x, w, b, eps):
    """float64 LayerNorm of f32 inputs (eps as the f32 the kernel receives) and the element bound delta of the module docstring"""
    x, w, b = x.astype(np.float64), w.astype(np.float64), b.astype(np.float64)
    eps = float(np.float32(eps))
    mu = x.mean(1, keepdims=True)
    rstd = 1.0 / np.sqrt(((x - mu) ** 2).mean(1, keepdims=True) + eps)
    xh = (x - mu) * rstd
    a = np.abs(x).mean(1, keepdims=True) * rstd
    return xh * w + b, 16 * U * (np.abs(xh * w) + np.abs(b) + a * np.abs(w))


def _note(form, ratio):
    name = FORM_NAME[form] if isinstance(form, int) else form
    RATIOS[name] = max(RATIOS.get(name, 0.0), float(ratio))


def _check_narrow(dec, v, delta, fmt, what):
    lo, hi = quantize(v - delta, fmt), quantize(v + delta, fmt)
    bad = ~((lo <= dec) & (dec <= hi))
    assert not bad.any(), (f"{what}: {bad.sum()} of {bad.size} stored {fmt} codes are not q(t) for any t in [v - delta, v + delta]; first at "
                           f"{tuple(np.argwhere(bad)[0])}: stored {dec[bad][0]!r}, v {v[bad][0]!r}, delta {delta[bad][0]:.3e}")


def _check_ln_rows(form, buf, rows, D, stride, v, delta, fill, what):
    """buf: the returned bytes, [rows, stride * ESZ]; judges the payload by the form's rule and every other byte against the fill"""
    esz, re_ = ESZ[form], _row_elems(form, D)
    b2 = buf.reshape(rows, stride * esz)
    f2 = fill.reshape(rows, stride * esz)
    written = np.zeros_like(b2, bool)
    written[:, :re_ * esz] = True
    if form == F16C_:
        written[:, 5 * D // 2:3 * D] = False            # the dx4 segment keeps the caller's bytes
    assert np.array_equal(b2[~written], f2[~written]), f"{what}: bytes outside the rows' payload changed"
    pay = np.ascontiguousarray(b2[:, :re_ * esz])
    if form == F32_:
        out = pay.view(np.float32).astype(np.float64)
        r = np.abs(out - v) / delta
        print(f"{what}: max |out - v| / delta = {r.max():.3f}")
        _note(form, r.max())
        assert (r <= 1.0).all(), f"{what}: |out - v| / delta reaches {r.max():.3f} at {np.unravel_index(r.argmax(), r.shape)}"
    elif form in (BF16_, F16_):
        _check_narrow(_val16(pay.view(np.uint16), BF16 if form == BF16_ else F16), v, delta, NARROW[form], what)
    elif form == E4M3_:
        dec = _e4m3_values(pay)
        assert not np.isnan(dec).any(), f"{what}: the kernel stored an e4m3 NaN"
        _check_narrow(dec, v, delta, "e4m3", what)
    elif form == SPLIT3_:
        h16 = pay.view(np.uint16)
        hi, lo, hi2 = h16[:, :D], h16[:, D:2 * D], h16[:, 2 * D:]
        assert np.array_equal(hi, hi2), f"{what}: the third segment is not the first"
        dh, dl = _val16(hi, F16), _val16(lo, F16)
        _check_narrow(dh, v, delta, "f16", what + " hi")
        r = np.abs(dh + dl - v) / (delta + 2.0 ** -11 * np.abs(dl) + 2.0 ** -25)
        print(f"{what}: max |hi + lo - v| / (delta + 2^-11 |lo| + 2^-25) = {r.max():.3f}")
        _note(form, r.max())
        assert (r <= 1.0).all(), f"{what}: hi + lo misses v by {r.max():.3f} of its bound at {np.unravel_index(r.argmax(), r.shape)}"
    else:
        dh = _val16(np.ascontiguousarray(pay[:, :2 * D]).view(np.uint16), F16)
        _check_narrow(dh, v, delta, "f16", what + " hi")
        x4 = _unpack_nibbles(pay[:, 2 * D:5 * D // 2])
        assert np.array_equal(x4, quantize(2.0 * dh, "e2m1")), f"{what}: x4 is not fp4(2 hi) of the kernel's own hi"
        if form == F16C2_:
            dx = _unpack_nibbles(pay[:, 5 * D // 2:])
            lo, hi = quantize((v - delta - dh) * 2.0 ** 13, "e2m1"), quantize((v + delta - dh) * 2.0 ** 13, "e2m1")
            bad = ~((lo <= dx) & (dx <= hi))
            assert not bad.any(), f"{what}: {bad.sum()} dx4 nibbles are not fp4((t - hi) 2^13) for any t in [v - delta, v + delta]"


def _run_ln(lib, form, x2d, in_stride, idx, w, b, rows, D, eps, out_stride):
    """x2d: the f32 array handed over whole; returns (rc, returned bytes, the fill they went up as)"""
    nbytes = rows * out_stride * ESZ[form]
    buf = _filled(nbytes)
    fill = buf.copy()
    rc = lib.lib.arp_op_layernorm_forms(form, _fp(x2d), x2d.size, in_stride, _ip(idx) if idx is not None else None, _fp(w), _fp(b), _vp(buf), nbytes,
                                        out_stride, rows, D, eps)
    return rc, buf, fill


# ---- LayerNorm: dense, every form, every width -------------------------------------------------------------------------------------------------

LN_DENSE = [(f, d) for f in range(7) for d in _widths_of(f)]


@pytest.mark.parametrize("form,D", LN_DENSE, ids=[f"{FORM_NAME[f]}-{d}" for f, d in LN_DENSE])
def test_layernorm_dense(gpu_lib, form, D):
    """layernorm_kernel<OutT, NV> through tower_layernorm, dense rows, eps 1e-5 and 1e-6, 1 / 5 / 9 rows (no multiple of the four rows of a workgroup).
    Measured on an MI355X: largest |out - v| / delta 0.175 (f32 form), 0.275 of its own bound for hi + lo of the split form; every bf16, binary16, e4m3
    and [hi | x4 (| dx4)] code inside the quantiser's image of [v - delta, v + delta]."""
    x9, w, b = _ln_inputs(D, form)
    stride = _row_elems(form, D)
    for eps in (1e-5, 1e-6):
        v9, d9 = _ln_ref(x9, w, b, eps)
        if D >= 256 and form == E4M3_:      # the inputs must keep exercising saturation and the subnormal range (asserted on the reference alone)
            assert (np.abs(v9) > 448).any(), "no e4m3 saturation in the reference"
            if D >= 516:
                assert ((np.abs(v9) < 2.0 ** -6) & (v9 != 0)).any(), "no e4m3 subnormal in the reference"
        if D >= 256 and form in (F16C_, F16C2_):
            share = (np.abs(2 * np.delete(v9, [2, 3], axis=0)) > 6).mean()   # (the outlier row and the scaled row are narrower by construction)
            assert 0.03 <= share <= 0.04, f"{share:.4f} of 2 hi beyond +-6"
            dxr = quantize((v9 - quantize(v9, "f16")) * 2.0 ** 13, "e2m1")
            assert set(np.unique(np.abs(dxr))) == set(_GRID), "not every e2m1 magnitude occurs in dx4"
        for rows, sel in ((9, slice(0, 9)), (5, slice(0, 5)), (1, slice(2, 3))):
            x = np.ascontiguousarray(x9[sel])
            rc, buf, fill = _run_ln(gpu_lib, form, x, D, None, w, b, rows, D, eps, stride)
            gpu_lib.check(rc)
            _check_ln_rows(form, buf, rows, D, stride, v9[sel], d9[sel], fill, f"layernorm {FORM_NAME[form]} D={D} eps={eps} rows={rows}")


LN_VARIANTS = [(f, d) for f in range(7) for d in (ONE_PER_NV_C if f >= SPLIT3_ else ONE_PER_NV)]


@pytest.mark.parametrize("form,D", LN_VARIANTS, ids=[f"{FORM_NAME[f]}-{d}" for f, d in LN_VARIANTS])
def test_layernorm_strided_padded_gathered(gpu_lib, form, D):
    """One width per NV: (a) the class-token form -- in_stride = 3 D -- into rows padded by 8 elements, the pad bytes untouched; (b) where it is instantiated
    (f32, bf16, binary16: run_text), layernorm_gather_kernel on a shuffled, repeating index list."""
    x9, w, b = _ln_inputs(D, form)
    eps = 1e-5
    v9, d9 = _ln_ref(x9, w, b, eps)
    rng = np.random.default_rng(D)
    wide = (rng.standard_normal((9, 3 * D)) * 3 + 1).astype(np.float32)
    wide[:, :D] = x9
    stride = _row_elems(form, D) + 8
    rc, buf, fill = _run_ln(gpu_lib, form, wide, 3 * D, None, w, b, 9, D, eps, stride)
    gpu_lib.check(rc)
    _check_ln_rows(form, buf, 9, D, stride, v9, d9, fill, f"layernorm {FORM_NAME[form]} D={D} strided in, padded out")
    idx = np.array([7, 2, 2, 8, 0, 7, 5, 3, 2, 1, 6], np.int32)
    src = np.ascontiguousarray(wide[:, :D + 4])          # in_stride = D + 4
    rc, buf, fill = _run_ln(gpu_lib, form, src, D + 4, idx, w, b, len(idx), D, eps, _row_elems(form, D))
    if form in (F32_, BF16_, F16_):
        gpu_lib.check(rc)
        _check_ln_rows(form, buf, len(idx), D, _row_elems(form, D), v9[idx], d9[idx], fill, f"layernorm_gather {FORM_NAME[form]} D={D}")
    else:
        assert rc != 0 and "gathered" in gpu_lib.last_error() and np.array_equal(buf, fill)


def test_layernorm_refusals(gpu_lib):
    """Widths the kernel or the consuming GEMM refuses are refused with that launcher's rule, and the output comes back as it went up.  D % 8 == 4 in the
    f16c forms would be an 8-byte store at a 4-byte-aligned address (rows of 3 D bytes): D % 256 covers it."""
    for form, D, word in ((F16C_, 260, "256"), (F16C2_, 260, "256"), (F16C2_, 64, "256"), (F16C_, 1028, "256"), (SPLIT3_, 68, "K % 64"),
                          (SPLIT3_, 260, "K % 64"), (F32_, 6, "unsupported width"), (F16_, 2052, "unsupported width"), (E4M3_, 2304, "unsupported width")):
        Dp = (D + 3) // 4 * 4
        x = np.ones((2, Dp), np.float32)
        w = np.ones(Dp, np.float32)
        rc, buf, fill = _run_ln(gpu_lib, form, x, Dp, None, w, w, 2, D, 1e-5, 2 * Dp)
        assert rc != 0 and word in gpu_lib.last_error(), (form, D, gpu_lib.last_error())
        assert np.array_equal(buf, fill)
    x = np.ones((2, 64), np.float32)
    w = np.ones(64, np.float32)
    rc, buf, fill = _run_ln(gpu_lib, F32_, x, 64, np.array([0, 2], np.int32), w, w, 2, 64, 1e-5, 64)   # row 2 of a two-row x
    assert rc != 0 and "outside" in gpu_lib.last_error() and np.array_equal(buf, fill)


# ---- row_stats_kernel --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [BF16, F16])
@pytest.mark.parametrize("D", [128, 384, 768, 1024])
def test_row_stats(gpu_lib, mode, D):
    """xb = the operand-type rounding of x, bit for bit; stats[r][s] = (sum, sum of squares) of columns 128 s .. 128 s + 127.  Longest path: 2 additions inside a
    lane's float4 and 5 shuffle levels inside a 32-lane half, L = 7; a square is one rounding more: bound (L + 1) u sum |terms| for both."""
    L = 7
    for rows in (1, 6):
        x = _ln_inputs(D, F32_, 6)[0][:rows].copy()
        parts = D // 128
        xb, st = _filled(rows * D * 2), _filled(rows * parts * 8)
        gpu_lib.check(gpu_lib.lib.arp_op_row_stats(mode, _fp(x), _vp(xb), xb.size, _vp(st), st.size, rows, D))
        assert np.array_equal(xb.view(np.uint16).reshape(rows, D), _bits16(x, mode)), "operand copy"
        st = st.view(np.float32).reshape(rows, parts, 2).astype(np.float64)
        seg = x.astype(np.float64).reshape(rows, parts, 128)
        for k, terms in enumerate((seg, seg * seg)):
            err = np.abs(st[:, :, k] - terms.sum(2))
            bound = (L + 1) * U * np.abs(terms).sum(2)
            assert (err <= bound).all(), f"row_stats D={D} rows={rows} {'sum' if k == 0 else 'sumsq'}: err / bound = {(err / bound).max():.3f}"
    assert gpu_lib.lib.arp_op_row_stats(mode, _fp(x), _vp(xb), xb.size, _vp(st), 8, 1, 64) != 0 and "128" in gpu_lib.last_error()


# ---- token assembly ------------------------------------------------------------------------------------------------------------------------------

def _nv(D):
    nv = (D + 255) // 256
    return nv if nv <= 4 else 8


@pytest.mark.parametrize("D", [64, 260, 768])
@pytest.mark.parametrize("ntok", [2, 5])
@pytest.mark.parametrize("B", [1, 3])
def test_vit_assemble(gpu_lib, B, ntok, D):
    """vit_assemble_lnpre_kernel, and vit_assemble_lat_kernel<T> with 1 to 4 slabs in both tails.  The assembled row is a chain of f32 additions in a fixed
    order (slab 0 + pos, + slab 1, + slab 2, + slab 3), restated here in numpy f32 bit for bit; x is then judged as the LayerNorm of THAT row.  Every slab
    and the position table are O(1) wide, so a dropped or doubled slab moves x at O(1).  The floats behind the class embedding, where a class row's slabs
    would be, are NaN.  Tail ln_1: h by the narrow rule against LayerNorm(returned x; w1, b1).  Tail stats: h = the operand rounding of the returned x bit for
    bit, strip 0 = (sum, sum of squares) of the returned x -- longest path 2 additions in a float4, NV - 1 across a lane's float4s, 6 shuffle levels:
    L = NV + 7 -- within (L + 1) u sum |terms|, strips 1 .. D / 16 - 1 exactly 0."""
    rng = np.random.default_rng(B * 100 + ntok * 10 + D)
    rows, prow, eps = B * ntok, B * (ntok - 1) * D, 1e-5
    slice_stride = prow + 8
    slabs = (rng.standard_normal((4, slice_stride)) * 3 + 1).astype(np.float32)
    cls = (rng.standard_normal(D) * 3).astype(np.float32)
    pos = (rng.standard_normal((ntok, D)) * 2).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(D)).astype(np.float32)
    b = rng.standard_normal(D).astype(np.float32)
    w1 = (1 + 0.1 * rng.standard_normal(D)).astype(np.float32)
    b1 = rng.standard_normal(D).astype(np.float32)
    tpos = np.tile(pos, (B, 1))
    is_cls = np.tile(np.arange(ntok) == 0, B)

    def assembled(S):
        row = np.empty((rows, D), np.float32)
        row[is_cls] = cls + pos[0]
        acc = slabs[0, :prow].reshape(-1, D) + tpos[~is_cls]
        for s in range(1, S):
            acc = acc + slabs[s, :prow].reshape(-1, D)
        row[~is_cls] = acc
        return row

    def check_x(xbuf, S, what):
        v, delta = _ln_ref(assembled(S), w, b, eps)
        x = xbuf.view(np.float32).reshape(rows, D)
        r = np.abs(x.astype(np.float64) - v) / delta
        _note("assemble x", r.max())
        assert (r <= 1.0).all(), f"{what}: x misses ln_pre of the assembled row, |x - v| / delta = {r.max()} (NaN: a class row read a slab)"
        return x

    xb = _filled(rows * D * 4)
    gpu_lib.check(gpu_lib.lib.arp_op_vit_assemble(0, LNPRE, _fp(slabs[0]), prow, 1, 0, _fp(cls), D, _fp(pos), _fp(w), _fp(b), None, None, _vp(xb), xb.size,
                                                  None, 0, None, 0, B, ntok, D, eps))
    check_x(xb, 1, f"assemble_lnpre B={B} ntok={ntok} D={D}")
    L = _nv(D) + 7
    parts = D >> 4
    for mode in (BF16, F16):
        fmt = "bf16" if mode == BF16 else "f16"
        for S in (1, 2, 3, 4):
            clsbuf = np.full((S - 1) * slice_stride + D, np.nan, np.float32)
            clsbuf[:D] = cls
            flat = np.ascontiguousarray(slabs[:S]).reshape(-1)
            for tail in (LAT_LN1, LAT_STATS):
                what = f"assemble_lat {fmt} tail={tail} S={S} B={B} ntok={ntok} D={D}"
                xb, hb, sb = _filled(rows * D * 4), _filled(rows * D * 2), _filled(rows * parts * 8)
                gpu_lib.check(gpu_lib.lib.arp_op_vit_assemble(mode, tail, _fp(flat), (S - 1) * slice_stride + prow, S, slice_stride, _fp(clsbuf), clsbuf.size,
                                                              _fp(pos), _fp(w), _fp(b), _fp(w1), _fp(b1), _vp(xb), xb.size, _vp(hb), hb.size,
                                                              _vp(sb) if tail == LAT_STATS else None, sb.size if tail == LAT_STATS else 0, B, ntok, D, eps))
                x = check_x(xb, S, what)
                h16 = hb.view(np.uint16).reshape(rows, D)
                if tail == LAT_LN1:
                    v1, d1 = _ln_ref(x, w1, b1, eps)
                    _check_narrow(_val16(h16, mode), v1, d1, fmt, what + " h")
                    assert (sb == FILL).all()
                else:
                    assert np.array_equal(h16, _bits16(x, mode)), what + ": operand copy"
                    st = sb.view(np.float32).reshape(rows, parts, 2).astype(np.float64)
                    assert (st[:, 1:] == 0).all(), what + ": strips 1 .. parts - 1 must be exactly 0"
                    x64 = x.astype(np.float64)
                    for k, terms in enumerate((x64, x64 * x64)):
                        err, bound = np.abs(st[:, 0, k] - terms.sum(1)), (L + 1) * U * np.abs(terms).sum(1)
                        assert (err <= bound).all(), f"{what} {'sum' if k == 0 else 'sumsq'}: err / bound = {(err / bound).max():.3f}"
    # five slabs: the kernel would silently drop the fifth -- the launcher refuses and nothing is written
    flat = np.zeros(5 * slice_stride, np.float32)
    xb, hb = _filled(rows * D * 4), _filled(rows * D * 2)
    rc = gpu_lib.lib.arp_op_vit_assemble(F16, LAT_LN1, _fp(flat), flat.size, 5, slice_stride, _fp(cls), D, _fp(pos), _fp(w), _fp(b), _fp(w1), _fp(b1), _vp(xb),
                                         xb.size, _vp(hb), hb.size, None, 0, B, ntok, D, eps)
    assert rc != 0 and "slabs" in gpu_lib.last_error() and (xb == FILL).all() and (hb == FILL).all()


# ---- text_embed, rows_gather, l2_normalize, reward ------------------------------------------------------------------------------------------------

SMALL_D = [4, 60, 64, 512, 768]


@pytest.mark.parametrize("D", SMALL_D)
def test_text_embed(gpu_lib, D):
    """x[r] = emb[tokens[r]] + pos[r % ctx]: one f32 addition per element, bit for bit; a token id repeats at different positions"""
    rng = np.random.default_rng(D)
    vocab, ctx = 11, 3
    emb = rng.standard_normal((vocab, D)).astype(np.float32)
    pos = rng.standard_normal((ctx, D)).astype(np.float32)
    for rows in (1, 7):
        tok = np.array([5, 10, 5, 0, 5, 3, 10], np.int32)[:rows].copy()
        xb = _filled((rows + 1) * D * 4)
        gpu_lib.check(gpu_lib.lib.arp_op_text_embed(_ip(tok), _fp(emb), vocab, _fp(pos), _vp(xb), xb.size, rows, ctx, D))
        x = xb.view(np.float32).reshape(rows + 1, D)
        assert np.array_equal(x[:rows].view(np.uint32), (emb[tok] + pos[np.arange(rows) % ctx]).view(np.uint32))
        assert (xb[rows * D * 4:] == FILL).all(), "row behind the last one written"
    assert gpu_lib.lib.arp_op_text_embed(_ip(np.array([11], np.int32)), _fp(emb), vocab, _fp(pos), _vp(xb), xb.size, 1, ctx, D) != 0


@pytest.mark.parametrize("D", SMALL_D)
def test_rows_gather(gpu_lib, D):
    """out[b, col0 + d] = x[row(b), d] with an index list (repeats) or a fixed row stride, into a wider table at a column offset: bit for bit, and every
    other element of the table untouched"""
    rng = np.random.default_rng(D + 1)
    x = rng.standard_normal((22, D)).astype(np.float32)
    for B in (1, 7):
        for idx, stride in ((np.array([9, 0, 9, 21, 3, 3, 14], np.int32)[:B].copy(), 0), (None, 3)):
            for ld, col0 in ((D, 0), (2 * D + 5, D + 3)):
                ob = _filled(B * ld * 4)
                gpu_lib.check(gpu_lib.lib.arp_op_rows_gather(_fp(x), x.size, D, _ip(idx) if idx is not None else None, stride, _vp(ob), ob.size, ld, col0, B))
                want = _filled(B * ld * 4).view(np.float32).reshape(B, ld).copy()
                want[:, col0:col0 + D] = x[idx] if idx is not None else x[np.arange(B) * stride]
                assert np.array_equal(ob.view(np.uint32), want.reshape(-1).view(np.uint32)), (B, stride, ld, col0)
    ob = _filled(4 * D)
    assert gpu_lib.lib.arp_op_rows_gather(_fp(x), x.size, D, _ip(np.array([22], np.int32)), 0, _vp(ob), ob.size, D, 0, 1) != 0


def _dot_L(E):
    """a lane accumulates ceil(E / 64) products one after the other (the first addition, to 0, is exact), then 6 shuffle levels"""
    return (E + 63) // 64 - 1 + 6


@pytest.mark.parametrize("E", SMALL_D)
def test_l2_normalize(gpu_lib, E):
    """f[r] *= 1 / sqrt(sum f[r]^2).  The sum of squares has relative error <= (L + 1) u (all terms positive; L = ceil(E / 64) - 1 + 6 additions, one rounding
    per square); the square root halves that and adds its own rounding, the reciprocal and the final product one each: |out - v| <= ((L + 1) / 2 + 3) u |v|,
    plus one u for the second-order terms."""
    rng = np.random.default_rng(E + 2)
    rel = ((_dot_L(E) + 1) / 2 + 4) * U
    for rows in (1, 7):
        f = (rng.standard_normal((rows, E)) * 10.0 ** rng.uniform(-3, 3, (rows, 1))).astype(np.float32)
        fb = np.concatenate([f.reshape(-1).view(np.uint8), _filled(E * 4)])
        gpu_lib.check(gpu_lib.lib.arp_op_l2_normalize(_vp(fb), fb.size, rows, E))
        out = fb[:rows * E * 4].view(np.float32).reshape(rows, E).astype(np.float64)
        v = f.astype(np.float64) / np.sqrt((f.astype(np.float64) ** 2).sum(1, keepdims=True))
        err = np.abs(out - v)
        assert (err <= rel * np.abs(v)).all(), f"l2_normalize E={E}: err / bound = {(err / (rel * np.abs(v)))[v != 0].max():.3f}"
        assert (fb[rows * E * 4:] == FILL).all()


@pytest.mark.parametrize("E", SMALL_D)
def test_reward(gpu_lib, E):
    """reward[r] = scale (dt / sqrt(ss)), dt = <img[r], txt>, ss = <img[r], img[r]>.  |d dt| <= (L + 1) u sum |a t|; ss as in test_l2_normalize; then the
    quotient and the scale are one rounding each: bound = scale ((L + 1) u sum |a t| + |dt| ((L + 1) / 2 + 4) u) / sqrt(ss)."""
    rng = np.random.default_rng(E + 3)
    L, scale = _dot_L(E), float(np.float32(np.exp(4.6052)))
    for rows in (1, 7):
        img = (rng.standard_normal((rows, E)) * 10.0 ** rng.uniform(-2, 2, (rows, 1))).astype(np.float32)
        txt = rng.standard_normal(E).astype(np.float32)
        txt /= np.float32(np.sqrt((txt.astype(np.float64) ** 2).sum()))
        rb = _filled((rows + 3) * 4)
        gpu_lib.check(gpu_lib.lib.arp_op_reward(_fp(img), _fp(txt), scale, _vp(rb), rb.size, rows, E))
        a, t = img.astype(np.float64), txt.astype(np.float64)
        ss, dt = (a * a).sum(1), (a * t).sum(1)
        v = scale * dt / np.sqrt(ss)
        bound = scale * ((L + 1) * U * np.abs(a * t).sum(1) + np.abs(dt) * ((L + 1) / 2 + 4) * U) / np.sqrt(ss)
        err = np.abs(rb[:rows * 4].view(np.float32).astype(np.float64) - v)
        assert (err <= bound).all(), f"reward E={E} rows={rows}: err / bound = {(err / bound).max():.3f}"
        assert (rb[rows * 4:] == FILL).all()


# ---- the operand converters ------------------------------------------------------------------------------------------------------------------------

def _conv_inputs(rows, D):
    """magnitudes from binary16's subnormal range up to 6e4 (none overflows binary16), and at fixed places: +-0, exact binary16 ties, e2m1 ties in both
    segments (2 hi in {1.25, 1.75, 2.5, 3.5, 5}; a residual of exactly 2.5 * 2^-13), binary16 subnormals and their ties, the largest values"""
    rng = np.random.default_rng(rows * 1000 + D)
    x = (rng.standard_normal((rows, D)) * 10.0 ** rng.uniform(-7.5, 4.3, (rows, D))).astype(np.float32)
    x = np.clip(x, -6e4, 6e4)
    special = np.array([0.0, -0.0, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 0.625, 0.875, 1.25, 1.75, 2.5, -1.25, -0.875, 1 + 2.5 * 2.0 ** -13,
                        -(1 + 2.5 * 2.0 ** -13), 3e-6, -1e-7, 1.5 * 2.0 ** -24, 2.0 ** -25, -2.0 ** -24, 6e4, -65504.0, 65519.0, 2.0 ** -14, -1e-9],
                       np.float32)
    flat = x.reshape(-1)
    n = min(len(special), flat.size)
    flat[rng.permutation(flat.size)[:n]] = special[:n]
    assert np.isfinite(x.astype(np.float16)).all()
    return x


def _f16c_rows(x):
    """the [hi | x4 | dx4] segments of f32 x, every one a deterministic function of x: hi = rn16(x), x4 = fp4(2 hi), dx4 = fp4((x - hi) 2^13), all of
    them exact f32 operations ahead of ONE rounding"""
    hi = x.astype(np.float16)
    h32 = hi.astype(np.float32)
    res = (x - h32) * np.float32(2.0 ** 13)        # x - hi is exact in f32; the scaling is a power of two
    assert np.array_equal((x.astype(np.float64) - h32.astype(np.float64)) * 2.0 ** 13, res.astype(np.float64))
    pack = lambda c: (c[:, 0::2] | (c[:, 1::2] << 4)).astype(np.uint8)
    return hi.view(np.uint16), pack(fp4_codes_signed(h32 * np.float32(2))), pack(fp4_codes_signed(res))


@pytest.mark.parametrize("D", [16, 24, 256, 768])
def test_convert_f16c(gpu_lib, D):
    """launch_convert_f16c: convert_f16c16_kernel<true> / <false> where D % 16 == 0, convert_f16c_kernel (four values per lane; D = 24) elsewhere.  xb and
    all three segments of xc bit for bit; without dx4 the 16-value kernel leaves that segment's bytes alone."""
    for rows in (1, 5):
        x = _conv_inputs(rows, D)
        hi, x4, dx4 = _f16c_rows(x)
        for with_dx in (1, 0):
            xb, xc = _filled(rows * D * 2 + 16), _filled(rows * D * 3 + 16)
            gpu_lib.check(gpu_lib.lib.arp_op_convert_f16c(with_dx, _fp(x), _vp(xb), xb.size, _vp(xc), xc.size, rows, D))
            what = f"convert_f16c D={D} rows={rows} with_dx={with_dx}"
            assert np.array_equal(xb[:rows * D * 2].view(np.uint16).reshape(rows, D), hi), what + ": xb"
            r = xc[:rows * D * 3].reshape(rows, 3 * D)
            assert np.array_equal(np.ascontiguousarray(r[:, :2 * D]).view(np.uint16), hi), what + ": hi"
            assert np.array_equal(_unpack_codes(r[:, 2 * D:5 * D // 2]), _unpack_codes(x4)), what + ": x4"
            if with_dx or D % 16:
                assert np.array_equal(_unpack_codes(r[:, 5 * D // 2:]), _unpack_codes(dx4)), what + ": dx4"
            else:
                assert (r[:, 5 * D // 2:] == FILL).all(), what + ": dx4 bytes must keep the fill"
            assert (xb[rows * D * 2:] == FILL).all() and (xc[rows * D * 3:] == FILL).all(), what + ": bytes behind the last row"
    xb, xc = _filled(2 * 20 * 2), _filled(2 * 20 * 3)
    assert gpu_lib.lib.arp_op_convert_f16c(1, _fp(np.ones((2, 20), np.float32)), _vp(xb), xb.size, _vp(xc), xc.size, 2, 20) != 0  # 8-byte stores, 60-byte rows
    assert (xb == FILL).all() and (xc == FILL).all()


@pytest.mark.parametrize("D", [16, 256, 768])
def test_extract_hi(gpu_lib, D):
    rng = np.random.default_rng(D + 4)
    for rows in (1, 5):
        for ld in (3 * D // 2, D + 8):
            src = rng.integers(0, 65536, (rows, ld), dtype=np.uint16)
            ob = _filled(rows * D * 2 + 16)
            gpu_lib.check(gpu_lib.lib.arp_op_extract_hi(_vp(src), src.size * 2, ld, _vp(ob), ob.size, rows, D))
            assert np.array_equal(ob[:rows * D * 2].view(np.uint16).reshape(rows, D), src[:, :D]) and (ob[rows * D * 2:] == FILL).all(), (rows, ld)


@pytest.mark.parametrize("K", [16, 256, 768])
def test_split3(gpu_lib, K):
    """split3_kernel: hi = rn16(x), lo = rn16(x - hi) (x - hi exact in f32; binary16 subnormals kept), third segment = hi: bit for bit"""
    for rows in (1, 5):
        x = _conv_inputs(rows, K)
        hi = x.astype(np.float16)
        lo = (x - hi.astype(np.float32)).astype(np.float16)
        ob = _filled(rows * K * 6 + 16)
        gpu_lib.check(gpu_lib.lib.arp_op_split3(_fp(x), _vp(ob), ob.size, rows, K))
        got = ob[:rows * K * 6].view(np.uint16).reshape(rows, 3 * K)
        for name, seg, want in (("hi", got[:, :K], hi), ("lo", got[:, K:2 * K], lo), ("hi again", got[:, 2 * K:], hi)):
            assert np.array_equal(seg, want.view(np.uint16)), f"split3 K={K} rows={rows}: {name}"
        assert (ob[rows * K * 6:] == FILL).all()
    assert gpu_lib.lib.arp_op_split3(_fp(x), _vp(ob), ob.size, 1, 12) != 0


# ---- the M3AE encoder's sequence assembly ------------------------------------------------------------------------------------------------------------

M3AE_VOCAB = 9
M3AE_ASM = [(1, 1, 4, "plain"), (1, 1, 4, "goal"), (1, 1, 4, "text1"),      # the smallest of each kind
            (2, 3, 128, "plain"),                                            # 2 * 4 * 128 = 1024 values: exactly one full 256-thread block, no guard
            (3, 5, 36, "plain"), (3, 5, 36, "goal"), (3, 5, 36, "text7"), (3, 5, 36, "text7-rows")]   # a ragged last block: the guard


def _m3ae_asm_inputs(nb, GG, D, kind):
    rng = np.random.default_rng(nb * 1000 + GG * 100 + D)
    goal, L, per_row = int(kind == "goal"), {"text1": 1, "text7": 7, "text7-rows": 7}.get(kind, 0), int(kind == "text7-rows")
    pe = rng.standard_normal(((1 + goal) * nb * GG, D)).astype(np.float32)
    cls, pos = rng.standard_normal(D).astype(np.float32), rng.standard_normal((GG, D)).astype(np.float32)
    emb, tpos = rng.standard_normal((M3AE_VOCAB, D)).astype(np.float32), rng.standard_normal((max(L, 1), D)).astype(np.float32)
    # ids 0 and vocab - 1, a repeated id; with per_row every row has its own ids
    tok = np.array([[3, 0, 8, 3, 5, 1, 7], [8, 8, 2, 0, 6, 4, 1], [5, 7, 0, 0, 3, 8, 2]], np.int32)[:nb if per_row else 1, :max(L, 1)].copy()
    return goal, L, per_row, pe, cls, pos, emb, tpos, tok


@pytest.mark.parametrize("nb,GG,D,kind", M3AE_ASM, ids=[f"{n}x{g}x{d}-{k}" for n, g, d, k in M3AE_ASM])
def test_m3ae_assemble(gpu_lib, nb, GG, D, kind):
    """enc_assemble_kernel: row 0 = cls, the frame's patches + pos, then the goal's patches + pos or text_emb[tok] + tpos.  Every value is a copy or ONE f32
    addition of the same two operands: bit for bit.  x goes up as NaN, so an unwritten row fails."""
    goal, L, per_row, pe, cls, pos, emb, tpos, tok = _m3ae_asm_inputs(nb, GG, D, kind)
    ntok = 1 + (1 + goal) * GG + L
    want = np.empty((nb, ntok, D), np.float32)
    want[:, 0] = cls
    want[:, 1:1 + GG] = pe[:nb * GG].reshape(nb, GG, D) + pos
    if goal:
        want[:, 1 + GG:] = pe[nb * GG:].reshape(nb, GG, D) + pos
    if L:
        want[:, 1 + GG:] = emb[np.broadcast_to(tok, (nb, L))] + tpos[:L]
    x = np.full((nb, ntok, D), np.nan, np.float32)
    gpu_lib.check(gpu_lib.lib.arp_op_m3ae_assemble(_fp(pe), _fp(cls), _fp(pos), _fp(emb), _fp(tpos), _ip(tok), nb, GG, goal, L, per_row, D, M3AE_VOCAB, _fp(x)))
    assert np.array_equal(x, want), (kind, np.argwhere(~(x == want))[:4])


def test_m3ae_assemble_refusals(gpu_lib):
    lib = gpu_lib.lib
    for D, goal, ids, word in ((6, 0, [1, 2], "multiple of 4"), (4, 1, [1, 2], "do not combine"), (4, 0, [1, M3AE_VOCAB], "outside the vocabulary"),
                               (4, 0, [-1, 2], "outside the vocabulary")):
        pe, cls, pos = np.ones((2 * 3, D), np.float32), np.ones(D, np.float32), np.ones((3, D), np.float32)
        emb, tpos, tok = np.ones((M3AE_VOCAB, D), np.float32), np.ones((2, D), np.float32), np.array(ids, np.int32)
        x = np.full((1, 1 + 2 * 3 + 2, D), 7.0, np.float32)
        rc = lib.arp_op_m3ae_assemble(_fp(pe), _fp(cls), _fp(pos), _fp(emb), _fp(tpos), _ip(tok), 1, 3, goal, 2, 0, D, M3AE_VOCAB, _fp(x))
        assert rc != 0 and word in gpu_lib.last_error(), (D, goal, ids, gpu_lib.last_error())
        assert (x == 7.0).all()


# ---- the split-K reduce + LayerNorm row kernel, element by element ---------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [BF16, F16])
@pytest.mark.parametrize("shape", [(17, 64, 128), (50, 768, 256), (50, 1280, 256)])
def test_skinny_reduce_layernorm_elementwise(gpu_lib, mode, shape):
    """skinny_reduce_ln_kernel's LayerNorm output, judged by the narrow-form rule against the LayerNorm of the returned `out` (tests/test_ops_gpu.py::
    test_skinny_gemm holds it to 1.6e-2 max |ln| only: a small element may be wrong by its own size there)"""
    M, N, K = shape
    rng = np.random.default_rng(M + N + K)
    A = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    resid = (rng.standard_normal((M, N)) * 3 + 1).astype(np.float32)
    lw = (1 + 0.1 * rng.standard_normal(N)).astype(np.float32)
    lb = rng.standard_normal(N).astype(np.float32)
    for S in (1, 2, 4):
        out, h = np.empty((M, N), np.float32), np.empty((M, N), np.float32)
        gpu_lib.check(gpu_lib.lib.arp_op_skinny_gemm(mode, 0, _fp(A), _fp(W), _fp(bias), _fp(resid), _fp(out), M, N, K, S, _fp(lw), _fp(lb), 1e-5, _fp(h)))
        v, delta = _ln_ref(out, lw, lb, 1e-5)
        _check_narrow(h.astype(np.float64), v, delta, "bf16" if mode == BF16 else "f16", f"skinny reduce + LayerNorm mode={mode} {shape} S={S}")


def test_zz_report_ratios():
    """prints what the LayerNorm tests of this run measured (pytest -s); runs last in the module"""
    for k, r in sorted(RATIOS.items()):
        print(f"largest |out - v| / delta, {k}: {r:.3f}")
