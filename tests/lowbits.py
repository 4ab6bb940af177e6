"""Host-side encoders / decoders of the narrow number formats the kernels store (binary16, bf16, OCP e2m1 nibbles, OCP e4m3 bytes), shared by the
op-level GPU test modules (tests/test_gemm_epilogues_gpu.py, tests/test_attention_forms_gpu.py, tests/test_row_kernels_gpu.py).  Plain numpy; nothing
here calls the library."""
import numpy as np

from conftest import bf16_round

F16, BF16 = 2, 1   # ARP_MODE_F16 / ARP_MODE_BF16


def _bits16(x, mode):
    """f32 / f64 values -> the nearest-even 16-bit words (bf16 via f32: a double rounding only within an f32 ulp of a midpoint)"""
    if mode == F16:
        return np.asarray(x, np.float64).astype(np.float16).view(np.uint16)
    return (bf16_round(np.asarray(x, np.float32)).view(np.uint32) >> 16).astype(np.uint16)


def _val16(b, mode):
    b = np.asarray(b, np.uint16)
    if mode == F16:
        return b.view(np.float16).astype(np.float64)
    return (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


# format -> (significand bits incl. the hidden one, exponent of the smallest normal, largest finite value, what an overflow becomes)
_FORMATS = {"f16": (11, -14, 65504.0, np.inf), "bf16": (8, -126, float.fromhex("0x1.fep127"), np.inf), "e4m3": (4, -6, 448.0, 448.0),
            "e2m1": (2, 0, 6.0, 6.0)}


def quantize(x, fmt):
    """float64 -> the format's round-to-nearest-even value, as float64, in ONE rounding (no detour through f32): subnormals on the format's own grid,
    e4m3 / e2m1 saturating at their largest value, binary16 / bf16 overflowing to infinity.  Monotone non-decreasing in x, which is what the acceptance
    rule q(v - delta) <= stored <= q(v + delta) of tests/test_row_kernels_gpu.py rests on."""
    p, emin, vmax, over = _FORMATS[fmt]
    x = np.asarray(x, np.float64)
    _, e = np.frexp(x)                           # |x| in [2^(e-1), 2^e)
    ulp = np.ldexp(1.0, np.maximum(e, emin + 1) - p)
    q = np.rint(x / ulp) * ulp                   # x / ulp is exact (a power of two); rint rounds half to even
    return np.where(np.abs(q) > vmax, np.copysign(over, x), q)


def fp4_codes_signed(x):
    """f32 / f64 values -> e2m1 codes of their round-to-nearest-even, saturating quantisation; the sign bit is the value's own (a negative value that
    rounds to zero keeps it, as csrc/common.h::host_f2fp4 does)"""
    x = np.asarray(x, np.float64)
    return (np.searchsorted(_GRID, np.abs(quantize(x, "e2m1"))) | np.where(np.signbit(x), 8, 0)).astype(np.uint8)


_GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def _quant_fp4(x):
    """OCP e2m1 with round-to-nearest-even, saturating at 6 (as tests/test_ops_gpu.py::_quant_fp4)"""
    x = np.asarray(x, np.float64)
    a = np.abs(x)
    idx = np.clip(np.searchsorted(_GRID, a, side="left"), 1, 7)
    lo, hi = _GRID[idx - 1], _GRID[idx]
    mid = 0.5 * (lo + hi)
    q = np.where(a < mid, lo, np.where(a > mid, hi, np.where((idx - 1) % 2 == 0, lo, hi)))
    return np.sign(x) * np.minimum(q, 6.0)


def _fp4_codes(v):
    """e2m1 values (already on the grid) -> 4-bit codes"""
    v = np.asarray(v, np.float64)
    return (np.searchsorted(_GRID, np.abs(v)) | np.where(v < 0, 8, 0)).astype(np.uint8)


def _pack_nibbles(codes):
    """[R, K] codes -> [R, K / 2] bytes, value 2j in the low nibble"""
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).astype(np.uint8)


def _unpack_codes(b):
    """[R, K / 2] bytes -> [R, K] 4-bit codes, value 2j from the low nibble"""
    b = np.asarray(b, np.uint8)
    codes = np.empty((b.shape[0], b.shape[1] * 2), np.uint8)
    codes[:, 0::2], codes[:, 1::2] = b & 15, b >> 4
    return codes


def _unpack_nibbles(b):
    codes = _unpack_codes(b)
    mag = _GRID[codes & 7]
    return np.where(codes & 8, -mag, mag)


def _e4m3_bits(q):
    """values already on the OCP e4m3fn grid (oracle.clip_np.quant_e4m3's output, |q| <= 448) -> bytes; the sign of a zero is kept"""
    q = np.asarray(q, np.float64)
    a = np.abs(q)
    e = np.clip(np.floor(np.log2(np.maximum(a, 2.0 ** -20))), -6, 8)
    sub = a < 2.0 ** -6
    man = np.where(sub, a * 2.0 ** 9, (a / 2.0 ** e - 1.0) * 8.0)
    exp = np.where(sub, 0, e + 7)
    assert (man == np.round(man)).all(), "value is not on the e4m3 grid"
    return (np.where(np.signbit(q), 0x80, 0) | (exp.astype(np.int64) << 3) | man.astype(np.int64)).astype(np.uint8)


def _e4m3_values(b):
    """e4m3fn bytes -> float64 (0x7f / 0xff: NaN)"""
    b = np.asarray(b, np.uint8).astype(np.int64)
    e, m = (b >> 3) & 15, b & 7
    v = np.where(e == 0, m * 2.0 ** -9, (1.0 + m / 8.0) * 2.0 ** (e - 7.0))
    return np.where((b & 0x7F) == 0x7F, np.nan, np.where(b & 0x80, -v, v))
