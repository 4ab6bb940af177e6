"""tests/lowbits.py::quantize, the monotone round-to-nearest-even quantiser the row-kernel tests judge stored codes with, against the independent
encoders the suite already trusts (numpy's binary16, conftest.bf16_round, the searchsorted e2m1 rounding, oracle.clip_np.quant_e4m3).  No GPU."""
import numpy as np

from conftest import bf16_round
from lowbits import _GRID, _e4m3_bits, _e4m3_values, _quant_fp4, fp4_codes_signed, quantize
from oracle import clip_np


def _samples():
    rng = np.random.default_rng(7)
    x = rng.standard_normal(20000) * 10.0 ** rng.uniform(-9, 5.5, 20000)
    edge = np.array([0.0, -0.0, 2.0 ** -24, 1.5 * 2.0 ** -24, 2.0 ** -25, 2.0 ** -14, 65504.0, 65519.9, 65520.0, 7e4, 448.0, 464.0, 480.0, 1e3, 2.0 ** -9,
                     2.0 ** -10, 1.5 * 2.0 ** -9, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 5.5, 6.0, 7.0, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11])
    return np.concatenate([x, edge, -edge])


def test_quantize_matches_the_trusted_encoders():
    x = _samples()
    with np.errstate(over="ignore"):
        assert np.array_equal(quantize(x, "f16"), x.astype(np.float16).astype(np.float64))
    x32 = x.astype(np.float32).astype(np.float64)  # bf16_round takes f32: compare on values that are f32 already (no double rounding)
    assert np.array_equal(quantize(x32, "bf16"), bf16_round(x32.astype(np.float32)).astype(np.float64))
    assert np.array_equal(quantize(x, "e2m1"), _quant_fp4(x))
    q8 = quantize(x, "e4m3")
    assert np.array_equal(q8, clip_np.quant_e4m3(x))
    assert np.array_equal(_e4m3_values(_e4m3_bits(q8)), q8) and np.abs(q8).max() == 448.0


def test_quantize_is_monotone_and_idempotent():
    x = np.sort(_samples())
    for fmt in ("f16", "bf16", "e4m3", "e2m1"):
        q = quantize(x, fmt)
        assert (q[1:] >= q[:-1]).all(), fmt
        assert np.array_equal(quantize(q, fmt), q), fmt


def test_fp4_codes_keep_the_sign_of_a_zero():
    v = np.array([0.0, -0.0, -0.1, 0.1, 0.25, -0.25, 0.26, 2.5, -3.5, 100.0, -100.0])
    assert fp4_codes_signed(v).tolist() == [0, 8, 8, 0, 0, 8, 1, 4, 8 | 6, 7, 15]
    assert np.array_equal(_GRID[fp4_codes_signed(v) & 7], np.abs(quantize(v, "e2m1")))
