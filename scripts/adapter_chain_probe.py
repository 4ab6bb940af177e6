#!/usr/bin/env python3
"""The corrected adapter INSIDE the policy step, piece by piece (round 6).  scripts/policy_floor_probe2.py: the unit-tested product (arp_op_gemm_f16c) chained on the
host leaves 1.1e-4 on the logits, as the fp64 emulation says it should; the same two products inside the step leave 3.6e-4.  Which piece?  After one forward
(plan 22e, B = 2, real geometry) the step's device buffers are read back (arp_dt_debug_read) and every segment is restated on the host from the layer before it:

  Xc   = [rn16(x) | fp4(2 rn16(x)) | fp4(2^13 (x - rn16(x)))]               from the encodings
  W1c  = [rn16(w) | fp4(2^sd (w - rn16(w))) | fp4(2^sw w)]                  from the parameter, scales as the device chose them
  H1c  = the same three segments of relu(fc1) where fc1 is the float64 product of the Xc / W1c AS READ BACK (+ bias)
  A32  = relu(float64 product of H1c / W2c as read back + bias)

    python scripts/adapter_chain_probe.py      (needs a GPU; test infrastructure: uses the oracle's parameter generator only)
"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("ARP_DT_ADAPTER_PLAN", "22e")
from arp_amd import _ffi, synth_policy as S  # noqa: E402
from arp_amd.train import PolicyConfig, PolicyTrainer  # noqa: E402

GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
DEC = np.concatenate([GRID, -GRID])  # code -> value (bit 3 = sign)


def q4(x):
    x = np.asarray(x, np.float64)
    a = np.minimum(np.abs(x), 6.0)
    idx = np.clip(np.searchsorted(GRID, a, side="left"), 1, 7)
    lo, hi = GRID[idx - 1], GRID[idx]
    mid = 0.5 * (lo + hi)
    up = (a > mid) | ((a == mid) & (idx % 2 == 0))
    return np.sign(x) * np.where(up, hi, lo)


def read(tr, name, nbytes):
    buf = np.empty(nbytes, np.uint8)
    n = _ffi.lib.arp_dt_debug_read(tr._h, name.encode(), buf.ctypes.data_as(C.c_void_p), nbytes)
    assert n >= nbytes, (name, n, nbytes)
    return buf


def rows(buf, M, D):
    """[M, 3 D bytes] -> hi [M, D] float64, seg1 [M, D], seg2 [M, D] (decoded e2m1 values, unscaled)"""
    b = buf[: M * 3 * D].reshape(M, 3 * D)
    hi = b[:, : 2 * D].copy().view(np.float16).astype(np.float64)

    def seg(x):
        lo, hi4 = x & 15, x >> 4
        out = np.empty((M, D), np.float64)
        out[:, 0::2] = DEC[lo]
        out[:, 1::2] = DEC[hi4]
        return out
    return hi, seg(b[:, 2 * D: 2 * D + D // 2]), seg(b[:, 2 * D + D // 2:])


def report(name, got, want, tol=0.0):
    d = np.abs(got - want)
    bad = d > tol
    print(f"{name:34s} differing {int(bad.sum()):9d} of {got.size:9d} ({bad.mean():.2e})   max |diff| {d.max():.3e}   rms {np.sqrt((d ** 2).mean()):.3e}", flush=True)


cfg = PolicyConfig(lambda_ret=0.01)
D = cfg.enc_dim
P = S.policy_params(cfg, seed=100)
enc, act, rtg = S.policy_batch(cfg, 2, seed=101)
M = enc.size // D
x = enc.reshape(M, D).astype(np.float64)
tr = PolicyTrainer(cfg, mode="f16", adapter_corrections=True)
tr.set_params(P)
tr.set_batch(enc, act, rtg)
tr.forward()
sc = read(tr, "wc_scal", 64).view(np.int32)
print("device scales: W1 sd, sw =", sc[4], sc[5], "  W2 sd, sw =", sc[12], sc[13])
Xc = rows(read(tr, "Xc", M * 3 * D), M, D)
H1c = rows(read(tr, "H1c", M * 3 * D), M, D)
W1c = rows(read(tr, "W1c", D * 3 * D), D, D)
W2c = rows(read(tr, "W2c", D * 3 * D), D, D)
A32 = read(tr, "A32", M * D * 4).view(np.float32).reshape(M, D).astype(np.float64)
W1 = np.asarray(P["AdapterMLP_0/Dense_0/kernel"]).astype(np.float64)  # Flax layout [in, out]
W2 = np.asarray(P["AdapterMLP_0/Dense_1/kernel"]).astype(np.float64)
b1, b2 = P["AdapterMLP_0/Dense_0/bias"].astype(np.float64), P["AdapterMLP_0/Dense_1/bias"].astype(np.float64)

h16 = lambda a: a.astype(np.float16).astype(np.float64)  # noqa: E731
print("== the encodings' operand rows")
report("Xc hi  vs rn16(x)", Xc[0], h16(x))
report("Xc x4  vs fp4(2 hi)", Xc[1], q4(2.0 * h16(x)))
report("Xc dx4 vs fp4(2^13 (x - hi))", Xc[2], q4((x - h16(x)) * 2.0 ** 13))
for nm, Wc, W, sd, sw in (("W1c", W1c, W1, sc[4], sc[5]), ("W2c", W2c, W2, sc[12], sc[13])):
    Wt = W.T  # rows = outputs
    if (Wc[0] != h16(Wt)).mean() > 0.5 and (Wc[0] != h16(W)).mean() < 0.5:
        print(f"   !! {nm}'s rows are the Flax kernel's ROWS (inputs), not its columns")
        Wt = W
    print(f"== {nm} (max |dw| 2^sd = {np.abs(Wt - h16(Wt)).max() * 2.0 ** sd:.2f}, max |w| 2^sw = {np.abs(Wt).max() * 2.0 ** sw:.2f}: both in (6, 12] as designed?)")
    report(f"{nm} hi  vs rn16(w)", Wc[0], h16(Wt))
    report(f"{nm} dW4 vs fp4(2^sd dw)", Wc[1], q4((Wt - h16(Wt)) * 2.0 ** sd))
    report(f"{nm} W4  vs fp4(2^sw w)", Wc[2], q4(Wt * 2.0 ** sw))


def product(Ac, Wc, sd, sw):
    return Ac[0] @ Wc[0].T + 2.0 ** -(1 + sd) * (Ac[1] @ Wc[1].T) + 2.0 ** -(13 + sw) * (Ac[2] @ Wc[2].T)


print("== fc1 (the float64 product of the segments as read back)")
v1 = np.maximum(product(Xc, W1c, sc[4], sc[5]) + b1, 0.0)
report("H1c hi  vs rn16(relu(fc1))", H1c[0], h16(v1), tol=0.0)
report("  ... allowing one binary16 ulp", H1c[0], h16(v1), tol=2.0 ** -10 * np.maximum(np.abs(v1), 2.0 ** -14))
report("H1c x4  vs fp4(2 hi)", H1c[1], q4(2.0 * H1c[0]))
report("H1c dx4 vs fp4(2^13 (v - hi))", H1c[2], q4((v1 - H1c[0]) * 2.0 ** 13))
if (H1c[1] != q4(2.0 * H1c[0])).mean() > 0.01:  # which mistake?
    want = q4(2.0 * H1c[0])
    print("   row 0, columns 0..31   hi :", " ".join(f"{v:6.3f}" for v in H1c[0][0, :32]))
    print("   row 0, columns 0..31 want :", " ".join(f"{v:6.1f}" for v in want[0, :32]))
    print("   row 0, columns 0..31  got :", " ".join(f"{v:6.1f}" for v in H1c[1][0, :32]))
    for nm, alt in (("fp4(hi)", q4(H1c[0])), ("fp4(4 hi)", q4(4.0 * H1c[0])), ("fp4(hi / 2)", q4(0.5 * H1c[0])), ("pairs swapped", want.reshape(M, D // 2, 2)[:, :, ::-1].reshape(M, D)),
                    ("bytes reversed within a dword", want.reshape(M, D // 8, 4, 2)[:, :, ::-1, :].reshape(M, D)), ("fp4(2 v) (unrounded)", q4(2.0 * v1)),
                    ("dwords of a 16-byte group reversed", want.reshape(M, D // 32, 4, 8)[:, :, ::-1, :].reshape(M, D)), ("columns + 8", np.roll(want, 8, axis=1)), ("columns - 8", np.roll(want, -8, axis=1)),
                    ("the row before", np.roll(want, 1, axis=0)), ("the row after", np.roll(want, -1, axis=0)), ("the row 16 before", np.roll(want, 16, axis=0))):
        print(f"   hypothesis {nm:36s}: differing {(H1c[1] != alt).mean():.3e}")
print("   (dx4 from the restated v: f32 summation noise moves a code here and there; a systematic error shows as a large fraction)")
exact1 = np.maximum(x @ W1 + b1, 0.0)
rec1 = H1c[0] + 2.0 ** -13 * H1c[2]
print(f"   hidden rows: rms error of hi alone {np.sqrt(((H1c[0] - exact1) ** 2).mean()):.3e}, of hi + 2^-13 dx4 {np.sqrt(((rec1 - exact1) ** 2).mean()):.3e}, of the restated v {np.sqrt(((v1 - exact1) ** 2).mean()):.3e}")
print("== fc2")
v2 = np.maximum(product(H1c, W2c, sc[12], sc[13]) + b2, 0.0)
report("A32 vs relu(fc2 of the segments)", A32, v2, tol=1e-5)
exact2 = np.maximum(exact1 @ W2 + b2, 0.0)
plain = np.maximum(h16(np.maximum(h16(x) @ h16(W1) + b1, 0.0)) @ h16(W2) + b2, 0.0)
print(f"   adapter output: rms error of A32 {np.sqrt(((A32 - exact2) ** 2).mean()):.3e}, of the restated product {np.sqrt(((v2 - exact2) ** 2).mean()):.3e}, of the plain binary16 products "
      f"{np.sqrt(((plain - exact2) ** 2).mean()):.3e}, of one binary16 rounding of the exact output {np.sqrt(((h16(exact2) - exact2) ** 2).mean()):.3e}")
tr.close()
