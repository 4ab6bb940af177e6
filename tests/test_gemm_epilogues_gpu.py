"""Every gemm256 epilogue path the product launches, one operator at a time, against float64 (arp_op_gemm_site: the product's own instances through
the tower's own routing, on device buffers).  References are built from the SAME rounded operands, so they are exact up to f32 summation and a layout
mistake shows at O(1), not inside a rounding step.  Every output lives inside a larger buffer pre-filled with a sentinel bit pattern: a stray write into
the gap between N and ldo, into rows a strided launch must skip, or a tile left unwritten, fails the test whatever the values."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import bf16_round
from lowbits import BF16, F16, _GRID, _bits16, _fp4_codes, _pack_nibbles, _quant_fp4, _unpack_nibbles, _val16

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S16 = np.uint16(0x7E5A)        # sentinel: a NaN in binary16, ~7e37 in bf16 -- neither is ever a result here
S8 = np.uint8(0xA5)
S32 = np.uint32(0x7FC0DEAD)   # an f32 NaN


# ---- host-side helpers ----------------------------------------------------------------------------------------------------------------------

def _act(x, name):
    if name.endswith("c_fc") and name.startswith("vit"):
        return x / (1.0 + np.exp(-1.702 * x))
    if name.endswith("c_fc"):
        return 0.5 * x * (1 + np.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))
    return x


def _check16(got_bits, v, noise, mode, what, stats=None):
    """The stored word must be RNE(v) everywhere, except where v lies within `noise` (f32 summation, the epilogue's own activation) of a rounding
    boundary: there the word must still be the rounding of a value within `noise` of v, on at most 1e-3 (bf16) / 2e-3 (binary16) of the entries.  (That is one ulp the other
    way wherever the value is not much smaller than its terms; on results that nearly cancel -- |v| ~ 1e-5 of sum |a||w| -- the f32 sum's absolute noise
    spans several ulps of the tiny result, and it is the noise bound, not an ulp count, that holds there.)"""
    want = _bits16(v, mode)
    bad = got_bits != want
    frac = float(bad.mean())
    if bad.any():
        gb = got_bits[bad]
        g, w, vv, nn = _val16(gb, mode), _val16(want[bad], mode), v[bad], noise[bad]
        half_ulp = 0.5 * (_val16((gb & 0x7FFF) + 1, mode) - _val16(gb & 0x7FFF, mode))
        ok = np.abs(g - vv) <= nn + half_ulp
        assert ok.all(), f"{what}: {int((~ok).sum())} stored words are not a rounding of the fp64 value (e.g. got {g[~ok][:4]} want {w[~ok][:4]} fp64 {vv[~ok][:4]})"
    # measured: bf16 1e-4 - 3.6e-4 of the words, binary16 0.9e-3 - 1.85e-3 (K = 3072) on zero-mean products (its 3 more significand bits put 8x as many results within
    # the f32 sum's noise of a midpoint); a rounding that is not to nearest moves ~1/2 of them
    cap = 2e-3 if mode == F16 else 1e-3
    assert frac <= cap, f"{what}: {frac:.2e} of the words sit a rounding step off (midpoint exceptions bounded by {cap:g})"
    if stats is not None:
        stats.append(frac)
    return frac


class _Dev:
    """device buffers of one test, freed at the end"""

    def __init__(self, lib):
        self.lib, self.bufs = lib, []

    def put(self, host, slack=4096):
        p = C.c_void_p()
        self.lib.check(self.lib.lib.arp_dev_malloc(C.byref(p), host.nbytes + slack))
        self.bufs.append(p)
        self.lib.check(self.lib.lib.arp_memcpy_h2d(p, host.ctypes.data, host.nbytes))
        return p.value

    def get(self, ptr, like):
        out = np.empty_like(like)
        self.lib.check(self.lib.lib.arp_memcpy_d2h(out.ctypes.data, C.c_void_p(ptr), out.nbytes))
        return out

    def free(self):
        for p in self.bufs:
            self.lib.lib.arp_dev_free(p)
        self.bufs = []


@pytest.fixture
def dev(gpu_lib):
    d = _Dev(gpu_lib)
    yield d
    d.free()


def _site(lib, name, mode, M, N, K, A, W, **kw):
    d = lib.GemmSite()
    d.name, d.mode, d.M, d.N, d.K, d.A, d.W = name.encode(), mode, M, N, K, A, W
    for k, v in kw.items():
        setattr(d, k, v)
    return lib.lib.arp_op_gemm_site(C.byref(d))


def _operands(mode, M, N, K, seed, a_scale=1.0):
    """A [M, K] and W [N, K] rounded to the operand type (16-bit words and their exact values), f32 bias"""
    rng = np.random.default_rng(seed)
    A = (rng.standard_normal((M, K)) * a_scale).astype(np.float32)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b = (rng.standard_normal(N) * 0.5).astype(np.float32)
    ab, wb = _bits16(A, mode), _bits16(W, mode)
    return ab, wb, _val16(ab, mode), _val16(wb, mode), b


def _rows(M, seed=0, n=384):
    """rows checked against float64 on the big shapes: the first and the last two row tiles in full, and a random sample"""
    if M <= 1024:
        return np.arange(M)
    rng = np.random.default_rng(seed)
    r = np.concatenate([np.arange(256), np.arange(max(0, (M - 1) // 256 * 256 - 256), M), rng.choice(M, n, replace=False)])
    return np.unique(r)


def _padded16(M, ld, N, fill_rows=8):
    return np.full((M + fill_rows, ld), S16, np.uint16)


def _gaps_hold(buf, M, N, what, sentinel):
    assert (buf[:M, N:] == sentinel).all(), f"{what}: stray writes between N and ldo"
    assert (buf[M:] == sentinel).all(), f"{what}: stray writes past the last row"


# ---- 1. 16-bit staged output, each production activation --------------------------------------------------------------------------------------

STAGED = [  # name, M, N, K
    ("vit.c_fc", 1, 3072, 768), ("vit.c_fc", 255, 3072, 768), ("vit.c_fc", 257, 3072, 768), ("vit.c_fc", 25600, 3072, 768),
    ("vit.qkv", 256, 2304, 768), ("vit.qkv", 257, 2304, 768), ("vit.qkv", 15420, 2304, 768), ("vit.qkv", 130, 768, 3072),
    ("vit.c_fc", 300, 520, 64), ("m3ae.c_fc", 15420, 3072, 768), ("m3ae.c_fc", 257, 3072, 768), ("m3ae.qkv", 255, 2304, 768),
    ("m3ae.c_fc", 257, 520, 3072),
]


# (one 25 600-row launch per file: f16, the labelling default)
@pytest.mark.parametrize("mode,case", [(m, c) for c in STAGED for m in (F16, BF16) if not (c[1] > 20000 and m == BF16)],
                         ids=lambda x: f"{x[0]}-{x[1]}x{x[2]}x{x[3]}" if isinstance(x, tuple) else str(x))
def test_staged_16bit_output(gpu_lib, dev, mode, case):
    name, M, N, K = case
    ab, wb, a64, w64, b = _operands(mode, M, N, K, seed=M + N + K + mode)
    ldo = N + 16 if M <= 4096 else N
    out = _padded16(M, ldo, N)
    po = dev.put(out)
    gpu_lib.check(_site(gpu_lib, name, mode, M, N, K, dev.put(ab), dev.put(wb), bias=dev.put(b), out=po, ldo=ldo))
    got = dev.get(po, out)
    _gaps_hold(got, M, N, name, S16)
    assert not (got[:M, :N] == S16).any(), f"{name}: tile(s) left unwritten"
    r = _rows(M, seed=M)
    pre = a64[r] @ w64.T + b
    v = _act(pre, name)
    # f32 summation of K terms: <= 2e-6 sum |a||w| (measured <= 3e-7 of it); the activations' exp2 / rcp approximations: <= 4e-6 |v|
    # (measured: the epilogue's QuickGELU / tanh-GELU sit within 1e-6 relative of the fp64 functions away from midpoints)
    noise = 1.2 * 2e-6 * (np.abs(a64[r]) @ np.abs(w64).T + np.abs(b)) + 4e-6 * np.abs(v) + 1e-30
    frac = _check16(got[r, :N], v, noise, mode, f"{name} {M}x{N}x{K}")
    print(f"staged {name} {M}x{N}x{K} mode {mode}: midpoint exceptions {frac:.2e}")


# ---- 2. 16-bit output on the unstaged path (N or ldo a multiple of 4, not of 8) ---------------------------------------------------------------

@pytest.mark.parametrize("mode", [F16, BF16])
@pytest.mark.parametrize("force", [1, 2])
@pytest.mark.parametrize("case", [("vit.c_fc", 300, 516, 768, 516), ("vit.qkv", 257, 512, 768, 516), ("m3ae.c_fc", 520, 772, 128, 780)])
def test_unstaged_16bit_output(gpu_lib, dev, mode, force, case):
    name, M, N, K, ldo = case
    ab, wb, a64, w64, b = _operands(mode, M, N, K, seed=N + K + force)
    out = _padded16(M, ldo, N)
    po = dev.put(out)
    gpu_lib.check(_site(gpu_lib, name, mode, M, N, K, dev.put(ab), dev.put(wb), bias=dev.put(b), out=po, ldo=ldo, force=force))
    got = dev.get(po, out)
    _gaps_hold(got, M, N, name, S16)
    v = _act(a64 @ w64.T + b, name)
    noise = 1.2 * 2e-6 * (np.abs(a64) @ np.abs(w64).T + np.abs(b)) + 4e-6 * np.abs(v) + 1e-30
    _check16(got[:M, :N], v, noise, mode, f"unstaged {name} force {force}")


# ---- 3. f32 residual in place (resid == out), ldr = ldo > N -----------------------------------------------------------------------------------

def _resid_inplace(gpu_lib, dev, name, mode, M, N, K, force, ld, seed, lda=0, rows=None, extra=None):
    """out_proj / c_proj as the tower launches them: x += A.W^T + b on the f32 residual stream x (rows `rows` of it; every other element keeps the
    sentinel).  Returns (x after, fp64 reference, tolerance) on the rows checked."""
    rows = np.arange(M) if rows is None else rows
    ab, wb, a64, w64, b = _operands(mode, M, N, K, seed=seed)
    rng = np.random.default_rng(seed + 1)
    x0 = rng.standard_normal((M, N)).astype(np.float32) * 4
    tot_rows = int(rows[-1]) + 1 + 8
    xbuf = np.full((tot_rows, ld), S32, np.uint32)
    xbuf[rows, :N] = x0.view(np.uint32)
    abuf = ab
    if lda:  # A rows at the same stride (class rows of the attention output)
        abuf = np.full((tot_rows, lda), S16, np.uint16)
        abuf[rows, :K] = ab
    px = dev.put(xbuf)
    kw = dict(bias=dev.put(b), resid=px, out=px, ldr=ld, ldo=ld, force=force, lda=lda)
    kw.update(extra or {})
    gpu_lib.check(_site(gpu_lib, name, mode, M, N, K, dev.put(abuf), dev.put(wb), **kw))
    got = dev.get(px, xbuf)
    mask = np.ones(got.shape, bool)
    mask[rows, :N] = False
    assert (got[mask] == S32).all(), f"{name}: stray writes outside the {M} rows x {N} columns it owns"
    ref = x0.astype(np.float64) + a64 @ w64.T + b
    tol = 2e-6 * (np.abs(a64) @ np.abs(w64).T + np.abs(b)) + 2e-7 * (np.abs(x0) + np.abs(ref)) + 1e-30
    return got[rows, :N].view(np.float32).astype(np.float64), ref, tol, (ab, wb, a64, w64, b, x0)


@pytest.mark.parametrize("mode", [F16, BF16])
@pytest.mark.parametrize("case", [("vit.out_proj", 300, 768, 768), ("vit.out_proj", 5000, 768, 768), ("vit.c_proj", 5000, 768, 3072),
                                  ("m3ae.c_proj", 257, 768, 3072)], ids=lambda c: f"{c[0]}-{c[1]}")
@pytest.mark.parametrize("force", [0, 2, 3])
def test_f32_residual_in_place(gpu_lib, dev, mode, case, force):
    """force 0 = the tower's own choice (out_proj at M >= 4096 goes to the two-workgroup kernel), 2 = 256 x 256 (ARP_OUT_G256=1), 3 = gemm2w"""
    name, M, N, K = case
    got, ref, tol, _ = _resid_inplace(gpu_lib, dev, name, mode, M, N, K, force, ld=N + 64, seed=M + K + force)
    err = np.abs(got - ref)
    assert (err <= tol).all(), f"{name} M={M} force {force}: max err / tol {float((err / tol).max()):.3g}"


# ---- 4. class-token-only views (tower.h, the last block): rows at stride N_tok * D ----------------------------------------------------------------

@pytest.mark.parametrize("mode", [F16, BF16])
@pytest.mark.parametrize("force", [0, 2])
@pytest.mark.parametrize("B", [60, 300])
def test_class_token_rows(gpu_lib, dev, mode, force, B):
    # the [B * N_tok, D] buffers seen at row stride N_tok * D: "row" b is sample b's N_tok tokens, its class token the first D columns; the other
    # tokens' columns must keep the sentinel
    D, ntok = 768, 50
    # out_proj: A, resid and out at row stride N_tok * D
    got, ref, tol, _ = _resid_inplace(gpu_lib, dev, "vit.out_proj", mode, B, D, D, force, ld=ntok * D, seed=B + force, lda=ntok * D)
    assert (np.abs(got - ref) <= tol).all(), float((np.abs(got - ref) / tol).max())
    # c_proj: dense A (the MLP hidden rows), resid and out at the stride
    got, ref, tol, _ = _resid_inplace(gpu_lib, dev, "vit.c_proj", mode, B, D, 4 * D, force, ld=ntok * D, seed=B + force + 7)
    assert (np.abs(got - ref) <= tol).all(), float((np.abs(got - ref) / tol).max())


# ---- 5. folded LayerNorm, consumer side -------------------------------------------------------------------------------------------------------

def _fold_weights(mode, N, D, seed):
    """W' = rn16(W diag(gamma)), c = sum_k W', d = W beta + bias -- as arp_clip.hip::load_tower (tower.h::fold_layernorm) builds them"""
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((N, D)) / np.sqrt(D)).astype(np.float32)
    gamma = (1.0 + 0.2 * rng.standard_normal(D)).astype(np.float32)
    beta = (0.1 * rng.standard_normal(D)).astype(np.float32)
    bias = (0.5 * rng.standard_normal(N)).astype(np.float32)
    wfb = _bits16((W * gamma).astype(np.float32), mode)
    wf = _val16(wfb, mode)
    c = wf.sum(1).astype(np.float32)
    d = (W.astype(np.float64) @ beta.astype(np.float64) + bias).astype(np.float32)
    return W, gamma, beta, bias, wfb, wf, c, d


def _ln_rows(M, D, seed):
    """LayerNorm inputs: ordinary rows, rows of mean 20 / std 1, near-constant rows (variance far below eps)"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((M, D)).astype(np.float32)
    x[1::3] = (20.0 + rng.standard_normal((len(x[1::3]), D))).astype(np.float32)
    x[2::7] = (5.0 + 1e-4 * rng.standard_normal((len(x[2::7]), D))).astype(np.float32)
    return x


def _stats(x):
    """per-128-column (sum, sum of squares), f32 [M, D / 128, 2]"""
    M, D = x.shape
    s = x.astype(np.float64).reshape(M, D // 128, 128)
    return np.stack([s.sum(2), (s * s).sum(2)], 2).astype(np.float32)


def _fold_consume(gpu_lib, dev, name, mode, xb, st, M, N, D, wfb, c, d, force, eps=1e-5, lda=0, pa=None, pst=None):
    ldo = N + 16
    out = _padded16(M, ldo, N)
    po = dev.put(out)
    pa = dev.put(xb) if pa is None else pa
    pst = dev.put(st) if pst is None else pst
    gpu_lib.check(_site(gpu_lib, name, mode, M, N, D, pa, dev.put(wfb), bias=dev.put(d), out=po, ldo=ldo, force=force, lda=lda,
                        ln_stats=pst, ln_c=dev.put(c), ln_parts=D // 128, ln_eps=eps))
    got = dev.get(po, out)
    _gaps_hold(got, M, N, name, S16)
    return got[:M, :N]


def _fold_exact(xb64, st, wf, c, d, eps, name):
    """the fold formula in fp64 on the same operand-type x, the same stats, the same W' / c / d, and its f32-noise bound"""
    D = xb64.shape[1]
    s, q = st[:, :, 0].astype(np.float64).sum(1), st[:, :, 1].astype(np.float64).sum(1)
    mu = s / D
    var = np.maximum(q / D - mu * mu, 0.0)
    rs = 1.0 / np.sqrt(var + eps)
    P = xb64 @ wf.T
    core = P - mu[:, None] * c.astype(np.float64)
    pre = rs[:, None] * core + d
    # f32: the product (2e-6 of its terms), mu c (c rounded to f32), and the one-pass variance (q / D - mu^2 in f32: a few ulp of q / D, which the
    # clamp and eps turn into a relative error of rs of dvar / (2 (var + eps)))
    dvar = 4 * 2.0 ** -24 * q / D
    noise = rs[:, None] * (2e-6 * (np.abs(xb64) @ np.abs(wf).T) + 2e-7 * np.abs(mu)[:, None] * np.abs(c)) + \
        np.abs(rs[:, None] * core) * (dvar / (2 * (var + eps)))[:, None] + 1e-6 * np.abs(pre)
    v = _act(pre, name)
    return v, 1.2 * noise + 4e-6 * np.abs(v) + 1e-30, rs, var, dvar


@pytest.mark.parametrize("mode", [F16, BF16])
@pytest.mark.parametrize("case", [("vit.qkv", 300, 2304, 0), ("vit.c_fc", 257, 3072, 2), ("vit.c_fc", 5000, 3072, 0)], ids=lambda c: f"{c[0]}-{c[1]}-f{c[3]}")
def test_fold_consumer(gpu_lib, dev, mode, case):
    name, M, N, force = case
    D, eps = 768, 1e-5
    x = _ln_rows(M, D, seed=M + N)
    xb = _bits16(x, mode)
    xb64 = _val16(xb, mode)
    st = _stats(x)
    W, gamma, beta, bias, wfb, wf, c, d = _fold_weights(mode, N, D, seed=N)
    got = _fold_consume(gpu_lib, dev, name, mode, xb, st, M, N, D, wfb, c, d, force, eps)
    r = _rows(M, seed=1, n=256)
    v, noise, rs, var, dvar = _fold_exact(xb64[r], st[r], wf, c, d, eps, name)
    # exact: within the stated f32 noise of the fp64 fold formula (no midpoint-fraction bound here: at mean 20 the product's terms are ~500x the result)
    gv = _val16(got[r], mode)
    err = np.abs(gv - v)
    ulp16 = np.abs(v) * (2.0 ** -11 if mode == F16 else 2.0 ** -8) + (2.0 ** -24 if mode == F16 else 1e-38)
    assert (err <= ulp16 + noise).all(), f"fold exact {name}: max (err - ulp) / noise {float(((err - ulp16) / noise).max()):.3g}"
    # semantic: against fp64 LayerNorm(x) W^T + b on the UNROUNDED x.  Inherent to the fold: x is rounded to the operand type before the mean is
    # subtracted (rs sum |xb - x||W'|), W' = rn16(W gamma) (sum |x - mu| |W' - W gamma| rs), the one-pass variance (above), the output rounding.
    x64 = x[r].astype(np.float64)
    mu_t = x64.mean(1)
    var_t = x64.var(1)
    ln = (x64 - mu_t[:, None]) / np.sqrt(var_t + eps)[:, None] * gamma + beta
    sem = _act(ln @ W.astype(np.float64).T + bias, name)
    wg = W.astype(np.float64) * gamma
    bound = rs[:, None] * (np.abs(xb64[r] - x64) @ np.abs(wf).T + np.abs(x64 - mu_t[:, None]) @ np.abs(wf - wg).T) + \
        np.abs(ln @ W.astype(np.float64).T) * np.abs(np.sqrt((var_t + eps) / (var + eps)) - 1)[:, None] + ulp16 + noise
    serr = np.abs(gv - sem)
    assert (serr <= 1.2 * bound).all(), f"fold semantic {name}: max err / bound {float((serr / bound).max()):.3g}"
    big = (np.abs(x64.mean(1)) > 10)
    const = var_t < 1e-6
    rel = serr.max(1) / np.abs(sem).max(1)
    print(f"fold {name} mode {mode}: semantic max err rel to row max: mean-20 rows {rel[big].max():.2e}, ordinary {rel[~big & ~const].max():.2e}, "
          f"near-constant {rel[const].max():.2e}; one-pass var error on near-constant rows (q/D - mu^2, f32) <= {float((dvar[const] / eps).max()):.2e} of eps")


# ---- 6. folded LayerNorm, producer side (xb_out + stats_out of the f32 residual epilogue), and producer -> consumer ---------------------------------

@pytest.mark.parametrize("mode", [F16, BF16])
@pytest.mark.parametrize("case", [("vit.out_proj", 300, 768, 0), ("vit.out_proj", 5000, 768, 0), ("vit.c_proj", 5000, 3072, 2), ("vit.out_proj", 1000, 768, 1)],
                         ids=lambda c: f"{c[0]}-{c[1]}-f{c[3]}")
def test_fold_producer(gpu_lib, dev, mode, case):
    name, M, K, force = case
    D = 768
    ldxb = D + 64
    xb = _padded16(M, ldxb, D)
    nseg = D // 128
    stb = np.full((M + 8) * nseg * 2, S32, np.uint32)
    pxb, pst = dev.put(xb), dev.put(stb)
    got, ref, tol, ops = _resid_inplace(gpu_lib, dev, name, mode, M, D, K, force, ld=D + 32, seed=M + K,
                                        extra=dict(xb_out=pxb, ldxb=ldxb, stats_out=pst))
    assert (np.abs(got - ref) <= tol).all(), float((np.abs(got - ref) / tol).max())
    out32 = got.astype(np.float32)
    gx = dev.get(pxb, xb)
    _gaps_hold(gx, M, D, "xb_out", S16)
    assert (gx[:M, :D] == _bits16(out32, mode)).all(), "xb_out is not the operand-type rounding of the f32 output"
    gs = dev.get(pst, stb)
    assert (gs[M * nseg * 2:] == S32).all(), "stats_out: stray writes past the last row"
    gs = gs[:M * nseg * 2].view(np.float32).reshape(M, nseg, 2).astype(np.float64)
    seg = out32.astype(np.float64).reshape(M, nseg, 128)
    ws, wq = seg.sum(2), (seg * seg).sum(2)
    assert (np.abs(gs[:, :, 0] - ws) <= 1e-6 * np.abs(seg).sum(2) + 1e-30).all(), "stats_out: segment sums"
    assert (np.abs(gs[:, :, 1] - wq) <= 1e-6 * wq + 1e-30).all(), "stats_out: segment sums of squares"
    if name == "vit.out_proj" and M == 5000:
        # producer -> consumer: c_fc reads the producer's xb_out / stats_out as the tower's fold does, against fp64 LayerNorm-then-GEMM of the f32 x
        N, eps = 3072, 1e-5
        W, gamma, beta, bias, wfb, wf, c, d = _fold_weights(mode, N, D, seed=5)
        g16 = _fold_consume(gpu_lib, dev, "vit.c_fc", mode, None, None, M, N, D, wfb, c, d, 0, eps, lda=ldxb, pa=pxb, pst=pst)
        r = _rows(M, seed=2, n=128)
        x64 = out32[r].astype(np.float64)
        mu_t, var_t = x64.mean(1), x64.var(1)
        sem = _act(((x64 - mu_t[:, None]) / np.sqrt(var_t + eps)[:, None] * gamma + beta) @ W.astype(np.float64).T + bias, "vit.c_fc")
        v, noise, rs, var, dvar = _fold_exact(_val16(gx[r, :D], mode), gs[r].astype(np.float32), wf, c, d, eps, "vit.c_fc")
        ulp16 = np.abs(v) * (2.0 ** -11 if mode == F16 else 2.0 ** -8)
        bound = rs[:, None] * (np.abs(_val16(gx[r, :D], mode) - x64) @ np.abs(wf).T + np.abs(x64 - mu_t[:, None]) @ np.abs(wf - W * gamma).T) + ulp16 + noise
        serr = np.abs(_val16(g16[r], mode) - sem)
        assert (serr <= 1.2 * bound).all(), f"producer -> consumer: max err / bound {float((serr / bound).max()):.3g}"


# ---- 7. split3: [hi | lo | hi] rows of the f32 result (the f16x3 encoder's c_fc -> c_proj) -----------------------------------------------------

@pytest.mark.parametrize("M", [300, 5000])
def test_split3_producer(gpu_lib, dev, M):
    N, K = 3072, 3 * 768
    ab, wb, a64, w64, b = _operands(F16, M, N, K, seed=M)
    ld3 = 3 * N + 16
    trip = _padded16(M, ld3, 3 * N)
    out = np.full((M + 8, N), S32, np.uint32)
    pt, po = dev.put(trip), dev.put(out)
    pa, pw, pb = dev.put(ab), dev.put(wb), dev.put(b)
    gpu_lib.check(_site(gpu_lib, "m3ae.x3.c_fc", F16, M, N, K, pa, pw, bias=pb, out=po, xb_out=pt, ldxb=ld3, split3=1))
    v = dev.get(po, out)[:M].view(np.float32)
    t = dev.get(pt, trip)
    _gaps_hold(t, M, 3 * N, "split3 rows", S16)
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)   # v - rn16(v) is exact in f32
    assert (t[:M, :N] == hi.view(np.uint16)).all() and (t[:M, 2 * N:3 * N] == hi.view(np.uint16)).all(), "split3: hi != rn16(v)"
    assert (t[:M, N:2 * N] == lo.view(np.uint16)).all(), "split3: lo != rn16(v - hi)"
    r = _rows(M, n=128)
    ref = _act(a64[r] @ w64.T + b, "m3ae.c_fc")
    tol = 1.2 * 2e-6 * (np.abs(a64[r]) @ np.abs(w64).T + np.abs(b)) + 4e-6 * np.abs(ref) + 1e-30
    assert (np.abs(v[r] - ref) <= tol).all()
    # the encoder's own launch: no f32 output at all, the same triples
    t2 = _padded16(M, ld3, 3 * N)
    pt2 = dev.put(t2)
    gpu_lib.check(_site(gpu_lib, "m3ae.x3.c_fc", F16, M, N, K, pa, pw, bias=pb, out=None, xb_out=pt2, ldxb=ld3, split3=1))
    assert (dev.get(pt2, t2) == t).all(), "split3 rows differ when the f32 output is not stored"


# ---- 8. fp4 side outputs of the f16c encoder's c_fc (MIXC, tanh-GELU) and the c_proj that reads them --------------------------------------------

def _weight_rows(W, plan):
    """W [N, K] f32 -> f16c weight rows [rn16(w) | fp4(dw 2^sd) (| fp4(w 2^sw))] and the restated pieces"""
    whi = W.astype(np.float16)
    w64, wh64 = W.astype(np.float64), whi.astype(np.float64)
    sd = int(np.floor(np.log2(12.0 / np.abs(w64 - wh64).max())))
    sw = int(np.floor(np.log2(12.0 / np.abs(w64).max())))
    dw4, w4 = _quant_fp4((w64 - wh64) * 2.0 ** sd), _quant_fp4(w64 * 2.0 ** sw)
    segs = [whi.view(np.uint8)]
    if plan >= 1:
        segs.append(_pack_nibbles(_fp4_codes(dw4)))
    if plan >= 2:
        segs.append(_pack_nibbles(_fp4_codes(w4)))
    return np.ascontiguousarray(np.concatenate(segs, 1)), wh64, dw4, w4, sd, sw


@pytest.mark.parametrize("plan", [1, 2])
def test_f16c_fp4_side_outputs(gpu_lib, dev, plan):
    M, D, H = 15420, 768, 3072
    rng = np.random.default_rng(plan)
    A = rng.standard_normal((M, D)).astype(np.float32)
    hi = A.astype(np.float16)
    h64 = hi.astype(np.float64)
    x4, dx4 = _quant_fp4(h64 * 2.0), _quant_fp4((A.astype(np.float64) - h64) * 2.0 ** 13)
    arows = np.concatenate([hi.view(np.uint8), _pack_nibbles(_fp4_codes(x4)), _pack_nibbles(_fp4_codes(dx4))], 1)
    arows = np.concatenate([arows, np.zeros((256, 3 * D), np.uint8)])     # the encoder's + one row tile of slack
    W1 = (rng.standard_normal((H, D)) * 0.03).astype(np.float32)
    b1 = (rng.standard_normal(H) * 0.5).astype(np.float32)
    w1rows, w1h, dw1, w1_4, sd1, sw1 = _weight_rows(W1, plan)
    # fc2's operand rows, written by fc1's epilogue: [hi: binary16 x H | x4: e2m1 x H | dx4: e2m1 x H], 3 H bytes per row
    a4h = np.full((M + 256, 3 * H), S8, np.uint8)
    p4 = dev.put(a4h)
    gpu_lib.check(_site(gpu_lib, "m3ae.f16c.c_fc", F16, M, H, D, dev.put(arows), dev.put(w1rows), bias=dev.put(b1), out=p4, ldo=3 * H // 2,
                        plan=plan, sd=sd1, sw=sw1, x4_out=p4 + 2 * H, ld4=3 * H, dx4_out=p4 + 2 * H + H // 2))
    g = dev.get(p4, a4h)
    assert (g[M:] == S8).all(), "stray writes past the last row"
    ghi = np.ascontiguousarray(g[:M, :2 * H]).view(np.uint16)
    gx4, gdx4 = _unpack_nibbles(g[:M, 2 * H:2 * H + H // 2]), _unpack_nibbles(g[:M, 2 * H + H // 2:])
    # x4 = fp4(2^x8_shift * stored binary16), exactly, nibble order included
    assert (gx4 == _quant_fp4(2.0 * _val16(ghi, F16))).all(), "x4 segment is not fp4(2 hi) of the stored tile"
    r = _rows(M, seed=3, n=256)
    pre = h64[r] @ w1h.T + 2.0 ** -(1 + sd1) * (x4[r] @ dw1.T) + b1
    if plan >= 2:
        pre = pre + 2.0 ** -(13 + sw1) * (dx4[r] @ w1_4.T)
    v = _act(pre, "m3ae.c_fc")
    noise = 1.2 * (3e-7 * (np.abs(h64[r]) @ np.abs(w1h).T) + 1e-6 * (np.abs(pre) + 1.0)) + 4e-6 * np.abs(v)
    frac = _check16(ghi[r], v, noise, F16, "f16c c_fc")
    # dx4 = fp4((v - rn16(v)) 2^13), straight from the accumulators: exact except where the f32 value's noise straddles an e2m1 boundary
    d = (v - _val16(ghi[r], F16)) * 2.0 ** 13
    e = noise * 2.0 ** 13
    want = _quant_fp4(d)
    bad = gdx4[r] != want
    okb = (gdx4[r] == _quant_fp4(d - e)) | (gdx4[r] == _quant_fp4(d + e))
    assert (okb | ~bad).all(), f"dx4: {int((bad & ~okb).sum())} codes are not fp4((v - rn16(v)) 2^13)"
    dfrac = float(bad.mean())
    assert dfrac <= 1e-2, dfrac
    # c_proj on those rows (MIXC, f32 residual in place): the restatement of test_ops_gpu::test_gemm_f16c_corrects_the_operand_roundings on what fc1 stored
    W2 = (rng.standard_normal((D, H)) * 0.02).astype(np.float32)
    b2 = (rng.standard_normal(D) * 0.5).astype(np.float32)
    w2rows, w2h, dw2, w2_4, sd2, sw2 = _weight_rows(W2, plan)
    x0 = rng.standard_normal((M, D)).astype(np.float32)
    px = dev.put(x0)
    gpu_lib.check(_site(gpu_lib, "m3ae.f16c.c_proj", F16, M, D, H, p4, dev.put(w2rows), bias=dev.put(b2), resid=px, out=px, plan=plan, sd=sd2, sw=sw2))
    got = dev.get(px, x0)[r].astype(np.float64)
    hh = _val16(ghi[r], F16)
    want2 = hh @ w2h.T + 2.0 ** -(1 + sd2) * (gx4[r] @ dw2.T) + b2 + x0[r]
    if plan >= 2:
        want2 = want2 + 2.0 ** -(13 + sw2) * (gdx4[r] @ w2_4.T)
    tol = 3e-7 * (np.abs(hh) @ np.abs(w2h).T) + 1e-6 * (np.abs(want2) + 1.0)
    assert (np.abs(got - want2) <= tol).all(), float((np.abs(got - want2) / tol).max())
    print(f"f16c c_fc plan {plan}: binary16 midpoint exceptions {frac:.2e}, dx4 boundary cases {dfrac:.2e}")


# ---- 9. launch routes -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [F16, BF16])
def test_routes_agree(gpu_lib, dev, mode):
    """force 1 (128 x 128) / 2 (256 x 256) / 3 (gemm2w) / 0 (auto) against fp64; the 128 and 256 kernels bit for bit (gemm256.h: "same MFMA, same k order,
    same epilogue arithmetic"), as gemm2w and gemm256 for out_proj (tower.h)"""
    outs = {}
    for name, M, N, K in (("vit.qkv", 5000, 2304, 768), ("vit.out_proj", 5000, 768, 768)):
        for force in (0, 1, 2, 3):
            if name == "vit.qkv":
                ab, wb, a64, w64, b = _operands(mode, M, N, K, seed=11)
                out = _padded16(M, N, N)
                po = dev.put(out)
                gpu_lib.check(_site(gpu_lib, name, mode, M, N, K, dev.put(ab), dev.put(wb), bias=dev.put(b), out=po, force=force))
                got = dev.get(po, out)
                _gaps_hold(got, M, N, name, S16)
                r = _rows(M, seed=4, n=128)
                v = a64[r] @ w64.T + b
                _check16(got[r, :N], v, 1.2 * 2e-6 * (np.abs(a64[r]) @ np.abs(w64).T + np.abs(b)) + 1e-30, mode, f"{name} force {force}")
                outs[name, force] = got[:M]
            else:
                got, ref, tol, _ = _resid_inplace(gpu_lib, dev, name, mode, M, N, K, force, ld=N, seed=12)
                assert (np.abs(got - ref) <= tol).all(), (force, float((np.abs(got - ref) / tol).max()))
                outs[name, force] = got
    for name in ("vit.qkv", "vit.out_proj"):
        assert (outs[name, 1] == outs[name, 2]).all(), f"{name}: the 128 and 256 kernels differ"
    assert (outs["vit.out_proj", 2] == outs["vit.out_proj", 3]).all(), "out_proj: gemm2w and the 256 kernel differ"


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gemm_epilogues_gpu as T
from arp_amd import _ffi
d = T._Dev(_ffi)
res = {}
for name, mode, M, N, K, force in (("vit.c_fc", 2, 15420, 3072, 768, 0), ("vit.qkv", 1, 25600, 2304, 768, 2), ("vit.c_proj", 2, 25600, 768, 3072, 2),
                                   ("vit.out_proj", 1, 25600, 768, 768, 2)):
    ab, wb, a64, w64, b = T._operands(mode, M, N, K, seed=M + N)
    if name.endswith("proj"):
        x = np.random.default_rng(1).standard_normal((M, N)).astype(np.float32)
        px = d.put(x)
        _ffi.check(T._site(_ffi, name, mode, M, N, K, d.put(ab), d.put(wb), bias=d.put(b), resid=px, out=px, force=force))
        res[name] = d.get(px, x).view(np.uint32)
    else:
        out = np.full((M, N), T.S16, np.uint16)
        po = d.put(out)
        _ffi.check(T._site(_ffi, name, mode, M, N, K, d.put(ab), d.put(wb), bias=d.put(b), out=po, force=force))
        res[name] = d.get(po, out)
    d.free()
np.savez(sys.argv[2], **{k.replace(".", "_"): v for k, v in res.items()})
"""


def test_route_switches_bitwise(gpu_lib, tmp_path):
    """ARP_GEMM_SPLITM / ARP_GEMM_PERSIST / ARP_GEMM_GROUP_M are read once per process (function-local statics): each runs in a fresh child process,
    one at a time, on grids of 300-1 000 tiles (persistence walks several tiles per workgroup; c_proj / out_proj at 25 600 rows = 300 tiles is the
    split-M shape: one full round + 44 tiles), and must give the default route's bits, 16-bit staged output included."""
    runs = {}
    for tag, env in (("default", {}), ("splitm", {"ARP_GEMM_SPLITM": "1"}), ("persist", {"ARP_GEMM_PERSIST": "1"}), ("groupm", {"ARP_GEMM_GROUP_M": "3"})):
        e = dict(os.environ)
        for k in ("ARP_GEMM_SPLITM", "ARP_GEMM_PERSIST", "ARP_GEMM_GROUP_M", "ARP_GEMM_TPW", "ARP_OUT_G256"):
            e.pop(k, None)
        e.update(env)
        f = tmp_path / f"{tag}.npz"
        p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(f)], env=e, timeout=300, capture_output=True, text=True)
        assert p.returncode == 0, f"{tag}: child exited {p.returncode}\n{p.stderr[-2000:]}"
        runs[tag] = np.load(f)
    base = runs["default"]
    for k in base.files:
        assert not (base[k] == S16).any() if base[k].dtype == np.uint16 else True, f"{k}: tiles left unwritten on the default route"
    for tag in ("splitm", "persist", "groupm"):
        for k in base.files:
            assert (runs[tag][k] == base[k]).all(), f"{tag}: {k} differs from the default route ({int((runs[tag][k] != base[k]).sum())} words)"


# ---- host-side refusals: what the epilogues would silently skip ------------------------------------------------------------------------------

def test_launchers_refuse_what_the_epilogue_would_skip(gpu_lib, dev):
    """Side outputs and the fold consumer are computed on the staged epilogues only; stats_out needs N % 128.  Each case must be refused by the
    launcher on the host (buffers are sized so that nothing could land out of bounds even if a refusal were missing)."""
    M, K = 64, 768
    big = np.zeros(4 * 1024 * 1024, np.uint32)
    pa, pw, pb, po, px, ps = (dev.put(big) for _ in range(6))
    for force in (1, 2):
        # f32 producer with an xb_out / stats_out on an unstaged shape (N % 8 != 0)
        assert _site(gpu_lib, "vit.out_proj", F16, M, 516, K, pa, pw, bias=pb, resid=po, out=po, xb_out=px, ldxb=516, force=force) != 0
        assert _site(gpu_lib, "vit.out_proj", F16, M, 768, K, pa, pw, bias=pb, resid=po, out=po, ldo=772, ldr=772, stats_out=ps, force=force) != 0
        # stats_out on N % 128 != 0
        assert _site(gpu_lib, "vit.out_proj", F16, M, 384 + 8, K, pa, pw, bias=pb, resid=po, out=po, stats_out=ps, force=force) != 0
        # the fold consumer on an unstaged shape
        assert _site(gpu_lib, "vit.c_fc", BF16, M, 516, K, pa, pw, bias=pb, out=po, ln_stats=ps, ln_c=pb, ln_parts=6, ln_eps=1e-5, force=force) != 0
        # split3 on the unstaged path
        assert _site(gpu_lib, "m3ae.x3.c_fc", F16, M, 516, K, pa, pw, bias=pb, out=po, xb_out=px, ldxb=3 * 516, split3=1, force=force) != 0
    # fp4 side outputs of the MIXC c_fc with an output stride off the staged path
    assert _site(gpu_lib, "m3ae.f16c.c_fc", F16, M, 3072, K, pa, pw, bias=pb, out=po, ldo=3 * 3072 // 2 + 4, plan=1, sd=8, sw=4,
                 x4_out=px, ld4=3 * 3072) != 0
    # ... and an fp4 side output asked of an instance that has none
    assert _site(gpu_lib, "m3ae.f16c.c_proj", F16, M, 768, 3072, pa, pw, bias=pb, resid=po, out=po, plan=1, sd=8, sw=4, x4_out=px, ld4=3 * 768) != 0
    # the unchanged in-domain launches still go through
    gpu_lib.check(_site(gpu_lib, "vit.out_proj", F16, M, 768, K, pa, pw, bias=pb, resid=po, out=po, xb_out=px, ldxb=768, stats_out=ps))
