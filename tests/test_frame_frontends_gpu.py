"""The kernels that turn frames into a tower's first operand, one at a time, in every instance and output form the passes launch.

Bicubic (csrc/preprocess.h through arp_op_preprocess_forms): integer arithmetic, Pillow-exact by construction, a lookup table for the normalisation -- every
stored word must EQUAL oracle.preprocess.preprocess re-laid patch-major and rounded once to the mode's type.  Each case also pins which kernel template
launch_preprocess picked and the tile build_plan settled on (the entry's info[]): a geometry that stopped reaching its instance fails, it does not pass as
one more run of preprocess_fast_kernel<5>.  The table's values are build_plan's arithmetic restated by hand (Pillow's tap windows, the LDS carve, the
52 KiB budget), not read back from the library.
crop_u8_kernel and the M3AE patchify kernels only move (and round) data: equality.
preprocess_bilinear_kernel is f32 arithmetic: the one bound of this module, derived at test_bilinear."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before the library's first HIP call: arp_amd/_ffi.py, process hygiene)

from conftest import TINY
from lowbits import BF16, F16, _bits16, _val16, quantize

pytestmark = pytest.mark.gpu

F32 = 0
MODE_NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
PATCH_MAJOR, NCHW = 0, 1
FILL = 0x5A
GENERIC = 0
COS_TOL_F32 = 1e-4   # tests/test_clip_gpu.py

_FRAMES, _REF = {}, {}


def _u8p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _frames(H, W):
    """one noise frame, one blocky frame (frame-index arithmetic needs two; flat colour hides index slips, noise does not); shared, read-only"""
    if (H, W) not in _FRAMES:
        from arp_amd import synth
        fr = np.concatenate([synth.noise_frames(1, H, W, seed=H * 7 + W), synth.procgen_like_frames(1, H, W, seed=3)])
        fr.setflags(write=False)
        _FRAMES[(H, W)] = fr
    return _FRAMES[(H, W)]


def _oracle(H, W, crop, res):
    """oracle.preprocess on _frames(H, W): f32 NCHW, computed once per geometry, read-only"""
    key = (H, W, crop, res)
    if key not in _REF:
        from oracle import preprocess as P
        r = P.preprocess(_frames(H, W), use_crop=bool(crop), n_px=res)
        r.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def _patch_major(nchw, P):
    """[n, 3, R, R] -> [(f G + oy // P) G + ox // P, c P^2 + (oy % P) P + ox % P]"""
    n, _, R, _ = nchw.shape
    G = R // P
    return np.ascontiguousarray(nchw.reshape(n, 3, G, P, G, P).transpose(0, 2, 4, 1, 3, 5).reshape(n * G * G, 3 * P * P))


def _words(x, mode):
    """f32 values -> the words the mode stores (one round-to-nearest-even for the 16-bit types)"""
    return np.ascontiguousarray(x, np.float32).view(np.uint32) if mode == F32 else _bits16(x, mode)


def _expected(H, W, crop, res, patch, mode, layout):
    ref = _oracle(H, W, crop, res)
    return _words(ref if layout == NCHW else _patch_major(ref, patch), mode)


def _run_forms(lib, fr, crop, res, patch, mode, layout, tr_start):
    """-> (rc, the returned buffer as the mode's words, info)"""
    n, H, W, _ = fr.shape
    buf = np.full(n * 3 * res * res * (4 if mode == F32 else 2), FILL, np.uint8)
    info = np.full(8, -1, np.int32)
    rc = lib.lib.arp_op_preprocess_forms(_u8p(fr), n, H, W, int(crop), res, patch, mode, layout, tr_start, _vp(buf),
                                         info.ctypes.data_as(C.POINTER(C.c_int32)))
    return rc, buf.view(np.uint32 if mode == F32 else np.uint16), info


def _assert_equal_words(got, want, what):
    got, want = got.reshape(-1), want.reshape(-1)
    assert got.shape == want.shape, f"{what}: {got.size} words returned, {want.size} expected"
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"{what}: {bad.size} of {want.size} words differ, first at flat index {bad[0]}: stored {int(got[bad[0]]):#x}, "
                           f"expected {int(want[bad[0]]):#x}")


def _vector_staging(H, W, crop):
    """the kernels stage input rows with 16-byte loads when nothing is cropped off a row and rows and frames are multiples of 16 bytes"""
    cw = W // 2 if crop else W
    return int(cw == W and (cw * 3) % 16 == 0 and (H * W * 3) % 16 == 0)


def _check_info(info, inst, TR, kmax, res, H, W, crop, what, budget_kb=52):
    inst_got, TR_got, kh, kv, max_rows, lds, vec, tiles = (int(v) for v in info)
    print(f"{what}: instance {'generic' if inst_got == 0 else 'fast<%d>' % inst_got}, TR {TR_got}, kmax {kh}/{kv}, max_rows {max_rows}, lds {lds} B, "
          f"{'16-byte' if vec else 'byte'} staging, {tiles} tiles/frame, last tile {res - (tiles - 1) * TR_got} rows, tap table {TR_got * (1 + kv)} entries")
    assert (inst_got, TR_got) == (inst, TR), f"{what}: reached instance {inst_got} at TR {TR_got}, the case is there for instance {inst} at TR {TR}"
    assert (kh, kv) == (kmax, kmax), f"{what}: longest filters {kh}/{kv}, expected {kmax}"
    assert vec == _vector_staging(H, W, crop), f"{what}: staging path"
    assert tiles == -(-res // TR) and 0 < lds <= budget_kb * 1024 and max_rows >= kv


def _check_case(lib, H, W, crop, res, inst, TR, kmax, tr_start, forms, what, budget_kb=52):
    fr = _frames(H, W)
    for patch, mode, layout in forms:
        w = f"{what} {MODE_NAME[mode]} {'NCHW' if layout == NCHW else 'patch %d' % patch} tr_start {tr_start}"
        rc, got, info = _run_forms(lib, fr, crop, res, patch, mode, layout, tr_start)
        lib.check(rc)
        _check_info(info, inst, TR, kmax, res, H, W, crop, w, budget_kb)
        _assert_equal_words(got, _expected(H, W, crop, res, patch, mode, layout), w)
    return info


# ---- bicubic, res 224 ------------------------------------------------------------------------------------------------------------------------------------
# name -> (H, W, crop, instance, kmax, TR from tr_start 32, TR from tr_start 8)
GEOM = {
    "256x256": (256, 256, 0, 5, 5, 16, 8),            # vector staging, unrolled copy loop; the shipped case
    "256x256-crop": (256, 256, 1, 5, 4, 32, 8),       # cx != 0: byte staging; kmax 4 < KT (zero-padded taps)
    "64x64": (64, 64, 0, 5, 4, 32, 8),                # upsampling, short staging loop only
    "200x300": (200, 300, 0, 5, 4, 16, 8),            # non-zero `left` into the tables
    "300x200": (300, 200, 0, 5, 4, 32, 8),            # non-zero `top`
    "288x288": (288, 288, 0, 6, 6, 16, 8),
    "320x320": (320, 320, 0, 6, 6, 8, 8),             # TR cut by the LDS budget
    "400x400": (400, 400, 0, 8, 8, 8, 8),
    "448x448": (448, 448, 0, 8, 8, 4, 4),
    "512x512": (512, 512, 0, GENERIC, 10, 4, 4),      # the reference's frame size under the default transform: kmax 10
    "64x66": (64, 66, 0, GENERIC, 4, 32, 8),          # 198-byte rows: byte staging in the generic kernel
    "132x132-crop": (132, 132, 1, GENERIC, 4, 32, 8), # crop 66: crop and misaligned rows
}
ALL_FORMS = [(p, m, PATCH_MAJOR) for m in (F32, BF16, F16) for p in (16, 32)] + [(16, F32, NCHW)]
TWO_FORMS = [(16, F16, PATCH_MAJOR), (16, F32, NCHW)]
EVERY_FORM = ("256x256", "320x320", "448x448", "512x512")
BICUBIC = [(name, t) for name, g in GEOM.items() for t in ((32, 8) if g[5] != g[6] else (32,))]


@pytest.mark.parametrize("name,tr_start", BICUBIC, ids=[f"{n}-tr{t}" for n, t in BICUBIC])
def test_bicubic_instances_and_forms(gpu_lib, name, tr_start):
    H, W, crop, inst, kmax, tr32, tr8 = GEOM[name]
    _check_case(gpu_lib, H, W, crop, 224, inst, tr32 if tr_start == 32 else tr8, kmax, tr_start, ALL_FORMS if name in EVERY_FORM else TWO_FORMS, name)


def test_bicubic_cases_cover_every_path():
    """the table above, read as a whole: all four instances, both staging paths under a fast and under the generic instance, TR 32, 16, 8 and 4"""
    assert {g[3] for g in GEOM.values()} == {GENERIC, 5, 6, 8}
    for fast in (True, False):
        assert {_vector_staging(g[0], g[1], g[2]) for g in GEOM.values() if (g[3] != GENERIC) == fast} == {0, 1}
    assert {t for g in GEOM.values() for t in g[5:7]} == {32, 16, 8, 4}


@pytest.mark.parametrize("name,inst,kmax", [("256x256", 5, 5), ("400x400", 8, 8)])
def test_bicubic_generic_switch(gpu_lib, monkeypatch, name, inst, kmax):
    """ARP_PREPROCESS_GENERIC=1 sends a geometry of a fast instance to the generic kernel: the same plan, the same words"""
    H, W, crop = GEOM[name][:3]
    _check_case(gpu_lib, H, W, crop, 224, inst, GEOM[name][5], kmax, 32, TWO_FORMS, name + " (switch unset)")
    monkeypatch.setenv("ARP_PREPROCESS_GENERIC", "1")
    _check_case(gpu_lib, H, W, crop, 224, GENERIC, GEOM[name][5], kmax, 32, ALL_FORMS, name + " ARP_PREPROCESS_GENERIC=1")


@pytest.mark.parametrize("kb,TR,max_rows", [(24, 4, None), (80, 32, 40)])
def test_bicubic_lds_budget_switch(gpu_lib, monkeypatch, kb, TR, max_rows):
    """ARP_PRE_LDS_KB moves the budget build_plan shrinks TR under: 24 KiB leaves 256 -> 224 four rows per workgroup, 80 KiB the whole tr_start of 32
    (40 input rows; 66 880 bytes of LDS, past the 64 KiB a kernel gets without asking)"""
    monkeypatch.setenv("ARP_PRE_LDS_KB", str(kb))
    _check_case(gpu_lib, 256, 256, 0, 224, 5, TR, 5, 32, ALL_FORMS, f"256x256 ARP_PRE_LDS_KB={kb}", budget_kb=kb)
    if max_rows is not None:
        _, _, info = _run_forms(gpu_lib, _frames(256, 256), 0, 224, 16, F32, PATCH_MAJOR, 32)
        assert int(info[4]) == max_rows and int(info[5]) > 64 * 1024


# ---- ragged last tile and the tap-table copy past 256 entries, at small res ----------------------------------------------------------------------------------
# (res, side, instance, kmax, rows of the last tile): every TR the plan reaches divides 224, so a last tile of fewer than TR rows needs another res; the LDS
# these need is small, so TR stays at tr_start.  kmax 8 at TR 32: a tap table of 32 (1 + 8) = 288 entries, past the 256 the fast kernel's prologue copies at once
SMALL = [(40, 80, 8, 8, 8), (40, 60, 6, 6, 8), (40, 48, 5, 5, 8), (40, 50, GENERIC, 5, 8), (48, 96, 8, 8, 16), (32, 64, 8, 8, 32)]
SMALL_FORMS = [(8, F32, PATCH_MAJOR), (8, BF16, PATCH_MAJOR), (8, F16, PATCH_MAJOR), (8, F32, NCHW)]


@pytest.mark.parametrize("res,side,inst,kmax,last", SMALL, ids=[f"{c[1]}to{c[0]}" for c in SMALL])
def test_bicubic_ragged_tile_and_long_tap_table(gpu_lib, res, side, inst, kmax, last):
    info = _check_case(gpu_lib, side, side, 0, res, inst, 32, kmax, 32, SMALL_FORMS, f"{side}x{side} -> {res}")
    assert res - (int(info[7]) - 1) * int(info[1]) == last
    if kmax == 8:
        assert int(info[1]) * (1 + int(info[3])) == 288
    _check_case(gpu_lib, side, side, 0, res, inst, 8, kmax, 8, SMALL_FORMS[:1], f"{side}x{side} -> {res}")


def test_bicubic_refusals(gpu_lib):
    """each refusal is an error that leaves the output alone, and the next valid call is still exact"""
    def refused(fr, crop, res, patch, mode, layout, needle):
        rc, got, _ = _run_forms(gpu_lib, fr, crop, res, patch, mode, layout, 32)
        assert rc != 0 and needle in gpu_lib.last_error(), (rc, gpu_lib.last_error())
        assert (got.view(np.uint8) == FILL).all()
        _check_case(gpu_lib, 64, 64, 0, 224, 5, 32, 4, 32, TWO_FORMS[:1], "64x64 after a refusal")

    fr = _frames(64, 64)
    refused(fr, 0, 30, 30, F32, NCHW, "patch")                                   # res % 4
    refused(fr, 0, 24, 6, F32, PATCH_MAJOR, "patch")                             # patch % 4
    refused(fr, 0, 224, 16, F16, NCHW, "NCHW")                                   # a form no pass launches
    refused(np.zeros((1, 100, 256, 3), np.uint8), 1, 224, 16, F32, PATCH_MAJOR, "use_crop needs H >= W/2")
    refused(_frames(512, 512), 0, 32, 8, F32, PATCH_MAJOR, "too wide for the LDS tile")   # 64 taps per axis: not even one output row fits


@pytest.mark.parametrize("side", [512, 400])
def test_bicubic_generic_and_fast8_through_the_handle(gpu_lib, side):
    """the labelling pass itself on the reference's 512 x 512 frames (generic kernel, TR 4) and on 400 x 400 (fast<8>), no crop: plan cache included"""
    from arp_amd import clip, synth
    from oracle import clip_np as CN
    ocfg = CN.ClipConfig(**TINY)
    Wt = synth.clip_weights(ocfg, seed=31)
    fr = np.concatenate([synth.noise_frames(1, side, side, seed=side), synth.procgen_like_frames(2, side, side, seed=5)])
    tok = synth.prompt_tokens(2, [7, 3], ctx=ocfg.ctx, vocab=ocfg.vocab, seed=33)
    ref = CN.compute_reward(Wt, ocfg, fr, tok)
    m = clip.ClipLabeller(clip.ClipConfig(**TINY), Wt, mode="f32").set_text(tok)
    scale = float(np.exp(Wt["logit_scale"]))
    for _ in range(2):   # the second call takes the plan from the handle's cache
        err = np.abs(m.label(fr) - ref).max() / scale
        print(f"{side}x{side} through ClipLabeller f32: cosine err {err:.2e} (bar {COS_TOL_F32})")
        assert err < COS_TOL_F32
    m.close()


# ---- bilinear (the fine-tune transform) -----------------------------------------------------------------------------------------------------------------------
U = 2.0 ** -24
MEAN = np.array([0.48145466, 0.4578275, 0.40821073], np.float32)
STD = np.array([0.26862954, 0.26130258, 0.27577711], np.float32)
DELTA_ARITH = (7 * 2.0 ** -16 / 255 + 2 * U) / float(STD.min()) + 4 * U
BILINEAR = [(448, 448, True), (112, 112, True), (448, 112, True), (224, 224, True),      # scale a power of two (224: no resize at all)
            (64, 64, False), (256, 256, False), (300, 200, False), (50, 44, False)]
_BIL = {}


def _bilinear_refs(H, W, R=224):
    """(float64 restatement of the kernel's formula, torch's own transform), both NCHW, once per geometry"""
    if (H, W) in _BIL:
        return _BIL[(H, W)]
    from oracle import clip_torch as CT
    fr = _frames(H, W)
    f32 = np.float32

    def axis(size):   # source coordinate and weights in f32 operations, in the kernel's order
        s = f32(size) / f32(R)
        f = np.maximum((np.arange(R, dtype=f32) + f32(0.5)) * s - f32(0.5), f32(0))
        i0 = f.astype(np.int64)
        w1 = f - i0.astype(f32)
        return i0, i0 + (i0 < size - 1), (f32(1) - w1).astype(np.float64), w1.astype(np.float64)

    x = fr.astype(np.float64)
    if H != R and W != R:
        y0, y1, h0, h1 = axis(H)
        x0, x1, w0, w1 = axis(W)
        top = x[:, y0][:, :, x0] * w0[None, None, :, None] + x[:, y0][:, :, x1] * w1[None, None, :, None]
        bot = x[:, y1][:, :, x0] * w0[None, None, :, None] + x[:, y1][:, :, x1] * w1[None, None, :, None]
        x = top * h0[None, :, None, None] + bot * h1[None, :, None, None]
    v = ((x / 255.0 - MEAN.astype(np.float64)) / STD.astype(np.float64)).transpose(0, 3, 1, 2)
    t = CT.finetune_transform(fr.copy()).numpy().astype(np.float64)
    v.setflags(write=False)
    t.setflags(write=False)
    _BIL[(H, W)] = (v, t)
    return v, t


@pytest.mark.parametrize("H,W,dyadic", BILINEAR, ids=[f"{h}x{w}" for h, w, _ in BILINEAR])
def test_bilinear(gpu_lib, H, W, dyadic):
    """preprocess_bilinear_kernel against v, the float64 value of its own formula on coordinates and weights formed in f32 in the kernel's order.

    u = 2^-24.  The interpolation rounds at most seven times (w0 = 1 - w1, h0 = 1 - h1 are the reference's too; four products and three sums per pixel,
    fewer where hipcc fuses) on values below 2^8, each by at most 2^-16; then / 255, - mean (two roundings of values below 1: 2 u), / std (amplifies by
    1 / min(std), result below 4: one more rounding of at most 4 u):

        delta_arith = (7 2^-16 / 255 + 2 u) / min(std) + 4 u  ~  2.3e-6

    hipcc may contract (o + 0.5) s - 0.5 into one fma, which moves a coordinate by at most one f32 ulp of a value <= max(H, W); bilinear interpolation is
    Lipschitz in each coordinate with constant <= 255 per axis (1 after / 255), so

        delta = delta_arith + 2 ulp32(max(H, W)) / min(std)

    Where the scale is a power of two the product (o + 0.5) s is exact, fused or not: delta = delta_arith.  torch (oracle.clip_torch.finetune_transform)
    forms its scale and weights its own way and rounds its own f32 arithmetic, by the same count: every element within delta + delta_arith of it.
    16-bit modes: q(v - delta) <= stored <= q(v + delta), q the type's round-to-nearest-even (lowbits.quantize; tests/test_row_kernels_gpu.py's rule)."""
    R = 224
    v, t = _bilinear_refs(H, W)
    delta = DELTA_ARITH + (0.0 if dyadic else 2 * 2.0 ** (np.floor(np.log2(max(H, W))) - 23) / float(STD.min()))
    print(f"{H}x{W}: delta {delta:.3e}; float64 formula vs torch {np.abs(v - t).max():.3e}")
    assert np.abs(v - t).max() <= delta + DELTA_ARITH          # the two references agree to the bound they are used at
    fr = _frames(H, W)
    for patch in (16, 32):
        vp, tp = _patch_major(v, patch), _patch_major(t, patch)
        for mode in (F32, BF16, F16):
            what = f"bilinear {H}x{W} {MODE_NAME[mode]} patch {patch}"
            buf = np.full(vp.size * (4 if mode == F32 else 2), FILL, np.uint8)
            gpu_lib.check(gpu_lib.lib.arp_op_preprocess_bilinear(_u8p(fr), 2, H, W, R, patch, mode, _vp(buf)))
            if mode == F32:
                got = buf.view(np.float32).reshape(vp.shape).astype(np.float64)
                e, et = np.abs(got - vp), np.abs(got - tp)
                print(f"{what}: max |out - v| {e.max():.3e} (bound {delta:.3e}), max |out - torch| {et.max():.3e} (bound {delta + DELTA_ARITH:.3e})")
                assert e.max() <= delta, f"{what}: |out - v| reaches {e.max():.3e} at {np.unravel_index(e.argmax(), e.shape)}, bound {delta:.3e}"
                assert et.max() <= delta + DELTA_ARITH, f"{what}: |out - torch| reaches {et.max():.3e}, bound {delta + DELTA_ARITH:.3e}"
            else:
                fmt = "bf16" if mode == BF16 else "f16"
                dec = _val16(buf.view(np.uint16).reshape(vp.shape), mode)
                print(f"{what}: max |out - v| {np.abs(dec - vp).max():.3e} (stored {fmt})")
                bad = ~((quantize(vp - delta, fmt) <= dec) & (dec <= quantize(vp + delta, fmt)))
                assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} stored codes are not q(t) for any t in [v - delta, v + delta]; first at {tuple(np.argwhere(bad)[0])}"


def test_bilinear_refuses_one_side_at_res(gpu_lib):
    fr = _frames(64, 64)
    for H, W in ((224, 100), (100, 224)):
        buf = np.full(2 * 3 * 224 * 224 * 4, FILL, np.uint8)
        rc = gpu_lib.lib.arp_op_preprocess_bilinear(_u8p(np.zeros((2, H, W, 3), np.uint8)), 2, H, W, 224, 16, F32, _vp(buf))
        assert rc != 0 and "exactly one side at 224" in gpu_lib.last_error() and (buf == FILL).all()
    buf = np.full(2 * 3 * 224 * 224 * 4, FILL, np.uint8)
    gpu_lib.check(gpu_lib.lib.arp_op_preprocess_bilinear(_u8p(fr), 2, 64, 64, 224, 16, F32, _vp(buf)))
    assert np.abs(buf.view(np.float32).reshape(-1, 768) - _patch_major(_bilinear_refs(64, 64)[0], 16)).max() <= DELTA_ARITH + 2 * 2.0 ** -17 / float(STD.min())


# ---- crop ---------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,side,y0,x0,cs", [(2, 64, 16, 16, 32),
                                              (2, 64, 15, 14, 33),       # odd offsets, 99-byte rows
                                              (22, 256, 64, 64, 128)],   # 1 081 344 bytes > 4096 blocks x 256: the grid-stride loop runs
                         ids=["cs32", "cs33-odd", "grid-stride"])
def test_crop_u8(gpu_lib, n, side, y0, x0, cs):
    fr = np.random.default_rng(cs).integers(0, 256, (n, side, side, 3), dtype=np.uint8)
    out = np.full((n, cs, cs, 3), FILL, np.uint8)
    gpu_lib.check(gpu_lib.lib.arp_op_crop_u8(_u8p(fr), n, side, side, y0, x0, cs, _u8p(out)))
    _assert_equal_words(out, fr[:, y0:y0 + cs, x0:x0 + cs, :], f"crop n {n} {side}x{side} ({y0}, {x0}) cs {cs}")
    assert gpu_lib.lib.arp_op_crop_u8(_u8p(fr), n, side, side, side - cs + 1, x0, cs, _u8p(out)) != 0    # window past the last row


# ---- M3AE patchify ------------------------------------------------------------------------------------------------------------------------------------------

def _patchify_input(n, res, scale):
    rng = np.random.default_rng(res * 10 + n)
    x = (rng.standard_normal((n, res, res, 3)) * scale).astype(np.float32)
    flat = x.reshape(-1)
    # +-0, values binary16 holds exactly (lo = 0), and values whose lo is a binary16 subnormal (1 + 2^-20: hi 1, lo 2^-20 < 2^-14)
    specials = np.array([0.0, -0.0, 1.5, -0.25, 1 + 2.0 ** -20, -(1 + 2.0 ** -20), 3 + 2.0 ** -22, 2.0 ** -15], np.float32)
    idx = rng.choice(flat.size, 64 * specials.size, replace=False)
    flat[idx] = np.tile(specials, 64)
    return x


@pytest.mark.parametrize("n,res,patch", [(3, 32, 16), (1, 48, 16),    # 6912 values: a ragged last block
                                         (1, 224, 16)])
@pytest.mark.parametrize("scale", [1.0, 1e-3, 300.0])
def test_patchify(gpu_lib, n, res, patch, scale):
    from oracle import m3ae_np
    x = _patchify_input(n, res, scale)
    want = np.ascontiguousarray(m3ae_np.patchify(x, patch).reshape(-1, 3 * patch * patch))
    rows, K = want.shape
    what = f"patchify n {n} res {res} patch {patch} scale {scale}"
    got = {}
    for form, nbytes in ((0, 4), (1, 2), (2, 2), (3, 6)):
        buf = np.full(want.size * nbytes, FILL, np.uint8)
        gpu_lib.check(gpu_lib.lib.arp_op_patchify(_fp(x), n, res, patch, form, _vp(buf)))
        got[form] = buf
    _assert_equal_words(got[0].view(np.uint32), want.view(np.uint32), what + " f32")
    _assert_equal_words(got[1].view(np.uint16), _bits16(want, BF16), what + " bf16")
    _assert_equal_words(got[2].view(np.uint16), _bits16(want, F16), what + " f16")
    hi = want.astype(np.float16)
    lo = (want - hi.astype(np.float32)).astype(np.float16)      # want - hi is exact in f32; subnormal lo kept
    assert (lo[np.isin(want, np.float32(1 + 2.0 ** -20))].view(np.uint16) == np.float16(2.0 ** -20).view(np.uint16)).all() and lo.view(np.uint16).min() == 0
    _assert_equal_words(got[3].view(np.uint16), np.concatenate([hi, lo, hi], axis=1).view(np.uint16), what + " split3")
    ob = np.full(rows * K * 6, FILL, np.uint8)
    gpu_lib.check(gpu_lib.lib.arp_op_split3(_fp(np.ascontiguousarray(got[0].view(np.float32))), _vp(ob), ob.size, rows, K))
    _assert_equal_words(got[3].view(np.uint16), ob.view(np.uint16), what + " split3 against arp_op_split3 of the f32 rows")


def test_patchify_refusals(gpu_lib):
    x = np.zeros((1, 24, 24, 3), np.float32)
    buf = np.full(24 * 24 * 3 * 6, FILL, np.uint8)
    assert gpu_lib.lib.arp_op_patchify(_fp(x), 1, 24, 6, 0, _vp(buf)) != 0     # patch % 4
    assert gpu_lib.lib.arp_op_patchify(_fp(x), 1, 24, 16, 0, _vp(buf)) != 0    # res % patch
    assert gpu_lib.lib.arp_op_patchify(_fp(x), 1, 24, 8, 4, _vp(buf)) != 0     # no such form
    assert (buf == FILL).all()
