"""GPU tests of the device-resident fine-tuned reward (arp_ft_reward_* in include/arp_hip.h; arp_amd/finetune.py::FinetunedClip.reward): uint8 frames ->
frozen towers -> the head's inference pass -> exp(logit_scale) <adapted image, adapted prompt>, against the fp64 oracle the host path's tests use
(oracle/clip_torch.py towers on oracle/preprocess.py frames or CT.finetune_transform, oracle/finetune_torch.py::_encode for the head)."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# the geometries of tests/test_finetune_gpu.py
TOWER = dict(patch=32, width=64, layers=2, heads=2, embed=64, img_res=224, txt_width=64, txt_layers=2, txt_heads=2, ctx=77, vocab=512)
TINY_HEAD = dict(layers=2, width_v=64, width_t=64, embed=64, hidden=64)      # contractions K = 128, 192
MID = dict(layers=3, width_v=128, width_t=64, embed=64, hidden=64, n_actions=15)  # contractions K = 384, 256
# MID's head has three layers of width 128 / 64: the towers in front of it are TOWER's with exactly those three numbers changed (a head behind towers of
# another geometry is one of the refusals this file tests)
MID_TOWER = dict(TOWER, width=128, layers=3, txt_layers=3)
GUARD = np.float32(-4096.0)
N_FRAMES = 19


def _live(lib):
    out = (C.c_int64 * 5)()
    lib.check(lib.lib.arp_debug_live(out))
    return list(out)


class _Setup:
    """Weights, frames, prompts and the fp64 oracle logits [transform, use_crop] -> [n_prompts, N_FRAMES] of one geometry; built once per process."""

    def __init__(self, tower_kw, head_kw, seed, n_frames=N_FRAMES, keys=None, clip_cfg=None, frames=None):
        import torch
        from arp_amd import clip, synth
        from oracle import clip_np as CN, clip_torch as CT, finetune_torch as O
        self.clip_cfg = clip_cfg if clip_cfg is not None else clip.ClipConfig(**tower_kw)
        self.ocfg = CN.ClipConfig(**tower_kw)
        self.hcfg = O.HeadConfig(**head_kw, logit_scale=float(np.log(100.0)))
        self.W = synth.clip_weights(self.ocfg, seed=seed)
        self.W["logit_scale"] = np.float32(self.hcfg.logit_scale) * np.ones((), np.float32)
        self.P = O.init_params(self.hcfg, seed=seed + 1)
        self.P["image_residual_weight"] = np.float32(0.5) * np.ones((), np.float32)
        self.P["text_residual_weight"] = np.float32(-0.2) * np.ones((), np.float32)
        self.frames = synth.procgen_like_frames(n_frames, 256, 256, seed=seed + 2) if frames is None else frames
        self.tok = synth.prompt_tokens(2, [6, 9], ctx=self.ocfg.ctx, vocab=self.ocfg.vocab, seed=seed + 3)
        self.Wt = CT.to_torch(self.W)
        self.keys = keys or [("label", False), ("label", True), ("finetune", False), ("finetune", True)]
        self.logits = self.oracle(self.P)

    def tower_inputs(self, transform, use_crop):
        import torch
        from oracle import clip_torch as CT, preprocess as PP
        fr = self.frames[:, 64:192, 64:192] if use_crop else self.frames  # the centre crop of side W // 2 of a 256 x 256 frame
        return torch.from_numpy(PP.preprocess(fr)).float() if transform == "label" else CT.finetune_transform(fr)

    def oracle(self, P):
        """fp64 head with parameters P behind the (f32 torch) tower oracle: {(transform, use_crop): logits [n_prompts, n_frames]}"""
        from oracle import clip_torch as CT, finetune_torch as O
        if not hasattr(self, "_feat"):
            self._feat = {k: CT.encode_image_multiscale(self.Wt, self.ocfg, self.tower_inputs(*k)) for k in self.keys}
            self._tfeat = CT.encode_text_multiscale(self.Wt, self.ocfg, self.tok)
        Pt = O.to_torch(P)
        t = O._encode(Pt, "text", self._tfeat[0].double(), self._tfeat[1].double()).numpy()
        out = {}
        for k, (ii, fi) in self._feat.items():
            a = O._encode(Pt, "image", ii.double(), fi.double()).numpy()
            out[k] = np.exp(self.hcfg.logit_scale) * (t @ a.T)
        return out

    def model(self, mode, max_batch=None, resident=False, P=None):
        from arp_amd import clip, finetune as FT
        kw = {} if max_batch is None else {"max_batch": max_batch}
        towers = clip.ClipLabeller(self.clip_cfg, self.W, mode=mode, **kw)
        h = self.hcfg
        head = FT.FinetuneTrainer(FT.FinetuneConfig(layers=h.layers, width_v=h.width_v, width_t=h.width_t, embed=h.embed, hidden=h.hidden, n_actions=h.n_actions,
                                                    logit_scale=h.logit_scale), mode=mode)
        head.load_state_dict(self.P if P is None else P)
        return FT.FinetunedClip(towers, head, resident=resident)


@functools.lru_cache(maxsize=None)
def _tiny():
    return _Setup(TOWER, TINY_HEAD, seed=171)


@functools.lru_cache(maxsize=None)
def _mid():
    return _Setup(MID_TOWER, MID, seed=271, keys=[("label", False)])


def _bar(transform, ref):
    # label transform: tol * 100 with tol = 2e-4, the f32 case of test_online_adapter_rewards; fine-tune transform: test_clip_ft_labelling_branch's
    return 2e-2 if transform == "label" else 2e-3 * max(1.0, float(np.abs(ref).max()))


def _ref(setup, transform, use_crop, reduce, n):
    lg = setup.logits[(transform, use_crop)][:, :n]
    return lg.mean(axis=0) if reduce == "mean" else lg[0]


def _host_call(m, frames, n, **kw):
    """arp_ft_reward into a caller buffer prefilled with the guard value: rewards [n], and the entries past n untouched"""
    from arp_amd import _ffi
    out = np.full(n + 3, GUARD, np.float32)
    f = np.ascontiguousarray(frames[:n])
    _ffi.check(_ffi.lib.arp_ft_reward(m.head._h, m.towers._h, _ffi.as_ptr(f, C.c_uint8), n, f.shape[1], f.shape[2], int(kw.get("use_crop", False)),
                                      m.TRANSFORMS[kw.get("transform", "finetune")], _ffi.as_ptr(out, C.c_float)))
    assert np.array_equal(out[n:], np.full(3, GUARD)), out[n:]
    return out[:n]


def _device_call(m, frames, n, **kw):
    from arp_amd import clip
    f = np.ascontiguousarray(frames[:n])
    fd, rd = clip.DeviceBuffer(f.nbytes).upload(f), clip.DeviceBuffer((n + 1) * 4).upload(np.full(n + 1, GUARD, np.float32))
    try:
        m.reward_device_async(fd, n, f.shape[1], f.shape[2], rd, **kw)
        m.towers.sync()
        out = rd.download(np.float32, n + 1)
    finally:
        fd.free(); rd.free()
    assert out[n] == GUARD
    return out[:n]


@pytest.mark.parametrize("n", [1, 3, 16, 17])
def test_f32_rewards_match_the_fp64_oracle(gpu_lib, n):
    """Both transforms, use_crop off and on, reduction "first" and "mean" over two prompts; host and device entry give the same bits."""
    s = _tiny()
    m = s.model("f32").set_text(s.tok)
    try:
        for transform in ("label", "finetune"):
            for use_crop in (False, True):
                for reduce in ("first", "mean"):
                    m.set_prompt_reduce(reduce)
                    ref = _ref(s, transform, use_crop, reduce, n)
                    got = _host_call(m, s.frames, n, use_crop=use_crop, transform=transform)
                    dev = _device_call(m, s.frames, n, use_crop=use_crop, transform=transform)
                    err = float(np.abs(got - ref).max())
                    print(f"n {n} {transform} crop {use_crop} {reduce}: max |r - ref| {err:.3e} (bar {_bar(transform, ref):.1e})")
                    assert err < _bar(transform, ref), (got, ref)
                    assert np.array_equal(got, dev)
                    assert np.array_equal(got, m.reward(s.frames[:n], use_crop=use_crop, transform=transform))
    finally:
        m.close()


def test_f32_chunks_of_max_batch(gpu_lib):
    """19 frames through towers built with max_batch = 8: two chunk boundaries and a ragged last chunk, from host and from device memory."""
    s = _tiny()
    m = s.model("f32", max_batch=8).set_text(s.tok)
    try:
        for transform, use_crop, reduce in (("label", False, "mean"), ("finetune", True, "first"), ("label", True, "first"), ("finetune", False, "mean")):
            m.set_prompt_reduce(reduce)
            ref = _ref(s, transform, use_crop, reduce, N_FRAMES)
            got = _host_call(m, s.frames, N_FRAMES, use_crop=use_crop, transform=transform)
            dev = _device_call(m, s.frames, N_FRAMES, use_crop=use_crop, transform=transform)
            print(f"19 frames {transform} crop {use_crop} {reduce}: max |r - ref| {float(np.abs(got - ref).max()):.3e}")
            assert np.abs(got - ref).max() < _bar(transform, ref), (got, ref)
            assert np.array_equal(got, dev)
    finally:
        m.close()


@pytest.mark.parametrize("mode", ["f16", "bf16"])
def test_16bit_modes_are_no_worse_than_the_host_path(gpu_lib, mode):
    """MID head, label transform, n = 1, 3, 17: e_new = max |resident - oracle| against e_old = max |FinetunedClip.online_reward(resident=False) - oracle| on
    the same frames.  Both paths round the same tensors at the same points and differ in summation order only: e_new <= 2 e_old.
    Measured on an MI355X, n = 1 / 3 / 17 (logit units, exp(logit_scale) = 100): f16 e_old 3.873e-3 / 4.365e-3 / 7.038e-3, e_new 3.873e-3 / 4.366e-3 /
    7.040e-3; bf16 e_old 8.381e-2 / 8.381e-2 / 8.669e-2, e_new the same to four digits."""
    s = _mid()
    m = s.model(mode).set_text(s.tok)
    try:
        for n in (1, 3, 17):
            ref = _ref(s, "label", False, "first", n)
            old = np.concatenate([m.online_reward(s.frames[i]) for i in range(n)])
            new = _host_call(m, s.frames, n, transform="label")
            e_old, e_new = float(np.abs(old - ref).max()), float(np.abs(new - ref).max())
            print(f"{mode} n {n}: e_old {e_old:.3e} e_new {e_new:.3e}")
            assert e_new <= 2 * e_old, (n, e_old, e_new)
            assert np.array_equal(new, _device_call(m, s.frames, n, transform="label"))
    finally:
        m.close()


def test_real_geometry_f16(gpu_lib):
    """ViT-B/16 + the 476 M-parameter head in f16, two frames, label transform: |r - ref| < 0.25 = 2.5e-3 * 100, the `full` bar of test_online_adapter_rewards."""
    from arp_amd import clip
    s = _Setup(dict(patch=16), {}, seed=171, n_frames=2, keys=[("label", False)], clip_cfg=clip.MODELS["ViT-B/16"])
    m = s.model("f16").set_text(s.tok)
    try:
        for reduce in ("first", "mean"):
            m.set_prompt_reduce(reduce)
            ref = _ref(s, "label", False, reduce, 2)
            got = _host_call(m, s.frames, 2, transform="label")
            print(f"full geometry f16 {reduce}: {got} ref {ref}")
            assert np.abs(got - ref).max() < 0.25, (got, ref)
    finally:
        m.close()


@pytest.mark.parametrize("F", [192, 256, 6656])
def test_reward_kernel_alone(gpu_lib, F):
    """ft_reward_kernel through arp_op_ft_reward against fp64 within 16 u (sum |y t| / ||y|| + |r|) s, u = 2^-24; a row with ||y|| = 0 (the clamp: reward 0);
    "mean" equals the kernel on the host-averaged prompt vector bit for bit."""
    lib = gpu_lib
    rng = np.random.default_rng(F)
    rows, npr, rw, scale = 5, 3, np.float32(0.5), np.float32(100.0)
    f, A = rng.standard_normal((rows, F)).astype(np.float32), rng.standard_normal((rows, F)).astype(np.float32)
    f[2] = 0
    A[2] = 0
    t = rng.standard_normal((npr, F)).astype(np.float32)
    t /= np.linalg.norm(t, axis=1, keepdims=True)

    def run(tv, mean):
        tv = np.ascontiguousarray(tv, np.float32)
        out = np.full(rows, GUARD, np.float32)
        p = lib.as_ptr
        lib.check(lib.lib.arp_op_ft_reward(p(f, C.c_float), p(A, C.c_float), float(rw), p(tv, C.c_float), tv.shape[0], mean, float(scale), p(out, C.c_float), rows, F))
        return out

    res = 1.0 / (1.0 + np.exp(-np.float64(rw)))
    y = res * f.astype(np.float64) + (1.0 - res) * A.astype(np.float64)
    nrm = np.maximum(np.linalg.norm(y, axis=1), 1e-12)
    u = 2.0 ** -24
    host_mean = ((t[0] + t[1]) + t[2]) / np.float32(npr)  # f32, rows in order: what ft_rows_mean_kernel computes
    assert host_mean.dtype == np.float32
    for tv, got in ((t[0], run(t, 0)), (host_mean, run(t, 1))):
        tv = tv.astype(np.float64)
        ref = scale * (y @ tv) / nrm
        bound = 16 * u * ((np.abs(y * tv).sum(axis=1) / nrm) + np.abs(ref) / scale) * scale
        print(f"F {F}: max err {np.abs(got - ref).max():.3e}, bounds {bound}")
        assert np.all(np.abs(got - ref) <= bound), (got, ref, bound)
        assert got[2] == 0.0
    assert np.array_equal(run(t, 1), run(host_mean[None], 0))


def test_isolation_and_versioning(gpu_lib):
    """A staged batch survives a reward call (forward() bit-equal before and after); the same frames twice give the same bits; after set_tensors and after a
    train step the call is refused until set_text runs again, and the rewards then follow the new parameters."""
    from arp_amd import finetune as FT
    s = _tiny()
    m = s.model("f32").set_text(s.tok)
    lib = gpu_lib
    try:
        head = m.head
        batch = FT.synth_batch(head.cfg, 4, seed=5)
        head.set_batch(*batch)
        before = head.forward()
        r1 = m.reward(s.frames[:3], transform="label")
        after = head.forward()
        for k in ("loss", "vip_loss", "id_loss", "lambda_id"):
            assert before[k] == after[k], k
        assert np.array_equal(before["scores"], after["scores"]) and np.array_equal(before["logits"], after["logits"])
        assert np.array_equal(r1, m.reward(s.frames[:3], transform="label"))
        assert np.abs(r1 - _ref(s, "label", False, "first", 3)).max() < 2e-2
        # a host write of the parameters
        P2 = {k: np.array(v, copy=True) for k, v in s.P.items()}
        P2["image_adapter.layers.3.bias"] = P2["image_adapter.layers.3.bias"] + np.float32(0.25)
        head.set_tensors(P2)
        with pytest.raises(lib.ArpError, match="set_text"):
            m.reward(s.frames[:3], transform="label")
        m.set_text(s.tok)
        r2 = m.reward(s.frames[:3], transform="label")
        ref2 = s.oracle(P2)[("label", False)][0, :3]
        assert np.abs(r2 - ref2).max() < 2e-2, (r2, ref2)
        assert np.abs(r2 - r1).max() > 0.1  # (the write moved the rewards by more than the bar: the new parameters are what was read)
        # a train step
        head.set_batch(*batch)
        head.train_step(1e-2)
        with pytest.raises(lib.ArpError, match="set_text"):
            m.reward(s.frames[:3], transform="label")
        m.set_text(s.tok)
        r3 = m.reward(s.frames[:3], transform="label")
        ref3 = s.oracle(head.get_params())[("label", False)][0, :3]
        assert np.abs(r3 - ref3).max() < 2e-2, (r3, ref3)
    finally:
        m.close()


def test_refusals(gpu_lib):
    from arp_amd import clip, finetune as FT
    lib = gpu_lib
    s = _tiny()
    m = s.model("f32")
    fr = s.frames[:2]
    h = s.hcfg
    try:
        with pytest.raises(lib.ArpError, match="no prompts cached"):
            m.reward(fr)
        m.set_text(s.tok)
        fd, rd = clip.DeviceBuffer(fr.nbytes).upload(fr), clip.DeviceBuffer(16).upload(np.full(4, GUARD, np.float32))
        with pytest.raises(lib.ArpError, match="null buffer"):
            m.reward_device_async(None, 2, 256, 256, rd)
        with pytest.raises(lib.ArpError, match="null buffer"):
            m.reward_device_async(fd, 2, 256, 256, None)
        with pytest.raises(lib.ArpError, match="empty"):
            m.reward_device_async(fd, 0, 256, 256, rd)
        with pytest.raises(lib.ArpError, match="empty"):
            m.reward(fr[:0])
        with pytest.raises(lib.ArpError, match="transform"):
            lib.check(lib.lib.arp_ft_reward_dev_async(m.head._h, m.towers._h, fd.ptr, 2, 256, 256, 0, 7, rd.ptr))
        with pytest.raises(lib.ArpError, match="null handle"):
            lib.check(lib.lib.arp_ft_reward_dev_async(m.head._h, None, fd.ptr, 2, 256, 256, 0, 0, rd.ptr))
        m.towers.sync()
        assert np.array_equal(rd.download(np.float32, 4), np.full(4, GUARD, np.float32))  # a refused call writes nothing
        fd.free(); rd.free()
        # a head of another geometry, and a goal-conditioned head, behind the same towers
        for kw, msg in ((dict(width_v=128), "do not match"), (dict(layers=3), "do not match"), (dict(embed=128), "do not match"), (dict(goal_conditioned=True), "goal")):
            cfg = FT.FinetuneConfig(**{**dict(layers=h.layers, width_v=h.width_v, width_t=h.width_t, embed=h.embed, hidden=h.hidden, n_actions=h.n_actions), **kw})
            other = FT.FinetuneTrainer(cfg, mode="f32")
            try:
                with pytest.raises(lib.ArpError, match=msg):
                    lib.check(lib.lib.arp_ft_reward_set_text(other._h, m.towers._h, lib.as_ptr(np.ascontiguousarray(s.tok, np.int32), C.c_int32), 2))
                with pytest.raises(lib.ArpError, match=msg):
                    FT.FinetunedClip(m.towers, other).reward(fr)
            finally:
                other.close()
        if lib.device_count() >= 2:  # towers and head on different devices
            other = FT.FinetuneTrainer(m.head.cfg, mode="f32", device=1)
            try:
                with pytest.raises(lib.ArpError, match="device"):
                    FT.FinetunedClip(m.towers, other).reward(fr)
            finally:
                other.close()
                lib.check(lib.lib.arp_set_device(0))
        assert np.abs(m.reward(fr, transform="label") - _ref(s, "label", False, "first", 2)).max() < 2e-2  # the pair is still usable
    finally:
        m.close()


def test_ownership(gpu_lib):
    """arp_debug_live returns to its starting values: after set_text, a latency-size call (captured), a 19-frame call and close(); and after a refused call."""
    lib = gpu_lib
    s = _tiny()
    start = _live(lib)
    m = s.model("f32", max_batch=8).set_text(s.tok)
    m.reward(s.frames[:1], transform="label")
    m.reward(s.frames[:1], transform="label")
    m.reward(s.frames, transform="finetune", use_crop=True)
    assert _live(lib) != start
    m.close()
    assert _live(lib) == start
    m = s.model("f32")
    with pytest.raises(lib.ArpError):
        m.reward(s.frames[:1])
    m.close()
    assert _live(lib) == start


# ---- the weight-streaming rows kernel alone (csrc/ftrows.h) through arp_op_ft_rows_gemm ------------------------------------------------
def _rows_gemm(lib, mode, act, A, W, bias, out, out_f32, M, N, K, ksplit):
    p = lib.as_ptr
    return lib.lib.arp_op_ft_rows_gemm({"bf16": lib.MODE_BF16, "f16": lib.MODE_F16}[mode], act, p(A, C.c_float), A.shape[1], p(W, C.c_float), W.shape[1],
                                       p(bias, C.c_float) if bias is not None else None, p(out, C.c_float), out.shape[1], out.shape[0], int(out_f32), M, N, K, ksplit)


@pytest.mark.parametrize("mode", ["f16", "bf16"])
@pytest.mark.parametrize("M", [1, 2, 15, 16])
def test_rows_gemm_alone(gpu_lib, mode, M):
    """K in {64, 128, 192, 448} x N in {16, 48, 208} (one, several and ragged 64-column groups); the dispatcher's slice count (K / 64 at these shapes),
    a forced 1 and a 2 in between; lda, ldw, ldo wider than the matrix; bias, ReLU and both output types.  Operands are multiples of 1/8 in [-1, 1], exact in
    both operand types.  Bound: (L + 1) u sum |terms| with u = 2^-24 and L = kper + S, the kernel's longest chain (the kper products of one slice through the
    MFMA accumulator, then the S slabs in the reduce; the bias is one more term), plus one ulp of a 16-bit output.  Guard row and columns keep their prefill;
    permuting the rows of A permutes the output rows bit for bit."""
    lib = gpu_lib
    rng = np.random.default_rng(1000 * M + (mode == "f16"))
    u, ulp_out = 2.0 ** -24, {"f16": 2.0 ** -10, "bf16": 2.0 ** -7}[mode]
    combo = 0
    for K in (64, 128, 192, 448):
        for N in (16, 48, 208):
            A = np.zeros((M, K + 8), np.float32)
            W = np.zeros((N, K + 16), np.float32)
            A[:, :K] = rng.integers(-8, 9, (M, K)) / 8.0
            W[:, :K] = rng.integers(-8, 9, (N, K)) / 8.0
            A[:, K:], W[:, K:] = 7.0, -7.0  # (never read: a kernel that did would be far off)
            b = rng.standard_normal(N).astype(np.float32)
            nk = K // 64
            for ksplit in sorted({0, 1, min(2, nk)}):
                act, bias, out_f32 = (0, 2)[combo & 1], (None, b)[(combo >> 1) & 1], bool((combo >> 2) & 1)
                combo += 1
                out = np.full((M + 1, N + 4), GUARD, np.float32)
                S = _rows_gemm(lib, mode, act, A, W, bias, out, out_f32, M, N, K, ksplit)
                assert S == (nk if ksplit == 0 else ksplit), (lib.last_error(), S)
                terms = np.abs(A[:, None, :K].astype(np.float64) * W[None, :, :K]).sum(axis=2) + (np.abs(bias) if bias is not None else 0.0)
                ref = A[:, :K].astype(np.float64) @ W[:, :K].astype(np.float64).T + (bias if bias is not None else 0.0)
                if act:
                    ref = np.maximum(ref, 0.0)
                L = -(-nk // S) * 64 + S
                bound = (L + 1) * u * terms + (0.0 if out_f32 else ulp_out * np.abs(ref))
                err = np.abs(out[:M, :N] - ref)
                assert np.all(err <= bound), (K, N, ksplit, act, bias is not None, out_f32, float(err.max()), float(bound.min()))
                assert np.all(out[M] == GUARD) and np.all(out[:, N:] == GUARD)
                if M >= 15:  # row independence
                    perm = rng.permutation(M)
                    out2 = np.full((M + 1, N + 4), GUARD, np.float32)
                    assert _rows_gemm(lib, mode, act, np.ascontiguousarray(A[perm]), W, bias, out2, out_f32, M, N, K, ksplit) == S
                    assert np.array_equal(out2[:M], out[perm])


def test_rows_gemm_refuses_what_is_outside_its_domain(gpu_lib):
    lib = gpu_lib
    for M, N, K, lda, ldw in ((17, 16, 64, 64, 64), (1, 16, 96, 96, 96), (1, 24, 64, 64, 64), (2, 16, 64, 68, 64), (2, 16, 64, 64, 68), (0, 16, 64, 64, 64)):
        A, W = np.ones((max(M, 1), lda), np.float32), np.ones((N, ldw), np.float32)
        out = np.full((max(M, 1) + 1, N + 4), GUARD, np.float32)
        rc = _rows_gemm(lib, "f16", 0, A, W, None, out, True, M, N, K, 0)
        assert rc < 0 and "rows_gemm" in lib.last_error(), (M, N, K, lda, ldw, rc)
        assert np.all(out == GUARD)
    A, W, out = np.ones((1, 64), np.float32), np.ones((16, 64), np.float32), np.full((2, 20), GUARD, np.float32)
    assert lib.lib.arp_op_ft_rows_gemm(lib.MODE_F32, 0, lib.as_ptr(A, C.c_float), 64, lib.as_ptr(W, C.c_float), 64, None, lib.as_ptr(out, C.c_float), 20, 2, 1, 1, 16, 64, 0) < 0
    assert np.all(out == GUARD)


@pytest.mark.parametrize("mode", ["f16", "bf16"])
def test_rows_kernel_inside_the_path_and_16bit_isolation(gpu_lib, mode):
    """MID head: calls of 1 and 16 frames take the rows kernel (three products each), 17 frames the training GEMMs; on and off agree within twice the host
    path's distance from the oracle (the bar of test_16bit_modes_are_no_worse_than_the_host_path); a latency-size call is captured once and replayed; a staged
    batch survives the reward calls in the 16-bit modes too (their workspace holds separate operand-type copies)."""
    from arp_amd import finetune as FT
    s = _mid()
    m = s.model(mode).set_text(s.tok)
    try:
        head = m.head
        head.set_batch(*FT.synth_batch(head.cfg, 4, seed=5))
        before = head.forward()
        st0 = m.reward_stats()
        on1 = _host_call(m, s.frames, 1, transform="label")
        st1 = m.reward_stats()
        assert st1["rows_products"] - st0["rows_products"] == 3 and st1["captured"] - st0["captured"] == 1
        assert np.array_equal(on1, _host_call(m, s.frames, 1, transform="label"))
        st2 = m.reward_stats()
        assert st2["replayed"] - st1["replayed"] == 1 and st2["captured"] == st1["captured"] and st2["rows_products"] == st1["rows_products"]
        on16 = _host_call(m, s.frames, 16, transform="label")
        n_rows = m.reward_stats()["rows_products"]
        on17 = _host_call(m, s.frames, 17, transform="label")
        assert m.reward_stats()["rows_products"] == n_rows  # 17 rows: the training GEMMs
        m.set_rows_kernel(False)
        off1, off16 = _host_call(m, s.frames, 1, transform="label"), _host_call(m, s.frames, 16, transform="label")
        assert m.reward_stats()["rows_products"] == n_rows
        m.set_rows_kernel(True)
        ref = _ref(s, "label", False, "first", 17)
        e_off, e_on = float(np.abs(off16 - ref[:16]).max()), float(np.abs(on16 - ref[:16]).max())
        print(f"{mode}: rows kernel off {e_off:.3e} on {e_on:.3e} (max |r - oracle| over 16 frames); 17 frames {float(np.abs(on17 - ref).max()):.3e}")
        assert e_on <= 2 * e_off and abs(on1[0] - ref[0]) <= 2 * max(abs(off1[0] - ref[0]), e_off)
        after = head.forward()
        for k in ("loss", "vip_loss", "id_loss", "lambda_id"):
            assert before[k] == after[k], k
        assert np.array_equal(before["scores"], after["scores"]) and np.array_equal(before["logits"], after["logits"])
    finally:
        m.close()


def test_prompts_belong_to_the_towers_they_came_through(gpu_lib):
    from arp_amd import clip
    lib = gpu_lib
    s = _tiny()
    m = s.model("f32").set_text(s.tok)
    other = clip.ClipLabeller(s.clip_cfg, s.W, mode="f32")
    try:
        out = np.full(2, GUARD, np.float32)
        f = np.ascontiguousarray(s.frames[:2])
        rc = lib.lib.arp_ft_reward(m.head._h, other._h, lib.as_ptr(f, C.c_uint8), 2, 256, 256, 0, 1, lib.as_ptr(out, C.c_float))
        assert rc < 0 and "another towers handle" in lib.last_error() and np.all(out == GUARD)
        assert np.abs(m.reward(f, transform="label") - _ref(s, "label", False, "first", 2)).max() < 2e-2
    finally:
        other.close(); m.close()
