// Kernels of path (2), the ARP-DT policy train step (reference: arp_dt/ARPDT.py, arp_dt/layers.py,
// arp_dt/main_procgen.py:104-141,490-507).  The big contractions (adapter MLP, image_text_input and
// their weight/input gradients) run on the MFMA GEMM kernels of gemm.h / gemm256.h; everything here is
// the glue around them: layout transposes, masks, the tiny 12-token transformer (f32, VALU), losses,
// reductions and the fused clip + Adam update.  All reductions are fixed-order (no float atomics), so a
// step is bitwise reproducible.
#pragma once
#include "common.h"

namespace arp {

// ---- generic small f32 GEMM:  C[M,N] (+)= act(opA(A) . opB(B) + bias)  (+ resid) -------------------
// opA(A)[m,k] = ta ? A[k*lda + m] : A[m*lda + k];  opB(B)[k,n] = tb ? B[n*ldb + k] : B[k*ldb + n].
// 32x32 output tile per 256-thread block (2x2 per thread), K in steps of 64 through LDS.  Used for the
// policy transformer (M = B*12 rows, E = 128): a few MFLOP per call, latency- not throughput-bound.
struct SmallGemm {
    const float* A; const float* B; const float* bias; const float* resid; float* C;
    int M, N, K, lda, ldb, ldc, ta, tb, act, accumulate;
};

__device__ __forceinline__ void small_gemm_tile(const SmallGemm& g, int bx, int by) {
    // K in steps of 64 (a 12-token-transformer GEMM has K = 128..512: 2..8 steps), operands prefetched into
    // registers one step ahead so the global-memory latency of step k+1 hides under the FMAs of step k.
    constexpr int KS = 64;
    __shared__ float As[KS][33];
    __shared__ float Bs[KS][33];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int m0 = by * 32, n0 = bx * 32;
    float acc[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
    float ra[8], rb[8];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int i = threadIdx.x + e * 256;  // 0..2047
            // consecutive threads walk the operand's CONTIGUOUS axis (k for a row-major operand, m/n for a
            // transposed one) so both layouts load coalesced
            const int ka = g.ta ? (i >> 5) : (i & 63), rra = g.ta ? (i & 31) : (i >> 6);
            const int kb = g.tb ? (i & 63) : (i >> 5), rrb = g.tb ? (i >> 6) : (i & 31);
            const int m = m0 + rra, n = n0 + rrb;
            ra[e] = (k0 + ka < g.K && m < g.M) ? (g.ta ? g.A[(size_t)(k0 + ka) * g.lda + m] : g.A[(size_t)m * g.lda + k0 + ka]) : 0.f;
            rb[e] = (k0 + kb < g.K && n < g.N) ? (g.tb ? g.B[(size_t)n * g.ldb + k0 + kb] : g.B[(size_t)(k0 + kb) * g.ldb + n]) : 0.f;
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < g.K; k0 += KS) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int i = threadIdx.x + e * 256;
            const int ka = g.ta ? (i >> 5) : (i & 63), rra = g.ta ? (i & 31) : (i >> 6);
            const int kb = g.tb ? (i & 63) : (i >> 5), rrb = g.tb ? (i >> 6) : (i & 31);
            As[ka][rra] = ra[e];
            Bs[kb][rrb] = rb[e];
        }
        __syncthreads();
        if (k0 + KS < g.K) fetch(k0 + KS);
#pragma unroll 16
        for (int kk = 0; kk < KS; ++kk) {
            const float a0 = As[kk][ty * 2], a1 = As[kk][ty * 2 + 1];
            const float b0 = Bs[kk][tx * 2], b1 = Bs[kk][tx * 2 + 1];
            acc[0][0] = fmaf(a0, b0, acc[0][0]); acc[0][1] = fmaf(a0, b1, acc[0][1]);
            acc[1][0] = fmaf(a1, b0, acc[1][0]); acc[1][1] = fmaf(a1, b1, acc[1][1]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int m = m0 + ty * 2 + i, n = n0 + tx * 2 + j;
            if (m < g.M && n < g.N) {
                float v = acc[i][j] + (g.bias ? g.bias[n] : 0.f);
                if (g.act == ACT_RELU) v = fmaxf(v, 0.f);
                else if (g.act == ACT_TANH) v = tanhf(v);
                else if (g.act == ACT_GELU_TANH) v = apply_act<ACT_GELU_TANH>(v);
                if (g.resid) v += g.resid[(size_t)m * g.ldc + n];
                float* c = g.C + (size_t)m * g.ldc + n;
                *c = g.accumulate ? *c + v : v;
            }
        }
}
static __global__ __launch_bounds__(256) void small_gemm_kernel(SmallGemm g) { small_gemm_tile(g, blockIdx.x, blockIdx.y); }

// ---- split-K partial reduce:  out[m,n] = act(sum_s part[s,m,n] + bias[n]) ---------------------------
template <typename OutT>
static __global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ part, int S, size_t MN, int N,
                                                            const float* __restrict__ bias, int act, OutT* __restrict__ out,
                                                            const float* __restrict__ resid = nullptr, int ldo = 0, float alpha = 1.f) {
    // 64 outputs per block, 4 slice groups per output (fixed order: group partials are added 0..3)
    __shared__ float red[4][64];
    const int x = threadIdx.x & 63, y = threadIdx.x >> 6;
    const size_t i = (size_t)blockIdx.x * 64 + x;
    float s = 0.f;
    if (i < MN) {
        // four independent partial sums: four slab loads in flight per thread instead of one dependent load-add chain
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        int k = y;
        for (; k + 12 < S; k += 16) {
            s0 += part[(size_t)k * MN + i];
            s1 += part[(size_t)(k + 4) * MN + i];
            s2 += part[(size_t)(k + 8) * MN + i];
            s3 += part[(size_t)(k + 12) * MN + i];
        }
        for (; k < S; k += 4) s0 += part[(size_t)k * MN + i];
        s = (s0 + s1) + (s2 + s3);
    }
    red[y][x] = s;
    __syncthreads();
    if (y != 0 || i >= MN) return;
    s = alpha * ((red[0][x] + red[1][x]) + (red[2][x] + red[3][x]));
    if (bias) s += bias[i % N];
    if (act == ACT_TANH) s = tanhf(s);
    else if (act == ACT_RELU) s = fmaxf(s, 0.f);
    // ldo > 0: the output (and the residual) are strided [M, ldo] views; otherwise dense [M, N]
    const size_t o = ldo > 0 ? (i / N) * (size_t)ldo + i % N : i;
    if (resid) s += resid[o];
    Elem<OutT>::st(out + o, s);
}

// The same reduction, four outputs per thread and SIXTEEN slice groups per output: 16-byte loads, four of them in flight per thread, 64 slab rows in
// flight per block where the kernel above keeps 16 -- the 257-slab reduce of image_text_input (16.8 MB) ran at 1.6 TB/s on it.  Fixed order: a thread
// adds its slabs y, y + 16, ... in four interleaved chains, the sixteen group sums are added as a balanced tree.  Needs MN, N (and ldo) multiples of 4.
template <typename OutT>
static __global__ __launch_bounds__(256) void splitk_reduce4_kernel(const float* __restrict__ part, int S, size_t MN, int N, const float* __restrict__ bias,
                                                             int act, OutT* __restrict__ out, const float* __restrict__ resid, int ldo, float alpha) {
    __shared__ float4 red[16][16];
    const int x = threadIdx.x & 15, y = threadIdx.x >> 4;
    const size_t i = ((size_t)blockIdx.x * 16 + x) * 4;
    auto add = [](float4& a, const float4 b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; };
    auto sum = [](const float4 a, const float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); };
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < MN) {
        float4 s0 = s, s1 = s, s2 = s, s3 = s;
        const float* p = part + i;
        int k = y;
        for (; k + 48 < S; k += 64) {
            const float4 a = *reinterpret_cast<const float4*>(p + (size_t)k * MN), b = *reinterpret_cast<const float4*>(p + (size_t)(k + 16) * MN);
            const float4 c = *reinterpret_cast<const float4*>(p + (size_t)(k + 32) * MN), d = *reinterpret_cast<const float4*>(p + (size_t)(k + 48) * MN);
            add(s0, a); add(s1, b); add(s2, c); add(s3, d);
        }
        for (; k < S; k += 16) add(s0, *reinterpret_cast<const float4*>(p + (size_t)k * MN));
        s = sum(sum(s0, s1), sum(s2, s3));
    }
    red[y][x] = s;
    __syncthreads();
    if (y != 0 || i >= MN) return;
    float4 t[8];
#pragma unroll
    for (int g = 0; g < 8; ++g) t[g] = sum(red[2 * g][x], red[2 * g + 1][x]);
    s = sum(sum(sum(t[0], t[1]), sum(t[2], t[3])), sum(sum(t[4], t[5]), sum(t[6], t[7])));
    float v[4] = {alpha * s.x, alpha * s.y, alpha * s.z, alpha * s.w};
    const int n = (int)(i % N);
    if (bias) {
        const float4 b = *reinterpret_cast<const float4*>(bias + n);
        v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (act == ACT_TANH) v[e] = tanhf(v[e]);
        else if (act == ACT_RELU) v[e] = fmaxf(v[e], 0.f);
    }
    const size_t o = ldo > 0 ? (i / N) * (size_t)ldo + n : i;
    if (resid) {
        const float4 r = *reinterpret_cast<const float4*>(resid + o);
        v[0] += r.x; v[1] += r.y; v[2] += r.z; v[3] += r.w;
    }
    store4(out + o, v[0], v[1], v[2], v[3]);
}
// out[m, n] = act(alpha * sum_s part[s, m, n] + bias[n]) (+ resid): the 4-wide kernel where the shape allows it
template <typename OutT>
static inline void launch_splitk_reduce(hipStream_t st, const float* part, int S, size_t MN, int N, const float* bias, int act, OutT* out,
                                        const float* resid = nullptr, int ldo = 0, float alpha = 1.f) {
    // (many-slab reductions only: at S = 8..32, the fine-tune head's, the step measured 3.28 ms on the narrow kernel and 3.35 on this one)
    if ((MN & 3) == 0 && (N & 3) == 0 && (ldo & 3) == 0 && S >= 64)
        hipLaunchKernelGGL((splitk_reduce4_kernel<OutT>), dim3((unsigned)((MN / 4 + 15) / 16)), dim3(256), 0, st, part, S, MN, N, bias, act, out, resid, ldo, alpha);
    else
        hipLaunchKernelGGL((splitk_reduce_kernel<OutT>), dim3((unsigned)((MN + 63) / 64)), dim3(256), 0, st, part, S, MN, N, bias, act, out, resid, ldo, alpha);
}

// ---- image_text_input forward on (hi, lo) binary16 pairs split in flight -----------------------------------------------------------------------------
// part[s][m][n] = sum over K-slice s of X[m][k] * W[n][k], X and W in f32 (the 16-bit modes keep this one contraction -- K = 197 376 -- at f32
// level: it is what buys the 1e-3 on 16 of 16 seeds).  On v_mfma_f32_16x16x4_f32 the product is bound by the f32 matrix rate (6.5 GF at 157 TF peak)
// on top of streaming 202 MB; here every 128 x 64 operand tile is split into (hi, lo) binary16 on its way from registers to LDS (X times 2^4, W
// times 2^10: W is ~1/sqrt(K), its lo halves would be subnormal unscaled) and the product is hi.hi + lo.hi + hi.lo on three v_mfma_f32_16x16x32_f16,
// which leaves the kernel bound by the stream alone.  One workgroup per (K slice, 128 x 128 output tile); four waves, each a 64 x 64 block with the W
// fragment as the MFMA's A operand so that a lane ends up with four consecutive n of one row m.  The next K-tile's sixteen float4 per thread are
// requested before this tile's MFMAs.  Fixed-order reduction of the slices by launch_splitk_reduce as before.
// y = res * a + (1 - res) * x, ONE expression for adapter_mix_kernel and for the mix done inside iti_x3_kernel's operand load (the two must agree bit for bit)
static __device__ __forceinline__ float adapter_mix1(float res, float a, float x) { return __builtin_fmaf(res, a, (1.f - res) * x); }
struct iti_nomix_t {};
// TA != iti_nomix_t: the adapter's mix inside the operand load -- X is the f32 encoder output, Amix the adapter's output (operand type, or f32 with the
// corrected adapter), and the X operand is adapter_mix1(sigmoid(rw), a, x) formed in registers; the rounded mix (what the backward's dWi reads) goes out as
// y16.  Saves the mix's own pass: it read a + x and wrote y16 + a 101 MB f32 copy that this kernel then read back (303 + 202 MB -> 303 MB at B = 32).
// X16 (with the mix only): x comes from its operand-type copy x16 (what fc1 and the backward read) instead of the f32 encodings -- 50 MB less per step at B = 32.
// The mix's value is rounded to the operand type for the backward anyway and its skip term weighs (1 - res) (0.018 at the initial residual_weight = 4), so
// x's own rounding is at most as large as the adapter output's, which has always been there (16-seed logits 8.73e-4 against 8.74e-4).
// ADX (round 6, with a binary16 Amix): adx holds, per adapter output value, the e2m1 code of its binary16 ROUNDING ERROR times 2^F16C_DX_SHIFT (two per byte, the layout
// fc2's epilogue writes as GemmArgs::dx4_out) -- the mix is formed on a_hi + 2^-13 fp4: the adapter output to ~2^-14 instead of 2^-12 for 12.6 MB more than the binary16
// hand-off, where the f32 hand-off costs 50 MB more here and the f32 read-modify epilogue in fc2 (arp_dt.hip, ARP_DT_ADAPTER_PLAN "d").
template <int AHEAD, typename TA = iti_nomix_t, typename TY = f16_t, bool X16 = false, bool ADX = false>  // AHEAD: K-tiles of operands in flight per thread
static __global__ __launch_bounds__(256) void iti_x3_kernel(const float* __restrict__ X, size_t ldx, const float* __restrict__ W, size_t ldw, float* __restrict__ part,
                                                     int M, int N, int K, int kslice, const TA* __restrict__ Amix = nullptr, const float* __restrict__ rw = nullptr,
                                                     TY* __restrict__ y16 = nullptr, const TY* __restrict__ x16 = nullptr, const uint8_t* __restrict__ adx = nullptr) {
    constexpr bool MIX = !__is_same(TA, iti_nomix_t);
    static_assert(!X16 || MIX, "the operand-type x is the mix's");
    static_assert(!ADX || (MIX && sizeof(TA) == 2), "the e2m1 correction belongs to a binary16 adapter output");
    constexpr int ROW = 80;  // binary16 elements per LDS row: 160 B = 40 dwords -- the sixteen lanes of a ds_read_b128 group (rows j, chunks g and g + 1) fall on sixteen
                             // distinct 4-bank slots; at 144 B seven of them met another's (SQ_LDS_BANK_CONFLICT 33 % of the LDS cycles, profiles/r4_x3_pmc.json)
    __shared__ __attribute__((aligned(16))) _Float16 sm[4][128 * ROW];  // X hi, X lo, W hi, W lo
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, j = lane & 15, g = lane >> 4;
    const int n_tiles = (N + 127) / 128;
    const int m0 = (blockIdx.y / n_tiles) * 128, n0 = (blockIdx.y % n_tiles) * 128;
    // kslice > 0: workgroup s owns the K range [s * kslice, (s + 1) * kslice); kslice <= 0: the 64-wide K-tiles are dealt round-robin (tile t of workgroup s is
    // s + t * gridDim.x), so that at any moment the chip reads ONE contiguous stretch of every row (gridDim.x * 256 B) instead of gridDim.x scattered 256-byte pieces
    const int kstep = kslice > 0 ? 64 : (int)gridDim.x * 64;
    const int k0 = kslice > 0 ? blockIdx.x * kslice : blockIdx.x * 64;
    const int klast = kslice > 0 ? min(K, k0 + kslice) - 64 : k0 + (K - 64 - k0) / kstep * kstep;  // this workgroup's last tile (K % 64 == 0; k0 < K: the launcher's grid)
    const int lrow = tid >> 4, lc4 = tid & 15;
    // 32-bit byte offsets from the (uniform) matrix bases: a scalar base + one address register per load (128 rows of a 197 376-wide f32 matrix are 101 MB)
    unsigned xo[8], wo[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        xo[i] = (unsigned)(((size_t)(min(m0 + lrow + 16 * i, M - 1) - m0) * ldx + 4 * lc4) * 4);
        wo[i] = (unsigned)(((size_t)(min(n0 + lrow + 16 * i, N - 1) - n0) * ldw + 4 * lc4) * 4);
    }
    X += (size_t)m0 * ldx;  // (offsets stay inside the tile's 128 rows: < 4 GB for rows of up to 8 M floats)
    W += (size_t)n0 * ldw;
    float res = 0.f;
    bool put_y = false;
    if constexpr (MIX) {
        Amix += (size_t)m0 * ldx;
        y16 += (size_t)m0 * ldx;
        if constexpr (X16) x16 += (size_t)m0 * ldx;
        if constexpr (ADX) adx += (size_t)m0 * ldx / 2;
        res = 1.0f / (1.0f + expf(-rw[0]));
        put_y = n0 == 0;  // (every X element belongs to exactly one (row tile, K slice); a second column tile would only repeat the store)
    }
    using areg_t = std::conditional_t<sizeof(TA) == 4, float4, uint2>;  // four a values of one lane
    areg_t ar[AHEAD][MIX ? 8 : 1];
    // TWO K-tiles of operands in flight per thread (2 x 16 float4; one workgroup per CU, so the registers are there): with one, a tile's loads were
    // issued behind the previous tile's split and had only its MFMAs (0.7 us) to land in -- 3.75 TB/s of the 202 MB stream
    using xreg_t = std::conditional_t<X16, uint2, float4>;
    xreg_t xr[AHEAD][8];
    float4 wreg[AHEAD][8];
    uint16_t dxr[AHEAD][ADX ? 8 : 1];  // four e2m1 codes per lane and row
    auto fetch = [&](auto ST, int k) {
        constexpr int st = decltype(ST)::value;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if constexpr (X16) xr[st][i] = *reinterpret_cast<const uint2*>(reinterpret_cast<const char*>(x16 + k) + (xo[i] >> 1));
            else xr[st][i] = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(X + k) + xo[i]);
            if constexpr (MIX) ar[st][i] = *reinterpret_cast<const areg_t*>(reinterpret_cast<const char*>(Amix + k) + (sizeof(TA) == 4 ? xo[i] : xo[i] >> 1));
            if constexpr (ADX) dxr[st][i] = *reinterpret_cast<const uint16_t*>(adx + (k >> 1) + (xo[i] >> 3));
            wreg[st][i] = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(W + k) + wo[i]);
        }
    };
    // the mix of one lane's four values (adapter_mix_kernel's arithmetic) + its rounded copy to y16
    auto mixed = [&](xreg_t xin, areg_t a, int k, int i, uint32_t dx = 0) __attribute__((always_inline)) {
        float4 x;
        if constexpr (X16) {
            float xv[4];
            load4(reinterpret_cast<const TY*>(&xin), xv);
            x = make_float4(xv[0], xv[1], xv[2], xv[3]);
        } else {
            x = xin;
        }
        if constexpr (MIX) {
            float av[4];
            if constexpr (sizeof(TA) == 4) { av[0] = a.x; av[1] = a.y; av[2] = a.z; av[3] = a.w; }
            else load4(reinterpret_cast<const TA*>(&a), av);
            if constexpr (ADX) {  // v_cvt_scalef32_pk_f32_fp4 multiplies by its scale operand on the way up (scripts/fp4_cvt_probe2.hip)
                typedef float f2 __attribute__((ext_vector_type(2)));
                constexpr float isd = 1.0f / (float)(1 << F16C_DX_SHIFT);
                const f2 d01 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(dx, isd, 0), d23 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(dx, isd, 1);
                av[0] += d01[0]; av[1] += d01[1]; av[2] += d23[0]; av[3] += d23[1];
            }
            x.x = adapter_mix1(res, av[0], x.x); x.y = adapter_mix1(res, av[1], x.y); x.z = adapter_mix1(res, av[2], x.z); x.w = adapter_mix1(res, av[3], x.w);
            if (put_y && m0 + lrow + 16 * i < M) store4(reinterpret_cast<TY*>(reinterpret_cast<char*>(y16 + k) + (xo[i] >> 1)), x.x, x.y, x.z, x.w);
        }
        return x;
    };
    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
    // Range: the fixed scales put |x| >= 4094 or |w| >= 64 beyond binary16 (hi = inf, lo = NaN -> NaN logits with no warning).  The operands
    // here are LayerNormed encodings mixed with a ReLU'd adapter output (|x| < sqrt(768) = 27.7 for unit gains) and a lecun-normal Dense(197 376 -> 128)
    // kernel (|w| ~ 1e-2), both far inside; values outside are CLAMPED to the largest magnitude the scale leaves finite (a saturated term, never a NaN).
    auto put = [&](_Float16* hi, _Float16* lo, float4 v, float sc, int row) {
        const float lim = 65280.f / sc;
        v.x = __builtin_amdgcn_fmed3f(v.x, -lim, lim); v.y = __builtin_amdgcn_fmed3f(v.y, -lim, lim);
        v.z = __builtin_amdgcn_fmed3f(v.z, -lim, lim); v.w = __builtin_amdgcn_fmed3f(v.w, -lim, lim);
        uint2 h, l;  // common.h::split2_f16: the (power-of-two) scale, hi and lo in four v_fma_mix instructions per pair
        split2_f16(v.x, v.y, sc, h.x, l.x);
        split2_f16(v.z, v.w, sc, h.y, l.y);
        *reinterpret_cast<uint2*>(hi + row * ROW + 4 * lc4) = h;
        *reinterpret_cast<uint2*>(lo + row * ROW + 4 * lc4) = l;
    };
    f32x4_v acc[4][4];  // [n fragment][m fragment]
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = f32x4_v{0.f, 0.f, 0.f, 0.f};
    using S0 = std::integral_constant<int, 0>;
    auto ktile = [&](auto ST, int k) __attribute__((always_inline)) {
        constexpr int st = decltype(ST)::value;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            put(sm[0], sm[1], mixed(xr[st][i], ar[st][MIX ? i : 0], k, i, ADX ? dxr[st][ADX ? i : 0] : 0), 16.f, lrow + 16 * i);
            put(sm[2], sm[3], wreg[st][i], 1024.f, lrow + 16 * i);
        }
        __syncthreads();
        // unconditional (the slice's last AHEAD tiles re-request its last tile: L2 hits): a conditional fetch makes the staged registers loop-carried
        // through a merge, and hipcc then waits for the loads right behind their issue (vmcnt(1) at the back edge) -- the prefetch gone
#ifdef ARP_ITI_R4  // the round-4 form, for same-box A/B builds (make ALT=iti_r4 EXTRA=-DARP_ITI_R4)
        if (k + kstep * AHEAD <= klast) fetch(ST, k + kstep * AHEAD);
#else
        __builtin_amdgcn_sched_barrier(0);  // the requests go out HERE, ahead of the MFMAs (left alone, hipcc sinks them to the end of the tile: nothing left to overlap)
        fetch(ST, min(k + kstep * AHEAD, klast));
        __builtin_amdgcn_sched_barrier(0);
#endif
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            f16x8_v xh[4], xl[4];
#pragma unroll
            for (int mf = 0; mf < 4; ++mf) {
                const int off = (wr * 64 + mf * 16 + j) * ROW + 32 * c + 8 * g;
                xh[mf] = *reinterpret_cast<const f16x8_v*>(sm[0] + off);
                xl[mf] = *reinterpret_cast<const f16x8_v*>(sm[1] + off);
            }
#pragma unroll
            for (int nf = 0; nf < 4; ++nf) {
                const int off = (wc * 64 + nf * 16 + j) * ROW + 32 * c + 8 * g;
                const f16x8_v wh = *reinterpret_cast<const f16x8_v*>(sm[2] + off), wl = *reinterpret_cast<const f16x8_v*>(sm[3] + off);
#pragma unroll
                for (int mf = 0; mf < 4; ++mf) acc[nf][mf] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xh[mf], acc[nf][mf], 0, 0, 0);
#pragma unroll
                for (int mf = 0; mf < 4; ++mf) acc[nf][mf] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, xh[mf], acc[nf][mf], 0, 0, 0);
#pragma unroll
                for (int mf = 0; mf < 4; ++mf) acc[nf][mf] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xl[mf], acc[nf][mf], 0, 0, 0);
            }
        }
        __syncthreads();
    };
    fetch(S0{}, k0);
    for (int k = k0; k <= klast; k += kstep) ktile(S0{}, k);
    float* out = part + (size_t)blockIdx.x * M * N;
    constexpr float inv = 1.0f / (16.f * 1024.f);
#pragma unroll
    for (int mf = 0; mf < 4; ++mf) {
        const int m = m0 + wr * 64 + mf * 16 + j;
        if (m >= M) continue;
#pragma unroll
        for (int nf = 0; nf < 4; ++nf) {
            const int n = n0 + wc * 64 + nf * 16 + 4 * g;  // N % 4 == 0
            if (n < N) *reinterpret_cast<float4*>(out + (size_t)m * N + n) = make_float4(acc[nf][mf][0] * inv, acc[nf][mf][1] * inv, acc[nf][mf][2] * inv, acc[nf][mf][3] * inv);
        }
    }
}

// ---- f32 -> T conversion ----------------------------------------------------------------------------
template <typename T> __global__ __launch_bounds__(256) void convert_kernel(const float* __restrict__ in, T* __restrict__ out, size_t n) {
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i + 3 < n) {
        float v[4];
        load4(in + i, v);
        store4(out + i, v[0], v[1], v[2], v[3]);
    } else {
        for (size_t j = i; j < n; ++j) Elem<T>::st(out + j, in[j]);
    }
}

// 8 values per lane (two 16-byte loads, one 16-byte store) with a grid-stride loop: the per-step f32 -> operand-type conversion of the
// encodings is a pure HBM stream (151 MB at B = 32), which 4-value lanes ran at 4.1 TB/s
template <typename T> __device__ __forceinline__ void convert8_block(const float* __restrict__ in, T* __restrict__ out, size_t n8, int bx, int gx) {
    static_assert(sizeof(T) == 2, "16-bit outputs");
    for (size_t i = (size_t)bx * 256 + threadIdx.x; i < n8; i += (size_t)gx * 256) {
        const float4 a = *reinterpret_cast<const float4*>(in + i * 8), b = *reinterpret_cast<const float4*>(in + i * 8 + 4);
        const u32x4_v o = {pack2<T>(a.x, a.y), pack2<T>(a.z, a.w), pack2<T>(b.x, b.y), pack2<T>(b.z, b.w)};
        *reinterpret_cast<u32x4_v*>(out + i * 8) = o;
    }
}
template <typename T> __global__ __launch_bounds__(256) void convert8_kernel(const float* __restrict__ in, T* __restrict__ out, size_t n8) {
    convert8_block<T>(in, out, n8, (int)blockIdx.x, (int)gridDim.x);
}

// ---- tiled transpose with optional mask/scale:  ---------------------------------------------------------
//   v[r,c] = scale * in[r,c] * (mask ? mask[r,c] > 0 : 1)
//   outN[r*ldn + c] = v (if outN)        outT[c*ldt + r] = v (if outT)
// 64x64 tiles through LDS.  Each thread moves 4 consecutive elements per access (16 B of f32, 8 B of bf16) on the read
// and on both writes whenever the leading dimensions are multiples of 4 and the chunk is inside the matrix; ragged
// edges and odd strides fall back to single elements.
template <typename TI, typename TM, typename TO>
__device__ __forceinline__ void transpose_mask_tile(const TI* __restrict__ in, int ldi, const TM* __restrict__ mask, const float* __restrict__ scale_ptr, float scale,
                                                    TO* __restrict__ outN, int ldn, TO* __restrict__ outT, int ldt, int R, int Ccols, int bx, int by) {
    __shared__ float tile[64][65];
    const int r0 = by * 64, c0 = bx * 64;
    const float s = scale_ptr ? scale * scale_ptr[0] : scale;
    const bool vin = (ldi & 3) == 0 && (!outN || (ldn & 3) == 0);
    for (int i = threadIdx.x; i < 64 * 16; i += 256) {
        const int lr = i >> 4, lc = (i & 15) * 4;
        const int r = r0 + lr, c = c0 + lc;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (r < R && c < Ccols) {
            if (vin && c + 3 < Ccols) {
                load4(in + (size_t)r * ldi + c, v);
                if (mask) {
                    float m[4];
                    load4(mask + (size_t)r * ldi + c, m);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = m[e] > 0.f ? v[e] * s : 0.f;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] *= s;
                }
                if constexpr (__is_same(TO, f16_t)) {  // saturate instead of overflowing to inf (the scaled backward activations); NaN stays NaN
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = v[e] > 65504.f ? 65504.f : (v[e] < -65504.f ? -65504.f : v[e]);
                }
                if (outN) store4(outN + (size_t)r * ldn + c, v[0], v[1], v[2], v[3]);
            } else {
                for (int e = 0; e < 4 && c + e < Ccols; ++e) {
                    float x = Elem<TI>::ld(in + (size_t)r * ldi + c + e) * s;
                    if (mask && !(Elem<TM>::ld(mask + (size_t)r * ldi + c + e) > 0.f)) x = 0.f;
                    if constexpr (__is_same(TO, f16_t)) x = x > 65504.f ? 65504.f : (x < -65504.f ? -65504.f : x);
                    v[e] = x;
                    if (outN) Elem<TO>::st(outN + (size_t)r * ldn + c + e, x);
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) tile[lr][lc + e] = v[e];
    }
    if (!outT) return;
    __syncthreads();
    const bool vout = (ldt & 3) == 0;
    for (int i = threadIdx.x; i < 64 * 16; i += 256) {
        const int lc = i >> 4, lr = (i & 15) * 4;  // consecutive threads -> consecutive r (contiguous in outT)
        const int r = r0 + lr, c = c0 + lc;
        if (c >= Ccols || r >= R) continue;
        if (vout && r + 3 < R) {
            store4(outT + (size_t)c * ldt + r, tile[lr][lc], tile[lr + 1][lc], tile[lr + 2][lc], tile[lr + 3][lc]);
        } else {
            for (int e = 0; e < 4 && r + e < R; ++e) Elem<TO>::st(outT + (size_t)c * ldt + r + e, tile[lr + e][lc]);
        }
    }
}
template <typename TI, typename TM, typename TO>
__global__ __launch_bounds__(256) void transpose_mask_kernel(const TI* __restrict__ in, int ldi, const TM* __restrict__ mask,
                                                             const float* __restrict__ scale_ptr, float scale, TO* __restrict__ outN,
                                                             int ldn, TO* __restrict__ outT, int ldt, int R, int Ccols) {
    transpose_mask_tile<TI, TM, TO>(in, ldi, mask, scale_ptr, scale, outN, ldn, outT, ldt, R, Ccols, (int)blockIdx.x, (int)blockIdx.y);
}

// ---- adapter mix (arp_dt/ARPDT.py:466-472):  y = res*a + (1-res)*x,  res = sigmoid(residual_weight) -----
// x is the f32 encoder output itself, not its operand-type copy: the skip term then carries no operand rounding.
template <typename T, typename TA = T>  // TA = float: the adapter output before its rounding to the operand type (arp_dt.hip `adapter_c`)
static __global__ __launch_bounds__(256) void adapter_mix_kernel(const TA* __restrict__ a, const float* __restrict__ x, const float* __restrict__ rw,
                                                          T* __restrict__ y, size_t n, float* __restrict__ y32 = nullptr) {
    // y32 (optional): the un-rounded mix in f32
    const float res = 1.0f / (1.0f + expf(-rw[0]));
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i + 3 < n) {
        float av[4], xv[4], yv[4];
        load4(a + i, av);
        load4(x + i, xv);
#pragma unroll
        for (int e = 0; e < 4; ++e) yv[e] = adapter_mix1(res, av[e], xv[e]);
        store4(y + i, yv[0], yv[1], yv[2], yv[3]);
        if (y32) store4(y32 + i, yv[0], yv[1], yv[2], yv[3]);
    } else {
        for (size_t j = i; j < n; ++j) {
            const float v = adapter_mix1(res, Elem<TA>::ld(a + j), x[j]);
            Elem<T>::st(y + j, v);
            if (y32) y32[j] = v;
        }
    }
}

// ---- the adapter's forward with its operand roundings corrected on the fp4 MFMA (ARP_MODE_F16C's product, common.h; arp_dt.hip `adapter_c`) -------------
// enc f32 [rows, D] -> xb [rows, D] binary16 (the backward's operand, as convert8_kernel writes it) AND xc [rows][hi | x4 | dx4] (3 D bytes per row)
static __global__ __launch_bounds__(256) void convert_f16c_kernel(const float* __restrict__ in, f16_t* __restrict__ xb, f16_t* __restrict__ xc, size_t rows, int D) {
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= rows * (size_t)D) return;
    const size_t r = i / D;
    const int c = (int)(i - r * D);
    float v[4];
    load4(in + i, v);
    store4(xb + i, v[0], v[1], v[2], v[3]);
    store_f16c<true>(xc + r * (size_t)(3 * D / 2), c, D, v[0], v[1], v[2], v[3]);
}
// the same with SIXTEEN values per lane (D % 16 == 0): two 16-byte loads ahead of 32 + 32 + 8 (+ 8) bytes of stores, where the four-value form stores 8 + 8 + 2 + 2
template <bool WITH_DX>
static __global__ __launch_bounds__(256) void convert_f16c16_kernel(const float* __restrict__ in, f16_t* __restrict__ xb, f16_t* __restrict__ xc, size_t rows, int D) {
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 16;
    if (i >= rows * (size_t)D) return;
    const size_t r = i / D;
    const int c = (int)(i - r * D);
    float v[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 t = *reinterpret_cast<const float4*>(in + i + 4 * q);
        v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
    }
    f16_t* row = xc + r * (size_t)(3 * D / 2);
    float h[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) h[j] = h2f(f2h(v[j]));
    const uint4 h0 = make_uint4(pack_h2(h[0], h[1]), pack_h2(h[2], h[3]), pack_h2(h[4], h[5]), pack_h2(h[6], h[7]));
    const uint4 h1 = make_uint4(pack_h2(h[8], h[9]), pack_h2(h[10], h[11]), pack_h2(h[12], h[13]), pack_h2(h[14], h[15]));
    reinterpret_cast<uint4*>(xb + i)[0] = h0; reinterpret_cast<uint4*>(xb + i)[1] = h1;
    reinterpret_cast<uint4*>(row + c)[0] = h0; reinterpret_cast<uint4*>(row + c)[1] = h1;
    uint8_t* seg = reinterpret_cast<uint8_t*>(row + D);
    constexpr float sx = (float)(1 << F16C_X_SHIFT), sd = (float)(1 << F16C_DX_SHIFT);
    float x0[8], x1[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { x0[j] = h[j] * sx; x1[j] = h[8 + j] * sx; }
    *reinterpret_cast<uint2*>(seg + (c >> 1)) = make_uint2(pack_fp4x8(x0), pack_fp4x8(x1));
    if constexpr (WITH_DX) {
        float d0[8], d1[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { d0[j] = (v[j] - h[j]) * sd; d1[j] = (v[8 + j] - h[8 + j]) * sd; }
        *reinterpret_cast<uint2*>(seg + (D >> 1) + (c >> 1)) = make_uint2(pack_fp4x8(d0), pack_fp4x8(d1));
    }
}
// rows [hi | ...] of stride ld (binary16 units) -> contiguous [rows, D] binary16 (the plain copy the backward reads)
static __global__ __launch_bounds__(256) void extract_hi_kernel(const f16_t* __restrict__ in, int ld, f16_t* __restrict__ out, size_t rows, int D) {
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 8;
    if (i >= rows * (size_t)D) return;
    const size_t r = i / D;
    const int c = (int)(i - r * D);
    *reinterpret_cast<u32x4_v*>(out + i) = *reinterpret_cast<const u32x4_v*>(in + r * (size_t)ld + c);
}
// enc -> xb and the [hi | x4 (| dx4)] rows: sixteen values per lane where the width allows it (with_dx = the consumer's plan wants the dx4 segment), else the
// four-value form, which always writes dx4.  A row is 3 D bytes and the four-value form stores 8 bytes at a time: D % 8.
static int launch_convert_f16c(hipStream_t stream, bool with_dx, const float* in, f16_t* xb, f16_t* xc, size_t rows, int D) {
    if (D <= 0 || D % 8) return fail("convert_f16c: the width must be a multiple of 8 (8-byte stores into rows of 3 D bytes)");
    const size_t n = rows * (size_t)D;
    if (D % 16 == 0) {
        if (with_dx) hipLaunchKernelGGL((convert_f16c16_kernel<true>), dim3((unsigned)((n + 4095) / 4096)), dim3(256), 0, stream, in, xb, xc, rows, D);
        else hipLaunchKernelGGL((convert_f16c16_kernel<false>), dim3((unsigned)((n + 4095) / 4096)), dim3(256), 0, stream, in, xb, xc, rows, D);
    } else {
        hipLaunchKernelGGL(convert_f16c_kernel, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, stream, in, xb, xc, rows, D);
    }
    ARP_HIP_OK(hipGetLastError());
    return 0;
}
static int launch_extract_hi(hipStream_t stream, const f16_t* in, int ld, f16_t* out, size_t rows, int D) {
    if (D <= 0 || D % 8 || ld % 8 || ld < D) return fail("extract_hi: width and row stride must be multiples of 8 (16-byte copies)");
    hipLaunchKernelGGL(extract_hi_kernel, dim3((unsigned)((rows * (size_t)D + 2047) / 2048)), dim3(256), 0, stream, in, ld, out, rows, D);
    ARP_HIP_OK(hipGetLastError());
    return 0;
}
// max |w - rn16(w)| and max |w| of a weight tensor -> mx[0], mx[1] (as non-negative float bits; mx zeroed by the caller)
static __global__ __launch_bounds__(256) void wc_absmax_kernel(const float* __restrict__ w, size_t n, unsigned int* __restrict__ mx) {
    float md = 0.f, mw = 0.f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float v = w[i];
        md = fmaxf(md, fabsf(v - h2f(f2h(v))));
        mw = fmaxf(mw, fabsf(v));
    }
    md = wave_max(md); mw = wave_max(mw);
    if ((threadIdx.x & 63) == 0) {
        atomicMax(mx, __float_as_uint(md));
        atomicMax(mx + 1, __float_as_uint(mw));
    }
}
// w f32 [N, K] -> rows [W_hi: binary16 x K | dW4: e2m1 x K | W4: e2m1 x K] (3 K bytes), scales 2^sc[0] / 2^sc[1] = the powers of two that put the largest
// |dW| / |W| into (6, 12] (as arp_enc.hip::pack_weight_c chooses them on the host); thread 0 publishes them for the product (GemmArgs::mix_sptr)
static __global__ __launch_bounds__(256) void wc_pack_kernel(const float* __restrict__ w, int N, int K, const unsigned int* __restrict__ mx, f16_t* __restrict__ out,
                                                             int* __restrict__ sc) {
    const float md = __uint_as_float(mx[0]), mw = __uint_as_float(mx[1]);
    const int sd = md > 0.f ? (int)floorf(log2f(6.0f / md)) + 1 : 0, sw = mw > 0.f ? (int)floorf(log2f(6.0f / mw)) + 1 : 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) { sc[0] = sd; sc[1] = sw; }
    const float fd = ldexpf(1.0f, sd), fw = ldexpf(1.0f, sw);
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= (size_t)N * K) return;
    const size_t r = i / K;
    const int c = (int)(i - r * K);
    float v[4];
    load4(w + i, v);
    f16_t* row = out + r * (size_t)(3 * K / 2);
    float h[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) h[j] = h2f(f2h(v[j]));
    *reinterpret_cast<uint2*>(row + c) = make_uint2(pack_h2(h[0], h[1]), pack_h2(h[2], h[3]));
    uint8_t* seg = reinterpret_cast<uint8_t*>(row + K);
    *reinterpret_cast<uint16_t*>(seg + (c >> 1)) = pack_fp4x4((v[0] - h[0]) * fd, (v[1] - h[1]) * fd, (v[2] - h[2]) * fd, (v[3] - h[3]) * fd);
    *reinterpret_cast<uint16_t*>(seg + (K >> 1) + (c >> 1)) = pack_fp4x4(v[0] * fw, v[1] * fw, v[2] * fw, v[3] * fw);
}
// Both adapter kernels in TWO launches per step instead of four and a memset (round 6): blockIdx.y = the tensor.  mx: words 8 y + 4 / 8 y + 5 hold tensor y's two
// scale exponents, written by wc_pack2_kernel for the product (GemmArgs::mix_sptr); from word 16 on, one (max |w - rn16(w)|, max |w|) pair of float bits per absmax
// block, which wc_pack2_kernel reduces.  Every word is overwritten each step and nothing accumulates: no memset node, and the same captured graph works every step.
static __global__ __launch_bounds__(256) void wc_absmax2_kernel(const float* __restrict__ w0, const float* __restrict__ w1, size_t n, unsigned int* __restrict__ mx) {
    // one (max |w - rn16(w)|, max |w|) pair PER BLOCK at mx[16 + 2 (32 y + x)]: no atomics, nothing to reset (round 6: the accumulator form -- 512 atomicMax on two
    // addresses here, a 1 152-block ticket in the pack kernel to zero them again -- measured 10.8 + 17.0 us per step for 9 MB of traffic)
    const float* __restrict__ w = blockIdx.y ? w1 : w0;
    __shared__ float red[2][4];
    float md = 0.f, mw = 0.f;
    for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (size_t)gridDim.x * 1024) {
        float v[4];
        load4(w + i, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            md = fmaxf(md, fabsf(v[j] - h2f(f2h(v[j]))));
            mw = fmaxf(mw, fabsf(v[j]));
        }
    }
    md = wave_max(md); mw = wave_max(mw);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = md; red[1][threadIdx.x >> 6] = mw; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float* part = reinterpret_cast<float*>(mx) + 16 + 2 * (gridDim.x * blockIdx.y + blockIdx.x);
        part[0] = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
        part[1] = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
    }
}
// nparts = wc_absmax2_kernel's gridDim.x (<= 64)
static __global__ __launch_bounds__(256) void wc_pack2_kernel(const float* __restrict__ w0, const float* __restrict__ w1, int N, int K, unsigned int* __restrict__ mx, int nparts,
                                                              f16_t* __restrict__ out0, f16_t* __restrict__ out1) {
    const float* __restrict__ w = blockIdx.y ? w1 : w0;
    f16_t* __restrict__ out = blockIdx.y ? out1 : out0;
    __shared__ float mm[2];
    if (threadIdx.x < 64) {  // the tensor's maxima from the per-block pairs: one load per lane, a wave reduction
        const float* part = reinterpret_cast<const float*>(mx) + 16 + 2 * (nparts * blockIdx.y);
        float md = (int)threadIdx.x < nparts ? part[2 * threadIdx.x] : 0.f, mw = (int)threadIdx.x < nparts ? part[2 * threadIdx.x + 1] : 0.f;
        md = wave_max(md); mw = wave_max(mw);
        if (threadIdx.x == 0) { mm[0] = md; mm[1] = mw; }
    }
    __syncthreads();
    const float md = mm[0], mw = mm[1];
    const int sd = md > 0.f ? (int)floorf(log2f(6.0f / md)) + 1 : 0, sw = mw > 0.f ? (int)floorf(log2f(6.0f / mw)) + 1 : 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) { reinterpret_cast<int*>(mx)[8 * blockIdx.y + 4] = sd; reinterpret_cast<int*>(mx)[8 * blockIdx.y + 5] = sw; }
    const float fd = ldexpf(1.0f, sd), fw = ldexpf(1.0f, sw);
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i < (size_t)N * K) {
        const size_t r = i / K;
        const int c = (int)(i - r * K);
        float v[4];
        load4(w + i, v);
        f16_t* row = out + r * (size_t)(3 * K / 2);
        float h[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) h[j] = h2f(f2h(v[j]));
        *reinterpret_cast<uint2*>(row + c) = make_uint2(pack_h2(h[0], h[1]), pack_h2(h[2], h[3]));
        uint8_t* seg = reinterpret_cast<uint8_t*>(row + K);
        *reinterpret_cast<uint16_t*>(seg + (c >> 1)) = pack_fp4x4((v[0] - h[0]) * fd, (v[1] - h[1]) * fd, (v[2] - h[2]) * fd, (v[3] - h[3]) * fd);
        *reinterpret_cast<uint16_t*>(seg + (K >> 1) + (c >> 1)) = pack_fp4x4(v[0] * fw, v[1] * fw, v[2] * fw, v[3] * fw);
    }
}

// partial[b] = sum over the block's slice of dy * (a - x)      (d loss / d res; finished by reduce_sum)
template <typename T>
static __global__ __launch_bounds__(256) void adapter_dres_kernel(const T* __restrict__ dy, const T* __restrict__ a, const float* __restrict__ x,
                                                           float* __restrict__ partial, size_t n) {
    __shared__ float red[4];
    float s = 0.f;
    const size_t n4 = n >> 2;  // 4 elements per access; the tail (n % 4) goes to block 0
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        float d[4], av[4], xv[4];
        load4(dy + 4 * i, d);
        load4(a + 4 * i, av);
        load4(x + 4 * i, xv);
        s += (d[0] * (av[0] - xv[0]) + d[1] * (av[1] - xv[1])) + (d[2] * (av[2] - xv[2]) + d[3] * (av[3] - xv[3]));
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const size_t i = (n4 << 2) + threadIdx.x;
        s += Elem<T>::ld(dy + i) * (Elem<T>::ld(a + i) - x[i]);
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// out[0] (+)= scale * sum_i in[i]   -- single block, fixed order
static __global__ __launch_bounds__(256) void reduce_sum_kernel(const float* __restrict__ in, int n, float scale, float* __restrict__ out,
                                                         int accumulate) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += in[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float v = scale * ((red[0] + red[1]) + (red[2] + red[3]));
        out[0] = accumulate ? out[0] + v : v;
    }
}

// two independent sums in one launch (the two norms of the update: block b sums in_b into out_b, reduce_sum_kernel's order)
static __global__ __launch_bounds__(256) void reduce_sum2_kernel(const float* __restrict__ in0, const float* __restrict__ in1, int n, float* __restrict__ out0, float* __restrict__ out1) {
    __shared__ float red[4];
    const float* __restrict__ in = blockIdx.x ? in1 : in0;
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += in[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) (blockIdx.x ? out1 : out0)[0] = 1.0f * ((red[0] + red[1]) + (red[2] + red[3]));
}

// d loss / d residual_weight from the per-workgroup partials of sum dY * (A - x): reduce (fixed order), un-scale, chain through the
// sigmoid -- reduce_sum_kernel + dres_to_drw_kernel in one launch
static __global__ __launch_bounds__(256) void reduce_dres_to_drw_kernel(const float* __restrict__ in, int n, float scale, const float* __restrict__ rw,
                                                                 float* __restrict__ grad) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += in[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float dres = scale * ((red[0] + red[1]) + (red[2] + red[3]));
        const float res = 1.0f / (1.0f + expf(-rw[0]));
        grad[0] = dres * res * (1.f - res);
    }
}

static __global__ void sigmoid_scalar_kernel(float* x) { x[0] = 1.0f / (1.0f + expf(-x[0])); }

// residual_weight gradient: d/d rw = dres * res * (1 - res)
static __global__ void dres_to_drw_kernel(const float* __restrict__ dres, const float* __restrict__ rw, float* __restrict__ grad) {
    const float res = 1.0f / (1.0f + expf(-rw[0]));
    grad[0] = dres[0] * res * (1.f - res);
}

// ---- row sums of a [R, ld] matrix (bias gradients from the TRANSPOSED gradient: one row per output unit)
template <typename T>
static __global__ __launch_bounds__(256) void rowsum_kernel(const T* __restrict__ in, int ld, int cols, float* __restrict__ out, int rows, float alpha = 1.f) {
    __shared__ float red[4];
    const int row = blockIdx.x;  // one workgroup per row; ld % 4 == 0 (rows are 8/16-byte aligned)
    const T* r = in + (size_t)row * ld;
    float s = 0.f;
    const int c4 = cols & ~3;
    for (int c = threadIdx.x * 4; c < c4; c += 1024) {
        float v[4];
        load4(r + c, v);
        s += (v[0] + v[1]) + (v[2] + v[3]);
    }
    for (int c = c4 + threadIdx.x; c < cols; c += 256) s += Elem<T>::ld(r + c);
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[row] = alpha * ((red[0] + red[1]) + (red[2] + red[3]));
}
// column sums of a small [R, C] f32 matrix: out[c] = sum_r in[r, c]
__device__ __forceinline__ void colsum_tile(const float* __restrict__ in, int R, int C, float* __restrict__ out, int bx, float alpha = 1.f) {
    // 64 columns per block (lane = column: coalesced rows), rows split over the 4 waves with 4 independent
    // accumulators each, then a fixed-order combine
    __shared__ float red[4][64];
    const int x = threadIdx.x & 63, y = threadIdx.x >> 6;
    const int c = bx * 64 + x;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (c < C) {
        // the operand is global memory whoever calls (kernel argument or a pointer read from a job table, which the compiler would
        // otherwise treat as generic: flat loads, each waited for alone); sixteen rows are requested before the first add -- the
        // adds keep their order, so the sums are bit for bit those of the four-rows-at-a-time loop
        const __attribute__((address_space(1))) float* gin = (const __attribute__((address_space(1))) float*)in;
        int r = y;
        for (; r + 60 < R; r += 64) {
            float t[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) t[u] = gin[(size_t)(r + 4 * u) * C + c];
#pragma unroll
            for (int u = 0; u < 16; u += 4) {
                s0 += t[u];
                s1 += t[u + 1];
                s2 += t[u + 2];
                s3 += t[u + 3];
            }
        }
        for (; r + 12 < R; r += 16) {
            s0 += gin[(size_t)r * C + c];
            s1 += gin[(size_t)(r + 4) * C + c];
            s2 += gin[(size_t)(r + 8) * C + c];
            s3 += gin[(size_t)(r + 12) * C + c];
        }
        for (; r < R; r += 4) s0 += gin[(size_t)r * C + c];
    }
    red[y][x] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (y == 0 && c < C) out[c] = alpha * ((red[0][x] + red[1][x]) + (red[2][x] + red[3][x]));
}
static __global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ in, int R, int C, float* __restrict__ out, float alpha = 1.f) {
    colsum_tile(in, R, C, out, blockIdx.x, alpha);
}
// The adapter backward's three small reductions in one launch, behind its last GEMM (nothing but the norm pass reads their results): the two bias gradients
// (column sums of the per-row-block partials of adapter_dy_kernel and of the dH1 GEMM's epilogue) and d loss / d residual_weight.  Blocks [0, nb) and
// [nb, 2 nb) are colsum_kernel's, block 2 nb is reduce_dres_to_drw_kernel's: same arithmetic, same order.
static __global__ __launch_bounds__(256) void adapter_grad_finish_kernel(const float* __restrict__ cp1, int rows1, float* __restrict__ bias1, const float* __restrict__ cp0, int rows0,
                                                                  float* __restrict__ bias0, int D, float alpha, const float* __restrict__ dres_part, int n,
                                                                  const float* __restrict__ rw, float* __restrict__ drw) {
    const int nb = (D + 63) / 64;
    int b = (int)blockIdx.x;
    if (b < nb) { colsum_tile(cp1, rows1, D, bias1, b, alpha); return; }
    b -= nb;
    if (b < nb) { colsum_tile(cp0, rows0, D, bias0, b, alpha); return; }
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += dres_part[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float dres = alpha * ((red[0] + red[1]) + (red[2] + red[3]));
        const float res = 1.0f / (1.0f + expf(-rw[0]));
        drw[0] = dres * res * (1.f - res);
    }
}

// ---- masked, scaled ROW-major copy with column partial sums (16-bit modes: operand of the TN weight-gradient GEMM) ----------
//   out[r,c] = scale * in[r,c] * (mask[r,c] > 0)          part[blockIdx.y][c] = sum over the block's 64 rows of out[r,c]
// The partial sums (of the ROUNDED values, as the transposed-copy path's row sums were) give the bias gradient after one
// colsum_kernel over gridDim.y rows: fixed order, no atomics.  C % 4 == 0; rows >= R are not written (callers keep them zero).
template <typename T>
static __global__ __launch_bounds__(256) void mask_copy_colsum_kernel(const T* __restrict__ in, const T* __restrict__ mask, const float* __restrict__ scale_ptr,
                                                               float scale, T* __restrict__ out, float* __restrict__ part, int R, int C,
                                                               const float* __restrict__ x32 = nullptr, float* __restrict__ dres_part = nullptr) {
    // x32 / dres_part (the adapter's first masked copy): also the block's share of d loss / d res = sum in * (mask - x32), i.e.
    // dY * (A - x) of y = res*A + (1-res)*x (arp_dt/ARPDT.py:466-472), so that dY and A are read once for both results
    __shared__ float red[4][256];
    __shared__ float dred[4];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int c = blockIdx.x * 256 + tx * 4;
    const float s = scale_ptr ? scale * scale_ptr[0] : scale;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    float dsum = 0.f;
    if (c < C) {
#pragma unroll 4
        for (int i = 0; i < 16; ++i) {
            const int r = blockIdx.y * 64 + i * 4 + ty;
            if (r >= R) break;
            float v[4], m[4];
            load4(in + (size_t)r * C + c, v);
            load4(mask + (size_t)r * C + c, m);
            if (x32) {
                float x[4];
                load4(x32 + (size_t)r * C + c, x);
                dsum += (v[0] * (m[0] - x[0]) + v[1] * (m[1] - x[1])) + (v[2] * (m[2] - x[2]) + v[3] * (m[3] - x[3]));
            }
            T o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                Elem<T>::st(&o[e], m[e] > 0.f ? v[e] * s : 0.f);
                acc[e] += Elem<T>::ld(&o[e]);
            }
            *reinterpret_cast<uint2*>(out + (size_t)r * C + c) = *reinterpret_cast<const uint2*>(o);
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) red[ty][tx * 4 + e] = acc[e];
    if (dres_part) {
        dsum = wave_sum(dsum);
        if (tx == 0) dred[ty] = dsum;
    }
    __syncthreads();
    const int cc = blockIdx.x * 256 + threadIdx.x;
    if (cc < C) part[(size_t)blockIdx.y * C + cc] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    if (dres_part && threadIdx.x == 0) dres_part[blockIdx.y * gridDim.x + blockIdx.x] = (dred[0] + dred[1]) + (dred[2] + dred[3]);
}

// ---- LayerNorm forward (f32 in/out, saves nothing: backward recomputes the statistics) ------------------
static __global__ __launch_bounds__(256) void ln_fwd_f32_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                         float* __restrict__ y, int rows, int D, float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + (size_t)row * D;
    float s = 0.f;
    for (int c = lane; c < D; c += 64) s += xr[c];
    const float mean = wave_sum(s) / D;
    float q = 0.f;
    for (int c = lane; c < D; c += 64) { const float d = xr[c] - mean; q += d * d; }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / D + eps);
    for (int c = lane; c < D; c += 64) y[(size_t)row * D + c] = (xr[c] - mean) * rstd * w[c] + b[c];
}
// LayerNorm backward: dx (written or accumulated), and per-row contributions to dscale / dbias
// (dws[row, c] = dy*xhat, dbs[row, c] = dy; summed over rows by colsum_kernel).
static __global__ __launch_bounds__(256) void ln_bwd_f32_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ dy,
                                                         float* __restrict__ dx, int accumulate, float* __restrict__ dws,
                                                         float* __restrict__ dbs, int rows, int D, float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + (size_t)row * D;
    const float* dyr = dy + (size_t)row * D;
    float s = 0.f;
    for (int c = lane; c < D; c += 64) s += xr[c];
    const float mean = wave_sum(s) / D;
    float q = 0.f;
    for (int c = lane; c < D; c += 64) { const float d = xr[c] - mean; q += d * d; }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / D + eps);
    float s1 = 0.f, s2 = 0.f;  // sum(g), sum(g * xhat), g = dy * w
    for (int c = lane; c < D; c += 64) {
        const float xh = (xr[c] - mean) * rstd, gg = dyr[c] * w[c];
        s1 += gg;
        s2 += gg * xh;
        dws[(size_t)row * D + c] = dyr[c] * xh;
        dbs[(size_t)row * D + c] = dyr[c];
    }
    s1 = wave_sum(s1) / D;
    s2 = wave_sum(s2) / D;
    for (int c = lane; c < D; c += 64) {
        const float xh = (xr[c] - mean) * rstd, gg = dyr[c] * w[c];
        const float v = rstd * (gg - s1 - xh * s2);
        float* o = dx + (size_t)row * D + c;
        *o = accumulate ? *o + v : v;
    }
}

// ---- causal multi-head attention backward for the policy (L <= 64 tokens, head_dim <= 64), f32 ---------
// qkv [B*L, 3E], dout [B*L, E] -> dqkv [B*L, 3E].  One workgroup per (sample, head); probabilities are
// recomputed (arp_dt/layers.py:70-90: scale, masked fill, softmax).
static __global__ __launch_bounds__(64) void attn_bwd_small_kernel(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                            float* __restrict__ dqkv, int L, int E, int heads, float scale,
                                                            const float* __restrict__ alibi = nullptr) {
    extern __shared__ float sm[];
    const int hd = E / heads;
    const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
    const float slope = alibi ? alibi[h] : 0.f;  // config.alibi_bias: a constant added to the scores -- it changes P, not the form of dS
    float* q = sm;                // [L][hd]
    float* k = q + L * hd;        // [L][hd]
    float* v = k + L * hd;        // [L][hd]
    float* dO = v + L * hd;       // [L][hd]
    float* P = dO + L * hd;       // [L][L]
    float* dS = P + L * L;        // [L][L]
    const size_t ld = 3 * (size_t)E;
    for (int i = threadIdx.x; i < L * hd; i += 64) {
        const int t = i / hd, d = i - t * hd;
        const size_t row = (size_t)b * L + t;
        q[i] = qkv[row * ld + h * hd + d];
        k[i] = qkv[row * ld + E + h * hd + d];
        v[i] = qkv[row * ld + 2 * E + h * hd + d];
        dO[i] = dout[row * E + h * hd + d];
    }
    __syncthreads();
    // probabilities, one query row per thread
    for (int i = threadIdx.x; i < L; i += 64) {
        float mx = -INFINITY;
        for (int j = 0; j <= i; ++j) {
            float s = 0.f;
            for (int d = 0; d < hd; ++d) s = fmaf(q[i * hd + d], k[j * hd + d], s);
            s = s * scale + slope * (float)j;
            P[i * L + j] = s;
            mx = fmaxf(mx, s);
        }
        float sum = 0.f;
        for (int j = 0; j <= i; ++j) { const float e = expf(P[i * L + j] - mx); P[i * L + j] = e; sum += e; }
        const float inv = 1.0f / sum;
        // dP = dO . V^T ; dS = P * (dP - sum_j P dP)
        float dot = 0.f;
        for (int j = 0; j <= i; ++j) {
            const float p = P[i * L + j] * inv;
            P[i * L + j] = p;
            float dp = 0.f;
            for (int d = 0; d < hd; ++d) dp = fmaf(dO[i * hd + d], v[j * hd + d], dp);
            dS[i * L + j] = dp;
            dot += p * dp;
        }
        for (int j = 0; j < L; ++j) {
            if (j <= i) dS[i * L + j] = P[i * L + j] * (dS[i * L + j] - dot) * scale;
            else { dS[i * L + j] = 0.f; P[i * L + j] = 0.f; }
        }
    }
    __syncthreads();
    // dq[i] = sum_j dS[i,j] k[j];  dk[j] = sum_i dS[i,j] q[i];  dv[j] = sum_i P[i,j] dO[i]
    for (int idx = threadIdx.x; idx < L * hd; idx += 64) {
        const int t = idx / hd, d = idx - t * hd;
        float dq = 0.f, dk = 0.f, dv = 0.f;
        for (int j = 0; j < L; ++j) {
            dq = fmaf(dS[t * L + j], k[j * hd + d], dq);
            dk = fmaf(dS[j * L + t], q[j * hd + d], dk);
            dv = fmaf(P[j * L + t], dO[j * hd + d], dv);
        }
        const size_t row = (size_t)b * L + t;
        dqkv[row * ld + h * hd + d] = dq;
        dqkv[row * ld + E + h * hd + d] = dk;
        dqkv[row * ld + 2 * E + h * hd + d] = dv;
    }
}

// ---- token assembly (arp_dt/ARPDT.py:159-172,278-293): per time step [image, rtg, action] -------------
// tok[(b*T + t)*3 + 0] = img[b*T+t];  +1 = rtg[b*T+t] * Wr;  +2 = Emb[action[b*T+t]]
// tps = 2 (model BC, arp_dt/BC.py:141-142): per time step [image, action], rtg and Wr unused
static __global__ __launch_bounds__(256) void tokens_fwd_kernel(const float* __restrict__ img, const float* __restrict__ rtg,
                                                         const int* __restrict__ action, const float* __restrict__ Wr,
                                                         const float* __restrict__ emb, float* __restrict__ tok, int R, int E, int tps) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= R * E) return;
    const int r = i / E, e = i - r * E;
    tok[((size_t)r * tps + 0) * E + e] = img[i];
    if (tps == 3) tok[((size_t)r * 3 + 1) * E + e] = rtg[r] * Wr[e];
    tok[((size_t)r * tps + tps - 1) * E + e] = emb[(size_t)action[r] * E + e];
}
// backward: dimg = dtok[.,0];  dWr[e] = sum_r rtg[r]*dtok[r,1,e];  dEmb[a,e] = sum_{r: action=a} dtok[r,2,e]   (tps = 2: no dWr, the action token is 1)
static __global__ __launch_bounds__(256) void tokens_bwd_kernel(const float* __restrict__ dtok, const float* __restrict__ rtg,
                                                         const int* __restrict__ action, float* __restrict__ dimg,
                                                         float* __restrict__ dWr, float* __restrict__ demb, int R, int E, int n_actions, int tps) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    float wr = 0.f;
    for (int a = 0; a < n_actions; ++a) demb[(size_t)a * E + e] = 0.f;
    for (int r = 0; r < R; ++r) {
        dimg[(size_t)r * E + e] = dtok[((size_t)r * tps + 0) * E + e];
        if (tps == 3) wr += rtg[r] * dtok[((size_t)r * 3 + 1) * E + e];
        demb[(size_t)action[r] * E + e] += dtok[((size_t)r * tps + tps - 1) * E + e];
    }
    if (tps == 3) dWr[e] = wr;
}

// gather / scatter of the head inputs (arp_dt/ARPDT.py:203-205): action head <- rtg-token rows (1::3),
// return head <- image-token rows (0::3).  tps = 2 (BC.py:166): action head <- image-token rows (0::2), no return head (r_in unused)
static __global__ __launch_bounds__(256) void heads_gather_kernel(const float* __restrict__ hf, float* __restrict__ a_in, float* __restrict__ r_in,
                                                           int R, int E, int tps) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= R * E) return;
    const int r = i / E, e = i - r * E;
    if (tps == 3) {
        r_in[i] = hf[((size_t)r * 3 + 0) * E + e];
        a_in[i] = hf[((size_t)r * 3 + 1) * E + e];
    } else {
        a_in[i] = hf[((size_t)r * 2 + 0) * E + e];
    }
}
static __global__ __launch_bounds__(256) void heads_scatter_kernel(const float* __restrict__ da_in, const float* __restrict__ dr_in,
                                                            float* __restrict__ dhf, int R, int E, int tps) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= R * E) return;
    const int r = i / E, e = i - r * E;
    if (tps == 3) {
        dhf[((size_t)r * 3 + 0) * E + e] = dr_in[i];
        dhf[((size_t)r * 3 + 1) * E + e] = da_in[i];
        dhf[((size_t)r * 3 + 2) * E + e] = 0.f;
    } else {
        dhf[((size_t)r * 2 + 0) * E + e] = da_in[i];
        dhf[((size_t)r * 2 + 1) * E + e] = 0.f;
    }
}

// ---- elementwise backward helpers -----------------------------------------------------------------------
enum { EW_RELU_BWD = 0, EW_TANH_BWD = 1, EW_GELU_BWD = 2 };
// RELU_BWD: out = g * (y > 0)   (ref = activation output)
// TANH_BWD: out = g * (1 - y^2) (ref = activation output)
// GELU_BWD: out = g * gelu_tanh'(u) (ref = PRE-activation)
static __global__ __launch_bounds__(256) void ew_bwd_kernel(const float* __restrict__ g, const float* __restrict__ ref, float* __restrict__ out,
                                                     size_t n, int op) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float r = ref[i];
    float d;
    if (op == EW_RELU_BWD) d = r > 0.f ? 1.f : 0.f;
    else if (op == EW_TANH_BWD) d = 1.f - r * r;
    else {
        const float c = 0.7978845608028654f, a = 0.044715f;
        const float t = tanhf(c * (r + a * r * r * r));
        d = 0.5f * (1.f + t) + 0.5f * r * (1.f - t * t) * c * (1.f + 3.f * a * r * r);
    }
    out[i] = g[i] * d;
}
static __global__ __launch_bounds__(256) void gelu_fwd_kernel(const float* __restrict__ u, float* __restrict__ y, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = apply_act<ACT_GELU_TANH>(u[i]);
}

// ---- losses (arp_dt/ARPDT.py:238-261,498-507), single block; also the gradients w.r.t. logits / return ---
// metrics: [0] loss = trans + lambda*ret, [1] acc (fraction), [2] trans_loss, [3] return_loss
// ret == nullptr (model BC, arp_dt/BC.py:175-181,230-241): the cross-entropy alone, no squared error, dret / rtg unused
static __global__ __launch_bounds__(256) void loss_kernel(const float* __restrict__ logits, const float* __restrict__ ret,
                                                   const int* __restrict__ action, const float* __restrict__ rtg, int R, int NA,
                                                   float lambda, float* __restrict__ metrics, float* __restrict__ dlogits,
                                                   float* __restrict__ dret) {
    __shared__ float red[3][4];
    float ce = 0.f, hit = 0.f, se = 0.f;
    for (int r = threadIdx.x; r < R; r += 256) {
        const float* l = logits + (size_t)r * NA;
        float mx = l[0];
        int am = 0;
        for (int c = 1; c < NA; ++c)
            if (l[c] > mx) { mx = l[c]; am = c; }
        float sum = 0.f;
        for (int c = 0; c < NA; ++c) sum += expf(l[c] - mx);
        const float lse = logf(sum) + mx;
        const int lab = action[r];
        ce += lse - l[lab];
        hit += (am == lab) ? 1.f : 0.f;
        for (int c = 0; c < NA; ++c) dlogits[(size_t)r * NA + c] = (expf(l[c] - lse) - (c == lab ? 1.f : 0.f)) / ((float)R * NA);
        if (ret) {
            const float d = ret[r] - rtg[r];
            se += d * d;
            dret[r] = lambda * 2.f * d / (float)R;
        }
    }
    ce = wave_sum(ce); hit = wave_sum(hit); se = wave_sum(se);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = ce; red[1][threadIdx.x >> 6] = hit; red[2][threadIdx.x >> 6] = se; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float tce = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        const float th = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
        const float tse = (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]);
        const float trans = tce / ((float)R * NA), rl = tse / (float)R;
        metrics[0] = trans + lambda * rl;
        metrics[1] = th / (float)R;
        metrics[2] = trans;
        metrics[3] = rl;
    }
}

// ---- optimizer ---------------------------------------------------------------------------------------------
// partial[b] = sum of x^2 over the block's grid-stride slice of [begin, end)
static __global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* __restrict__ x, size_t n, float* __restrict__ partial) {
    __shared__ float red[4];
    float s = 0.f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) s += x[i] * x[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
// One pass for both norms of the update: pg[b] = sum (g*gscale + wd*p [i < n_decay])^2 (the gradient of loss + L2 term,
// averaged over ranks), pp[b] = sum p^2 over i < n_decay (weight_l2 of main_procgen.py:114-117).
static __global__ __launch_bounds__(256) void norms_partial_kernel(const float* __restrict__ g, const float* __restrict__ p, size_t n, size_t n_decay,
                                                                   float gscale, float wd, float* __restrict__ pg, float* __restrict__ pp) {
    // n and n_decay are multiples of 4 (every tensor's offset is): 16-byte accesses, fixed grid-stride order
    __shared__ float red[2][4];
    float sg = 0.f, sp = 0.f;
    const size_t n4 = n >> 2, d4 = n_decay >> 2;
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
    const float4* __restrict__ p4 = reinterpret_cast<const float4*>(p);
    auto term = [&](size_t i, const float4 gv, const float4 pv) {
        float g0 = gv.x * gscale, g1 = gv.y * gscale, g2 = gv.z * gscale, g3 = gv.w * gscale;
        if (i < d4) {
            g0 += wd * pv.x; g1 += wd * pv.y; g2 += wd * pv.z; g3 += wd * pv.w;
            sp += (pv.x * pv.x + pv.y * pv.y) + (pv.z * pv.z + pv.w * pv.w);
        }
        sg += (g0 * g0 + g1 * g1) + (g2 * g2 + g3 * g3);
    };
    // four grid-stride steps' loads (g and p, p unconditionally: it is n long) in flight before the first add; the adds keep the
    // one-step-at-a-time order, so the sums are bit for bit the same (two loads in flight per lane ran this pass at 4.9 TB/s)
    const size_t stride = (size_t)gridDim.x * 256;
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (; i + 3 * stride < n4; i += 4 * stride) {
        float4 gv[4], pv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            gv[u] = g4[i + u * stride];
            pv[u] = p4[i + u * stride];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) term(i + u * stride, gv[u], pv[u]);
    }
    for (; i < n4; i += stride) term(i, g4[i], p4[i]);
    sg = wave_sum(sg);
    sp = wave_sum(sp);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sg; red[1][threadIdx.x >> 6] = sp; }
    __syncthreads();
    if (threadIdx.x == 0) {
        pg[blockIdx.x] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        pp[blockIdx.x] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
}
// g += wd * p on a range (the explicit L2 term of main_procgen.py:114-117 differentiates to wd * p)
static __global__ __launch_bounds__(256) void add_scaled_kernel(float* __restrict__ g, const float* __restrict__ p, float wd, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) g[i] += wd * p[i];
}
// scal: [0] = sum of squares of the (already averaged-over-ranks) gradient.
// optax.clip_by_global_norm(c) then adam (b1, b2, eps outside the sqrt, bias correction with t = step+1);
// the adamw decay mask of the reference is all-False, so no decoupled decay.
// The L2 term's gradient wd*p (first n_decay entries) is added here, not materialised: g holds the raw (rank-summed) loss
// gradient, scal[0] the squared norm of g*gscale + wd*p from norms_partial_kernel.
// mirror (16-bit modes): the operand-type copy of the first n_mirror parameters (the three big Dense kernels, device layout
// [out, in] = the NT operand layout), written here so that the next step's forward needs no conversion pass over them.
template <typename TM>
static __global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ mu,
                                                   float* __restrict__ nu, const float* __restrict__ scal, float gscale, float wd, size_t n_decay,
                                                   float clip, float lr, float b1, float b2, float eps, float bc1, float bc2, size_t n,
                                                   TM* __restrict__ mirror, size_t n_mirror, int reverse) {
    // one float4 per thread; n, n_decay, n_mirror are multiples of 4.  reverse: the workgroups walk the state from its end -- the norm pass
    // just read g and p front to back, so their tails are what the Infinity Cache still holds (element-wise arithmetic: same result)
    const size_t i = (size_t)(reverse ? gridDim.x - 1 - blockIdx.x : blockIdx.x) * 256 + threadIdx.x;
    if (i >= (n >> 2)) return;
    const float gnorm = sqrtf(scal[0]);
    // A non-finite gradient norm (an f16 backward activation that overflowed its fixed power-of-two scale: a loss spike, huge rtg
    // targets at tiny B*window) would turn clip / inf * inf into NaN in EVERY parameter and moment, for good.  Such a step is
    // dropped instead: parameters, moments and the operand mirror keep their values (the step counter still advances, and the
    // caller sees it in aux: grad_norm is not finite).
    if (!(gnorm < 3.0e38f)) return;
    const float s = (gnorm < clip) ? 1.0f : clip / gnorm;
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 pv = reinterpret_cast<float4*>(p)[i];
    float4 mv = reinterpret_cast<float4*>(mu)[i];
    float4 vv = reinterpret_cast<float4*>(nu)[i];
    const float dw = (i < (n_decay >> 2)) ? wd : 0.f;
    float gg[4] = {gv.x, gv.y, gv.z, gv.w}, pp[4] = {pv.x, pv.y, pv.z, pv.w}, mm[4] = {mv.x, mv.y, mv.z, mv.w}, nn[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float gi = (gg[e] * gscale + dw * pp[e]) * s;
        mm[e] = b1 * mm[e] + (1.f - b1) * gi;
        nn[e] = b2 * nn[e] + (1.f - b2) * gi * gi;
        pp[e] -= lr * (mm[e] / bc1) / (sqrtf(nn[e] / bc2) + eps);
    }
    reinterpret_cast<float4*>(mu)[i] = make_float4(mm[0], mm[1], mm[2], mm[3]);
    reinterpret_cast<float4*>(nu)[i] = make_float4(nn[0], nn[1], nn[2], nn[3]);
    reinterpret_cast<float4*>(p)[i] = make_float4(pp[0], pp[1], pp[2], pp[3]);
    if constexpr (sizeof(TM) == 2) {
        if (mirror && i < (n_mirror >> 2)) store4(mirror + 4 * i, pp[0], pp[1], pp[2], pp[3]);
    }
}

}  // namespace arp
