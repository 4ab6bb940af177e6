// Weight-streaming NT GEMM for M <= 16 activation rows (the fine-tuned reward's head at rollout size: Wint [6144, 9216], fc1 [13312, 6656], fc2 [6656, 13312] at
// the real geometry -- 468 MB of 16-bit weights per call, each byte of which is used once).  16-bit operand types only.
//
// One wave owns 16 output columns of one K slice: its lanes load the 16 weight rows straight into VGPRs with 16-byte loads (lane = row fr = lane % 16, 8 k
// values at fg = lane / 16: the B-side fragment of v_mfma_f32_16x16x32 as stored, no LDS round trip), eight K steps of loads ahead of their MFMAs.  The <= 16
// activation rows of the slice, zero-padded to 16, are staged once per workgroup in LDS (<= 1024 k per chunk) and read as the other operand.  f32 accumulation;
// a lane ends with out[m = fr][n = n0 + 4 fg + i].  Grid = (ceil(N / 64), S): the split over K fills the chip where N alone does not; partials are raw f32
// slabs [S][M][N] summed in slab order by launch_splitk_reduce (bias, ReLU, output type): no atomics, bit-reproducible, and a row's result depends on that
// row alone.  Longest summation chain of one output: the kper products of a slice (32 inside each MFMA, the MFMAs chained through the accumulator), then S slabs.
#pragma once
#include "common.h"

namespace arp {

struct RowsArgs {
    const void* A;   // [M, lda] T
    const void* W;   // [N, ldw] T
    float* part;     // [S][M][N] f32
    int M, N, K, lda, ldw;
    int kper;        // k values per slice (a multiple of 64)
};
constexpr int ROWS_MAX_M = 16, ROWS_KC = 1024, ROWS_LDS_LD = ROWS_KC + 8;  // (+ 8 elements: the 16 rows of a fragment read start in different banks)

inline bool rows_gemm_supported(int M, int N, int K, int lda, int ldw, const void* A, const void* W) {
    return M >= 1 && M <= ROWS_MAX_M && K > 0 && K % 64 == 0 && N > 0 && N % 16 == 0 && lda >= K && ldw >= K && lda % 8 == 0 && ldw % 8 == 0 &&
           ((uintptr_t)A & 15) == 0 && ((uintptr_t)W & 15) == 0;
}
// slices of K the dispatcher asks for: about four workgroups per CU
inline int rows_gemm_split(int N, int K) {
    const int nk = K / 64, blocks = (N + 63) / 64;
    int S = std::max(1, std::min(nk, (1024 + blocks - 1) / blocks));
    const int per = (nk + S - 1) / S;
    return (nk + per - 1) / per;
}

template <typename T>
static __global__ __launch_bounds__(256) void ft_rows_gemm_kernel(RowsArgs g) {
    __shared__ __attribute__((aligned(16))) uint16_t As[16 * ROWS_LDS_LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 15, fg = lane >> 4;
    const int n0 = blockIdx.x * 64 + wave * 16;
    const bool active = n0 < g.N;  // (N % 16 == 0: an active wave owns 16 whole columns)
    const int k0 = blockIdx.y * g.kper, k1 = min(g.K, k0 + g.kper);
    const uint16_t* A = static_cast<const uint16_t*>(g.A);
    const uint16_t* wrow = static_cast<const uint16_t*>(g.W) + (size_t)(active ? n0 + fr : 0) * g.ldw + fg * 8;
    const uint16_t* arow = As + fr * ROWS_LDS_LD + fg * 8;
    f32x4_v acc = {0.f, 0.f, 0.f, 0.f};
    for (int kc = k0; kc < k1; kc += ROWS_KC) {
        const int kn = min(ROWS_KC, k1 - kc);  // a multiple of 64
        if (kc != k0) __syncthreads();
        for (int i = threadIdx.x; i < 16 * (kn >> 3); i += 256) {  // 16 rows x kn / 8 vectors of 8 elements; rows M .. 15 are zeros
            const int m = i / (kn >> 3), v = i - m * (kn >> 3);
            u32x4_v x = {0u, 0u, 0u, 0u};
            if (m < g.M) x = *reinterpret_cast<const u32x4_v*>(A + (size_t)m * g.lda + kc + v * 8);
            *reinterpret_cast<u32x4_v*>(As + m * ROWS_LDS_LD + v * 8) = x;
        }
        __syncthreads();
        if (!active) continue;
        int k = 0;
        for (; k + 256 <= kn; k += 256) {  // eight 16-byte weight loads per lane in flight ahead of the MFMAs
            u32x4_v wf[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) wf[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_v*>(wrow + kc + k + 32 * j));
#pragma unroll
            for (int j = 0; j < 8; ++j) acc = mfma16<T>(wf[j], *reinterpret_cast<const u32x4_v*>(arow + k + 32 * j), acc);
        }
        for (; k < kn; k += 64) {
            u32x4_v wf[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) wf[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_v*>(wrow + kc + k + 32 * j));
#pragma unroll
            for (int j = 0; j < 2; ++j) acc = mfma16<T>(wf[j], *reinterpret_cast<const u32x4_v*>(arow + k + 32 * j), acc);
        }
    }
    if (!active || fr >= g.M) return;
    float* o = g.part + ((size_t)blockIdx.y * g.M + fr) * g.N + n0 + fg * 4;  // D[n = 4 fg + i][m = fr]
    *reinterpret_cast<float4*>(o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
}

// part must hold S * M * N floats.  S >= 1 slices of ceil(K / 64 / S) * 64 k values each (the last may be shorter; S is lowered to the slices that are not empty).
template <typename T>
static int launch_rows_gemm(hipStream_t st, const void* A, int lda, const void* W, int ldw, float* part, int M, int N, int K, int* S_io) {
    static_assert(sizeof(T) == 2, "16-bit operand types only");
    if (!rows_gemm_supported(M, N, K, lda, ldw, A, W)) return fail("rows_gemm: needs 1 <= M <= 16, K % 64 == 0, N % 16 == 0, 16-byte aligned operands and leading dimensions");
    const int nk = K / 64;
    int S = std::max(1, std::min(*S_io, nk));
    const int per = (nk + S - 1) / S;
    S = (nk + per - 1) / per;
    *S_io = S;
    RowsArgs g{A, W, part, M, N, K, lda, ldw, per * 64};
    hipLaunchKernelGGL((ft_rows_gemm_kernel<T>), dim3((N + 63) / 64, S), dim3(256), 0, st, g);
    ARP_HIP_OK(hipGetLastError());
    return 0;
}

}  // namespace arp
