// Key-blocked (online-softmax) self-attention for sequences past the LDS-resident kernels of attention.h: head_dim 64, 289 .. 1024 keys.
// The goal-conditioned M3AE pass (class token + 256 frame patches + 256 goal patches = 513 tokens) is what needs it: at 513 keys neither a head's K / V
// (2 x 513 x 128 B as 16-bit, twice that as f32) nor a query block's score row (136 registers per lane) fits where attn_mfma_kernel keeps them.
//
//   attn_long_kernel<T>   : binary16 / bf16.  Same plan as attn_mfma_kernel -- S^T = K.Q^T on v_mfma_f32_16x16x32, the softmax'd accumulator is the B operand of
//                           O^T = V^T.P^T, V^T fragments by ds_read_b64_tr_b16 -- with the keys walked in blocks of 64 through a ring of three LDS stages.
//   attn_long_f32_kernel  : exact f32, the parity mode.  attn_valu_kernel's arithmetic (one query per lane, one key at a time, expf), K / V staged
//                           128 keys at a time: a row comes out with the bits attn_valu_kernel gives it.
//   attn_long_masked_kernel<T>, attn_long_f32_masked_kernel : the same two bodies with a per-sample KEY MASK (one bit per key; M3AE's image + text pass takes
//                           its padded instruction tokens out of every softmax), for any N from 1 to 1024.  The unmasked kernels are the MASKED = false
//                           instances of the bodies and compile none of it.
//
// What a row's bits depend on: its own q row, the K / V rows, N, causal.  Not on B, the workgroup, the wave or gridDim.y: a 16-query block is always
// computed by one wave, over key blocks 0, 1, 2, ... in that order, and query blocks never share an accumulator.
#pragma once
#include "attention.h"

namespace arp {

constexpr int ATTN_LONG_MIN = 289, ATTN_LONG_MAX = 1024;  // key counts the launcher sends here
constexpr int ATTN_LONG_KB = 64;                           // keys per block
constexpr int ATTN_LONG_RING = 3;                          // LDS stages: one being read, one landed or landing, one being requested
constexpr int ATTN_LONG_LDS = ATTN_LONG_RING * ATTN_LONG_KB * 256;

// One workgroup (4 waves) takes a TILE of four 16-query blocks, one per wave, and walks the key blocks of its (sample, head) once per tile.
// Stage image = attn_mfma_kernel's: K [64 keys][128 B] then V [64 keys][128 B], 16-byte chunk index XOR (key & 7), filled by LDS-DMA with the swizzle on
// the source address (a block starts at a multiple of 64 keys, so key & 7 is the row's own low bits).  A wave requests two 8-row pieces of K and of V per
// block: 4 LDS-DMA instructions, which is what the counted waits below count.
// Iteration j: wait until this wave's pieces of block j have landed (vmcnt(4) leaves block j + 1 in flight, vmcnt(0) on the last block) -> barrier (every
// wave's pieces of block j are in LDS, and every wave is done reading block j - 1) -> request block j + 2 into the stage block j - 1 occupied -> compute
// block j.  One barrier per block; a stage is read only after the wait and the barrier that retire it, and rewritten only after the barrier that follows
// its last read.
// Online softmax per query (= per lane column fr; the four lane groups fg hold different keys of the same query): running maximum m of the raw scores and
// this lane's share l of the running sum.  m starts at -inf and block 0 is computed for every query block with key 0 visible, so from block 0 on m is
// finite and the rescale factor 2^((m - m') c2) is 2^-inf = 0 once and in (0, 1] afterwards: never (-inf) - (-inf).
// Causal: a tile stops at the last block one of its queries can see; a wave skips the blocks wholly behind its own 16 queries (it still stages and meets
// the barriers).  The upper 32 keys of a block are skipped when they are all pad (>= N) or all behind the wave's queries.  Pad keys alias key N - 1.
// The V^T fragment reads are inline asm.  Issued through the builtin, hipcc (7.0) cannot tell the transposing read's address from the LDS-DMA's and puts an
// s_waitcnt vmcnt(0) in front of the first one of every key block: blocks j + 1 and j + 2, requested to arrive during block j's work, were drained in the
// middle of it and the counted waits above had nothing left to count.  An asm statement has no memory operand for that analysis to look at.  The eight
// reads of a 32-key step (four d-tiles x two 16-key halves; the step and the half are instruction offsets) go out right behind the QK^T MFMAs, so that they
// land under the softmax's VALU work; the wait is a second statement that takes the eight results as in-out operands -- whatever consumes them is data-
// dependent on the wait and cannot be scheduled ahead of it.  lgkmcnt(0) also covers the compiler's own LDS reads issued before: stricter, never weaker
// (LDS operations return in order, and the compiler's counts for its own reads only ever see more outstanding behind them, not fewer).
#define ARP_AL_VREAD(OFF, R, A)                                                                                                        \
    asm volatile("ds_read_b64_tr_b16 %0, %8 offset:%12\n\tds_read_b64_tr_b16 %1, %8 offset:%13\n\t"                                  \
                 "ds_read_b64_tr_b16 %2, %9 offset:%12\n\tds_read_b64_tr_b16 %3, %9 offset:%13\n\t"                                  \
                 "ds_read_b64_tr_b16 %4, %10 offset:%12\n\tds_read_b64_tr_b16 %5, %10 offset:%13\n\t"                                \
                 "ds_read_b64_tr_b16 %6, %11 offset:%12\n\tds_read_b64_tr_b16 %7, %11 offset:%13"                                     \
                 : "=&v"(R[0]), "=&v"(R[1]), "=&v"(R[2]), "=&v"(R[3]), "=&v"(R[4]), "=&v"(R[5]), "=&v"(R[6]), "=&v"(R[7])              \
                 : "v"(A[0]), "v"(A[1]), "v"(A[2]), "v"(A[3]), "n"(OFF), "n"((OFF) + 2048)                                              \
                 : "memory")
#define ARP_AL_VWAIT(R)                                                                                                               \
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(R[0]), "+v"(R[1]), "+v"(R[2]), "+v"(R[3]), "+v"(R[4]), "+v"(R[5]), "+v"(R[6]), "+v"(R[7]) : : "memory")

// MASKED: a key mask per sample (the comment above attn_long_masked_kernel); the unmasked instance compiles none of it.
template <typename T, bool MASKED>
__device__ __forceinline__ void attn_long_body(const T* __restrict__ qkv, T* __restrict__ out, int N, int D, int heads, float scale, int causal, int nq,
                                               const uint32_t* __restrict__ mask, int mask_stride) {
    constexpr int KB = ATTN_LONG_KB, STAGE = KB * 256;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
    const size_t ld = 3 * (size_t)D;
    const T* base = qkv + (size_t)b * N * ld + h * 64;
    const int fr = lane & 15, fg = lane >> 4, trq = fr >> 2, trp = fr & 3;
    const int prow = lane >> 3, pch = lane & 7;
    const int nqb = (nq + 15) >> 4, ntiles = (nqb + 3) >> 2, nkb = (N + KB - 1) / KB;
    const float c2 = scale * 1.4426950408889634f;  // exp(x * scale) = exp2(x * c2)
    const uint32_t* mw = MASKED ? mask + (size_t)b * mask_stride : nullptr;  // this sample's visible-bit words: workgroup-uniform
    // transposing-read addressing (attn_mfma_kernel's): lane 4q + p of a 16-lane group points at row 4 fg + q (+ 32 st, + 16 for the second half: neither
    // changes row & 7), columns 4p .. 4p + 3 of the 16-column block dt.  vrd[dt]: this lane's byte address inside the V image of ring stage 0.
    uint32_t vrd[4];
    {
        const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
        const int row = 4 * fg + trq;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) vrd[dt] = lds0 + KB * 128 + row * 128 + (((2 * dt + (trp >> 1)) ^ (row & 7)) << 4) + (trp & 1) * 8;
    }

    auto stage = [&](int jb, int buf) {
        char* Kd = smem + buf * STAGE;
        char* Vd = Kd + KB * 128;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int p = wave + 4 * i;
            const int key = jb * KB + p * 8 + prow;
            const int kk = key < N ? key : N - 1;
            const T* src = base + (size_t)kk * ld + ((pch ^ (key & 7)) << 3);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + D),
                                             (__attribute__((address_space(3))) void*)(Kd + p * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + 2 * D),
                                             (__attribute__((address_space(3))) void*)(Vd + p * 1024), 16, 0, 0);
        }
    };

    for (int tile = blockIdx.y; tile < ntiles; tile += gridDim.y) {
        const int qb = tile * 4 + wave;
        const bool active = qb < nqb;
        const int qidx = qb * 16 + fr;
        const int qrow = qidx < N ? qidx : N - 1;
        u32x4_v qf[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) qf[ks] = *reinterpret_cast<const u32x4_v*>(base + qrow * ld + ks * 32 + fg * 8);
        const int klim = causal ? (qidx < N ? qidx + 1 : N) : N;
        const int nk = causal ? min(nkb, tile + 1) : nkb;  // a tile is 64 queries = one key block: queries 64 t .. 64 t + 63 see blocks 0 .. t
        // the Q fragments are in and the previous tile's output stores are retired: from here on only LDS-DMA is outstanding, so the counts below are exact;
        // the barrier keeps this tile's first requests behind the other waves' last reads of the previous tile
        // (the empty statement "uses" the Q fragments HERE: left to their first MFMA, hipcc waits vmcnt(0) for them at the head of the key loop, behind the two
        //  requests below, and blocks 0 and 1 are drained before block 0's work starts)
        asm volatile("" : "+v"(qf[0]), "+v"(qf[1]));
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        stage(0, 0);
        if (nk > 1) stage(1, 1);

        float m = -INFINITY, l = 0.f;
        f32x4_v o[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4_v{0.f, 0.f, 0.f, 0.f};
        int buf = 0;
        for (int j = 0; j < nk; ++j) {
            if (j + 1 < nk) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (j + 2 < nk) stage(j + 2, buf == 0 ? 2 : buf - 1);
            const int kb0 = j * KB;
            // MASKED: the block's two words, pad keys (>= N) cleared -- bit i of vis <-> key kb0 + i.  Uniform over the workgroup; read behind the barrier
            // and the requests, so the ring protocol above sees the same waits, barriers and requests whatever the words hold.
            uint64_t vis = ~0ull;
            if constexpr (MASKED) {
                const int left = N - kb0;  // >= 1
                const uint32_t lo = mw[2 * j] & (left >= 32 ? 0xffffffffu : (1u << left) - 1u);
                const uint32_t hi = left > 32 ? mw[2 * j + 1] & (left >= 64 ? 0xffffffffu : (1u << (left - 32)) - 1u) : 0u;
                vis = (uint64_t)hi << 32 | lo;
            }
            if (active && !(causal && kb0 > qb * 16 + 15) && !(MASKED && vis == 0)) {
                const char* Ks = smem + buf * STAGE;
                const char* Vs = Ks + KB * 128;
                const bool upper = MASKED ? (vis >> 32) != 0 : kb0 + 32 < N && !(causal && kb0 + 32 > qb * 16 + 15);  // wave-uniform
                // S^T tile kt: rows = keys kb0 + 16 kt + 4 fg + r, column = query fr
                f32x4_v s[4];
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) {
                    if (kt < 2 || upper) {
                        s[kt] = f32x4_v{0.f, 0.f, 0.f, 0.f};
                        const int krow = kt * 16 + fr;
#pragma unroll
                        for (int ks = 0; ks < 2; ++ks) {
                            const u32x4_v kf = *reinterpret_cast<const u32x4_v*>(Ks + krow * 128 + (((ks * 4 + fg) ^ (krow & 7)) << 4));
                            s[kt] = mfma16<T>(kf, qf[ks], s[kt]);
                        }
                    } else {
                        s[kt] = f32x4_v{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
                    }
                }
                // this block's V^T fragments: requested now, waited for in front of the PV MFMAs
                uint32_t va[4];
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) va[dt] = vrd[dt] + buf * STAGE;
                u32x2_v v0[8], v1[8];  // [2 dt + half] of the lower / upper 32 keys
                ARP_AL_VREAD(0, v0, va);
                if (upper) ARP_AL_VREAD(4096, v1, va);
                // masks only where the block holds a pad key or a key behind one of the wave's queries
                if constexpr (MASKED) {
                    if (vis != ~0ull) {  // a hidden or pad key in the block
                        const uint64_t mine = vis >> (fg * 4);
#pragma unroll
                        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                            for (int r = 0; r < 4; ++r) s[kt][r] = (mine >> (kt * 16 + r)) & 1 ? s[kt][r] : -INFINITY;
                    }
                } else if (kb0 + KB > N || (causal && kb0 + KB - 1 > qb * 16)) {
#pragma unroll
                    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int key = kb0 + kt * 16 + fg * 4 + r;
                            s[kt][r] = key < klim ? s[kt][r] : -INFINITY;
                        }
                }
                float mx = -INFINITY;
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) mx = fmaxf(fmaxf(fmaxf(s[kt][0], s[kt][1]), fmaxf(s[kt][2], s[kt][3])), mx);
                mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
                mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
                const float mn = fmaxf(m, mx);  // finite from block 0 on
                const float alpha = __builtin_amdgcn_exp2f((m - mn) * c2);  // block 0: 2^-inf = 0; afterwards both finite
                const float mc = mn * c2;
                float sum = 0.f;
#pragma unroll
                for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float p = __builtin_amdgcn_exp2f(fmaf(s[kt][r], c2, -mc));  // masked keys: 2^-inf = 0
                        s[kt][r] = p;
                        sum += p;
                    }
                l = fmaf(l, alpha, sum);
                m = mn;
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) o[dt] *= alpha;
                // O^T[d][q] += sum_key V^T[d][key] P^T[key][q]: k-slot (fg, i) of step st <-> key kb0 + 32 st + 16 (i >> 2) + 4 fg + (i & 3)
                auto pv = [&](int st, const u32x2_v (&vf)[8]) {
                    u32x4_v pb;
                    pb[0] = pack2<T>(s[2 * st][0], s[2 * st][1]);
                    pb[1] = pack2<T>(s[2 * st][2], s[2 * st][3]);
                    pb[2] = pack2<T>(s[2 * st + 1][0], s[2 * st + 1][1]);
                    pb[3] = pack2<T>(s[2 * st + 1][2], s[2 * st + 1][3]);
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt) {
                        const u32x4_v vt = {vf[2 * dt][0], vf[2 * dt][1], vf[2 * dt + 1][0], vf[2 * dt + 1][1]};
                        o[dt] = mfma16<T>(vt, pb, o[dt]);
                    }
                };
                ARP_AL_VWAIT(v0);
                pv(0, v0);
                if (upper) {
                    ARP_AL_VWAIT(v1);
                    pv(1, v1);
                }
            }
            buf = buf == 2 ? 0 : buf + 1;
        }
        l += __shfl_xor(l, 16, 64);
        l += __shfl_xor(l, 32, 64);
        if (active && qidx < nq) {
            const float inv = 1.0f / l;
            T* orow = out + ((size_t)b * N + qidx) * D + h * 64;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) store4(orow + dt * 16 + fg * 4, o[dt][0] * inv, o[dt][1] * inv, o[dt][2] * inv, o[dt][3] * inv);
        }
    }
}
template <typename T>
__global__ __launch_bounds__(256) void attn_long_kernel(const T* __restrict__ qkv, T* __restrict__ out, int N, int D, int heads, float scale, int causal,
                                                        int nq) {
    attn_long_body<T, false>(qkv, out, N, D, heads, scale, causal, nq, nullptr, 0);
}
// The key-masked instance (M3AE's image + text pass: padded instruction tokens are taken out of every softmax).  mask: one bit per key, 1 = visible, key k in
// bit k & 31 of word k >> 5, (N + 31) / 32 words per sample, sample b's words at mask + b * mask_stride (stride 0: one mask for the whole call).  A hidden key
// scores -inf for every query of its sample.  A block of 64 keys that are all hidden is staged and meets its barriers like any other, and its compute is
// skipped (as the causal skip does: m, l and o stay as they are); the upper 32 keys are skipped when all hidden; the per-score select runs only in blocks
// that hold a hidden or pad key.  Key 0 must be visible (the launcher refuses otherwise): block 0 is then computed for every query and m is finite from
// there on.  No causal mask in this instance.  With every key visible each query block runs the unmasked instance's operations in its order: the same bits.
// Any N from 1 to 1024: pad keys alias key N - 1 and are cleared from the words.
template <typename T>
__global__ __launch_bounds__(256) void attn_long_masked_kernel(const T* __restrict__ qkv, T* __restrict__ out, int N, int D, int heads, float scale, int nq,
                                                               const uint32_t* __restrict__ mask, int mask_stride) {
    attn_long_body<T, true>(qkv, out, N, D, heads, scale, 0, nq, mask, mask_stride);
}
#undef ARP_AL_VREAD
#undef ARP_AL_VWAIT

// exact f32: 128 queries per workgroup (one per lane), keys in blocks of 128 through one LDS stage of f32 rows.  Per query this is attn_valu_kernel's loop,
// operation for operation; only where K and V rows are when they are read differs.
constexpr int ATTN_LONG_F32_KB = 128, ATTN_LONG_F32_Q = 128;
constexpr int ATTN_LONG_F32_LDS = 2 * ATTN_LONG_F32_KB * 64 * 4;
// MASKED (mask format as attn_long_masked_kernel's): a hidden key is skipped in the per-key loop -- a uniform branch -- so a query row gets the bits the
// unmasked kernel gives it on the sequence with the hidden K / V rows removed.
template <int QW, bool MASKED>  // queries (= lanes) per workgroup
__device__ __forceinline__ void attn_long_f32_body(const float* __restrict__ qkv, float* __restrict__ out, int N, int D, int heads, float scale, int causal,
                                                   int nq, const uint32_t* __restrict__ mask, int mask_stride) {
    constexpr int HD = 64, KB = ATTN_LONG_F32_KB;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* Ks = reinterpret_cast<float*>(smem);
    float* Vs = Ks + KB * HD;
    const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
    const size_t ld = 3 * (size_t)D;
    const float* base = qkv + (size_t)b * N * ld + h * HD;
    const int q0 = blockIdx.y * QW, qi = q0 + (int)threadIdx.x;
    const int qr = qi < N ? qi : N - 1;
    float q[HD], acc[HD];
#pragma unroll
    for (int d = 0; d < HD; ++d) {
        q[d] = base[qr * ld + d] * scale;
        acc[d] = 0.f;
    }
    float m = -INFINITY, l = 0.f;
    const int kend_wg = causal ? min(N, min(q0 + QW, nq)) : N;  // keys one of this workgroup's queries can see
    const int kend = causal ? qr + 1 : N;
    for (int k0 = 0; k0 < kend_wg; k0 += KB) {
        const int nb = min(KB, kend_wg - k0);
        __syncthreads();  // the previous block has been read
        for (int i = threadIdx.x; i < nb * (HD / 4); i += QW) {
            const int t = i >> 4, c4 = (i & 15) * 4;
            *reinterpret_cast<float4*>(Ks + t * HD + c4) = *reinterpret_cast<const float4*>(base + (size_t)(k0 + t) * ld + D + c4);
            *reinterpret_cast<float4*>(Vs + t * HD + c4) = *reinterpret_cast<const float4*>(base + (size_t)(k0 + t) * ld + 2 * D + c4);
        }
        __syncthreads();
        const int ke = min(nb, kend - k0);
        for (int k = 0; k < ke; ++k) {
            if constexpr (MASKED) {
                const int key = k0 + k;
                if (!((mask[(size_t)b * mask_stride + (key >> 5)] >> (key & 31)) & 1)) continue;
            }
            const float* kr = Ks + k * HD;
            float s = 0.f;
#pragma unroll
            for (int d = 0; d < HD; ++d) s = fmaf(q[d], kr[d], s);
            const float mn = fmaxf(m, s);
            const float alpha = expf(m - mn);  // exp(-inf) = 0 on key 0; m is finite afterwards
            const float p = expf(s - mn);
            const float* vr = Vs + k * HD;
            l = l * alpha + p;
#pragma unroll
            for (int d = 0; d < HD; ++d) acc[d] = fmaf(p, vr[d], acc[d] * alpha);
            m = mn;
        }
    }
    if (qi < nq) {
        const float inv = 1.0f / l;
        float* o = out + ((size_t)b * N + qi) * D + h * HD;
#pragma unroll
        for (int d = 0; d < HD; d += 4) store4(o + d, acc[d] * inv, acc[d + 1] * inv, acc[d + 2] * inv, acc[d + 3] * inv);
    }
}
template <int QW>
__global__ __launch_bounds__(QW) void attn_long_f32_kernel(const float* __restrict__ qkv, float* __restrict__ out, int N, int D, int heads,
                                                                         float scale, int causal, int nq) {
    attn_long_f32_body<QW, false>(qkv, out, N, D, heads, scale, causal, nq, nullptr, 0);
}
template <int QW>
__global__ __launch_bounds__(QW) void attn_long_f32_masked_kernel(const float* __restrict__ qkv, float* __restrict__ out, int N, int D, int heads, float scale,
                                                                  int nq, const uint32_t* __restrict__ mask, int mask_stride) {
    attn_long_f32_body<QW, true>(qkv, out, N, D, heads, scale, 0, nq, mask, mask_stride);
}

}  // namespace arp
