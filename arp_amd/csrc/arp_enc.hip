// Row N1: the frozen M3AE image encoder (forward_representation) on MI355X -- host orchestration + C ABI.
// Reference: /root/reference/arp_dt/models/m3ae/model.py:471-496 (forward_representation), :200-312 (blocks),
// :95-136 (sincos pos-emb), arp_dt/ARPDT.py:111-116,413-458 (patchify, call site under stop_gradient).
// Same kernels as the CLIP image tower (tower.h) with tanh-GELU, LayerNorm eps 1e-6, a biased patch
// embedding, fixed 2-D sincos position embedding + type embedding, no ln_pre and a final LN over all tokens.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/arp_hip.h"
#include "enc_internal.h"
#include "tower.h"

using namespace arp;

namespace {

// images f32 NHWC -> patch matrix [n*G*G, P*P*3] (T), "b (h p1) (w p2) c -> b (h w) (p1 p2 c)"
template <typename T>
__global__ __launch_bounds__(256) void patchify_kernel(const float* __restrict__ img, T* __restrict__ out, int n, int res, int P) {
    const int G = res / P, K = P * P * 3;
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= (size_t)n * G * G * K) return;
    const int k = (int)(i % K);
    const size_t row = i / K;
    const int px = (int)(row % G), py = (int)((row / G) % G);
    const size_t b = row / ((size_t)G * G);
    const int p1 = k / (P * 3), rem = k - p1 * P * 3;  // rem = p2*3 + c, contiguous in the source row
    const float* src = img + ((b * res + (size_t)py * P + p1) * res + (size_t)px * P) * 3 + rem;
    store4(out + i, src[0], src[1], src[2], src[3]);
}

// The assembled sequence of a sample (EncSeq, enc_internal.h; arp_dt/models/m3ae/model.py:471-525), f32 [nb, ntok, D], ntok = 1 + GG (+ GG | + L):
//   x[b, 0] = cls;  x[b, 1 + p] = pe[b*GG + p] + pos[p]                  (pos already holds the 2-D sincos + the image type embedding)
//   goal:  x[b, 1 + GG + p] = pe[(nb + b)*GG + p] + pos[p]               (pe: the patch embeddings of the nb frames first, then those of the nb goals)
//   L > 0: x[b, 1 + GG + j] = text_emb[tok[j]] + tpos[j]                 (tpos already holds get_1d_sincos_pos_embed(width, L)[j] + the text type embedding)
// tok: int32 ids, [L] shared by the nb frames (per_row = 0) or [nb, L]; the host has checked them against the vocabulary.  Never both goal and L > 0.
// KIND (EncSeq::Kind) is a compile-time argument, so that each kind's instance carries only its own rows' index arithmetic and branches.
template <int KIND> __global__ __launch_bounds__(256) void enc_assemble_kernel(const float* __restrict__ pe, const float* __restrict__ cls, const float* __restrict__ pos,
                                                           const float* __restrict__ text_emb, const float* __restrict__ tpos, const int32_t* __restrict__ tok,
                                                           int per_row, float* __restrict__ x, int nb, int GG, int L_, int D) {
    constexpr bool goal = KIND == EncSeq::GOAL;
    const int L = KIND == EncSeq::TEXT ? L_ : 0, ntok = 1 + (goal ? 2 : 1) * GG + L;
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= (size_t)nb * ntok * D) return;
    const int c = (int)(i % D);
    const size_t row = i / D;
    const int t = (int)(row % ntok);
    const size_t b = row / ntok;
    float v[4];
    if (t == 0) {
        load4(cls + c, v);
    } else {
        float p4[4];
        const int j = t > GG ? t - 1 - GG : t - 1;  // the row's place in its block: patches, goal patches or instruction
        if (t <= GG || goal) {
            load4(pe + (((t > GG ? (size_t)nb : 0) + b) * GG + j) * D + c, v);
            load4(pos + (size_t)j * D + c, p4);
        } else {
            const int id = tok[(per_row ? b * L : 0) + j];
            load4(text_emb + (size_t)id * D + c, v);
            load4(tpos + (size_t)j * D + c, p4);
        }
        v[0] += p4[0]; v[1] += p4[1]; v[2] += p4[2]; v[3] += p4[3];
    }
    store4(x + i, v[0], v[1], v[2], v[3]);
}
int launch_assemble(hipStream_t stream, const float* pe, const float* cls, const float* pos, const float* text_emb, const float* tpos, const EncSeq& seq, float* x,
                    int nb, int GG, int D) {
    // goal rows and text rows both follow seq.kind, as seq.tokens does: a descriptor filled in by hand cannot ask for both
    const size_t tot = (size_t)nb * seq.tokens(1 + GG) * D;
    const auto kern = seq.kind == EncSeq::GOAL ? enc_assemble_kernel<EncSeq::GOAL> : seq.kind == EncSeq::TEXT ? enc_assemble_kernel<EncSeq::TEXT> : enc_assemble_kernel<EncSeq::PLAIN>;
    hipLaunchKernelGGL(kern, dim3((unsigned)((tot / 4 + 255) / 256)), dim3(256), 0, stream, pe, cls, pos, text_emb, tpos, seq.tok_dev, seq.per_row, x, nb, GG, seq.L, D);
    ARP_HIP_OK(hipGetLastError());
    return 0;
}

// ARP_MODE_F16X3: f32 [rows, K] -> binary16 [rows, 3K] = [hi | lo | hi], hi = rn16(x), lo = rn16(x - hi): the A operand of a K-concatenated product against
// [W_hi | W_hi | W_lo] -- x.W to ~2^-22 on three 16-bit MFMAs (hi.hi is exact in the f32 accumulator; lo.lo, ~2^-24, is dropped).  Values whose lo falls below
// binary16's normal range keep an absolute error <= 3e-8 (subnormals are not flushed on this path).  8 elements per thread.
__global__ __launch_bounds__(256) void split3_kernel(const float* __restrict__ x, f16_t* __restrict__ out, size_t rows, int K) {
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 8;
    if (i >= rows * (size_t)K) return;
    const size_t r = i / K;
    const int k = (int)(i - r * K);
    float va[4], vb[4];
    load4(x + i, va);
    load4(x + i + 4, vb);
    const float v[8] = {va[0], va[1], va[2], va[3], vb[0], vb[1], vb[2], vb[3]};
    uint32_t hi[4], lo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float h0 = h2f(f2h(v[2 * j])), h1 = h2f(f2h(v[2 * j + 1]));
        hi[j] = pack_h2(h0, h1);
        lo[j] = pack_h2(v[2 * j] - h0, v[2 * j + 1] - h1);
    }
    f16_t* o = out + r * 3 * (size_t)K + k;
    *reinterpret_cast<uint4*>(o) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
    *reinterpret_cast<uint4*>(o + K) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
    *reinterpret_cast<uint4*>(o + 2 * (size_t)K) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
}

int launch_split3(hipStream_t stream, const float* src, f16_t* out, size_t rows, int K) {
    if (K % 8) return fail("f16x3: widths must be multiples of 8");
    hipLaunchKernelGGL(split3_kernel, dim3((unsigned)((rows * K / 8 + 255) / 256)), dim3(256), 0, stream, src, out, rows, K);
    ARP_HIP_OK(hipGetLastError());
    return 0;
}

// patchify_kernel<float> + split3_kernel in one pass (round 6; f16x3 and f16c modes): the f32 patch matrix is never written (100 MB per 128 frames written and
// read back).  Same values: each element is loaded once, hi = rn16(v), lo = rn16(v - hi) as split3_kernel forms them.
__global__ __launch_bounds__(256) void patchify_split3_kernel(const float* __restrict__ img, f16_t* __restrict__ out, int n, int res, int P) {
    const int G = res / P, K = P * P * 3;
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= (size_t)n * G * G * K) return;
    const int k = (int)(i % K);
    const size_t row = i / K;
    const int px = (int)(row % G), py = (int)((row / G) % G);
    const size_t b = row / ((size_t)G * G);
    const int p1 = k / (P * 3), rem = k - p1 * P * 3;
    const float* src = img + ((b * res + (size_t)py * P + p1) * res + (size_t)px * P) * 3 + rem;
    const float v[4] = {src[0], src[1], src[2], src[3]};
    uint32_t hi[2], lo[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const float h0 = h2f(f2h(v[2 * j])), h1 = h2f(f2h(v[2 * j + 1]));
        hi[j] = pack_h2(h0, h1);
        lo[j] = pack_h2(v[2 * j] - h0, v[2 * j + 1] - h1);
    }
    f16_t* o = out + row * 3 * (size_t)K + k;
    *reinterpret_cast<uint2*>(o) = make_uint2(hi[0], hi[1]);
    *reinterpret_cast<uint2*>(o + K) = make_uint2(lo[0], lo[1]);
    *reinterpret_cast<uint2*>(o + 2 * (size_t)K) = make_uint2(hi[0], hi[1]);
}

// nb images -> patch rows of type T at `out`, or (X3) rows of (hi, lo, hi) binary16 triples; four values per thread
template <typename T, bool X3> int launch_patchify(hipStream_t stream, const float* src, T* out, int nb, int res, int P) {
    const size_t tot = (size_t)nb * (res / P) * (res / P) * P * P * 3;
    const dim3 grid((unsigned)((tot / 4 + 255) / 256));
    if constexpr (X3) hipLaunchKernelGGL(patchify_split3_kernel, grid, dim3(256), 0, stream, src, out, nb, res, P);
    else hipLaunchKernelGGL((patchify_kernel<T>), grid, dim3(256), 0, stream, src, out, nb, res, P);
    ARP_HIP_OK(hipGetLastError());
    return 0;
}

struct HostTensor {
    std::vector<float> data;
    std::vector<int64_t> shape;
};

}  // namespace

struct arp_enc {
    arp_enc_cfg cfg;
    Stream stream;  // serves arp_enc_forward only; created by its first call
    std::map<std::string, HostTensor> staged;
    std::vector<DevBuf> owned;  // every device allocation holding weights
    bool finalized = false;
    TowerW tower;
    void* w_emb = nullptr;  // T [D, P*P*3]
    float *b_emb = nullptr, *cls = nullptr, *pos = nullptr, *lnf_w = nullptr, *lnf_b = nullptr;
    // Part streams (round 6, as arp_clip.hip::label_dev): a call's frames are cut into contiguous parts, part 0 on the caller's stream, part k on ws[k].stream,
    // forked and joined by events -- one part's HBM-bound LayerNorm / attention kernels and GEMM grid tails (M = 128 x 257 rows: c_fc 6.05 rounds of tiles,
    // out_proj / c_proj 1.51) run beside the other part's GEMMs.  Every part has its own workspace; weights are shared.  A frame's encoding does not depend on
    // which part it is in (every row's dot products run in the same order whatever M is): tests/test_m3ae_gpu.py::test_part_streams_are_exact.
    struct Ws {
        int frames = 0;
        DevBuf patches, pe, x, h, qkv, ao, fc;
        DevBuf a3;  // ARP_MODE_F16X3: the [hi | lo | hi] operand of the current GEMM, binary16 [rows, 3 * (mlp_ratio * width)]
                    // ARP_MODE_F16C: the [hi | x4 | dx4] operand rows (3 bytes per value): [M, D] for LayerNorm / attention outputs, then [M, H] for the hidden activation
        Stream stream;  // parts 1..: the part's own stream (part 0 runs on the caller's)
        Event done;
    };
    static constexpr int MAX_PARTS = 4;
    Ws ws[MAX_PARTS];
    int n_parts = 2;          // arp_enc_set_streams / ARP_ENC_STREAMS
    int min_part_frames = 24; // a part of fewer frames does not fill the chip's GEMM grid (24 x 257 rows = 24 row tiles x 3..12 column tiles)
    // frames of part 0 of two (ARP_ENC_SPLIT); 0 = the default cut, 15/32 of the frames (60 + 68 of the step's 128); < 0 = equal parts.  Uneven parts end at different
    // times, so that one part's GEMM grid tails and LayerNorms keep meeting the other's full rounds instead of its tails: 9.05-9.08 against 9.19-9.26 ms per 32-sample step
    // (three boxes, three repetitions each: profiles/r6_n1_streams.txt, r6_plans_time.txt, r6_n1_split_final.txt); 56 + 72 the same, 43 + 43 + 42 slower
    int first_part = 0;
    Event ev_fork;
    bool shared_chip = false; // the pass being enqueued runs beside another part's kernels (tower.h: out_proj's kernel choice)
    DevBuf img_in, out;
    // Latency path (the rollout session's per-step pass of its E new frames): a call of at most lat_rows token rows IN TOTAL, in the plain 16-bit
    // modes, runs as ONE part on tower.h's latency path -- the W-tiled skinny GEMMs (patch embedding, in_proj, c_fc), out_proj / c_proj as split-K slabs whose
    // reduction kernel adds bias + residual and applies the next LayerNorm.  Only callers that ask for it (enc_forward_on's `latency`: the rollout session, and
    // arp_enc_forward once arp_enc_set_latency turned lat_host on) take it; the training paths never do, whatever their row count.  A goal-conditioned call
    // (EncSeq::GOAL, arp_enc_forward_gc) follows the same rule on pairs x (2 P + 1) rows: one real pair is 513 rows, measured 1.224 against 1.474 ms per
    // GCBC session step with the path on / off (profiles/gc_rollout_timing.txt); two pairs are over SKINNY_MAX_M.
    // Default 514 = two frames at 257 tokens, the largest row count at which the path was measured faster inside a rollout step (ViT-B/16, f16 / bf16:
    // 257 rows 1.10 against 1.56 ms per step, 514 rows 1.39 against 1.69, 771 rows 1.80 against 1.69 -- slower; profiles/rollout_step_timing.txt).
    int lat_rows = 514;  // arp_enc_set_latency / ARP_ENC_LAT_ROWS (up to SKINNY_MAX_M); 0 = the throughput kernels at every size
    bool lat_host = false;        // arp_enc_forward asks for the latency path too (off: host calls keep the bits they always had)
    bool lat_now = false;         // the pass being enqueued runs on the latency path
    DevBuf lat_part;              // split-K slabs, f32 [<= 4][rows][width]
    // ARP_MODE_F16C: per GEMM g in {in_proj, out_proj, fc1, fc2} the correction plan (0 plain, 1 weights, 2 weights + activations) and, per layer, the
    // power-of-two exponents the e2m1 (fp4) weight segments were scaled by: dW4 = fp4(dW * 2^sw_d), W4 = fp4(W * 2^sw_w)
    bool vperm = true;  // ARP_MODE_F16C: V's columns permuted inside every head so that the attention's [hi | x4 | dx4] rows leave in whole pieces (attention.h, outc == 2); cleared by geometry
    // Default 1110 (round 6): the weight roundings of in_proj, out_proj and fc1 corrected, fc2 plain.  Encoder-inside logits over 8 seeds (max) and the 32-sample step
    // on one box, AFTER the epilogue's x4 segment was repaired (gemm256.h; rounds 5 and 6 measured fc2's correction as noise): 1221 3.7e-4 / 10.19 ms,
    // 1121 5.4e-4, 1111 6.0e-4 / 9.82, 1220 6.4e-4 / 9.83, 1211 6.9e-4 / 9.88, 1210 6.8e-4 / 9.54, 1120 6.7e-4 / 9.76, 1110 7.0e-4 / 9.48 (profiles/r6_n1_plan_sweep.txt,
    // r6_plans_time.txt): one plan is clearly better (1221, round 5's, for +0.7 ms) and the rest are one cloud at 5.4 ... 7.0e-4 -- the cheapest of it is the default,
    // ARP_F16C_PLAN=1221 buys the other.  Producers skip the segments a plan never reads (the attention's dx4, fc1's x4).
    int plan[4] = {1, 1, 1, 0};
    std::vector<int> sw_d[4], sw_w[4];
    void* w_emb3 = nullptr;  // ARP_MODE_F16C: the patch embedding's [W_hi | W_hi | W_lo] (its product runs as ARP_MODE_F16X3's K-concatenation)
    // The optional text branch (arp_enc_forward_text): text_embedding/embedding [vocab, width] and encoder_text_type_embedding, loaded when the caller staged them.
    // text_pos rows i < text_pos_L hold get_1d_sincos_pos_embed(width, L)[i] + the type embedding (row i does not depend on L), built at the first call that
    // needs them.  txt_pin / txt_dev: a host call's token ids followed by its visible-bit words, staged through pinned memory with one async copy on the call's stream.
    float *text_emb = nullptr, *text_type = nullptr;
    int vocab = 0;
    std::vector<float> text_type_host;
    DevBuf text_pos;
    int text_pos_L = 0;
    PinBuf txt_pin;
    DevBuf txt_dev;
    Profiler prof;
    int gemm_force = 0;
    int tokens() const { return (cfg.img_res / cfg.patch) * (cfg.img_res / cfg.patch) + 1; }
    size_t esz() const { return (cfg.mode == ARP_MODE_F32 || cfg.mode == ARP_MODE_F16X3) ? 4 : 2; }  // element size of the ACTIVATION buffers
    size_t wsz() const { return cfg.mode == ARP_MODE_F32 ? 4 : 2; }
};
static_assert(!std::is_copy_constructible_v<arp_enc>);

namespace {

int up_f32(arp_enc* c, const float* v, size_t n, float** out) {
    return upload_owned(c->owned, v, n * 4, std::max<size_t>(n * 4, 16), reinterpret_cast<void**>(out));
}
// [out, 3 in] = [W_hi | W_hi | W_lo] from the transposed kernel t [out, in] (ARP_MODE_F16X3; the patch embedding of ARP_MODE_F16C)
int up_kernel_x3(arp_enc* c, const std::vector<float>& t, int in, int out_, void** out) {
    const size_t n = (size_t)in * out_;
    std::vector<f16_t> hb(3 * n);
    for (int o = 0; o < out_; ++o)
        for (int i = 0; i < in; ++i) {
            const float w = t[(size_t)o * in + i];
            const f16_t h = host_f2h(w);
            const float hf = (float)__builtin_bit_cast(_Float16, h.b);
            f16_t* row = hb.data() + (size_t)o * 3 * in;
            row[i] = h;
            row[in + i] = h;
            row[2 * in + i] = host_f2h(w - hf);
        }
    return upload_owned(c->owned, hb.data(), 3 * n * 2, 3 * n * 2, out);
}
// Flax kernel [in, out] -> device [out, in] in the operand type
int up_kernel(arp_enc* c, const float* src, int in, int out_, void** out) {
    const size_t n = (size_t)in * out_;
    std::vector<float> t(n);
    for (int i = 0; i < in; ++i)
        for (int o = 0; o < out_; ++o) t[(size_t)o * in + i] = src[(size_t)i * out_ + o];
    if (c->cfg.mode == ARP_MODE_F16X3) return up_kernel_x3(c, t, in, out_, out);
    const size_t alloc = std::max<size_t>(n * c->wsz(), 16);
    if (c->cfg.mode == ARP_MODE_BF16) {
        std::vector<bf16_t> hb(n);
        for (size_t i = 0; i < n; ++i) hb[i] = host_f2bf(t[i]);
        return upload_owned(c->owned, hb.data(), n * 2, alloc, out);
    }
    if (c->cfg.mode == ARP_MODE_F16 || c->cfg.mode == ARP_MODE_F16C) {
        std::vector<f16_t> hb(n);
        for (size_t i = 0; i < n; ++i) hb[i] = host_f2h(t[i]);
        return upload_owned(c->owned, hb.data(), n * 2, alloc, out);
    }
    return upload_owned(c->owned, t.data(), n * 4, alloc, out);
}
// ARP_MODE_F16C: Flax kernel [in, out] -> device rows [W_hi: binary16 x in | dW4: e2m1 x in (| W4: e2m1 x in)] (plan 1 / 2; plan 0: binary16 only)
// src(i, o) = the weight of input i, output o.  Rows [W_hi: binary16 x in | dW4: e2m1 x in (| W4: e2m1 x in)] for plan 1 (2); two e2m1 values per byte, value 2j in the
// low nibble (the order common.h::pack_fp4x8 packs activations in).  dW4 = fp4((w - W_hi) 2^*sd), W4 = fp4(w 2^*sw): per-tensor powers of two that put the largest
// magnitude into (6, 12] (e2m1 saturates at 6: the few values of the top half-binade lose part of their correction, every other value gains a bit).
template <typename F> void pack_weight_c(F src, int in, int out_, int plan, std::vector<uint8_t>& hb, int* sd, int* sw) {
    const size_t row_bytes = (size_t)in * 2 + (size_t)plan * (in / 2);
    hb.assign(row_bytes * out_, 0);
    float max_d = 0.f, max_w = 0.f;
    for (int i = 0; i < in; ++i)
        for (int o = 0; o < out_; ++o) {
            const float w = src(i, o);
            const float hf = (float)__builtin_bit_cast(_Float16, host_f2h(w).b);
            max_d = std::max(max_d, std::fabs(w - hf));
            max_w = std::max(max_w, std::fabs(w));
        }
    auto pick = [](float mx) { return mx > 0.f ? (int)std::floor(std::log2(6.0 / (double)mx)) + 1 : 0; };  // the top binade saturates at 6: measured better than wasting a code on it
    *sd = std::min(pick(max_d), 100);
    *sw = std::min(pick(max_w), 100);
    const float fd = std::ldexp(1.0f, *sd), fw = std::ldexp(1.0f, *sw);
    for (int o = 0; o < out_; ++o) {
        uint8_t* row = hb.data() + (size_t)o * row_bytes;
        for (int i = 0; i < in; ++i) {
            const float w = src(i, o);
            const f16_t h = host_f2h(w);
            const float hf = (float)__builtin_bit_cast(_Float16, h.b);
            memcpy(row + 2 * (size_t)i, &h.b, 2);
            const int sh = (i & 1) * 4;
            if (plan >= 1) row[2 * (size_t)in + i / 2] |= (uint8_t)(host_f2fp4((w - hf) * fd) << sh);
            if (plan >= 2) row[2 * (size_t)in + in / 2 + i / 2] |= (uint8_t)(host_f2fp4(w * fw) << sh);
        }
    }
}
int up_kernel_c(arp_enc* c, const float* src, int in, int out_, int plan, void** out, int* sd, int* sw) {
    std::vector<uint8_t> hb;
    pack_weight_c([&](int i, int o) { return src[(size_t)i * out_ + o]; }, in, out_, plan, hb, sd, sw);
    return upload_owned(c->owned, hb.data(), hb.size(), hb.size() + 512, out);  // + the 256 bytes gemm256 MIXC reads past the last row (GemmArgs::mix_nk16)
}
int staged(arp_enc* c, const std::string& name, std::vector<int64_t> shape, const HostTensor** out) {
    auto it = c->staged.find(name);
    if (it == c->staged.end()) return fail("missing weight: " + name);
    if (it->second.shape != shape) return fail("weight " + name + " has an unexpected shape");
    *out = &it->second;
    return 0;
}

int ensure_ws(arp_enc* c, arp_enc::Ws& w, int frames) {
    if (frames <= w.frames) return 0;
    const arp_enc_cfg& k = c->cfg;
    const size_t e = c->esz(), G = k.img_res / k.patch, D = k.width, N = c->tokens(), B = frames, M = B * N;
    ARP_TRY(w.patches.ensure(B * G * G * k.patch * k.patch * 3 * e));
    ARP_TRY(w.pe.ensure(B * G * G * D * 4));
    ARP_TRY(w.x.ensure(M * D * 4)); ARP_TRY(w.h.ensure(M * D * e)); ARP_TRY(w.qkv.ensure(M * 3 * D * e));
    ARP_TRY(w.ao.ensure(M * D * e)); ARP_TRY(w.fc.ensure(M * k.mlp_ratio * D * e));
    if (k.mode == ARP_MODE_F16X3)  // [M, 3 D] (a GEMM's A operand) followed by [M, 3 H] (c_fc's own epilogue writes c_proj's operand there)
        ARP_TRY(w.a3.ensure(std::max(M * 3 * (D + k.mlp_ratio * D), B * G * G * 3 * k.patch * k.patch * 3) * 2));
    if (k.mode == ARP_MODE_F16C) {  // [M, D] and [M, H] operand rows of 3 bytes per value; the patch embedding's (hi, lo, hi) triples share the space
        // (+ one 256-row tile of slack: the MIXC instances read ceil(M / 256) * 256 operand rows unclamped)
        ARP_TRY(w.a3.ensure(std::max((M + 256) * 3 * (D + k.mlp_ratio * D) + 4096, B * G * G * 3 * k.patch * k.patch * 3 * 2)));
        ARP_TRY(w.patches.ensure(B * G * G * k.patch * k.patch * 3 * 4));  // f32 patches (split into triples on the device)
    }
    w.frames = frames;
    return 0;
}

AttnKeyMask key_mask_of(const EncSeq& seq, int P1) {  // (no instruction: no mask, dev == null)
    AttnKeyMask km;
    km.dev = seq.words_dev; km.stride = seq.per_row ? seq.words(P1) : 0; km.host = seq.words_host;
    return km;
}

// ARP_MODE_F16C runs the plain sequence only
int f16c_plain_only(const arp_enc* c, const EncSeq& seq) {
    if (c->cfg.mode != ARP_MODE_F16C) return 0;
    if (seq.kind == EncSeq::GOAL) return fail("f16c: no goal-conditioned pass (its [hi | x4 | dx4] attention rows exist on the LDS-resident kernel only, <= 288 tokens)");
    if (seq.kind == EncSeq::TEXT) return fail("f16c: no image + text pass (its [hi | x4 | dx4] attention rows exist on the LDS-resident kernel only, <= 288 tokens)");
    return 0;
}

// The front end of every forward_chunk*: the nb frames (a GOAL sequence: then the nb goal frames) -> patch rows at `patches`, typed, or as (hi, lo, hi) binary16
// triples in one pass (X3: the f16x3 and f16c operand) -> the patch-embedding product against w_emb into w.pe -> the assembled sequences in w.x.
template <typename T, bool X3> int front_end(arp_enc* c, arp_enc::Ws& w, TowerCtx& t, const float* img_dev, int nb, const EncSeq& seq, T* patches, const void* w_emb) {
    const arp_enc_cfg& k = c->cfg;
    const int G = k.img_res / k.patch, KP = k.patch * k.patch * 3, sets = seq.kind == EncSeq::GOAL ? 2 : 1, seg = X3 ? 3 : 1;
    const size_t tot = (size_t)nb * G * G * KP;
    {
        ProfScope ps(c->prof, t.stream, "m3ae.patchify");
        for (int s = 0; s < sets; ++s) {
            ARP_TRY((launch_patchify<T, X3>(t.stream, s ? seq.goals_dev : img_dev, patches + s * seg * tot, nb, k.img_res, k.patch)));
        }
    }
    ARP_TRY((tower_gemm<T, float, ACT_NONE, false, 8 + SITE_PATCH>(t, "m3ae.image_embedding", patches, w_emb, c->b_emb, nullptr, w.pe.p, sets * nb * G * G, k.width,
                                                                   seg * KP)));
    ProfScope ps(c->prof, t.stream, "m3ae.assemble");
    return launch_assemble(t.stream, w.pe.as<float>(), c->cls, c->pos, c->text_emb, c->text_pos.as<float>(), seq, w.x.as<float>(), nb, G * G, k.width);
}

template <typename T> int forward_chunk(arp_enc* c, arp_enc::Ws& w, hipStream_t stream, const float* img_dev, int nb, float* out_dev, const EncSeq& seq) {
    const arp_enc_cfg& k = c->cfg;
    const int N = seq.tokens(c->tokens()), D = k.width;
    TowerCtx t;
    t.stream = stream; t.prof = &c->prof; t.attn_impl = k.attn_impl; t.gemm_force = c->gemm_force; t.shared_chip = c->shared_chip;
    if (sizeof(T) == 2 && c->lat_now) {  // (the patch embedding then goes through tower_gemm's skinny route where skinny_supported holds)
        t.skinny = true; t.part = c->lat_part.as<float>(); t.part_floats = c->lat_part.bytes / 4;
    }
    ARP_TRY((front_end<T, false>(c, w, t, img_dev, nb, seq, w.patches.as<T>(), c->w_emb)));
    const AttnKeyMask km = key_mask_of(seq, c->tokens());
    ARP_TRY((run_blocks<T, ACT_GELU_TANH, 8>(t, c->tower, "m3ae", w.x.as<float>(), w.h.as<T>(), w.qkv.as<T>(), w.ao.as<T>(), w.fc.as<T>(), nb, N, 0,
                                             1e-6f, nullptr, km.dev ? &km : nullptr)));
    ARP_TRY(tower_layernorm<float>(t, "m3ae.ln_final", w.x.as<float>(), (size_t)D, out_dev, D, c->lnf_w, c->lnf_b, nb * N, D, 1e-6f));
    return 0;
}

// ARP_MODE_F16X3: the same network with every GEMM as a K-concatenated (hi, lo) product on the f16 kernels and everything between the GEMMs in f32
// (LayerNorm outputs, the exact-f32 attention kernel, the tanh-GELU'd hidden activation): 12 x (ln -> split -> in_proj -> attention -> split -> out_proj -> ln ->
// split -> fc1 -> split -> fc2).  Three MFMAs per product plus the split passes: ~4x the plain f16 step, ~2x faster than the f32-MFMA mode, f32-level error.
int forward_chunk_x3(arp_enc* c, arp_enc::Ws& w, hipStream_t stream, const float* img_dev, int nb, float* out_dev, const EncSeq& seq) {
    const arp_enc_cfg& k = c->cfg;
    const int N = seq.tokens(c->tokens()), D = k.width, H = k.mlp_ratio * D, M = nb * N;
    TowerCtx t;
    t.stream = stream; t.prof = &c->prof; t.attn_impl = k.attn_impl; t.gemm_force = c->gemm_force; t.shared_chip = c->shared_chip;
    f16_t* a3 = w.a3.as<f16_t>();
    auto split = [&](const char* site, const float* src, size_t rows, int K) -> int {
        ProfScope ps(c->prof, stream, site);
        return launch_split3(stream, src, a3, rows, K);
    };
    ARP_TRY((front_end<f16_t, true>(c, w, t, img_dev, nb, seq, a3, c->w_emb)));
    const AttnKeyMask km = key_mask_of(seq, c->tokens());
    const AttnKeyMask* mask = km.dev ? &km : nullptr;
    float *x = w.x.as<float>(), *qkv = w.qkv.as<float>(), *ao = w.ao.as<float>();
    for (int i = 0; i < k.layers; ++i) {
        const LayerW& L = c->tower.L[i];
        // LayerNorm and the attention write the (hi, lo, hi) triples of their f32 results themselves (f16x3_t / out3): no f32 copy, no split pass
        const bool direct = k.attn_impl == 0 && D / k.heads == 64 && N <= 288 && !mask;  // (the VALU attention has no such output, nor has a masked call -- the exact-f32 masked kernel: both keep the split pass)
        ARP_TRY(tower_layernorm<f16x3_t>(t, "m3ae.ln_1", x, D, reinterpret_cast<f16x3_t*>(a3), 3 * D, L.ln1_w, L.ln1_b, M, D, 1e-6f));
        ARP_TRY((tower_gemm<f16_t, float, ACT_NONE, false, 8 + SITE_QKV>(t, "m3ae.qkv", a3, L.w_in, L.b_in, nullptr, qkv, M, 3 * D, 3 * D)));
        {
            ProfScope ps(c->prof, stream, "m3ae.attn");
            // the (hi, lo) binary16 attention (attention.h::attn_x3_kernel) where it exists
            ARP_TRY(launch_attention<float>(stream, direct ? 3 : k.attn_impl, qkv, ao, nb, N, D, k.heads, 0, 0, 0.f, direct ? a3 : nullptr, 0, mask));
        }
        if (!direct) ARP_TRY(split("m3ae.split", ao, M, D));
        ARP_TRY((tower_gemm<f16_t, float, ACT_NONE, true, 8 + SITE_OUT>(t, "m3ae.out_proj", a3, L.w_out, L.b_out, x, x, M, D, 3 * D)));
        ARP_TRY(tower_layernorm<f16x3_t>(t, "m3ae.ln_2", x, D, reinterpret_cast<f16x3_t*>(a3), 3 * D, L.ln2_w, L.ln2_b, M, D, 1e-6f));
        // c_fc's epilogue writes the (hi, lo, hi) triples of the tanh-GELU'd hidden activation itself: no f32 copy of it, no split pass (2.4 ms of a 30.9 ms step)
        f16_t* a3b = a3 + (size_t)M * 3 * D;
        GemmFold pair;
        pair.xb_out = a3b; pair.ldxb = 3 * H; pair.split3 = 1;
        ARP_TRY((tower_gemm<f16_t, float, ACT_GELU_TANH, false, 8 + SITE_FC1>(t, "m3ae.c_fc", a3, L.w_fc, L.b_fc, nullptr, nullptr, M, H, 3 * D, &pair)));
        ARP_TRY((tower_gemm<f16_t, float, ACT_NONE, true, 8 + SITE_FC2>(t, "m3ae.c_proj", a3b, L.w_proj, L.b_proj, x, x, M, D, 3 * H)));
    }
    ARP_TRY(tower_layernorm<float>(t, "m3ae.ln_final", x, (size_t)D, out_dev, D, c->lnf_w, c->lnf_b, M, D, 1e-6f));
    return 0;
}

// ARP_MODE_F16C: the binary16 encoder with its GEMMs' operand roundings corrected on the scaled fp4 MFMA (include/arp_hip.h).  Per block:
//   ln_1 -> [hi | x4 (| dx4)] -> in_proj (MIXC) -> qkv binary16 -> MFMA attention -> [hi | x4 | dx4] -> out_proj (MIXC) into the f32 residual stream ->
//   ln_2 -> [hi | x4 (| dx4)] -> fc1 (MIXC, tanh-GELU; the epilogue stores hi AND the e2m1 segment of fc2's operand) -> fc2 (MIXC) into the residual stream.
template <int ACT, bool RESID, typename OutT, int SITE>
int gemm_c(arp_enc* c, TowerCtx& t, const char* site, const void* A, const void* W, int plan, int sd, int sw, const float* bias, const float* resid, void* out,
           int M, int N, int Kc, int ldo, void* x4_out = nullptr, int ld4 = 0, void* dx4_out = nullptr) {
    // A rows: binary16 x Kc, then e2m1 x Kc (x4), then e2m1 x Kc (dx4): 3 Kc bytes; W rows: binary16 x Kc followed by `plan` e2m1 segments
    if (Kc % 256) return fail("f16c: widths must be multiples of 256");
    GemmArgs g;
    g.A = A; g.W = W; g.bias = bias; g.resid = resid; g.out = out;
    g.M = M; g.N = N;
    g.lda = Kc + Kc / 2; g.ldw = Kc + plan * Kc / 4; g.ldr = N; g.ldo = ldo;
    g.mix_nk16 = Kc / 64;
    g.mix_nkc_a = plan >= 1 ? Kc / 256 : 0;
    g.K = Kc + plan * Kc / 4;
    g.mix_sa = F16C_X_SHIFT + sd;
    g.mix_sb = F16C_DX_SHIFT + sw;
    if (x4_out) { g.xb_out = x4_out; g.ldxb = ld4; g.x8_shift = F16C_X_SHIFT; g.dx4_out = dx4_out; }
    ProfScope ps(*t.prof, t.stream, site);
    // plan 0 (fc2's in the default plan 1110): the plain binary16 instance, which has no fp4 side output (arp_enc_create refuses a plain fc1 in front of a corrected fc2)
    if (plan == 0) return launch_gemm256_nt<f16_t, OutT, ACT, RESID, SITE>(g, t.stream);
    return launch_gemm256_nt<f16_t, OutT, ACT, RESID, SITE, false, 1, true>(g, t.stream);
}

int forward_chunk_c(arp_enc* c, arp_enc::Ws& w, hipStream_t stream, const float* img_dev, int nb, float* out_dev, const EncSeq& seq) {
    const arp_enc_cfg& k = c->cfg;
    const int N = c->tokens(), D = k.width, H = k.mlp_ratio * D, M = nb * N;  // (the plain sequence only: forward_part)
    if (D / k.heads != 64 || N > 288 || k.attn_impl != 0) return fail("f16c: needs the MFMA attention kernel (head_dim 64, <= 288 tokens)");
    TowerCtx t;
    t.stream = stream; t.prof = &c->prof; t.attn_impl = 0; t.gemm_force = c->gemm_force; t.shared_chip = c->shared_chip;
    char* a4 = static_cast<char*>(w.a3.p);                 // [M, D] operand rows, 3 D bytes each: [hi | x4 | dx4]
    char* a4h = a4 + (((size_t)M * 3 * D + 255) & ~(size_t)255);  // [M, H] operand rows, 3 H bytes each (fc1's epilogue -> fc2)
    // patch embedding on (hi, lo) binary16 pairs (its input rounding alone is a third of the plain f16 encoder's logit error; the product is 0.6 % of the FLOPs)
    ARP_TRY((front_end<f16_t, true>(c, w, t, img_dev, nb, seq, reinterpret_cast<f16_t*>(a4), c->w_emb3)));
    float* x = w.x.as<float>();
    f16_t* qkv = w.qkv.as<f16_t>();
    auto ln = [&](const char* site, const float* w, const float* b, int plan) -> int {
        if (plan >= 2) return tower_layernorm<f16c2_t>(t, site, x, D, reinterpret_cast<f16c2_t*>(a4), 3 * D / 2, w, b, M, D, 1e-6f);
        return tower_layernorm<f16c_t>(t, site, x, D, reinterpret_cast<f16c_t*>(a4), 3 * D / 2, w, b, M, D, 1e-6f);
    };
    for (int i = 0; i < k.layers; ++i) {
        const LayerW& L = c->tower.L[i];
        ARP_TRY(ln("m3ae.ln_1", L.ln1_w, L.ln1_b, c->plan[0]));
        ARP_TRY((gemm_c<ACT_NONE, false, f16_t, 8 + SITE_QKV>(c, t, "m3ae.qkv", a4, L.w_in, c->plan[0], c->sw_d[0][i], c->sw_w[0][i], L.b_in, nullptr, qkv, M, 3 * D, D, 3 * D)));
        {
            ProfScope ps(c->prof, stream, "m3ae.attn");
            ARP_TRY(launch_attention<f16_t>(stream, 0, qkv, reinterpret_cast<f16_t*>(a4), nb, N, D, k.heads, 0, 0, 0.f, nullptr, (c->vperm ? 2 : 1) | (c->plan[1] >= 2 ? 0 : 4)));
        }
        ARP_TRY((gemm_c<ACT_NONE, true, float, 8 + SITE_OUT>(c, t, "m3ae.out_proj", a4, L.w_out, c->plan[1], c->sw_d[1][i], c->sw_w[1][i], L.b_out, x, x, M, D, D, D)));
        ARP_TRY(ln("m3ae.ln_2", L.ln2_w, L.ln2_b, c->plan[2]));
        // fc1's epilogue stores the binary16 hidden activation at the head of fc2's operand rows and its e2m1 copy behind it (row stride 3 H bytes)
        ARP_TRY((gemm_c<ACT_GELU_TANH, false, f16_t, 8 + SITE_FC1>(c, t, "m3ae.c_fc", a4, L.w_fc, c->plan[2], c->sw_d[2][i], c->sw_w[2][i], L.b_fc, nullptr, a4h, M, H, D, 3 * H / 2,
                                                                  c->plan[3] >= 1 ? a4h + 2 * (size_t)H : nullptr, 3 * H, c->plan[3] >= 2 ? a4h + 2 * (size_t)H + H / 2 : nullptr)));
        ARP_TRY((gemm_c<ACT_NONE, true, float, 8 + SITE_FC2>(c, t, "m3ae.c_proj", a4h, L.w_proj, c->plan[3], c->sw_d[3][i], c->sw_w[3][i], L.b_proj, x, x, M, D, H, D)));
    }
    ARP_TRY(tower_layernorm<float>(t, "m3ae.ln_final", x, (size_t)D, out_dev, D, c->lnf_w, c->lnf_b, M, D, 1e-6f));
    return 0;
}

}  // namespace

namespace arp {

static int forward_part(arp_enc* c, arp_enc::Ws& w, hipStream_t stream, const float* img, int nb, float* out, const EncSeq& seq) {
    ARP_TRY(f16c_plain_only(c, seq));  // (forward_chunk_c; before any workspace is sized)
    ARP_TRY(ensure_ws(c, w, seq.ws_frames(nb, c->tokens())));
    if (c->cfg.mode == ARP_MODE_F16X3) return forward_chunk_x3(c, w, stream, img, nb, out, seq);
    if (c->cfg.mode == ARP_MODE_F16C) return forward_chunk_c(c, w, stream, img, nb, out, seq);
    if (c->cfg.mode == ARP_MODE_BF16) return forward_chunk<bf16_t>(c, w, stream, img, nb, out, seq);
    if (c->cfg.mode == ARP_MODE_F16) return forward_chunk<f16_t>(c, w, stream, img, nb, out, seq);
    return forward_chunk<float>(c, w, stream, img, nb, out, seq);
}

// the encoder's GEMM instances (forward_chunk / forward_chunk_x3 / forward_chunk_c above), by name
template <typename T> static int enc_gemm_site_t(const arp_gemm_site& d, const std::string& s) {
    if (s == "m3ae.qkv") return tower_gemm_site<T, T, ACT_NONE, false, 8 + SITE_QKV>(d);
    if (s == "m3ae.c_fc") return tower_gemm_site<T, T, ACT_GELU_TANH, false, 8 + SITE_FC1>(d);
    if (s == "m3ae.out_proj") return tower_gemm_site<T, float, ACT_NONE, true, 8 + SITE_OUT>(d);
    if (s == "m3ae.c_proj") return tower_gemm_site<T, float, ACT_NONE, true, 8 + SITE_FC2>(d);
    return fail("gemm_site: unknown instance " + s);
}
int enc_op_gemm_site(const arp_gemm_site& d) {
    const std::string s(d.name);
    if (s == "m3ae.x3.c_fc") return tower_gemm_site<f16_t, float, ACT_GELU_TANH, false, 8 + SITE_FC1>(d);
    if (s == "m3ae.f16c.c_fc" || s == "m3ae.f16c.c_proj") {
        // K is Kc, the binary16 width of a row; A / W are operand rows as the encoder lays them out (gemm_c); the plain instance (plan 0) has no fp4 side output
        if (d.plan < 1 || d.plan > 2) return fail("gemm_site: f16c plans 1 and 2 only");
        Profiler prof;
        TowerCtx t;
        t.prof = &prof;
        if (s == "m3ae.f16c.c_fc")
            return gemm_c<ACT_GELU_TANH, false, f16_t, 8 + SITE_FC1>(nullptr, t, "op.gemm_site", d.A, d.W, d.plan, d.sd, d.sw, d.bias, nullptr, d.out, d.M, d.N,
                                                                      d.K, d.ldo ? d.ldo : d.N, d.x4_out, d.ld4, d.dx4_out);
        if (d.x4_out || d.dx4_out) return fail("gemm_site: m3ae.f16c.c_proj has no fp4 side output");
        return gemm_c<ACT_NONE, true, float, 8 + SITE_FC2>(nullptr, t, "op.gemm_site", d.A, d.W, d.plan, d.sd, d.sw, d.bias, d.resid, d.out, d.M, d.N, d.K,
                                                          d.ldo ? d.ldo : d.N);
    }
    if (d.mode == ARP_MODE_F16) return enc_gemm_site_t<f16_t>(d, s);
    if (d.mode == ARP_MODE_BF16) return enc_gemm_site_t<bf16_t>(d, s);
    return fail("gemm_site: 16-bit modes only");
}

// What a text call needs before anything is enqueued: both text weights, a supported mode and length, and the position rows of L tokens on the device
// (built and uploaded, synchronously, by the first call that needs rows this far; never again afterwards).
static int text_prepare(arp_enc* c, int L) {
    if (!c || !c->finalized) return fail("encoder weights not finalized");
    ARP_TRY(f16c_plain_only(c, EncSeq::text(L)));
    if (!c->text_emb || !c->text_type)
        return fail("forward_text: the text weights were not loaded (text_embedding/embedding [vocab, width] and encoder_text_type_embedding [1, 1, width])");
    if (L < 1 || c->tokens() + L > ATTN_LONG_MAX) return fail("forward_text: 1 + P + L must be at most 1024 token rows and L at least 1");
    if (c->cfg.width / c->cfg.heads != 64) return fail("forward_text: the key-masked attention kernels need head_dim 64");
    if (L <= c->text_pos_L) return 0;
    const int D = c->cfg.width, half = D / 2;
    std::vector<float> pos((size_t)L * D);
    for (int i = 0; i < L; ++i)  // get_1d_sincos_pos_embed (m3ae/model.py:95-115) + the text type embedding
        for (int d = 0; d < half; ++d) {
            const double omega = 1.0 / std::pow(10000.0, (double)d / (double)half);
            pos[(size_t)i * D + d] = (float)std::sin(i * omega) + c->text_type_host[d];
            pos[(size_t)i * D + half + d] = (float)std::cos(i * omega) + c->text_type_host[half + d];
        }
    ARP_TRY(c->text_pos.ensure(pos.size() * 4));
    ARP_HIP_OK(hipMemcpy(c->text_pos.p, pos.data(), pos.size() * 4, hipMemcpyHostToDevice));
    c->text_pos_L = L;
    return 0;
}

// (enc_internal.h)  max_frames and the part sizes count samples of the sequence: frames, pairs, or frames with their instruction.
int enc_forward_on(arp_enc* c, hipStream_t stream, const float* images_dev, int n, float* out_dev, const EncSeq& seq, bool latency) {
    if (seq.kind == EncSeq::GOAL) {
        if (!seq.goals_dev) return fail("forward_gc: null goal frames");
        if (c) ARP_TRY(f16c_plain_only(c, seq));
    }
    if (seq.kind == EncSeq::TEXT) {
        ARP_TRY(text_prepare(c, seq.L));
        if (!seq.tok_dev || !seq.words_dev || !seq.words_host) return fail("forward_text: null instruction");
    }
    if (!c || !c->finalized) return fail("encoder weights not finalized");
    if (n <= 0) return 0;
    const int mb = c->cfg.max_frames, P1 = c->tokens(), ntok = seq.tokens(P1);
    const size_t fi = (size_t)c->cfg.img_res * c->cfg.img_res * 3, fo = (size_t)ntok * c->cfg.width;
    // the latency path: decided on the call's TOTAL rows (never per part or per chunk: a sample's bits must not depend on how a call is cut), one part
    // (one real (frame, goal) pair is 513 rows, two pairs are over SKINNY_MAX_M)
    const long rows = (long)n * ntok;
    if (latency && (c->cfg.mode == ARP_MODE_F16 || c->cfg.mode == ARP_MODE_BF16) && n <= mb && rows <= c->lat_rows) {
        ARP_TRY(c->lat_part.ensure((size_t)4 * rows * c->cfg.width * 4));
        c->lat_now = true;
        const int rc = forward_part(c, c->ws[0], stream, images_dev, n, out_dev, seq);
        c->lat_now = false;
        return rc;
    }
    for (int off = 0; off < n; off += mb) {
        const int nb = std::min(mb, n - off);
        const float* img = images_dev + off * fi;
        float* out = out_dev + off * fo;
        const EncSeq so = seq.at(off, fi, P1);
        int parts = std::min(c->n_parts, (int)arp_enc::MAX_PARTS);
        while (parts > 1 && nb / parts < c->min_part_frames) --parts;
        if (parts < 2) {
            ARP_TRY(forward_part(c, c->ws[0], stream, img, nb, out, so));
            continue;
        }
        // contiguous parts: part 0 on the caller's stream, part k on its own
        int cut[arp_enc::MAX_PARTS + 1];
        cut[0] = 0;
        for (int i = 1; i <= parts; ++i) cut[i] = (int)((long long)nb * i / parts);
        if (parts == 2 && c->first_part > 0 && c->first_part < nb) cut[1] = c->first_part;
        else if (parts == 2 && c->first_part == 0 && nb >= 32) cut[1] = (int)(((long long)nb * 15 + 16) / 32);
        if (!c->ev_fork) ARP_TRY(c->ev_fork.create());
        for (int i = 1; i < parts; ++i) {
            if (!c->ws[i].stream) ARP_TRY(c->ws[i].stream.create());
            if (!c->ws[i].done) ARP_TRY(c->ws[i].done.create());
        }
        ARP_HIP_OK(hipEventRecord(c->ev_fork, stream));
        c->shared_chip = true;
        int rc = 0;
        for (int i = 0; i < parts && !rc; ++i) {
            hipStream_t st = i == 0 ? stream : c->ws[i].stream;
            if (i > 0 && hipStreamWaitEvent(st, c->ev_fork, 0) != hipSuccess) rc = fail("hipStreamWaitEvent(fork) failed");
            if (!rc) rc = forward_part(c, c->ws[i], st, img + (size_t)cut[i] * fi, cut[i + 1] - cut[i], out + (size_t)cut[i] * fo, so.at(cut[i], fi, P1));
        }
        c->shared_chip = false;
        // join even after a failure: a part stream that entered a capture must leave it before the capture ends
        for (int i = 1; i < parts; ++i) {
            if (hipEventRecord(c->ws[i].done, c->ws[i].stream) != hipSuccess || hipStreamWaitEvent(stream, c->ws[i].done, 0) != hipSuccess)
                if (!rc) rc = fail("part stream join failed");
        }
        if (rc) return rc;
    }
    return 0;
}
// Host side of an instruction: ids checked against the vocabulary, the visible-bit words built from the padding mask (mask > 0 = padded, the reference's
// convention; class and patch keys always visible).  S instructions of L tokens -> words [S, (1 + P + L + 31) / 32].
static int text_words(arp_enc* c, const int32_t* tokens, const float* mask, int S, int L, uint32_t* words) {
    if (!c || !tokens || !mask || !words) return fail("forward_text: null instruction");
    const int P1 = c->tokens(), per = (P1 + L + 31) / 32;
    for (int s = 0; s < S; ++s) {
        uint32_t* w = words + (size_t)s * per;
        std::fill(w, w + per, 0u);
        for (int k = 0; k < P1 + L; ++k) {
            if (k >= P1) {
                const int id = tokens[(size_t)s * L + k - P1];
                if (id < 0 || id >= c->vocab) return fail("forward_text: token id " + std::to_string(id) + " is outside the vocabulary [0, " + std::to_string(c->vocab) + ")");
                if (mask[(size_t)s * L + k - P1] > 0.f) continue;
            }
            w[k >> 5] |= 1u << (k & 31);
        }
    }
    return 0;
}
int EncText::set(arp_enc* e, const int32_t* tokens, const float* mask, int L_) {
    ARP_TRY(text_prepare(e, L_));
    const int per = EncSeq::text(L_).words(e->tokens());
    std::vector<uint32_t> w(per);
    ARP_TRY(text_words(e, tokens, mask, 1, L_, w.data()));
    std::vector<int32_t> blob(L_ + per);
    memcpy(blob.data(), tokens, (size_t)L_ * 4);
    memcpy(blob.data() + L_, w.data(), (size_t)per * 4);
    ARP_TRY(dev.ensure(blob.size() * 4));
    ARP_HIP_OK(hipMemcpy(dev.p, blob.data(), blob.size() * 4, hipMemcpyHostToDevice));
    words = std::move(w);
    L = L_;
    return 0;
}
int enc_seq_tokens(arp_enc* c, const EncSeq& seq, int* tokens) {
    if (!c) return fail("null encoder");
    *tokens = seq.tokens(c->tokens());
    return 0;
}
int enc_geometry(arp_enc* c, int* tokens, int* width, int* img_res, int* device) {
    if (!c) return fail("null encoder");
    *tokens = c->tokens(); *width = c->cfg.width; *img_res = c->cfg.img_res; *device = c->cfg.device;
    return 0;
}

}  // namespace arp

extern "C" {

int arp_enc_create(const arp_enc_cfg* cfg, arp_enc** out) {
    if (!cfg || !out) return fail("null argument");
    const arp_enc_cfg& k = *cfg;
    if (k.mode != ARP_MODE_F32 && k.mode != ARP_MODE_BF16 && k.mode != ARP_MODE_F16 && k.mode != ARP_MODE_F16X3 && k.mode != ARP_MODE_F16C) return fail("bad mode");
    if (k.patch <= 0 || k.img_res % k.patch || k.width % k.heads || k.width % 4) return fail("bad geometry");
    const int kq = k.mode == ARP_MODE_F32 ? 32 : 64;
    if (k.width % kq || (k.patch * k.patch * 3) % kq) return fail("width and 3*patch^2 must be multiples of " + std::to_string(kq));
    int ndev = 0;
    ARP_HIP_OK(hipGetDeviceCount(&ndev));
    if (k.device < 0 || k.device >= ndev) return fail("no such HIP device");
    ARP_HIP_OK(hipSetDevice(k.device));
    ARP_TRY(prime_runtime(k.device));  // (runtime.h: one null-stream copy before the process's first stream exists)
    arp_enc* c = new arp_enc();
    c->cfg = k;
    if (c->cfg.max_frames <= 0) c->cfg.max_frames = 128;
    if (const char* e = getenv("ARP_GEMM")) c->gemm_force = atoi(e);
    if (const char* e = getenv("ARP_F16C_PLAN")) {  // four digits: in_proj, out_proj, fc1, fc2 (0 plain, 1 weight correction, 2 + activation correction)
        for (int i = 0; i < 4 && e[i]; ++i)
            if (e[i] >= '0' && e[i] <= '2') c->plan[i] = e[i] - '0';
    }
    if (const char* e = getenv("ARP_ENC_STREAMS")) c->n_parts = std::max(1, std::min(atoi(e), (int)arp_enc::MAX_PARTS));
    if (const char* e = getenv("ARP_ENC_SPLIT")) c->first_part = std::max(-1, atoi(e));
    if (const char* e = getenv("ARP_ENC_MIN_PART")) c->min_part_frames = std::max(1, atoi(e));
    if (const char* e = getenv("ARP_ENC_LAT_ROWS")) c->lat_rows = std::min(std::max(atoi(e), 0), SKINNY_MAX_M);
    // fc1's plan-0 instance has no e2m1 side output, which fc2's correction K-tiles read: such a plan would run on stale operand segments
    if (c->plan[2] == 0 && c->plan[3] >= 1) {
        delete c;
        return fail("ARP_F16C_PLAN: fc2 cannot be corrected (digit 4 >= 1) when fc1 runs on the plain instance (digit 3 = 0)");
    }
    // (fc2's operand comes out of fc1's epilogue: its x4 segment from the rounded tile, its dx4 segment -- plan 2 -- straight from the accumulators)
    // (the handle's own stream serves arp_enc_forward only and is created by its first call: inside a policy step the encoder runs on the step's streams, and a
    //  process's streams share GPU_MAX_HW_QUEUES hardware queues -- arp_dt.hip)
    *out = c;
    return 0;
}

int arp_enc_destroy(arp_enc* c) {
    if (!c) return 0;
    (void)hipSetDevice(c->cfg.device);
    (void)hipDeviceSynchronize();
    delete c;
    return 0;
}

int arp_enc_load_weight(arp_enc* c, const char* name, const float* data, const int64_t* shape, int ndim) {
    if (!c || !name || !data || (ndim > 0 && !shape)) return fail("null argument");
    if (c->finalized) return fail("weights already finalized");
    HostTensor t;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) {
        t.shape.push_back(shape[i]);
        n *= (size_t)shape[i];
    }
    t.data.assign(data, data + n);
    c->staged[name] = std::move(t);
    return 0;
}

int arp_enc_finalize_weights(arp_enc* c) {
    if (!c) return fail("null handle");
    if (c->finalized) return 0;
    ARP_HIP_OK(hipSetDevice(c->cfg.device));
    const arp_enc_cfg& k = c->cfg;
    const int D = k.width, KP = k.patch * k.patch * 3, H = k.mlp_ratio * D, G = k.img_res / k.patch;
    const HostTensor* t;
    ARP_TRY(staged(c, "image_embedding/kernel", {KP, D}, &t)); ARP_TRY(up_kernel(c, t->data.data(), KP, D, &c->w_emb));
    const bool f16c = k.mode == ARP_MODE_F16C;
    if (f16c) {
        std::vector<float> tr((size_t)KP * D);
        for (int i = 0; i < KP; ++i)
            for (int o = 0; o < D; ++o) tr[(size_t)o * KP + i] = t->data[(size_t)i * D + o];
        ARP_TRY(up_kernel_x3(c, tr, KP, D, &c->w_emb3));
        for (int gi = 0; gi < 4; ++gi) { c->sw_d[gi].assign(k.layers, 0); c->sw_w[gi].assign(k.layers, 0); }
    }
    // the block GEMMs' weights: operand type, or ARP_MODE_F16C's [W_hi | dW4 (| W4)] rows (e2m1 segments) with their per-tensor scales
    // f16c with vperm: output column o of in_proj's V third (o = 2 D + head * 64 + d') carries the ORIGINAL column 2 D + head * 64 + pi(d'), pi = the swap of
    // bits [5:4] and [3:2] (an involution): the MFMA attention then holds sixteen consecutive original columns per lane (attention.h, outc == 2)
    const bool vp = f16c && c->vperm && attn_vperm_applies(c->tokens(), D / k.heads);  // (the attention instances of <= 64 tokens keep round 5's stores: tower.h)
    c->vperm = vp;
    auto vperm_col = [&](int o) { return attn_vperm_col(o, D); };
    std::vector<float> permuted;
    auto up_w = [&](const HostTensor* ht, int in, int out_, int gi, int layer, void** dst) -> int {
        const float* src = ht->data.data();
        if (vp && gi == 0) {
            permuted.resize((size_t)in * out_);
            for (int i = 0; i < in; ++i)
                for (int o = 0; o < out_; ++o) permuted[(size_t)i * out_ + o] = src[(size_t)i * out_ + vperm_col(o)];
            src = permuted.data();
        }
        if (f16c) return up_kernel_c(c, src, in, out_, c->plan[gi], dst, &c->sw_d[gi][layer], &c->sw_w[gi][layer]);
        return up_kernel(c, src, in, out_, dst);
    };
    ARP_TRY(staged(c, "image_embedding/bias", {D}, &t)); ARP_TRY(up_f32(c, t->data.data(), D, &c->b_emb));
    ARP_TRY(staged(c, "cls_token", {1, 1, D}, &t)); ARP_TRY(up_f32(c, t->data.data(), D, &c->cls));
    ARP_TRY(staged(c, "encoder_image_type_embedding", {1, 1, D}, &t));
    {   // get_2d_sincos_pos_embed (m3ae/model.py:95-136, "w goes first") + the image type embedding
        std::vector<float> pos((size_t)G * G * D);
        const int q = D / 4;  // embed_dim/2 per axis, half sin half cos
        for (int i = 0; i < G; ++i)
            for (int j = 0; j < G; ++j) {
                float* row = pos.data() + ((size_t)i * G + j) * D;
                for (int half = 0; half < 2; ++half) {
                    const double p = half == 0 ? (double)j : (double)i;  // first half encodes the w coordinate
                    for (int d = 0; d < q; ++d) {
                        const double omega = 1.0 / std::pow(10000.0, (double)d / (double)q);
                        row[half * 2 * q + d] = (float)std::sin(p * omega);
                        row[half * 2 * q + q + d] = (float)std::cos(p * omega);
                    }
                }
                for (int d = 0; d < D; ++d) row[d] += t->data[d];
            }
        ARP_TRY(up_f32(c, pos.data(), pos.size(), &c->pos));
    }
    c->tower.width = D; c->tower.layers = k.layers; c->tower.heads = k.heads;
    c->tower.L.resize(k.layers);
    for (int i = 0; i < k.layers; ++i) {
        const std::string p = "encoder/Block_" + std::to_string(i) + "/";
        LayerW& L = c->tower.L[i];
        ARP_TRY(staged(c, p + "LayerNorm_0/scale", {D}, &t)); ARP_TRY(up_f32(c, t->data.data(), D, &L.ln1_w));
        ARP_TRY(staged(c, p + "LayerNorm_0/bias", {D}, &t)); ARP_TRY(up_f32(c, t->data.data(), D, &L.ln1_b));
        ARP_TRY(staged(c, p + "LayerNorm_1/scale", {D}, &t)); ARP_TRY(up_f32(c, t->data.data(), D, &L.ln2_w));
        ARP_TRY(staged(c, p + "LayerNorm_1/bias", {D}, &t)); ARP_TRY(up_f32(c, t->data.data(), D, &L.ln2_b));
        ARP_TRY(staged(c, p + "Attention_0/Dense_0/kernel", {D, 3 * D}, &t)); ARP_TRY(up_w(t, D, 3 * D, 0, i, &L.w_in));
        ARP_TRY(staged(c, p + "Attention_0/Dense_0/bias", {3 * D}, &t));
        if (vp) {
            std::vector<float> pb(3 * D);
            for (int o = 0; o < 3 * D; ++o) pb[o] = t->data[vperm_col(o)];
            ARP_TRY(up_f32(c, pb.data(), 3 * D, &L.b_in));
        } else {
            ARP_TRY(up_f32(c, t->data.data(), 3 * D, &L.b_in));
        }
        ARP_TRY(staged(c, p + "Attention_0/Dense_1/kernel", {D, D}, &t)); ARP_TRY(up_w(t, D, D, 1, i, &L.w_out));
        ARP_TRY(staged(c, p + "Attention_0/Dense_1/bias", {D}, &t)); ARP_TRY(up_f32(c, t->data.data(), D, &L.b_out));
        ARP_TRY(staged(c, p + "TransformerMLP_0/fc1/kernel", {D, H}, &t)); ARP_TRY(up_w(t, D, H, 2, i, &L.w_fc));
        ARP_TRY(staged(c, p + "TransformerMLP_0/fc1/bias", {H}, &t)); ARP_TRY(up_f32(c, t->data.data(), H, &L.b_fc));
        ARP_TRY(staged(c, p + "TransformerMLP_0/fc2/kernel", {H, D}, &t)); ARP_TRY(up_w(t, H, D, 3, i, &L.w_proj));
        ARP_TRY(staged(c, p + "TransformerMLP_0/fc2/bias", {D}, &t)); ARP_TRY(up_f32(c, t->data.data(), D, &L.b_proj));
    }
    ARP_TRY(staged(c, "encoder/LayerNorm_0/scale", {D}, &t)); ARP_TRY(up_f32(c, t->data.data(), D, &c->lnf_w));
    ARP_TRY(staged(c, "encoder/LayerNorm_0/bias", {D}, &t)); ARP_TRY(up_f32(c, t->data.data(), D, &c->lnf_b));
    // the optional text branch: each of the two tensors is uploaded when it was staged (f32 in every mode: a row kernel adds them into the f32 residual stream);
    // arp_enc_forward_text needs both.  The vocabulary size is the embedding's first dimension.
    if (auto it = c->staged.find("text_embedding/embedding"); it != c->staged.end()) {
        const HostTensor& e = it->second;
        if (e.shape.size() != 2 || e.shape[0] < 1 || e.shape[0] > INT32_MAX || e.shape[1] != D) return fail("weight text_embedding/embedding has an unexpected shape");
        ARP_TRY(up_f32(c, e.data.data(), e.data.size(), &c->text_emb));
        c->vocab = (int)e.shape[0];
    }
    if (c->staged.count("encoder_text_type_embedding")) {
        ARP_TRY(staged(c, "encoder_text_type_embedding", {1, 1, D}, &t));
        ARP_TRY(up_f32(c, t->data.data(), D, &c->text_type));
        c->text_type_host = t->data;
    }
    c->staged.clear();
    c->finalized = true;
    return 0;
}

// The host entries' loop: frames (and goal frames) on the host -> encodings on the host, a chunk of max_frames samples at a time on the handle's own stream:
// stage, enqueue, copy out, synchronise.  goals != null is the goal-conditioned call: `seq` is ignored and built here, because its device pointer is this
// function's staging area (a chunk's goal frames behind its frames), the same for every chunk.  Otherwise seq is the call's instruction, if any, its device
// pointers into txt_dev, whose txt_bytes (ids, then words) leave the pinned block in ONE async copy in front of the first chunk; seq.at walks it by chunk.
static int forward_host(arp_enc* c, const float* images, const float* goals, int n, float* out, EncSeq seq = {}, size_t txt_bytes = 0) {
    ARP_HIP_OK(hipSetDevice(c->cfg.device));
    const int mb = c->cfg.max_frames, P1 = c->tokens(), nb0 = std::min(n, mb);
    const size_t fi = (size_t)c->cfg.img_res * c->cfg.img_res * 3;
    if (!c->stream) ARP_TRY(c->stream.create());
    if (txt_bytes) ARP_HIP_OK(hipMemcpyAsync(c->txt_dev.p, c->txt_pin.p, txt_bytes, hipMemcpyHostToDevice, c->stream));
    ARP_TRY(c->img_in.ensure((goals ? 2 : 1) * nb0 * fi * 4));
    if (goals) seq = EncSeq::goal(c->img_in.as<float>() + nb0 * fi);
    const size_t fo = (size_t)seq.tokens(P1) * c->cfg.width;
    ARP_TRY(c->out.ensure(nb0 * fo * 4));
    for (int off = 0; off < n; off += mb) {
        const int nb = std::min(mb, n - off);
        ARP_HIP_OK(hipMemcpyAsync(c->img_in.p, images + off * fi, nb * fi * 4, hipMemcpyHostToDevice, c->stream));
        if (goals) ARP_HIP_OK(hipMemcpyAsync(const_cast<float*>(seq.goals_dev), goals + off * fi, nb * fi * 4, hipMemcpyHostToDevice, c->stream));
        ARP_TRY(enc_forward_on(c, c->stream, c->img_in.as<float>(), nb, c->out.as<float>(), goals ? seq : seq.at(off, fi, P1), c->lat_host && n <= mb));
        ARP_HIP_OK(hipMemcpyAsync(out + off * fo, c->out.p, nb * fo * 4, hipMemcpyDeviceToHost, c->stream));
        ARP_HIP_OK(hipStreamSynchronize(c->stream));
    }
    return 0;
}

int arp_enc_forward(arp_enc* c, const float* images, int n, float* out) {
    if (!c || !c->finalized) return fail("encoder weights not finalized");
    if (n < 0) return fail("negative frame count");
    if (n == 0) return 0;
    if (!images || !out) return fail("null buffer");
    return forward_host(c, images, nullptr, n, out);
}

int arp_enc_forward_gc(arp_enc* c, const float* images, const float* goals, int n, float* out) {
    if (!c || !c->finalized) return fail("encoder weights not finalized");
    if (n < 0) return fail("negative pair count");
    if (n == 0) return 0;
    if (!images || !goals || !out) return fail("null buffer");
    ARP_TRY(f16c_plain_only(c, EncSeq::goal()));
    return forward_host(c, images, goals, n, out);
}
int arp_enc_gc_tokens(arp_enc* c) { return c ? EncSeq::goal().tokens(c->tokens()) : fail("null handle"); }

int arp_enc_forward_text(arp_enc* c, const float* images, int n, const int32_t* tokens, const float* mask, int L, int per_row, float* out) {
    if (!c || !c->finalized) return fail("encoder weights not finalized");
    if (n < 0) return fail("negative frame count");
    if (n == 0) return 0;
    if (!images || !out || !tokens || !mask) return fail("null buffer");
    ARP_HIP_OK(hipSetDevice(c->cfg.device));
    ARP_TRY(text_prepare(c, L));
    // ids, then words: one pinned block (the previous call synchronised before it returned: the block is free)
    const int S = per_row ? n : 1;
    const size_t tb = (size_t)S * L * 4, wb = (size_t)S * EncSeq::text(L).words(c->tokens()) * 4;
    ARP_TRY(c->txt_pin.ensure(tb + wb));
    ARP_TRY(c->txt_dev.ensure(tb + wb));
    uint32_t* words_h = reinterpret_cast<uint32_t*>(c->txt_pin.as<char>() + tb);
    ARP_TRY(text_words(c, tokens, mask, S, L, words_h));
    memcpy(c->txt_pin.p, tokens, tb);
    return forward_host(c, images, nullptr, n, out, EncSeq::text(L, per_row, c->txt_dev.as<int32_t>(), reinterpret_cast<const uint32_t*>(c->txt_dev.as<char>() + tb), words_h),
                        tb + wb);
}
int arp_enc_text_tokens(arp_enc* c, int L) { return c && L >= 0 ? c->tokens() + L : fail("null handle or negative length"); }

// Part streams of a call (see arp_enc::Ws).  n_streams 1 = everything on the caller's stream (rounds 1-5); first_part_frames > 0: that many frames in part 0 of two, 0: the default cut (15/32), < 0: equal parts;
// min_part_frames <= 0 keeps the default (a part of fewer frames runs with fewer parts).  Takes effect from the next call.
int arp_enc_set_streams(arp_enc* c, int n_streams, int first_part_frames, int min_part_frames) {
    if (!c || n_streams < 1 || n_streams > arp_enc::MAX_PARTS) return fail("n_streams must be 1..4");
    c->n_parts = n_streams;
    c->first_part = first_part_frames;
    if (min_part_frames > 0) c->min_part_frames = min_part_frames;
    return 0;
}

// The latency path's row limit (arp_enc::lat_rows; 0 disables the path for every caller) and whether arp_enc_forward takes the path too (host_calls: 0 / 1,
// < 0 leaves it).  Takes effect from the next call.
int arp_enc_set_latency(arp_enc* c, int rows, int host_calls) {
    if (!c || rows < 0) return fail("set_latency: rows must be >= 0");
    c->lat_rows = std::min(rows, SKINNY_MAX_M);
    if (host_calls >= 0) c->lat_host = host_calls != 0;
    return 0;
}

int arp_enc_profile_enable(arp_enc* c, int on) {
    if (!c) return fail("null handle");
    c->prof.on = on != 0;
    return 0;
}
int arp_enc_profile_json(arp_enc* c, char* buf, int buf_len) {
    if (!c || !buf) return fail("null argument");
    const std::string s = c->prof.json();
    if ((int)s.size() + 1 > buf_len) return fail("profile buffer too small");
    memcpy(buf, s.c_str(), s.size() + 1);
    return (int)s.size();
}

// Test hook for the MIXC instances of gemm256_nt_kernel (ARP_MODE_F16C's products): A [M, K] and W [N, K] f32; the operand rows are built as the
// encoder builds them -- A: [rn16(a) | fp4(rn16(a) 2^1) | fp4((a - rn16(a)) 2^13)], W: [rn16(w) | fp4(dw 2^sd) (| fp4(w 2^sw))] for plan 1 (2) --
// and out = A.W^T + bias as f32.  sd_sw (optional, 2 ints) receives the weight scales so that a test can restate the quantisation exactly.
int arp_op_gemm_f16c(int plan, const float* A, const float* W, const float* bias, float* out, int M, int N, int K, int* sd_sw) {
    if (!A || !W || !out || M <= 0 || N <= 0 || K < 512 || K % 256 || N % 8 || plan < 0 || plan > 2) return fail("bad argument (K % 256, K >= 512, N % 8, plan 0..2)");
    DevBuf dA, dW, dB, dO;
    std::vector<uint8_t> ha((size_t)M * 3 * K, 0), hw;
    constexpr float sx = (float)(1 << F16C_X_SHIFT), sdx = (float)(1 << F16C_DX_SHIFT);
    for (int m = 0; m < M; ++m) {
        uint8_t* row = ha.data() + (size_t)m * 3 * K;
        for (int k = 0; k < K; ++k) {
            const float a = A[(size_t)m * K + k];
            const f16_t h = host_f2h(a);
            const float hf = (float)__builtin_bit_cast(_Float16, h.b);
            memcpy(row + 2 * (size_t)k, &h.b, 2);
            const int sh = (k & 1) * 4;
            row[2 * (size_t)K + k / 2] |= (uint8_t)(host_f2fp4(hf * sx) << sh);
            row[2 * (size_t)K + K / 2 + k / 2] |= (uint8_t)(host_f2fp4((a - hf) * sdx) << sh);
        }
    }
    int sd = 0, sw = 0;
    pack_weight_c([&](int i, int o) { return W[(size_t)o * K + i]; }, K, N, plan, hw, &sd, &sw);
    if (sd_sw) { sd_sw[0] = sd; sd_sw[1] = sw; }
    ARP_TRY(dA.ensure(ha.size() + 512)); ARP_TRY(dW.ensure(hw.size() + 512)); ARP_TRY(dO.ensure((size_t)M * N * 4));
    ARP_HIP_OK(hipMemcpy(dA.p, ha.data(), ha.size(), hipMemcpyHostToDevice));
    ARP_HIP_OK(hipMemcpy(dW.p, hw.data(), hw.size(), hipMemcpyHostToDevice));
    if (bias) {
        ARP_TRY(dB.ensure((size_t)N * 4));
        ARP_HIP_OK(hipMemcpy(dB.p, bias, (size_t)N * 4, hipMemcpyHostToDevice));
    }
    GemmArgs g;
    g.A = dA.p; g.W = dW.p; g.bias = bias ? dB.as<float>() : nullptr; g.out = dO.p;
    g.M = M; g.N = N; g.lda = K + K / 2; g.ldw = K + plan * K / 4; g.ldr = N; g.ldo = N;
    g.mix_nk16 = K / 64; g.mix_nkc_a = plan >= 1 ? K / 256 : 0; g.K = K + plan * K / 4;
    g.mix_sa = F16C_X_SHIFT + sd; g.mix_sb = F16C_DX_SHIFT + sw;
    if (plan == 0) ARP_TRY((launch_gemm256_nt<f16_t, float, ACT_NONE, false, 8 + SITE_OP>(g, nullptr)));
    else ARP_TRY((launch_gemm256_nt<f16_t, float, ACT_NONE, false, 8 + SITE_OP, false, 1, true>(g, nullptr)));
    ARP_HIP_OK(hipDeviceSynchronize());
    ARP_HIP_OK(hipMemcpy(out, dO.p, (size_t)M * N * 4, hipMemcpyDeviceToHost));
    return 0;
}

// split3_kernel through the f16x3 encoder's own launcher: x f32 [rows, K] -> out, a byte buffer the caller fills (up before the launch, back after it
// whatever the launcher returned), rows of 3 K binary16 values [hi | lo | hi]
int arp_op_split3(const float* x, void* out, size_t out_bytes, int rows, int K) {
    if (!x || !out || rows <= 0 || K <= 0 || out_bytes < (size_t)rows * K * 6) return fail("arp_op_split3: bad argument");
    DevBuf dx, dout;
    ARP_TRY(dx.ensure((size_t)rows * K * 4)); ARP_TRY(dout.ensure(out_bytes));
    ARP_HIP_OK(hipMemcpy(dx.p, x, (size_t)rows * K * 4, hipMemcpyHostToDevice));
    ARP_HIP_OK(hipMemcpy(dout.p, out, out_bytes, hipMemcpyHostToDevice));
    const int rc = launch_split3(nullptr, dx.as<float>(), dout.as<f16_t>(), (size_t)rows, K);
    ARP_HIP_OK(hipDeviceSynchronize());
    ARP_HIP_OK(hipMemcpy(out, dout.p, out_bytes, hipMemcpyDeviceToHost));
    return rc;
}

// The encoder's front: images f32 NHWC [n, res, res, 3] -> patch rows through the launcher front_end calls.  form 0 / 1 / 2: patchify_kernel<float | bf16 |
// binary16>, rows of 3 P^2 values; form 3: patchify_split3_kernel, rows of 9 P^2 binary16 values [hi | lo | hi].  out goes up before the launch and comes back
// after it.
int arp_op_patchify(const float* images, int n, int res, int patch, int form, void* out) {
    if (!images || !out || n <= 0 || res <= 0 || patch <= 0 || form < 0 || form > 3) return fail("arp_op_patchify: bad argument");
    if (patch % 4 || res % patch) return fail("arp_op_patchify: patch must be a multiple of 4 that divides res (four values of a patch row per thread)");
    const size_t vals = (size_t)n * res * res * 3, ob = vals * (form == 0 ? 4 : form == 3 ? 6 : 2);
    DevBuf dx, dout;
    ARP_TRY(dx.ensure(vals * 4)); ARP_TRY(dout.ensure(ob));
    ARP_HIP_OK(hipMemcpy(dx.p, images, vals * 4, hipMemcpyHostToDevice));
    ARP_HIP_OK(hipMemcpy(dout.p, out, ob, hipMemcpyHostToDevice));
    const float* src = dx.as<float>();
    const int rc = form == 0   ? launch_patchify<float, false>(nullptr, src, dout.as<float>(), n, res, patch)
                   : form == 1 ? launch_patchify<bf16_t, false>(nullptr, src, dout.as<bf16_t>(), n, res, patch)
                   : form == 2 ? launch_patchify<f16_t, false>(nullptr, src, dout.as<f16_t>(), n, res, patch)
                               : launch_patchify<f16_t, true>(nullptr, src, dout.as<f16_t>(), n, res, patch);
    ARP_HIP_OK(hipDeviceSynchronize());
    ARP_HIP_OK(hipMemcpy(out, dout.p, ob, hipMemcpyDeviceToHost));
    return rc;
}

// enc_assemble_kernel through the encoder's own launcher, on host arrays: pe [(goal ? 2 : 1) nb GG, D], cls [D], pos [GG, D]; with L > 0 text_emb [vocab, D],
// tpos [L, D] and tok int32 [L] (per_row: [nb, L]); x [nb, 1 + GG (+ GG | + L), D] goes up before the launch and comes back after it
int arp_op_m3ae_assemble(const float* pe, const float* cls, const float* pos, const float* text_emb, const float* tpos, const int32_t* tok, int nb, int GG, int goal,
                         int L, int per_row, int D, int vocab, float* x) {
    if (!pe || !cls || !pos || !x || nb <= 0 || GG <= 0 || D <= 0 || L < 0 || (L > 0 && (!text_emb || !tpos || !tok || vocab <= 0))) return fail("m3ae_assemble: bad argument");
    if (D % 4) return fail("m3ae_assemble: the width must be a multiple of 4 (float4 accesses)");
    if (goal && L > 0) return fail("m3ae_assemble: an instruction and a goal frame do not combine");
    const size_t n_tok = L > 0 ? (size_t)(per_row ? nb : 1) * L : 0;
    for (size_t i = 0; i < n_tok; ++i)
        if (tok[i] < 0 || tok[i] >= vocab) return fail("m3ae_assemble: token id " + std::to_string(tok[i]) + " is outside the vocabulary [0, " + std::to_string(vocab) + ")");
    DevBuf dpe, dcls, dpos, demb, dtpos, dtok, dx;
    auto up = [](DevBuf& d, const void* src, size_t bytes) -> int {
        ARP_TRY(d.ensure(bytes));
        ARP_HIP_OK(hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice));
        return 0;
    };
    ARP_TRY(up(dpe, pe, (size_t)(goal ? 2 : 1) * nb * GG * D * 4)); ARP_TRY(up(dcls, cls, (size_t)D * 4)); ARP_TRY(up(dpos, pos, (size_t)GG * D * 4));
    if (L > 0) { ARP_TRY(up(demb, text_emb, (size_t)vocab * D * 4)); ARP_TRY(up(dtpos, tpos, (size_t)L * D * 4)); ARP_TRY(up(dtok, tok, n_tok * 4)); }
    const EncSeq seq = goal ? EncSeq::goal() : L > 0 ? EncSeq::text(L, per_row, dtok.as<int32_t>()) : EncSeq{};
    const size_t xb = (size_t)nb * seq.tokens(1 + GG) * D * 4;
    ARP_TRY(up(dx, x, xb));
    const int rc = launch_assemble(nullptr, dpe.as<float>(), dcls.as<float>(), dpos.as<float>(), demb.as<float>(), dtpos.as<float>(), seq, dx.as<float>(), nb, GG, D);
    ARP_HIP_OK(hipDeviceSynchronize());
    ARP_HIP_OK(hipMemcpy(x, dx.p, xb, hipMemcpyDeviceToHost));
    return rc;
}

}  // extern "C"
