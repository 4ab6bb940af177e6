// A demonstration set resident in HBM, and the gathers that build policy batches from row indices.
// Reference seam: ProcgenDataset.__getitem__, /root/reference/arp_dt/data_procgen.py:180-213 -- `ob[i][-T:]`, `act[i][-T:]`, `rtgs[i][-T:]` of a file whose
// rows the recorder stacks (data/PPG/trajectory_recorder.py:103-112): row i adds ONE frame, ob[i, -1], and its window is
//     j(t) = max(i - (T - 1 - t), s[i]),  t = 0..T-1,   s[i] = the first row of i's trajectory.
// The set keeps that one frame per row (uint8), the per-row action / return-to-go / s, optionally one encoding per row, and a batch is B row indices:
// no frame crosses PCIe after the load.  Host orchestration + C ABI of the arp_ds handle; the policy handle's side is arp_dt.hip (ds_internal.h).

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/arp_hip.h"
#include "common.h"
#include "ds_internal.h"
#include "enc_internal.h"
#include "runtime.h"

using namespace arp;

struct arp_ds {
    int n_rows = 0, res = 0, device = 0;
    size_t fb = 0;  // bytes of one uint8 frame = floats of one f32 frame
    DevBuf frames, action, rtg, start, lut, enc, iota, qfirst, qlast;  // qfirst / qlast: the fine-tune quads' per-row trajectory interval (arp_ds_set_quad_bounds)
    std::vector<uint8_t> row_up, enc_up;  // which rows have been uploaded
    int n_up = 0, n_enc_up = 0;
    bool labels = false, has_rtg = false, has_lut = false, has_quads = false;
    int n_actions = 0, tokens = 0, dim = 0;
    size_t enc_row() const { return (size_t)tokens * dim; }
};
static_assert(!std::is_copy_constructible_v<arp_ds>);

namespace {

constexpr int DS_THREADS = 256;
constexpr int DS_TARGET_BLOCKS = 2048;  // 8 per CU: enough 16-byte loads in flight to cover the HBM latency

// the source row of frame f = b * T + t of the batch (uniform per block: scalar loads)
__device__ __forceinline__ int ds_source_row(const int32_t* __restrict__ idx, const int32_t* __restrict__ start, int f, int T) {
    const int i = idx[f / T], t = f % T;
    return max(i - (T - 1 - t), start ? start[i] : 0);
}

// out[f] = lut[c][frames[j(f)]]: uint8 NHWC frames -> the f32 frames the encoder reads.  One block walks `iters` tiles of 256 x 16 bytes of ONE frame:
// every lane loads 16 bytes (1 KiB per wave instruction), the tile is turned through LDS so that lane l of store s holds the dword (s * 256 + l) of the tile,
// and every store instruction writes 16 bytes per lane, 1 KiB contiguous per wave.  The table sits in LDS (3 KB); the written value is exactly lut[c][u].
__device__ __forceinline__ void ds_frame_gather_body(const uint8_t* __restrict__ frames, const int32_t* __restrict__ idx, const int32_t* __restrict__ start,
                                                     const float* __restrict__ lut, float* __restrict__ out, int T, uint32_t chunks, int iters) {
    __shared__ float s_lut[3 * 256];
    __shared__ uint4 s_tile[2][DS_THREADS];
    const int tid = threadIdx.x, f = blockIdx.y;
    for (int i = tid; i < 3 * 256; i += DS_THREADS) s_lut[i] = lut[i];
    const int j = ds_source_row(idx, start, f, T);
    const uint4* __restrict__ src = reinterpret_cast<const uint4*>(frames + (size_t)j * chunks * 16);
    float4* __restrict__ dst = reinterpret_cast<float4*>(out + (size_t)f * chunks * 16);
    const uint32_t dwords = chunks * 4;
    for (int it = 0; it < iters; ++it) {
        const uint32_t c0 = ((uint32_t)blockIdx.x * iters + it) * DS_THREADS;  // (uniform)
        if (c0 >= chunks) break;
        s_tile[it & 1][tid] = c0 + tid < chunks ? src[c0 + tid] : make_uint4(0, 0, 0, 0);
        __syncthreads();  // (also orders the table's fill before its first read; the other half of s_tile is what iteration it - 1 read)
        const uint32_t* w = reinterpret_cast<const uint32_t*>(s_tile[it & 1]);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const uint32_t k = s * DS_THREADS + tid, dw = c0 * 4 + k;
            if (dw < dwords) {
                const uint32_t u = w[k], ph = dw % 3;  // byte 4 * dw of an RGB-interleaved frame is channel (4 * dw) % 3 = dw % 3
                const uint32_t c1 = ph == 2 ? 0 : ph + 1, c2 = c1 == 2 ? 0 : c1 + 1;
                dst[dw] = make_float4(s_lut[ph * 256 + (u & 255)], s_lut[c1 * 256 + ((u >> 8) & 255)], s_lut[c2 * 256 + ((u >> 16) & 255)],
                                      s_lut[ph * 256 + (u >> 24)]);
            }
        }
    }
}

__global__ __launch_bounds__(DS_THREADS) void ds_frame_gather_kernel(const uint8_t* __restrict__ frames, const int32_t* __restrict__ idx,
                                                                      const int32_t* __restrict__ start, const float* __restrict__ lut,
                                                                      float* __restrict__ out, int T, uint32_t chunks, int iters) {
    ds_frame_gather_body(frames, idx, start, lut, out, T, chunks, iters);
}

// A (frame, goal) pair slot in ONE launch (model GCBC): grid z = 0 fills `out` with the windows of idx, z = 1 fills `goals` with the windows of gidx -- the
// goal frames of sample b are the window of its goal row under the same rule (data_procgen.py:189 reads ob[g][-T:]).  z and not a doubled y: B * T alone may
// reach grid y's 65 535.  Same block shape, same loads, same LDS turn, same stores as the kernel above (its body).
__global__ __launch_bounds__(DS_THREADS) void ds_frame_gather_pairs_kernel(const uint8_t* __restrict__ frames, const int32_t* __restrict__ idx,
                                                                            const int32_t* __restrict__ gidx, const int32_t* __restrict__ start,
                                                                            const float* __restrict__ lut, float* __restrict__ out, float* __restrict__ goals,
                                                                            int T, uint32_t chunks, int iters) {
    const bool g = blockIdx.z != 0;  // (uniform)
    ds_frame_gather_body(frames, g ? gidx : idx, start, lut, g ? goals : out, T, chunks, iters);
}

// out[f] = cache[j(f)]: row copies of `vec` 16-byte vectors
__global__ __launch_bounds__(DS_THREADS) void ds_enc_gather_kernel(const float* __restrict__ cache, const int32_t* __restrict__ idx,
                                                                    const int32_t* __restrict__ start, float* __restrict__ out, int T, uint32_t vec) {
    const int f = blockIdx.y;
    const int j = ds_source_row(idx, start, f, T);
    const uint4* __restrict__ src = reinterpret_cast<const uint4*>(cache + (size_t)j * vec * 4);
    uint4* __restrict__ dst = reinterpret_cast<uint4*>(out + (size_t)f * vec * 4);
    for (uint32_t v = blockIdx.x * DS_THREADS + threadIdx.x; v < vec; v += gridDim.x * DS_THREADS) dst[v] = src[v];
}

__global__ void ds_label_gather_kernel(const int32_t* __restrict__ action, const float* __restrict__ rtg, const int32_t* __restrict__ idx,
                                       const int32_t* __restrict__ start, int32_t* __restrict__ action_out, float* __restrict__ rtg_out, int T, int n) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    const int j = ds_source_row(idx, start, f, T);
    if (action_out) action_out[f] = action[j];
    if (rtg_out) rtg_out[f] = rtg[j];
}

// The fine-tune step's four rows (finetune_module/action_finetune_data_procgen.py:144,162,164): one lane per sample,
//     q = sort(first[i], i, min(i + 1, last[i]), last[i]),  r = q[2] == q[3],  action = action[q[0]].
// The sort is not a formality: a row behind the last done flag carries trajectory 0's interval, which does not contain it (arp_amd/finetune_data.py).  A fixed
// five-comparator network; rows go out group-major (rows_out[g * B + b], g < G), the order the head reads image0 | image1 | image2 (| image3).
__global__ void ds_quads_kernel(const int32_t* __restrict__ idx, const int32_t* __restrict__ first, const int32_t* __restrict__ last,
                                const int32_t* __restrict__ action, int B, int G, int32_t* __restrict__ rows_out, float* __restrict__ r_out,
                                int32_t* __restrict__ action_out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int i = idx[b], l = last[i];
    int q0 = first[i], q1 = i, q2 = min(i + 1, l), q3 = l;
    auto cx = [](int& x, int& y) { const int lo = min(x, y), hi = max(x, y); x = lo; y = hi; };
    cx(q0, q1); cx(q2, q3); cx(q0, q2); cx(q1, q3); cx(q1, q2);
    const int q[4] = {q0, q1, q2, q3};
#pragma unroll
    for (int g = 0; g < 4; ++g)
        if (g < G) rows_out[(size_t)g * B + b] = q[g];
    r_out[b] = q2 == q3 ? 1.f : 0.f;
    action_out[b] = action[q0];
}

// blocks along a row: enough for DS_TARGET_BLOCKS in all, at most one per tile
inline int row_blocks(size_t tiles, int n) { return (int)std::max<size_t>(1, std::min<size_t>(tiles, (DS_TARGET_BLOCKS + n - 1) / n)); }

int check_rows(const arp_ds* d, int row0, int n, const void* host) {
    if (!d || !host) return fail("null argument");
    if (row0 < 0 || n <= 0 || (long long)row0 + n > d->n_rows) return fail("rows [" + std::to_string(row0) + ", " + std::to_string((long long)row0 + n) + ") are outside the dataset's " + std::to_string(d->n_rows) + " rows");
    return 0;
}

}  // namespace

namespace arp {

int ds_check_batch(arp_ds* d, const int64_t* idx, int B, int window, int device, int n_actions, bool need_rtg, int use_encodings, int res, int tokens, int dim) {
    if (!d || !idx || B <= 0) return fail("bad argument");
    if (window < 1 || window > 64) return fail("window must be in 1..64");
    if ((long long)B * window > 65535) return fail("B * window must not exceed 65535");
    if (d->device != device) return fail("the dataset lives on device " + std::to_string(d->device) + ", the handle on device " + std::to_string(device));
    if (use_encodings > 0) {
        if (!d->enc.p) return fail("use_encodings: the dataset holds no encodings (cache_encodings / set_encodings first)");
        if (d->n_enc_up != d->n_rows) return fail("use_encodings: only " + std::to_string(d->n_enc_up) + " of " + std::to_string(d->n_rows) + " encoding rows are present");
        if (d->tokens != tokens || d->dim != dim)
            return fail("the dataset's encodings are [" + std::to_string(d->tokens) + ", " + std::to_string(d->dim) + "] per frame, the handle expects [" + std::to_string(tokens) + ", " + std::to_string(dim) + "]");
    } else if (use_encodings == 0) {
        if (d->n_up != d->n_rows) return fail("only " + std::to_string(d->n_up) + " of " + std::to_string(d->n_rows) + " frame rows were uploaded");
        if (!d->has_lut) return fail("the dataset has no byte -> float table (arp_ds_set_lut)");
        if (d->res != res) return fail("the dataset's frames are " + std::to_string(d->res) + " pixels square, the encoder reads " + std::to_string(res));
    }
    if (!d->labels) return fail("the dataset's labels are not set (arp_ds_set_labels)");
    if (need_rtg && !d->has_rtg) return fail("the dataset holds no return-to-go (only model BC reads none)");
    if (n_actions > 0 && d->n_actions > n_actions) return fail("the dataset's actions go up to " + std::to_string(d->n_actions) + " ids, the handle has " + std::to_string(n_actions));
    for (int b = 0; b < B; ++b)
        if (idx[b] < 0 || idx[b] >= d->n_rows) return fail("index " + std::to_string((long long)idx[b]) + " (batch position " + std::to_string(b) + ") is outside [0, " + std::to_string(d->n_rows) + ")");
    return 0;
}

// start == nullptr: no clamp (arp_ds_encode's identity gather, window 1: the source row is the index itself)
static int gather_impl(arp_ds* d, hipStream_t st, const int32_t* idx_dev, const int32_t* start, int B, int T, float* frames_out, float* enc_out, int32_t* action_out,
                       float* rtg_out) {
    const int n = B * T;
    if (frames_out) {
        const uint32_t chunks = (uint32_t)(d->fb / 16);
        const size_t tiles = (chunks + DS_THREADS - 1) / DS_THREADS;
        const int iters = (int)((tiles + row_blocks(tiles, n) - 1) / row_blocks(tiles, n));
        const int gx = (int)((tiles + iters - 1) / iters);
        hipLaunchKernelGGL(ds_frame_gather_kernel, dim3(gx, n), dim3(DS_THREADS), 0, st, d->frames.as<uint8_t>(), idx_dev, start, d->lut.as<float>(), frames_out, T,
                           chunks, iters);
    }
    if (enc_out) {
        const uint32_t vec = (uint32_t)(d->enc_row() / 4);
        const size_t tiles = (vec + DS_THREADS - 1) / DS_THREADS;
        hipLaunchKernelGGL(ds_enc_gather_kernel, dim3(row_blocks(tiles, n), n), dim3(DS_THREADS), 0, st, d->enc.as<float>(), idx_dev, start, enc_out, T, vec);
    }
    if (action_out || rtg_out)
        hipLaunchKernelGGL(ds_label_gather_kernel, dim3((n + 63) / 64), dim3(64), 0, st, d->action.as<int32_t>(), rtg_out ? d->rtg.as<float>() : nullptr, idx_dev, start,
                           action_out, rtg_out, T, n);
    ARP_HIP_OK(hipGetLastError());
    return 0;
}

int ds_gather_on(arp_ds* d, hipStream_t st, const int32_t* idx_dev, int B, int T, float* frames_out, float* enc_out, int32_t* action_out, float* rtg_out) {
    if (!d->labels) return fail("the dataset's labels are not set (arp_ds_set_labels)");
    return gather_impl(d, st, idx_dev, d->start.as<int32_t>(), B, T, frames_out, enc_out, action_out, rtg_out);
}

int ds_check_goals(arp_ds* d, const int64_t* gidx, int B) {
    if (!d || !gidx || B <= 0) return fail("bad argument");
    for (int b = 0; b < B; ++b)
        if (gidx[b] < 0 || gidx[b] >= d->n_rows)
            return fail("goal index " + std::to_string((long long)gidx[b]) + " (batch position " + std::to_string(b) + ") is outside [0, " + std::to_string(d->n_rows) + ")");
    return 0;
}

int ds_gather_pairs_on(arp_ds* d, hipStream_t st, const int32_t* idx_dev, const int32_t* gidx_dev, int B, int T, float* frames_out, float* goals_out,
                       int32_t* action_out) {
    if (!d->labels) return fail("the dataset's labels are not set (arp_ds_set_labels)");
    if (!frames_out != !goals_out) return fail("a pair gather writes frames and goals together (or the labels alone)");
    const int n = B * T;
    if (frames_out) {  // the grid of gather_impl's frame launch, twice along z
        const uint32_t chunks = (uint32_t)(d->fb / 16);
        const size_t tiles = (chunks + DS_THREADS - 1) / DS_THREADS;
        const int iters = (int)((tiles + row_blocks(tiles, n) - 1) / row_blocks(tiles, n));
        const int gx = (int)((tiles + iters - 1) / iters);
        hipLaunchKernelGGL(ds_frame_gather_pairs_kernel, dim3(gx, n, 2), dim3(DS_THREADS), 0, st, d->frames.as<uint8_t>(), idx_dev, gidx_dev, d->start.as<int32_t>(),
                           d->lut.as<float>(), frames_out, goals_out, T, chunks, iters);
    }
    if (action_out)  // GCBC reads no return-to-go
        hipLaunchKernelGGL(ds_label_gather_kernel, dim3((n + 63) / 64), dim3(64), 0, st, d->action.as<int32_t>(), (const float*)nullptr, idx_dev,
                           d->start.as<int32_t>(), action_out, (float*)nullptr, T, n);
    ARP_HIP_OK(hipGetLastError());
    return 0;
}

int ds_check_quads(arp_ds* d, const int64_t* idx, int B, int G, int device, int n_actions, int* res) {
    if (!d || !idx || B <= 0) return fail("bad argument");
    if (G != 3 && G != 4) return fail("a fine-tune sample has 3 image groups, or 4 with its goal frame");
    if (d->device != device) return fail("the dataset lives on device " + std::to_string(d->device) + ", the handle on device " + std::to_string(device));
    if (!d->labels) return fail("the dataset's labels are not set (arp_ds_set_labels)");
    if (!d->has_quads) return fail("the dataset's quad bounds are not set (arp_ds_set_quad_bounds)");
    if (d->n_up != d->n_rows) return fail("only " + std::to_string(d->n_up) + " of " + std::to_string(d->n_rows) + " frame rows were uploaded");
    if (n_actions > 0 && d->n_actions > n_actions) return fail("the dataset's actions go up to " + std::to_string(d->n_actions) + " ids, the handle has " + std::to_string(n_actions));
    for (int b = 0; b < B; ++b)
        if (idx[b] < 0 || idx[b] >= d->n_rows) return fail("index " + std::to_string((long long)idx[b]) + " (batch position " + std::to_string(b) + ") is outside [0, " + std::to_string(d->n_rows) + ")");
    if (res) *res = d->res;
    return 0;
}

int ds_quads_on(arp_ds* d, hipStream_t st, const int32_t* idx_dev, int B, int G, int32_t* rows_out, float* r_out, int32_t* action_out) {
    if (!d->labels || !d->has_quads) return fail("the dataset's labels and quad bounds must be set (arp_ds_set_labels, arp_ds_set_quad_bounds)");
    if (B <= 0 || (G != 3 && G != 4) || !idx_dev || !rows_out || !r_out || !action_out) return fail("ds_quads_on: bad argument");
    hipLaunchKernelGGL(ds_quads_kernel, dim3((B + 63) / 64), dim3(64), 0, st, idx_dev, d->qfirst.as<int32_t>(), d->qlast.as<int32_t>(), d->action.as<int32_t>(), B, G,
                       rows_out, r_out, action_out);
    ARP_HIP_OK(hipGetLastError());
    return 0;
}

const uint8_t* ds_frames_of(arp_ds* d) { return d->frames.as<uint8_t>(); }

int ds_info(arp_ds* d, int* n_rows, int* res, int* device) {
    if (!d) return fail("null dataset handle");
    *n_rows = d->n_rows; *res = d->res; *device = d->device;
    return 0;
}

}  // namespace arp

extern "C" {

// The per-row trajectory interval the fine-tune quads are computed from (ProcgenActionDataset.bounds()): 0 <= first <= last < n_rows for every row.
// NOT first <= row <= last: the rows behind the last done flag carry trajectory 0's interval (the reference's quirk, kept).
int arp_ds_set_quad_bounds(arp_ds* d, const int32_t* first, const int32_t* last) {
    if (!d || !first || !last) return fail("null argument");
    for (int i = 0; i < d->n_rows; ++i)
        if (first[i] < 0 || first[i] > last[i] || last[i] >= d->n_rows)
            return fail("row " + std::to_string(i) + ": quad bounds [" + std::to_string(first[i]) + ", " + std::to_string(last[i]) + "] are not an interval inside [0, " +
                        std::to_string(d->n_rows) + ")");
    ARP_HIP_OK(hipSetDevice(d->device));
    const size_t nb = (size_t)d->n_rows * 4;
    ARP_TRY(d->qfirst.ensure(nb));
    ARP_TRY(d->qlast.ensure(nb));
    ARP_HIP_OK(hipMemcpy(d->qfirst.p, first, nb, hipMemcpyHostToDevice));
    ARP_HIP_OK(hipMemcpy(d->qlast.p, last, nb, hipMemcpyHostToDevice));
    d->has_quads = true;
    return 0;
}

// Debug read-back of the quads B indices name: rows_out int32 [G, B] (group-major), r_out f32 [B], action_out int32 [B].  Synchronous, on the null stream.
int arp_ds_quads_debug(arp_ds* d, const int64_t* idx, int B, int G, int32_t* rows_out, float* r_out, int32_t* action_out) {
    if (!d || !rows_out || !r_out || !action_out) return fail("null argument");
    ARP_TRY(ds_check_quads(d, idx, B, G, d->device, 0, nullptr));
    ARP_HIP_OK(hipSetDevice(d->device));
    std::vector<int32_t> h(idx, idx + B);
    // each output is followed on the device by one guard word the kernel must leave alone: a store past an array's end is an error of this call
    constexpr uint32_t GUARD = 0x5a5a5a5au;
    const size_t nq = (size_t)G * B, nb = (size_t)B;
    DevBuf di, dq, dr, da;  // (freed on every return; hipFree waits for the kernel)
    ARP_TRY(di.ensure(nb * 4));
    ARP_TRY(dq.ensure((nq + 1) * 4));
    ARP_TRY(dr.ensure((nb + 1) * 4));
    ARP_TRY(da.ensure((nb + 1) * 4));
    ARP_HIP_OK(hipMemcpy(di.p, h.data(), nb * 4, hipMemcpyHostToDevice));
    ARP_HIP_OK(hipMemcpy(dq.as<uint32_t>() + nq, &GUARD, 4, hipMemcpyHostToDevice));
    ARP_HIP_OK(hipMemcpy(dr.as<uint32_t>() + nb, &GUARD, 4, hipMemcpyHostToDevice));
    ARP_HIP_OK(hipMemcpy(da.as<uint32_t>() + nb, &GUARD, 4, hipMemcpyHostToDevice));
    ARP_TRY(ds_quads_on(d, nullptr, di.as<int32_t>(), B, G, dq.as<int32_t>(), dr.as<float>(), da.as<int32_t>()));
    uint32_t g[3] = {0, 0, 0};
    ARP_HIP_OK(hipMemcpy(&g[0], dq.as<uint32_t>() + nq, 4, hipMemcpyDeviceToHost));
    ARP_HIP_OK(hipMemcpy(&g[1], dr.as<uint32_t>() + nb, 4, hipMemcpyDeviceToHost));
    ARP_HIP_OK(hipMemcpy(&g[2], da.as<uint32_t>() + nb, 4, hipMemcpyDeviceToHost));
    if (g[0] != GUARD || g[1] != GUARD || g[2] != GUARD) return fail("arp_ds_quads_debug: the quad kernel wrote past the end of an output");
    ARP_HIP_OK(hipMemcpy(rows_out, dq.p, nq * 4, hipMemcpyDeviceToHost));
    ARP_HIP_OK(hipMemcpy(r_out, dr.p, nb * 4, hipMemcpyDeviceToHost));
    ARP_HIP_OK(hipMemcpy(action_out, da.p, nb * 4, hipMemcpyDeviceToHost));
    return 0;
}

int arp_ds_create(int64_t n_rows, int res, int device, arp_ds** out) {
    if (!out) return fail("null argument");
    if (n_rows <= 0 || n_rows > (1ll << 30)) return fail("n_rows must be in 1..2^30");
    if (res <= 0 || res > 4096) return fail("res must be in 1..4096");
    if ((size_t)res * res * 3 % 16) return fail("res * res * 3 must be a multiple of 16 (the gather moves 16 bytes per lane)");
    int ndev = 0;
    ARP_HIP_OK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail("no such HIP device: " + std::to_string(device));
    ARP_HIP_OK(hipSetDevice(device));
    ARP_TRY(prime_runtime(device));
    arp_ds* d = new arp_ds();
    d->n_rows = (int)n_rows;
    d->res = res;
    d->device = device;
    d->fb = (size_t)res * res * 3;
    d->row_up.assign(d->n_rows, 0);
    if (d->frames.ensure(d->fb * d->n_rows) != 0 || d->lut.ensure(3 * 256 * 4) != 0) {  // (an allocation that fails is an error string)
        arp_ds_destroy(d);
        return -1;
    }
    *out = d;
    return 0;
}

int arp_ds_destroy(arp_ds* d) {
    if (!d) return 0;
    (void)hipSetDevice(d->device);
    (void)hipDeviceSynchronize();  // (a gather of a policy handle may still be reading)
    delete d;
    return 0;
}

int arp_ds_upload_frames(arp_ds* d, int64_t row0, int64_t n, const uint8_t* u8_host) {
    if (!d || row0 < 0 || n <= 0 || row0 > d->n_rows || n > d->n_rows) return fail("bad argument");
    ARP_TRY(check_rows(d, (int)row0, (int)n, u8_host));
    ARP_HIP_OK(hipSetDevice(d->device));
    ARP_HIP_OK(hipMemcpy(d->frames.as<uint8_t>() + (size_t)row0 * d->fb, u8_host, (size_t)n * d->fb, hipMemcpyHostToDevice));
    for (int64_t r = row0; r < row0 + n; ++r)
        if (!d->row_up[r]) { d->row_up[r] = 1; ++d->n_up; }
    return 0;
}

int arp_ds_set_labels(arp_ds* d, const int32_t* action, const float* rtg, const int32_t* traj_start, int n_actions) {
    if (!d || !action || !traj_start) return fail("null argument");
    if (n_actions <= 0) return fail("n_actions must be positive");
    for (int i = 0; i < d->n_rows; ++i) {
        if (action[i] < 0 || action[i] >= n_actions) return fail("row " + std::to_string(i) + ": action id " + std::to_string(action[i]) + " is outside [0, " + std::to_string(n_actions) + ")");
        if (traj_start[i] < 0 || traj_start[i] > i) return fail("row " + std::to_string(i) + ": traj_start " + std::to_string(traj_start[i]) + " is outside [0, row]");
        if (i && traj_start[i] < traj_start[i - 1]) return fail("row " + std::to_string(i) + ": traj_start decreases");
    }
    ARP_HIP_OK(hipSetDevice(d->device));
    const size_t nb = (size_t)d->n_rows * 4;
    ARP_TRY(d->action.ensure(nb));
    ARP_TRY(d->start.ensure(nb));
    if (rtg) ARP_TRY(d->rtg.ensure(nb));
    ARP_HIP_OK(hipMemcpy(d->action.p, action, nb, hipMemcpyHostToDevice));
    ARP_HIP_OK(hipMemcpy(d->start.p, traj_start, nb, hipMemcpyHostToDevice));
    if (rtg) ARP_HIP_OK(hipMemcpy(d->rtg.p, rtg, nb, hipMemcpyHostToDevice));
    d->labels = true;
    d->has_rtg = rtg != nullptr;
    d->n_actions = n_actions;
    return 0;
}

int arp_ds_set_lut(arp_ds* d, const float* lut768) {
    if (!d || !lut768) return fail("null argument");
    ARP_HIP_OK(hipSetDevice(d->device));
    ARP_HIP_OK(hipMemcpy(d->lut.p, lut768, 3 * 256 * 4, hipMemcpyHostToDevice));
    d->has_lut = true;
    return 0;
}

int arp_ds_alloc_encodings(arp_ds* d, int tokens, int dim) {
    if (!d || tokens <= 0 || dim <= 0) return fail("bad argument");
    if (((size_t)tokens * dim) % 4) return fail("tokens * dim must be a multiple of 4 (the gather moves 16 bytes per lane)");
    ARP_HIP_OK(hipSetDevice(d->device));
    if (d->enc.p && (d->tokens != tokens || d->dim != dim)) d->enc.release();
    d->tokens = tokens;
    d->dim = dim;
    d->enc_up.assign(d->n_rows, 0);
    d->n_enc_up = 0;
    ARP_TRY(d->enc.ensure(d->enc_row() * 4 * d->n_rows));
    return 0;
}

int arp_ds_upload_encodings(arp_ds* d, int64_t row0, int64_t n, const float* f32_host) {
    if (!d || row0 < 0 || n <= 0 || row0 > d->n_rows || n > d->n_rows) return fail("bad argument");
    ARP_TRY(check_rows(d, (int)row0, (int)n, f32_host));
    if (!d->enc.p) return fail("no encodings allocated (arp_ds_alloc_encodings)");
    ARP_HIP_OK(hipSetDevice(d->device));
    ARP_HIP_OK(hipMemcpy(d->enc.as<float>() + (size_t)row0 * d->enc_row(), f32_host, (size_t)n * d->enc_row() * 4, hipMemcpyHostToDevice));
    for (int64_t r = row0; r < row0 + n; ++r)
        if (!d->enc_up[r]) { d->enc_up[r] = 1; ++d->n_enc_up; }
    return 0;
}

// Every frame through the frozen encoder into the cache: an identity gather (window 1) of at most `chunk` rows into a scratch f32 frame buffer, then
// enc_forward_on into the cache's rows.  Synchronous.  Shares the encoder's workspace with every other pass of that encoder: it must not run beside a live
// prefetcher (or a step) of a policy handle the encoder is attached to -- the caller's side of the contract (arp_amd/dataset.py refuses it).
int arp_ds_encode(arp_ds* d, arp_enc* enc, int chunk) {
    if (!d || !enc) return fail("null argument");
    int tokens = 0, width = 0, res = 0, dev = 0;
    ARP_TRY(enc_geometry(enc, &tokens, &width, &res, &dev));
    if (dev != d->device) return fail("the encoder lives on device " + std::to_string(dev) + ", the dataset on device " + std::to_string(d->device));
    if (res != d->res) return fail("the dataset's frames are " + std::to_string(d->res) + " pixels square, the encoder reads " + std::to_string(res));
    if (d->n_up != d->n_rows) return fail("only " + std::to_string(d->n_up) + " of " + std::to_string(d->n_rows) + " frame rows were uploaded");
    if (!d->has_lut) return fail("the dataset has no byte -> float table (arp_ds_set_lut)");
    if (chunk <= 0) chunk = 128;
    chunk = std::min(chunk, d->n_rows);
    if (!d->enc.p || d->tokens != tokens || d->dim != width) ARP_TRY(arp_ds_alloc_encodings(d, tokens, width));
    ARP_HIP_OK(hipSetDevice(d->device));
    ARP_HIP_OK(hipDeviceSynchronize());  // (an encode-ahead pass of a prefetcher that has just been dropped may still hold the encoder's workspace)
    if (!d->iota.p) {
        std::vector<int32_t> h(d->n_rows);
        for (int i = 0; i < d->n_rows; ++i) h[i] = i;
        ARP_TRY(d->iota.ensure((size_t)d->n_rows * 4));
        ARP_HIP_OK(hipMemcpy(d->iota.p, h.data(), (size_t)d->n_rows * 4, hipMemcpyHostToDevice));
    }
    DevBuf scratch;
    Stream st;  // a stream for the duration of this call (load time: no step runs beside it)
    ARP_TRY(scratch.ensure((size_t)chunk * d->fb * 4));
    ARP_TRY(st.create());
    int rc = 0;
    for (int r0 = 0; r0 < d->n_rows && !rc; r0 += chunk) {
        const int nb = std::min(chunk, d->n_rows - r0);
        rc = gather_impl(d, st, d->iota.as<int32_t>() + r0, nullptr, nb, 1, scratch.as<float>(), nullptr, nullptr, nullptr);
        if (!rc) rc = enc_forward_on(enc, st, scratch.as<float>(), nb, d->enc.as<float>() + (size_t)r0 * d->enc_row());
    }
    const hipError_t e = hipStreamSynchronize(st);  // (after a failure too: nothing may still read the scratch buffer when it is freed)
    if (rc) return rc;
    ARP_HIP_OK(e);
    d->enc_up.assign(d->n_rows, 1);
    d->n_enc_up = d->n_rows;
    return 0;
}

// Debug read-back of the batch B indices name: frames_out f32 [B, window, res, res, 3], action_out int32 [B, window], rtg_out f32 [B, window]
// (each may be NULL).  Synchronous, on the null stream.
int arp_ds_gather_debug(arp_ds* d, const int64_t* idx, int B, int window, float* frames_out, int32_t* action_out, float* rtg_out) {
    if (!d) return fail("null handle");
    ARP_TRY(ds_check_batch(d, idx, B, window, d->device, 0, rtg_out != nullptr, frames_out ? 0 : -1, d->res, 0, 0));
    ARP_HIP_OK(hipSetDevice(d->device));
    const size_t n = (size_t)B * window;
    std::vector<int32_t> h(idx, idx + B);
    DevBuf di, df, da, dr;  // (freed on every return; hipFree waits for the gather)
    ARP_TRY(di.ensure((size_t)B * 4));
    if (frames_out) ARP_TRY(df.ensure(n * d->fb * 4));
    if (action_out) ARP_TRY(da.ensure(n * 4));
    if (rtg_out) ARP_TRY(dr.ensure(n * 4));
    ARP_HIP_OK(hipMemcpy(di.p, h.data(), (size_t)B * 4, hipMemcpyHostToDevice));
    ARP_TRY(ds_gather_on(d, nullptr, di.as<int32_t>(), B, window, df.as<float>(), nullptr, da.as<int32_t>(), dr.as<float>()));
    if (frames_out) ARP_HIP_OK(hipMemcpy(frames_out, df.p, n * d->fb * 4, hipMemcpyDeviceToHost));
    if (action_out) ARP_HIP_OK(hipMemcpy(action_out, da.p, n * 4, hipMemcpyDeviceToHost));
    if (rtg_out) ARP_HIP_OK(hipMemcpy(rtg_out, dr.p, n * 4, hipMemcpyDeviceToHost));
    return 0;
}

// arp_ds_gather_debug for (frame, goal) pairs: goals_out f32 [B, window, res, res, 3] holds the windows of the goal rows.  Frames and goals come from the
// one pair launch (both are gathered whenever either is asked for); each output may be NULL.  Synchronous, on the null stream.
int arp_ds_gather_pairs_debug(arp_ds* d, const int64_t* idx, const int64_t* goal_idx, int B, int window, float* frames_out, float* goals_out, int32_t* action_out) {
    if (!d) return fail("null handle");
    const bool fr = frames_out || goals_out;
    ARP_TRY(ds_check_batch(d, idx, B, window, d->device, 0, false, fr ? 0 : -1, d->res, 0, 0));
    ARP_TRY(ds_check_goals(d, goal_idx, B));
    ARP_HIP_OK(hipSetDevice(d->device));
    const size_t n = (size_t)B * window;
    std::vector<int32_t> h(idx, idx + B);
    h.insert(h.end(), goal_idx, goal_idx + B);
    DevBuf di, df, dg, da;  // (freed on every return; hipFree waits for the gather)
    ARP_TRY(di.ensure((size_t)B * 8));
    if (fr) ARP_TRY(df.ensure(n * d->fb * 4));
    if (fr) ARP_TRY(dg.ensure(n * d->fb * 4));
    if (action_out) ARP_TRY(da.ensure(n * 4));
    ARP_HIP_OK(hipMemcpy(di.p, h.data(), (size_t)B * 8, hipMemcpyHostToDevice));
    ARP_TRY(ds_gather_pairs_on(d, nullptr, di.as<int32_t>(), di.as<int32_t>() + B, B, window, df.as<float>(), dg.as<float>(), da.as<int32_t>()));
    if (frames_out) ARP_HIP_OK(hipMemcpy(frames_out, df.p, n * d->fb * 4, hipMemcpyDeviceToHost));
    if (goals_out) ARP_HIP_OK(hipMemcpy(goals_out, dg.p, n * d->fb * 4, hipMemcpyDeviceToHost));
    if (action_out) ARP_HIP_OK(hipMemcpy(action_out, da.p, n * 4, hipMemcpyDeviceToHost));
    return 0;
}

// HBM the dataset holds, in bytes
int64_t arp_ds_nbytes(arp_ds* d) {
    if (!d) return 0;
    return (int64_t)(d->frames.bytes + d->action.bytes + d->rtg.bytes + d->start.bytes + d->lut.bytes + d->enc.bytes + d->iota.bytes + d->qfirst.bytes + d->qlast.bytes);
}

}  // extern "C"
