// Internal (C++) hook that lets the policy step run the frozen encoder on its own stream.
#pragma once
#include <hip/hip_runtime.h>

struct arp_enc;
struct arp_gemm_site;
namespace arp {
// images_dev: f32 NHWC [n, res, res, 3] in HBM; out_dev: f32 [n * tokens, width].  Enqueued on `stream`.
// latency: the caller is a rollout step (a handful of frames, one pass per environment step): a call of at most arp_enc::lat_rows token rows in the plain
// 16-bit modes then runs on tower.h's latency path.  The training paths leave it false and keep their kernels at every size.
int enc_forward_on(arp_enc* e, hipStream_t stream, const float* images_dev, int n, float* out_dev, bool latency = false);
int enc_geometry(arp_enc* e, int* tokens, int* width, int* img_res, int* device);
// The goal-conditioned pass: n (frame, goal) pairs, both f32 NHWC [n, res, res, 3] in HBM -> out_dev f32 [n * (2 P + 1), width], P = (res / patch)^2: per pair the
// class token, the frame's patches, the goal frame's patches.  max_frames counts pairs here; part streams as in enc_forward_on; latency: as there, counted on
// the call's n * (2 P + 1) rows (the rollout session's pass of its E new pairs; the GCBC train step leaves it false).
int enc_forward_gc_on(arp_enc* e, hipStream_t stream, const float* images_dev, const float* goals_dev, int n, float* out_dev, bool latency = false);
int enc_gc_tokens(arp_enc* e, int* tokens);  // 2 P + 1
// The image + text pass: n frames in HBM with an instruction of L tokens -> out_dev f32 [n * (1 + P + L), width].  tok_dev: int32 ids, [L] shared by the frames or
// [n, L] (per_row); words_dev / words_host: the visible-bit words over the 1 + P + L keys, (1 + P + L + 31) / 32 per instruction, in HBM and on the host
// (enc_text_words builds them from the reference's padding mask and checks the ids against the vocabulary).  Chunks, part streams and latency as enc_forward_on.
int enc_forward_text_on(arp_enc* e, hipStream_t stream, const float* images_dev, int n, const int32_t* tok_dev, const uint32_t* words_dev, const uint32_t* words_host,
                        int L, int per_row, float* out_dev, bool latency = false);
int enc_text_words(arp_enc* e, const int32_t* tokens, const float* mask, int S, int L, uint32_t* words);
int enc_text_tokens(arp_enc* e, int L, int* tokens);  // 1 + P + L
int enc_text_prepare(arp_enc* e, int L);  // refuses what a text call of L tokens would refuse, and puts the position rows on the device (synchronous, once per L)
// arp_op_gemm_site's "m3ae.*" instances (the encoder's own, in this unit)
int enc_op_gemm_site(const arp_gemm_site& d);
}  // namespace arp
