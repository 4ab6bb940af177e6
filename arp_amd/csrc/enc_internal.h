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
// arp_op_gemm_site's "m3ae.*" instances (the encoder's own, in this unit)
int enc_op_gemm_site(const arp_gemm_site& d);
}  // namespace arp
