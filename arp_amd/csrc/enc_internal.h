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
// arp_op_gemm_site's "m3ae.*" instances (the encoder's own, in this unit)
int enc_op_gemm_site(const arp_gemm_site& d);
}  // namespace arp
