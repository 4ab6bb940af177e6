// Internal (C++) hooks that let the rollout session (arp_rollout.hip) drive the policy handle's forward on data it builds on the device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct arp_dt;
struct arp_enc;
namespace arp {
struct DtRolloutInfo {
    int window, enc_tokens, enc_dim, n_actions, device, bc, gcbc;
    arp_enc* enc;         // the attached frozen encoder, or null
    hipStream_t stream;   // the handle's compute stream: everything the session enqueues for the policy goes here
};
int dt_rollout_info(arp_dt* c, DtRolloutInfo* out);
// Selects the synchronous batch slot (bt[2]) for B samples of ENCODINGS, sizes its buffers and the activations, and hands out the slot's device pointers:
// enc32 f32 [B, T, tokens, dim], action int32 [B, T], rtg f32 [B, T] (null for model BC).  Nothing is copied: the caller's kernels fill them on the handle's
// stream.  The pointers hold until the next call that stages a batch in that slot; the session asks again at every step.
int dt_rollout_bind(arp_dt* c, int B, float** enc32, int32_t** action, float** rtg);
// The forward of arp_dt_forward on the bound slot -- the same launches (eager or the handle's captured forward chain) -- enqueued, not waited for.
// *logits: f32 [B, T, n_actions] in HBM, valid behind the stream.
int dt_rollout_forward(arp_dt* c, const float** logits);
}  // namespace arp
