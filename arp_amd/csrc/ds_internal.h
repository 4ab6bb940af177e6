// Internal (C++) hooks that let the policy handle fill a batch slot from a device-resident dataset (arp_ds.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct arp_ds;
namespace arp {
// What a batch of indices may read, checked on the HOST before any launch (a bad index is an error string, never an out-of-bounds gather):
// the dataset lives on `device`, labels are set (with returns-to-go if `need_rtg`), actions fit `n_actions`, every idx is in [0, n_rows), and
// either every frame row is uploaded and the frame edge is `res` (use_encodings == 0) or every encoding row is present with geometry (tokens, dim)
// (use_encodings > 0); use_encodings < 0: labels only.
int ds_check_batch(arp_ds* d, const int64_t* idx, int B, int window, int device, int n_actions, bool need_rtg, int use_encodings, int res, int tokens, int dim);
// The gathers of one batch, enqueued on `st`.  idx_dev: int32[B] in HBM.  Row of (b, t): j = max(idx[b] - (T - 1 - t), traj_start[idx[b]]).
// frames_out f32 [B*T, res, res, 3] (= lut[c][u]) or enc_out f32 [B*T, tokens*dim], whichever is non-null; action_out int32 [B*T]; rtg_out f32 [B*T] or null.
int ds_gather_on(arp_ds* d, hipStream_t st, const int32_t* idx_dev, int B, int T, float* frames_out, float* enc_out, int32_t* action_out, float* rtg_out);
// Model GCBC's (frame, goal) pairs.  ds_check_goals: every gidx in [0, n_rows), on the host, naming the batch position -- bounds only, not the hindsight rule
// (a caller may name goals from elsewhere; traj_start[g] <= g keeps the gather inside the buffer).  ds_gather_pairs_on: ONE frame-gather launch whose grid z
// selects the half -- z = 0 reads idx_dev and writes frames_out, z = 1 reads gidx_dev and writes goals_out (the window of the goal row under the same rule);
// both non-null or both null.  action_out int32 [B*T] follows idx_dev; no return-to-go.
int ds_check_goals(arp_ds* d, const int64_t* gidx, int B);
int ds_gather_pairs_on(arp_ds* d, hipStream_t st, const int32_t* idx_dev, const int32_t* gidx_dev, int B, int T, float* frames_out, float* goals_out,
                       int32_t* action_out);
// The fine-tune step's quads (arp_ft_feed_*).  ds_check_quads, on the HOST before any launch: the dataset lives on `device`, labels and quad bounds are set,
// every frame row is uploaded, the actions fit `n_actions` (every id in the table was range-checked by arp_ds_set_labels), every idx is in [0, n_rows);
// *res: the frame edge.  ds_quads_on: ONE small kernel on `st`, one lane per sample -- q = sort4(first[i], i, min(i + 1, last[i]), last[i]);
// rows_out[g * B + b] = q[g] for g < G (3 or 4; group-major), r_out[b] = q[2] == q[3] (from all four rows whatever G is), action_out[b] = action[q[0]].
int ds_check_quads(arp_ds* d, const int64_t* idx, int B, int G, int device, int n_actions, int* res);
int ds_quads_on(arp_ds* d, hipStream_t st, const int32_t* idx_dev, int B, int G, int32_t* rows_out, float* r_out, int32_t* action_out);
// the resident uint8 frames [n_rows, res, res, 3]
const uint8_t* ds_frames_of(arp_ds* d);
int ds_info(arp_ds* d, int* n_rows, int* res, int* device);
}  // namespace arp
