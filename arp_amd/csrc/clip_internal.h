// Internal (C++) hooks of a labelling handle: the stream it enqueues on, so that another handle can order device-side work against it with events, and the
// multi-scale export of the vision tower into buffers the handle keeps, for the fine-tune head's resident reward path (arp_ft_reward_*).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct arp_clip;
namespace arp {
int clip_stream_of(arp_clip* c, hipStream_t* stream, int* device);

struct ClipMsInfo {
    int width, layers, embed, txt_width, txt_layers, max_batch, device;
    hipStream_t stream;
};
// geometry and stream of a finalized handle (no prompt set needed)
int clip_ms_info(arp_clip* c, ClipMsInfo* out);
enum { CLIP_TF_FINETUNE = 0, CLIP_TF_LABEL = 1 };
// Everything clip_ms_enqueue needs for `nb` <= max_batch frames of H x W, allocated now: workspace, export buffers, resize plan.  Synchronises the stream
// when a buffer has to grow.  *generation changes whenever a buffer moved (a captured pass that holds the old pointers is stale); *capturable: the pass
// is a latency-size one on a handle that replays captured passes (no profiler, ARP_CLIP_GRAPH not 0).
int clip_ms_prepare(arp_clip* c, int nb, int H, int W, int use_crop, int transform, uint64_t* generation, int* capturable);
// Enqueue preprocess + vision tower for nb frames already in device memory, on the handle's stream: no copy out, no synchronisation, no allocation.
// *inter [nb, layers * width] (the per-block CLS rows) and *final_feat [nb, embed] (un-normalised) stay in the handle's buffers until its next pass.
int clip_ms_enqueue(arp_clip* c, const uint8_t* frames_dev, int nb, int H, int W, int use_crop, int transform, const float** inter, const float** final_feat);
// clip_ms_enqueue for the fine-tune transform with the frames taken through a row table from a RESIDENT set: frame f of the pass is row rows_dev[f] of the
// uint8 set [n_rows, H, W, 3] at set_base_dev (every entry a row of the set: the caller's contract).  No gathered copy of the frames, no crop buffer (use_crop
// becomes the transform's source window); same clip_ms_prepare, no allocation, copy out or synchronisation, the non-graph tower dispatch.
int clip_ms_enqueue_rows(arp_clip* c, const uint8_t* set_base_dev, const int32_t* rows_dev, int nb, int H, int W, int use_crop, const float** inter,
                         const float** final_feat);
}  // namespace arp
