// Internal (C++) hook: the stream a labelling handle enqueues on, so that another handle can order device-side work against it with events.
#pragma once
#include <hip/hip_runtime.h>

struct arp_clip;
namespace arp {
int clip_stream_of(arp_clip* c, hipStream_t* stream, int* device);
}  // namespace arp
