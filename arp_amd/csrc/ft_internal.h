// Internal (C++) hook of a fine-tune head handle, for the rollout session that computes its rewards with it.
#pragma once

struct arp_ft;
struct arp_clip;
namespace arp {
// what arp_ft_reward_dev_async would refuse about this pair of handles before it looks at a frame: devices, geometry, a goal_conditioned head
int ft_reward_check(arp_ft* head, arp_clip* towers);
}  // namespace arp
