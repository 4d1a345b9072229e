// policy_limits.h - the limits of a policy shape: what every kernel of the
// policy and of its gradients is built for and check_policy_shape
// (host_util.h) enforces. Included inside each translation unit's anonymous
// namespace.
#pragma once

constexpr int kMaxAgentsP = 64, kMaxObstP = 256, kMaxHidden = 512;
constexpr int kMaxD = 2 * kMaxAgentsP + 2 * kMaxObstP;  // 640
