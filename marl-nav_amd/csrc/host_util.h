// host_util.h - what the host side of every entry point outside the step
// kernels shares: the formatted failure, the launch status, the overlap test,
// the failure of one step of a chained call and the policy shape check.
// Included at file scope, after <stdarg.h>, <stdio.h> and marlnav.h; what it
// defines lives in the translation unit's anonymous namespace.
#pragma once

// marlnav_step.hip: stores the message for marlnav_last_error, returns code
__attribute__((visibility("hidden"))) int marlnav_internal_fail(int code, const char *msg);

namespace {

#include "policy_limits.h"

int failf(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int failf(int code, const char *fmt, ...)
{
    char msg[400];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof(msg), fmt, ap);
    va_end(ap);
    return marlnav_internal_fail(code, msg);
}

// 0, or MARLNAV_ELAUNCH with the runtime's message for the launches enqueued so far
int launch_status()
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return marlnav_internal_fail(MARLNAV_ELAUNCH, hipGetErrorString(e));
    return 0;
}

bool overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + nb && b0 < a0 + na;
}

// step t of `who` failed inside `what` (an entry point, whose message is the
// last error, or a launch): that message, with the step named
int fail_step(const char *who, int code, int64_t t, const char *what)
{
    char inner[256];
    snprintf(inner, sizeof(inner), "%s", marlnav_last_error());
    return failf(code, "%s: step %lld, %s: %s", who, (long long)t, what, inner);
}

// P envs of A agents with rows of D inputs against H hidden units: what every
// kernel of the policy and of its gradients is built for
int check_policy_shape(const char *who, int64_t P, int A, int D, int H)
{
    if (P < 1) return failf(MARLNAV_EINVAL, "%s: num_parallel=%lld < 1", who, (long long)P);
    if (A < 2 || A > kMaxAgentsP)
        return failf(MARLNAV_EINVAL, "%s: num_agents=%d outside [2, %d]", who, A, kMaxAgentsP);
    if (H < 1 || H > kMaxHidden)
        return failf(MARLNAV_EINVAL, "%s: hidden_size=%d outside [1, %d]", who, H, kMaxHidden);
    // D = 2 + 2 O + 2 (A - 1) for an observed obstacle count O in [1, 256]
    const int twoO = D - 2 * A;
    if (twoO < 2 || (twoO & 1) || twoO > 2 * kMaxObstP)
        return failf(MARLNAV_EINVAL,
                     "%s: obs_dim=%d is not 2 + 2*O + 2*(A-1) for num_agents=%d and an O in "
                     "[1, %d]", who, D, A, kMaxObstP);
    return 0;
}

}  // namespace
