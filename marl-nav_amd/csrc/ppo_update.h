// ppo_update.h - one PPO update of one minibatch as the host side describes
// it, and the two hidden functions through which marlnav_adam.hip (the update
// and phase entries) reaches marlnav_ppo.hip (the gradient launches and the
// one place that decides them: DESIGN.md §14, "The launch paths"). Included at
// file scope, after marlnav.h.
#pragma once

#include <stdint.h>

// the clipped step's own arguments
struct ClipArgs {
    double max_norm;
    double *norm_work;
    double *norm_out;  // of this update; NULL: not recorded
};

struct PpoUpdate {
    int network;  // MARLNAV_NETWORK_ACTOR / _CRITIC
    double epsilon, ent_const;
    int advantage_mode;    // the actor's
    const int32_t *steps;  // the gather table of the minibatch (§18), or NULL
    // the monitor (§17), the actor's; diag_row NULL: not monitored
    double *diag_row;  // the update's row of MARLNAV_DIAG_ROW doubles
    int64_t *stop;     // NULL: no stop
    double target_kl;
    int64_t k;  // the update's index in its phase call; 0 resets the stop
    // the optimiser; ad NULL: a gradient-only call, nothing below is read
    const MarlnavAdamDims *ad;
    const MarlnavAdamBuffers *ab;
    const ClipArgs *clip;  // NULL: no clip
    bool may_fold;         // the phases; a single-update entry never folds
};

// The dims and buffer checks of one update of `network` and nothing launched.
__attribute__((visibility("hidden"))) int marlnav_internal_ppo_validate(
    int network, int advantage_mode, const MarlnavPpoDims *d, const MarlnavPpoBuffers *b);

// The update's gradient launches, from checked arguments. *adam_owed: the
// caller still has to enqueue the Adam step (clipped and gated as the update
// says); false for a gradient-only call and where a finish launch took the step.
__attribute__((visibility("hidden"))) int marlnav_internal_ppo_enqueue(
    const PpoUpdate *u, const MarlnavPpoDims *d, const MarlnavPpoBuffers *b, void *stream,
    bool *adam_owed);
