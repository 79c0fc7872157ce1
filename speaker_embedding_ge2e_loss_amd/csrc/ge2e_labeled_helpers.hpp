// Launchers of the labelled calc_loss helpers (see ge2e_labeled_helpers.hip): the loss of a caller-made similarity matrix
// over the rows and columns that ge2e_cos_sim_labeled found active, forward and backward.  No workspace.
#pragma once
#include "ge2e_common.hpp"

namespace ge2e {

// per [B][R] (0 on rows that do not count), then, with `loss`, a second small launch: loss [B] = the batch's sum of per.
hipError_t launch_calc_loss_labeled(const float* sim, const int* col, const int* active, int B, int N, int R, float eps,
                                    int variant, float* loss, float* per, hipStream_t stream);
// dS [B][R][N], every element written: (gloss[b] + gper[b][r]) d per_r / d sim[r][k]; a null gradient counts as 0.
hipError_t launch_calc_loss_labeled_bwd(const float* sim, const int* col, const int* active, int B, int N, int R, float eps,
                                        int variant, const float* gloss, const float* gper, float* dS, hipStream_t stream);

}  // namespace ge2e
