// Tiles, limits + launcher of ge2e_sgd_clip_step (see ge2e_optim.hip): clip by group norm, then SGD, over the trainer's flat
// gradient bucket in two launches -- the trainer step's last statements (s4:201-203).
#pragma once
#include "ge2e_common.hpp"

namespace ge2e {

constexpr int kSgdThreads = 256;
constexpr int kSgdChunk = 4096;           // elements of one segment a workgroup owns: four 16-byte pieces a thread
constexpr int kSgdMaxGroups = 8;
constexpr int kSgdFlagZeroGrad = 1, kSgdFlagSkipNonfinite = 2;

// partial [C] float: the chunks' sums of squares, written by launch 1 and read by every workgroup of launch 2
inline size_t sgd_workspace_bytes(int C) { return align_up((size_t)C * sizeof(float), 256); }

struct ProblemSgd {
    const long long* seg;         // [S][4]: parameter address, offset in the gradient bucket, numel, group; sorted by group
    const int* chunk_start;       // [S + 1]
    int S, C, G;
    float* grad;
    float* momentum;              // the gradient bucket's layout, or null
    const float* hyper;           // [G][4]: lr, max_norm, weight_decay, momentum
    float grad_scale;
    int flags;
    float* stats;                 // [G][2]: norm, coef; or null
    int* skipped;                 // or null
    float* partial;               // [C]: the workspace
};

hipError_t launch_sgd_clip_step(const ProblemSgd& p, hipStream_t stream);
// "sgd_sqsum/4096/C,sgd_update<mom|plain>/4096/C", snprintf-style.
int plan_string_sgd(int C, bool has_momentum, char* buf, size_t cap);

}  // namespace ge2e
