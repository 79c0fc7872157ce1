// Speaker labels -> the ragged kernel's offset table and row order, on the device (see ge2e_labels.hip).
#pragma once
#include "ge2e_common.hpp"

namespace ge2e {

// Speaker counts up to this keep their per-speaker counters in LDS; above it they live in the workspace, one slice of N
// int32 per workgroup of the launch (ragged_grid(B) of them).
constexpr int kLabelLdsSpeakers = 1024;

size_t label_index_workspace_bytes(int B, int N, int R);      // 0 while the counters fit LDS
// labels [B][R] -> offsets [B][N+1], order [B][R]; ws: label_index_workspace_bytes (unused, may be null, when that is 0)
hipError_t launch_label_index(const int* labels, int B, int N, int R, int* offsets, int* order, int* ws, hipStream_t stream);

// The masked form: labels of any content.  speakers [B][N], active [B][2] = {active speakers, active rows}; the same
// workspace rule.
size_t label_index_masked_workspace_bytes(int B, int N, int R);
hipError_t launch_label_index_masked(const int* labels, int B, int N, int R, int* offsets, int* order, int* speakers,
                                     int* active, int* ws, hipStream_t stream);

}  // namespace ge2e
