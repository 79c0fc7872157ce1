// Layout + launcher of speaker identification (see ge2e_identify.hip): the best k_top enrolled speakers of every trial row,
// over a bank axis that is split into slices.
#pragma once
#include "ge2e_common.hpp"

namespace ge2e {

constexpr int kIdentifyMaxTop = 32;     // GE2E_IDENTIFY_MAX_TOP
constexpr int kIdentifyGroup = 64;      // models per group of the rows kernel: a slice is a whole number of groups
// W of DESIGN.md 3.4i: the workgroups a call should at least put on the chip (two per CU of a whole MI355X; measured
// against one and four per CU, profiles/identify_bench.txt).  A constant: the split is a function of (K, R) alone.
constexpr int kIdentifyMinWorkgroups = 512;
constexpr long long kIdentifyMaxGrid = 1LL << 30;   // tiles x slices of one launch

// The split of the bank axis: `slices` non-empty slices of `groups` groups of 64 models each (the last one may be shorter).
struct IdentifySplit { int slices, groups; };
// want <= 0: the product's choice, S = clamp(ceil(W / tiles), 1, ceil(K / 64)); otherwise `want`, clamped the same way.
// Slice length ceil(ceil(K / 64) / S) groups; slices that would start past the bank are not counted.
inline IdentifySplit identify_split(int K, int R, int want) {
    const long long G = ((long long)K + kIdentifyGroup - 1) / kIdentifyGroup;
    const long long tiles = ((long long)R + 63) / 64;
    long long S = want > 0 ? want : (kIdentifyMinWorkgroups + tiles - 1) / tiles;
    S = S < 1 ? 1 : S > G ? G : S;
    if (S * tiles > kIdentifyMaxGrid) S = kIdentifyMaxGrid / tiles > 1 ? kIdentifyMaxGrid / tiles : 1;
    const long long len = (G + S - 1) / S;
    return {(int)((G + len - 1) / len), (int)len};
}
// The workspace: the partial lists [slices][R][k_top] of 64-bit keys and nothing else.
inline size_t identify_workspace_bytes(int R, int k_top, int slices) {
    return align_up((size_t)slices * (size_t)R * (size_t)k_top * sizeof(unsigned long long), 256);
}

// Launch-time description of ge2e_identify.  Every pointer is a device pointer.
struct ProblemIdentify {
    const float* E;        // [R][D] trial rows, in the caller's order
    const int* labels;     // [R] or null
    const float* models;   // [K][D]
    const int* cnt;        // [K]
    int* idx;              // [R][k_top]
    float* score;          // [R][k_top] or null
    int* rank;             // [R] or null
    int* hist;             // [k_top + 1] or null
    unsigned long long* part;   // the workspace: [slices][R][k_top]
    int K, R, D, k_top;
    float eps_cos, eps;
};
// [A zeroing launch where hist is wanted,] the rows kernel on tiles x slices workgroups, the merge kernel.
hipError_t launch_identify(const ProblemIdentify& p, IdentifySplit split, hipStream_t stream);

}  // namespace ge2e
