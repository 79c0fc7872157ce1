// Layout + launcher of adaptive score normalisation (see ge2e_snorm.hip): the mean and the spread of the n best cohort
// scores of every row.  (The verification scores normalised with them are ge2e_enroll.hip's rows kernel.)
#pragma once
#include <algorithm>

#include "ge2e_common.hpp"

namespace ge2e {

constexpr int kCohortMax = 65536;                        // GE2E_COHORT_MAX
// The cohort scores of one chunk of rows, [chunk][C] keys of 4 bytes: measured at 8, 32 and 128 MiB.
constexpr size_t kCohortChunkBytes = (size_t)32 << 20;

// Rows per chunk: a multiple of 64 and a function of C alone (of `want` where a test forces it: rounded up to 64 rows).
inline int cohort_chunk_rows(int C, int want) {
    if (want > 0) return (int)std::min<long long>(((long long)want + 63) / 64 * 64, 1LL << 30);
    const size_t rows = kCohortChunkBytes / ((size_t)C * sizeof(unsigned)) / 64 * 64;
    return (int)std::min<size_t>(std::max<size_t>(rows, 64), (size_t)1 << 30);
}
// The workspace: the keys of one chunk -- of all rows, rounded up to 64, where there are fewer -- and nothing else.
inline size_t cohort_workspace_bytes(int C, int R, int chunk_rows) {
    const long long rows = std::min<long long>(chunk_rows, ((long long)R + 63) / 64 * 64);
    return align_up((size_t)rows * (size_t)C * sizeof(unsigned), 256);
}

// Launch-time description of ge2e_cohort_stats.  Every pointer is a device pointer.
struct ProblemCohort {
    const float* X;        // [R][D] rows, in the caller's order
    const int* sel;        // [R] or null: a row is scored iff sel[r] >= sel_min
    const float* cohort;   // [C][D]
    const int* ccnt;       // [C]: a member iff > 0
    float* stats;          // [R][2]
    unsigned* keys;        // the workspace: [chunk][C]
    int C, R, D, n_top, sel_min;
    float eps_cos, eps, eps_std;
};
// Per chunk of rows: the rows kernel (cohort scores as keys into the workspace), the select kernel (one workgroup per row).
hipError_t launch_cohort_stats(const ProblemCohort& p, int chunk_rows, hipStream_t stream);

}  // namespace ge2e
