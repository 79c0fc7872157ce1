// Workspace layout + launchers of the labelled evaluation kernels (see ge2e_labeled_eval.hip): cosines and EER counts for
// rows in any order, one speaker label per row.
#pragma once
#include "ge2e_common.hpp"
#include "ge2e_labels.hpp"

namespace ge2e {

// Launch-time description of ge2e_cos_sim_labeled.  Every pointer is a device pointer; the index tables are those the
// masked index kernel has written earlier on the same stream.
struct ProblemLabeledEval {
    const float* E;      // [B][R][D], rows in the caller's order
    const int* off;      // [B][N+1]
    const int* order;    // [B][R]
    const int* active;   // [B][2] = {n_act, r_act}
    const float* thr;    // [T] non-decreasing, or null
    float* cos;          // [B][R][N] or null
    int* col;            // [B][R]
    int* counts;         // [B][T][2] or null
    float* CH;           // [B][NA][D] unit centroids
    float* SS;           // [B][NA][D] per-speaker sums
    float* CST;          // [B][NA][4] 1 / |c|, kappa, m, m - 1
    int* spk;            // [B][R]     sorted position -> compact speaker
    int B, N, R, D;
    int NA;              // speakers the centroid planes are laid out for: max(1, min(N, R / 2))
    int T;
    float eps_cos, eps;
};

// ge2e_cos_sim_labeled's workspace, per BATCH (no per-workgroup slices): the centroid planes for speaker_capacity(N, R)
// speakers, spk, then the index tables (ge2e_labels.hpp) with col [B][R] as their extra part; every part starts 256-byte
// aligned.
struct LabeledEvalLayout {
    size_t ch, ss, cstat, spk;   // bytes
    IndexTables t;               // t.extra: col
};
inline LabeledEvalLayout labeled_eval_layout(int B, int N, int R, int D) {
    LabeledEvalLayout L;
    const size_t NA = (size_t)speaker_capacity(N, R), b = (size_t)B;
    L.ch = 0;
    L.ss = L.ch + align_up(b * NA * D * sizeof(float), 256);
    L.cstat = L.ss + align_up(b * NA * D * sizeof(float), 256);
    L.spk = L.cstat + align_up(b * NA * 4 * sizeof(float), 256);
    L.t = index_tables(L.spk + align_up(b * R * sizeof(int), 256), B, N, R, true, b * R * sizeof(int));
    return L;
}

// The centroid kernel alone: SS, CH, CST and spk of every active speaker (and col, for the evaluation).  `loss_stats`: the
// labelled loss's wide route (ge2e_labeled_wide.hip), which reads E, off, order, active, B, N, R, D, NA, eps_cos and writes
// CH, SS, spk and CST; col and counts are not touched.
hipError_t launch_labeled_centroids(const ProblemLabeledEval& p, bool loss_stats, hipStream_t stream);
// The two kernels of ge2e_cos_sim_labeled (centroids, rows), enqueued after the index kernel.
hipError_t launch_labeled_eval(const ProblemLabeledEval& p, hipStream_t stream);
// ge2e_eer_counts_labeled: a zeroing launch, then one workgroup per (batch, tile of 64 rows).
hipError_t launch_eer_counts_labeled(const float* sim, const int* col, const int* active, int B, int N, int R,
                                     const float* thr, int T, int* counts, hipStream_t stream);

}  // namespace ge2e
