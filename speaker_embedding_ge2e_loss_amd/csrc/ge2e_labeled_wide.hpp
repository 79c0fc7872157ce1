// Workspace layout + launcher of the labelled loss's wide route (see ge2e_labeled_wide.hip): the masked labelled loss,
// forward and backward, as a chain of many-workgroup kernels.
#pragma once
#include "ge2e_common.hpp"
#include "ge2e_labels.hpp"

namespace ge2e {

constexpr int kWideTile = 64;        // sorted positions per workgroup of the rows and dE kernels
constexpr int kWideMaxSplit = 8;     // pieces of the GC contraction's K = r_act
constexpr int kWideSplitRows = 128;  // rows per piece until there are kWideMaxSplit of them

inline int wide_tiles(int R) { return (R + kWideTile - 1) / kWideTile; }
// The number of pieces GC's K loop is cut into: a function of R alone, so the order of every sum is fixed by the shape.
inline int wide_split(int R) {
    const int s = (R + kWideSplitRows - 1) / kWideSplitRows;
    return s < 1 ? 1 : s > kWideMaxSplit ? kWideMaxSplit : s;
}
// Row length of A: the speaker capacity rounded up to a multiple of 4, so every row starts 16-byte aligned.
inline int wide_nap(int NA) { return (NA + 3) & ~3; }

// Launch-time description of ge2e_loss_fwd_bwd_labeled_wide.  Every pointer is a device pointer; off, order and active are
// what the masked index kernel has written earlier on the same stream.
struct ProblemLabeledWide {
    const float* E;      // [B][R][D], rows in the caller's order
    const int* off;      // [B][N+1]
    const int* order;    // [B][R]
    const int* active;   // [B][2] = {n_act, r_act}
    const float* w;      // device scalar
    const float* b;      // device scalar
    float* loss;         // [B]
    float* per;          // [B][R] or null
    float* dE;           // [B][R][D] or null (forward only)
    float* dw;           // [B] or null
    float* db;           // [B] or null
    float* CH;           // [B][NA][D]   unit centroids
    float* SS;           // [B][NA][D]   per-speaker sums
    float* GC;           // [B][NA][D]   dL/d c-hat, then dL/dc
    float* DUS;          // [B][NA][D]   per-speaker sum of dL/du
    float* GCP;          // [B][S][NA][D] GC's pieces, S = wide_split(R) (not there when S == 1: the one piece is GC)
    float* CST;          // [B][NA][4]   1 / |c|, kappa, m, m - 1
    float* A;            // [B][R][NAp]  cos, then dL/dcos with the own column zeroed
    float* RST;          // [B][R][8]    row statistics
    int* spk;            // [B][R]       sorted position -> compact speaker
    float* PART;         // [B][tiles][4] {loss, dw, db, -} of every tile of 64 sorted positions
    int B, N, R, D;
    int NA;              // speaker_capacity(N, R)
    int variant;
    float eps_cos, eps, log_eps;
};

// ge2e_loss_fwd_bwd_labeled_wide's workspace, per BATCH (no per-workgroup slices), byte offsets; every part starts
// 256-byte aligned.  The index tables (ge2e_labels.hpp) come last.  `partials` false: no tile partials (the cosine backward,
// which has no loss to sum).
struct LabeledWideLayout {
    size_t ch, ss, gc, dus, gcp, cstat, a, rowstat, spk, part;
    IndexTables t;
};
inline LabeledWideLayout labeled_wide_layout(int B, int N, int R, int D, bool partials = true) {
    LabeledWideLayout L;
    const size_t NA = (size_t)speaker_capacity(N, R), b = (size_t)B, f = sizeof(float);
    const size_t plane = align_up(b * NA * D * f, 256);
    const int S = wide_split(R);
    L.ch = 0;
    L.ss = L.ch + plane;
    L.gc = L.ss + plane;
    L.dus = L.gc + plane;
    L.gcp = L.dus + plane;
    L.cstat = L.gcp + (S > 1 ? align_up(b * S * NA * D * f, 256) : 0);
    L.a = L.cstat + align_up(b * NA * 4 * f, 256);
    L.rowstat = L.a + align_up(b * R * (size_t)wide_nap((int)NA) * f, 256);
    L.spk = L.rowstat + align_up(b * R * 8 * f, 256);
    L.part = L.spk + align_up(b * R * sizeof(int), 256);
    L.t = index_tables(L.part + (partials ? align_up(b * wide_tiles(R) * 4 * f, 256) : 0), B, N, R, true);
    return L;
}

// The kernels behind the index kernel: centroids, rows, sums and, with p.dE, launch_labeled_wide_backward.
hipError_t launch_labeled_wide(const ProblemLabeledWide& p, hipStream_t stream);
// The backward behind a rows kernel: GC, speakers, dE (phases C1, C2, D1) from A, RST and the centroid planes.  One copy
// for the wide loss and for ge2e_cos_sim_labeled_bwd.
hipError_t launch_labeled_wide_backward(const ProblemLabeledWide& p, hipStream_t stream);
// ge2e_cos_sim_labeled_bwd behind the index kernel: centroids, the cos-grad rows kernel (A, RS_AD and RS_COEF from the
// caller's g_cos [B][R][N] instead of a loss), launch_labeled_wide_backward.  Its workspace is labeled_wide_layout's with
// partials = false; w, b, loss, per, dw, db, PART, variant, eps and log_eps are not looked at.
hipError_t launch_labeled_cos_grad(const ProblemLabeledWide& p, const float* g_cos, hipStream_t stream);

}  // namespace ge2e
