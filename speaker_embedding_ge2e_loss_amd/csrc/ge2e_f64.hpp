// Workspace layout + launcher of the double-precision loss kernel (see ge2e_f64.hip).
#pragma once
#include "ge2e_common.hpp"

namespace ge2e {

// Launch-time problem description of ge2e_loss_fwd_bwd_f64: the fp64 subset of Problem (no cos_out, no raw input,
// no diagnostics).
struct ProblemF64 {
    const double* E;   // [B][N][M][D]
    const double* w;   // device scalar (s3:16)
    const double* b;   // device scalar (s3:17)
    double* loss;      // [B]
    double* per;       // [B][N][M] or null
    double* dE;        // [B][N][M][D] or null (forward only)
    double* dw;        // [B] or null
    double* db;        // [B] or null
    double* ws;        // workspace
    int B, N, M, D;
    int variant;
    double eps_cos;    // cosine_similarity eps (1e-8)
    double eps;        // hp.general.small_err (1e-6)
    double log_eps;    // log(eps), -inf when eps == 0
};

// Per-workgroup workspace slice, offsets in doubles.
struct F64Layout {
    size_t ch, ss, gc, dus, a, rowstat, cstat, total;
};

__host__ __device__ inline F64Layout f64_layout(int N, int M, int D) {
    F64Layout L;
    const size_t nd = (size_t)N * D;
    L.ch = 0;                                    // [N][D]   unit centroids
    L.ss = L.ch + nd;                            // [N][D]   per-speaker sums
    L.gc = L.ss + nd;                            // [N][D]   dL/d c-hat, then dL/dc
    L.dus = L.gc + nd;                           // [N][D]   per-speaker sum of dL/du (leave-one-out centroids)
    L.a = L.dus + nd;                            // [NM][N]  cos, then dL/dcos with the diagonal zeroed
    L.rowstat = L.a + (size_t)N * M * N;         // [NM][8]
    L.cstat = L.rowstat + (size_t)N * M * 8;     // [N][2]
    L.total = align_up(L.cstat + (size_t)N * 2, 32);
    return L;
}

int f64_grid(int B);
size_t f64_workspace_bytes(int B, int N, int M, int D);
hipError_t launch_f64(const ProblemF64& p, hipStream_t stream);

}  // namespace ge2e
