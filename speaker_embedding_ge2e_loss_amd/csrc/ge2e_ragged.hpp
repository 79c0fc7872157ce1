// Workspace layout + launcher of the ragged loss kernel (see ge2e_ragged.hip): every speaker has its own utterance count.
#pragma once
#include "ge2e_common.hpp"

namespace ge2e {

// Launch-time problem description of ge2e_loss_fwd_bwd_ragged.
struct ProblemRagged {
    const float* E;    // [B][R][D]: the rows of speaker j of batch bi at off[bi][j] .. off[bi][j+1]-1
    const int* off;    // [B][N+1] on the device; the caller guarantees 0 = off[0] < ... < off[N] = R, steps >= 2
    const int* order;  // [B][R] on the device or null: sorted row r is row order[r] of E, dE and per (a permutation per batch)
    const int* active; // [B][2] on the device or null: {speakers, rows} that count in each batch (with order; see NA)
    const float* w;    // device scalar (s3:16)
    const float* b;    // device scalar (s3:17)
    float* loss;       // [B]
    float* per;        // [B][R] or null
    float* dE;         // [B][R][D] or null (forward only)
    float* dw;         // [B] or null
    float* db;         // [B] or null
    float* ws;         // workspace
    int B, N, R, D;
    int NA;            // with active: the speakers the workspace slices are laid out for; N is the offset table's stride
    int variant;
    float eps_cos;     // cosine_similarity eps (1e-8)
    float eps;         // hp.general.small_err (1e-6)
    float log_eps;     // logf(eps), -inf when eps == 0
};

// Per-workgroup workspace slice, offsets in 4-byte words (spk holds int32).
struct RaggedLayout {
    size_t ch, ss, gc, dus, a, rowstat, cstat, spk, total;
};

__host__ __device__ inline RaggedLayout ragged_layout(int N, int R, int D) {
    RaggedLayout L;
    const size_t nd = align_up((size_t)N * D, 4);   // every plane starts 16-byte aligned (the slice does: total % 64 == 0)
    L.ch = 0;                                        // [N][D]  unit centroids
    L.ss = L.ch + nd;                                // [N][D]  per-speaker sums
    L.gc = L.ss + nd;                                // [N][D]  dL/d c-hat, then dL/dc
    L.dus = L.gc + nd;                               // [N][D]  per-speaker sum of dL/du (leave-one-out centroids)
    L.a = L.dus + nd;                                // [R][N]  cos, then dL/dcos with the own-speaker column zeroed
    L.rowstat = L.a + align_up((size_t)R * N, 4);    // [R][8]
    L.cstat = L.rowstat + (size_t)R * 8;             // [N][4]  1 / |c|, kappa, m_j, m_j - 1
    L.spk = L.cstat + (size_t)N * 4;                 // [R]     row -> speaker (int32)
    L.total = align_up(L.spk + (size_t)R, 64);
    return L;
}

int ragged_grid(int B);
size_t ragged_workspace_bytes(int B, int N, int R, int D);
hipError_t launch_ragged(const ProblemRagged& p, hipStream_t stream);

}  // namespace ge2e
