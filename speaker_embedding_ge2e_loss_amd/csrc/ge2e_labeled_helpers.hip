// ge2e_calc_loss_labeled / ge2e_calc_loss_labeled_bwd: the labelled counterpart of ge2e_calc_loss / _bwd (include/ge2e_hip.h).
// The caller's sim [B][R][N] -- rows in the caller's order, column k = compact speaker k, e.g. w cos + b on what
// ge2e_cos_sim_labeled returned -- with that call's col [B][R] and active [B][2].  A row counts iff 0 <= col[r] < n_act,
// n_act = clamp(active[0], 0, N); of a counting row the columns below n_act are read, nothing else of sim is.
// One wave per row, grid-strided over all rows of all batches; the arithmetic is the row-loss step of the exact kernels
// (row_scan, row_loss in ge2e_rows_dev.hpp) with w = 1, bias = 0 and no cosine-side eps, which leaves the scores as they
// are: S_k = 1 (sim_k + 0) + 0.  Every sum has a fixed order; no atomics.
#include "ge2e_labeled_helpers.hpp"

#include <math.h>

#include <algorithm>

#include "ge2e_rows_dev.hpp"

namespace ge2e {

namespace {
constexpr int kThreads = 256, kWaves = kThreads / kWave;
constexpr int kMaxBlocks = 1 << 16;

// The row's own column, or -1 where the row does not count.
__device__ __forceinline__ int own_column(const int* col, size_t r, int n_act) {
    const int j = col[r];
    return (j >= 0 && j < n_act) ? j : -1;
}

__global__ __launch_bounds__(kThreads) void calc_loss_labeled_kernel(const float* sim, const int* col, const int* active, int B,
                                                                     int N, int R, float log_eps, int variant, float* per) {
    const int lane = threadIdx.x & 63;
    const size_t rows = (size_t)B * R, nwaves = (size_t)gridDim.x * kWaves;
    for (size_t r = (size_t)blockIdx.x * kWaves + (threadIdx.x >> 6); r < rows; r += nwaves) {
        const int n_act = index_n_act(active, r / R, N);   // (the caller's active: N is the bound)
        const int j = own_column(col, r, n_act);
        if (j < 0) {   // uniform over the wave
            if (lane == 0) per[r] = 0.f;
            continue;
        }
        float* row = const_cast<float*>(sim) + r * N;   // (row_loss stores nothing: store = false)
        float mx, best, dw = 0.f, db = 0.f;
        int besti;
        row_scan<kWave>(row, lane, n_act, j, 1.f, 0.f, 0.f, mx, best, besti);
        const RowLoss<float> rl = row_loss<kWave>(row, lane, n_act, j, row[j], 1.f, 0.f, 0.f, log_eps, variant == 1, mx, best,
                                                  besti, false, dw, db);
        if (lane == 0) per[r] = rl.per;
    }
}

// loss[b]: one wave per batch, lane l the rows l, l + 64, ... in that order (eight loads in flight per lane: a row past the
// end adds 0, which changes nothing), then the wave's fixed-order sum.
__global__ __launch_bounds__(kThreads) void calc_loss_labeled_sum_kernel(const float* per, int B, int R, float* loss) {
    constexpr int kAhead = 8;
    const int lane = threadIdx.x & 63;
    const size_t nwaves = (size_t)gridDim.x * kWaves;
    for (size_t bi = (size_t)blockIdx.x * kWaves + (threadIdx.x >> 6); bi < (size_t)B; bi += nwaves) {
        const float* pb = per + bi * R;
        float s = 0.f;
        for (int r0 = lane; r0 < R; r0 += kAhead * kWave) {
            float v[kAhead];
#pragma unroll
            for (int u = 0; u < kAhead; ++u) v[u] = r0 + u * kWave < R ? pb[r0 + u * kWave] : 0.f;
#pragma unroll
            for (int u = 0; u < kAhead; ++u) s += v[u];
        }
        s = wave_sum(s);
        if (lane == 0) loss[bi] = s;
    }
}

// d_sim: a lane copies its own columns of the row, runs the row-loss step on the copy in place (a lane reads and writes
// its own columns only), then scales; the own column's gradient comes back from row_loss as `ad`, not in the row.
__global__ __launch_bounds__(kThreads) void calc_loss_labeled_bwd_kernel(const float* sim, const int* col, const int* active,
                                                                         int B, int N, int R, float log_eps, int variant,
                                                                         const float* gloss, const float* gper, float* dS) {
    const int lane = threadIdx.x & 63;
    const size_t rows = (size_t)B * R, nwaves = (size_t)gridDim.x * kWaves;
    for (size_t r = (size_t)blockIdx.x * kWaves + (threadIdx.x >> 6); r < rows; r += nwaves) {
        const size_t bi = r / R;
        const int n_act = index_n_act(active, bi, N);
        const int j = own_column(col, r, n_act);
        float* out = dS + r * N;
        if (j < 0) {   // uniform over the wave
            for (int k = lane; k < N; k += kWave) out[k] = 0.f;
            continue;
        }
        const float* row = sim + r * N;
        const float gr = (gloss ? gloss[bi] : 0.f) + (gper ? gper[r] : 0.f);
        for (int k = lane; k < n_act; k += kWave) out[k] = row[k];
        float mx, best, dw = 0.f, db = 0.f;
        int besti;
        row_scan<kWave>(out, lane, n_act, j, 1.f, 0.f, 0.f, mx, best, besti);
        const RowLoss<float> rl = row_loss<kWave>(out, lane, n_act, j, row[j], 1.f, 0.f, 0.f, log_eps, variant == 1, mx, best,
                                                  besti, true, dw, db);
        for (int k = lane; k < N; k += kWave) out[k] = k < n_act ? gr * (k == j ? rl.ad : out[k]) : 0.f;
    }
}

unsigned blocks_for(size_t waves) {
    return (unsigned)std::max<size_t>(1, std::min<size_t>((waves + kWaves - 1) / kWaves, kMaxBlocks));
}
}  // namespace

hipError_t launch_calc_loss_labeled(const float* sim, const int* col, const int* active, int B, int N, int R, float eps,
                                    int variant, float* loss, float* per, hipStream_t stream) {
    const float log_eps = eps > 0.f ? logf(eps) : -INFINITY;
    hipLaunchKernelGGL(calc_loss_labeled_kernel, dim3(blocks_for((size_t)B * R)), dim3(kThreads), 0, stream, sim, col, active, B,
                       N, R, log_eps, variant, per);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess || !loss) return err;
    hipLaunchKernelGGL(calc_loss_labeled_sum_kernel, dim3(blocks_for((size_t)B)), dim3(kThreads), 0, stream, per, B, R, loss);
    return hipGetLastError();
}

hipError_t launch_calc_loss_labeled_bwd(const float* sim, const int* col, const int* active, int B, int N, int R, float eps,
                                        int variant, const float* gloss, const float* gper, float* dS, hipStream_t stream) {
    const float log_eps = eps > 0.f ? logf(eps) : -INFINITY;
    hipLaunchKernelGGL(calc_loss_labeled_bwd_kernel, dim3(blocks_for((size_t)B * R)), dim3(kThreads), 0, stream, sim, col, active,
                       B, N, R, log_eps, variant, gloss, gper, dS);
    return hipGetLastError();
}

}  // namespace ge2e
