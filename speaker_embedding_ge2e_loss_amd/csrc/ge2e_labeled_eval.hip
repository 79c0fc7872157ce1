// ge2e_cos_sim_labeled / ge2e_eer_counts_labeled: the evaluation side of the labelled path.  One speaker label per row,
// rows in any order; the masked index kernel (ge2e_labels.hip) has decided which rows and speakers count and left
// offsets, order and active = {n_act, r_act} on the device.  The forward half of the labelled loss needs no hand-off
// between workgroups, so a batch spreads over the chip here: two kernels, many workgroups per batch.
//   centroids  one WAVE per (batch, compact speaker k): the speaker's rows E[order[p]], p = off[k] .. off[k+1]-1, summed in
//              ascending p (the stable order: the sum's order is fixed).  SS[k] = the sum, CH[k] = the unit centroid,
//              CST[k] = {1 / |c|, kappa, m, m - 1}, spk[p] = k, col[order[p]] = k.  The row indices of up to 64 positions come
//              with ONE coalesced load and are handed out with v_readlane: no dependent order[p] -> row pair per row.
//              The wave of speaker 0 zeroes the batch's counts.
//   rows       one 256-thread workgroup per (batch, tile of 64 sorted positions), 16 positions per wave.  Per row the
//              norm and the leave-one-out cosine from the explicit difference SS[j] - e_r (all 16 rows of the wave at
//              once, on the MFMA's own row fragments); then
//              CH . E^T over K = D on v_mfma_f32_16x16x4_f32 (exact fp32), column tiles of 16 speakers, four tiles =
//              four independent accumulators in flight.  Operand map (lane l, l15 = l & 15, q = l >> 4):
//              A[i = l15][k = q] = CH[kt 16 + l15][..], B[k = q][j = l15] = E[row l15][..]; result C[i = 4 q + g][j = l15]:
//              a lane ends with FOUR CONSECUTIVE COLUMNS of ONE row, one 16-byte store.  The k index is permuted the
//              same way in both operands (lane group q takes d0 + 4 q + s in step s): one 16-byte load per operand
//              and step where D % 4 == 0.  The wave's 16 rows of E are loaded once into registers (D <= 256, D % 4 == 0)
//              and stay there for every column tile; CH streams from L2, its loads four k steps ahead of the MFMAs.  Epilogue: x 1 / |e_r|, the own column replaced, + eps,
//              stored at cos[order[p]][k]; columns n_act .. N-1 and the rows order[r_act .. R) are written as 0 and
//              col = -1 there.  With counts: every value is binned as it is produced by the number of thresholds below
//              it (binary search on the fp32 table in LDS, the comparison is fp32 `>`; bin 0 counts for no threshold and
//              is not recorded), LDS histograms [2][T+1], a suffix sum, INTEGER atomics into counts: exact, so the same
//              bits every launch.  No floating-point atomics anywhere.
// The index tables are read through a batch's IndexView (ge2e_rows_dev.hpp has the contract).
// An active row's bits depend on that row, on its speaker's rows in their order and on the other speakers' rows in their
// order: the sums have a fixed order, every output element of an MFMA is the same fmaf chain over k, and nothing looks
// at blockIdx beyond choosing the work.
#include "ge2e_labeled_eval.hpp"

#include <math.h>

#include <algorithm>

#include "ge2e_counting_dev.hpp"
#include "ge2e_rows_dev.hpp"

namespace ge2e {

namespace {
using namespace tile_geom;   // kThreads, kWaves, kTile, kWaveRows, kAcc
constexpr int kMaxCentroidBlocks = 8192, kMaxRowBlocks = 1 << 20;

// (the counting epilogue -- counting_begin, count_value, counting_end -- is in ge2e_counting_dev.hpp)
static_assert(kThreads == kCountThreads, "the counting helpers are written for this workgroup");

// ---- kernel 1: centroids ---------------------------------------------------------------------------------------------
// kLoss: the labelled loss's wide route (ge2e_labeled_wide.hip) runs the same kernel for its SS, CH, CST and spk.  It keeps
// no col and no counts.  The sums and their order are the same in both forms.
template <bool kLoss>
__global__ __launch_bounds__(kThreads) void labeled_eval_centroids_kernel(ProblemLabeledEval p) {
    const int lane = threadIdx.x & 63;
    const int D = p.D, R = p.R, NA = p.NA;
    const bool vecD = (D & 3) == 0;
    const long long total = (long long)p.B * NA, nwaves = (long long)gridDim.x * kWaves;
    for (long long w = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6); w < total; w += nwaves) {
        const int bi = (int)(w / NA), k = (int)(w - (long long)bi * NA);
        if (!kLoss && k == 0 && p.counts) {
            int* c = p.counts + (size_t)bi * 2 * p.T;
            for (int t = lane; t < 2 * p.T; t += kWave) c[t] = 0;
        }
        const IndexView ix = index_view(p, bi);
        if (k >= ix.n_act) continue;
        const IndexSpan sp = ix.span(k);
        const float* E = p.E + (size_t)bi * R * D;
        float* SS = p.SS + ((size_t)bi * NA + k) * D;
        float* CH = p.CH + ((size_t)bi * NA + k) * D;
        const float fm = (float)(sp.r1 - sp.r0);

        for (int pp = sp.r0 + lane; pp < sp.r1; pp += kWave) {
            p.spk[(size_t)bi * R + pp] = k;
            if constexpr (!kLoss) p.col[(size_t)bi * R + ix.row_at(pp)] = k;
        }
        // the sums (speaker_sum, ge2e_rows_dev.hpp: rows in ascending position), stored once, and |c|^2 on the way
        float sq = 0.f;
        for (int d0 = 0; d0 < D; d0 += wave_stretch(vecD)) {
            const int d = wave_elem(d0, lane, vecD);
            const bool ok = d < D;
            const v4f s = speaker_sum(E, ix.order, sp, R, D, d, ok, vecD);
            if (ok) {
                if (vecD) *reinterpret_cast<v4f*>(SS + d) = s;
                else SS[d] = s[0];
                sq = mean_sq(sq, s, fm, vecD);
            }
        }
        sq = wave_sum(sq);
        float rn, kap;
        unit_stats(sq, p.eps_cos, rn, kap);
        unit_scale(SS, CH, D, fm, rn, vecD);   // (every lane reads back what it wrote itself)
        if (lane == 0) {
            float* cs = p.CST + ((size_t)bi * NA + k) * 4;
            cs[CS_RN] = rn; cs[CS_KAP] = kap; cs[CS_M] = fm; cs[CS_M1] = fm - 1.f;
        }
    }
}

// ---- kernel 2: rows --------------------------------------------------------------------------------------------------
// kSteps: the form of the cosine-tile stage (tile_rows and tile_cosines in ge2e_rows_dev.hpp have the reasons): > 0 with the
// wave's E fragments in registers (D a multiple of 4 and at most 16 kSteps), 0 for any D.
template <int kSteps>
__global__ __launch_bounds__(kThreads) void labeled_eval_rows_kernel(ProblemLabeledEval p, int tiles) {
    extern __shared__ int lds[];
    __shared__ int wtot[2][kWaves];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int q = lane >> 4;
    const int D = p.D, R = p.R, N = p.N, NA = p.NA;
    const int T = p.counts ? p.T : 0;
    int* hist = lds;
    float* thr_lds = reinterpret_cast<float*>(lds + 2 * (T + 1));
    const bool vecN = p.cos && (N & 3) == 0 && ((uintptr_t)p.cos & 15) == 0;
    const float eps = p.eps, eps_cos = p.eps_cos;
    const v4f zero4 = {0.f, 0.f, 0.f, 0.f};

    const long long items = (long long)p.B * tiles;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int bi = (int)(item / tiles), tile = (int)(item - (long long)bi * tiles);
        const IndexView ix = index_view(p, bi);
        const int n_act = ix.n_act, r_act = ix.r_act;
        const float* E = p.E + (size_t)bi * R * D;
        const float* CHb = p.CH + (size_t)bi * NA * D;
        const float* SSb = p.SS + (size_t)bi * NA * D;
        const float* CSTb = p.CST + (size_t)bi * NA * 4;
        float* cosb = p.cos ? p.cos + (size_t)bi * R * N : nullptr;
        const int p0 = tile * kTile + wid * kWaveRows;

        // the rows that do not count: the whole cos row is 0, col = -1 (one wave per row)
        for (int i = 0; i < kWaveRows; ++i) {
            const int pp = p0 + i;
            if (pp >= R) break;
            if (pp < r_act) continue;
            const int row = ix.row_at(pp);
            if (lane == 0) p.col[(size_t)bi * R + row] = -1;
            if (cosb) {
                float* cr = cosb + (size_t)row * N;
                if (vecN) for (int c = 4 * lane; c < N; c += 4 * kWave) *reinterpret_cast<v4f*>(cr + c) = zero4;
                else for (int c = lane; c < N; c += kWave) cr[c] = 0.f;
            }
        }
        const bool tile_active = tile * kTile < r_act && n_act > 0;   // uniform over the workgroup
        if (!tile_active) continue;
        if (T) counting_begin(hist, thr_lds, p.thr, T);

        if (p0 < r_act) {   // uniform over the wave
            const int nrow = min(kWaveRows, r_act - p0);
            // ---- row norms and the leave-one-out cosine of the wave's 16 positions (ge2e_rows_dev.hpp) ----
            const TileRows<kSteps> t = tile_rows<kSteps>(E, SSb, CSTb, ix, p0, nrow, D, eps_cos);
            float* cr = cosb ? cosb + (size_t)t.row * N : nullptr;
            // ---- cos tiles on the matrix core: unit centroids x rows, K = D; kAcc column tiles at a time ----
            const int KT = (n_act + 15) >> 4;
            tile_cosines<kSteps, kAcc>(t, CHb, n_act, D, [&](int kt0, const v4f (&acc)[kAcc]) {
                // epilogue: the lane holds columns c0 .. c0+3 of row l15
#pragma unroll
                for (int a = 0; a < kAcc; ++a) {
                    const int c0 = (kt0 + a) * 16 + 4 * q;
                    if (kt0 + a >= KT || !t.row_ok || c0 >= N) continue;
                    v4f v;
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int c = c0 + g;
                        const bool own = c == t.j;
                        v[g] = c < n_act ? (own ? t.cosd : acc[a][g] * t.rne) + eps : 0.f;
                        if (T && c < n_act) count_value(v[g], own, hist, thr_lds, T);
                    }
                    if (cr) store4(cr, c0, N, v, vecN);
                }
            });
            // the columns past the last tile of active speakers: 0
            if (cosb) {
                for (int i = 0; i < nrow; ++i) {
                    float* zr = cosb + (size_t)__builtin_amdgcn_readlane(t.row, i) * N;
                    for (int c = KT * 16 + lane; c < N; c += kWave) zr[c] = 0.f;
                }
            }
        }
        if (T) {
            __syncthreads();
            counting_end(hist, T, p.counts + (size_t)bi * 2 * T, wtot);
            __syncthreads();   // hist and wtot are reused by the workgroup's next item
        }
    }
}

// ---- the zeroing launch of every call that counts (launch_zero_ints, ge2e_counting_dev.hpp) --------------------------------
__global__ __launch_bounds__(kThreads) void zero_ints_kernel(int* a, size_t n, int* b, int nb) {
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) a[i] = 0;
    if (blockIdx.x == 0 && (int)threadIdx.x < nb) b[threadIdx.x] = 0;
}

// ---- ge2e_eer_counts_labeled -------------------------------------------------------------------------------------------

// One workgroup per (batch, tile of 64 rows in the caller's order), one wave per row, lanes over the columns < n_act.
__global__ __launch_bounds__(kThreads) void eer_counts_labeled_kernel(const float* __restrict__ sim, const int* __restrict__ col,
                                                                      const int* __restrict__ active, int B, int N, int R,
                                                                      const float* __restrict__ thr, int T, int* counts,
                                                                      int tiles) {
    extern __shared__ int lds[];
    __shared__ int wtot[2][kWaves];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int* hist = lds;
    float* thr_lds = reinterpret_cast<float*>(lds + 2 * (T + 1));
    const long long items = (long long)B * tiles;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int bi = (int)(item / tiles), tile = (int)(item - (long long)bi * tiles);
        const int n_act = index_n_act(active, (size_t)bi, N);   // (the caller's active: N is the bound)
        if (n_act == 0) continue;
        counting_begin(hist, thr_lds, thr, T);
        for (int i = wid; i < kTile; i += kWaves) {
            const int r = tile * kTile + i;
            if (r >= R) break;
            const int own = col[(size_t)bi * R + r];
            if (own < 0) continue;
            const float* sr = sim + ((size_t)bi * R + r) * N;
            for (int c0 = 0; c0 < n_act; c0 += 4 * kWave) {   // four loads in flight per lane
                float v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int c = c0 + u * kWave + lane;
                    v[u] = c < n_act ? sr[c] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int c = c0 + u * kWave + lane;
                    if (c < n_act) count_value(v[u], c == own, hist, thr_lds, T);
                }
            }
        }
        __syncthreads();
        counting_end(hist, T, counts + (size_t)bi * 2 * T, wtot);
        __syncthreads();
    }
}
}  // namespace

hipError_t launch_zero_ints(int* a, size_t n, int* b, int nb, hipStream_t stream) {
    const size_t blocks = std::min<size_t>((n + kThreads - 1) / kThreads, 1024);
    hipLaunchKernelGGL(zero_ints_kernel, dim3((unsigned)std::max<size_t>(blocks, 1)), dim3(kThreads), 0, stream, a, n, b, nb);
    return hipGetLastError();
}

hipError_t launch_labeled_centroids(const ProblemLabeledEval& p, bool loss_stats, hipStream_t stream) {
    const long long waves = (long long)p.B * p.NA;
    const long long cblocks = (waves + kWaves - 1) / kWaves;
    const dim3 grid((unsigned)std::min<long long>(cblocks, kMaxCentroidBlocks));
    if (loss_stats) hipLaunchKernelGGL(labeled_eval_centroids_kernel<true>, grid, dim3(kThreads), 0, stream, p);
    else hipLaunchKernelGGL(labeled_eval_centroids_kernel<false>, grid, dim3(kThreads), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_labeled_eval(const ProblemLabeledEval& p, hipStream_t stream) {
    hipError_t err = launch_labeled_centroids(p, false, stream);
    if (err != hipSuccess) return err;
    const int tiles = (p.R + kTile - 1) / kTile;
    const long long items = (long long)p.B * tiles;
    const unsigned grid = (unsigned)std::min<long long>(items, kMaxRowBlocks);
    const int T = p.counts ? p.T : 0;
    const size_t lds = (size_t)(3 * T + 2) * sizeof(int);
    dispatch_tile_steps(p.D, [&](auto ks) {
        hipLaunchKernelGGL((labeled_eval_rows_kernel<decltype(ks)::value>), dim3(grid), dim3(kThreads), lds, stream, p, tiles);
    });
    return hipGetLastError();
}

hipError_t launch_eer_counts_labeled(const float* sim, const int* col, const int* active, int B, int N, int R,
                                     const float* thr, int T, int* counts, hipStream_t stream) {
    hipError_t err = launch_zero_ints(counts, (size_t)B * T * 2, nullptr, 0, stream);
    if (err != hipSuccess) return err;
    const int tiles = (R + kTile - 1) / kTile;
    const unsigned grid = (unsigned)std::min<long long>((long long)B * tiles, kMaxRowBlocks);
    hipLaunchKernelGGL(eer_counts_labeled_kernel, dim3(grid), dim3(kThreads), (size_t)(3 * T + 2) * sizeof(int), stream, sim,
                       col, active, B, N, R, thr, T, counts, tiles);
    return hipGetLastError();
}

}  // namespace ge2e
