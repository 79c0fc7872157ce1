// ge2e_cos_sim_labeled / ge2e_eer_counts_labeled: the evaluation side of the labelled path.  One speaker label per row,
// rows in any order; the masked index kernel (ge2e_labels.hip) has decided which rows and speakers count and left
// offsets, order and active = {n_act, r_act} on the device.  The forward half of the labelled loss needs no hand-off
// between workgroups, so a batch spreads over the chip here: two kernels, many workgroups per batch.
//   centroids  one WAVE per (batch, compact speaker k): the speaker's rows E[order[p]], p = off[k] .. off[k+1]-1, summed in
//              ascending p (the stable order: the sum's order is fixed).  SS[k] = the sum, CH[k] = the unit centroid,
//              CST[k] = {1 / |c|, m, m - 1}, spk[p] = k, col[order[p]] = k.  The row indices of up to 64 positions come
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
// n_act and r_act are clamped to [0, NA] and [0, R] where they are read, every offset to [0, r_act], every row index to
// [0, R-1], every speaker id to [0, n_act-1]: whatever the memory holds, no access leaves the buffers.
// An active row's bits depend on that row, on its speaker's rows in their order and on the other speakers' rows in their
// order: the sums have a fixed order, every output element of an MFMA is the same fmaf chain over k, and nothing looks
// at blockIdx beyond choosing the work.
#include "ge2e_labeled_eval.hpp"

#include <math.h>

#include <algorithm>

namespace ge2e {

namespace {
constexpr int kThreads = 256, kWaves = kThreads / kWave;
constexpr int kTile = 64, kWaveRows = kTile / kWaves;   // sorted positions per workgroup / per wave
constexpr int kAcc = 4;                                 // column tiles (accumulators) in flight per wave
constexpr int kMaxCentroidBlocks = 8192, kMaxRowBlocks = 1 << 20;
constexpr int CS_RN = 0, CS_M = 1, CS_M1 = 2;

typedef float v4f __attribute__((ext_vector_type(4)));

__device__ __forceinline__ v4f mfma_f32(float a, float b, v4f c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// Elements k .. k+3 of a row of `len` floats (k a multiple of 4), zero where the row is absent or ends.  `vec`: the row
// starts 16-byte aligned and len is a multiple of 4, so the four are there together or not at all.
__device__ __forceinline__ v4f load4(const float* row, int k, int len, bool row_ok, bool vec) {
    v4f v = {0.f, 0.f, 0.f, 0.f};
    if (vec) {
        if (row_ok && k < len) v = *reinterpret_cast<const v4f*>(row + k);
    } else {
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (row_ok && k + s < len) v[s] = row[k + s];
    }
    return v;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// ---- the counting epilogue, shared by the fused kernel and ge2e_eer_counts_labeled ---------------------------------
// LDS: hist [2][T+1] (false accepts, own accepts), then the T thresholds.
__device__ __forceinline__ void counting_begin(int* hist, float* thr_lds, const float* thr, int T) {
    for (int t = threadIdx.x; t < 2 * (T + 1); t += kThreads) hist[t] = 0;
    for (int t = threadIdx.x; t < T; t += kThreads) thr_lds[t] = thr[t];
    __syncthreads();
}
// v is binned by the number of thresholds below it (the first t with !(v > thr[t]); NaN: 0); bin 0 is above no threshold
__device__ __forceinline__ void count_value(float v, bool own, int* hist, const float* thr_lds, int T) {
    if (!(v > thr_lds[0])) return;   // bin 0 (most other-speaker cosines, and NaN): nothing to search, nothing to record
    int lo = 1, hi = T;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (v > thr_lds[mid]) lo = mid + 1; else hi = mid;
    }
    if (lo > 0) atomicAdd(&hist[(own ? T + 1 : 0) + lo], 1);
}
// counts[t][a] += number of recorded values whose bin is > t.  Every thread owns a run of bins; a suffix scan over the
// runs' totals (lanes, then waves), then each run from its end.  Called by all threads after a barrier.
__device__ __forceinline__ void counting_end(const int* hist, int T, int* counts, int (*wtot)[kWaves]) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int per = (T + kThreads - 1) / kThreads;
    const int lo = min(1 + (int)threadIdx.x * per, T + 1), hi = min(lo + per, T + 1);   // bins lo .. hi-1 of 1 .. T
    int own[2], suf[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        int s = 0;
        for (int u = lo; u < hi; ++u) s += hist[a * (T + 1) + u];
        own[a] = s;
        int v = s;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const int t = __shfl_down(v, d);
            if (lane + d < kWave) v += t;
        }
        suf[a] = v;                                      // this run and every later run of the wave
        if (lane == 0) wtot[a][wid] = v;
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        int run = suf[a] - own[a];
        for (int i = wid + 1; i < kWaves; ++i) run += wtot[a][i];
        for (int u = hi - 1; u >= lo; --u) {
            run += hist[a * (T + 1) + u];
            if (run) atomicAdd(&counts[(size_t)(u - 1) * 2 + a], run);
        }
    }
}

// ---- kernel 1: centroids ---------------------------------------------------------------------------------------------
// kLoss: the labelled loss's wide route (ge2e_labeled_wide.hip) runs the same kernel for its SS, CH and spk.  It keeps no
// col and no counts, and its CST is the ragged kernel's {1 / |c|, kappa, m, m - 1}: kappa where the evaluation has a
// spare word.  The sums and their order are the same in both forms.
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
        const int n_act = clampi(p.active[(size_t)bi * 2], 0, NA);
        const int r_act = clampi(p.active[(size_t)bi * 2 + 1], 0, R);
        if (k >= n_act) continue;
        const int* offs = p.off + (size_t)bi * ((size_t)p.N + 1);
        const int r0 = clampi(offs[k], 0, r_act), r1 = max(clampi(offs[k + 1], 0, r_act), r0);
        const int* ord = p.order + (size_t)bi * R;
        const float* E = p.E + (size_t)bi * R * D;
        float* SS = p.SS + ((size_t)bi * NA + k) * D;
        float* CH = p.CH + ((size_t)bi * NA + k) * D;
        const float fm = (float)(r1 - r0);

        for (int pp = r0 + lane; pp < r1; pp += kWave) {
            const int row = clampi(ord[pp], 0, R - 1);
            p.spk[(size_t)bi * R + pp] = k;
            if constexpr (!kLoss) p.col[(size_t)bi * R + row] = k;
        }
        // the sums: a lane owns 4 (vecD) or 1 element of every stretch of 256 / 64; rows in ascending position
        float sq = 0.f;
        const int stretch = vecD ? 4 * kWave : kWave;
        for (int d0 = 0; d0 < D; d0 += stretch) {
            const int d = d0 + (vecD ? 4 * lane : lane);
            const bool ok = d < D;
            v4f s = {0.f, 0.f, 0.f, 0.f};
            for (int c0 = r0; c0 < r1; c0 += kWave) {
                const int pp = c0 + lane;
                const int idx = pp < r1 ? clampi(ord[pp], 0, R - 1) : 0;   // one coalesced load for up to 64 rows
                const int cnt = min(kWave, r1 - c0);
                for (int i = 0; i < cnt; ++i) {
                    const float* er = E + (size_t)__builtin_amdgcn_readlane(idx, i) * D;
                    if (ok) {
                        if (vecD) s += *reinterpret_cast<const v4f*>(er + d);
                        else s[0] += er[d];
                    }
                }
            }
            if (ok) {
                if (vecD) {
                    *reinterpret_cast<v4f*>(SS + d) = s;
#pragma unroll
                    for (int t = 0; t < 4; ++t) { const float c = s[t] / fm; sq += c * c; }
                } else {
                    SS[d] = s[0];
                    const float c = s[0] / fm;
                    sq += c * c;
                }
            }
        }
        sq = wave_sum(sq);
        float rn, kap;
        unit_stats(sq, p.eps_cos, rn, kap);
        for (int d0 = 0; d0 < D; d0 += stretch) {   // (every lane reads back what it wrote itself)
            const int d = d0 + (vecD ? 4 * lane : lane);
            if (d < D) {
                if (vecD) {
                    const v4f s = *reinterpret_cast<const v4f*>(SS + d);
                    v4f c;
#pragma unroll
                    for (int t = 0; t < 4; ++t) c[t] = s[t] / fm * rn;
                    *reinterpret_cast<v4f*>(CH + d) = c;
                } else {
                    CH[d] = SS[d] / fm * rn;
                }
            }
        }
        if (lane == 0) {
            float* cs = p.CST + ((size_t)bi * NA + k) * 4;
            if constexpr (kLoss) { cs[0] = rn; cs[1] = kap; cs[2] = fm; cs[3] = fm - 1.f; }
            else { cs[CS_RN] = rn; cs[CS_M] = fm; cs[CS_M1] = fm - 1.f; cs[3] = 0.f; }
        }
    }
}

// ---- kernel 2: rows --------------------------------------------------------------------------------------------------
// Elements k .. k+3 of a 16-byte aligned row whose length is a multiple of 4, WITHOUT a branch: the load always happens, at
// element 0 where k is past the row, and the result is zeroed by a select.  `row` must be readable whatever `ok` says.
__device__ __forceinline__ v4f load4_always(const float* row, int k, int len, bool ok) {
    const bool in = k < len;
    const v4f v = *reinterpret_cast<const v4f*>(row + (in ? k : 0));
    const v4f z = {0.f, 0.f, 0.f, 0.f};
    return (ok && in) ? v : z;
}

// The same without the select, for the centroid side of the contraction: past the row's end the E fragment is zero, so
// whatever (finite) centroid element stands there adds nothing, and a centroid row that does not exist (its pointer is
// row 0's) only feeds output columns that the epilogue drops.  No use of the value next to the load: it can stay in flight.
__device__ __forceinline__ v4f load4_raw(const float* row, int k, int len) {
    return *reinterpret_cast<const v4f*>(row + (k < len ? k : 0));
}

// kSteps > 0: D is a multiple of 4 and at most 16 kSteps.  The wave's E fragments stay in registers over all column tiles
// and every loop over k is unrolled and free of branches, so the loads run ahead of the MFMAs that use them: the row
// fragments all at once, the centroid fragments kAhead steps ahead in a ring of registers.  (With a branch per step the
// kernel waited out one L2 round trip per 16 MFMAs; DESIGN.md 3.4e has the figures.)
// kSteps == 0: any D; a plain loop over k that loads as it goes (L1 / L2), rows and centroids alike.
template <int kSteps>
__global__ __launch_bounds__(kThreads) void labeled_eval_rows_kernel(ProblemLabeledEval p, int tiles) {
    constexpr bool kHold = kSteps > 0;
    constexpr int kAhead = kSteps < 4 ? (kSteps > 0 ? kSteps : 1) : 4;
    extern __shared__ int lds[];
    __shared__ int wtot[2][kWaves];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int l15 = lane & 15, q = lane >> 4;
    const int D = p.D, R = p.R, N = p.N, NA = p.NA;
    const int T = p.counts ? p.T : 0;
    int* hist = lds;
    float* thr_lds = reinterpret_cast<float*>(lds + 2 * (T + 1));
    const bool vecD = (D & 3) == 0;
    const bool vecN = p.cos && (N & 3) == 0 && ((uintptr_t)p.cos & 15) == 0;
    [[maybe_unused]] const int steps = (D + 15) >> 4;
    const float eps = p.eps, eps_cos = p.eps_cos;
    const v4f zero4 = {0.f, 0.f, 0.f, 0.f};

    const long long items = (long long)p.B * tiles;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int bi = (int)(item / tiles), tile = (int)(item - (long long)bi * tiles);
        const int n_act = clampi(p.active[(size_t)bi * 2], 0, NA);       // the same two words for every thread
        const int r_act = clampi(p.active[(size_t)bi * 2 + 1], 0, R);
        const int* ord = p.order + (size_t)bi * R;
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
            const int row = clampi(ord[pp], 0, R - 1);
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
            // ---- row norms and the leave-one-out cosine from the explicit difference SS[j] - e_r, all 16 rows at once: the
            // lane's row is position p0 + l15 (index, speaker and m - 1 come with one load each for the whole wave, no
            // dependent chain per row), lane group q holds the elements d0 + 4 q .. + 3 of every step -- the MFMA's own
            // fragments -- and the four groups' partial sums meet through two lane swaps, in a fixed order.  The lanes
            // past the wave's last row point at its first one (an active row: readable) and zero what they load ----
            const bool row_ok = l15 < nrow;
            const int my_pp = p0 + (row_ok ? l15 : 0);
            const int my_row = clampi(ord[my_pp], 0, R - 1);
            const int sp = clampi(p.spk[(size_t)bi * R + my_pp], 0, n_act - 1);
            const int my_j = row_ok ? sp : -1;
            const float fm1 = CSTb[(size_t)sp * 4 + CS_M1];
            const float* pe = E + (size_t)my_row * D;
            const float* ps = SSb + (size_t)sp * D;
            float* cr = cosb ? cosb + (size_t)my_row * N : nullptr;
            [[maybe_unused]] v4f eh[kHold ? kSteps : 1];
            float ee = 0.f, uu = 0.f, eu = 0.f;
            auto row_step = [&](const v4f& sj, const v4f& e) {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float u = (sj[t] - e[t]) / fm1;
                    ee += e[t] * e[t]; uu += u * u; eu += e[t] * u;
                }
            };
            if constexpr (kHold) {
                v4f sh[kSteps];
#pragma unroll
                for (int s = 0; s < kSteps; ++s) eh[s] = load4_always(pe, 16 * s + 4 * q, D, row_ok);
#pragma unroll
                for (int s = 0; s < kSteps; ++s) sh[s] = load4_always(ps, 16 * s + 4 * q, D, row_ok);
#pragma unroll
                for (int s = 0; s < kSteps; ++s) row_step(sh[s], eh[s]);
            } else {
                for (int s = 0; s < steps; ++s)
                    row_step(load4(ps, 16 * s + 4 * q, D, row_ok, vecD), load4(pe, 16 * s + 4 * q, D, row_ok, vecD));
            }
            float part[3] = {ee, uu, eu};
#pragma unroll
            for (int t = 0; t < 3; ++t) {   // lanes l15, l15 + 16, l15 + 32, l15 + 48: (q0 + q1) + (q2 + q3) in every lane
                auto a = GE2E_SWAP16(__float_as_uint(part[t]));
                const float h = __uint_as_float(a[0]) + __uint_as_float(a[1]);
                auto b = GE2E_SWAP32(__float_as_uint(h));
                part[t] = __uint_as_float(b[0]) + __uint_as_float(b[1]);
            }
            float my_rne, ke, rnu, ku;
            unit_stats(part[0], eps_cos, my_rne, ke);
            unit_stats(part[1], eps_cos, rnu, ku);
            const float my_cosd = part[2] * my_rne * rnu;
            // ---- cos tiles on the matrix core: unit centroids x rows, K = D; kAcc column tiles at a time ----
            const int KT = (n_act + 15) >> 4;
            for (int kt0 = 0; kt0 < KT; kt0 += kAcc) {
                v4f acc[kAcc];
                const float* pc[kAcc];
                bool c_ok[kAcc];
#pragma unroll
                for (int a = 0; a < kAcc; ++a) {
                    const int kb = (kt0 + a) * 16 + l15;
                    acc[a] = zero4;
                    c_ok[a] = kb < n_act;
                    pc[a] = CHb + (size_t)(c_ok[a] ? kb : 0) * D;
                }
                if constexpr (kHold) {
                    v4f ring[kAhead][kAcc];
#pragma unroll
                    for (int s = 0; s < kAhead; ++s)
#pragma unroll
                        for (int a = 0; a < kAcc; ++a) ring[s][a] = load4_raw(pc[a], 16 * s + 4 * q, D);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int s = 0; s < kSteps; ++s) {
                        v4f c[kAcc];
#pragma unroll
                        for (int a = 0; a < kAcc; ++a) c[a] = ring[s % kAhead][a];
                        if (s + kAhead < kSteps) {   // (known at compile time: the loop is unrolled)
#pragma unroll
                            for (int a = 0; a < kAcc; ++a)
                                ring[s % kAhead][a] = load4_raw(pc[a], 16 * (s + kAhead) + 4 * q, D);
                        }
                        // (left alone, the scheduler sinks every load to the step that uses it and the ring is gone)
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int t = 0; t < 4; ++t)
#pragma unroll
                            for (int a = 0; a < kAcc; ++a) acc[a] = mfma_f32(c[a][t], eh[s][t], acc[a]);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                } else {
                    for (int s = 0; s < steps; ++s) {
                        const v4f e = load4(pe, 16 * s + 4 * q, D, row_ok, vecD);
                        v4f c[kAcc];
#pragma unroll
                        for (int a = 0; a < kAcc; ++a) c[a] = load4(pc[a], 16 * s + 4 * q, D, c_ok[a], vecD);
#pragma unroll
                        for (int t = 0; t < 4; ++t)
#pragma unroll
                            for (int a = 0; a < kAcc; ++a) acc[a] = mfma_f32(c[a][t], e[t], acc[a]);
                    }
                }
                // epilogue: the lane holds columns c0 .. c0+3 of row l15
#pragma unroll
                for (int a = 0; a < kAcc; ++a) {
                    const int c0 = (kt0 + a) * 16 + 4 * q;
                    if (kt0 + a >= KT || !row_ok || c0 >= N) continue;
                    v4f v;
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int c = c0 + g;
                        const bool own = c == my_j;
                        v[g] = c < n_act ? (own ? my_cosd : acc[a][g] * my_rne) + eps : 0.f;
                        if (T && c < n_act) count_value(v[g], own, hist, thr_lds, T);
                    }
                    if (cr) {
                        if (vecN) {
                            *reinterpret_cast<v4f*>(cr + c0) = v;
                        } else {
#pragma unroll
                            for (int g = 0; g < 4; ++g)
                                if (c0 + g < N) cr[c0 + g] = v[g];
                        }
                    }
                }
            }
            // the columns past the last tile of active speakers: 0
            if (cosb) {
                for (int i = 0; i < nrow; ++i) {
                    float* zr = cosb + (size_t)__builtin_amdgcn_readlane(my_row, i) * N;
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

// ---- ge2e_eer_counts_labeled -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void zero_counts_kernel(int* counts, size_t n) {
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) counts[i] = 0;
}

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
        const int n_act = clampi(active[(size_t)bi * 2], 0, N);
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
    // the register-resident forms need 16-byte row loads; D <= 64, <= 128, <= 256 (steps of 16 that only hold zeros still
    // run: at most half of them)
    const int hold = (p.D & 3) ? 0 : p.D <= 64 ? 4 : p.D <= 128 ? 8 : p.D <= 256 ? 16 : 0;
    if (hold == 4) hipLaunchKernelGGL((labeled_eval_rows_kernel<4>), dim3(grid), dim3(kThreads), lds, stream, p, tiles);
    else if (hold == 8) hipLaunchKernelGGL((labeled_eval_rows_kernel<8>), dim3(grid), dim3(kThreads), lds, stream, p, tiles);
    else if (hold == 16) hipLaunchKernelGGL((labeled_eval_rows_kernel<16>), dim3(grid), dim3(kThreads), lds, stream, p, tiles);
    else hipLaunchKernelGGL((labeled_eval_rows_kernel<0>), dim3(grid), dim3(kThreads), lds, stream, p, tiles);
    return hipGetLastError();
}

hipError_t launch_eer_counts_labeled(const float* sim, const int* col, const int* active, int B, int N, int R,
                                     const float* thr, int T, int* counts, hipStream_t stream) {
    const size_t n = (size_t)B * T * 2;
    hipLaunchKernelGGL(zero_counts_kernel, dim3((unsigned)std::min<size_t>((n + kThreads - 1) / kThreads, 1024)),
                       dim3(kThreads), 0, stream, counts, n);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    const int tiles = (R + kTile - 1) / kTile;
    const unsigned grid = (unsigned)std::min<long long>((long long)B * tiles, kMaxRowBlocks);
    hipLaunchKernelGGL(eer_counts_labeled_kernel, dim3(grid), dim3(kThreads), (size_t)(3 * T + 2) * sizeof(int), stream, sim,
                       col, active, B, N, R, thr, T, counts, tiles);
    return hipGetLastError();
}

}  // namespace ge2e
