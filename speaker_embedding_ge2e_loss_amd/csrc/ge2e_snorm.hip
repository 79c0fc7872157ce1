// ge2e_cohort_stats / ge2e_verify_scores_normed: adaptive score normalisation (AS-norm) against a cohort.  A COHORT is a
// bank's finalised form, cohort [C][D] and ccnt [C]; speaker c is a MEMBER iff ccnt[c] > 0.  The score of (row, member) is
// ge2e_verify_scores' score with the same bits: tile_rows_plain / tile_cosines and the same epilogue expression.
//   rows     one 256-thread workgroup per (64 rows of a CHUNK of rows, slice of the cohort), 16 rows per wave, the verify rows
//            kernel's shape.  A chunk is a few tiles of rows (21 at C = 5 994), far fewer than the chip has CUs, and a
//            workgroup that walked the whole cohort alone set the call's time whatever the chunk held (measured: 0.9 ms per
//            chunk of 320, 1 344 or 5 568 rows alike), so the cohort axis is split as ge2e_identify splits its bank
//            (identify_split: at least 512 workgroups where the cohort has the groups for it).  An output element is the
//            same fmaf chain whatever the split.  Every score goes into the workspace [chunk][C] as a 32-bit KEY, identify's monotone map: -0 taken as +0, b ^ 0x80000000
//            for b >= 0 and ~b otherwise, 1 for a NaN (behind every number: -inf is 0x007fffff) and 0 for a column that is
//            no member, which no member's key equals.  A 16-byte store where C % 4 == 0.  Rows that are not scored are
//            neither loaded nor written.
//   select   one workgroup per row of the chunk.  A row that is not scored, or a cohort without members, gets {+0, 1}.
//            Otherwise an exact radix selection of the n-th largest key, n = min(n_top, members): four passes over eight
//            bits from the top, each an LDS histogram (integer atomics) of the keys that carry the prefix found so far, a
//            suffix scan over the 256 bins (bin t in thread t) and the one thread whose bin holds the n-th key publishing
//            bin and remainder.  With v the value of that key the n best are every key above it plus n - #{above} copies
//            of v, whichever members those are: ties need no index rule.  Then two passes in a fixed order -- thread t takes
//            the columns t, t + 256, ... ascending, the lanes meet on the wave's DPP tree, the four waves are added 0..3 --
//            the sum, mean = sum / n, and the squared deviations from that mean: the population spread, clamped from below
//            by eps_std with a comparison that a NaN does not pass.  Up to 24 keys per thread (C <= 6 144) stay in registers
//            over all six passes; above that every pass reads the row from the workspace (L2 / MALL: it was just written).
//            Both forms visit the keys in the same order: the same bits.
//   chunk    the host loops over chunks of chunk_rows(C) rows, rows then select, all on one stream and one workspace of at
//            most 32 MiB: the matrix [R][C] never exists.  A row's keys and its statistics do not depend on its chunk.
//   normed   ge2e_verify_scores' streamed rows kernel with another epilogue: v -> 0.5 ((v - mu_k) (1 / sd_k) + (v - mu_r)
//            (1 / sd_r)), every operation rounded on its own (no contraction), then stored and counted as verify does.
// No index is read from memory anywhere here: sel and ccnt are compared, never used as an offset.
#include "ge2e_snorm.hpp"

#include <math.h>

#include <algorithm>

#include "ge2e_counting_dev.hpp"
#include "ge2e_identify.hpp"
#include "ge2e_rows_dev.hpp"

namespace ge2e {

namespace {
constexpr int kThreads = 256, kWaves = kThreads / kWave;
constexpr int kTile = 64, kWaveRows = kTile / kWaves;   // rows per workgroup / per wave
constexpr int kAcc = 4;                                 // column tiles (accumulators) in flight per wave
constexpr int kMaxRowBlocks = 1 << 20;
constexpr int kBins = 256, kRadixBits = 8;
static_assert(kThreads == kCountThreads, "the counting helpers are written for this workgroup");
static_assert(kBins == kThreads, "the suffix scan gives bin t to thread t");

typedef unsigned v4u __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned make_key32(float v) {
    unsigned b = __float_as_uint(v);
    if (b == 0x80000000u) b = 0u;
    const unsigned k = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return v != v ? 1u : k;
}
__device__ __forceinline__ float key_value(unsigned k) {
    if (k == 1u) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// ---- cohort scores of a chunk of rows ---------------------------------------------------------------------------------------
// Workgroup b: tile b % tiles of the chunk's rows, slice b / tiles of the cohort (slice_models columns, a multiple of 64) --
// workgroups that run together read the same slice of the cohort.
template <int kSteps>
__global__ __launch_bounds__(kThreads) void cohort_rows_kernel(ProblemCohort p, int row0, int nrows, int tiles, int slice_models) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int l15 = lane & 15, q = lane >> 4;
    const int D = p.D, C = p.C;
    const bool vecC = (C & 3) == 0;   // (the workspace is 256-byte aligned and a row of it C keys long)
    const float eps = p.eps;
    {
        const int tile = (int)(blockIdx.x % (unsigned)tiles), slice = (int)(blockIdx.x / (unsigned)tiles);
        const int k0 = slice * slice_models;                  // (the host counts non-empty slices only: k0 < C)
        const int n_models = min(slice_models, C - k0);
        if (tile * kTile + wid * kWaveRows >= nrows) return;  // (the whole wave; waves share nothing and meet at no barrier)
        const int i = tile * kTile + wid * kWaveRows + l15;   // the row's place in the chunk
        const int r = row0 + i;
        const bool row_ok = i < nrows && (!p.sel || p.sel[r] >= p.sel_min);
        const TileRows<kSteps> t = tile_rows_plain<kSteps>(p.X, r, row_ok, D, p.eps_cos);
        unsigned* kr = p.keys + (size_t)(row_ok ? i : 0) * C;
        // epilogue: the lane holds columns c0 .. c0+3 of row l15
        auto epi = [&](int kt0, const v4f (&acc)[kAcc]) {
#pragma unroll
            for (int a = 0; a < kAcc; ++a) {
                const int c0 = k0 + (kt0 + a) * 16 + 4 * q;
                if (!row_ok || c0 >= k0 + n_models) continue;
                v4u key;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int c = c0 + g;
                    const bool member = c < C && p.ccnt[c] > 0;
                    const float v = acc[a][g] * t.rne + eps;
                    key[g] = member ? make_key32(v) : 0u;
                }
                if (vecC) {
                    *reinterpret_cast<v4u*>(kr + c0) = key;
                } else {
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        if (c0 + g < C) kr[c0 + g] = key[g];
                }
            }
        };
        tile_cosines<kSteps, kAcc>(t, p.cohort + (size_t)k0 * D, n_models, D, epi);
    }
}

// ---- the n best of a row: selection, mean, spread ------------------------------------------------------------------------------
// The sum of one value per thread, in every thread: the wave's DPP tree, then the waves 0 .. 3 in that order.
__device__ __forceinline__ float block_sum(float v, float* part) {
    v = wave_sum(v);
    __syncthreads();   // (part may still be read from the sum before)
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((part[0] + part[1]) + part[2]) + part[3];
}

// kRegs: keys per thread kept in registers (C <= kRegs * 256); 0: every pass reads the row from the workspace.
template <int kRegs>
__global__ __launch_bounds__(kThreads) void cohort_select_kernel(ProblemCohort p, int row0, int nrows) {
    __shared__ unsigned hist[kBins];
    __shared__ unsigned wtot[kWaves];
    __shared__ unsigned pick[2];
    __shared__ float part[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int C = p.C;
    for (int i = blockIdx.x; i < nrows; i += gridDim.x) {
        const int r = row0 + i;
        float* out = p.stats + (size_t)r * 2;
        const bool scored = !p.sel || p.sel[r] >= p.sel_min;   // (the whole workgroup alike)
        if (!scored) {
            if (tid < 2) out[tid] = tid ? 1.f : 0.f;
            continue;
        }
        const unsigned* krow = p.keys + (size_t)i * C;
        [[maybe_unused]] unsigned kreg[kRegs > 0 ? kRegs : 1];
        if constexpr (kRegs > 0) {
#pragma unroll
            for (int j = 0; j < kRegs; ++j) {
                const int c = j * kThreads + tid;
                kreg[j] = c < C ? krow[c] : 0u;   // (0: no member, counted nowhere)
            }
        }
        // f(key) for the thread's columns tid, tid + 256, ... in ascending order
        auto each_key = [&](auto&& f) {
            if constexpr (kRegs > 0) {
#pragma unroll
                for (int j = 0; j < kRegs; ++j) f(kreg[j]);
            } else {
                for (int c = tid; c < C; c += kThreads) f(krow[c]);
            }
        };

        unsigned prefix = 0, want = 0;
        int n = 0;
        for (int pass = 0; pass < 32 / kRadixBits; ++pass) {
            const int shift = 32 - kRadixBits * (pass + 1);
            hist[tid] = 0;
            __syncthreads();
            each_key([&](unsigned k) {
                const unsigned above = (unsigned)((unsigned long long)k >> (shift + kRadixBits));   // (pass 0: nothing above)
                if (k != 0u && above == prefix) atomicAdd(&hist[(k >> shift) & (kBins - 1)], 1u);
            });
            __syncthreads();
            const unsigned h = hist[tid];
            unsigned suf = h;                                 // the bins tid .. 255: lanes, then waves
#pragma unroll
            for (int d = 1; d < kWave; d <<= 1) {
                const unsigned o = __shfl_down(suf, d);
                if (lane + d < kWave) suf += o;
            }
            if (lane == 0) wtot[wid] = suf;
            __syncthreads();
            for (int w = wid + 1; w < kWaves; ++w) suf += wtot[w];
            if (pass == 0) {                                  // every member's key is in the first histogram
                const unsigned members = ((wtot[0] + wtot[1]) + wtot[2]) + wtot[3];
                n = (int)min((unsigned)p.n_top, members);
                want = (unsigned)n;
            }
            // the bin of the want-th largest key: at least `want` keys from it on, fewer above it
            if (n > 0 && suf >= want && suf - h < want) { pick[0] = (unsigned)tid; pick[1] = want - (suf - h); }
            __syncthreads();
            if (n == 0) break;
            prefix = (prefix << kRadixBits) | pick[0];
            want = pick[1];
        }
        if (n == 0) {   // no members
            if (tid < 2) out[tid] = tid ? 1.f : 0.f;
            continue;
        }
        const unsigned vkey = prefix;                         // the n-th largest key, taken `want` times
        const float v = key_value(vkey), fn = (float)n, copies = (float)want;
        float s = 0.f;
        each_key([&](unsigned k) { if (k > vkey) s += key_value(k); });
        const float mean = (block_sum(s, part) + copies * v) / fn;
        float d2 = 0.f;
        each_key([&](unsigned k) {
            if (k > vkey) { const float d = key_value(k) - mean; d2 += d * d; }
        });
        const float dv = v - mean;
        const float sd = sqrtf((block_sum(d2, part) + copies * (dv * dv)) / fn);
        if (tid == 0) {
            out[0] = mean;
            out[1] = sd < p.eps_std ? p.eps_std : sd;         // (a NaN stays)
        }
    }
}

// ---- normalised verification ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void snorm_zero_kernel(int* counts, int n, int* trials) {
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) counts[i] = 0;
    if (trials && blockIdx.x == 0 && threadIdx.x < 2) trials[threadIdx.x] = 0;
}

// 0.5 ((v - mu_k) rs_k + (v - mu_r) rs_r), rs = the correctly rounded 1 / sd: five roundings, nothing fused.
__device__ __forceinline__ float snorm_value(float v, float mu_k, float rs_k, float mu_r, float rs_r) {
#pragma clang fp contract(off)
    const float a = (v - mu_k) * rs_k;
    const float b = (v - mu_r) * rs_r;
    return 0.5f * (a + b);
}
__device__ __forceinline__ float snorm_recip(float sd) {
#pragma clang fp contract(off)
    return 1.0f / sd;
}

template <int kSteps>
__global__ __launch_bounds__(kThreads) void verify_normed_rows_kernel(ProblemVerifyNormed pn, int tiles) {
    extern __shared__ __attribute__((aligned(16))) int lds[];
    __shared__ int wtot[2][kWaves];
    const ProblemVerify& p = pn.v;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int l15 = lane & 15, q = lane >> 4;
    const int D = p.D, R = p.R, K = p.K;
    const int T = p.counts ? p.T : 0;
    int* hist = lds;
    float* thr_lds = reinterpret_cast<float*>(hist + 2 * (T + 1));
    const bool vecK = p.scores && (K & 3) == 0 && ((uintptr_t)p.scores & 15) == 0;
    const bool labelled = p.labels != nullptr;
    const float eps = p.eps;
    const v4f zero4 = {0.f, 0.f, 0.f, 0.f};

    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int p0 = tile * kTile + wid * kWaveRows;
        const int r = p0 + l15;
        const bool in = r < R;
        const int lab = (labelled && in) ? p.labels[r] : 0;
        const bool row_ok = in && lab >= 0;
        int tgt = -1;
        if (labelled && row_ok && lab < K && p.cnt[lab] > 0) tgt = lab;
        float mu_r = 0.f, rs_r = 1.f;   // (an ignored row's statistics are not read)
        if (row_ok) {
            mu_r = pn.row_stats[(size_t)r * 2];
            rs_r = snorm_recip(pn.row_stats[(size_t)r * 2 + 1]);
        }

        // the ignored rows: the whole score row is +0 (one wave per row; the row of E is not read)
        if (p.scores && labelled) {
            const unsigned long long okmask = __ballot(row_ok);
            for (int i = 0; i < kWaveRows && p0 + i < R; ++i) {
                if ((okmask >> i) & 1) continue;
                float* zr = p.scores + (size_t)(p0 + i) * K;
                if (vecK) for (int c = 4 * lane; c < K; c += 4 * kWave) *reinterpret_cast<v4f*>(zr + c) = zero4;
                else for (int c = lane; c < K; c += kWave) zr[c] = 0.f;
            }
        }
        if (T) counting_begin(hist, thr_lds, p.thr, T);

        const TileRows<kSteps> t = tile_rows_plain<kSteps>(p.E, r, row_ok, D, p.eps_cos);
        float* cr = p.scores ? p.scores + (size_t)t.row * K : nullptr;
        int n_imp = 0, n_tgt = 0;
        // epilogue: the lane holds columns c0 .. c0+3 of row l15
        auto epi = [&](int kt0, const v4f (&acc)[kAcc]) {
#pragma unroll
            for (int a = 0; a < kAcc; ++a) {
                const int c0 = (kt0 + a) * 16 + 4 * q;
                if (!row_ok || c0 >= K) continue;
                v4f v;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int c = c0 + g;
                    const bool enrolled = c < K && p.cnt[c] > 0;
                    v[g] = 0.f;
                    if (enrolled) {   // (the statistics of a speaker that is not enrolled are not read)
                        const float raw = acc[a][g] * t.rne + eps;
                        const float mu_k = pn.model_stats[(size_t)c * 2];
                        const float rs_k = snorm_recip(pn.model_stats[(size_t)c * 2 + 1]);
                        v[g] = snorm_value(raw, mu_k, rs_k, mu_r, rs_r);
                        if (labelled) {
                            const bool own = c == tgt;
                            if (T) count_value(v[g], own, hist, thr_lds, T);
                            if (own) ++n_tgt; else ++n_imp;
                        }
                    }
                }
                if (cr) store4(cr, c0, K, v, vecK);
            }
        };
        tile_cosines<kSteps, kAcc>(t, p.models, K, D, epi);

        if (labelled && p.trials) {   // the tallies of the wave: one integer atomic each
#pragma unroll
            for (int d = kWave / 2; d >= 1; d >>= 1) {
                n_imp += __shfl_down(n_imp, d);
                n_tgt += __shfl_down(n_tgt, d);
            }
            if (lane == 0) {
                if (n_imp) atomicAdd(&p.trials[0], n_imp);
                if (n_tgt) atomicAdd(&p.trials[1], n_tgt);
            }
        }
        if (T) {
            __syncthreads();
            counting_end(hist, T, p.counts, wtot);
            __syncthreads();   // hist and wtot are reused by the workgroup's next tile
        }
    }
}
}  // namespace

hipError_t launch_cohort_stats(const ProblemCohort& p, int chunk_rows, hipStream_t stream) {
    for (long long row0 = 0; row0 < p.R; row0 += chunk_rows) {
        const int nrows = (int)std::min<long long>(chunk_rows, p.R - row0);
        const int tiles = (nrows + kTile - 1) / kTile;
        // a chunk is a few tiles of rows: the cohort axis is split as identify splits its bank, a function of (C, rows) alone
        const IdentifySplit split = identify_split(p.C, nrows, 0);
        const unsigned grid_rows = (unsigned)((long long)tiles * split.slices);
        dispatch_tile_steps(p.D, [&](auto ks) {
            constexpr int kSteps = decltype(ks)::value;
            hipLaunchKernelGGL((cohort_rows_kernel<kSteps>), dim3(grid_rows), dim3(kThreads), 0, stream, p, (int)row0, nrows, tiles,
                               split.groups * kIdentifyGroup);
        });
        hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
        const dim3 grid((unsigned)std::min(nrows, kMaxRowBlocks));
        if (p.C <= 8 * kThreads)
            hipLaunchKernelGGL((cohort_select_kernel<8>), grid, dim3(kThreads), 0, stream, p, (int)row0, nrows);
        else if (p.C <= 24 * kThreads)
            hipLaunchKernelGGL((cohort_select_kernel<24>), grid, dim3(kThreads), 0, stream, p, (int)row0, nrows);
        else
            hipLaunchKernelGGL((cohort_select_kernel<0>), grid, dim3(kThreads), 0, stream, p, (int)row0, nrows);
        err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}

hipError_t launch_verify_scores_normed(const ProblemVerifyNormed& pn, hipStream_t stream) {
    const ProblemVerify& p = pn.v;
    const int T = p.counts ? p.T : 0;
    if (p.counts || p.trials) {
        const int n = 2 * T;
        hipLaunchKernelGGL(snorm_zero_kernel, dim3(std::max(1, std::min((n + kThreads - 1) / kThreads, 64))), dim3(kThreads), 0,
                           stream, p.counts, n, p.trials);
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    const int tiles = (p.R + kTile - 1) / kTile;
    const unsigned grid = (unsigned)std::min(tiles, kMaxRowBlocks);
    const size_t lds = (size_t)(3 * T + 2) * sizeof(int);
    dispatch_tile_steps(p.D, [&](auto ks) {
        constexpr int kSteps = decltype(ks)::value;
        hipLaunchKernelGGL((verify_normed_rows_kernel<kSteps>), dim3(grid), dim3(kThreads), lds, stream, pn, tiles);
    });
    return hipGetLastError();
}

}  // namespace ge2e
