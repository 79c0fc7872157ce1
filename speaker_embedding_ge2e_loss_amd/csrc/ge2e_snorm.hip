// ge2e_cohort_stats: the statistics of adaptive score normalisation (AS-norm) against a cohort.  A COHORT is a bank's
// finalised form, cohort [C][D] and ccnt [C]; speaker c is a MEMBER iff ccnt[c] > 0.  The score of (row, member) is
// ge2e_verify_scores' score with the same bits: tile_rows_plain / tile_cosines and raw_score (ge2e_bank_dev.hpp), the very
// functions the verify kernel calls.
//   rows     one 256-thread workgroup per (64 rows of a CHUNK of rows, slice of the cohort), 16 rows per wave, the verify rows
//            kernel's shape.  A chunk is a few tiles of rows (21 at C = 5 994), far fewer than the chip has CUs, and a
//            workgroup that walked the whole cohort alone set the call's time whatever the chunk held (measured: 0.9 ms per
//            chunk of 320, 1 344 or 5 568 rows alike), so the cohort axis is split as ge2e_identify splits its bank
//            (identify_split and slice_frame: at least 512 workgroups where the cohort has the groups for it).  An output
//            element is the same fmaf chain whatever the split.  Every score goes into the workspace [chunk][C] as a 32-bit
//            KEY, score_key (ge2e_bank_dev.hpp: the high word of identify's key), and 0 for a column that is no member,
//            which no member's key equals.  A 16-byte store where C % 4 == 0.  Rows that are not scored are neither
//            loaded nor written.
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
//   normed   ge2e_verify_scores_normed, which takes these statistics, is the verify rows kernel itself (ge2e_enroll.hip).
// No index is read from memory anywhere here: sel and ccnt are compared, never used as an offset.
#include "ge2e_snorm.hpp"

#include <math.h>

#include <algorithm>

#include "ge2e_bank_dev.hpp"
#include "ge2e_identify.hpp"

namespace ge2e {

namespace {
using namespace tile_geom;   // kThreads, kWaves, kTile, kWaveRows, kAcc
constexpr int kMaxRowBlocks = 1 << 20;
constexpr int kBins = 256, kRadixBits = 8;
static_assert(kBins == kThreads, "the suffix scan gives bin t to thread t");

typedef unsigned v4u __attribute__((ext_vector_type(4)));

// ---- cohort scores of a chunk of rows ---------------------------------------------------------------------------------------
// Workgroup b: a tile of the chunk's rows and a slice of the cohort (slice_frame, ge2e_bank_dev.hpp).
template <int kSteps>
__global__ __launch_bounds__(kThreads) void cohort_rows_kernel(ProblemCohort p, int row0, int nrows, int tiles, int slice_models) {
    const int lane = threadIdx.x & 63;
    const int l15 = lane & 15, q = lane >> 4;
    const int D = p.D, C = p.C;
    const bool vecC = (C & 3) == 0;   // (the workspace is 256-byte aligned and a row of it C keys long)
    const float eps = p.eps;
    {
        SliceFrame f;
        if (!slice_frame(tiles, slice_models, C, nrows, f)) return;
        const int k0 = f.k0, n_models = f.n_models;
        const int i = f.p0 + l15;                             // the row's place in the chunk
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
                    key[g] = member ? score_key(raw_score(acc[a][g], t.rne, eps)) : 0u;
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
        const float v = key_to_score(vkey), fn = (float)n, copies = (float)want;
        float s = 0.f;
        each_key([&](unsigned k) { if (k > vkey) s += key_to_score(k); });
        const float mean = (block_sum(s, part) + copies * v) / fn;
        float d2 = 0.f;
        each_key([&](unsigned k) {
            if (k > vkey) { const float d = key_to_score(k) - mean; d2 += d * d; }
        });
        const float dv = v - mean;
        const float sd = sqrtf((block_sum(d2, part) + copies * (dv * dv)) / fn);
        if (tid == 0) {
            out[0] = mean;
            out[1] = sd < p.eps_std ? p.eps_std : sd;         // (a NaN stays)
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

}  // namespace ge2e
