// ge2e_identify: closed- or open-set speaker identification against a bank (models [K][D], cnt [K]; ge2e_enroll.hip): the
// best k_top enrolled speakers of every trial row, the position of the row's target among them and the histogram of those
// positions.  The score matrix [R][K] is never materialised.
//   A CANDIDATE of a scored row is an enrolled speaker k (cnt[k] > 0) with ge2e_verify_scores' score, the same fmaf chain
//   (tile_cosines on models + k0 D) and the same epilogue function (raw_score, ge2e_bank_dev.hpp).  The order of candidates is total: a stands before b
//   iff score_a > score_b as fp32 values, -0 and +0 being equal and a NaN standing behind every number; where the scores are
//   equal, or both NaN, the lower speaker index stands first.  One 64-bit KEY per candidate implements it with one unsigned
//   compare (a larger key stands first):
//     high word  score_key (ge2e_bank_dev.hpp): the score's bits made monotone (-0 taken as +0; b ^ 0x80000000 for b >= 0,
//                ~b otherwise), 1 for a NaN: -inf gives 0x007fffff, so a NaN stands behind it and in front of
//     key 0      the empty slot (index -1, score -inf), which no candidate's key equals;
//     low word   ~index: of two equal scores the lower index has the larger key.
//   A returned NaN score is the quiet NaN 0x7fc00000 and a returned -0 is +0: the key does not carry the difference.
//   rows    one 256-thread workgroup per (tile of 64 trial rows, slice of the bank), 16 rows per wave, in the verify kernel's
//           operand map: after a group of 64 models a lane holds 16 scores of ONE row.  Each row's running list, k_top keys
//           in descending order, lives in LDS (64 rows x 33 keys: 16.5 KiB; the odd stride keeps 16 rows on different
//           banks); a lane keeps the list's last key -- the threshold: 0 while the list is not full -- in registers and
//           compares every key of its own with it.  Only where some lane of the wave wins does the wave enter the insertion
//           passes: the four lanes of a row take turns (lane group q = 0 .. 3, the lanes of one group hold different rows),
//           each inserting its winners by a shift from the list's end, and every lane reads its row's threshold again
//           after each turn.  A wave owns its 16 rows: no workgroup barrier anywhere.  At the end the lists go to the
//           workspace [slice][R][k_top]; an ignored row's list is empty and its row of E is never read.
//   merge   one wave per trial row: k_top rounds of "the largest key below the last one taken" over the row's S lists
//           (keys are distinct: they carry the index), lane t keeps round t's.  Decodes idx / score, finds the target,
//           writes rank and counts it in the workgroup's LDS histogram; one integer atomic per workgroup and non-empty bin.
//           It always runs, also for S = 1: one output path.
//   zero    hist, only when hist is wanted (launch_zero_ints).
// The k_top best of the bank are among the k_top best of their slices and the order is total, so the result does not depend
// on the split; the lists' contents depend on nothing but the candidates, so it does not depend on what the workspace held.
// Every index read from memory is range-checked where it is read (a label indexes cnt only after 0 <= label < K).
#include "ge2e_identify.hpp"

#include <math.h>

#include <algorithm>

#include "ge2e_bank_dev.hpp"
#include "ge2e_counting_dev.hpp"

namespace ge2e {

namespace {
typedef unsigned long long u64;
using namespace tile_geom;                              // kThreads, kWaves, kTile, kWaveRows, kAcc
constexpr int kListStride = kIdentifyMaxTop + 1;        // keys between two rows' lists in LDS (odd: 16 rows, 16 bank pairs)
constexpr int kMaxMergeBlocks = 1024;
static_assert(16 * kAcc == kIdentifyGroup, "a slice starts on a group of the rows kernel");
static_assert(kIdentifyMaxTop <= 32, "the merge kernel reads a list with half a wave");

__device__ __forceinline__ u64 make_key(float v, int c) { return ((u64)score_key(v) << 32) | (unsigned)~c; }
__device__ __forceinline__ int key_index(u64 key) { return key ? (int)~(unsigned)key : -1; }
__device__ __forceinline__ float key_score(u64 key) {   // (the empty slot: -inf)
    const unsigned hi = (unsigned)(key >> 32);
    return hi == 0u ? -INFINITY : key_to_score(hi);
}

// key into the descending list L[0 .. k - 1] (key > L[k - 1]) -> the new last key.  One pass from the end without a branch
// on what it reads: position i takes its upper neighbour where that one is below the key, the key where only its own old
// value is, and keeps its value otherwise.  Four positions at a time: their reads are independent of each other, so one LDS
// round trip serves four.  (A shift that stops at the key's place waits out one round trip per position.)
__device__ __forceinline__ u64 list_insert(volatile u64* L, int k, u64 key) {
    int i = k - 1;
    u64 cur = L[i];                                   // the old value of position i
    for (; i >= 4; i -= 4) {
        const u64 a = L[i - 1], b = L[i - 2], c = L[i - 3], d = L[i - 4];
        L[i] = a < key ? a : (cur < key ? key : cur);
        L[i - 1] = b < key ? b : (a < key ? key : a);
        L[i - 2] = c < key ? c : (b < key ? key : b);
        L[i - 3] = d < key ? d : (c < key ? key : c);
        cur = d;
    }
    for (; i >= 1; --i) {
        const u64 prev = L[i - 1];
        L[i] = prev < key ? prev : (cur < key ? key : cur);
        cur = prev;
    }
    L[0] = cur < key ? key : cur;
    return L[k - 1];
}

// kSteps: the form of the row fragments (ge2e_rows_dev.hpp).  Workgroup b: a tile of the rows and a slice of the models
// (slice_frame, ge2e_bank_dev.hpp).
template <int kSteps>
__global__ __launch_bounds__(kThreads) void identify_rows_kernel(ProblemIdentify p, int tiles, int slice_models) {
    __shared__ u64 lists[kTile * kListStride];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int l15 = lane & 15, q = lane >> 4;
    const int D = p.D, R = p.R, K = p.K, k_top = p.k_top;
    const float eps = p.eps;
    SliceFrame f;
    if (!slice_frame(tiles, slice_models, K, R, f)) return;    // (the online case: R = 16 is one wave)
    const int slice = f.slice, k0 = f.k0, n_models = f.n_models, p0 = f.p0;
    const int r = p0 + l15;
    const bool in = r < R;
    const int lab = (p.labels && in) ? p.labels[r] : 0;
    const bool row_ok = in && lab >= 0;

    volatile u64* wave_lists = lists + wid * kWaveRows * kListStride;
    volatile u64* mine = wave_lists + l15 * kListStride;
    for (int i = lane; i < kWaveRows * kListStride; i += kWave) wave_lists[i] = 0;
    wave_lds_point();
    u64 thr = 0;

    const TileRows<kSteps> t = tile_rows_plain<kSteps>(p.E, r, row_ok, D, p.eps_cos);
    // epilogue: the lane holds columns c0 .. c0+3 of row l15, one accumulator at a time
    auto epi = [&](int kt0, const v4f (&acc)[kAcc]) {
#pragma unroll
        for (int a = 0; a < kAcc; ++a) {
            const int c0 = k0 + (kt0 + a) * 16 + 4 * q;
            u64 key[4];
            bool win = false;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = c0 + g;
                const bool cand = row_ok && c < k0 + n_models && p.cnt[c] > 0;
                key[g] = cand ? make_key(raw_score(acc[a][g], t.rne, eps), c) : 0;
                win |= key[g] > thr;
            }
            if (__ballot(win) == 0) continue;   // (the whole wave: almost always, once the lists have filled)
#pragma unroll 1
            for (int turn = 0; turn < 4; ++turn) {
                if (q == turn && win) {
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        if (key[g] > thr) thr = list_insert(mine, k_top, key[g]);
                }
                wave_lds_point();
                thr = mine[k_top - 1];
                wave_lds_point();
            }
        }
    };
    tile_cosines<kSteps, kAcc>(t, p.models + (size_t)k0 * D, n_models, D, epi);

    // the wave's 16 lists, rows p0 .. p0 + 15 of the slice's part: contiguous
    wave_lds_point();
    u64* out = p.part + ((size_t)slice * R + p0) * k_top;
    for (int e = lane; e < kWaveRows * k_top; e += kWave) {
        const int i = e / k_top, j = e - i * k_top;
        if (p0 + i < R) out[e] = wave_lists[i * kListStride + j];
    }
}

__device__ __forceinline__ u64 wave_max_key(u64 v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const u64 other = __shfl_xor(v, o);
        v = other > v ? other : v;
    }
    return v;
}

__global__ __launch_bounds__(kThreads) void identify_merge_kernel(ProblemIdentify p, int slices) {
    __shared__ int lh[kIdentifyMaxTop + 1];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int K = p.K, R = p.R, k_top = p.k_top;
    if (p.hist) {
        if ((int)threadIdx.x <= k_top) lh[threadIdx.x] = 0;
        __syncthreads();
    }
    const int j = lane & 31, s0 = lane >> 5;       // the lane's position in a list, and its first list
    for (long long row = (long long)blockIdx.x * kWaves + wid; row < R; row += (long long)gridDim.x * kWaves) {
        u64 last = ~0ull, kept = 0;
        for (int round = 0; round < k_top; ++round) {
            u64 best = 0;
            if (j < k_top)
                for (int s = s0; s < slices; s += 2) {
                    const u64 key = p.part[((size_t)s * R + (size_t)row) * k_top + j];
                    if (key < last && key > best) best = key;
                }
            best = wave_max_key(best);
            if (best == 0) break;                  // (the whole wave) the lists are exhausted: the rest stays empty
            if (lane == round) kept = best;
            last = best;
        }
        const int id = key_index(kept);
        if (lane < k_top) {
            p.idx[(size_t)row * k_top + lane] = id;
            if (p.score) p.score[(size_t)row * k_top + lane] = key_score(kept);
        }
        if (p.labels && (p.rank || p.hist)) {
            const int lab = p.labels[row];
            const bool has = lab >= 0 && lab < K && p.cnt[lab] > 0;
            const unsigned long long at = __ballot(has && lane < k_top && id == lab);
            const int rank = !has ? -1 : at ? __builtin_ctzll(at) : k_top;
            if (lane == 0) {
                if (p.rank) p.rank[row] = rank;
                if (p.hist && has) atomicAdd(&lh[rank], 1);
            }
        }
    }
    if (p.hist) {
        __syncthreads();
        if ((int)threadIdx.x <= k_top && lh[threadIdx.x]) atomicAdd(&p.hist[threadIdx.x], lh[threadIdx.x]);
    }
}
}  // namespace

hipError_t launch_identify(const ProblemIdentify& p, IdentifySplit split, hipStream_t stream) {
    if (p.hist) {
        const hipError_t err = launch_zero_ints(p.hist, (size_t)p.k_top + 1, nullptr, 0, stream);
        if (err != hipSuccess) return err;
    }
    const int tiles = (p.R + kTile - 1) / kTile;
    const unsigned grid = (unsigned)((long long)tiles * split.slices);
    const int slice_models = (int)std::min<long long>((long long)split.groups * kIdentifyGroup, 0x7fffffc0LL);   // (K near 2^31)
    dispatch_tile_steps(p.D, [&](auto ks) {
        constexpr int kSteps = decltype(ks)::value;
        hipLaunchKernelGGL((identify_rows_kernel<kSteps>), dim3(grid), dim3(kThreads), 0, stream, p, tiles, slice_models);
    });
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    const int blocks = (int)std::min<long long>(((long long)p.R + kWaves - 1) / kWaves, kMaxMergeBlocks);
    hipLaunchKernelGGL(identify_merge_kernel, dim3(blocks), dim3(kThreads), 0, stream, p, split.slices);
    return hipGetLastError();
}

}  // namespace ge2e
