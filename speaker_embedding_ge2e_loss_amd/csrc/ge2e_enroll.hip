// ge2e_enroll_accumulate / ge2e_enroll_finalize / ge2e_verify_scores: enrolment and verification.  A BANK is two buffers
// of the caller's for the speaker ids 0 .. K-1, sums [K][D] float32 and cnt [K] int32; rows are taken as given (the encoder
// normalises its output), there is no batch dimension, and a trial row is never part of the model it is scored against:
// no leave-one-out anywhere.
//   accumulate  behind the masked index kernel's lone-speaker instantiation (ge2e_labels.hip: a speaker is active from ONE
//               valid row on), one WAVE per compact speaker k: the speaker's rows E[order[p]], p = off[k] .. off[k+1]-1,
//               summed from 0 in ascending p (ascending row index: the sort is stable), then ONE read-modify-write of
//               sums[speakers[k]] and cnt[speakers[k]].  The row indices of up to 64 positions come with one coalesced
//               load and are handed out with v_readlane: speaker_sum (ge2e_rows_dev.hpp), the step that
//               labeled_eval_centroids_kernel runs.  Exactly one wave touches a speaker per launch and a speaker without a
//               valid row is touched by none: no atomics, a fixed order.
//   finalize    one wave per speaker: models[s] = c / max(|c|, eps_cos), c = sums[s] / cnt[s], with the centroid kernel's
//               own steps (mean_sq, unit_stats, unit_scale: s / m * rn); +0 where cnt[s] <= 0, and sums[s] is not read there.
//   rows        one 256-thread workgroup per 64 trial rows IN THE CALLER'S ORDER (no sort, no index kernel), 16 rows per
//               wave.  Row norms on the MFMA's own row fragments (tile_rows_plain), then models . E^T over K = D on
//               v_mfma_f32_16x16x4_f32 with the operand map of ge2e_rows_dev.hpp: a lane ends with four consecutive columns
//               of one row.  Groups of 64 models (four accumulators) at a time.  Two forms of feeding the models:
//                 streamed  tile_cosines: every wave reads its model fragments from L2 itself (the evaluation kernel's way).
//                           THE PRODUCT CALL'S FORM: measured faster at K = 1 251, D = 256, R = 16 384.
//                 staged    a tile of 64 models x 64 elements of k (16 KiB) is fetched ONCE per workgroup into LDS and read
//                           by all four waves with ds_read_b128; two buffers, the next tile's global loads are issued
//                           before the current tile's MFMAs and stored after them, one barrier per tile.  A model's 16
//                           16-byte slots are stored at slot ^ (model & 15): each of ds_read_b128's lane groups (16 model
//                           rows, two neighbouring slots) then lands on 16 different slots of the 256-byte bank row.
//                           A quarter of the L2 traffic, and slower all the same (DESIGN.md 3.4h has the figures and what
//                           is supposed to cost it): reachable through ge2e_selftest_verify_form only, so that the
//                           figures can be taken again.
//               Both walk k in the same order, lane group q taking the elements 16 s + 4 q .. + 3 of step s: an output
//               element is the same fmaf chain either way, whatever its workgroup, wave or lane.
//               Epilogue: x 1 / |e_r|, + eps (raw_score, ge2e_bank_dev.hpp), 0 where cnt[k] <= 0, a 16-byte store where
//               K % 4 == 0 and scores is aligned; with counts every value of an enrolled column is binned
//               (ge2e_counting_dev.hpp) as own where k is the row's target and as impostor otherwise, and tallied in
//               trials.  Integer atomics only.
//   normed      ge2e_verify_scores_normed (AS-norm, ge2e_snorm.hip has the statistics) is the SAME rows kernel, streamed,
//               with kNormed: the score v of an enrolled column becomes 0.5 ((v - mu_k) (1 / sd_k) + (v - mu_r) (1 / sd_r)),
//               every operation rounded on its own (no contraction), and that value is stored and counted.  mu_r and
//               1 / sd_r are read once per tile and only for a scored row, model_stats[k] only for an enrolled column.
//               Everything else -- labels, targets, ignored rows, counting, tallies, barriers -- is the one text.
// Every index read from memory is clamped or range-checked where it is read (active, offsets and order through the index
// reader of ge2e_rows_dev.hpp; speakers; a label indexes cnt only after 0 <= label < K): no access leaves the buffers.
#include "ge2e_enroll.hpp"

#include <math.h>

#include <algorithm>

#include "ge2e_bank_dev.hpp"
#include "ge2e_counting_dev.hpp"

namespace ge2e {

namespace {
using namespace tile_geom;                              // kThreads, kWaves, kTile, kWaveRows, kAcc
constexpr int kGroup = 16 * kAcc;                       // models per group
constexpr int kChunk = 64;                              // elements of k per staged tile: four MFMA steps of 16
constexpr int kStageFloats = kGroup * kChunk;           // one staging buffer, 16 KiB
constexpr int kMaxSpeakerBlocks = 8192, kMaxRowBlocks = 1 << 20;
constexpr size_t kLdsLimit = 64 * 1024;                 // dynamic LDS of a launch without a function attribute
static_assert(kThreads == kCountThreads, "the counting helpers are written for this workgroup");
static_assert(kStageFloats == 4 * 4 * kThreads, "a thread fetches four 16-byte slots of a tile");

// ---- enrolment ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void enroll_accumulate_kernel(const float* __restrict__ E, const int* __restrict__ off,
                                                                      const int* __restrict__ order,
                                                                      const int* __restrict__ speakers,
                                                                      const int* __restrict__ active, int K, int R, int D,
                                                                      int NA, float* sums, int* cnt) {
    const int lane = threadIdx.x & 63;
    const bool vecD = (D & 3) == 0;
    const int nwaves = gridDim.x * kWaves;
    for (int k = blockIdx.x * kWaves + (threadIdx.x >> 6); k < NA; k += nwaves) {
        const int n_act = index_n_act(active, 0, NA);   // (one batch)
        if (k >= n_act) continue;
        const IndexSpan span = index_span(off, k, index_r_act(active, 0, R, n_act));
        if (span.r1 == span.r0) continue;
        const int sp = clampi(speakers[k], 0, K - 1);
        float* S = sums + (size_t)sp * D;
        for (int d0 = 0; d0 < D; d0 += wave_stretch(vecD)) {
            const int d = wave_elem(d0, lane, vecD);
            const bool ok = d < D;
            const v4f s = speaker_sum(E, order, span, R, D, d, ok, vecD);
            if (ok) {   // the bank takes the partial sum once
                if (vecD) *reinterpret_cast<v4f*>(S + d) = *reinterpret_cast<const v4f*>(S + d) + s;
                else S[d] = S[d] + s[0];
            }
        }
        if (lane == 0) cnt[sp] += span.r1 - span.r0;
    }
}

__global__ __launch_bounds__(kThreads) void enroll_finalize_kernel(const float* __restrict__ sums, const int* __restrict__ cnt,
                                                                    int K, int D, float eps_cos, float* __restrict__ models) {
    const int lane = threadIdx.x & 63;
    const bool vecD = (D & 3) == 0 && (((uintptr_t)sums | (uintptr_t)models) & 15) == 0;
    const int nwaves = gridDim.x * kWaves;
    const v4f zero4 = {0.f, 0.f, 0.f, 0.f};
    for (int sp = blockIdx.x * kWaves + (threadIdx.x >> 6); sp < K; sp += nwaves) {
        const int m = cnt[sp];
        const float* S = sums + (size_t)sp * D;
        float* M = models + (size_t)sp * D;
        if (m <= 0) {
            for (int d0 = 0; d0 < D; d0 += wave_stretch(vecD)) {
                const int d = wave_elem(d0, lane, vecD);
                if (d < D) {
                    if (vecD) *reinterpret_cast<v4f*>(M + d) = zero4;
                    else M[d] = 0.f;
                }
            }
            continue;
        }
        const float fm = (float)m;
        float sq = 0.f;
        for (int d0 = 0; d0 < D; d0 += wave_stretch(vecD)) {
            const int d = wave_elem(d0, lane, vecD);
            if (d < D) {
                v4f s = {0.f, 0.f, 0.f, 0.f};
                if (vecD) s = *reinterpret_cast<const v4f*>(S + d);
                else s[0] = S[d];
                sq = mean_sq(sq, s, fm, vecD);
            }
        }
        sq = wave_sum(sq);
        float rn, kap;
        unit_stats(sq, eps_cos, rn, kap);
        unit_scale(S, M, D, fm, rn, vecD);
    }
}

// ---- verification ------------------------------------------------------------------------------------------------------
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

// The slots of a staged tile: model sp (0 .. 63 of the group), 16-byte slot c (0 .. 15 of the chunk).
__device__ __forceinline__ int stage_at(int sp, int c) { return sp * kChunk + ((c ^ (sp & 15)) << 2); }

// kSteps: the form of the row fragments (ge2e_rows_dev.hpp): > 0 in registers (D a multiple of 4 and at most 16 kSteps), 0
// for any D.  kStaged: the model tiles come through LDS.  kNormed: the score is normalised with p.row_stats and
// p.model_stats before it is stored and counted (streamed form only).
template <int kSteps, bool kStaged, bool kNormed>
__global__ __launch_bounds__(kThreads) void verify_rows_kernel(ProblemVerify p, int tiles) {
    extern __shared__ __attribute__((aligned(16))) int lds[];
    __shared__ int wtot[2][kWaves];
    constexpr bool kHold = kSteps > 0;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int l15 = lane & 15, q = lane >> 4;
    const int D = p.D, R = p.R, K = p.K;
    const int T = p.counts ? p.T : 0;
    float* stage = reinterpret_cast<float*>(lds);
    int* hist = lds + (kStaged ? 2 * kStageFloats : 0);
    float* thr_lds = reinterpret_cast<float*>(hist + 2 * (T + 1));
    const bool vecK = p.scores && (K & 3) == 0 && ((uintptr_t)p.scores & 15) == 0;
    const bool vecD = (D & 3) == 0;
    const bool labelled = p.labels != nullptr;
    const float eps = p.eps;
    const v4f zero4 = {0.f, 0.f, 0.f, 0.f};
    const int G = (K + kGroup - 1) / kGroup;                         // groups of 64 models
    const int NC = kHold ? kSteps / 4 : (D + kChunk - 1) / kChunk;   // staged tiles per group

    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int p0 = tile * kTile + wid * kWaveRows;
        const int r = p0 + l15;
        const bool in = r < R;
        const int lab = (labelled && in) ? p.labels[r] : 0;
        const bool row_ok = in && lab >= 0;
        int tgt = -1;
        if (labelled && row_ok && lab < K && p.cnt[lab] > 0) tgt = lab;
        [[maybe_unused]] float mu_r = 0.f, rs_r = 1.f;   // (an ignored row's statistics are not read)
        if constexpr (kNormed) {
            if (row_ok) {
                mu_r = p.row_stats[(size_t)r * 2];
                rs_r = snorm_recip(p.row_stats[(size_t)r * 2 + 1]);
            }
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
                    v[g] = enrolled ? raw_score(acc[a][g], t.rne, eps) : 0.f;
                    if constexpr (kNormed) {   // (the statistics of a speaker that is not enrolled are not read)
                        if (enrolled)
                            v[g] = snorm_value(v[g], p.model_stats[(size_t)c * 2], snorm_recip(p.model_stats[(size_t)c * 2 + 1]),
                                               mu_r, rs_r);
                    }
                    if (labelled && enrolled) {
                        const bool own = c == tgt;
                        if (T) count_value(v[g], own, hist, thr_lds, T);
                        if (own) ++n_tgt; else ++n_imp;
                    }
                }
                if (cr) store4(cr, c0, K, v, vecK);
            }
        };

        if constexpr (!kStaged) {
            tile_cosines<kSteps, kAcc>(t, p.models, K, D, epi);
        } else {
            // a thread's four slots of a tile: slot idx = i 256 + tid, model idx / 16, 16-byte slot idx % 16
            v4f pre[4];
            auto fetch = [&](int g, int kc) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int idx = i * kThreads + (int)threadIdx.x;
                    const int m = g * kGroup + (idx >> 4);
                    const bool ok = m < K;
                    pre[i] = load4(p.models + (size_t)(ok ? m : 0) * D, kc * kChunk + 4 * (idx & 15), D, ok, vecD);
                }
            };
            auto put = [&](float* buf) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int idx = i * kThreads + (int)threadIdx.x;
                    *reinterpret_cast<v4f*>(buf + stage_at(idx >> 4, idx & 15)) = pre[i];
                }
            };
            // (the workgroup's last tile ended on a barrier behind its last read of the buffers)
            fetch(0, 0);
            put(stage);
            __syncthreads();
            int it = 0;
            for (int g = 0; g < G; ++g) {
                v4f acc[kAcc] = {zero4, zero4, zero4, zero4};
                // one staged tile: the next one's loads first, the MFMAs on this one, then the next one's stores
                auto chunk = [&](int kc, const v4f (&e)[4]) {
                    const bool last = kc + 1 == NC;
                    const bool more = !(last && g + 1 == G);
                    if (more) fetch(last ? g + 1 : g, last ? 0 : kc + 1);
                    __builtin_amdgcn_sched_barrier(0);   // (the loads stay ahead of the MFMAs)
                    const float* buf = stage + (it & 1) * kStageFloats;
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        v4f c[kAcc];
#pragma unroll
                        for (int a = 0; a < kAcc; ++a)
                            c[a] = *reinterpret_cast<const v4f*>(buf + stage_at(a * 16 + l15, 4 * s + q));
#pragma unroll
                        for (int i = 0; i < 4; ++i)
#pragma unroll
                            for (int a = 0; a < kAcc; ++a) acc[a] = mfma_f32(c[a][i], e[s][i], acc[a]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    if (more) put(stage + ((it + 1) & 1) * kStageFloats);
                    __syncthreads();
                    ++it;
                };
                if constexpr (kHold) {
#pragma unroll
                    for (int kc = 0; kc < kSteps / 4; ++kc) {
                        const v4f e[4] = {t.eh[4 * kc], t.eh[4 * kc + 1], t.eh[4 * kc + 2], t.eh[4 * kc + 3]};
                        chunk(kc, e);
                    }
                } else {
                    for (int kc = 0; kc < NC; ++kc) {
                        v4f e[4];
#pragma unroll
                        for (int s = 0; s < 4; ++s) e[s] = load4(t.pe, kc * kChunk + 16 * s + 4 * q, D, row_ok, vecD);
                        chunk(kc, e);
                    }
                }
                epi(g * kAcc, acc);
            }
        }

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

size_t verify_lds_bytes(int T, bool staged) {
    return (size_t)(3 * T + 2) * sizeof(int) + (staged ? 2 * kStageFloats * sizeof(float) : 0);
}
}  // namespace

hipError_t launch_enroll_accumulate(const float* E, const int* off, const int* order, const int* speakers, const int* active,
                                    int K, int R, int D, float* sums, int* cnt, hipStream_t stream) {
    const int NA = enroll_capacity(K, R);
    const int blocks = std::min((NA + kWaves - 1) / kWaves, kMaxSpeakerBlocks);
    hipLaunchKernelGGL(enroll_accumulate_kernel, dim3(blocks), dim3(kThreads), 0, stream, E, off, order, speakers, active, K, R,
                       D, NA, sums, cnt);
    return hipGetLastError();
}

hipError_t launch_enroll_finalize(const float* sums, const int* cnt, int K, int D, float eps_cos, float* models,
                                  hipStream_t stream) {
    const int blocks = std::min((K + kWaves - 1) / kWaves, kMaxSpeakerBlocks);
    hipLaunchKernelGGL(enroll_finalize_kernel, dim3(blocks), dim3(kThreads), 0, stream, sums, cnt, K, D, eps_cos, models);
    return hipGetLastError();
}

bool verify_staged_fits(int T) { return verify_lds_bytes(T, true) <= kLdsLimit; }

hipError_t launch_verify_scores(const ProblemVerify& p, VerifyForm form, hipStream_t stream) {
    const int T = p.counts ? p.T : 0;
    if (p.counts || p.trials) {
        const hipError_t err = launch_zero_ints(p.counts, (size_t)2 * T, p.trials, p.trials ? 2 : 0, stream);
        if (err != hipSuccess) return err;
    }
    const int tiles = (p.R + kTile - 1) / kTile;
    const unsigned grid = (unsigned)std::min(tiles, kMaxRowBlocks);
    const bool normed = p.row_stats != nullptr;
    const bool staged = form == VERIFY_STAGED && !normed && verify_staged_fits(T);
    const size_t lds = verify_lds_bytes(T, staged);
    dispatch_tile_steps(p.D, [&](auto ks) {
        constexpr int kSteps = decltype(ks)::value;
        if (normed) hipLaunchKernelGGL((verify_rows_kernel<kSteps, false, true>), dim3(grid), dim3(kThreads), lds, stream, p, tiles);
        else if (staged) hipLaunchKernelGGL((verify_rows_kernel<kSteps, true, false>), dim3(grid), dim3(kThreads), lds, stream, p, tiles);
        else hipLaunchKernelGGL((verify_rows_kernel<kSteps, false, false>), dim3(grid), dim3(kThreads), lds, stream, p, tiles);
    });
    return hipGetLastError();
}

}  // namespace ge2e
