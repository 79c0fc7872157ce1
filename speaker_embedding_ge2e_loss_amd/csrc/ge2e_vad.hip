// ge2e_vad_flags / ge2e_vad_mask / ge2e_vad_trim: the reference's trim_long_silences (utils/audio_utils.py:107-148) between
// the gain and ge2e_melspec.  Integers from the quantiser on: every result is exact and the same on every call.
//
// ENERGY (launch 1 of ge2e_vad_flags; the only kernel that reads every sample).  A workgroup of 256 threads owns T = 16
// consecutive windows (S >= 64: G = 64 lanes a window; below, G = 8 and T = 128), group g the windows 4 g .. 4 g + 3 in turn.
// Lane l reads samples l, l + G, ... of the window (consecutive words over the lanes; an utterance starts anywhere, so a word
// at a time), quantises q = sat16(rint(fl32(fl32(x gain) 32767))) and adds q to an int32 and q^2 to an int64; a butterfly over
// the G lanes; e = S sum(q^2) - (sum q)^2 goes to the workspace.  The samples past the last whole window are never read.
// FLAG (launch 2).  A workgroup owns 256 consecutive windows and stages their energies and floor_span either side in LDS;
// thread t takes the minimum over its window's span, clipped to its own utterance, and compares
// e 256 > floor ratio_q8 in 128 bits.
// MASK.  One workgroup of 1024 threads per utterance walks its windows in chunks of 4096 with the count of kept windows
// carried: flags (64 either side) to LDS, the moving-average mask m (32 either side) to LDS, keep for four consecutive
// windows a thread, an exclusive scan over the workgroup (shuffles in the wave, the 16 wave totals through LDS).
// TRIM.  Tiled as ENERGY.  A window with dst < 0 is skipped before any of its samples is touched; a kept one is copied as
// bits, 16 bytes a lane where source and destination are both 16-byte aligned, a word a lane otherwise.
// A window finds its utterance in win_start: the last u with win_start[u] <= w (last_not_above, ge2e_common.hpp: empty
// utterances among them share their start with the next one and are passed over).
#include "ge2e_vad.hpp"

#include <stdint.h>
#include <stdio.h>

namespace ge2e {

namespace {

__device__ __forceinline__ int vad_utterance(const long long* __restrict__ win_start, int U, long long w) {
    return last_not_above(U, w, [&](int u) { return win_start[u]; });
}

// The walk of ENERGY and TRIM over the workgroup's tile: group g of G lanes takes its kVadWindowsPerGroup windows in turn.
// A window w whose rank(w) is negative is left before its utterance is looked up; body(w, u, x, lane, rank(w)) gets the
// others: window w of utterance u, whose S samples start at x.  p is taken, and captured by the bodies, by value: its fields
// are scalars read once, which no store of a body can be taken to change.
template <int G, class Rank, class Body>
__device__ __forceinline__ void vad_walk(const ProblemVad p, Rank&& rank, Body&& body) {
    constexpr int kTile = kVadThreads / G * kVadWindowsPerGroup;
    const int g = threadIdx.x / G, lane = threadIdx.x % G;
    const long long w0 = (long long)blockIdx.x * kTile + g * kVadWindowsPerGroup;
    for (int i = 0; i < kVadWindowsPerGroup; ++i) {
        const long long w = w0 + i;
        if (w >= p.total_windows) break;                    // (uniform over the group)
        const int r = rank(w);
        if (r < 0) continue;
        const int u = vad_utterance(p.win_start, p.U, w);
        body(w, u, p.wav + p.utt_start[u] + (w - p.win_start[u]) * p.S, lane, r);
    }
}

// numpy's np.round(x * g * 32767) in float32 -- two roundings, no fma -- then int16 with saturation; NaN -> 0
__device__ __forceinline__ int vad_quantise(float x, float g) {
    const float r = rintf(__fmul_rn(__fmul_rn(x, g), 32767.0f));
    if (r != r) return 0;
    return (int)fminf(fmaxf(r, -32768.0f), 32767.0f);
}

template <int G>
__global__ __launch_bounds__(kVadThreads) void vad_energy_kernel(ProblemVad p, long long* __restrict__ energy) {
    vad_walk<G>(p, [](long long) { return 0; }, [=](long long w, int u, const float* __restrict__ x, int lane, int) {
        const float gain = p.gain ? p.gain[u] : 1.0f;
        int s = 0;
        long long sq = 0;
#pragma unroll 4
        for (int j = lane; j < p.S; j += G) {
            const int q = vad_quantise(x[j], gain);
            s += q;
            sq += q * q;                                     // at most 2^30
        }
#pragma unroll
        for (int o = G / 2; o >= 1; o >>= 1) {
            s += __shfl_xor(s, o);
            sq += __shfl_xor(sq, o);
        }
        if (lane == 0) energy[w] = (long long)p.S * sq - (long long)s * s;
    });
}

__global__ __launch_bounds__(kVadThreads) void vad_flag_kernel(const long long* __restrict__ energy,
                                                                const long long* __restrict__ win_start, int U, long long total,
                                                                int span, unsigned long long ratio_q8, long long min_energy,
                                                                unsigned char* __restrict__ flags) {
    __shared__ long long e_lds[kVadFlagTile + 2 * kVadMaxSpan];
    const long long t0 = (long long)blockIdx.x * kVadFlagTile;
    const long long lo = t0 - span > 0 ? t0 - span : 0;
    const long long hi = t0 + kVadFlagTile + span < total ? t0 + kVadFlagTile + span : total;
    for (int j = threadIdx.x; j < (int)(hi - lo); j += kVadThreads) e_lds[j] = energy[lo + j];
    __syncthreads();
    const long long w = t0 + threadIdx.x;
    if (w >= total) return;
    const int u = vad_utterance(win_start, U, w);
    const long long first = win_start[u], last = win_start[u + 1] - 1;
    const long long a = w - span > first ? w - span : first, b = w + span < last ? w + span : last;
    long long fl = e_lds[a - lo];
    for (long long v = a + 1; v <= b; ++v) {
        const long long ev = e_lds[v - lo];
        fl = ev < fl ? ev : fl;
    }
    const unsigned long long e = (unsigned long long)e_lds[w - lo], f = (unsigned long long)fl;
    const unsigned long long lhi = __umul64hi(e, 256ull), llo = e * 256ull;
    const unsigned long long rhi = __umul64hi(f, ratio_q8), rlo = f * ratio_q8;
    const bool above = lhi > rhi || (lhi == rhi && llo > rlo);
    flags[w] = (unsigned char)((long long)e >= min_energy && above);
}

__global__ __launch_bounds__(kVadMaskThreads) void vad_mask_kernel(const unsigned char* __restrict__ flags,
                                                                    const long long* __restrict__ win_start, int S, int A, int n,
                                                                    int* __restrict__ dst, long long* __restrict__ out_len) {
    constexpr int kHaloM = kVadMaxWidth / 2, kHaloF = kVadMaxWidth;        // windows either side: of m, of the flags
    __shared__ unsigned char f_lds[kVadMaskChunk + 2 * kHaloF], m_lds[kVadMaskChunk + 2 * kHaloM];
    __shared__ int wave_total[kVadMaskThreads / kWave];
    const int u = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const long long first = win_start[u], W = win_start[u + 1] - first;
    const int aL = (A - 1) / 2, aR = A / 2, nL = (n - 1) / 2, nR = n / 2;
    long long carry = 0;
    for (long long c0 = 0; c0 < W; c0 += kVadMaskChunk) {
        for (int j = tid; j < kVadMaskChunk + 2 * kHaloF; j += kVadMaskThreads) {
            const long long lw = c0 - kHaloF + j;
            f_lds[j] = (lw >= 0 && lw < W) ? (unsigned char)(flags[first + lw] != 0) : (unsigned char)0;
        }
        __syncthreads();
        for (int j = tid; j < kVadMaskChunk + 2 * kHaloM; j += kVadMaskThreads) {
            const long long lw = c0 - kHaloM + j;            // its flag is f_lds[j + kHaloF - kHaloM]
            int sum = 0;
            for (int k = -aL; k <= aR; ++k) sum += f_lds[j + kHaloF - kHaloM + k];
            m_lds[j] = (unsigned char)(lw >= 0 && lw < W && 2 * sum > A);
        }
        __syncthreads();
        int keep[kVadMaskPerThread], cnt = 0;
#pragma unroll
        for (int r = 0; r < kVadMaskPerThread; ++r) {
            const int i = tid * kVadMaskPerThread + r;       // its m is m_lds[i + kHaloM]
            int any = 0;
            for (int k = -nL; k <= nR; ++k) any |= m_lds[i + kHaloM + k];
            keep[r] = (any != 0 && c0 + i < W) ? 1 : 0;
            cnt += keep[r];
        }
        int incl = cnt;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const int t = __shfl_up(incl, o);
            if (lane >= o) incl += t;
        }
        if (lane == kWave - 1) wave_total[wave] = incl;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int v = 0; v < kVadMaskThreads / kWave; ++v) {
            const int t = wave_total[v];
            before += v < wave ? t : 0;
            all += t;
        }
        long long rank = carry + before + incl - cnt;
#pragma unroll
        for (int r = 0; r < kVadMaskPerThread; ++r) {
            const long long lw = c0 + tid * kVadMaskPerThread + r;
            if (lw < W) dst[first + lw] = keep[r] ? (int)rank : -1;
            rank += keep[r];
        }
        carry += all;
        __syncthreads();                                     // the LDS arrays are written again
    }
    if (tid == 0) out_len[u] = (long long)S * carry;
}

template <int G>
__global__ __launch_bounds__(kVadThreads) void vad_trim_kernel(ProblemVad p, const int* __restrict__ dst,
                                                                const long long* __restrict__ out_start,
                                                                float* __restrict__ out) {
    // a window with dst < 0 is dropped: not a sample of it is read
    vad_walk<G>(p, [=](long long w) { return dst[w]; }, [=](long long, int u, const float* __restrict__ x, int lane, int d) {
        const unsigned* __restrict__ from = (const unsigned*)x;
        unsigned* __restrict__ to = (unsigned*)(out + out_start[u] + (long long)p.S * d);
        int done = 0;
        if ((((uintptr_t)from | (uintptr_t)to) & 15) == 0) {
            const int quads = p.S >> 2;
            for (int j = lane; j < quads; j += G) ((uint4*)to)[j] = ((const uint4*)from)[j];
            done = quads << 2;
        }
        for (int j = done + lane; j < p.S; j += G) to[j] = from[j];
    });
}

// ENERGY and TRIM have one tiling: the instantiation for the window's lane group over vad_tile(S) windows a workgroup.
template <class... Args>
hipError_t launch_walk(void (*k64)(ProblemVad, Args...), void (*k8)(ProblemVad, Args...), const ProblemVad& p,
                       hipStream_t stream, Args... args) {
    const long long grid = vad_grid(p.total_windows, vad_tile(p.S));
    hipLaunchKernelGGL(vad_group(p.S) == 64 ? k64 : k8, dim3((unsigned)grid), dim3(kVadThreads), 0, stream, p, args...);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_vad_flags(const ProblemVad& p, int floor_span, unsigned long long ratio_q8, long long min_energy,
                            unsigned char* flags, long long* energy, hipStream_t stream) {
    const hipError_t err = launch_walk(vad_energy_kernel<64>, vad_energy_kernel<8>, p, stream, energy);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(vad_flag_kernel, dim3((unsigned)vad_grid(p.total_windows, kVadFlagTile)), dim3(kVadThreads), 0, stream,
                       energy, p.win_start, p.U, p.total_windows, floor_span, ratio_q8, min_energy, flags);
    return hipGetLastError();
}

hipError_t launch_vad_mask(const unsigned char* flags, const long long* win_start, int U, int S, int avg_width, int max_silence,
                           int* dst, long long* out_len, hipStream_t stream) {
    hipLaunchKernelGGL(vad_mask_kernel, dim3((unsigned)U), dim3(kVadMaskThreads), 0, stream, flags, win_start, S, avg_width,
                       max_silence + 1, dst, out_len);
    return hipGetLastError();
}

hipError_t launch_vad_trim(const ProblemVad& p, const int* dst, const long long* out_start, float* out, hipStream_t stream) {
    return launch_walk(vad_trim_kernel<64>, vad_trim_kernel<8>, p, stream, dst, out_start, out);
}

int plan_string_vad(long long total_windows, int U, int S, char* buf, size_t cap) {
    if (total_windows == 0) return snprintf(buf, cap, "%s", "");
    const int G = vad_group(S), T = vad_tile(S);
    const long long grid = vad_grid(total_windows, T);
    return snprintf(buf, cap, "vad_energy<%d>/%d/%lld,vad_flag/%d/%lld,vad_mask/%d/%d,vad_trim<%d>/%d/%lld", G, T, grid,
                    kVadFlagTile, vad_grid(total_windows, kVadFlagTile), kVadMaskChunk, U, G, T, grid);
}

}  // namespace ge2e
