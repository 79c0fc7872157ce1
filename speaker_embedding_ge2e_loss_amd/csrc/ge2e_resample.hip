// ge2e_resample_pack / ge2e_resample / ge2e_volume_gain: the stage in front of ge2e_melspec -- recordings at any rate to
// the model's rate (the reference's librosa.resample, utils/audio_utils.py:83-85) and the gain of its normalize_volume.
//
// RESAMPLE.  Rates sr_in -> sr_out with g = gcd: L = sr_out / g (up), M = sr_in / g (down), a bank taps[L][W], W = 2 lead + 1,
// of ANY float32 values.  Utterance u is x = wav[in_start[u] .. + in_len[u]), zero outside its own extent; output n, with
// t = n M (64-bit), i0 = t div L, p = t mod L, is
//     y[n] = sum_{k=0}^{W-1} taps[p][k] x[i0 + lead - k]
//   order     ONE fp32 accumulator per output, started at -0, acc = fma(taps[p][k], x[i0 + lead - k], acc) for k = 0, 1, ...,
//             W - 1 in this order, zeros of the extent included (they are staged as +0, never skipped).  Nothing else enters:
//             the bits of y[n] depend on the utterance's samples, on n and on the bank alone.
//   bank      packed[k][q], q < pad4(L), holds taps[(q M) mod L][k]: the phases in the order consecutive outputs meet them,
//             so 64 lanes with consecutive outputs read 64 consecutive words (one or two lines) at every k.  At L = 1 every
//             lane reads the same word.  The bank stays in L2 / L1 (up to 2.6 MB at the largest shape), not in LDS.
//   tile      a 256-thread workgroup owns tile = L B R consecutive outputs of one utterance, starting at a multiple of the
//             tile (so of L), as L B items (q, b) of R outputs n = q + L (b + B r): one tap load feeds R FMAs, and the lanes of
//             a wave (consecutive q, or consecutive b at small L) read LDS words floor(q M / L) resp. b M apart -- at M = 3 and
//             at 441 / 160 without a bank conflict of note.  The tile's B R M + W - 1 input samples are staged in LDS once,
//             the zeros of the extent filled in there; a sample outside the utterance is never read.  ge2e_resample.hpp has
//             the choice of B and R and the block numbering by which a workgroup finds its utterance from out_start.
//   global    a shape whose span does not fit the LDS budget (M large under a short filter) reads its samples from global
//             memory under the same extent test; same order, same bits.
// A NaN sample poisons exactly the outputs whose window holds it (0 x NaN is NaN; no tap is skipped).
//
// GAIN.  Launch 1, grid (U, 128): workgroup (u, s) walks the tiles j = s, s + 128, ... of 2048 samples of utterance u; thread t
// adds x^2 (in double) of samples j 2048 + t + 256 i, i = 0 .. 7, tile after tile in index order, to its own sum; the 256 sums
// are added by a butterfly over each wave and then wave 0 .. 3 in order, and the slice's sum goes to ws[u][s].  Launch 2: one
// thread per utterance adds its 128 slices in index order, rms = sqrt(S / n), gain = 10^((target - 20 log10(rms)) / 20) in
// double, rounded once.  No atomics: the same bits on every call, and nothing of another utterance enters.
#include "ge2e_resample.hpp"

#include <math.h>
#include <stdio.h>

namespace ge2e {

namespace {

__global__ __launch_bounds__(256) void resample_pack_kernel(const float* __restrict__ taps, int L, int M, int W, int lpad,
                                                             float* __restrict__ packed, size_t total) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        const int k = (int)(idx / lpad), q = (int)(idx % lpad);
        packed[idx] = q < L ? taps[(size_t)((q * M) % L) * W + k] : 0.f;
    }
}

template <int R, bool STAGED>
__global__ __launch_bounds__(kResampleThreads) void resample_kernel(ProblemResample p) {
    extern __shared__ __attribute__((aligned(16))) float res_lds[];
    // the block's utterance: the last u whose first block, out_start[u] / tile + u, is not past this one
    const long long blk = blockIdx.x;
    const int u = last_not_above(p.U, blk, [&](int i) { return p.out_start[i] / p.tile + i; });
    const long long o0 = p.out_start[u], n_out = p.out_start[u + 1] - o0;
    const long long lt = blk - (o0 / p.tile + u);           // the tile of the utterance
    if (lt < 0 || lt * p.tile >= n_out) return;             // (uniform over the workgroup)
    const long long len = p.in_len[u];
    const float* __restrict__ x = p.wav + p.in_start[u];
    const long long t0 = lt * p.tile;
    // output t0 has i0 = t0 M / L exactly (L divides the tile); local word j of the span is sample span_lo + j
    const long long span_lo = lt * ((long long)p.B * R * p.M) + p.lead - (p.W - 1);
    auto sample = [&](long long g) -> float { return (g >= 0 && g < len) ? x[g] : 0.f; };
    if constexpr (STAGED) {
        for (int j = threadIdx.x; j < p.span; j += kResampleThreads) res_lds[j] = sample(span_lo + j);
        __syncthreads();
    }
    const int items = p.L * p.B;
    for (int item = threadIdx.x; item < items; item += kResampleThreads) {
        const int b = item / p.L, q = item - b * p.L;
        const float* __restrict__ tp = p.packed + q;
        // word of (r, k): floor(q M / L) + (b + B r) M + (W - 1) - k
        const int at = (q * p.M) / p.L + b * p.M + p.W - 1;
        float acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = -0.f;   // the identity of addition: -0 + -0 = -0, so a copying bank keeps a -0
#pragma unroll 4
        for (int k = 0; k < p.W; ++k) {
            const float t = tp[(size_t)k * p.lpad];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int j = at + r * p.B * p.M - k;
                acc[r] = fmaf(t, STAGED ? res_lds[j] : sample(span_lo + j), acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const long long n = t0 + q + (long long)p.L * (b + p.B * r);
            if (n < n_out) p.out[o0 + n] = acc[r];
        }
    }
}

__global__ __launch_bounds__(kGainThreads) void gain_partial_kernel(const float* __restrict__ wav,
                                                                     const long long* __restrict__ utt_start,
                                                                     const long long* __restrict__ utt_len,
                                                                     double* __restrict__ ws) {
    __shared__ double wave_part[kGainThreads / kWave];
    const int u = blockIdx.x, s = blockIdx.y;
    const long long len = utt_len[u];
    const float* __restrict__ x = wav + utt_start[u];
    double sum = 0.0;
    for (long long base = (long long)s * kGainTile; base < len; base += (long long)kGainSlices * kGainTile) {
        float v[kGainTile / kGainThreads];
#pragma unroll
        for (int i = 0; i < kGainTile / kGainThreads; ++i) {
            const long long g = base + threadIdx.x + i * kGainThreads;
            v[i] = g < len ? x[g] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < kGainTile / kGainThreads; ++i) sum += (double)v[i] * (double)v[i];
    }
    sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = wave_part[0];
        for (int w = 1; w < kGainThreads / kWave; ++w) total += wave_part[w];
        ws[(size_t)u * kGainSlices + s] = total;
    }
}

__global__ __launch_bounds__(kGainThreads) void gain_final_kernel(const long long* __restrict__ utt_len,
                                                                   const double* __restrict__ ws, int U, double target_dbfs,
                                                                   int increase_only, float* __restrict__ gain_out) {
    const int u = blockIdx.x * kGainThreads + threadIdx.x;
    if (u >= U) return;
    double total = 0.0;
    for (int s = 0; s < kGainSlices; ++s) total += ws[(size_t)u * kGainSlices + s];
    const double rms = sqrt(total / (double)utt_len[u]);
    const double change = target_dbfs - 20.0 * log10(rms);
    double gain = pow(10.0, change / 20.0);
    if (increase_only && change < 0.0) gain = 1.0;           // (a NaN change keeps its NaN gain)
    gain_out[u] = (float)gain;
}

template <int R, bool STAGED>
hipError_t launch_resample_r(const ProblemResample& p, long long grid, hipStream_t stream) {
    const unsigned lds = STAGED ? (unsigned)(sizeof(float) * p.span) : 0u;
    hipLaunchKernelGGL((resample_kernel<R, STAGED>), dim3((unsigned)grid), dim3(kResampleThreads), lds, stream, p);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_resample_pack(const float* taps, int L, int M, int W, float* packed, hipStream_t stream) {
    return launch_per_element(resample_pack_kernel, resample_packed_floats(L, W), stream, taps, L, M, W, resample_lpad(L), packed);
}

hipError_t launch_resample(const ProblemResample& p, const ResamplePlan& plan, long long grid, hipStream_t stream) {
    if (!plan.staged) return launch_resample_r<4, false>(p, grid, stream);
    switch (plan.R) {
        case 8: return launch_resample_r<8, true>(p, grid, stream);
        case 4: return launch_resample_r<4, true>(p, grid, stream);
        case 2: return launch_resample_r<2, true>(p, grid, stream);
        default: return launch_resample_r<1, true>(p, grid, stream);
    }
}

hipError_t launch_volume_gain(const float* wav, const long long* utt_start, const long long* utt_len, int U,
                              double target_dbfs, int increase_only, float* gain_out, double* ws, hipStream_t stream) {
    hipLaunchKernelGGL(gain_partial_kernel, dim3((unsigned)U, kGainSlices), dim3(kGainThreads), 0, stream, wav, utt_start,
                       utt_len, ws);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(gain_final_kernel, dim3((unsigned)((U + kGainThreads - 1) / kGainThreads)), dim3(kGainThreads), 0,
                       stream, utt_len, ws, U, target_dbfs, increase_only, gain_out);
    return hipGetLastError();
}

int plan_string_resample(long long total_out, int U, int L, int M, int W, char* buf, size_t cap) {
    const ResamplePlan plan = resample_plan(L, M, W);
    return snprintf(buf, cap, "resample<%s,%d>/%d/%lld", plan.staged ? "lds" : "global", plan.R, plan.tile,
                    resample_grid(total_out, U, plan.tile));
}

}  // namespace ge2e
