// The counting epilogue of the evaluation kernels, written once: ge2e_labeled_eval.hip (the fused row kernel and
// ge2e_eer_counts_labeled) and ge2e_enroll.hip (ge2e_verify_scores).  Every value is binned as it is produced by the number
// of thresholds below it (binary search on the fp32 table in LDS, the comparison is fp32 `>`; bin 0 counts for no threshold
// and is not recorded), LDS histograms [2][T+1], a suffix sum, INTEGER atomics into counts: exact, so the same bits every
// launch.  For workgroups of kCountThreads threads.
#pragma once
#include "ge2e_common.hpp"

namespace ge2e {

constexpr int kCountThreads = 256, kCountWaves = kCountThreads / kWave;

// The zeroing launch in front of a call that adds into integer outputs: a[0 .. n) = 0 and b[0 .. nb) = 0, nb <= 256; a
// pointer whose count is 0 is not touched.  One kernel for every such call (ge2e_labeled_eval.hip); a launch, not a memset
// node: the calls are captured into graphs as launches.  (Hidden: the library's symbol table stays as it was.)
__attribute__((visibility("hidden"))) hipError_t launch_zero_ints(int* a, size_t n, int* b, int nb, hipStream_t stream);

// LDS: hist [2][T+1] (false accepts, own accepts), then the T thresholds.
__device__ __forceinline__ void counting_begin(int* hist, float* thr_lds, const float* thr, int T) {
    for (int t = threadIdx.x; t < 2 * (T + 1); t += kCountThreads) hist[t] = 0;
    for (int t = threadIdx.x; t < T; t += kCountThreads) thr_lds[t] = thr[t];
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
__device__ __forceinline__ void counting_end(const int* hist, int T, int* counts, int (*wtot)[kCountWaves]) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int per = (T + kCountThreads - 1) / kCountThreads;
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
        for (int i = wid + 1; i < kCountWaves; ++i) run += wtot[a][i];
        for (int u = hi - 1; u >= lo; --u) {
            run += hist[a * (T + 1) + u];
            if (run) atomicAdd(&counts[(size_t)(u - 1) * 2 + a], run);
        }
    }
}

}  // namespace ge2e
