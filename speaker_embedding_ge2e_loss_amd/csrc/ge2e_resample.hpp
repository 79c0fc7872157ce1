// Layout of the packed bank, the tile plan + launchers of ge2e_resample_pack / ge2e_resample / ge2e_volume_gain (see
// ge2e_resample.hip): band-limited rational resampling and the per-utterance gain, the stage in front of ge2e_melspec.
#pragma once
#include "ge2e_common.hpp"

namespace ge2e {

constexpr int kResampleThreads = 256;
constexpr int kResampleMaxL = 640, kResampleMaxM = 640, kResampleMaxW = 1025;
constexpr int kResampleSpanMax = 10240;   // floats of LDS a tile may stage: 40 KB, four workgroups on a CU

inline bool resample_supported(long long L, long long M, long long W) {
    return L >= 1 && L <= kResampleMaxL && M >= 1 && M <= kResampleMaxM && W >= 1 && W <= kResampleMaxW && (W & 1);
}
// The packed bank in floats: [W][pad4(L)], packed[k][q] = taps[(q M) mod L][k] -- the phases in the order consecutive
// outputs meet them (output n has phase (n M) mod L, a function of n mod L), so the lanes of a wave, which hold consecutive
// outputs, read consecutive words at every k.  Zero in the pad columns.
__host__ __device__ inline int resample_lpad(int L) { return (L + 3) & ~3; }
inline size_t resample_packed_floats(int L, int W) { return (size_t)W * resample_lpad(L); }

// The tile of a shape.  A workgroup owns `tile` = L B R consecutive outputs of ONE utterance, as L B items of R outputs:
// item (q, b), q < L, b < B, holds outputs q + L (b + B r), r < R, which share phase q's taps; the tile reads B R M + W - 1
// consecutive input samples.  B: the count in ceil(256 / L) .. ceil(2048 / L) that leaves the fewest idle lanes in the last
// pass of 256 threads over the items (the first such).  R: the largest of 8, 4, 2, 1 whose input span fits kResampleSpanMax
// floats of LDS; where none does (a long down-sampling step under a short filter) the samples are read from global memory
// instead (staged = false, R = 4).
struct ResamplePlan {
    bool staged;
    int R, B, tile, span;
};
inline ResamplePlan resample_plan(int L, int M, int W) {
    int B = (kResampleThreads + L - 1) / L;
    double best = 0.0;
    for (int b = B; b <= (2048 + L - 1) / L; ++b) {
        const int items = L * b, passes = (items + kResampleThreads - 1) / kResampleThreads;
        const double eff = (double)items / ((double)passes * kResampleThreads);
        if (eff > best + 1e-12) { best = eff; B = b; }
    }
    for (int R = 8; R >= 1; R >>= 1) {
        const long long span = (long long)B * R * M + W - 1;
        if (span <= kResampleSpanMax) return {true, R, B, L * B * R, (int)span};
    }
    return {false, 4, B, L * B * 4, 0};
}
// Workgroups of a call: utterance u owns blocks out_start[u] / tile + u up to that of u + 1 (at least its ceil(n_out / tile)
// tiles: the numbers grow strictly, so a block finds its utterance with last_not_above); floor(total_out / tile) + U in all.
inline long long resample_grid(long long total_out, int U, int tile) { return total_out / tile + U; }

struct ProblemResample {
    const float* packed;
    const float* wav;
    const long long* in_start;    // [U]
    const long long* in_len;      // [U]
    const long long* out_start;   // [U + 1]
    float* out;                   // [total_out]
    int U, L, M, lead, W, lpad, B, tile, span;
};

constexpr int kGainThreads = 256;
constexpr int kGainTile = 2048;     // samples of a tile: eight per thread
constexpr int kGainSlices = 128;    // workgroups per utterance
// Workspace of ge2e_volume_gain: one double per (utterance, slice).
inline size_t volume_gain_workspace_bytes(int U) { return (size_t)U * kGainSlices * sizeof(double); }

hipError_t launch_resample_pack(const float* taps, int L, int M, int W, float* packed, hipStream_t stream);
hipError_t launch_resample(const ProblemResample& p, const ResamplePlan& plan, long long grid, hipStream_t stream);
hipError_t launch_volume_gain(const float* wav, const long long* utt_start, const long long* utt_len, int U,
                              double target_dbfs, int increase_only, float* gain_out, double* ws, hipStream_t stream);
// "resample<lds|global,R>/tile/grid": the instantiation, the outputs of a tile and the grid, snprintf-style.
int plan_string_resample(long long total_out, int U, int L, int M, int W, char* buf, size_t cap);

}  // namespace ge2e
