// Device helpers of the bank kernels, written once: ge2e_enroll.hip (verification, plain and normalised), ge2e_identify.hip
// and ge2e_snorm.hip (the cohort scores).  "The same bits" between those calls rests on this file: every one of them takes
// its rows from tile_rows_plain, its products from tile_cosines (ge2e_rows_dev.hpp) and its score from raw_score, and the
// two that order scores do it through score_key.
#pragma once
#include "ge2e_rows_dev.hpp"

namespace ge2e {

// The score of (row, model): the product before the row norm, x 1 / |e_r|, + eps.
__device__ __forceinline__ float raw_score(float acc, float rne, float eps) { return acc * rne + eps; }

// The monotone map of a score onto 32 bits, a larger key for a larger score: -0 taken as +0, b ^ 0x80000000 for b >= 0 and
// ~b otherwise; 1 for a NaN, behind every number (-inf is 0x007fffff).  No score's key is 0.  Back: a NaN is the quiet NaN
// 0x7fc00000 and -0 is +0, the key does not carry the difference.
__device__ __forceinline__ unsigned score_key(float v) {
    unsigned b = __float_as_uint(v);
    if (b == 0x80000000u) b = 0u;
    const unsigned k = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return v != v ? 1u : k;
}
__device__ __forceinline__ float key_to_score(unsigned k) {
    if (k == 1u) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// Workgroup b of a grid of tiles x slices: tile b % tiles of the rows, slice b / tiles of the models (slice_models of them,
// a multiple of 64; the host counts non-empty slices only: k0 < K) -- workgroups that run together read the same slice.
// p0: the first of the wave's 16 rows.
struct SliceFrame { int slice, k0, n_models, p0; };
// -> false where the wave's rows are past the last of `nrows`: the whole wave leaves (the callers' waves share nothing and
// meet at no barrier).
__device__ __forceinline__ bool slice_frame(int tiles, int slice_models, int K, int nrows, SliceFrame& f) {
    const int tile = (int)(blockIdx.x % (unsigned)tiles);
    f.slice = (int)(blockIdx.x / (unsigned)tiles);
    f.k0 = f.slice * slice_models;
    f.n_models = min(slice_models, K - f.k0);
    f.p0 = tile * tile_geom::kTile + (int)(threadIdx.x >> 6) * tile_geom::kWaveRows;
    return f.p0 < nrows;
}

}  // namespace ge2e
