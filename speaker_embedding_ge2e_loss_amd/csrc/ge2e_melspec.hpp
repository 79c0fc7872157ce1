// Layout of the packed tables + launchers of ge2e_melspec_pack / ge2e_melspec (see ge2e_melspec.hip): the mel front end,
// waveforms to (log-)mel frames in one launch.
#pragma once
#include "ge2e_common.hpp"

namespace ge2e {

constexpr int kMelTile = 16;        // frames (rows of out) of a workgroup: one MFMA row tile
constexpr int kMelThreads = 512;    // eight waves: two frames each, then one 16-column tile of the mel product each
constexpr int kMelWaves = kMelThreads / kWave;
constexpr int kMelMaxMels = 128;    // eight column tiles

inline bool melspec_supported(int n_fft, int n_mels) {
    return (n_fft == 256 || n_fft == 512 || n_fft == 1024 || n_fft == 2048) && n_mels >= 1 && n_mels <= kMelMaxMels;
}
__host__ __device__ inline int mel_pad16(int n) { return (n + 15) & ~15; }
// Rows of the basis, n_fft / 2 + 1, padded to whole K-steps of 4.
__host__ __device__ inline int mel_kpad(int n_fft) { return n_fft / 2 + 4; }
// The packed buffer in floats: window [n_fft], twiddles exp(-2 pi i k / n_fft) as (cos, sin) [n_fft][2], then the basis
// [column tile][K-step][lane]: lane q * 16 + l15 of K-step s of column tile ct holds basis[4 s + q][16 ct + l15], the B
// fragment of v_mfma_f32_16x16x4_f32, zero past n_fft / 2 + 1 rows and past n_mels columns.
inline size_t melspec_packed_floats(int n_fft, int n_mels) {
    return 3 * (size_t)n_fft + (size_t)mel_kpad(n_fft) * mel_pad16(n_mels);
}
// LDS: the magnitude tile [16][n_fft / 2 + 34] (the row stride is 2 mod 32: the 32 lanes of an A-fragment read fall on 32
// banks) and per wave the transform's two planes (re, im) of n_fft / 2 points, one pad word after every 32.
__host__ __device__ inline int mel_tile_stride(int n_fft) { return n_fft / 2 + 34; }
__host__ __device__ inline int mel_plane_floats(int n_fft) { return n_fft / 2 + n_fft / 64; }
inline size_t melspec_lds_bytes(int n_fft) {
    return sizeof(float) * ((size_t)kMelTile * mel_tile_stride(n_fft) + (size_t)kMelWaves * 2 * mel_plane_floats(n_fft));
}

struct ProblemMelspec {
    const float* packed;
    const float* wav;
    const long long* utt_start;         // [U]
    const long long* utt_len;           // [U]
    const long long* utt_padded_len;    // [U] or null: utt_len
    const float* gain;                  // [U] or null: 1
    const long long* frame_start;       // [U + 1]
    float* out;                         // [total_frames][n_mels]
    long long total_frames;
    int U, hop, n_mels, mode;
    float min_level, min_level_db, ref_level_db;   // min_level = 10^(min_level_db / 20)
};

hipError_t launch_melspec_pack(const float* window, const float* basis, int n_fft, int n_mels, float* packed, hipStream_t stream);
hipError_t launch_melspec(const ProblemMelspec& p, int n_fft, hipStream_t stream);
// "melspec<n_fft>/tiles": the instantiation and its grid, snprintf-style.
int plan_string_melspec(long long total_frames, int n_fft, char* buf, size_t cap);

}  // namespace ge2e
