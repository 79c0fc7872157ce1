// Tiles, limits + launchers of ge2e_vad_flags / ge2e_vad_mask / ge2e_vad_trim (see ge2e_vad.hip): the reference's
// trim_long_silences between the gain and ge2e_melspec -- window energies, voice flags, mask, compaction.
#pragma once
#include "ge2e_common.hpp"

namespace ge2e {

constexpr int kVadThreads = 256;          // the energy, flag and trim kernels
constexpr int kVadMinS = 2, kVadMaxS = 4096;
constexpr int kVadMaxSpan = 1024;         // floor_span: windows either side of the sliding minimum
constexpr int kVadMaxWidth = 64;          // avg_width and max_silence + 1
constexpr int kVadWindowsPerGroup = 4;    // windows a group of lanes takes in turn
constexpr int kVadFlagTile = kVadThreads; // windows a workgroup of the flag kernel owns, one a thread
constexpr int kVadMaskThreads = 1024, kVadMaskPerThread = 4;
constexpr int kVadMaskChunk = kVadMaskThreads * kVadMaskPerThread;   // windows a step of the mask kernel's walk

inline bool vad_window_supported(long long S) { return S >= kVadMinS && S <= kVadMaxS; }
// Lanes a window in the energy and trim kernels: a whole wave from 64 samples on, eight lanes below.
inline int vad_group(int S) { return S >= 64 ? 64 : 8; }
// Consecutive windows a workgroup of those kernels owns: 256 / G groups of lanes, four windows each.
inline int vad_tile(int S) { return kVadThreads / vad_group(S) * kVadWindowsPerGroup; }
inline long long vad_grid(long long total_windows, int tile) { return (total_windows + tile - 1) / tile; }
inline size_t vad_workspace_bytes(long long total_windows) { return (size_t)total_windows * sizeof(long long); }

struct ProblemVad {
    const float* wav;
    const long long* utt_start;   // [U]
    const float* gain;            // [U] or null
    const long long* win_start;   // [U + 1]
    int U, S;
    long long total_windows;
};

hipError_t launch_vad_flags(const ProblemVad& p, int floor_span, unsigned long long ratio_q8, long long min_energy,
                            unsigned char* flags, long long* energy, hipStream_t stream);
hipError_t launch_vad_mask(const unsigned char* flags, const long long* win_start, int U, int S, int avg_width, int max_silence,
                           int* dst, long long* out_len, hipStream_t stream);
hipError_t launch_vad_trim(const ProblemVad& p, const int* dst, const long long* out_start, float* out, hipStream_t stream);
// "vad_energy<G>/T/grid,vad_flag/256/grid,vad_mask/4096/U,vad_trim<G>/T/grid", snprintf-style.
int plan_string_vad(long long total_windows, int U, int S, char* buf, size_t cap);

}  // namespace ge2e
