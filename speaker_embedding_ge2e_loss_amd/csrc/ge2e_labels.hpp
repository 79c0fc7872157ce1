// Speaker labels -> the ragged kernel's offset table and row order, on the device (see ge2e_labels.hip).
#pragma once
#include "ge2e_common.hpp"

namespace ge2e {

// Speaker counts up to this keep their per-speaker counters in LDS; above it they live in the workspace, one slice of N
// int32 per workgroup of the launch (ragged_grid(B) of them).
constexpr int kLabelLdsSpeakers = 1024;

size_t label_index_workspace_bytes(int B, int N, int R);      // 0 while the counters fit LDS
// labels [B][R] -> offsets [B][N+1], order [B][R]; ws: label_index_workspace_bytes (unused, may be null, when that is 0)
hipError_t launch_label_index(const int* labels, int B, int N, int R, int* offsets, int* order, int* ws, hipStream_t stream);

// The masked form: labels of any content.  speakers [B][N], active [B][2] = {active speakers, active rows}; the same
// workspace rule.  A speaker is active from two valid rows on; with `lone_speakers` (enrolment, ge2e_enroll.hip) from one,
// and then up to min(N, R) speakers are active, not speaker_capacity's R / 2.
size_t label_index_masked_workspace_bytes(int B, int N, int R);
hipError_t launch_label_index_masked(const int* labels, int B, int N, int R, int* offsets, int* order, int* speakers,
                                     int* active, int* ws, hipStream_t stream, bool lone_speakers = false);

// R rows hold at most R / 2 speakers of two rows each: the NA that the kernels behind the masked index kernel lay their
// per-speaker planes out for, max(1, min(N, R / 2)).
inline int speaker_capacity(int N, int R) {
    const int n = N < R / 2 ? N : R / 2;
    return n > 1 ? n : 1;
}

// The index tables inside the workspace of a call that runs an index kernel first (host side; byte offsets): behind
// `base` bytes of the caller's own planes come offsets [B][N+1] | order [B][R] | with `masked`: speakers [B][N] |
// active [B][2] | `extra` bytes of the caller's (the evaluation call keeps its col [B][R] there) | the index kernel's
// counters.  Every part starts 256-byte aligned; a part that is not asked for takes no room.
struct IndexTables {
    size_t off, order, speakers, active, extra, index, total;
};
inline IndexTables index_tables(size_t base, int B, int N, int R, bool masked, size_t extra_bytes = 0) {
    const size_t b = (size_t)B;
    IndexTables L;
    L.off = base;
    L.order = L.off + align_up(b * ((size_t)N + 1) * sizeof(int), 256);
    L.speakers = L.order + align_up(b * R * sizeof(int), 256);
    L.active = L.speakers + (masked ? align_up(b * N * sizeof(int), 256) : 0);
    L.extra = L.active + (masked ? align_up(b * 2 * sizeof(int), 256) : 0);
    L.index = L.extra + align_up(extra_bytes, 256);
    L.total = L.index + (masked ? label_index_masked_workspace_bytes(B, N, R) : label_index_workspace_bytes(B, N, R));
    return L;
}

}  // namespace ge2e
