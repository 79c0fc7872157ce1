// ge2e_label_index: one speaker label per row -> what the ragged loss kernel reads, without leaving the device.
//   offsets [N+1]  offsets[j] = number of rows with a label < j
//   order   [R]    order[p] = the original row at sorted position p, STABLE (numpy.argsort(labels, kind="stable"))
// One 256-thread workgroup per batch, grid-stride over B with the ragged kernel's grid.  A counting sort in three steps:
//   1  histogram of the labels (integer atomics: the sum does not depend on their order)
//   2  exclusive scan of the histogram, 256 speakers at a time with a running carry: the offsets, and the start value of a
//      cursor per speaker
//   3  the rows in chunks of 256, IN ROW ORDER, inside a chunk one wave after the other: the lanes of a wave that hold the
//      same label find each other with ballots (rank = equal labels in lower lanes), the lowest of them reads the speaker's
//      cursor, advances it by the group's size and hands the old value to the others: position = cursor + rank.
// Earlier chunks, earlier waves and lower lanes come first, and those are the earlier rows: the rows of a speaker keep
// their order.  No step looks at blockIdx beyond choosing the batch, so a batch's result does not depend on its place.
// The counters are in LDS up to kLabelLdsSpeakers speakers and in the workgroup's workspace slice above that.
// Every label is clamped into [0, N-1] where it is read (both times), so the positions are a permutation of 0..R-1 and
// offsets[N] = R whatever the labels hold.
#include "ge2e_labels.hpp"
#include "ge2e_ragged.hpp"

namespace ge2e {

namespace {
constexpr int kThreads = 256, kWaves = kThreads / kWave;

__device__ __forceinline__ int wave_inclusive_scan(int v, int lane) {
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const int t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

// One batch.  cnt: N counters (LDS or workspace); wtot: kWaves ints of LDS.
__device__ __forceinline__ void index_batch(const int* lab, int N, int R, int* offs, int* ord, int* cnt, int* wtot) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    auto label_at = [&](long long r) { return min(max(lab[r], 0), N - 1); };

    // ---- 1: histogram ----
    for (int j = tid; j < N; j += kThreads) cnt[j] = 0;
    __syncthreads();
    for (long long r = tid; r < R; r += kThreads) atomicAdd(&cnt[label_at(r)], 1);
    __syncthreads();

    // ---- 2: exclusive scan -> offsets and cursors ----
    int carry = 0;
    for (long long j0 = 0; j0 < N; j0 += kThreads) {
        const long long j = j0 + tid;
        const int c = j < N ? cnt[j] : 0;
        const int inc = wave_inclusive_scan(c, lane);
        if (lane == kWave - 1) wtot[wid] = inc;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int i = 0; i < kWaves; ++i) {
            const int t = wtot[i];
            if (i < wid) before += t;
            total += t;
        }
        const int excl = carry + before + inc - c;
        if (j < N) { offs[j] = excl; cnt[j] = excl; }
        carry += total;
        __syncthreads();   // wtot is rewritten by the next round; the cursors are read by other threads below
    }
    if (tid == 0) offs[N] = carry;

    // ---- 3: positions, chunk by chunk in row order ----
    for (long long r0 = 0; r0 < R; r0 += kThreads) {
        const long long r = r0 + tid;
        const bool valid = r < R;
        const int l = valid ? label_at(r) : -1;
        int rank = 0, group = 0, lead = lane;
        bool todo = valid;
        for (;;) {   // one round per distinct label of the wave; every lane of the wave takes every round
            const unsigned long long open = __ballot(todo);
            if (!open) break;
            const int first = __ffsll((long long)open) - 1;
            const bool same = todo && l == __shfl(l, first);
            const unsigned long long g = __ballot(same);
            if (same) {
                rank = __popcll(g & ((1ull << lane) - 1ull));
                group = __popcll(g);
                lead = first;
                todo = false;
            }
        }
        for (int w = 0; w < kWaves; ++w) {
            if (wid == w) {
                int base = 0;
                if (valid && rank == 0) {   // one lane per label: nobody else touches this cursor now
                    base = cnt[l];
                    cnt[l] = base + group;
                }
                base = __shfl(base, lead);
                if (valid) ord[base + rank] = (int)r;
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(kThreads) void ge2e_label_index_kernel(const int* labels, int B, int N, int R, int* offsets,
                                                                     int* order, int* ws) {
    __shared__ int lds_cnt[kLabelLdsSpeakers];
    __shared__ int wtot[kWaves];
    for (int bi = blockIdx.x; bi < B; bi += gridDim.x) {
        const int* lab = labels + (size_t)bi * R;
        int* offs = offsets + (size_t)bi * (N + 1);
        int* ord = order + (size_t)bi * R;
        if (N <= kLabelLdsSpeakers) index_batch(lab, N, R, offs, ord, lds_cnt, wtot);
        else index_batch(lab, N, R, offs, ord, ws + (size_t)blockIdx.x * N, wtot);
        // (index_batch ends on a barrier: the counters are free for the next batch of this workgroup)
    }
}
}  // namespace

size_t label_index_workspace_bytes(int B, int N, int R) {
    (void)R;
    return N <= kLabelLdsSpeakers ? 0 : align_up((size_t)ragged_grid(B) * N * sizeof(int), 256);
}

hipError_t launch_label_index(const int* labels, int B, int N, int R, int* offsets, int* order, int* ws, hipStream_t stream) {
    hipLaunchKernelGGL(ge2e_label_index_kernel, dim3(ragged_grid(B)), dim3(kThreads), 0, stream, labels, B, N, R, offsets,
                       order, ws);
    return hipGetLastError();
}

}  // namespace ge2e
