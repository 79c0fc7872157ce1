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

// Step 3's grouping, for both forms: the lanes of a wave that hold the same key find each other with ballots.  rank = the
// equal keys in lower lanes, group = how many there are, lead = the lowest of them.  Called by the whole wave; a lane that
// is not `valid` joins no group.
struct KeyGroup { int rank, group, lead; };
__device__ __forceinline__ KeyGroup wave_group_by_key(int key, bool valid, int lane) {
    KeyGroup g = {0, 0, lane};
    bool todo = valid;
    for (;;) {   // one round per distinct key of the wave; every lane of the wave takes every round
        const unsigned long long open = __ballot(todo);
        if (!open) break;
        const int first = __ffsll((long long)open) - 1;
        const bool same = todo && key == __shfl(key, first);
        const unsigned long long m = __ballot(same);
        if (same) {
            g.rank = __popcll(m & ((1ull << lane) - 1ull));
            g.group = __popcll(m);
            g.lead = first;
            todo = false;
        }
    }
    return g;
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
        const KeyGroup g = wave_group_by_key(l, valid, lane);
        for (int w = 0; w < kWaves; ++w) {
            if (wid == w) {
                int base = 0;
                if (valid && g.rank == 0) {   // one lane per label: nobody else touches this cursor now
                    base = cnt[l];
                    cnt[l] = base + g.group;
                }
                base = __shfl(base, g.lead);
                if (valid) ord[base + g.rank] = (int)r;
            }
            __syncthreads();
        }
    }
}

// The MASKED form (ge2e_label_index_masked): the labels may hold anything.  A row is valid iff 0 <= label < N (nothing is
// clamped), a speaker is active iff at least 2 valid rows carry its label, a row is active iff it is valid and its speaker
// is active.  The same plan with two scans where the plain form has one:
//   1  histogram of the VALID labels only
//   2  per speaker the active flag (count >= 2); an exclusive scan of the flags gives the speaker's compact id k (the active
//      speakers numbered by ascending label) and speakers[k]; an exclusive scan of the counts of the active speakers gives
//      offsets[k] and the speaker's cursor.  The cursor of a speaker that is not active is -1, which is how step 3 tells.
//      offsets[n_act .. N] = r_act, speakers[n_act .. N-1] = -1, active = {n_act, r_act}.
//   3  the rows in row order as above; the key of an active row is its label, every other row has the key N, whose cursor is
//      the tail cursor (one int of LDS, starting at r_act): the rows that do not count follow the active ones in ascending
//      row index, so order is a permutation of 0..R-1 whatever the labels hold.
// Whether a row is active is read from the cursors before any of the chunk moves (one barrier): cursors only grow from a
// value >= 0, so the answer is the same for every chunk.
// kMinRows: the activity threshold, the valid rows a speaker needs to be active: 2 for the loss and the training-time
// evaluation (a lone row has no leave-one-out centroid), 1 for enrolment (ge2e_enroll.hip), where every valid row counts.
// cnt: N counters (LDS or workspace); wtot: 2 kWaves ints of LDS; tail: one int of LDS.
template <int kMinRows>
__device__ __forceinline__ void index_batch_masked(const int* lab, int N, int R, int* offs, int* ord, int* spkr, int* act,
                                                   int* cnt, int* wtot, int* tail) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;

    // ---- 1: histogram of the valid labels ----
    for (int j = tid; j < N; j += kThreads) cnt[j] = 0;
    __syncthreads();
    for (long long r = tid; r < R; r += kThreads) {
        const int l = lab[r];
        if (l >= 0 && l < N) atomicAdd(&cnt[l], 1);
    }
    __syncthreads();

    // ---- 2: active flags; scans of the flags and of the active counts ----
    int ncarry = 0, rcarry = 0;
    for (long long j0 = 0; j0 < N; j0 += kThreads) {
        const long long j = j0 + tid;
        const int c = j < N ? cnt[j] : 0;
        const int f = c >= kMinRows ? 1 : 0, a = f ? c : 0;
        const int incf = wave_inclusive_scan(f, lane), inca = wave_inclusive_scan(a, lane);
        if (lane == kWave - 1) { wtot[wid] = incf; wtot[kWaves + wid] = inca; }
        __syncthreads();
        int beforef = 0, totalf = 0, beforea = 0, totala = 0;
#pragma unroll
        for (int i = 0; i < kWaves; ++i) {
            const int tf = wtot[i], ta = wtot[kWaves + i];
            if (i < wid) { beforef += tf; beforea += ta; }
            totalf += tf; totala += ta;
        }
        if (j < N) {
            if (f) {
                const int k = ncarry + beforef + incf - f, o = rcarry + beforea + inca - a;
                offs[k] = o; spkr[k] = (int)j; cnt[j] = o;
            } else {
                cnt[j] = -1;
            }
        }
        ncarry += totalf; rcarry += totala;
        __syncthreads();   // wtot is rewritten by the next round; the cursors are read by other threads below
    }
    for (long long k = (long long)ncarry + tid; k <= N; k += kThreads) offs[k] = rcarry;
    for (long long k = (long long)ncarry + tid; k < N; k += kThreads) spkr[k] = -1;
    if (tid == 0) { act[0] = ncarry; act[1] = rcarry; *tail = rcarry; }
    __syncthreads();

    // ---- 3: positions, chunk by chunk in row order; the rows that do not count go to the tail ----
    for (long long r0 = 0; r0 < R; r0 += kThreads) {
        const long long r = r0 + tid;
        const bool valid = r < R;
        int key = -1;
        if (valid) {
            const int l = lab[r];
            key = (l >= 0 && l < N && cnt[l] >= 0) ? l : N;
        }
        __syncthreads();   // every key of the chunk is decided before a cursor moves
        const KeyGroup g = wave_group_by_key(key, valid, lane);
        for (int w = 0; w < kWaves; ++w) {
            if (wid == w) {
                int base = 0;
                if (valid && g.rank == 0) {   // one lane per key: nobody else touches this cursor now
                    int* cur = key < N ? &cnt[key] : tail;
                    base = *cur;
                    *cur = base + g.group;
                }
                base = __shfl(base, g.lead);
                // (the clamp holds only for labels that change between the two reads: otherwise the positions are exact)
                if (valid) ord[min(max(base + g.rank, 0), R - 1)] = (int)r;
            }
            __syncthreads();
        }
    }
}

template <int kMinRows>
__global__ __launch_bounds__(kThreads) void ge2e_label_index_masked_kernel(const int* labels, int B, int N, int R,
                                                                            int* offsets, int* order, int* speakers,
                                                                            int* active, int* ws) {
    __shared__ int lds_cnt[kLabelLdsSpeakers];
    __shared__ int wtot[2 * kWaves];
    __shared__ int tail;
    for (int bi = blockIdx.x; bi < B; bi += gridDim.x) {
        const int* lab = labels + (size_t)bi * R;
        int* offs = offsets + (size_t)bi * ((size_t)N + 1);
        int* ord = order + (size_t)bi * R;
        int* spkr = speakers + (size_t)bi * N;
        int* act = active + (size_t)bi * 2;
        int* cnt = N <= kLabelLdsSpeakers ? lds_cnt : ws + (size_t)blockIdx.x * N;
        index_batch_masked<kMinRows>(lab, N, R, offs, ord, spkr, act, cnt, wtot, &tail);
        // (index_batch_masked ends on a barrier: counters, wtot and tail are free for the next batch of this workgroup)
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

size_t label_index_masked_workspace_bytes(int B, int N, int R) { return label_index_workspace_bytes(B, N, R); }

hipError_t launch_label_index_masked(const int* labels, int B, int N, int R, int* offsets, int* order, int* speakers,
                                     int* active, int* ws, hipStream_t stream, bool lone_speakers) {
    if (lone_speakers)
        hipLaunchKernelGGL(ge2e_label_index_masked_kernel<1>, dim3(ragged_grid(B)), dim3(kThreads), 0, stream, labels, B, N, R,
                           offsets, order, speakers, active, ws);
    else
        hipLaunchKernelGGL(ge2e_label_index_masked_kernel<2>, dim3(ragged_grid(B)), dim3(kThreads), 0, stream, labels, B, N, R,
                           offsets, order, speakers, active, ws);
    return hipGetLastError();
}

}  // namespace ge2e
