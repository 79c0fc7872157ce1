// ge2e_sgd_clip_step: torch.nn.utils.clip_grad_norm_ per parameter group, then torch.optim.SGD, over the trainer's flat
// gradient bucket (the training step's last statements, s4:201-203) in two launches.  No atomics; every sum has one fixed
// order, so a call gives the same bits every time, and every rounding is an IEEE operation of its own (no fused
// multiply-add: contraction is off for this file), so a float32 emulation on the host reproduces the update bit for bit.
//
// A SEGMENT is one parameter tensor (include/ge2e_hip.h); a CHUNK is at most kSgdChunk = 4096 consecutive elements of one
// segment, one workgroup of 256 threads in either launch.  Workgroup c finds its segment in chunk_start: the last s with
// chunk_start[s] <= c (last_not_above, ge2e_common.hpp).
// THE WALK over a chunk of n elements: `head` elements (0 .. 3) up to the first 16-byte boundary, one a thread; then whole
// 16-byte pieces, piece j of thread j mod 256 (consecutive pieces over the lanes; a full chunk is four global_load_dwordx4
// a thread and array); then the tail of at most 3 elements, one a thread.  A chunk starts 16 KiB times k past its
// segment's start, so every chunk of a segment has the segment's own head.  SQSUM looks at the gradient's address alone;
// UPDATE needs the parameter, the gradient and the momentum slot congruent mod 16 and walks a segment where they are not a
// word at a time (head = 0, no pieces, the "tail" strided over all n).  Nothing outside [0, n) is touched.
// SQSUM (launch 1): thread t adds fl((g scale)^2) of its elements in the walk's order (which is index order) to a float32;
// wave_sum (a butterfly on the VALU: all lanes end with the same bits); the four wave sums through LDS as (w0 + w1) +
// (w2 + w3); partial[c].  At most 16 + 6 + 2 additions on an element's path.
// UPDATE (launch 2): every workgroup first sums the partials of EACH group with the same code: thread t adds partial[b + t],
// partial[b + t + 256], ... of the group's chunk range [b, e) in that order, then the same two trees (ceil((e - b) / 256)
// + 8 more additions: 10^8 parameters in one group give 96 + 8).  All workgroups hold the same bits of norm[g], coef[g]
// and of the verdict "some norm is not finite"; there is no second pass and no flag to wait for.  The gradient bucket
// (5.9 MB for the reference encoder) was read by launch 1 through the same workgroup -> chunk map, and workgroups b and b
// + 8 share an XCD in either launch as observed on this chip, so launch 2 finds it in that XCD's L2 (4 MiB each, 32 MiB in all).
#include "ge2e_optim.hpp"

#include <stdint.h>
#include <stdio.h>

// Every product and sum below is an IEEE operation of its own: none may be fused into a multiply-add (the intrinsics
// __fmul_rn / __fadd_rn do not keep hipcc from contracting them with their neighbours; this does).
#pragma clang fp contract(off)

namespace ge2e {

namespace {

struct SgdChunk {
    float* param;          // the chunk's first element
    long long goff;        // ... and its offset in the gradient bucket (and the momentum buffer)
    int n, group;
};

__device__ __forceinline__ SgdChunk sgd_chunk(const ProblemSgd& p, int c) {
    const int s = last_not_above(p.S, c, [&](int i) { return p.chunk_start[i]; });
    const long long* e = p.seg + 4 * (long long)s;
    const long long base = (long long)(c - p.chunk_start[s]) * kSgdChunk, left = e[2] - base;
    return {(float*)(uintptr_t)e[0] + base, e[1] + base, (int)(left < kSgdChunk ? left : kSgdChunk), (int)e[3]};
}

__device__ __forceinline__ int sgd_misalign(const void* q) { return (int)((uintptr_t)q & 15); }

// The walk: one(i) for the single elements, four(i) for the pieces that start at element i.  `vec` false: a word at a time.
template <class One, class Four>
__device__ __forceinline__ void sgd_walk(int n, int misalign, bool vec, One&& one, Four&& four) {
    const int t = threadIdx.x;
    int head = vec ? ((16 - misalign) & 15) >> 2 : 0;
    head = head < n ? head : n;
    const int pieces = vec ? (n - head) >> 2 : 0;
    if (t < head) one(t);
    for (int j = t; j < pieces; j += kSgdThreads) four(head + 4 * j);
    for (int i = head + 4 * pieces + t; i < n; i += kSgdThreads) one(i);
}

// wave sums of K values, each left in wsum[k][wave]; the caller's barrier, then sgd_block_total
__device__ __forceinline__ void sgd_wave_part(float v, float (*wsum)[kSgdThreads / kWave], int k) {
    v = wave_sum(v);
    if ((threadIdx.x & (kWave - 1)) == 0) wsum[k][threadIdx.x / kWave] = v;
}
__device__ __forceinline__ float sgd_block_total(const float (*wsum)[kSgdThreads / kWave], int k) {
    return (wsum[k][0] + wsum[k][1]) + (wsum[k][2] + wsum[k][3]);
}

__global__ __launch_bounds__(kSgdThreads) void sgd_sqsum_kernel(ProblemSgd p) {
    __shared__ float wsum[1][kSgdThreads / kWave];
    const SgdChunk ch = sgd_chunk(p, blockIdx.x);
    const float* g = p.grad + ch.goff;
    const float scale = p.grad_scale;
    float acc = 0.0f;
    auto add = [&](float x) {
        const float g1 = x * scale;
        acc = acc + g1 * g1;
    };
    sgd_walk(ch.n, sgd_misalign(g), true, [&](int i) { add(g[i]); },
             [&](int i) {
                 const float4 x = *(const float4*)(g + i);
                 add(x.x); add(x.y); add(x.z); add(x.w);
             });
    sgd_wave_part(acc, wsum, 0);
    __syncthreads();
    if (threadIdx.x == 0) p.partial[blockIdx.x] = sgd_block_total(wsum, 0);
}

// what one element becomes (include/ge2e_hip.h): every operation rounded on its own
struct SgdCoefs {
    float scale, coef, lr, wd, mu;
    bool skip, zero;
};
__device__ __forceinline__ void sgd_element(const SgdCoefs& k, float g, float p, float m, float& g_out, float& p_out, float& m_out) {
    const float g2 = g * k.scale * k.coef;
    const float g3 = k.wd != 0.0f ? g2 + k.wd * p : g2;
    m_out = k.mu != 0.0f ? k.mu * m + g3 : g3;
    p_out = p - k.lr * m_out;
    g_out = k.zero ? 0.0f : g2;
}

template <bool MOM>
__global__ __launch_bounds__(kSgdThreads) void sgd_update_kernel(ProblemSgd p) {
    __shared__ int bound[kSgdMaxGroups + 1];                       // group g's chunks are [bound[g], bound[g + 1])
    __shared__ float wsum[kSgdMaxGroups][kSgdThreads / kWave];
    const int t = threadIdx.x;
    if (t <= p.G) {
        int b = 0;
        if (t > 0) {                                               // behind the last segment of a group below t, if there is one
            const int s = last_not_above(p.S, (long long)(t - 1), [&](int i) { return p.seg[4 * (long long)i + 3]; });
            b = p.seg[4 * (long long)s + 3] <= t - 1 ? p.chunk_start[s + 1] : 0;
        }
        bound[t] = b;
    }
    __syncthreads();
    for (int g = 0; g < p.G; ++g) {
        float v = 0.0f;
        for (int c = bound[g] + t; c < bound[g + 1]; c += kSgdThreads) v += p.partial[c];
        sgd_wave_part(v, wsum, g);
    }
    __syncthreads();
    const SgdChunk ch = sgd_chunk(p, blockIdx.x);
    SgdCoefs k = {p.grad_scale, 0.0f, 0.0f, 0.0f, 0.0f, false, (p.flags & kSgdFlagZeroGrad) != 0};
    bool nonfinite = false;
    for (int g = 0; g < p.G; ++g) {
        const float norm = sqrtf(sgd_block_total(wsum, g));
        const float c = p.hyper[4 * g + 1] / (norm + 1e-6f);
        const float coef = c > 1.0f ? 1.0f : c;                    // torch.clamp(c, max=1): a NaN passes
        nonfinite |= !(fabsf(norm) <= 3.402823466e38f);
        if (g == ch.group) {
            k.coef = coef;
            k.lr = p.hyper[4 * g];
            k.wd = p.hyper[4 * g + 2];
            k.mu = p.hyper[4 * g + 3];
        }
        if (blockIdx.x == 0 && t == 0 && p.stats) {
            p.stats[2 * g] = norm;
            p.stats[2 * g + 1] = coef;
        }
    }
    k.skip = (p.flags & kSgdFlagSkipNonfinite) != 0 && nonfinite;
    if (blockIdx.x == 0 && t == 0 && k.skip) *p.skipped += 1;     // one writer: no atomic

    float* g = p.grad + ch.goff;
    float* w = ch.param;
    float* m = MOM ? p.momentum + ch.goff : nullptr;
    const int a = sgd_misalign(g);
    const bool vec = sgd_misalign(w) == a && (!MOM || sgd_misalign(m) == a);
    if (k.skip) {                                                  // parameters and momentum stay as they are, bit for bit
        auto clipped = [&](float x) { return k.zero ? 0.0f : x * k.scale * k.coef; };
        sgd_walk(ch.n, a, true, [&](int i) { g[i] = clipped(g[i]); },
                 [&](int i) {
                     const float4 x = *(const float4*)(g + i);
                     *(float4*)(g + i) = make_float4(clipped(x.x), clipped(x.y), clipped(x.z), clipped(x.w));
                 });
        return;
    }
    const bool read_m = MOM && k.mu != 0.0f;
    sgd_walk(ch.n, a, vec,
             [&](int i) {
                 float go, po, mo;
                 sgd_element(k, g[i], w[i], read_m ? m[i] : 0.0f, go, po, mo);
                 g[i] = go;
                 w[i] = po;
                 if (MOM) m[i] = mo;
             },
             [&](int i) {
                 const float4 gi = *(const float4*)(g + i), wi = *(const float4*)(w + i);
                 const float4 mi = read_m ? *(const float4*)(m + i) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                 float4 go, po, mo;
                 sgd_element(k, gi.x, wi.x, mi.x, go.x, po.x, mo.x);
                 sgd_element(k, gi.y, wi.y, mi.y, go.y, po.y, mo.y);
                 sgd_element(k, gi.z, wi.z, mi.z, go.z, po.z, mo.z);
                 sgd_element(k, gi.w, wi.w, mi.w, go.w, po.w, mo.w);
                 *(float4*)(g + i) = go;
                 *(float4*)(w + i) = po;
                 if (MOM) *(float4*)(m + i) = mo;
             });
}

}  // namespace

hipError_t launch_sgd_clip_step(const ProblemSgd& p, hipStream_t stream) {
    hipLaunchKernelGGL(sgd_sqsum_kernel, dim3((unsigned)p.C), dim3(kSgdThreads), 0, stream, p);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(p.momentum ? sgd_update_kernel<true> : sgd_update_kernel<false>, dim3((unsigned)p.C), dim3(kSgdThreads), 0,
                       stream, p);
    return hipGetLastError();
}

int plan_string_sgd(int C, bool has_momentum, char* buf, size_t cap) {
    return snprintf(buf, cap, "sgd_sqsum/%d/%d,sgd_update<%s>/%d/%d", kSgdChunk, C, has_momentum ? "mom" : "plain", kSgdChunk, C);
}

}  // namespace ge2e
