// ge2e_encoder_pack_bwd / ge2e_encode_bwd: the backward pass of the d-vector encoder (ge2e_encoder.hip is the forward; its
// kTape instantiation leaves the tape this file reads), float32, exact fp32 on the matrix core (v_mfma_f32_16x16x4_f32).
//   recurrence  encode_bwd_kernel: one 512-thread workgroup owns 16 rows for all frames (downwards) and all layers
//               (downwards inside a frame); no workgroup waits for another.  Opens with the norm's and the projection's
//               backward: dy = (g - e (e.g)) / |y| (no epsilon, s2:34), dh_top = dy Wp.  Per layer-step: a lane reads
//               the saved gates and cells of its units (the forward's ownership map: wave w the units w H/8 .., lane
//               unit l15 of a block, rows 4 q + v), holds dc in registers, forms dz = (di, df, dg, do), writes it to
//               the dZ planes in global memory and to LDS [16][4 H + 4] as the A operand of d[input | h_prev] = dz W
//               (K = 4 H; the transposed pack, 16 contiguous bytes per lane and group).  The gradient into layer l - 1
//               at frame t is the recurrent part from frame t + 1 plus the input gradient of layer l at frame t: one LDS
//               plane per layer, the input half's accumulators initialised FROM the plane, the recurrent half's written
//               over the plane of the layer itself.  Two barriers per layer-step.  Layer 0 has the recurrent half alone.
//   weights     encode_wgrad_kernel: dW_l [4 H][I_l + H] = sum over k = (t, r) of dz^T [in | h_prev], a GEMM with
//               K = R T straight from the dZ planes and the tape (layer 0's input from the mels through the same row
//               addressing); an output block of 64 x 64 times a K-slice per workgroup, the slice count from the shape
//               alone.  The blocks of the first column also sum dZ's columns (an MFMA against ones): the bias gradient.
//               The projection's dW = dy^T h_top and db = sum dy are the same kernel with K = R.  Partials go to the
//               workspace, one flat-buffer image per slice.
//   reduce      encode_reduce_kernel: every element of the flat gradient buffer is the sum of its slices in ascending
//               order, written once (bias_hh reads bias_ih's partials).  No atomics: the same bits on every call.
// Index maps: ge2e_encoder_train.hpp (tape, backward pack), ge2e_encoder.hpp (flat buffer, fragments); the K loop: enc_contract.
// Pad rows of the last tile: dy = 0 and every saved value reads as 0, so their dz are exact zeros in LDS and nothing of
// them is stored.  A row whose upstream gradient is zero has dy = 0, dh = 0 and dc = 0: exact zeros in every dz.
#include "ge2e_encoder_train.hpp"

#include <math.h>

#include "ge2e_encoder_dev.hpp"
#include "ge2e_plan.hpp"

namespace ge2e {

namespace {

__global__ __launch_bounds__(256) void encoder_pack_bwd_kernel(const float* __restrict__ flat, int n_mels, int H, int L, int D,
                                                                float* __restrict__ packed, size_t total) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        int l = 0;
        while (l < L && idx >= enc_bwd_pack_layer(l + 1, H)) ++l;
        const EncFragIdx e = enc_frag_decode(idx - enc_bwd_pack_layer(l, H), (l == 0 || l == L ? H : 2 * H) / 16);
        const int k = e.k, col = e.tile * 16 + e.l15;
        float val;
        if (l < L) {
            const EncFlatLayer f = enc_flat_layer(l, n_mels, H);
            if (l == 0) val = flat[f.w_hh + (size_t)k * H + col];
            else val = col < H ? flat[f.w_ih + (size_t)k * H + col] : flat[f.w_hh + (size_t)k * H + (col - H)];
        } else {
            val = k < D ? flat[enc_flat_proj(n_mels, H, L, D).w + (size_t)k * H + col] : 0.f;
        }
        packed[idx] = val;
    }
}

template <int H>
__global__ __launch_bounds__(kEncThreads) void encode_bwd_kernel(ProblemEncodeBwd p) {
    extern __shared__ __attribute__((aligned(16))) float bwd_lds[];
    constexpr int UB = H / 128, ZS = 4 * H + kEncBwdPad, G = 4 * H / 16;
    static_assert(H == 128 || H == 256, "a wave owns one or two blocks of 16 units");
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int l15 = lane & 15, q = lane >> 4;
    const int L = p.L, T = p.T, D = p.D, R = p.R;
    const int Dp = enc_pad16(D), YS = Dp + kEncBwdPad;
    const long long r0 = (long long)blockIdx.x * kEncBwdTile;
    const size_t RH = (size_t)R * H;
    const EncTape tape = enc_tape(R, T, H, L);
    const v4f zero4 = {0.f, 0.f, 0.f, 0.f};
    float* dh = bwd_lds;                                   // [L][16][H]
    float* dzs = bwd_lds + (size_t)L * kEncBwdTile * H;    // [16][ZS]; before the first step dy [16][YS]

    for (int i = threadIdx.x; i < L * kEncBwdTile * H; i += kEncThreads) dh[i] = 0.f;

    // the norm's backward, one wave per two rows: dy into LDS (zero past D and for pad rows) and into the workspace
    const float* ytape = p.tape + enc_tape_y(tape);
    for (int i = 0; i < kEncBwdTile / 8; ++i) {
        const int tr = wid * (kEncBwdTile / 8) + i;
        const long long r = r0 + tr;
        if (r < R) {   // (uniform over the wave)
            const float* yr = ytape + (size_t)r * D;
            const float* gr = p.d_out + (size_t)r * D;
            float n = 1.f, eg = 0.f;
            if (p.normalize) {
                float ss = 0.f;
                for (int d = lane; d < D; d += kWave) ss += yr[d] * yr[d];
                ss = wave_sum(ss);
                n = sqrtf(ss);
                for (int d = lane; d < D; d += kWave) eg += (yr[d] / n) * gr[d];
                eg = wave_sum(eg);
            }
            for (int d = lane; d < Dp; d += kWave) {
                float v = 0.f;
                if (d < D) {
                    v = p.normalize ? (gr[d] - (yr[d] / n) * eg) / n : gr[d];
                    p.dy[(size_t)r * D + d] = v;
                }
                dzs[tr * YS + d] = v;
            }
        } else {
            for (int d = lane; d < Dp; d += kWave) dzs[tr * YS + d] = 0.f;
        }
    }
    __syncthreads();

    // the projection's backward: dh of the top layer at the last frame = dy Wp, K = pad16(D)
    {
        const float* wp = p.packed_bwd + enc_bwd_pack_layer(L, H);
        v4f acc[UB][1];
#pragma unroll
        for (int ub = 0; ub < UB; ++ub) acc[ub][0] = zero4;
        auto afrag = [&](int g, int) -> v4f { return *reinterpret_cast<const v4f*>(dzs + l15 * YS + 16 * g + 4 * q); };
        enc_contract<1, UB, 1>(wp + enc_frag_slot(0, H / 16, wid * UB, lane), enc_frag_slot(1, H / 16, 0, 0), Dp / 16, afrag, acc);
        float* top = dh + (size_t)(L - 1) * kEncBwdTile * H;
#pragma unroll
        for (int ub = 0; ub < UB; ++ub)
#pragma unroll
            for (int v = 0; v < 4; ++v) top[(4 * q + v) * H + (wid * UB + ub) * 16 + l15] = acc[ub][0][v];
    }
    __syncthreads();   // dy has been read, the top plane is there

    v4f dc[kEncMaxLayers][UB];
#pragma unroll
    for (int l = 0; l < kEncMaxLayers; ++l)
#pragma unroll
        for (int ub = 0; ub < UB; ++ub) dc[l][ub] = zero4;

    for (int t = T - 1; t >= 0; --t) {
        static_for<0, kEncMaxLayers>([&](auto lc) {
            constexpr int l = kEncMaxLayers - 1 - decltype(lc)::value;
            if (l < L) {
                float* dhl = dh + (size_t)l * kEncBwdTile * H;
                // ---- dz of the lane's cells from dh, dc and the tape ----
                const float* tl = p.tape + enc_tape_at(tape, l, EncTape::I, t, 0, 0);   // (uniform: the layer's frame t)
                float* dzl = p.dz + ((size_t)l * T + t) * RH * 4;
#pragma unroll
                for (int ub = 0; ub < UB; ++ub)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const int tr = 4 * q + v, u = (wid * UB + ub) * 16 + l15;
                        const long long r = r0 + tr;
                        float dzi = 0.f, dzf = 0.f, dzg = 0.f, dzo = 0.f;
                        if (r < R) {
                            const float dhv = dhl[tr * H + u];
                            const float* tp = tl + enc_tape_at(tape, 0, EncTape::I, 0, r, u);
                            auto saved = [&](int plane, int frames) { return tp[enc_tape_step(tape, plane, frames)]; };
                            const float ig = saved(EncTape::I, 0), fg = saved(EncTape::F, 0), gg = saved(EncTape::G, 0);
                            const float og = saved(EncTape::O, 0), cn = saved(EncTape::C, 0), cprev = t > 0 ? saved(EncTape::C, -1) : 0.f;
                            const float tc = tanhf(cn);
                            const float dcv = dc[l][ub][v] + dhv * og * (1.0f - tc * tc);
                            dzi = dcv * gg * (ig * (1.0f - ig));
                            dzf = dcv * cprev * (fg * (1.0f - fg));
                            dzg = dcv * ig * (1.0f - gg * gg);
                            dzo = dhv * tc * (og * (1.0f - og));
                            dc[l][ub][v] = dcv * fg;
                            float* zp = dzl + (size_t)r * 4 * H + u;
                            zp[0] = dzi;
                            zp[H] = dzf;
                            zp[2 * H] = dzg;
                            zp[3 * H] = dzo;
                        }
                        float* zs = dzs + tr * ZS + u;
                        zs[0] = dzi;
                        zs[H] = dzf;
                        zs[2 * H] = dzg;
                        zs[3 * H] = dzo;
                    }
                __syncthreads();   // the dz plane is whole; every lane has read its dh
                // ---- d[input | h_prev] = dz W: column tiles wid NTB .. of C / 16, the input half first ----
                constexpr int C = l ? 2 * H : H, CT = C / 16, NTB = CT / 8;
                const float* wl = p.packed_bwd + enc_bwd_pack_layer(l, H) + enc_frag_slot(0, CT, wid * NTB, lane);
                float* dst[NTB];
                v4f acc[NTB];
#pragma unroll
                for (int j = 0; j < NTB; ++j) {
                    const int col = (wid * NTB + j) * 16 + l15;
                    const bool input = l > 0 && col < H;
                    dst[j] = input ? dh + (size_t)(l > 0 ? l - 1 : 0) * kEncBwdTile * H + col : dhl + (col - (l ? H : 0));
#pragma unroll
                    for (int v = 0; v < 4; ++v) acc[j][v] = input ? dst[j][(4 * q + v) * H] : 0.f;
                }
                const float* arow = dzs + l15 * ZS + 4 * q;
                // This site keeps its own K loop, enc_contract's for one row half and one chunk: through the shared function
                // the training step measured 0.6 .. 0.8 ms (1.2 %) above the parent's in two sets
                // (profiles/encoder_refactor_ab.txt, 5a).  The same order for every accumulator: g ascending, i = 0 .. 3.
                v4f an = *reinterpret_cast<const v4f*>(arow), bn[NTB];
#pragma unroll
                for (int j = 0; j < NTB; ++j) bn[j] = *reinterpret_cast<const v4f*>(wl + (size_t)j * kEncFragTile);
#pragma clang loop unroll(disable)
                for (int g = 0; g < G; ++g) {
                    const v4f ac = an;
                    v4f bc[NTB];
#pragma unroll
                    for (int j = 0; j < NTB; ++j) bc[j] = bn[j];
                    if (g + 1 < G) {
                        an = *reinterpret_cast<const v4f*>(arow + 16 * (g + 1));
#pragma unroll
                        for (int j = 0; j < NTB; ++j) bn[j] = *reinterpret_cast<const v4f*>(wl + enc_frag_slot(g + 1, CT, j, 0));
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < NTB; ++j) acc[j] = mfma_f32(ac[i], bc[j][i], acc[j]);
                }
#pragma unroll
                for (int j = 0; j < NTB; ++j)
#pragma unroll
                    for (int v = 0; v < 4; ++v) dst[j][(4 * q + v) * H] = acc[j][v];
                __syncthreads();   // the planes are whole; the dz plane is free
            }
        });
    }
}

// One weight-gradient GEMM: out [M][N0 + N1] = sum over k of A[k][m] * [B0 | B1][k][n], and the column sums of A.
struct WgradJob {
    const float* A;               // [K][lda], m < M
    const float* B0;              // part 0, n < N0: [K][ldb0], or the mels through the row addressing (mel_part)
    const float* B1;              // part 1: row k is B1[k - shift], zero for k < shift
    const long long* row_start;
    float* partial;               // [slices][pstride], each a flat-buffer image
    long long K, slice_len, shift;
    size_t pstride, out0, out1, outb;   // flat offsets of part 0 (row stride N0), part 1 (row stride N1), the column sums
    int lda, M, ldb0, N0, N1, mel_part, R, T;
};

__global__ __launch_bounds__(kWgradThreads) void encode_wgrad_kernel(WgradJob p) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int l15 = lane & 15, q = lane >> 4;
    const int m = blockIdx.y * kWgradBlock + wid * 16 + l15;
    const long long k0 = (long long)blockIdx.z * p.slice_len;
    const long long k1 = k0 + p.slice_len < p.K ? k0 + p.slice_len : p.K;
    const bool mok = m < p.M, sums = blockIdx.x == 0;
    const int N = p.N0 + p.N1;
    int n[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) n[j] = blockIdx.x * kWgradBlock + j * 16 + l15;
    const v4f zero4 = {0.f, 0.f, 0.f, 0.f};
    v4f acc[4] = {zero4, zero4, zero4, zero4}, accb = zero4;
    for (long long kk = k0; kk < k1; kk += 4) {
        const long long k = kk + q;
        const bool kv = k < k1;
        const float a = (kv && mok) ? p.A[(size_t)k * p.lda + m] : 0.f;
        size_t melrow = 0;
        if (p.mel_part && kv) {
            const long long t = k / p.R, r = k - t * p.R;
            melrow = (size_t)((p.row_start ? p.row_start[r] : r * p.T) + t) * p.N0;
        }
        float b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            b[j] = 0.f;
            if (kv && n[j] < N) {
                if (n[j] < p.N0) b[j] = p.mel_part ? p.B0[melrow + n[j]] : p.B0[(size_t)k * p.ldb0 + n[j]];
                else if (k >= p.shift) b[j] = p.B1[(size_t)(k - p.shift) * p.N1 + (n[j] - p.N0)];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = mfma_f32(a, b[j], acc[j]);
        if (sums) accb = mfma_f32(a, 1.0f, accb);
    }
    float* out = p.partial + (size_t)blockIdx.z * p.pstride;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int mo = blockIdx.y * kWgradBlock + wid * 16 + 4 * q + v;
        if (mo >= p.M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (n[j] < p.N0) out[p.out0 + (size_t)mo * p.N0 + n[j]] = acc[j][v];
            else if (n[j] < N) out[p.out1 + (size_t)mo * p.N1 + (n[j] - p.N0)] = acc[j][v];
        }
        if (sums && l15 == 0) out[p.outb + mo] = accb[v];
    }
}

__global__ __launch_bounds__(256) void encode_reduce_kernel(const float* __restrict__ partial, size_t pstride, int s_lstm,
                                                             int s_proj, int n_mels, int H, int L, size_t total,
                                                             float* __restrict__ d_flat) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        size_t src = idx;
        int S = s_proj;
        for (int l = 0; l < L; ++l) {
            const EncFlatLayer f = enc_flat_layer(l, n_mels, H);
            if (idx < f.end) {
                S = s_lstm;
                if (idx >= f.b_hh) src = idx - (f.b_hh - f.b_ih);   // bias_hh = bias_ih
                break;
            }
        }
        float sum = partial[src];
        for (int s = 1; s < S; ++s) sum += partial[(size_t)s * pstride + src];
        d_flat[idx] = sum;
    }
}

KernelLaunchState g_encode_bwd_state[2];

dim3 wgrad_grid(int M, int N, long long K) {
    return dim3((unsigned)enc_tiles(N, kWgradBlock), (unsigned)enc_tiles(M, kWgradBlock), (unsigned)wgrad_slices(K));
}
}  // namespace

hipError_t launch_encoder_pack_bwd(const float* flat, int n_mels, int H, int L, int D, float* packed, hipStream_t stream) {
    const size_t total = encoder_packed_bwd_floats(H, L, D);
    hipLaunchKernelGGL(encoder_pack_bwd_kernel, dim3(reduce_blocks(total)), dim3(256), 0, stream, flat, n_mels, H, L, D, packed,
                       total);
    return hipGetLastError();
}

hipError_t launch_encode_bwd(const ProblemEncodeBwd& p0, int H, hipStream_t stream) {
    ProblemEncodeBwd p = p0;
    const EncBwdWorkspace ws = encoder_bwd_workspace(p.R, p.T, p.n_mels, H, p.L, p.D);
    p.dz = p.ws + ws.dz;
    p.dy = p.ws + ws.dy;
    hipError_t err = launch_for_h(H, encode_bwd_kernel<128>, encode_bwd_kernel<256>, g_encode_bwd_state,
                                  (unsigned)enc_tiles(p.R, kEncBwdTile), (unsigned)encoder_bwd_lds_bytes(H, p.L), p, stream);
    if (err != hipSuccess) return err;

    const long long K = (long long)p.R * p.T;
    const EncTape tape = enc_tape(p.R, p.T, H, p.L);
    const size_t total = encoder_flat_floats(p.n_mels, H, p.L, p.D);
    WgradJob j{};
    j.row_start = p.row_start;
    j.partial = p.ws + ws.partial;
    j.pstride = enc_round64(total);
    j.R = p.R;
    j.T = p.T;
    for (int l = 0; l < p.L; ++l) {
        const EncFlatLayer f = enc_flat_layer(l, p.n_mels, H);
        j.A = p.dz + (size_t)l * K * 4 * H;
        j.lda = j.M = 4 * H;
        j.K = K;
        j.slice_len = wgrad_slice_len(K);
        j.mel_part = l == 0;
        j.B0 = l ? p.tape + enc_tape_at(tape, l - 1, EncTape::Hid, 0, 0, 0) : p.mel;
        j.ldb0 = j.N0 = f.I;
        j.B1 = p.tape + enc_tape_at(tape, l, EncTape::Hid, 0, 0, 0);
        j.N1 = H;
        j.shift = p.R;
        j.out0 = f.w_ih;
        j.out1 = f.w_hh;
        j.outb = f.b_ih;
        hipLaunchKernelGGL(encode_wgrad_kernel, wgrad_grid(j.M, f.I + H, K), dim3(kWgradThreads), 0, stream, j);
        if ((err = hipGetLastError()) != hipSuccess) return err;
    }
    const EncFlatProj f = enc_flat_proj(p.n_mels, H, p.L, p.D);
    j.A = p.dy;
    j.lda = j.M = p.D;
    j.K = p.R;
    j.slice_len = wgrad_slice_len(p.R);
    j.mel_part = 0;
    j.B0 = p.tape + enc_tape_at(tape, p.L - 1, EncTape::Hid, p.T - 1, 0, 0);
    j.ldb0 = j.N0 = H;
    j.B1 = nullptr;
    j.N1 = 0;
    j.shift = 0;
    j.out0 = j.out1 = f.w;
    j.outb = f.b;
    hipLaunchKernelGGL(encode_wgrad_kernel, wgrad_grid(p.D, H, p.R), dim3(kWgradThreads), 0, stream, j);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    hipLaunchKernelGGL(encode_reduce_kernel, dim3(reduce_blocks(total)), dim3(256), 0, stream, (const float*)j.partial, j.pstride,
                       wgrad_slices(K), wgrad_slices(p.R), p.n_mels, H, p.L, total, p.d_flat);
    return hipGetLastError();
}

int plan_string_encode_bwd(int R, int T, int n_mels, int H, int L, int D, char* buf, size_t cap) {
    const long long K = (long long)R * T;
    Out o{buf, cap};
    o.add("encode_bwd<%d>/%d", H, enc_tiles(R, kEncBwdTile));
    for (int l = 0; l <= L; ++l) {
        const dim3 g = l < L ? wgrad_grid(4 * H, (l ? H : n_mels) + H, K) : wgrad_grid(D, H, R);
        o.add("encode_wgrad/%ux%ux%u", g.x, g.y, g.z);
    }
    o.add("encode_reduce/%u", reduce_blocks(encoder_flat_floats(n_mels, H, L, D)));
    return o.done();
}

}  // namespace ge2e
