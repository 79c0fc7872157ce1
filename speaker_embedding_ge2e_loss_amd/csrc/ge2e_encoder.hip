// ge2e_encoder_pack / ge2e_encode: the d-vector encoder's forward pass for inference (s2:7-35: stacked LSTM over the frames of
// a window, the last frame's top hidden state through one Linear, L2-normalised), mel windows to embeddings in ONE launch.
//   tile      one 512-thread workgroup owns 32 rows (windows) for all T steps and all L layers; no workgroup waits for
//             another.  Time is the outer loop, layers the inner one.  Wave w owns the hidden units w H/8 .. (w+1) H/8 - 1 of
//             every layer (UB = H / 128 blocks of 16 units) and both 16-row halves of the tile.
//   operands  v_mfma_f32_16x16x4_f32, exact fp32 (ge2e_rows_dev.hpp has the operand map): A[i = l15][k = q] is the
//             activation of row l15, B[k = q][j = l15] the weight of gate column l15, C[i = 4 q + v][j = l15].  The k index
//             is permuted the same way in both operands: over the four steps of a GROUP of 16 k, lane group q takes
//             k = 16 g + 4 q + i in step i, so a lane fetches 16 contiguous bytes per operand and group.
//   packed    per layer the matrix [pad16(I) + H][4 H] (rows: the input's k, zero-padded to a multiple of 16, then the
//             recurrent k) as [group][column tile][lane][4]: one coalesced 1 KiB line per wave, group and tile.  Column
//             tile pc = (w UB + ub) 4 + gate holds the gate's columns of the 16 units of block ub of wave w, so i, f, g, o of
//             one unit land in the same lane and register slot of four accumulators and the cell update runs in
//             registers.  Then the 4 H biases b_ih + b_hh in the same column order.  The projection likewise:
//             [H][pad16(D)] and pad16(D) biases, zero past D.  (Every index map: ge2e_encoder.hpp; the K loop: enc_contract.)
//   state     c in registers (UB x 2 x 4 per layer), h of every layer in LDS [L][32][H]; x_t and the weights come from
//             global memory (L2) one group ahead of the MFMAs that use them.  Two barriers per layer-step: the old h of the
//             layer is read by every wave before any wave overwrites it.
//   epilogue  projection of the top layer's h into LDS [32][pad16(D)] (over the h planes), then one wave per four rows:
//             sum of squares in a fixed order, y / sqrt(ss) (no epsilon, s2:34: a zero row gives NaN) or y itself, stored.
// Every K chain has a fixed order and MFMA rows are independent: the bits of an output row depend on that row's frames and
// the weights alone.  Pad rows of the last tile compute on zeros and are never stored.
//   training  ge2e_encode_train is the SAME kernel in its kTape instantiation: the cell update also stores the gates, c and h,
//             the epilogue the raw projection, into the caller's tape (ge2e_encoder_train.hpp) for ge2e_encode_bwd.
#include "ge2e_encoder.hpp"
#include "ge2e_encoder_train.hpp"

#include <math.h>

#include "ge2e_encoder_dev.hpp"
#include "ge2e_plan.hpp"

namespace ge2e {

namespace {

// The row of torch's [4 H][..] gate matrices (gate order i, f, g, o) behind column l15 of packed column tile pc.
__device__ __forceinline__ int enc_gate_row(int pc, int l15, int H) {
    const int UB = H / 128, NT = 4 * UB;
    const int w = pc / NT, j = pc % NT;
    return (j & 3) * H + (w * UB + (j >> 2)) * 16 + l15;
}

__global__ __launch_bounds__(256) void encoder_pack_kernel(const float* __restrict__ flat, int n_mels, int H, int L, int D,
                                                            float* __restrict__ packed, size_t total) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        int l = 0;
        while (l < L && idx >= enc_pack_layer(l + 1, n_mels, H)) ++l;
        const size_t local = idx - enc_pack_layer(l, n_mels, H);
        float val;
        if (l < L) {
            const EncFlatLayer f = enc_flat_layer(l, n_mels, H);
            const int I = f.I, Ip = enc_pad16(I), C = 4 * H;
            const size_t wsz = (size_t)(Ip + H) * C;
            if (local < wsz) {
                const EncFragIdx e = enc_frag_decode(local, C / 16);
                const int k = e.k, row = enc_gate_row(e.tile, e.l15, H);
                if (k < Ip) val = k < I ? flat[f.w_ih + (size_t)row * I + k] : 0.f;
                else val = flat[f.w_hh + (size_t)row * H + (k - Ip)];
            } else {
                const int b = (int)(local - wsz), row = enc_gate_row(b >> 4, b & 15, H);
                val = flat[f.b_ih + row] + flat[f.b_hh + row];
            }
        } else {
            const EncFlatProj f = enc_flat_proj(n_mels, H, L, D);
            const int Dp = enc_pad16(D);
            const size_t wsz = (size_t)H * Dp;
            if (local < wsz) {
                const EncFragIdx e = enc_frag_decode(local, Dp / 16);
                const int d = e.tile * 16 + e.l15;
                val = d < D ? flat[f.w + (size_t)d * H + e.k] : 0.f;
            } else {
                const int d = (int)(local - wsz);
                val = d < D ? flat[f.b + d] : 0.f;
            }
        }
        packed[idx] = val;
    }
}

__device__ __forceinline__ float enc_sigmoid(float z) { return 1.0f / (1.0f + expf(-z)); }   // finite at z = +-100 and beyond

// kTape: the training forward.  The same kernel, and what the backward reads goes to p.tape on the way (layout:
// ge2e_encoder_train.hpp): the gate activations, c and h of every layer, frame and row, and the raw projection.
template <int H, bool kTape>
__global__ __launch_bounds__(kEncThreads) void encode_kernel(ProblemEncode p) {
    extern __shared__ __attribute__((aligned(16))) float enc_lds[];
    constexpr int UB = H / 128, NT = 4 * UB, CT = H / 4, GH = H / 16;
    static_assert(H == 128 || H == 256, "a wave owns one or two blocks of 16 units");
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int l15 = lane & 15, q = lane >> 4;
    const int L = p.L, T = p.T, n_mels = p.n_mels, D = p.D, R = p.R;
    const int Dp = enc_pad16(D), DT = Dp / 16, G0 = enc_pad16(n_mels) / 16;
    const bool vecX = (n_mels & 3) == 0;
    const v4f zero4 = {0.f, 0.f, 0.f, 0.f};
    float* hs = enc_lds;                                   // [L][32][H]

    for (int i = threadIdx.x; i < L * kEncTile * H; i += kEncThreads) hs[i] = 0.f;

    // the lane's two rows as the A operand: rows l15 and 16 + l15 of the tile
    const float* xrow[2];
    bool xok[2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
        const long long r = (long long)blockIdx.x * kEncTile + rt * 16 + l15;
        xok[rt] = r < R;
        const long long f0 = !xok[rt] ? 0 : (p.row_start ? p.row_start[r] : r * T);
        xrow[rt] = p.mel + (size_t)f0 * n_mels;
    }
    v4f c[kEncMaxLayers][UB][2];
#pragma unroll
    for (int l = 0; l < kEncMaxLayers; ++l)
#pragma unroll
        for (int ub = 0; ub < UB; ++ub) c[l][ub][0] = c[l][ub][1] = zero4;
    __syncthreads();

    const EncTape tape = enc_tape(R, T, H, L);
    for (int t = 0; t < T; ++t) {
        static_for<0, kEncMaxLayers>([&](auto lc) {
            constexpr int l = decltype(lc)::value;
            if (l < L) {
                const int Gin = l == 0 ? G0 : GH, G = Gin + GH;
                const float* wl = p.packed + enc_pack_layer(l, n_mels, H);
                const float* bias = wl + (size_t)G * 16 * 4 * H;
                v4f acc[NT][2];
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const float b = bias[(wid * NT + j) * 16 + l15];
                    acc[j][0] = acc[j][1] = v4f{b, b, b, b};
                }
                const float* hown = hs + (size_t)l * kEncTile * H;
                const float* hbelow = hs + (size_t)(l > 0 ? l - 1 : 0) * kEncTile * H;
                auto afrag = [&](int g, int rt) -> v4f {
                    if (g < Gin) {
                        if constexpr (l == 0) return load4(xrow[rt] + (size_t)t * n_mels, 16 * g + 4 * q, n_mels, xok[rt], vecX);
                        else return *reinterpret_cast<const v4f*>(hbelow + (rt * 16 + l15) * H + 16 * g + 4 * q);
                    }
                    return *reinterpret_cast<const v4f*>(hown + (rt * 16 + l15) * H + 16 * (g - Gin) + 4 * q);
                };
                enc_contract<2, 4, UB>(wl + enc_frag_slot(0, CT, wid * NT, lane), enc_frag_slot(1, CT, 0, 0), G, afrag, acc);
                // the cell update, in registers: the lane holds i, f, g, o of unit l15 of block ub for the rows 4 q + v
                v4f hnew[UB][2];
#pragma unroll
                for (int ub = 0; ub < UB; ++ub)
#pragma unroll
                    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            const float ig = enc_sigmoid(acc[4 * ub + 0][rt][v]), fg = enc_sigmoid(acc[4 * ub + 1][rt][v]);
                            const float gg = tanhf(acc[4 * ub + 2][rt][v]), og = enc_sigmoid(acc[4 * ub + 3][rt][v]);
                            const float cn = fg * c[l][ub][rt][v] + ig * gg;
                            c[l][ub][rt][v] = cn;
                            hnew[ub][rt][v] = og * tanhf(cn);
                            if constexpr (kTape) {
                                const long long r = (long long)blockIdx.x * kEncTile + rt * 16 + 4 * q + v;
                                if (r < R) {   // pad rows write nothing
                                    float* tp = p.tape + enc_tape_at(tape, l, EncTape::I, t, r, (wid * UB + ub) * 16 + l15);
                                    tp[enc_tape_step(tape, EncTape::I, 0)] = ig;
                                    tp[enc_tape_step(tape, EncTape::F, 0)] = fg;
                                    tp[enc_tape_step(tape, EncTape::G, 0)] = gg;
                                    tp[enc_tape_step(tape, EncTape::O, 0)] = og;
                                    tp[enc_tape_step(tape, EncTape::C, 0)] = cn;
                                    tp[enc_tape_step(tape, EncTape::Hid, 0)] = hnew[ub][rt][v];
                                }
                            }
                        }
                __syncthreads();   // every wave has read the layer's old h
                float* hw = hs + (size_t)l * kEncTile * H;
#pragma unroll
                for (int ub = 0; ub < UB; ++ub)
#pragma unroll
                    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                        for (int v = 0; v < 4; ++v)
                            hw[(rt * 16 + 4 * q + v) * H + (wid * UB + ub) * 16 + l15] = hnew[ub][rt][v];
                __syncthreads();   // ... and the new one is there for the layer above and for the next step
            }
        });
    }

    // projection of the top layer's h: column tiles wid and wid + 8 of pad16(D) / 16
    const float* wp = p.packed + enc_pack_layer(L, n_mels, H);
    const float* pbias = wp + (size_t)H * Dp;
    const float* htop = hs + (size_t)(L - 1) * kEncTile * H;
    v4f y[2][2];
#pragma unroll
    for (int jt = 0; jt < 2; ++jt) {
        const int dt = wid + 8 * jt;
        y[jt][0] = y[jt][1] = zero4;
        if (dt < DT) {   // (uniform over the wave)
            const float b = pbias[dt * 16 + l15];
            v4f acc[1][2];
            acc[0][0] = acc[0][1] = v4f{b, b, b, b};
            auto afrag = [&](int g, int rt) -> v4f {
                return *reinterpret_cast<const v4f*>(htop + (rt * 16 + l15) * H + 16 * g + 4 * q);
            };
            enc_contract<2, 1, 1>(wp + enc_frag_slot(0, DT, dt, lane), enc_frag_slot(1, DT, 0, 0), GH, afrag, acc);
            y[jt][0] = acc[0][0];
            y[jt][1] = acc[0][1];
        }
    }
    __syncthreads();   // the h planes are free: the raw projection goes over them
    float* ys = enc_lds;                                   // [32][Dp]
#pragma unroll
    for (int jt = 0; jt < 2; ++jt) {
        const int dt = wid + 8 * jt;
        if (dt < DT)
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int v = 0; v < 4; ++v) ys[(rt * 16 + 4 * q + v) * Dp + dt * 16 + l15] = y[jt][rt][v];
    }
    __syncthreads();
    // one wave per four rows: the row's norm in a fixed order, then the store
    for (int i = 0; i < kEncTile / 8; ++i) {
        const int tr = wid * (kEncTile / 8) + i;
        const long long r = (long long)blockIdx.x * kEncTile + tr;
        if (r >= R) break;   // (uniform over the wave)
        const float* yr = ys + tr * Dp;
        float ss = 0.f;
        for (int d = lane; d < D; d += kWave) ss += yr[d] * yr[d];
        ss = wave_sum(ss);
        const float n = sqrtf(ss);
        float* o = p.out + (size_t)r * D;
        for (int d = lane; d < D; d += kWave) o[d] = p.normalize ? yr[d] / n : yr[d];
        if constexpr (kTape) {
            float* ty = p.tape + enc_tape_y(tape) + (size_t)r * D;
            for (int d = lane; d < D; d += kWave) ty[d] = yr[d];
        }
    }
}

KernelLaunchState g_encode_state[2][2];

template <bool kTape>
hipError_t launch_encode_as(const ProblemEncode& p, int H, hipStream_t stream) {
    return launch_for_h(H, encode_kernel<128, kTape>, encode_kernel<256, kTape>, g_encode_state[kTape],
                        (unsigned)enc_tiles(p.R, kEncTile), (unsigned)encoder_lds_bytes(H, p.L, p.D), p, stream);
}
}  // namespace

hipError_t launch_encoder_pack(const float* flat, int n_mels, int H, int L, int D, float* packed, hipStream_t stream) {
    const size_t total = encoder_packed_floats(n_mels, H, L, D);
    hipLaunchKernelGGL(encoder_pack_kernel, dim3(reduce_blocks(total)), dim3(256), 0, stream, flat, n_mels, H, L, D, packed, total);
    return hipGetLastError();
}

hipError_t launch_encode(const ProblemEncode& p, int H, hipStream_t stream) { return launch_encode_as<false>(p, H, stream); }
hipError_t launch_encode_train(const ProblemEncode& p, int H, hipStream_t stream) { return launch_encode_as<true>(p, H, stream); }

static int plan_string_tiles(const char* kernel, int R, int H, char* buf, size_t cap) {
    Out o{buf, cap};
    o.add("%s<%d>/%d", kernel, H, enc_tiles(R, kEncTile));
    return o.done();
}
int plan_string_encode(int R, int H, char* buf, size_t cap) { return plan_string_tiles("encode", R, H, buf, cap); }
int plan_string_encode_train(int R, int H, char* buf, size_t cap) { return plan_string_tiles("encode_train", R, H, buf, cap); }

}  // namespace ge2e
