// What the two encoder sources (ge2e_encoder.hip, ge2e_encoder_train.hip) share beyond their layouts: the contraction of
// a wave's column tiles over groups of 16 k, and the launch of a kernel that is instantiated for H = 128 and 256.
#pragma once
#include "ge2e_encoder.hpp"
#include "ge2e_rows_dev.hpp"

namespace ge2e {

// The wave's column tiles against RH row halves over G groups of 16 k, in NCG chunks of TPC tiles per group.  `bw`: the
// lane's slot (enc_frag_slot) of the wave's first tile in group 0, groups `gstride` floats apart; `afrag(g, rt)`: the
// lane's four activations of row half rt; `acc`: the caller's accumulators, initialised.  The weights of the next chunk
// and the activations of the next group are fetched before the MFMAs of the current chunk.  Every accumulator takes its
// MFMAs in ONE order, groups ascending and i = 0 .. 3 inside a group: the bits of the encoder depend on that.
template <int RH, int TPC, int NCG, class AFrag>
__device__ __forceinline__ void enc_contract(const float* bw, size_t gstride, int G, AFrag&& afrag, v4f (&acc)[NCG * TPC][RH]) {
    v4f bn[TPC], an[RH];
#pragma unroll
    for (int j = 0; j < TPC; ++j) bn[j] = *reinterpret_cast<const v4f*>(bw + (size_t)j * kEncFragTile);
#pragma unroll
    for (int rt = 0; rt < RH; ++rt) an[rt] = afrag(0, rt);
#pragma clang loop unroll(disable)
    for (int g = 0; g < G; ++g) {
        v4f ac[RH];
#pragma unroll
        for (int rt = 0; rt < RH; ++rt) ac[rt] = an[rt];
        const bool more = g + 1 < G;
        if (more) {
#pragma unroll
            for (int rt = 0; rt < RH; ++rt) an[rt] = afrag(g + 1, rt);
        }
        static_for<0, NCG>([&](auto uc) {
            constexpr int u = decltype(uc)::value;
            v4f bc[TPC];
#pragma unroll
            for (int j = 0; j < TPC; ++j) bc[j] = bn[j];
            if (u + 1 < NCG || more) {
                const float* nb = u + 1 < NCG ? bw + (size_t)g * gstride + (size_t)(u + 1) * TPC * kEncFragTile
                                              : bw + (size_t)(g + 1) * gstride;
#pragma unroll
                for (int j = 0; j < TPC; ++j) bn[j] = *reinterpret_cast<const v4f*>(nb + (size_t)j * kEncFragTile);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < TPC; ++j)
#pragma unroll
                    for (int rt = 0; rt < RH; ++rt)
                        acc[u * TPC + j][rt] = mfma_f32(ac[rt][i], bc[j][i], acc[u * TPC + j][rt]);
        });
    }
}

// Prepares (once per instantiation: `state`) and launches k128 or k256, whichever H names, on `tiles` workgroups.
template <class P>
static hipError_t launch_for_h(int H, void (*k128)(P), void (*k256)(P), KernelLaunchState (&state)[2], unsigned tiles, unsigned lds,
                               const P& p, hipStream_t stream) {
    void (*const fn)(P) = H == 256 ? k256 : k128;
    const hipError_t err = prepare_kernel(state[H == 256], (const void*)fn, kEncThreads, lds, nullptr);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(fn, dim3(tiles), dim3(kEncThreads), lds, stream, p);
    return hipGetLastError();
}

}  // namespace ge2e
