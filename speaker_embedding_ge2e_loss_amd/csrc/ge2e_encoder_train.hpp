// Layouts and launchers of the encoder's TRAINING path (ge2e_encoder_train.hip; the forward with a tape is the second
// instantiation of encode_kernel in ge2e_encoder.hip): ge2e_encode_train, ge2e_encoder_pack_bwd, ge2e_encode_bwd.
//
//   tape       what the backward reads, ALL of it stored (nothing is recomputed but tanh(c_t)): six planes per layer --
//              the gate activations i, f, g, o, the cell c and the hidden state h -- each [T][R][H], then the raw
//              projection y [R][D]; EncTape below is the index map, the only one.
//              6 L H T 4 bytes a window (+ 4 D): 2.9 MB at 3 x 256, T = 160, i.e. 24 GB at R = 8192.  h [T R][H] of a
//              layer is one contiguous matrix over k = t R + r: the weight-gradient GEMM's B operand as it lies.
//   bwd pack   per layer the matrix [4 H][C] (C = 2 H: weight_ih | weight_hh; layer 0: C = H, weight_hh alone -- no
//              gradient goes to the mels), rows in torch's own gate order, as [group of 16 k][column tile][lane][4]: the
//              B operand of d[input | h_prev] = dz W, 16 contiguous bytes per lane and group.  Then the projection
//              [pad16(D)][H] likewise, rows past D zero.
//   workspace  dZ [L][T R][4 H] (torch's gate order), dY [R][D], then the K-slice partials [S][flat] of the weight
//              gradients, each slice in the flat buffer's own layout; offsets rounded up to 64 floats.
#pragma once
#include "ge2e_encoder.hpp"

namespace ge2e {

constexpr int kEncBwdTile = 16;          // rows (windows) of a workgroup of the backward recurrence
constexpr int kEncBwdPad = 4;            // floats between the rows of the dz plane in LDS: b128 reads of 16 rows miss each other
constexpr int kWgradThreads = 256;       // four waves: an output block of 64 x 64, wave w owns rows 16 w .. 16 w + 15
constexpr int kWgradBlock = 64;
constexpr int kWgradSliceMin = 512;      // k = (t, r) pairs of a slice while there are at most kWgradMaxSlices of them
constexpr int kWgradMaxSlices = 32;

// The tape as the kernels and the launcher address it: plane stride T R H, a frame R H, planes named.  c_{t-1} is
// plane C at t - 1: a kernel addresses one element with enc_tape_at and its neighbours in other planes and frames with
// enc_tape_step from there (one 64-bit address per element, the steps uniform over the workgroup).
struct EncTape {
    enum Plane { I, F, G, O, C, Hid, kPlanes };
    size_t plane;
    int R, H, L;
};
__host__ __device__ inline EncTape enc_tape(long long R, int T, int H, int L) { return {(size_t)T * (size_t)R * H, (int)R, H, L}; }
__host__ __device__ inline size_t enc_tape_at(const EncTape& v, int l, int plane, long long t, long long r, int u) {
    return ((size_t)l * EncTape::kPlanes + plane) * v.plane + ((size_t)t * v.R + (size_t)r) * v.H + u;
}
__host__ __device__ inline ptrdiff_t enc_tape_step(const EncTape& v, int planes, int frames) {
    return planes * (ptrdiff_t)v.plane + frames * ((ptrdiff_t)v.R * v.H);
}
__host__ __device__ inline size_t enc_tape_y(const EncTape& v) { return (size_t)EncTape::kPlanes * v.L * v.plane; }   // y [R][D]
inline size_t encoder_tape_floats(long long R, int T, int H, int L, int D) { return enc_tape_y(enc_tape(R, T, H, L)) + (size_t)R * D; }
// A layer's block of the backward pack, in floats; where layer l starts (l = L: the projection); the whole of it.
__host__ __device__ inline size_t enc_bwd_layer_floats(int l, int H) { return (size_t)4 * H * (l ? 2 * H : H); }
__host__ __device__ inline size_t enc_bwd_pack_layer(int l, int H) {
    return l ? enc_bwd_layer_floats(0, H) + (size_t)(l - 1) * enc_bwd_layer_floats(1, H) : 0;
}
inline size_t encoder_packed_bwd_floats(int H, int L, int D) { return enc_bwd_pack_layer(L, H) + (size_t)enc_pad16(D) * H; }
// LDS of the backward recurrence: the dh planes [L][16][H] and the dz plane [16][4 H + 4] (the projection's dy
// [16][pad16(D) + 4] lies in it before the first step).  H = 256, L = 4: 64 KiB + 64.25 KiB of the CU's 160.
inline size_t encoder_bwd_lds_bytes(int H, int L) {
    return sizeof(float) * ((size_t)L * kEncBwdTile * H + (size_t)kEncBwdTile * (4 * H + kEncBwdPad));
}
// The K-slices of a weight-gradient GEMM over K pairs: their length (a multiple of 4) and their number, from K alone.
inline long long wgrad_slice_len(long long K) {
    long long s = (K + kWgradSliceMin - 1) / kWgradSliceMin;
    if (s > kWgradMaxSlices) s = kWgradMaxSlices;
    const long long len = (K + s - 1) / s;
    return (len + 3) & ~3LL;
}
inline int wgrad_slices(long long K) { const long long len = wgrad_slice_len(K); return (int)((K + len - 1) / len); }

inline size_t enc_round64(size_t n) { return (n + 63) & ~(size_t)63; }
struct EncBwdWorkspace { size_t dz, dy, partial, total; int slices; };   // offsets and the total in floats
inline EncBwdWorkspace encoder_bwd_workspace(long long R, int T, int n_mels, int H, int L, int D) {
    EncBwdWorkspace w;
    const int s_lstm = wgrad_slices(R * T), s_proj = wgrad_slices(R);
    w.slices = s_lstm > s_proj ? s_lstm : s_proj;
    w.dz = 0;
    w.dy = enc_round64((size_t)L * T * (size_t)R * 4 * H);
    w.partial = w.dy + enc_round64((size_t)R * D);
    w.total = w.partial + (size_t)w.slices * enc_round64(encoder_flat_floats(n_mels, H, L, D));
    return w;
}

struct ProblemEncodeBwd {
    const float* packed_bwd;
    const float* mel;
    const long long* row_start;
    const float* tape;
    const float* d_out;           // [R][D]
    float* d_flat;                // the flat gradient buffer, torch's layout
    float* ws;
    int R, T, n_mels, L, D, normalize;
    float *dz, *dy;               // the workspace's dZ and dY (set by the launcher)
};

hipError_t launch_encoder_pack_bwd(const float* flat, int n_mels, int H, int L, int D, float* packed, hipStream_t stream);
hipError_t launch_encode_train(const ProblemEncode& p, int H, hipStream_t stream);   // (ge2e_encoder.hip; p.tape set)
hipError_t launch_encode_bwd(const ProblemEncodeBwd& p, int H, hipStream_t stream);
// "encode_bwd<H>/tiles,encode_wgrad<H>/blocks x slices" per layer and for the projection, then "encode_reduce/blocks".
int plan_string_encode_bwd(int R, int T, int n_mels, int H, int L, int D, char* buf, size_t cap);
int plan_string_encode_train(int R, int H, char* buf, size_t cap);

}  // namespace ge2e
