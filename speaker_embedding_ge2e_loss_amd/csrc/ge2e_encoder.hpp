// Layout of the packed encoder weights + launchers of ge2e_encoder_pack / ge2e_encode (see ge2e_encoder.hip): the d-vector
// encoder's forward pass for inference, mel windows to embeddings in one launch.
#pragma once
#include "ge2e_common.hpp"

namespace ge2e {

constexpr int kEncTile = 32;        // rows (windows) of a workgroup
constexpr int kEncThreads = 512;    // eight waves, each owning H / 8 hidden units of every layer
constexpr int kEncMaxLayers = 4, kEncMaxMels = 256, kEncMaxDim = 256;

inline bool encoder_supported(int n_mels, int H, int L, int D) {
    return (H == 128 || H == 256) && L >= 1 && L <= kEncMaxLayers && n_mels >= 1 && n_mels <= kEncMaxMels && D >= 1 &&
           D <= kEncMaxDim;
}
__host__ __device__ inline int enc_pad16(int n) { return (n + 15) & ~15; }
// A layer's block of the packed buffer, in floats: the matrix [pad16(I) + H][4 H] in fragment order, then the 4 H summed
// biases.  I = n_mels for layer 0 and H above it.
__host__ __device__ inline size_t enc_layer_floats(int I, int H) { return (size_t)(enc_pad16(I) + H) * 4 * H + 4 * (size_t)H; }
// ... and the projection's: [H][pad16(D)] in fragment order, then pad16(D) biases.
__host__ __device__ inline size_t enc_proj_floats(int H, int D) { return (size_t)H * enc_pad16(D) + enc_pad16(D); }
inline size_t encoder_packed_floats(int n_mels, int H, int L, int D) {
    return enc_layer_floats(n_mels, H) + (size_t)(L - 1) * enc_layer_floats(H, H) + enc_proj_floats(H, D);
}
// The flat parameter buffer in torch's layout, in floats.
inline size_t encoder_flat_floats(int n_mels, int H, int L, int D) {
    return 4 * (size_t)H * (n_mels + H + 2) + (size_t)(L - 1) * 4 * H * (2 * (size_t)H + 2) + (size_t)D * H + D;
}
inline size_t encoder_lds_bytes(int H, int L, int D) {
    const size_t h = (size_t)L * kEncTile * H, y = (size_t)kEncTile * enc_pad16(D);
    return sizeof(float) * (h > y ? h : y);
}

struct ProblemEncode {
    const float* packed;
    const float* mel;             // [frames][n_mels]
    const long long* row_start;   // [R] first frame of every row, or null: row r starts at frame r T
    float* out;                   // [R][D]
    int R, T, n_mels, L, D, normalize;
    float* tape;                  // the training forward's tape (ge2e_encoder_train.hpp), or null: inference
};

hipError_t launch_encoder_pack(const float* flat, int n_mels, int H, int L, int D, float* packed, hipStream_t stream);
hipError_t launch_encode(const ProblemEncode& p, int H, hipStream_t stream);
// "encode<H>/tiles": the instantiation and its grid, snprintf-style.
int plan_string_encode(int R, int H, char* buf, size_t cap);

}  // namespace ge2e
