// Layouts of the encoder's parameter buffers + launchers of ge2e_encoder_pack / ge2e_encode (see ge2e_encoder.hip): the
// d-vector encoder's forward pass for inference, mel windows to embeddings in one launch.  Each layout is described ONCE
// here (the training path's in ge2e_encoder_train.hpp); kernels and launchers of both encoder sources read these functions.
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
inline int enc_tiles(long long R, int tile) { return (int)((R + tile - 1) / tile); }   // workgroups of `tile` rows over R
inline unsigned reduce_blocks(size_t total) { return (unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096); }

// The flat parameter buffer in torch's layout, float offsets: per layer weight_ih [4 H][I] (I = n_mels for layer 0 and H
// above it), weight_hh [4 H][H], bias_ih [4 H], bias_hh [4 H]; then the projection's weight [D][H] and bias [D].
struct EncFlatLayer { size_t w_ih, w_hh, b_ih, b_hh, end; int I; };
__host__ __device__ inline EncFlatLayer enc_flat_layer(int l, int n_mels, int H) {
    const size_t C = 4 * (size_t)H, I = l ? H : n_mels;
    const size_t w_ih = l ? C * (n_mels + H + 2) + (size_t)(l - 1) * C * (2 * H + 2) : 0;   // (the layers below, whole)
    const size_t w_hh = w_ih + C * I, b_ih = w_hh + C * H;
    return {w_ih, w_hh, b_ih, b_ih + C, b_ih + 2 * C, (int)I};
}
struct EncFlatProj { size_t w, b, end; };
__host__ __device__ inline EncFlatProj enc_flat_proj(int n_mels, int H, int L, int D) {
    const size_t w = enc_flat_layer(L - 1, n_mels, H).end, b = w + (size_t)D * H;
    return {w, b, b + D};
}
inline size_t encoder_flat_floats(int n_mels, int H, int L, int D) { return enc_flat_proj(n_mels, H, L, D).end; }

// The fragment order of every packed matrix [K][tiles * 16], both packs: [group of 16 k][tile][lane][4], one coalesced
// 1 KiB line per wave, group and tile.  Over the four MFMA steps of a group, lane group q = lane >> 4 takes
// k = 16 g + 4 q + i in step i, so a lane fetches 16 contiguous bytes per group and tile.
constexpr int kEncFragTile = 256;   // floats of one (group, tile): 64 lanes x 4
struct EncFragIdx { int k, tile, l15; };
// ... what lies at float `local` of such a matrix: row k, column l15 of column tile `tile`
__host__ __device__ inline EncFragIdx enc_frag_decode(size_t local, int tiles) {
    const int i = (int)(local & 3), lane = (int)((local >> 2) & 63), rest = (int)(local / kEncFragTile);
    return {16 * (rest / tiles) + 4 * (lane >> 4) + i, rest % tiles, lane & 15};
}
// ... and where a lane's 16 bytes of (group, tile) lie
__host__ __device__ inline size_t enc_frag_slot(int g, int tiles, int tile, int lane) {
    return ((size_t)g * tiles + tile) * kEncFragTile + (size_t)lane * 4;
}

// A layer's block of the packed buffer, in floats: the matrix [pad16(I) + H][4 H] in fragment order, then the 4 H summed
// biases.  I = n_mels for layer 0 and H above it.
__host__ __device__ inline size_t enc_layer_floats(int I, int H) { return (size_t)(enc_pad16(I) + H) * 4 * H + 4 * (size_t)H; }
// ... and the projection's: [H][pad16(D)] in fragment order, then pad16(D) biases.
__host__ __device__ inline size_t enc_proj_floats(int H, int D) { return (size_t)H * enc_pad16(D) + enc_pad16(D); }
// Where layer l starts in the packed buffer; l = L: the projection.
__host__ __device__ inline size_t enc_pack_layer(int l, int n_mels, int H) {
    return l ? enc_layer_floats(n_mels, H) + (size_t)(l - 1) * enc_layer_floats(H, H) : 0;
}
inline size_t encoder_packed_floats(int n_mels, int H, int L, int D) { return enc_pack_layer(L, n_mels, H) + enc_proj_floats(H, D); }
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
