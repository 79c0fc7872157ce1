// ge2e_melspec_pack / ge2e_melspec: the mel front end (s0:29-66, 201-219: reflect pad, overlapping frames, periodic Hann
// window, |rfft|, the mel basis, 20 log10 and the clip), waveforms to frames of [total_frames][n_mels] in ONE launch.
//   tile      one 512-thread workgroup owns 16 consecutive rows (frames) of out; a row finds its utterance in frame_start
//             (last_not_above, ge2e_common.hpp).  Wave w transforms rows w and w + 8, then owns column tile w of the mel
//             product.
//   gather    sample n of frame f of an utterance is x[reflect(f hop + n - n_fft / 2)] of the signal extended with zeros to
//             its padded length; reflection, extension and the utterance's offset are address arithmetic, and a sample at
//             or past utt_len is never read.  (x gain) window[n], two samples as one complex point.
//   transform the n_fft real samples as H = n_fft / 2 complex points z[j] = x[2 j] + i x[2 j + 1]: a Stockham autosort FFT
//             in radix-8 and radix-4 passes (128 = 8 4 4, 256 = 8 8 4, 512 = 8 8 8, 1024 = 8 8 4 4) whose butterflies are
//             held in registers: pass with radix R at sub-length Ns takes z[j + r H / R], r < R, of butterfly j < H / R,
//             turns them by exp(-2 pi i r k / (Ns R)), k = j mod Ns, and leaves the R outputs at (j - k) R + k + r Ns.  The
//             first pass takes its points straight from the gather; between passes the points go through the wave's two
//             LDS planes (re and im apart, one pad word after every 32: a radix-8 pass stores at a stride of 8 words).
//             The planes are the wave's own, so a pass is ordered by wave_lds_point, not by a workgroup barrier; the one
//             barrier of the kernel stands between the 16 rows of magnitudes and the product.
//             The post-pass X[k] = (Z[k] + conj Z[H - k]) / 2 + exp(-2 pi i k / n_fft) (Z[k] - conj Z[H - k]) / (2 i),
//             k = 0 .. H, gives the H + 1 bins, whose magnitudes go to the row of the LDS tile.  Twiddles come from the
//             packed table, made in double and rounded once.
//   product   [16][H + 4] magnitudes times the packed basis on v_mfma_f32_16x16x4_f32 (ge2e_rows_dev.hpp has the operand
//             map): A[i = l15][k = q] from the LDS tile, B[k = q][j = l15] one coalesced 256-byte line per K-step from L2,
//             two accumulators (even and odd K-steps) added at the end.
//   epilogue  mode 0: the linear mel; mode 1: clip((20 log10(max(min_level, m)) - ref - min_db) / -min_db, 0, 1) of those
//             very bits.  Comparisons are written so that a NaN stays a NaN (numpy's maximum and clip).
// A frame with a NaN or Inf sample gets NaN magnitudes in every bin, so every element of its row is NaN whatever the basis
// holds.  Every sum has a fixed order and MFMA rows are independent: the bits of a row depend on its samples, its gain and
// the packed tables alone.  Rows of the last tile past total_frames transform zeros and are never stored.
#include "ge2e_melspec.hpp"

#include <math.h>
#include <stdio.h>

#include "ge2e_rows_dev.hpp"

namespace ge2e {

namespace {

__global__ __launch_bounds__(256) void melspec_pack_kernel(const float* __restrict__ window, const float* __restrict__ basis,
                                                            int n_fft, int n_mels, float* __restrict__ packed, size_t total) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const int K = n_fft / 2 + 1, S = mel_kpad(n_fft) / 4;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        float val;
        if (idx < (size_t)n_fft) {
            val = window[idx];
        } else if (idx < 3 * (size_t)n_fft) {
            const int t = (int)(idx - n_fft), k = t >> 1;
            double s, c;
            sincospi(-2.0 * (double)k / (double)n_fft, &s, &c);
            val = (float)((t & 1) ? s : c);
        } else {
            const size_t local = idx - 3 * (size_t)n_fft;
            const int lane = (int)(local & 63), rest = (int)(local >> 6), s = rest % S, ct = rest / S;
            const int k = 4 * s + (lane >> 4), col = 16 * ct + (lane & 15);
            val = (k < K && col < n_mels) ? basis[(size_t)k * n_mels + col] : 0.f;
        }
        packed[idx] = val;
    }
}

// The radix of pass `pass` over H complex points, and the number of passes.
__host__ __device__ constexpr int mel_radix(int H, int pass) {
    return pass == 0 ? 8 : pass == 1 ? (H == 128 ? 4 : 8) : pass == 2 ? (H == 512 ? 8 : 4) : 4;
}
__host__ __device__ constexpr int mel_passes(int H) { return H == 1024 ? 4 : 3; }
__host__ __device__ constexpr int mel_sub_length(int H, int pass) {   // Ns: the product of the radices before `pass`
    int ns = 1;
    for (int p = 0; p < pass; ++p) ns *= mel_radix(H, p);
    return ns;
}
__device__ __forceinline__ int mel_pad(int i) { return i + (i >> 5); }

__device__ __forceinline__ void dft4(float& r0, float& i0, float& r1, float& i1, float& r2, float& i2, float& r3, float& i3) {
    const float ar = r0 + r2, ai = i0 + i2, br = r0 - r2, bi = i0 - i2;
    const float cr = r1 + r3, ci = i1 + i3, dr = i1 - i3, di = r3 - r1;   // d = -i (v1 - v3)
    r0 = ar + cr; i0 = ai + ci;
    r1 = br + dr; i1 = bi + di;
    r2 = ar - cr; i2 = ai - ci;
    r3 = br - dr; i3 = bi - di;
}

template <int R>
__device__ __forceinline__ void dft(float (&vr)[R], float (&vi)[R]) {
    static_assert(R == 4 || R == 8, "radix 4 or 8");
    if constexpr (R == 4) {
        dft4(vr[0], vi[0], vr[1], vi[1], vr[2], vi[2], vr[3], vi[3]);
    } else {
        dft4(vr[0], vi[0], vr[2], vi[2], vr[4], vi[4], vr[6], vi[6]);   // the even points: E[k] in 0, 2, 4, 6
        dft4(vr[1], vi[1], vr[3], vi[3], vr[5], vi[5], vr[7], vi[7]);   // the odd ones: O[k] in 1, 3, 5, 7
        constexpr float h = 0.70710678118654752440f;
        // O[k] w^k, w = exp(-i pi / 4): 1, (1 - i) h, -i, (-1 - i) h
        const float o1r = (vr[3] + vi[3]) * h, o1i = (vi[3] - vr[3]) * h;
        const float o2r = vi[5], o2i = -vr[5];
        const float o3r = (vi[7] - vr[7]) * h, o3i = -(vr[7] + vi[7]) * h;
        const float er[4] = {vr[0], vr[2], vr[4], vr[6]}, ei[4] = {vi[0], vi[2], vi[4], vi[6]};
        const float orr[4] = {vr[1], o1r, o2r, o3r}, oi[4] = {vi[1], o1i, o2i, o3i};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            vr[k] = er[k] + orr[k];     vi[k] = ei[k] + oi[k];
            vr[k + 4] = er[k] - orr[k]; vi[k + 4] = ei[k] - oi[k];
        }
    }
}

template <int NFFT>
__global__ __launch_bounds__(kMelThreads) void melspec_kernel(ProblemMelspec p) {
    extern __shared__ __attribute__((aligned(16))) float mel_lds[];
    constexpr int H = NFFT / 2, NP = mel_passes(H), KP = H + 4, S = KP / 4;
    constexpr int TS = H + 34, PL = H + H / 32;     // mel_tile_stride, mel_plane_floats
    constexpr int MAXPTS = H / 64;                  // complex points a lane holds between two passes
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    float* tile = mel_lds;                                         // [16][TS]
    float* re = mel_lds + kMelTile * TS + wid * 2 * PL;            // the wave's planes
    float* im = re + PL;
    const float* window = p.packed;
    const float2* tw = reinterpret_cast<const float2*>(p.packed + NFFT);
    const float* basis = p.packed + 3 * NFFT;
    const float qnan = __int_as_float(0x7fc00000);

#pragma clang loop unroll(disable)
    for (int fr = 0; fr < kMelTile / kMelWaves; ++fr) {
        const int trow = wid + fr * kMelWaves;
        const long long row = (long long)blockIdx.x * kMelTile + trow;
        const bool valid = row < p.total_frames;
        long long pos0 = 0, len = 0, P = 1;
        const float* x = p.wav;
        float gain = 1.f;
        if (valid) {
            // the row's utterance: the last u with frame_start[u] <= row (the pointer by value: with p captured by
            // reference hipcc allocates and vectorises the transform of <256> and <512> differently;
            // profiles/audio_front_end_refactor_ab.txt, section 3)
            const int u = last_not_above(p.U, row, [fs = p.frame_start](int i) { return fs[i]; });
            len = p.utt_len[u];
            P = p.utt_padded_len ? p.utt_padded_len[u] : len;
            x = p.wav + p.utt_start[u];
            gain = p.gain ? p.gain[u] : 1.f;
            pos0 = (row - p.frame_start[u]) * (long long)p.hop - NFFT / 2;
        }
        bool bad = false;
        // sample n of the frame, times gain and window; never reads at or past utt_len (or before 0, whatever P is)
        auto sample = [&](int n) -> float {
            long long s = pos0 + n;
            if (s < 0) s = -s;
            if (s >= P) s = 2 * (P - 1) - s;
            float v = 0.f;
            if (valid && s >= 0 && s < len) v = x[s];
            bad = bad || !(fabsf(v) <= 3.402823466e+38f);
            return (v * gain) * window[n];
        };

        // every pass: the lane's points into registers, the butterflies, the outputs into the planes
        float vr[MAXPTS < 8 ? 8 : MAXPTS], vi[MAXPTS < 8 ? 8 : MAXPTS];
        static_for<0, NP>([&](auto pc) {
            constexpr int pass = decltype(pc)::value;
            constexpr int R = mel_radix(H, pass), NS = mel_sub_length(H, pass), NB = H / R, IT = (NB + 63) / 64;
            static_assert(IT * R <= (MAXPTS < 8 ? 8 : MAXPTS), "the lane's registers hold the pass");
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                const int j = lane + 64 * it;
                if (NB % 64 == 0 || j < NB) {
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const int e = j + r * NB;
                        if constexpr (pass == 0) {
                            vr[it * R + r] = sample(2 * e);
                            vi[it * R + r] = sample(2 * e + 1);
                        } else {
                            vr[it * R + r] = re[mel_pad(e)];
                            vi[it * R + r] = im[mel_pad(e)];
                        }
                    }
                }
            }
            wave_lds_point();   // the wave has read its planes (pass 0: in the previous row's post-pass)
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                const int j = lane + 64 * it;
                if (NB % 64 == 0 || j < NB) {
                    const int k = j & (NS - 1);
                    float ar[R], ai[R];
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        ar[r] = vr[it * R + r];
                        ai[r] = vi[it * R + r];
                        if (NS > 1 && r > 0) {
                            const float2 w = tw[2 * (r * k * (H / (NS * R)))];
                            const float tr = ar[r] * w.x - ai[r] * w.y, ti = ar[r] * w.y + ai[r] * w.x;
                            ar[r] = tr;
                            ai[r] = ti;
                        }
                    }
                    dft<R>(ar, ai);
                    const int base = (j - k) * R + k;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        re[mel_pad(base + r * NS)] = ar[r];
                        im[mel_pad(base + r * NS)] = ai[r];
                    }
                }
            }
            wave_lds_point();   // ... and written them
        });
        const bool poison = __builtin_amdgcn_ballot_w64(bad) != 0;

        // the real transform's bins from the complex one's, their magnitudes into the tile's row
        float* trw = tile + trow * TS;
#pragma unroll
        for (int it = 0; it < MAXPTS; ++it) {
            const int k = lane + 64 * it, kk = (H - k) & (H - 1);
            const float ar = re[mel_pad(k)], ai = im[mel_pad(k)], br = re[mel_pad(kk)], bi = im[mel_pad(kk)];
            const float er = 0.5f * (ar + br), ei = 0.5f * (ai - bi);
            const float orr = 0.5f * (ai + bi), oi = 0.5f * (br - ar);
            const float2 w = tw[k];
            const float xr = er + (w.x * orr - w.y * oi), xi = ei + (w.x * oi + w.y * orr);
            trw[k] = poison ? qnan : sqrtf(xr * xr + xi * xi);
            if (k == 0) trw[H] = poison ? qnan : fabsf(ar - ai);
        }
        if (lane >= 1 && lane <= 3) trw[H + lane] = 0.f;
    }
    __syncthreads();

    // the mel product: column tile `wid` of pad16(n_mels) / 16, all 16 rows
    const int CT = mel_pad16(p.n_mels) / 16;
    if (wid < CT) {   // (uniform over the wave)
        const int l15 = lane & 15, q = lane >> 4;
        const float* a = tile + l15 * TS + q;
        const float* b = basis + (size_t)wid * S * 64 + lane;
        v4f acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
        int s = 0;
#pragma unroll 4
        for (; s + 1 < S; s += 2) {
            acc0 = mfma_f32(a[4 * s], b[(size_t)s * 64], acc0);
            acc1 = mfma_f32(a[4 * s + 4], b[(size_t)(s + 1) * 64], acc1);
        }
        if (s < S) acc0 = mfma_f32(a[4 * s], b[(size_t)s * 64], acc0);
        const int col = 16 * wid + l15;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const long long row = (long long)blockIdx.x * kMelTile + 4 * q + v;
            float m = acc0[v] + acc1[v];
            if (p.mode) {
                const float c = m < p.min_level ? p.min_level : m;                       // NaN stays
                const float d = (20.f * log10f(c) - p.ref_level_db - p.min_level_db) / -p.min_level_db;
                m = d < 0.f ? 0.f : d > 1.f ? 1.f : d;
            }
            if (row < p.total_frames && col < p.n_mels) p.out[(size_t)row * p.n_mels + col] = m;
        }
    }
}

KernelLaunchState g_melspec_state[4];
}  // namespace

hipError_t launch_melspec_pack(const float* window, const float* basis, int n_fft, int n_mels, float* packed, hipStream_t stream) {
    return launch_per_element(melspec_pack_kernel, melspec_packed_floats(n_fft, n_mels), stream, window, basis, n_fft, n_mels,
                              packed);
}

template <int NFFT>
static hipError_t launch_melspec_n(const ProblemMelspec& p, KernelLaunchState& st, hipStream_t stream) {
    const unsigned lds = (unsigned)melspec_lds_bytes(NFFT);
    const unsigned tiles = (unsigned)((p.total_frames + kMelTile - 1) / kMelTile);
    const hipError_t err = prepare_kernel(st, (const void*)melspec_kernel<NFFT>, kMelThreads, lds, nullptr);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(melspec_kernel<NFFT>, dim3(tiles), dim3(kMelThreads), lds, stream, p);
    return hipGetLastError();
}

hipError_t launch_melspec(const ProblemMelspec& p, int n_fft, hipStream_t stream) {
    switch (n_fft) {
        case 256: return launch_melspec_n<256>(p, g_melspec_state[0], stream);
        case 512: return launch_melspec_n<512>(p, g_melspec_state[1], stream);
        case 1024: return launch_melspec_n<1024>(p, g_melspec_state[2], stream);
        default: return launch_melspec_n<2048>(p, g_melspec_state[3], stream);
    }
}

int plan_string_melspec(long long total_frames, int n_fft, char* buf, size_t cap) {
    return snprintf(buf, cap, "melspec<%d>/%lld", n_fft, (total_frames + kMelTile - 1) / kMelTile);
}

}  // namespace ge2e
