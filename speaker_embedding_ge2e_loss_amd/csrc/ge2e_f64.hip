// ge2e_loss_fwd_bwd_f64: the whole loss, forward + backward, in double precision.  Same semantics and the same phase
// structure as GE2E_IMPL_GENERIC (ge2e_generic.hip, oracle/ge2e_oracle.py:closed_form line by line) with every value,
// accumulator and transcendental in fp64: one 256-thread workgroup per (N,M,D) batch, grid-stride over B, intermediates
// in a per-workgroup slice of the caller's workspace, phases separated by __syncthreads().  Any shape (no alignment rule
// on D).  The three contractions run on v_mfma_f64_16x16x4_f64, one 16 x 16 output tile per wave at a time:
//   B1  X  [NM][N] = E . CH^T            (cosines before the row norm)      K = D
//   C1  GC [N][D]  = (A_off rne)^T . E   (dL/d c-hat)                       K = N M
//   D1  G  [NM][D] = A_off . CH          (centroid side of dL/d e-hat)      K = N
// Operand map of the instruction (lane l, l15 = l & 15, q = l >> 4): A[i = l15][k = q], B[k = q][j = l15];
// results C[i = q + 4 reg][j = l15], reg = 0..3 -- NOT the row map of the f32 / f16 forms.  Edge tiles are zero-filled by
// predicated loads; nothing is read or written past a row.  Norms, the leave-one-out column, the stabilised exp / log
// (shift by max(max_k S_k, log eps), as closed_form(stable=True)) and the row statistics stay on the fp64 VALU.
// Deterministic: no atomics, every sum in a fixed order that does not depend on the batch's position in the launch.
#include "ge2e_f64.hpp"

#include <math.h>

#include "ge2e_rows_dev.hpp"

namespace ge2e {

namespace {
constexpr int kMaxWaves = 16;
constexpr int kF64MaxGrid = 512;   // two workgroups per CU of a whole MI355X; bounds the workspace (one slice each)

typedef double v4d __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void unit_stats_d(double sq, double eps_cos, double& rn, double& kappa) {
    const double n = sqrt(sq);
    const double nc = fmax(n, eps_cos);
    rn = 1.0 / nc;
    kappa = n > 0.0 ? nc / n : 0.0;
}
__device__ __forceinline__ v4d mfma_f64(double a, double b, v4d c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}
}  // namespace

__global__ __launch_bounds__(256) void ge2e_f64_kernel(ProblemF64 p, size_t ws_stride) {
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    const int NW = blockDim.x >> 6;
    const int l15 = lane & 15, q = lane >> 4;
    const int N = p.N, M = p.M, D = p.D, NM = N * M;
    const F64Layout L = f64_layout(N, M, D);
    double* ws = p.ws + (size_t)blockIdx.x * ws_stride;
    double* CH = ws + L.ch;
    double* SS = ws + L.ss;
    double* GC = ws + L.gc;
    double* DUS = ws + L.dus;
    double* A = ws + L.a;
    double* RST = ws + L.rowstat;
    double* CST = ws + L.cstat;
    __shared__ double red[3][kMaxWaves];

    const double w = *p.w, bias = *p.b;
    const double eps = p.eps, eps_cos = p.eps_cos, log_eps = p.log_eps;
    const double fM = (double)M, fM1 = (double)(M - 1);
    const bool contrast = p.variant == 1;
    const int RT = (NM + 15) >> 4, KT = (N + 15) >> 4, DT = (D + 15) >> 4;   // 16-wide tiles over rows, centroids, D

    for (int bi = blockIdx.x; bi < p.B; bi += gridDim.x) {
        const double* E = p.E + (size_t)bi * NM * D;

        // ---- phase A: speaker sums and unit centroids --------------------------------
        for (int j = wid; j < N; j += NW) {
            double sq = 0.0;
            for (int d = lane; d < D; d += kWave) {
                double s = 0.0;
                for (int i = 0; i < M; ++i) s += E[(size_t)(j * M + i) * D + d];
                SS[(size_t)j * D + d] = s;
                const double c = s / fM;
                sq += c * c;
            }
            sq = wave_sum(sq);
            double rn, kap;
            unit_stats_d(sq, eps_cos, rn, kap);
            for (int d = lane; d < D; d += kWave) CH[(size_t)j * D + d] = SS[(size_t)j * D + d] / fM * rn;
            if (lane == 0) { CST[j * 2 + CS_RN] = rn; CST[j * 2 + CS_KAP] = kap; }
        }
        __syncthreads();

        // ---- phase B0: row norms and the leave-one-out (own-speaker) cosine ------------
        for (int r = wid; r < NM; r += NW) {
            const int j = r / M;
            const double* er = E + (size_t)r * D;
            double ee = 0.0, uu = 0.0, eu = 0.0;
            for (int d = lane; d < D; d += kWave) {
                const double e = er[d];
                const double u = (SS[(size_t)j * D + d] - e) / fM1;
                ee += e * e; uu += u * u; eu += e * u;
            }
            ee = wave_sum(ee); uu = wave_sum(uu); eu = wave_sum(eu);
            double rne, ke, rnu, ku;
            unit_stats_d(ee, eps_cos, rne, ke);
            unit_stats_d(uu, eps_cos, rnu, ku);
            if (lane == 0) {
                double* rs = RST + (size_t)r * 8;
                rs[RS_RNE] = rne; rs[RS_KE] = ke; rs[RS_RNU] = rnu; rs[RS_KU] = ku;
                rs[RS_COSD] = eu * rne * rnu;
            }
        }
        __syncthreads();

        // ---- phase B1: cos tiles on the matrix core: rows x unit centroids, K = D --------
        // (the k index of the contraction is a free permutation as long as both operands use the same one: lane group q
        //  takes d0 + 4 q + s in step s, so a lane walks 4 consecutive elements of its row)
        for (int t = wid; t < RT * KT; t += NW) {
            const int rt = t / KT, kt = t - rt * KT;
            const int ra = rt * 16 + l15, kb = kt * 16 + l15;
            const bool ra_ok = ra < NM, kb_ok = kb < N;
            const double* pa = E + (size_t)(ra_ok ? ra : 0) * D;
            const double* pb = CH + (size_t)(kb_ok ? kb : 0) * D;
            v4d acc = {0.0, 0.0, 0.0, 0.0};
            for (int d0 = 0; d0 < D; d0 += 16) {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int d = d0 + 4 * q + s;
                    const double a = (ra_ok && d < D) ? pa[d] : 0.0;
                    const double b = (kb_ok && d < D) ? pb[d] : 0.0;
                    acc = mfma_f64(a, b, acc);
                }
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int r = rt * 16 + q + 4 * g;
                if (r < NM && kb_ok) {
                    const double* rs = RST + (size_t)r * 8;
                    A[(size_t)r * N + kb] = (kb == r / M) ? rs[RS_COSD] : acc[g] * rs[RS_RNE];
                }
            }
        }
        __syncthreads();

        // ---- phase B2: per row: loss, dL/dcos (one wave per row, lane <-> centroid) -----
        double loss_acc = 0.0, dw_acc = 0.0, db_acc = 0.0;
        for (int r = wid; r < NM; r += NW) {
            const int j = r / M;
            double* Arow = A + (size_t)r * N;
            const double cosd = RST[(size_t)r * 8 + RS_COSD];
            const double sjj = w * (cosd + eps) + bias;
            double mx, best;
            int besti;
            row_scan<kWave>(Arow, lane, N, j, w, bias, eps, mx, best, besti);
            const RowLoss<double> rl = row_loss<kWave>(Arow, lane, N, j, sjj, w, bias, eps, log_eps, contrast, mx, best, besti,
                                                       true, dw_acc, db_acc);
            const double per = rl.per, coef = rl.coef, ad = rl.ad;
            loss_acc += per;
            if (lane == 0) {
                if (p.per) p.per[(size_t)bi * NM + r] = per;
                double* rs = RST + (size_t)r * 8;
                rs[RS_AD] = ad; rs[RS_COEF] = coef;
            }
        }
        dw_acc = wave_sum(dw_acc);
        db_acc = wave_sum(db_acc);
        if (lane == 0) { red[0][wid] = loss_acc; red[1][wid] = dw_acc; red[2][wid] = db_acc; }
        __syncthreads();
        if (threadIdx.x == 0) {
            double l = 0.0, a = 0.0, c = 0.0;
            for (int i = 0; i < NW; ++i) { l += red[0][i]; a += red[1][i]; c += red[2][i]; }
            p.loss[bi] = l;
            if (p.dw) p.dw[bi] = a;
            if (p.db) p.db[bi] = c;
        }

        if (p.dE) {
            double* dE = p.dE + (size_t)bi * NM * D;
            // ---- phase C1: dL/d c-hat = (A_off rne)^T . E on the matrix core, K = N M ------
            for (int t = wid; t < KT * DT; t += NW) {
                const int kt = t / DT, dt = t - kt * DT;
                const int ka = kt * 16 + l15, dcol = dt * 16 + l15;
                const bool ka_ok = ka < N, d_ok = dcol < D;
                v4d acc = {0.0, 0.0, 0.0, 0.0};
                for (int r0 = 0; r0 < NM; r0 += 16) {
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const int r = r0 + 4 * q + s;
                        const bool r_ok = r < NM;
                        const double a = (ka_ok && r_ok) ? A[(size_t)r * N + ka] * RST[(size_t)r * 8 + RS_RNE] : 0.0;
                        const double b = (d_ok && r_ok) ? E[(size_t)r * D + dcol] : 0.0;
                        acc = mfma_f64(a, b, acc);
                    }
                }
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int k = kt * 16 + q + 4 * g;
                    if (k < N && d_ok) GC[(size_t)k * D + dcol] = acc[g];
                }
            }
            __syncthreads();
            // ---- phase C2: through the centroid norm; D0: per-speaker sum of dL/du ------------
            for (int j = wid; j < N; j += NW) {
                double coef = 0.0;
                for (int d = lane; d < D; d += kWave) coef += GC[(size_t)j * D + d] * CH[(size_t)j * D + d];
                coef = wave_sum(coef);
                const double rn = CST[j * 2 + CS_RN], kap = CST[j * 2 + CS_KAP];
                for (int d = lane; d < D; d += kWave) {
                    GC[(size_t)j * D + d] = (GC[(size_t)j * D + d] - kap * coef * CH[(size_t)j * D + d]) * rn;
                    const double s = SS[(size_t)j * D + d];
                    double dusum = 0.0;
                    for (int i = 0; i < M; ++i) {
                        const int r = j * M + i;
                        const double* rs = RST + (size_t)r * 8;
                        dusum += loo_term(E[(size_t)r * D + d], s, fM1, rs[RS_RNE], rs[RS_RNU], rs[RS_KU], rs[RS_COSD],
                                          rs[RS_AD]).du;
                    }
                    DUS[(size_t)j * D + d] = dusum;
                }
            }
            __syncthreads();
            // ---- phase D1: dE tiles: A_off . CH on the matrix core (K = N), then the row epilogue ----
            for (int t = wid; t < RT * DT; t += NW) {
                const int rt = t / DT, dt = t - rt * DT;
                const int ra = rt * 16 + l15, d = dt * 16 + l15;
                const bool ra_ok = ra < NM, d_ok = d < D;
                const double* pa = A + (size_t)(ra_ok ? ra : 0) * N;
                v4d acc = {0.0, 0.0, 0.0, 0.0};
                for (int k0 = 0; k0 < N; k0 += 16) {
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const int k = k0 + 4 * q + s;
                        const bool k_ok = k < N;
                        const double a = (ra_ok && k_ok) ? pa[k] : 0.0;
                        const double b = (d_ok && k_ok) ? CH[(size_t)k * D + d] : 0.0;
                        acc = mfma_f64(a, b, acc);
                    }
                }
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int r = rt * 16 + q + 4 * g;
                    if (r < NM && d_ok) {
                        const int j = r / M;
                        const double* rs = RST + (size_t)r * 8;
                        const LooTerm<double> lo = loo_term(E[(size_t)r * D + d], SS[(size_t)j * D + d], fM1, rs[RS_RNE],
                                                            rs[RS_RNU], rs[RS_KU], rs[RS_COSD], rs[RS_AD]);
                        const double ge = acc[g] + rs[RS_AD] * lo.uh;
                        dE[(size_t)r * D + d] = (ge - rs[RS_KE] * rs[RS_COEF] * lo.eh) * rs[RS_RNE] + GC[(size_t)j * D + d] / fM +
                                                (DUS[(size_t)j * D + d] - lo.du) / fM1;
                    }
                }
            }
        }
        __syncthreads();  // workspace slice is reused by the next batch of this workgroup
    }
}

int f64_grid(int B) { return B < kF64MaxGrid ? B : kF64MaxGrid; }

size_t f64_workspace_bytes(int B, int N, int M, int D) {
    return align_up((size_t)f64_grid(B) * f64_layout(N, M, D).total * sizeof(double), 256);
}

hipError_t launch_f64(const ProblemF64& p, hipStream_t stream) {
    const int grid = f64_grid(p.B);
    const size_t stride = f64_layout(p.N, p.M, p.D).total;
    hipLaunchKernelGGL(ge2e_f64_kernel, dim3(grid), dim3(256), 0, stream, p, stride);
    return hipGetLastError();
}

}  // namespace ge2e
