// ge2e_loss_fwd_bwd_ragged: the whole loss, forward + backward, for a batch whose speakers have DIFFERENT utterance
// counts.  E [R][D] holds the rows of speaker j at off[j] .. off[j+1]-1 (m_j = off[j+1] - off[j] >= 2); the semantics are
// the dense loss's (ge2e_generic.hip, oracle/ge2e_oracle.py:closed_form) with M replaced by m_j wherever it appears:
// c_k = mean of speaker k's rows, u_r = (sum_j - e_r) / (m_j - 1), dL/dc_j spread as / m_j, dL/du as / (m_j - 1).
// The plan is ge2e_f64.hip's, in fp32: one 256-thread workgroup per batch, grid-stride over B, intermediates in a
// per-workgroup slice of the caller's workspace, phases separated by __syncthreads().  Any N >= 1, D >= 1, R >= 2 N.
//   0   spk[r] = speaker of row r (binary search in the offsets); per-speaker sums, m_j and unit centroids
//   B0  row norms and the leave-one-out (own-speaker) cosine
//   B1  X  [R][N] = E . CH^T            (cosines before the row norm)      K = D      matrix core
//   B2  per row: loss, dL/dcos (one wave per row, lane <-> centroid)
//   C1  GC [N][D] = (A_off rne)^T . E   (dL/d c-hat)                       K = R      matrix core
//   C2  through the centroid norm; per-speaker sum of dL/du over off[j] .. off[j+1]
//   D1  G  [R][D] = A_off . CH          (centroid side of dL/d e-hat)      K = N      matrix core, then the row epilogue
// The contractions run on v_mfma_f32_16x16x4_f32 (exact fp32: an fmaf chain), one 16 x 16 output tile per wave at a
// time.  Operand map (lane l, l15 = l & 15, q = l >> 4): A[i = l15][k = q], B[k = q][j = l15]; results
// C[i = 4 q + reg][j = l15], reg = 0..3 (the f64 form's rows are q + 4 reg).  The k index is permuted the same way in
// both operands (lane group q takes k0 + 4 q + s in step s), so a lane walks 4 consecutive floats of its row in B1 / D1:
// one 16-byte load where the row length is a multiple of 4.  Edge tiles are zero-filled by predicated loads; nothing is
// read or written past a row.  A speaker may be longer than any tile and many speakers may share one: everything after
// phase 0 uses spk[r] and off[j] where the dense kernels use r / M and j M.
// Every offset is clamped into [0, R] where it is read and spk[r] is in [0, N) whatever the offsets hold: offsets that
// break the contract give wrong or non-finite numbers, never an access outside the buffers.
// Deterministic: no atomics, every sum in a fixed order that does not depend on the batch's position in the launch.
// ge2e_loss_fwd_bwd_labeled runs the kGather instantiation: the rows arrive in any order and order[r] (ge2e_labels.hip)
// names the row of E that stands at sorted position r.  Every read of E, and the stores to dE and per, go through it; all
// intermediates (spk, rowstat, A) stay in sorted order, so the arithmetic and its order are those of the plain form on
// gathered rows.  A row still starts at a multiple of D floats: the 16-byte loads hold as before.
// ge2e_loss_fwd_bwd_labeled_masked runs the kMasked instantiation, which gathers and takes the batch's EXTENTS from the
// device: active[bi] = {n_act, r_act} (ge2e_label_index_masked) stand wherever N and R are loop bounds, tile counts or the
// row length of A, so the arithmetic and its order are the plain form's on the n_act speakers and the r_act rows
// order[0 .. r_act): the same bits.  p.N is only the stride of the offset table, p.R that of E, dE, per and order, and the
// slice is laid out for p.NA speakers and p.R rows.  Every thread of the workgroup reads the same two words, so every
// barrier stays uniform; both are clamped where they are read, to [0, NA] and [0, R]: whatever the memory holds, nothing
// is accessed outside the buffers and no loop is unbounded.  The rows order[r_act .. R) of dE and per are written as 0
// after the last phase; a batch without active speakers writes zeros and takes no phase.
#include "ge2e_ragged.hpp"

#include <math.h>

#include "ge2e_rows_dev.hpp"

namespace ge2e {

namespace {
constexpr int kMaxWaves = 16;
constexpr int kRaggedMaxGrid = 512;   // two workgroups per CU of a whole MI355X; bounds the workspace (one slice each)
}  // namespace

// kGather: row r of the sorted layout is row order[r] of E, dE and per (ge2e_loss_fwd_bwd_labeled); otherwise it is row r.
// kMasked (with kGather): the batch's speaker and row counts are active[bi] (ge2e_loss_fwd_bwd_labeled_masked).
template <bool kGather, bool kMasked>
__global__ __launch_bounds__(256) void ge2e_ragged_kernel(ProblemRagged p, size_t ws_stride) {
    static_assert(kGather || !kMasked, "the masked form gathers");
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    const int NW = blockDim.x >> 6;
    const int l15 = lane & 15, q = lane >> 4;
    const int D = p.D;
    const int RC = p.R;   // rows per batch of E, dE, per and order
    const RaggedLayout L = ragged_layout(kMasked ? p.NA : p.N, RC, D);
    float* ws = p.ws + (size_t)blockIdx.x * ws_stride;
    float* CH = ws + L.ch;
    float* SS = ws + L.ss;
    float* GC = ws + L.gc;
    float* DUS = ws + L.dus;
    float* A = ws + L.a;
    float* RST = ws + L.rowstat;
    float* CST = ws + L.cstat;
    int* SPK = reinterpret_cast<int*>(ws + L.spk);
    __shared__ float red[3][kMaxWaves];

    const float w = *p.w, bias = *p.b;
    const float eps = p.eps, eps_cos = p.eps_cos, log_eps = p.log_eps;
    const bool contrast = p.variant == 1;
    const bool vecD = (D & 3) == 0;
    const int DT = (D + 15) >> 4;

    for (int bi = blockIdx.x; bi < p.B; bi += gridDim.x) {
        int N = p.N, R = RC;
        if constexpr (kMasked) {   // the same two words for every thread of the workgroup
            N = min(max(p.active[(size_t)bi * 2], 0), p.NA);
            R = min(max(p.active[(size_t)bi * 2 + 1], 0), RC);
        }
        const bool vecN = (N & 3) == 0;
        const int RT = (R + 15) >> 4, KT = (N + 15) >> 4;   // 16-wide tiles over rows, centroids (DT: over D)
        const float* E = p.E + (size_t)bi * RC * D;
        const int* offs = p.off + (size_t)bi * ((size_t)p.N + 1);
        auto off_at = [&](int j) { return min(max(offs[j], 0), R); };   // j in [0, N]
        [[maybe_unused]] const int* ord = kGather ? p.order + (size_t)bi * RC : nullptr;
        auto row = [&](int r) -> int {   // where sorted row r lives in E, dE and per
            if constexpr (kGather) return ord[r];
            else return r;
        };
        // (kMasked) the rows that do not count: order[R .. RC) of dE and per are 0, one wave per row
        [[maybe_unused]] auto zero_tail = [&]() {
            for (int r = R + wid; r < RC; r += NW) {
                const size_t at = (size_t)bi * RC + row(r);
                if (p.per && lane == 0) p.per[at] = 0.f;
                if (p.dE) {
                    float* g = p.dE + at * D;
                    if (vecD) {
                        const v4f z = {0.f, 0.f, 0.f, 0.f};
                        for (int d = 4 * lane; d < D; d += 4 * kWave) *reinterpret_cast<v4f*>(g + d) = z;
                    } else {
                        for (int d = lane; d < D; d += kWave) g[d] = 0.f;
                    }
                }
            }
        };
        if constexpr (kMasked) {
            if (N == 0) {   // no active speaker: zeros and no phase (uniform: every thread read the same N)
                R = 0;      // every row of the batch is written
                zero_tail();
                if (threadIdx.x == 0) {
                    p.loss[bi] = 0.f;
                    if (p.dw) p.dw[bi] = 0.f;
                    if (p.db) p.db[bi] = 0.f;
                }
                continue;
            }
        }

        // ---- phase 0: row -> speaker; speaker sums, counts and unit centroids ------------
        // the largest j in [0, N) with off[j] <= r: the speaker of row r under the contract, some speaker without it
        for (int r = threadIdx.x; r < R; r += blockDim.x) SPK[r] = last_not_above(N, r, off_at);
        for (int j = wid; j < N; j += NW) {
            const int r0 = off_at(j), r1 = off_at(j + 1);
            const float fm = (float)(r1 - r0);
            float sq = 0.f;
            for (int d = lane; d < D; d += kWave) {
                float s = 0.f;
                for (int r = r0; r < r1; ++r) s += E[(size_t)row(r) * D + d];
                SS[(size_t)j * D + d] = s;
                const float c = s / fm;
                sq += c * c;
            }
            sq = wave_sum(sq);
            float rn, kap;
            unit_stats(sq, eps_cos, rn, kap);
            for (int d = lane; d < D; d += kWave) CH[(size_t)j * D + d] = SS[(size_t)j * D + d] / fm * rn;
            if (lane == 0) {
                float* cs = CST + (size_t)j * 4;
                cs[CS_RN] = rn; cs[CS_KAP] = kap; cs[CS_M] = fm; cs[CS_M1] = fm - 1.f;
            }
        }
        __syncthreads();

        // ---- phase B0: row norms and the leave-one-out (own-speaker) cosine ------------
        for (int r = wid; r < R; r += NW) {
            const int j = SPK[r];
            const float fm1 = CST[(size_t)j * 4 + CS_M1];
            const float* er = E + (size_t)row(r) * D;
            float ee = 0.f, uu = 0.f, eu = 0.f;
            for (int d = lane; d < D; d += kWave) {
                const float e = er[d];
                const float u = (SS[(size_t)j * D + d] - e) / fm1;
                ee += e * e; uu += u * u; eu += e * u;
            }
            ee = wave_sum(ee); uu = wave_sum(uu); eu = wave_sum(eu);
            float rne, ke, rnu, ku;
            unit_stats(ee, eps_cos, rne, ke);
            unit_stats(uu, eps_cos, rnu, ku);
            if (lane == 0) {
                float* rs = RST + (size_t)r * 8;
                rs[RS_RNE] = rne; rs[RS_KE] = ke; rs[RS_RNU] = rnu; rs[RS_KU] = ku;
                rs[RS_COSD] = eu * rne * rnu;
            }
        }
        __syncthreads();

        // ---- phase B1: cos tiles on the matrix core: rows x unit centroids, K = D --------
        for (int t = wid; t < RT * KT; t += NW) {
            const int rt = t / KT, kt = t - rt * KT;
            const int ra = rt * 16 + l15, kb = kt * 16 + l15;
            const bool ra_ok = ra < R, kb_ok = kb < N;
            const float* pa = E + (size_t)(ra_ok ? row(ra) : 0) * D;
            const float* pb = CH + (size_t)(kb_ok ? kb : 0) * D;
            v4f acc = {0.f, 0.f, 0.f, 0.f};
            for (int d0 = 0; d0 < D; d0 += 16) {
                const v4f a = load4(pa, d0 + 4 * q, D, ra_ok, vecD);
                const v4f b = load4(pb, d0 + 4 * q, D, kb_ok, vecD);
#pragma unroll
                for (int s = 0; s < 4; ++s) acc = mfma_f32(a[s], b[s], acc);
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int r = rt * 16 + 4 * q + g;
                if (r < R && kb_ok) {
                    const float* rs = RST + (size_t)r * 8;
                    A[(size_t)r * N + kb] = (kb == SPK[r]) ? rs[RS_COSD] : acc[g] * rs[RS_RNE];
                }
            }
        }
        __syncthreads();

        // ---- phase B2: per row: loss, dL/dcos (one wave per row, lane <-> centroid) -----
        float loss_acc = 0.f, dw_acc = 0.f, db_acc = 0.f;
        for (int r = wid; r < R; r += NW) {
            const int j = SPK[r];
            float* Arow = A + (size_t)r * N;
            const float cosd = RST[(size_t)r * 8 + RS_COSD];
            const float sjj = w * (cosd + eps) + bias;
            float mx, best;
            int besti;
            row_scan<kWave>(Arow, lane, N, j, w, bias, eps, mx, best, besti);
            const RowLoss<float> rl = row_loss<kWave>(Arow, lane, N, j, sjj, w, bias, eps, log_eps, contrast, mx, best, besti,
                                                      true, dw_acc, db_acc);
            const float per = rl.per, coef = rl.coef, ad = rl.ad;
            loss_acc += per;
            if (lane == 0) {
                if (p.per) p.per[(size_t)bi * RC + row(r)] = per;
                float* rs = RST + (size_t)r * 8;
                rs[RS_AD] = ad; rs[RS_COEF] = coef;
            }
        }
        dw_acc = wave_sum(dw_acc);
        db_acc = wave_sum(db_acc);
        if (lane == 0) { red[0][wid] = loss_acc; red[1][wid] = dw_acc; red[2][wid] = db_acc; }
        __syncthreads();
        if (threadIdx.x == 0) {
            float l = 0.f, a = 0.f, c = 0.f;
            for (int i = 0; i < NW; ++i) { l += red[0][i]; a += red[1][i]; c += red[2][i]; }
            p.loss[bi] = l;
            if (p.dw) p.dw[bi] = a;
            if (p.db) p.db[bi] = c;
        }

        if (p.dE) {
            float* dE = p.dE + (size_t)bi * RC * D;
            // ---- phase C1: dL/d c-hat = (A_off rne)^T . E on the matrix core, K = R ------
            for (int t = wid; t < KT * DT; t += NW) {
                const int kt = t / DT, dt = t - kt * DT;
                const int ka = kt * 16 + l15, dcol = dt * 16 + l15;
                const bool ka_ok = ka < N, d_ok = dcol < D;
                v4f acc = {0.f, 0.f, 0.f, 0.f};
                for (int r0 = 0; r0 < R; r0 += 16) {
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const int r = r0 + 4 * q + s;
                        const bool r_ok = r < R;
                        const float a = (ka_ok && r_ok) ? A[(size_t)r * N + ka] * RST[(size_t)r * 8 + RS_RNE] : 0.f;
                        const float b = (d_ok && r_ok) ? E[(size_t)row(r) * D + dcol] : 0.f;
                        acc = mfma_f32(a, b, acc);
                    }
                }
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int k = kt * 16 + 4 * q + g;
                    if (k < N && d_ok) GC[(size_t)k * D + dcol] = acc[g];
                }
            }
            __syncthreads();
            // ---- phase C2: through the centroid norm; D0: per-speaker sum of dL/du ------------
            for (int j = wid; j < N; j += NW) {
                const int r0 = off_at(j), r1 = off_at(j + 1);
                const float* cs = CST + (size_t)j * 4;
                const float rn = cs[CS_RN], kap = cs[CS_KAP], fm1 = cs[CS_M1];
                float coef = 0.f;
                for (int d = lane; d < D; d += kWave) coef += GC[(size_t)j * D + d] * CH[(size_t)j * D + d];
                coef = wave_sum(coef);
                for (int d = lane; d < D; d += kWave) {
                    GC[(size_t)j * D + d] = (GC[(size_t)j * D + d] - kap * coef * CH[(size_t)j * D + d]) * rn;
                    const float s = SS[(size_t)j * D + d];
                    float dusum = 0.f;
                    for (int r = r0; r < r1; ++r) {
                        const float* rs = RST + (size_t)r * 8;
                        dusum += loo_term(E[(size_t)row(r) * D + d], s, fm1, rs[RS_RNE], rs[RS_RNU], rs[RS_KU], rs[RS_COSD],
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
                const bool ra_ok = ra < R, d_ok = d < D;
                const float* pa = A + (size_t)(ra_ok ? ra : 0) * N;
                v4f acc = {0.f, 0.f, 0.f, 0.f};
                for (int k0 = 0; k0 < N; k0 += 16) {
                    const v4f a = load4(pa, k0 + 4 * q, N, ra_ok, vecN);
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const int k = k0 + 4 * q + s;
                        const float b = (d_ok && k < N) ? CH[(size_t)k * D + d] : 0.f;
                        acc = mfma_f32(a[s], b, acc);
                    }
                }
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int r = rt * 16 + 4 * q + g;
                    if (r < R && d_ok) {
                        const int j = SPK[r];
                        const float* rs = RST + (size_t)r * 8;
                        const float* cs = CST + (size_t)j * 4;
                        const size_t at = (size_t)row(r) * D + d;
                        // (loo_term's expressions, written out: through the helper the masked instantiation comes out with
                        //  another register allocation and its forward call measured slower,
                        //  profiles/exact_kernels_shared_steps.txt)
                        const float e = E[at];
                        const float s = SS[(size_t)j * D + d];
                        const float eh = e * rs[RS_RNE];
                        const float uh = (s - e) / cs[CS_M1] * rs[RS_RNU];
                        const float du = rs[RS_AD] * (eh - rs[RS_KU] * rs[RS_COSD] * uh) * rs[RS_RNU];
                        const float ge = acc[g] + rs[RS_AD] * uh;
                        dE[at] = (ge - rs[RS_KE] * rs[RS_COEF] * eh) * rs[RS_RNE] +
                                                GC[(size_t)j * D + d] / cs[CS_M] + (DUS[(size_t)j * D + d] - du) / cs[CS_M1];
                    }
                }
            }
        }
        if constexpr (kMasked) zero_tail();
        __syncthreads();  // workspace slice is reused by the next batch of this workgroup
    }
}

int ragged_grid(int B) { return B < kRaggedMaxGrid ? B : kRaggedMaxGrid; }

size_t ragged_workspace_bytes(int B, int N, int R, int D) {
    return align_up((size_t)ragged_grid(B) * ragged_layout(N, R, D).total * sizeof(float), 256);
}

hipError_t launch_ragged(const ProblemRagged& p, hipStream_t stream) {
    const int grid = ragged_grid(p.B);
    const size_t stride = ragged_layout(p.active ? p.NA : p.N, p.R, p.D).total;
    if (p.active) hipLaunchKernelGGL((ge2e_ragged_kernel<true, true>), dim3(grid), dim3(256), 0, stream, p, stride);
    else if (p.order) hipLaunchKernelGGL((ge2e_ragged_kernel<true, false>), dim3(grid), dim3(256), 0, stream, p, stride);
    else hipLaunchKernelGGL((ge2e_ragged_kernel<false, false>), dim3(grid), dim3(256), 0, stream, p, stride);
    return hipGetLastError();
}

}  // namespace ge2e
