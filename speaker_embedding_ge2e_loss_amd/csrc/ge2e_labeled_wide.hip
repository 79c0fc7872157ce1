// ge2e_loss_fwd_bwd_labeled_wide: the masked labelled loss, forward + backward, spread over the chip.  The semantics are
// ge2e_loss_fwd_bwd_labeled_masked's and the arithmetic is ge2e_ragged_kernel's phases 0 .. D1 (ge2e_ragged.hip: the
// specification of every formula); what differs is the work decomposition, and with it the low bits.  The masked index
// kernel (ge2e_labels.hip) has left offsets, order and active = {n_act, r_act} on the device; behind it, on the stream:
//   centroids  labeled_eval_centroids_kernel<true> (ge2e_labeled_eval.hip): one wave per (batch, speaker); SS, CH,
//              CST = {1 / |c|, kappa, m, m - 1}, spk.                                                       phase 0
//   rows       one 256-thread workgroup per (batch, tile of 64 sorted positions), 16 positions per wave.  Row norms and the
//              leave-one-out cosine from SS[j] - e_r; the cosines CH . E^T over K = D on v_mfma_f32_16x16x4_f32, the
//              wave's rows held in registers (D <= 256, D % 4 == 0) and the centroid fragments in a ring of loads, as in
//              labeled_eval_rows_kernel; the cosines go to A [R][NAp], a barrier, then the row pass over the wave's own 16
//              rows, 16 lanes per row and four rows at a time: loss, dL/dcos back into A with the own column zeroed, RS_AD
//              and RS_COEF, per through order.  One {loss, dw, db} partial per tile, the waves' sums added in wave order.
//                                                                                                         phases B0 - B2
//   sums       one wave per batch: the partials of the tiles below r_act, lane l taking tiles l, l + 64, ..., then the
//              wave's fixed-order sum; loss, dw, db.  n_act = 0: three zeros.
//   gc         one wave per (batch, piece of K, 32 speakers, 64 columns): GC = (A rne)^T . E over the piece's rows, eight
//              accumulators.  The row indices of 64 positions come with one coalesced load and are handed out with
//              v_readlane (four per MFMA step, one per lane group).  K = r_act is cut into wide_split(R) pieces of whole
//              64-row blocks -- a number fixed by the shape -- each with a plane of its own.                     phase C1
//   speakers   one wave per (batch, speaker): the pieces added in ascending order, the centroid-norm backward into GC,
//              and DUS, the speaker's sum of dL/du over its rows (indices by v_readlane again).                 phase C2
//   de         one workgroup per (batch, tile of 64 positions, slab of 64 columns): CH^T . A^T over K = n_act, so that a
//              lane ends with four consecutive columns of one row; D1's row epilogue; 16-byte stores through order where
//              D % 4 == 0.  Positions r_act .. R-1 are written as 0.                                              phase D1
// ge2e_cos_sim_labeled_bwd (launch_labeled_cos_grad) is the same chain with another rows kernel and without sums: centroids,
// labeled_cos_grad_rows_kernel -- B0 and B1 as above, then the caller's dL/dcos where the loss's stood: A, RS_AD, RS_COEF --
// and gc, speakers, de as they are (launch_labeled_wide_backward: one copy for both entries).
// No floating-point atomics, no integer ones either; every sum has a fixed order that depends on the shapes and on the
// batch's own labels only, never on the batch's place in the stack or on which workgroup took the work.  Grids are sized
// from R and NA = speaker_capacity(N, R); n_act and r_act are read on the device, and every table through a batch's
// IndexView (ge2e_rows_dev.hpp has the contract), here with r_act = 0 where n_act = 0: nothing counts without a speaker.
// Rows that do not count are never read.  Every barrier is reached by the whole workgroup (the conditions are uniform).
#include "ge2e_labeled_wide.hpp"

#include <math.h>

#include <algorithm>

#include "ge2e_labeled_eval.hpp"
#include "ge2e_rows_dev.hpp"

namespace ge2e {

namespace {
constexpr int kThreads = 256, kWaves = kThreads / kWave;
constexpr int kTile = kWideTile, kWaveRows = kTile / kWaves;   // sorted positions per workgroup / per wave
constexpr int kAcc = 4;                                        // 16-wide tiles (accumulators) in flight per wave
constexpr int kSlab = 16 * kAcc;                               // columns of D per wave of gc and per workgroup of de
constexpr int kGcTiles = 2;                                    // 16-speaker tiles per wave of gc
constexpr int kGcAhead = 8;                                    // steps of gc whose loads are in flight together
constexpr int kDeAhead = 2;                                    // steps of de whose loads are in flight together
constexpr int kMaxBlocks = 1 << 20;
static_assert(kWaveRows == 16, "a wave's rows are one MFMA tile");

// What a lane of the speakers kernel owns at column d: four elements where D % 4 == 0, one (then three zeros) otherwise.
__device__ __forceinline__ v4f load_own(const float* row, int d, bool vec) {
    v4f v = {0.f, 0.f, 0.f, 0.f};
    if (vec) v = *reinterpret_cast<const v4f*>(row + d);
    else v[0] = row[d];
    return v;
}
__device__ __forceinline__ void store_own(float* row, int d, const v4f& v, bool vec) {
    if (vec) *reinterpret_cast<v4f*>(row + d) = v;
    else row[d] = v[0];
}

constexpr bool kRowsNeedSpeaker = true;   // every batch's IndexView here: nothing counts without a speaker

// The batch's planes as the two rows kernels read and write them.
struct RowPlanes {
    const float *E, *CH, *SS, *CST;
    float *A, *RST;
};
__device__ __forceinline__ RowPlanes row_planes(const ProblemLabeledWide& p, int bi, int NAp) {
    const size_t b = (size_t)bi, R = (size_t)p.R, NA = (size_t)p.NA, D = (size_t)p.D;
    return {p.E + b * R * D, p.CH + b * NA * D, p.SS + b * NA * D, p.CST + b * NA * 4, p.A + b * R * NAp, p.RST + b * R * 8};
}

// ---- rows: phases B0, B1, B2 ---------------------------------------------------------------------------------------------
// kSteps > 0: D is a multiple of 4 and at most 16 kSteps; the wave's E fragments stay in registers over all column tiles
// and every loop over k is unrolled and free of branches (tile_cosines has the reasons).  kSteps == 0: any D, a plain loop
// over k.
template <int kSteps>
__global__ __launch_bounds__(kThreads) void wide_rows_kernel(ProblemLabeledWide p, int tiles) {
    __shared__ float red[3][kWaves];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int l15 = lane & 15, q = lane >> 4;
    const int D = p.D, R = p.R, NA = p.NA;
    const int NAp = (NA + 3) & ~3;
    const float eps = p.eps, eps_cos = p.eps_cos, log_eps = p.log_eps;
    const float w = *p.w, bias = *p.b;
    const bool contrast = p.variant == 1;

    const long long items = (long long)p.B * tiles;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int bi = (int)(item / tiles), tile = (int)(item - (long long)bi * tiles);
        const IndexView ix = index_view(p, bi, kRowsNeedSpeaker);
        const int n_act = ix.n_act, r_act = ix.r_act;
        const RowPlanes b = row_planes(p, bi, NAp);
        const int p0 = tile * kTile + wid * kWaveRows;

        // the positions that do not count: per = 0
        if (p.per && lane < kWaveRows) {
            const int pp = p0 + lane;
            if (pp < R && pp >= r_act) p.per[(size_t)bi * R + ix.row_at(pp)] = 0.f;
        }
        if (tile * kTile >= r_act) continue;   // uniform over the workgroup

        const bool wave_active = p0 < r_act;   // uniform over the wave
        const int nrow = wave_active ? min(kWaveRows, r_act - p0) : 0;
        if (wave_active) {
            // ---- B0: row norms and the leave-one-out cosine of the wave's 16 positions (ge2e_rows_dev.hpp) ----
            const TileRows<kSteps> t = tile_rows<kSteps>(b.E, b.SS, b.CST, ix, p0, nrow, D, eps_cos);
            if (t.row_ok && q == 0) {
                float* rs = b.RST + (size_t)t.pp * 8;
                const v4f st = {t.rne, t.ke, t.rnu, t.ku};
                *reinterpret_cast<v4f*>(rs) = st;
                rs[RS_COSD] = t.cosd;
            }
            // ---- B1: cos tiles on the matrix core: unit centroids x rows, K = D; kAcc column tiles at a time ----
            float* ar = b.A + (size_t)t.pp * NAp;
            const int KT = (n_act + 15) >> 4;
            tile_cosines<kSteps, kAcc>(t, b.CH, n_act, D, [&](int kt0, const v4f (&acc)[kAcc]) {
                // the lane holds columns c0 .. c0+3 of row l15: the cosine before eps, the own column replaced
#pragma unroll
                for (int a = 0; a < kAcc; ++a) {
                    const int c0 = (kt0 + a) * 16 + 4 * q;
                    if (kt0 + a >= KT || !t.row_ok || c0 >= NAp) continue;
                    v4f v;
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int c = c0 + g;
                        v[g] = c < n_act ? (c == t.j ? t.cosd : acc[a][g] * t.rne) : 0.f;
                    }
                    *reinterpret_cast<v4f*>(ar + c0) = v;
                }
            });
        }
        __syncthreads();   // A and the row statistics of the wave's rows, written lane by lane, are read row by row

        // ---- B2: per row: loss, dL/dcos.  Four of the wave's rows at a time: lane group q takes row p0 + 4 it + q, its 16
        // lanes the centroids l15, l15 + 16, ...; a row's sums meet inside its group.  A group past the wave's last row
        // goes through the motions on the wave's first row and neither stores nor counts ----
        float loss_acc = 0.f, dw_acc = 0.f, db_acc = 0.f;
        for (int it = 0; 4 * it < nrow; ++it) {   // uniform over the wave
            const bool ok = 4 * it + q < nrow;
            const int r = p0 + (ok ? 4 * it + q : 0);
            const int j = ix.speaker_at(r);
            float* Arow = b.A + (size_t)r * NAp;
            float* rs = b.RST + (size_t)r * 8;
            const float cosd = rs[RS_COSD];
            const float sjj = w * (cosd + eps) + bias;
            float mx, best, dwr = 0.f, dbr = 0.f;
            int besti;
            row_scan<16>(Arow, l15, n_act, j, w, bias, eps, mx, best, besti);
            const RowLoss<float> rl = row_loss<16>(Arow, l15, n_act, j, sjj, w, bias, eps, log_eps, contrast, mx, best, besti,
                                                   ok, dwr, dbr);
            if (ok) {
                dw_acc += dwr;
                db_acc += dbr;
                if (l15 == 0) {
                    loss_acc += rl.per;
                    if (p.per) p.per[(size_t)bi * R + ix.row_at(r)] = rl.per;
                    rs[RS_AD] = rl.ad; rs[RS_COEF] = rl.coef;
                }
            }
        }
        loss_acc = wave_sum(loss_acc);
        dw_acc = wave_sum(dw_acc);
        db_acc = wave_sum(db_acc);
        if (lane == 0) { red[0][wid] = loss_acc; red[1][wid] = dw_acc; red[2][wid] = db_acc; }
        __syncthreads();
        if (threadIdx.x == 0) {
            float l = 0.f, a = 0.f, c = 0.f;
            for (int i = 0; i < kWaves; ++i) { l += red[0][i]; a += red[1][i]; c += red[2][i]; }
            float* pt = p.PART + ((size_t)bi * tiles + tile) * 4;
            pt[0] = l; pt[1] = a; pt[2] = c;
        }
        __syncthreads();   // red is reused by the workgroup's next item
    }
}

// ---- cos-grad rows: B0, B1 and, in place of B2, the caller's dL/dcos ---------------------------------------------------
// ge2e_cos_sim_labeled_bwd's row kernel: wide_rows_kernel's decomposition, row statistics and cosine tiles; what it leaves
// behind for gc, speakers and de is what row_loss leaves there, with a_k = g_cos[order[p]][k] for the softmax's gradient:
// A[p][k] = a_k (own column j and the padding 0), RS_AD = a_j, RS_COEF = sum_{k != j} a_k cos_k + a_j cosd (cos before eps).
// In tile_cosines' epilogue a lane holds four consecutive columns of one row: it takes the matching four words of g_cos --
// one 16-byte load where N % 4 == 0, g_cos is 16-byte aligned (vecG) and all four count, element loads otherwise -- and
// keeps a partial of coef over its columns in ascending order; the four lanes of a row join theirs as tile_rows does.  No
// barrier, no second pass over A.  The loads of a group of kAcc tiles are issued behind the MFMAs of the group before it
// (the first group's ahead of the stage) and stay in flight over the group's own MFMAs.  Every address is inside the
// buffers and names an entry that counts (a column past n_act reads column 0, a lane past the wave's last row the wave's
// first row, and a select drops the value): rows and columns of g_cos that do not count are never read.
template <int kSteps>
__global__ __launch_bounds__(kThreads) void labeled_cos_grad_rows_kernel(ProblemLabeledWide p, const float* g_cos, int tiles) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int q = lane >> 4;
    const int D = p.D, R = p.R, N = p.N, NA = p.NA;
    const int NAp = (NA + 3) & ~3;
    const float eps_cos = p.eps_cos;
    const bool vecG = (N & 3) == 0 && ((uintptr_t)g_cos & 15) == 0;

    const long long items = (long long)p.B * tiles;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int bi = (int)(item / tiles), tile = (int)(item - (long long)bi * tiles);
        const IndexView ix = index_view(p, bi, kRowsNeedSpeaker);
        const int n_act = ix.n_act, r_act = ix.r_act;
        const int p0 = tile * kTile + wid * kWaveRows;
        if (p0 >= r_act) continue;   // uniform over the wave; no barrier in this kernel
        const RowPlanes b = row_planes(p, bi, NAp);
        const int nrow = min(kWaveRows, r_act - p0);

        const TileRows<kSteps> t = tile_rows<kSteps>(b.E, b.SS, b.CST, ix, p0, nrow, D, eps_cos);
        float* rs = b.RST + (size_t)t.pp * 8;
        if (t.row_ok && q == 0) {
            const v4f st = {t.rne, t.ke, t.rnu, t.ku};
            *reinterpret_cast<v4f*>(rs) = st;
            rs[RS_COSD] = t.cosd;
        }
        const float* gr = g_cos + ((size_t)bi * R + t.row) * N;   // (!row_ok: the wave's first row, an active one)
        float* ar = b.A + (size_t)t.pp * NAp;
        const int KT = (n_act + 15) >> 4;
        // the lane's four words of g_cos in every tile of the group that starts at tile kt0
        v4f gnext[kAcc];
        auto load_g = [&](int kt0) {
#pragma unroll
            for (int a = 0; a < kAcc; ++a) {
                const int c0 = (kt0 + a) * 16 + 4 * q;
                if (vecG && c0 + 3 < n_act) {   // (the four count: only the lanes at the row's last columns go the other way)
                    gnext[a] = *reinterpret_cast<const v4f*>(gr + c0);
                } else {
#pragma unroll
                    for (int g = 0; g < 4; ++g) gnext[a][g] = gr[c0 + g < n_act ? c0 + g : 0];
                }
            }
        };
        load_g(0);
        float coef = 0.f;
        tile_cosines<kSteps, kAcc>(t, b.CH, n_act, D, [&](int kt0, const v4f (&acc)[kAcc]) {
            v4f gc[kAcc];
#pragma unroll
            for (int a = 0; a < kAcc; ++a) gc[a] = gnext[a];
            if (kt0 + kAcc < KT) load_g(kt0 + kAcc);   // uniform over the wave
#pragma unroll
            for (int a = 0; a < kAcc; ++a) {
                const int c0 = (kt0 + a) * 16 + 4 * q;
                if (kt0 + a >= KT || !t.row_ok || c0 >= NAp) continue;
                v4f v;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int c = c0 + g;
                    const bool in = c < n_act, own = c == t.j;
                    const float ak = in ? gc[a][g] : 0.f;
                    if (in) coef += ak * (own ? t.cosd : acc[a][g] * t.rne);
                    if (own) rs[RS_AD] = ak;
                    v[g] = own ? 0.f : ak;
                }
                *reinterpret_cast<v4f*>(ar + c0) = v;
            }
        });
        // lanes l15, l15 + 16, l15 + 32, l15 + 48: (q0 + q1) + (q2 + q3) in every lane, as in tile_rows
        auto s16 = GE2E_SWAP16(__float_as_uint(coef));
        const float h = __uint_as_float(s16[0]) + __uint_as_float(s16[1]);
        auto s32 = GE2E_SWAP32(__float_as_uint(h));
        coef = __uint_as_float(s32[0]) + __uint_as_float(s32[1]);
        if (t.row_ok && q == 0) rs[RS_COEF] = coef;
    }
}

// ---- sums: loss, dw, db of every batch ------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void wide_sums_kernel(ProblemLabeledWide p, int tiles) {
    const int lane = threadIdx.x & 63;
    const long long nwaves = (long long)gridDim.x * kWaves;
    for (long long wv = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6); wv < p.B; wv += nwaves) {
        const int bi = (int)wv;
        const int r_act = index_r_act(p.active, (size_t)bi, p.R, index_n_act(p.active, (size_t)bi, p.NA), kRowsNeedSpeaker);
        const int nt = min((r_act + kTile - 1) / kTile, tiles);
        float l = 0.f, a = 0.f, c = 0.f;
        for (int t = lane; t < nt; t += kWave) {
            const float* pt = p.PART + ((size_t)bi * tiles + t) * 4;
            l += pt[0]; a += pt[1]; c += pt[2];
        }
        l = wave_sum(l); a = wave_sum(a); c = wave_sum(c);
        if (lane == 0) {
            p.loss[bi] = l;
            if (p.dw) p.dw[bi] = a;
            if (p.db) p.db[bi] = c;
        }
    }
}

// ---- gc: phase C1 ---------------------------------------------------------------------------------------------------------
// One wave per (batch, piece, kGcTiles tiles of 16 speakers, slab of 64 columns).  Operand map: A[i = l15 <-> speaker]
// [k = q], B[k = q][j = l15 <-> column], C[i = 4 q + g][j = l15]; in step s of a 64-row block lane group q takes position
// 4 s + q.  A block always takes its 16 steps, unrolled and free of branches, so the loads of many steps are in flight
// together: every load happens, at an address inside the buffers (a position past the piece's end reads the piece's
// last row, an absent speaker or column reads number 0), and a select zeroes what does not count.
__global__ __launch_bounds__(kThreads) void wide_gc_kernel(ProblemLabeledWide p, int S, int KTc, int DB) {
    const int lane = threadIdx.x & 63;
    const int l15 = lane & 15, q = lane >> 4;
    const int D = p.D, NA = p.NA;
    const int NAp = (NA + 3) & ~3;
    const v4f zero4 = {0.f, 0.f, 0.f, 0.f};
    const long long per_batch = (long long)S * KTc * DB;
    const long long items = (long long)p.B * per_batch, nwaves = (long long)gridDim.x * kWaves;
    for (long long item = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6); item < items; item += nwaves) {
        const int bi = (int)(item / per_batch);
        long long rem = item - (long long)bi * per_batch;
        const int piece = (int)(rem / ((long long)KTc * DB));
        rem -= (long long)piece * KTc * DB;
        const int kt = (int)(rem / DB), db = (int)(rem - (long long)kt * DB);
        const IndexView ix = index_view(p, bi, kRowsNeedSpeaker);
        const int n_act = ix.n_act, r_act = ix.r_act;
        const int k_base = kt * 16 * kGcTiles;
        if (k_base >= n_act) continue;   // uniform over the wave
        // the piece's rows: whole blocks of 64, the same cut for every wave of the batch
        const int len = ((r_act + S - 1) / S + kWave - 1) / kWave * kWave;
        const int r_begin = min(piece * len, r_act), r_end = min(r_begin + len, r_act);
        const RowPlanes pl = row_planes(p, bi, NAp);
        int ka[kGcTiles], dcol[kAcc];
        bool ka_ok[kGcTiles], d_ok[kAcc];
#pragma unroll
        for (int u = 0; u < kGcTiles; ++u) {
            ka_ok[u] = k_base + u * 16 + l15 < n_act;
            ka[u] = ka_ok[u] ? k_base + u * 16 + l15 : 0;
        }
#pragma unroll
        for (int t = 0; t < kAcc; ++t) {
            d_ok[t] = db * kSlab + t * 16 + l15 < D;
            dcol[t] = d_ok[t] ? db * kSlab + t * 16 + l15 : 0;
        }
        v4f acc[kGcTiles][kAcc];
#pragma unroll
        for (int u = 0; u < kGcTiles; ++u)
#pragma unroll
            for (int t = 0; t < kAcc; ++t) acc[u][t] = zero4;
        for (int rb = r_begin; rb < r_end; rb += kWave) {
            const int idx = ix.row_at(min(rb + lane, r_end - 1));   // one coalesced load for 64 positions
            // kGcAhead steps at a time: all their loads, then all their MFMAs (left alone, the scheduler sinks every load
            // to the step that uses it and a step waits out a round trip to L2)
#pragma unroll
            for (int s0 = 0; s0 < kWave / 4; s0 += kGcAhead) {
                float ra[kGcAhead][kGcTiles], rb4[kGcAhead][kAcc], rne[kGcAhead];
                bool r_ok[kGcAhead];
#pragma unroll
                for (int i = 0; i < kGcAhead; ++i) {
                    const int s = s0 + i;
                    const int i0 = __builtin_amdgcn_readlane(idx, 4 * s), i1 = __builtin_amdgcn_readlane(idx, 4 * s + 1);
                    const int i2 = __builtin_amdgcn_readlane(idx, 4 * s + 2), i3 = __builtin_amdgcn_readlane(idx, 4 * s + 3);
                    const int row = q == 0 ? i0 : q == 1 ? i1 : q == 2 ? i2 : i3;
                    r_ok[i] = rb + 4 * s + q < r_end;
                    const int r = min(rb + 4 * s + q, r_end - 1);
                    rne[i] = pl.RST[(size_t)r * 8 + RS_RNE];
                    const float* ar = pl.A + (size_t)r * NAp;
                    const float* er = pl.E + (size_t)row * D;
#pragma unroll
                    for (int u = 0; u < kGcTiles; ++u) ra[i][u] = ar[ka[u]];
#pragma unroll
                    for (int t = 0; t < kAcc; ++t) rb4[i][t] = er[dcol[t]];
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < kGcAhead; ++i) {
                    float a[kGcTiles], b[kAcc];
#pragma unroll
                    for (int u = 0; u < kGcTiles; ++u) a[u] = (ka_ok[u] && r_ok[i]) ? ra[i][u] * rne[i] : 0.f;
#pragma unroll
                    for (int t = 0; t < kAcc; ++t) b[t] = (d_ok[t] && r_ok[i]) ? rb4[i][t] : 0.f;
#pragma unroll
                    for (int u = 0; u < kGcTiles; ++u)
#pragma unroll
                        for (int t = 0; t < kAcc; ++t) acc[u][t] = mfma_f32(a[u], b[t], acc[u][t]);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        float* out = S > 1 ? p.GCP + ((size_t)bi * S + piece) * NA * D : p.GC + (size_t)bi * NA * D;
#pragma unroll
        for (int u = 0; u < kGcTiles; ++u)
#pragma unroll
            for (int t = 0; t < kAcc; ++t)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int k = k_base + u * 16 + 4 * q + g;
                    if (k < n_act && d_ok[t]) out[(size_t)k * D + dcol[t]] = acc[u][t][g];
                }
    }
}

// ---- speakers: phase C2 ---------------------------------------------------------------------------------------------------
// One wave per (batch, compact speaker).  A lane owns 4 (D % 4 == 0) or 1 element of every stretch of 256 / 64 columns.
__global__ __launch_bounds__(kThreads) void wide_speakers_kernel(ProblemLabeledWide p, int S) {
    const int lane = threadIdx.x & 63;
    const int D = p.D, R = p.R, NA = p.NA;
    const bool vecD = (D & 3) == 0;
    const int stretch = vecD ? 4 * kWave : kWave;
    const long long total = (long long)p.B * NA, nwaves = (long long)gridDim.x * kWaves;
    for (long long wv = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6); wv < total; wv += nwaves) {
        const int bi = (int)(wv / NA), k = (int)(wv - (long long)bi * NA);
        const IndexView ix = index_view(p, bi, kRowsNeedSpeaker);
        if (k >= ix.n_act) continue;
        const auto [r0, r1] = ix.span(k);
        const float* E = p.E + (size_t)bi * R * D;
        const float* RSTb = p.RST + (size_t)bi * R * 8;
        const size_t at = ((size_t)bi * NA + k) * D;
        const float* CH = p.CH + at;
        const float* SS = p.SS + at;
        float* GC = p.GC + at;
        float* DUS = p.DUS + at;
        const float* cs = p.CST + ((size_t)bi * NA + k) * 4;
        const float rn = cs[CS_RN], kap = cs[CS_KAP], fm1 = cs[CS_M1];

        // dL/d c-hat: the pieces in ascending order; its product with c-hat
        float coef = 0.f;
        for (int d0 = 0; d0 < D; d0 += stretch) {
            const int d = d0 + (vecD ? 4 * lane : lane);
            if (d >= D) continue;
            v4f g = {0.f, 0.f, 0.f, 0.f};
            if (S > 1) {
                for (int s = 0; s < S; ++s) {
                    const float* gp = p.GCP + (((size_t)bi * S + s) * NA + k) * D;
                    g += load_own(gp, d, vecD);
                }
                store_own(GC, d, g, vecD);
            } else {
                g = load_own(GC, d, vecD);
            }
            const v4f c = load_own(CH, d, vecD);
#pragma unroll
            for (int t = 0; t < 4; ++t) coef += g[t] * c[t];
        }
        coef = wave_sum(coef);
        for (int d0 = 0; d0 < D; d0 += stretch) {   // (every lane reads back what it wrote itself)
            const int d = d0 + (vecD ? 4 * lane : lane);
            const bool ok = d < D;
            v4f ss = {0.f, 0.f, 0.f, 0.f};
            if (ok) {
                const v4f c = load_own(CH, d, vecD);
                const v4f g = load_own(GC, d, vecD);
                ss = load_own(SS, d, vecD);
                v4f o;
#pragma unroll
                for (int t = 0; t < 4; ++t) o[t] = (g[t] - kap * coef * c[t]) * rn;
                store_own(GC, d, o, vecD);
            }
            // the speaker's sum of dL/du, rows in ascending position
            v4f dus = {0.f, 0.f, 0.f, 0.f};
            for (int c0 = r0; c0 < r1; c0 += kWave) {
                const int pp = c0 + lane;
                const int idx = pp < r1 ? ix.row_at(pp) : 0;   // one coalesced load for up to 64 rows
                const int cnt = min(kWave, r1 - c0);
                for (int i = 0; i < cnt; ++i) {
                    const float* er = E + (size_t)__builtin_amdgcn_readlane(idx, i) * D;
                    const float* rs = RSTb + (size_t)(c0 + i) * 8;
                    const float rne = rs[RS_RNE], rnu = rs[RS_RNU], ku = rs[RS_KU], cosd = rs[RS_COSD], ad = rs[RS_AD];
                    if (ok) {
                        const v4f e = load_own(er, d, vecD);
#pragma unroll
                        for (int t = 0; t < 4; ++t) dus[t] += loo_term(e[t], ss[t], fm1, rne, rnu, ku, cosd, ad).du;
                    }
                }
            }
            if (ok) store_own(DUS, d, dus, vecD);
        }
    }
}

// ---- de: phase D1 ---------------------------------------------------------------------------------------------------------
// One workgroup per (batch, tile of 64 positions, slab of 64 columns), 16 positions per wave.  Operand map:
// A[i = l15 <-> column][k = q] = CH[k][column], B[k = q][j = l15 <-> row] = A[row][k], C[i = 4 q + g][j = l15]: a lane ends
// with four consecutive columns of one row.  Lane group q takes k0 + 4 q + s in step s: one 16-byte load of the row of A.
__global__ __launch_bounds__(kThreads) void wide_de_kernel(ProblemLabeledWide p, int tiles, int DB) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int l15 = lane & 15, q = lane >> 4;
    const int D = p.D, R = p.R, NA = p.NA;
    const int NAp = (NA + 3) & ~3;
    const bool vecD = (D & 3) == 0;
    const v4f zero4 = {0.f, 0.f, 0.f, 0.f};
    const long long per_batch = (long long)tiles * DB;
    const long long items = (long long)p.B * per_batch;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int bi = (int)(item / per_batch);
        const long long rem = item - (long long)bi * per_batch;
        const int tile = (int)(rem / DB), db = (int)(rem - (long long)tile * DB);
        const IndexView ix = index_view(p, bi, kRowsNeedSpeaker);
        const int n_act = ix.n_act, r_act = ix.r_act;
        float* dE = p.dE + (size_t)bi * R * D;
        const int p0 = tile * kTile + wid * kWaveRows;
        const int pp = p0 + l15;
        if (p0 >= R) continue;   // uniform over the wave; no barrier in this kernel
        const bool in_R = pp < R, row_ok = pp < r_act;
        const int my_row = ix.row_at(in_R ? pp : p0);
        float* out = dE + (size_t)my_row * D;
        if (p0 >= r_act) {   // uniform over the wave: nothing counts here
            if (in_R) {
#pragma unroll
                for (int t = 0; t < kAcc; ++t) {
                    const int d0 = db * kSlab + t * 16 + 4 * q;
                    if (d0 < D) store4(out, d0, D, zero4, vecD);
                }
            }
            continue;
        }
        const int my_pp = row_ok ? pp : p0;   // (p0 is an active position: readable)
        const int sp = ix.speaker_at(my_pp);
        const float* pa = p.A + ((size_t)bi * R + my_pp) * NAp;
        const float* CHb = p.CH + (size_t)bi * NA * D;
        v4f acc[kAcc];
#pragma unroll
        for (int t = 0; t < kAcc; ++t) acc[t] = zero4;
        int dc[kAcc];
        bool dc_ok[kAcc];
#pragma unroll
        for (int t = 0; t < kAcc; ++t) {
            dc_ok[t] = db * kSlab + t * 16 + l15 < D;
            dc[t] = dc_ok[t] ? db * kSlab + t * 16 + l15 : 0;
        }
        // kDeAhead steps of 16 speakers at a time: all their loads, then all their MFMAs, free of branches (see gc).  Every
        // load happens inside the buffers -- a speaker past n_act reads speaker 0, a column past D column 0 -- and a select
        // zeroes what does not count.  kq < n_act: the four words are inside the row of NAp.
        for (int k0 = 0; k0 < n_act; k0 += 16 * kDeAhead) {
            v4f ra[kDeAhead];
            float rc[kDeAhead][4][kAcc];
#pragma unroll
            for (int i = 0; i < kDeAhead; ++i) {
                const int kq = k0 + 16 * i + 4 * q;
                ra[i] = *reinterpret_cast<const v4f*>(pa + (kq < n_act ? kq : 0));
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float* cr = CHb + (size_t)(kq + s < n_act ? kq + s : 0) * D;
#pragma unroll
                    for (int t = 0; t < kAcc; ++t) rc[i][s][t] = cr[dc[t]];
                }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < kDeAhead; ++i) {
                const int kq = k0 + 16 * i + 4 * q;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const bool k_ok = kq + s < n_act;
                    const float av = (k_ok && row_ok) ? ra[i][s] : 0.f;
#pragma unroll
                    for (int t = 0; t < kAcc; ++t) acc[t] = mfma_f32((k_ok && dc_ok[t]) ? rc[i][s][t] : 0.f, av, acc[t]);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (!in_R) continue;
        if (!row_ok) {
#pragma unroll
            for (int t = 0; t < kAcc; ++t) {
                const int d0 = db * kSlab + t * 16 + 4 * q;
                if (d0 < D) store4(out, d0, D, zero4, vecD);
            }
            continue;
        }
        const float* rs = p.RST + ((size_t)bi * R + pp) * 8;
        const v4f r0 = *reinterpret_cast<const v4f*>(rs), r1 = *reinterpret_cast<const v4f*>(rs + 4);
        const float rne = r0[RS_RNE], ke = r0[RS_KE], rnu = r0[RS_RNU], ku = r0[RS_KU];
        const float cosd = r1[RS_COSD - 4], ad = r1[RS_AD - 4], coef = r1[RS_COEF - 4];
        const v4f cst = *reinterpret_cast<const v4f*>(p.CST + ((size_t)bi * NA + sp) * 4);
        const float fm = cst[CS_M], fm1 = cst[CS_M1];
        const size_t at = ((size_t)bi * NA + sp) * D;
        const float* er = p.E + ((size_t)bi * R + my_row) * D;
#pragma unroll
        for (int t = 0; t < kAcc; ++t) {
            const int d0 = db * kSlab + t * 16 + 4 * q;
            if (d0 >= D) continue;
            const v4f e = load4(er, d0, D, true, vecD);
            const v4f ss = load4(p.SS + at, d0, D, true, vecD);
            const v4f gc = load4(p.GC + at, d0, D, true, vecD);
            const v4f dus = load4(p.DUS + at, d0, D, true, vecD);
            v4f o;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const LooTerm<float> lo = loo_term(e[g], ss[g], fm1, rne, rnu, ku, cosd, ad);
                const float ge = acc[t][g] + ad * lo.uh;
                o[g] = (ge - ke * coef * lo.eh) * rne + gc[g] / fm + (dus[g] - lo.du) / fm1;
            }
            store4(out, d0, D, o, vecD);
        }
    }
}

unsigned blocks_for(long long items, long long per_block = 1) {
    return (unsigned)std::max<long long>(1, std::min<long long>((items + per_block - 1) / per_block, kMaxBlocks));
}

// The front of both chains: the centroid launch (what labeled_eval_centroids_kernel<true> reads and writes, from the wide
// problem), then the chain's rows kernel, one workgroup per (batch, tile): rows(ks, grid, tiles) launches its instantiation.
template <class Rows>
hipError_t launch_wide_front(const ProblemLabeledWide& p, hipStream_t stream, Rows&& rows) {
    ProblemLabeledEval c{};
    c.E = p.E; c.off = p.off; c.order = p.order; c.active = p.active;
    c.CH = p.CH; c.SS = p.SS; c.CST = p.CST; c.spk = p.spk;
    c.B = p.B; c.N = p.N; c.R = p.R; c.D = p.D; c.NA = p.NA;
    c.eps_cos = p.eps_cos; c.eps = p.eps;
    const hipError_t err = launch_labeled_centroids(c, true, stream);
    if (err != hipSuccess) return err;
    const int tiles = wide_tiles(p.R);
    dispatch_tile_steps(p.D, [&](auto ks) { rows(ks, dim3(blocks_for((long long)p.B * tiles)), tiles); });
    return hipGetLastError();
}
}  // namespace

hipError_t launch_labeled_wide(const ProblemLabeledWide& p, hipStream_t stream) {
    hipError_t err = launch_wide_front(p, stream, [&](auto ks, dim3 grid, int tiles) {
        hipLaunchKernelGGL((wide_rows_kernel<decltype(ks)::value>), grid, dim3(kThreads), 0, stream, p, tiles);
    });
    if (err != hipSuccess) return err;

    hipLaunchKernelGGL(wide_sums_kernel, dim3(blocks_for(p.B, kWaves)), dim3(kThreads), 0, stream, p, wide_tiles(p.R));
    if ((err = hipGetLastError()) != hipSuccess || !p.dE) return err;

    return launch_labeled_wide_backward(p, stream);
}

hipError_t launch_labeled_wide_backward(const ProblemLabeledWide& p, hipStream_t stream) {
    hipError_t err;
    const int tiles = wide_tiles(p.R);
    const int S = wide_split(p.R), KTc = (p.NA + 16 * kGcTiles - 1) / (16 * kGcTiles), DB = (p.D + kSlab - 1) / kSlab;
    hipLaunchKernelGGL(wide_gc_kernel, dim3(blocks_for((long long)p.B * S * KTc * DB, kWaves)), dim3(kThreads), 0, stream, p,
                       S, KTc, DB);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    hipLaunchKernelGGL(wide_speakers_kernel, dim3(blocks_for((long long)p.B * p.NA, kWaves)), dim3(kThreads), 0, stream, p, S);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    hipLaunchKernelGGL(wide_de_kernel, dim3(blocks_for((long long)p.B * tiles * DB)), dim3(kThreads), 0, stream, p, tiles, DB);
    return hipGetLastError();
}

hipError_t launch_labeled_cos_grad(const ProblemLabeledWide& p, const float* g_cos, hipStream_t stream) {
    const hipError_t err = launch_wide_front(p, stream, [&](auto ks, dim3 grid, int tiles) {
        hipLaunchKernelGGL((labeled_cos_grad_rows_kernel<decltype(ks)::value>), grid, dim3(kThreads), 0, stream, p, g_cos, tiles);
    });
    if (err != hipSuccess) return err;
    return launch_labeled_wide_backward(p, stream);
}

}  // namespace ge2e
