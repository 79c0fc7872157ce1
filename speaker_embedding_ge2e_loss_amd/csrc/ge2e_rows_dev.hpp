// Device helpers of the exact kernels, written once: ge2e_generic.hip, ge2e_f64.hip, ge2e_ragged.hip,
// ge2e_labeled_wide.hip, ge2e_labeled_eval.hip and the bank kernels (ge2e_enroll.hip, ge2e_identify.hip, ge2e_snorm.hip).
// The statistic indices, the reader of the label index tables (IndexView), the 16-byte fragment loads of the fp32 MFMA, the
// row-loss step (row_scan, row_loss), the leave-one-out gradient term (loo_term), the cosine-tile stage of the row kernels
// (tile_rows, tile_rows_plain, tile_cosines) with the geometry of a workgroup that runs it (tile_geom), and the speaker sum
// and the unit scaling of the centroid and enrolment kernels (speaker_sum, mean_sq, unit_scale).  Algebra:
// oracle/ge2e_oracle.py:closed_form and the header of
// ge2e_generic.hip.  The operand order and the parentheses of every expression are part of the results: the kernels agree
// bit for bit with what they computed when each carried its own copy (tools/output_digest.py).
#pragma once
#include <math.h>

#include "ge2e_common.hpp"

namespace ge2e {

// row statistics [row][8] and centroid statistics [speaker][4] (the f64 kernel keeps the first two of the latter)
constexpr int RS_RNE = 0, RS_KE = 1, RS_RNU = 2, RS_KU = 3, RS_COSD = 4, RS_AD = 5, RS_COEF = 6;
constexpr int CS_RN = 0, CS_KAP = 1, CS_M = 2, CS_M1 = 3;

typedef float v4f __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// ---- the one reader of the index tables ----------------------------------------------------------------------------------
// An index kernel (ge2e_labels.hip) has left offsets [B][N+1], order [B][R] and active [B][2] = {n_act, r_act}; the centroid
// kernel adds spk [B][R], the compact speaker of every sorted position.  Every kernel behind them reads the tables here
// and nowhere else, under ONE contract: n_act and r_act are clamped to [0, n_bound] and [0, R] where they are read, every
// offset to [0, r_act], every row index to [0, R-1], every speaker id to [0, n_act-1]: whatever the memory holds, no
// access leaves the buffers and no loop over them is unbounded.  n_bound: the speakers the reader's planes are laid out for
// (speaker_capacity, enroll_capacity), or the caller's N where active is the caller's.  (ge2e_ragged.hip is no client: its
// gather trusts the permutation the index kernel writes, and its offsets may be the caller's.)
__device__ __forceinline__ int index_n_act(const int* active, size_t bi, int n_bound) { return clampi(active[bi * 2], 0, n_bound); }
// `rows_need_speaker`: r_act = 0 where n_act = 0 (the wide route, whose kernels ask r_act alone whether there is work); the
// evaluation kernels ask n_act first and take r_act as it stands.
__device__ __forceinline__ int index_r_act(const int* active, size_t bi, int R, int n_act, bool rows_need_speaker = false) {
    return (rows_need_speaker && n_act == 0) ? 0 : clampi(active[bi * 2 + 1], 0, R);
}
struct IndexSpan { int r0, r1; };   // the sorted positions r0 .. r1 - 1 of a compact speaker (r1 >= r0 whatever off holds)
__device__ __forceinline__ IndexSpan index_span(const int* off, int k, int r_act) {   // off: the batch's; k < n_act
    const int r0 = clampi(off[k], 0, r_act);
    return {r0, max(clampi(off[k + 1], 0, r_act), r0)};
}
__device__ __forceinline__ int index_row(const int* order, int p, int R) { return clampi(order[p], 0, R - 1); }   // p < R
// One batch's tables and extents, of a launch description that carries them (ProblemLabeledEval, ProblemLabeledWide).
struct IndexView {
    const int *off, *order, *spk;   // the batch's offsets [N+1], order [R], spk [R]
    int R, n_act, r_act;
    __device__ __forceinline__ IndexSpan span(int k) const { return index_span(off, k, r_act); }
    __device__ __forceinline__ int row_at(int p) const { return index_row(order, p, R); }
    __device__ __forceinline__ int speaker_at(int p) const { return clampi(spk[p], 0, n_act - 1); }   // p < r_act
};
template <class P>
__device__ __forceinline__ IndexView index_view(const P& p, int bi, bool rows_need_speaker = false) {
    const size_t b = (size_t)bi;
    const int n_act = index_n_act(p.active, b, p.NA);
    const int r_act = index_r_act(p.active, b, p.R, n_act, rows_need_speaker);
    return {p.off + b * ((size_t)p.N + 1), p.order + b * p.R, p.spk + b * p.R, p.R, n_act, r_act};
}

__device__ __forceinline__ v4f mfma_f32(float a, float b, v4f c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// Elements k .. k+3 of a row of `len` floats (k a multiple of 4), zero where the row is absent or ends.  `vec`: the row
// starts 16-byte aligned and len is a multiple of 4, so the four are there together or not at all.
__device__ __forceinline__ v4f load4(const float* row, int k, int len, bool row_ok, bool vec) {
    v4f v = {0.f, 0.f, 0.f, 0.f};
    if (vec) {
        if (row_ok && k < len) v = *reinterpret_cast<const v4f*>(row + k);
    } else {
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (row_ok && k + s < len) v[s] = row[k + s];
    }
    return v;
}
// The same without a branch, for a 16-byte aligned row whose length is a multiple of 4: the load always happens, at
// element 0 where k is past the row, and a select zeroes it.  `row` must be readable whatever `ok` says.
__device__ __forceinline__ v4f load4_always(const float* row, int k, int len, bool ok) {
    const bool in = k < len;
    const v4f v = *reinterpret_cast<const v4f*>(row + (in ? k : 0));
    const v4f z = {0.f, 0.f, 0.f, 0.f};
    return (ok && in) ? v : z;
}
// ... and without the select, for the centroid side of the cosines: past the row's end the E fragment is zero, so
// whatever (finite) centroid element stands there adds nothing, and a centroid row that does not exist (its pointer is
// row 0's) only feeds columns that the epilogue drops.  No use of the value next to the load: it can stay in flight.
__device__ __forceinline__ v4f load4_raw(const float* row, int k, int len) {
    return *reinterpret_cast<const v4f*>(row + (k < len ? k : 0));
}
__device__ __forceinline__ void store4(float* row, int k, int len, const v4f& v, bool vec) {
    if (vec) {
        *reinterpret_cast<v4f*>(row + k) = v;
    } else {
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (k + s < len) row[k + s] = v[s];
    }
}

// exp, log and max of the row-loss step's scalar type: the float form keeps the fp32 calls
__device__ __forceinline__ float exp_t(float x) { return expf(x); }
__device__ __forceinline__ double exp_t(double x) { return exp(x); }
__device__ __forceinline__ float log_t(float x) { return logf(x); }
__device__ __forceinline__ double log_t(double x) { return log(x); }
__device__ __forceinline__ float max_t(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double max_t(double a, double b) { return fmax(a, b); }

// ---- the row-loss step (phase B2) --------------------------------------------------------------------------------------
// One row of A = cos before eps, N columns, own-speaker column j (whose score is sjj = w (cosd + eps) + bias), on an aligned
// group of W lanes of which this one is lane l: lane l takes the columns l, l + W, ...
// row_scan: the scores S_k = w (cos_k + eps) + bias, this lane's maximum and its best other speaker (lowest index first).
template <int W, class T>
__device__ __forceinline__ void row_scan(const T* Arow, int l, int N, int j, T w, T bias, T eps, T& mx, T& best, int& besti) {
    mx = -INFINITY; best = -INFINITY;
    besti = 0x7fffffff;
    for (int k = l; k < N; k += W) {
        const T s = w * (Arow[k] + eps) + bias;
        mx = max_t(mx, s);
        if (k != j && s > best) { best = s; besti = k; }
    }
}
// row_loss: from the lanes' mx / best / besti to the row's loss `per`, coef = (dL/dcos) . cos and ad = dL/dcos on the own
// column, all three in every lane of the group.  dw and db take this lane's share of the row's dL/dw and dL/db.  `store`:
// dL/dcos goes back into Arow with the own column zeroed (a group that only goes through the motions does not store).
template <class T>
struct RowLoss { T per, coef, ad; };
template <int W, class T>
__device__ __forceinline__ RowLoss<T> row_loss(T* Arow, int l, int N, int j, T sjj, T w, T bias, T eps, T log_eps, bool contrast,
                                               T mx, T best, int besti, bool store, T& dw, T& db) {
    T per, coef = 0, ad = 0;
    if (!contrast) {
        mx = max_t(group_max<W>(mx), log_eps);
        // z_off = everything except the own-speaker term: 1 - p_jj = z_off / z has no cancellation when the softmax is
        // peaked on the diagonal (trained embeddings)
        T zoff = 0;
        for (int k = l; k < N; k += W)
            if (k != j) zoff += exp_t(w * (Arow[k] + eps) + bias - mx);
        zoff = group_sum<W>(zoff) + exp_t(log_eps - mx);
        const T z = zoff + exp_t(sjj - mx);
        per = (mx - sjj) + log_t(z);
        const T rz = T(1) / z;
        for (int k = l; k < N; k += W) {
            const T c0 = Arow[k];
            const T g = (k == j) ? -zoff * rz : exp_t(w * (c0 + eps) + bias - mx) * rz;
            dw += g * (c0 + eps);
            db += g;
            const T a = w * g;
            coef += a * c0;
            if (k == j) ad = a;
            if (store) Arow[k] = (k == j) ? T(0) : a;
        }
    } else {
        group_argmax<W>(best, besti);
        const T pos = T(1) / (T(1) + exp_t(-sjj));
        const T neg = (N > 1) ? T(1) / (T(1) + exp_t(-best)) : T(0);
        per = T(1) - pos + neg;
        for (int k = l; k < N; k += W) {
            const T c0 = Arow[k];
            T g = 0;
            if (k == j) g = -pos * (T(1) - pos);
            else if (k == besti) g = neg * (T(1) - neg);
            dw += g * (c0 + eps);
            db += g;
            const T a = w * g;
            coef += a * c0;
            if (k == j) ad = a;
            if (store) Arow[k] = (k == j) ? T(0) : a;
        }
    }
    return {per, group_sum<W>(coef), group_sum<W>(ad)};
}

// ---- the leave-one-out gradient term -----------------------------------------------------------------------------------
// Element e of a row and s of its speaker's sum: eh = e-hat, uh = u-hat (u = (s - e) / (m - 1), the leave-one-out centroid)
// and du = dL/du-hat through u's norm, from the row's statistics.
template <class T>
struct LooTerm { T eh, uh, du; };
template <class T>
__device__ __forceinline__ LooTerm<T> loo_term(T e, T s, T fm1, T rne, T rnu, T ku, T cosd, T ad) {
    LooTerm<T> t;
    t.eh = e * rne;
    t.uh = (s - e) / fm1 * rnu;
    t.du = ad * (t.eh - ku * cosd * t.uh) * rnu;
    return t;
}

// ---- the cosine-tile stage of the labelled row kernels -------------------------------------------------------------------
// A wave and its 16 sorted positions p0 .. p0 + 15, of which the first nrow >= 1 count.  Operand map of
// v_mfma_f32_16x16x4_f32 (lane l, l15 = l & 15, q = l >> 4): A[i = l15][k = q] = CH[kt 16 + l15][..], B[k = q][j = l15] =
// E[row l15][..]; result C[i = 4 q + g][j = l15]: a lane ends with FOUR CONSECUTIVE COLUMNS of ONE row.  The k index is
// permuted the same way in both operands (lane group q takes d0 + 4 q + s in step s): one 16-byte load per operand and step
// where D % 4 == 0.
// kSteps > 0: D is a multiple of 4 and at most 16 kSteps.  The wave's E fragments stay in registers over all column tiles
// and every loop over k is unrolled and free of branches, so the loads run ahead of the MFMAs that use them: the row
// fragments all at once, the centroid fragments kAhead steps ahead in a ring of registers.  (With a branch per step the
// kernel waited out one L2 round trip per 16 MFMAs; DESIGN.md 3.4e has the figures.)
// kSteps == 0: any D; a plain loop over k that loads as it goes (L1 / L2), rows and centroids alike.
template <int kSteps>
struct TileRows {
    bool row_ok;        // the lane's position p0 + l15 is one of the nrow
    int pp, row, j;     // the position (p0 where !row_ok), its row of E through order, its compact speaker (-1 where !row_ok)
    float rne, ke, rnu, ku, cosd;
    const float* pe;    // the row of E
    v4f eh[kSteps > 0 ? kSteps : 1];   // (kSteps > 0) its fragments
};
// Row norms and the leave-one-out cosine from the explicit difference SS[j] - e_r, all 16 rows at once on the MFMA's own row
// fragments: index, speaker and m - 1 come with one load each for the whole wave (no dependent chain per row), lane group q
// holds the elements d0 + 4 q .. + 3 of every step, and the four groups' partial sums meet through two lane swaps in a
// fixed order.  The lanes past the wave's last row point at its first one (an active row: readable) and zero what they
// load.  ix: the batch's tables, which clamp every index where it is read.
template <int kSteps>
__device__ __forceinline__ TileRows<kSteps> tile_rows(const float* E, const float* SSb, const float* CSTb, const IndexView& ix,
                                                      int p0, int nrow, int D, float eps_cos) {
    constexpr bool kHold = kSteps > 0;
    const int l15 = threadIdx.x & 15, q = (threadIdx.x & 63) >> 4;
    TileRows<kSteps> t;
    t.row_ok = l15 < nrow;
    t.pp = p0 + (t.row_ok ? l15 : 0);
    t.row = ix.row_at(t.pp);
    const int sp = ix.speaker_at(t.pp);
    t.j = t.row_ok ? sp : -1;
    const float fm1 = CSTb[(size_t)sp * 4 + CS_M1];
    t.pe = E + (size_t)t.row * D;
    const float* ps = SSb + (size_t)sp * D;
    float ee = 0.f, uu = 0.f, eu = 0.f;
    auto row_step = [&](const v4f& sj, const v4f& e) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float u = (sj[i] - e[i]) / fm1;
            ee += e[i] * e[i]; uu += u * u; eu += e[i] * u;
        }
    };
    if constexpr (kHold) {
        v4f sh[kSteps];
#pragma unroll
        for (int s = 0; s < kSteps; ++s) t.eh[s] = load4_always(t.pe, 16 * s + 4 * q, D, t.row_ok);
#pragma unroll
        for (int s = 0; s < kSteps; ++s) sh[s] = load4_always(ps, 16 * s + 4 * q, D, t.row_ok);
#pragma unroll
        for (int s = 0; s < kSteps; ++s) row_step(sh[s], t.eh[s]);
    } else {
        const bool vecD = (D & 3) == 0;
        for (int s = 0; s < (D + 15) >> 4; ++s)
            row_step(load4(ps, 16 * s + 4 * q, D, t.row_ok, vecD), load4(t.pe, 16 * s + 4 * q, D, t.row_ok, vecD));
    }
    float part[3] = {ee, uu, eu};
#pragma unroll
    for (int i = 0; i < 3; ++i) {   // lanes l15, l15 + 16, l15 + 32, l15 + 48: (q0 + q1) + (q2 + q3) in every lane
        auto a = GE2E_SWAP16(__float_as_uint(part[i]));
        const float h = __uint_as_float(a[0]) + __uint_as_float(a[1]);
        auto b = GE2E_SWAP32(__float_as_uint(h));
        part[i] = __uint_as_float(b[0]) + __uint_as_float(b[1]);
    }
    unit_stats(part[0], eps_cos, t.rne, t.ke);
    unit_stats(part[1], eps_cos, t.rnu, t.ku);
    t.cosd = part[2] * t.rne * t.rnu;
    return t;
}
// The same builder without the leave-one-out part, for rows that are scored against models they are no part of
// (ge2e_enroll.hip): the lane's row is `row` of E where row_ok, and is not read otherwise.  Only the row's norm is taken,
// on the same fragments and with the same two lane swaps; pp = row, j = -1, and rnu, ku, cosd are 0.
template <int kSteps>
__device__ __forceinline__ TileRows<kSteps> tile_rows_plain(const float* E, int row, bool row_ok, int D, float eps_cos) {
    const int q = (threadIdx.x & 63) >> 4;
    TileRows<kSteps> t;
    t.row_ok = row_ok;
    t.pp = t.row = row_ok ? row : 0;
    t.j = -1;
    t.rnu = t.ku = t.cosd = 0.f;
    t.pe = E + (size_t)t.row * D;
    float ee = 0.f;
    if constexpr (kSteps > 0) {
#pragma unroll
        for (int s = 0; s < kSteps; ++s) t.eh[s] = load4(t.pe, 16 * s + 4 * q, D, row_ok, true);
#pragma unroll
        for (int s = 0; s < kSteps; ++s)
#pragma unroll
            for (int i = 0; i < 4; ++i) ee += t.eh[s][i] * t.eh[s][i];
    } else {
        const bool vecD = (D & 3) == 0;
        for (int s = 0; s < (D + 15) >> 4; ++s) {
            const v4f e = load4(t.pe, 16 * s + 4 * q, D, row_ok, vecD);
#pragma unroll
            for (int i = 0; i < 4; ++i) ee += e[i] * e[i];
        }
    }
    auto a = GE2E_SWAP16(__float_as_uint(ee));   // (q0 + q1) + (q2 + q3) in every lane, as in tile_rows
    const float h = __uint_as_float(a[0]) + __uint_as_float(a[1]);
    auto b = GE2E_SWAP32(__float_as_uint(h));
    unit_stats(__uint_as_float(b[0]) + __uint_as_float(b[1]), eps_cos, t.rne, t.ke);
    return t;
}
// The cos tiles on the matrix core: unit centroids x the wave's rows, K = D, kAcc column tiles of 16 speakers (independent
// accumulators) at a time.  After each group epi(kt0, acc): acc[a][g] is the product of the lane's row with centroid
// (kt0 + a) 16 + 4 q + g, before the row norm; tiles past the last one and centroids past n_act hold what must be dropped.
template <int kSteps, int kAcc, class Epi>
__device__ __forceinline__ void tile_cosines(const TileRows<kSteps>& t, const float* CHb, int n_act, int D, Epi&& epi) {
    constexpr bool kHold = kSteps > 0;
    constexpr int kAhead = kSteps < 4 ? (kSteps > 0 ? kSteps : 1) : 4;
    const int l15 = threadIdx.x & 15, q = (threadIdx.x & 63) >> 4;
    const v4f zero4 = {0.f, 0.f, 0.f, 0.f};
    const int KT = (n_act + 15) >> 4;
    for (int kt0 = 0; kt0 < KT; kt0 += kAcc) {
        v4f acc[kAcc];
        const float* pc[kAcc];
        [[maybe_unused]] bool c_ok[kAcc];
#pragma unroll
        for (int a = 0; a < kAcc; ++a) {
            const int kb = (kt0 + a) * 16 + l15;
            acc[a] = zero4;
            c_ok[a] = kb < n_act;
            pc[a] = CHb + (size_t)(c_ok[a] ? kb : 0) * D;
        }
        if constexpr (kHold) {
            v4f ring[kAhead][kAcc];
#pragma unroll
            for (int s = 0; s < kAhead; ++s)
#pragma unroll
                for (int a = 0; a < kAcc; ++a) ring[s][a] = load4_raw(pc[a], 16 * s + 4 * q, D);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int s = 0; s < kSteps; ++s) {
                v4f c[kAcc];
#pragma unroll
                for (int a = 0; a < kAcc; ++a) c[a] = ring[s % kAhead][a];
                if (s + kAhead < kSteps) {   // (known at compile time: the loop is unrolled)
#pragma unroll
                    for (int a = 0; a < kAcc; ++a) ring[s % kAhead][a] = load4_raw(pc[a], 16 * (s + kAhead) + 4 * q, D);
                }
                // (left alone, the scheduler sinks every load to the step that uses it and the ring is gone)
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int a = 0; a < kAcc; ++a) acc[a] = mfma_f32(c[a][i], t.eh[s][i], acc[a]);
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
            const bool vecD = (D & 3) == 0;
            for (int s = 0; s < (D + 15) >> 4; ++s) {
                const v4f e = load4(t.pe, 16 * s + 4 * q, D, t.row_ok, vecD);
                v4f c[kAcc];
#pragma unroll
                for (int a = 0; a < kAcc; ++a) c[a] = load4(pc[a], 16 * s + 4 * q, D, c_ok[a], vecD);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int a = 0; a < kAcc; ++a) acc[a] = mfma_f32(c[a][i], e[i], acc[a]);
            }
        }
        epi(kt0, acc);
    }
}

// The workgroup of a row kernel built on tile_rows / tile_cosines, whose lane map these describe: four waves, one MFMA tile
// of 16 rows each.  (`using namespace tile_geom` in the kernels' files.)
namespace tile_geom {
constexpr int kThreads = 256, kWaves = kThreads / kWave;
constexpr int kTile = 64, kWaveRows = kTile / kWaves;   // rows (sorted positions) per workgroup / per wave
constexpr int kAcc = 4;                                 // column tiles (accumulators) in flight per wave
}  // namespace tile_geom

// ---- a speaker's sum and its unit form: one wave per speaker --------------------------------------------------------------
// A lane owns 4 (vecD: D % 4 == 0 and 16-byte aligned rows) or 1 element of every stretch of 256 / 64 elements of a row:
// the elements from wave_elem(d0, lane, vecD) on, for d0 = 0, wave_stretch(vecD), ...
__device__ __forceinline__ int wave_stretch(bool vecD) { return vecD ? 4 * kWave : kWave; }
__device__ __forceinline__ int wave_elem(int d0, int lane, bool vecD) { return d0 + (vecD ? 4 * lane : lane); }
// The lane's elements d .. (`ok`: d < D) of the sum of the rows E[order[p]], p = r0 .. r1 - 1 (a speaker's span), from 0 in
// ascending p.  The row indices of up to 64 positions come with ONE coalesced load (index_row) and are handed out with
// v_readlane: no dependent order[p] -> row pair per row.  order: the batch's.  Called by the whole wave.
__device__ __forceinline__ v4f speaker_sum(const float* E, const int* order, IndexSpan sp, int R, int D, int d, bool ok,
                                           bool vecD) {
    const int lane = threadIdx.x & 63, r0 = sp.r0, r1 = sp.r1;
    v4f s = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = r0; c0 < r1; c0 += kWave) {
        const int pp = c0 + lane;
        const int idx = pp < r1 ? index_row(order, pp, R) : 0;
        const int n = min(kWave, r1 - c0);
        for (int i = 0; i < n; ++i) {
            const float* er = E + (size_t)__builtin_amdgcn_readlane(idx, i) * D;
            if (ok) {
                if (vecD) s += *reinterpret_cast<const v4f*>(er + d);
                else s[0] += er[d];
            }
        }
    }
    return s;
}
// sq + the squares of the lane's elements of the centroid c = s / fm.  The roundings are spelled out, because they are part of
// the results and were the optimiser's choice while each kernel carried its own copy (packed multiplies for the four, one fma
// for the single element): the four squares are rounded and added on in turn, nothing fused; the single one is fused.
__device__ __forceinline__ float mean_sq(float sq, const v4f& s, float fm, bool vecD) {
    if (vecD) {
#pragma clang fp contract(off)
#pragma unroll
        for (int t = 0; t < 4; ++t) { const float c = s[t] / fm; sq = sq + c * c; }
    } else {
        const float c = s[0] / fm;
        sq = fmaf(c, c, sq);
    }
    return sq;
}
// U = S / fm * rn over the D elements of a speaker: the unit centroid from the sum, the count and 1 / |c| (unit_stats)
__device__ __forceinline__ void unit_scale(const float* S, float* U, int D, float fm, float rn, bool vecD) {
    const int lane = threadIdx.x & 63;
    for (int d0 = 0; d0 < D; d0 += wave_stretch(vecD)) {
        const int d = wave_elem(d0, lane, vecD);
        if (d < D) {
            if (vecD) {
                const v4f s = *reinterpret_cast<const v4f*>(S + d);
                v4f c;
#pragma unroll
                for (int t = 0; t < 4; ++t) c[t] = s[t] / fm * rn;
                *reinterpret_cast<v4f*>(U + d) = c;
            } else {
                U[d] = S[d] / fm * rn;
            }
        }
    }
}

// The register-resident forms need 16-byte row loads; D <= 64, <= 128, <= 256 (steps of 16 that only hold zeros still run: at
// most half of them).  f(std::integral_constant<int, kSteps>): the launcher's call of its row kernel's instantiation.
template <class F>
inline void dispatch_tile_steps(int D, F&& f) {
    const int hold = (D & 3) ? 0 : D <= 64 ? 4 : D <= 128 ? 8 : D <= 256 ? 16 : 0;
    if (hold == 4) f(std::integral_constant<int, 4>{});
    else if (hold == 8) f(std::integral_constant<int, 8>{});
    else if (hold == 16) f(std::integral_constant<int, 16>{});
    else f(std::integral_constant<int, 0>{});
}

}  // namespace ge2e
