// GE2E_IMPL_TILED: shapes whose centroids do not fit one workgroup's LDS (N > 64 or D > 256:
// BASELINE configs 4 and 5).  Many workgroups per batch, five or six kernels on one stream, the
// three contractions on one split-fp16 MFMA tile core (ge2e_tile_gemm.hpp) over operand images that are split
// ONCE into fp16 hi / lo planes in the workspace:
//
//   k_prep    per speaker : sums, c-hat -> CH images + fp32 copy; per row: 1/|e|, e-hat -> EH images
//   k_sim     X = EH . CH^T                    tiles (rows x centroids), K = D                    (s3:64-70)
//   k_rows    per row     : leave-one-out cosine from X's own column, S, loss, dL/dS -> GH images (the own-speaker
//                           column carries the coefficient of s_j), row coefficients of the gradient  (s3:27, 115-127)
//   k_simrows = k_sim + k_rows in one kernel where a 256-slot tile holds a whole similarity row (128 < N <= 256): X never
//               goes to memory
//   k_gc      gC = GH^T . EH                   tiles (centroids x d), K = all N*M rows (cut into pieces where that fills
//                                              the chip; k_spk adds the partial sums)
//   k_spk     per speaker : gC through the centroid norm + a multiple of c-hat_j -> KJ rows (the leave-one-out speaker row
//                           sum_i c3_i e-hat_i is already in gC_j through GH's own column: no second pass over the rows);
//                           the batch's loss / dw / db sums
//   k_ge      gE = GH . CH, epilogue dE = ra gE + c1e e + KJ_j
//   k_reduce  loss / dw / db of forward-only calls
//
// Tile core (ge2e_tile_gemm.hpp; this file holds the kernels, the plan and the launcher): 128 x 128 x 64 on four waves (one
// LDS stage + register prefetch, two workgroups per CU), 256 x 256 x 32 on eight waves with two LDS stages -- register-staged
// (gemm_tile) or, when K is a multiple of 32, fed by buffer_load ... lds with one workgroup per CU walking its tiles
// (gemm_tile_dma / walk_tiles, GemmCfgDma).
//
// Shapes: D % 8 == 0 (rows of the fp16 planes 16-byte aligned; ragged K-steps and tiles are the cores' business), D <= 1024, N <= 1024 (row values of k_rows live in registers), any M >= 2.
// Same algebra and same split arithmetic as ge2e_fused_split.hip.  Config 5 is bound by the contractions, config
// 4 by the bytes the pipeline moves.
#include "ge2e_common.hpp"
#include "ge2e_dev.hpp"
#include "ge2e_row.hpp"
#include "ge2e_split_gemm.hpp"
#include "ge2e_tile_gemm.hpp"
#include "ge2e_tiled.hpp"

namespace ge2e {

// ---------------------------------------------------------------------------------------------
// k_prep: one wave per speaker.  D <= 1024: four float4 per lane cover a row.
// RM > 0: the speaker's rows (M <= RM, D <= 256 NP) stay in registers between the speaker sum and the row pass -- E is
// read from memory ONCE (the generic form reads every row twice, and with a few hundred KB of rows in flight per CU the
// second read misses the L2: FETCH_SIZE of this kernel was twice the size of E).
template <int RM, int NP>
__global__ __launch_bounds__(256) void ge2e_tiled_prep(Problem p, TiledWs L) {
    const int lane = threadIdx.x & 63;
    const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);   // global wave = (batch, speaker)
    const int N = p.N, M = p.M, D = p.D;
    if (gw >= p.B * N) return;
    const int bi = gw / N, j = gw - bi * N;
    const float* E = p.E + ((size_t)bi * N + j) * M * D;
    const size_t NMp = (size_t)N * M;
    _Float16* CHh = reinterpret_cast<_Float16*>(p.ws + L.ch) + (size_t)bi * 2 * N * D;
    _Float16* CHl = CHh + (size_t)N * D;
    _Float16* EHh = reinterpret_cast<_Float16*>(p.ws + L.eh) + (size_t)bi * 2 * NMp * D;
    _Float16* EHl = EHh + NMp * D;
    float* CHf = p.ws + L.chf + (size_t)bi * N * D;
    float* CST = p.ws + L.cst + ((size_t)bi * N + j) * 4;
    float* RST = p.ws + L.rst + ((size_t)bi * N + j) * M * 4;
    const float fM = (float)M;
    constexpr int NPC = RM > 0 ? NP : 4;                  // float4 chunks of a row per lane
    const int npass = RM > 0 ? NP : (D + 255) >> 8;

    float4 s[NPC];
    float4 rows[RM > 0 ? RM : 1][NPC];
#pragma unroll
    for (int c = 0; c < NPC; ++c) s[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (RM > 0) {
#pragma unroll
        for (int i = 0; i < (RM > 0 ? RM : 1); ++i)
#pragma unroll
            for (int c = 0; c < NPC; ++c) {
                const int d = 256 * c + 4 * lane;
                rows[i][c] = (i < M && d < D) ? *reinterpret_cast<const float4*>(E + (size_t)i * D + d) : make_float4(0.f, 0.f, 0.f, 0.f);
                s[c].x += rows[i][c].x; s[c].y += rows[i][c].y; s[c].z += rows[i][c].z; s[c].w += rows[i][c].w;
            }
    } else {
        for (int i = 0; i < M; ++i)
#pragma unroll
            for (int c = 0; c < NPC; ++c) {
                const int d = 256 * c + 4 * lane;
                if (c < npass && d < D) {
                    const float4 v = *reinterpret_cast<const float4*>(E + (size_t)i * D + d);
                    s[c].x += v.x; s[c].y += v.y; s[c].z += v.z; s[c].w += v.w;
                }
            }
    }
    float sq = 0.f, ss = 0.f;   // |c|^2 with c = s / M formed first, like the reference; |s|^2 for the row stats
#pragma unroll
    for (int c = 0; c < NPC; ++c) {
        const float4 cc = make_float4(s[c].x / fM, s[c].y / fM, s[c].z / fM, s[c].w / fM);
        sq += dot4(cc, cc);
        ss += dot4(s[c], s[c]);
    }
    sq = wave_sum(sq);
    ss = wave_sum(ss);
    float rn, kap;
    unit_stats(sq, p.eps_cos, rn, kap);
    float4 chv[NPC];            // c-hat_j, this lane's columns (the rows' own-speaker cosine xo below)
#pragma unroll
    for (int c = 0; c < NPC; ++c) {
        const int d = 256 * c + 4 * lane;
        chv[c] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < npass && d < D) {
            const float4 ch = make_float4(s[c].x / fM * rn, s[c].y / fM * rn, s[c].z / fM * rn, s[c].w / fM * rn);
            chv[c] = ch;
            *reinterpret_cast<float4*>(CHf + (size_t)j * D + d) = ch;
            h4 hi, lo;
            split4(scale4(ch, kSplitScale), hi, lo);
            *reinterpret_cast<h4*>(CHh + (size_t)j * D + d) = hi;
            *reinterpret_cast<h4*>(CHl + (size_t)j * D + d) = lo;
        }
    }
    if (lane == 0) *reinterpret_cast<float4*>(CST) = make_float4(rn, kap, fM / rn, ss);
    // rows: 1/|e| and the e-hat images
    auto row_out = [&](int i, const float4 (&v)[NPC]) {
        float red2[2] = {0.f, 0.f};      // |e|^2 and e . c-hat_j, reduced together
#pragma unroll
        for (int c = 0; c < NPC; ++c) { red2[0] += dot4(v[c], v[c]); red2[1] += dot4(v[c], chv[c]); }
        wave_sum_n<2>(red2);
        const float ee = red2[0];
        float rne, ke;
        unit_stats_fast(ee, p.eps_cos, rne, ke);
        const size_t r = (size_t)j * M + i;
#pragma unroll
        for (int c = 0; c < NPC; ++c) {
            const int d = 256 * c + 4 * lane;
            if (c < npass && d < D) {
                h4 hi, lo;
                split4(scale4(v[c], rne * kSplitScale), hi, lo);
                *reinterpret_cast<h4*>(EHh + r * D + d) = hi;
                *reinterpret_cast<h4*>(EHl + r * D + d) = lo;
            }
        }
        // rne, kappa_e, |e|^2 and xo = e-hat . c-hat_j in exact fp32 (the fused similarity + row kernel takes the own-speaker
        // cosine from here: in its tile the column sits in ONE lane of another wave)
        if (lane == 0) *reinterpret_cast<float4*>(RST + (size_t)i * 4) = make_float4(rne, ke, ee, red2[1] * rne);
    };
    if (RM > 0) {
#pragma unroll
        for (int i = 0; i < (RM > 0 ? RM : 1); ++i)
            if (i < M) row_out(i, rows[i]);
    } else {
        for (int i = 0; i < M; ++i) {
            float4 v[NPC];
#pragma unroll
            for (int c = 0; c < NPC; ++c) {
                const int d = 256 * c + 4 * lane;
                v[c] = (c < npass && d < D) ? *reinterpret_cast<const float4*>(E + (size_t)i * D + d)
                                            : make_float4(0.f, 0.f, 0.f, 0.f);
            }
            row_out(i, v);
        }
    }
}
// the instantiation for a shape: rows in registers when M <= 10 and D <= 768 (40 / 80 / 120 row registers per lane)
static PrepPlan plan_prep(int M, int D) {
    if (M <= 10 && D <= 256) return {10, 1};
    if (M <= 10 && D <= 512) return {10, 2};
    if (M <= 10 && D <= 768) return {10, 3};
    return {0, 4};
}
static void launch_prep(const Problem& p, const TiledWs& L, const PrepPlan& plan, hipStream_t stream) {
    const dim3 grid((unsigned)((p.B * p.N + 3) / 4)), block(256);
    switch (plan.np) {
        case 1: hipLaunchKernelGGL((ge2e_tiled_prep<10, 1>), grid, block, 0, stream, p, L); break;
        case 2: hipLaunchKernelGGL((ge2e_tiled_prep<10, 2>), grid, block, 0, stream, p, L); break;
        case 3: hipLaunchKernelGGL((ge2e_tiled_prep<10, 3>), grid, block, 0, stream, p, L); break;
        default: hipLaunchKernelGGL((ge2e_tiled_prep<0, 4>), grid, block, 0, stream, p, L); break;
    }
}

// ---------------------------------------------------------------------------------------------
// k_sim: X[r][k] = sum_d EH[r][d] CH[k][d].  One workgroup per TM x TN tile (both operands K-contiguous).
template <class C>
__global__ __launch_bounds__(C::NT, 2) void ge2e_tiled_sim(Problem p, TiledWs L) {
    extern __shared__ __attribute__((aligned(16))) _Float16 gsm[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int N = p.N, D = p.D, NM = p.N * p.M;
    const int rt = (NM + C::TM - 1) / C::TM, ct = (N + C::TN - 1) / C::TN;
    const size_t NMp = (size_t)NM;
    struct Ix { int kt, rtile, bi; };
    auto decode = [&](int t, Opnd& A, Opnd& Bo, Ix& ix, int& ktotal) {
        ix.kt = t % ct; t /= ct;
        ix.rtile = t % rt;
        ix.bi = t / rt;
        A.hi = reinterpret_cast<const _Float16*>(p.ws + L.eh) + (size_t)ix.bi * 2 * NMp * D + (size_t)ix.rtile * C::TM * D;
        A.lo = A.hi + NMp * D;
        A.ld = D; A.valid = min(C::TM, NM - ix.rtile * C::TM);
        Bo.hi = reinterpret_cast<const _Float16*>(p.ws + L.ch) + (size_t)ix.bi * 2 * N * D + (size_t)ix.kt * C::TN * D;
        Bo.lo = Bo.hi + (size_t)N * D;
        Bo.ld = D; Bo.valid = min(C::TN, N - ix.kt * C::TN);
        ktotal = D;
    };
    auto epilogue = [&](const Ix& ix, f32x16 (&acc)[C::A2][C::B2]) {
        store_tile<C>(acc, lane, wid, p.ws + L.x + (size_t)ix.bi * NMp * L.npad, L.npad, ix.rtile * C::TM, ix.kt * C::TN, NM, L.npad);
    };
    walk_tiles<C, true, true, Ix>(p, 0, p.B * rt * ct, gsm, tid, decode, epilogue);
}

// What a row pass leaves of global row gr for the kernels behind it, from ad = w dL/dS on the own column and coef =
// w sum_k dL/dS_k c0_k: L.rs[gr] = (ra, c1e, 0, 0 | the row's share c4' of the c-hat_j coefficient of KJ_j, loss, dw, db),
// and the row's loss.  sj, kap: the speaker's |s_j| scale and kappa_j; xo: the own column of the similarity.
__device__ __forceinline__ void write_row_scalars(const Problem& p, const TiledWs& L, size_t gr, float w, float ad, float coef,
                                                  float rne, float ke, const OwnCos& oc, float inv_m1, float sj, float kap,
                                                  float xo, float per, float dwv, float dbv) {
    const RowCoeffs rc = row_coeffs(ad, coef, rne, ke, oc.rnu, oc.ku, oc.cosd, inv_m1);
    float* rs = p.ws + L.rs + gr * 8;
    *reinterpret_cast<float4*>(rs) = make_float4(rne * (w * kSplitInv2), rc.c1 * rne, 0.f, 0.f);
    *reinterpret_cast<float4*>(rs + 4) = make_float4(row_c4_share(rc, inv_m1, sj, kap, xo), per, dwv, dbv);
    if (p.per) p.per[gr] = per;
}

// ---------------------------------------------------------------------------------------------
// k_simrows (N <= 256, i.e. one 256-slot tile holds a row's whole similarity vector): k_sim and k_rows<16> in ONE kernel --
// the fp32 similarity block never goes to memory (2 x N M npad 4 bytes per batch less: 1.3 GB per launch at config 4,
// where every kernel of this pipeline runs at the HBM rate) and one launch fewer.
// The contraction is taken with the SLOTS as the A operand (C layout: register = slot, lane = row), so a row's 256
// similarities are 64 registers of TWO lanes (l, l + 32) of TWO waves (wa = 0, 1): the row reductions are in-lane loops,
// one half swap and one exchange through LDS.  The dL/dS tile then goes through LDS (the GEMM's stages are free by
// then) so that the GH planes are written as whole rows.
// CONTRAST / FULL (N == 256: every slot of the tile exists) are compile-time: the three passes over the 128 accumulators of a
// lane are the kernel's vector work, and every per-element test in them is two instructions.
template <class C, bool CONTRAST, bool FULL>
__global__ __launch_bounds__(C::NT, 2) void ge2e_tiled_simrows(Problem p, TiledWs L) {
    static_assert(C::TM == 256 && C::TN == 256, "one 256 x 256 tile per workgroup");
    extern __shared__ __attribute__((aligned(16))) _Float16 gsm[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int N = p.N, M = p.M, D = p.D, NM = N * M, npad = L.npad;
    const int rt = (NM + C::TN - 1) / C::TN;
    const int t = xcd_major_tile(blockIdx.x, gridDim.x);
    const int rtile = t % rt, bi = t / rt;
    const size_t NMp = (size_t)NM;
    Opnd A, Bo;
    A.hi = reinterpret_cast<const _Float16*>(p.ws + L.ch) + (size_t)bi * 2 * N * D;
    A.lo = A.hi + (size_t)N * D;
    A.ld = D; A.valid = min(C::TM, N);
    Bo.hi = reinterpret_cast<const _Float16*>(p.ws + L.eh) + (size_t)bi * 2 * NMp * D + (size_t)rtile * C::TN * D;
    Bo.lo = Bo.hi + NMp * D;
    Bo.ld = D; Bo.valid = min(C::TN, NM - rtile * C::TN);
    f32x16 acc[C::A2][C::B2];
    gemm_zero<C>(acc);
    gemm_tile<C, true, true>(A, Bo, D, gsm, tid, acc);      // ends with a barrier: the stages are free

    // acc[a2][b2][v] = 2^16 X[slot][row], slot = 128 wa + 32 a2 + 8 (v >> 2) + 4 h + (v & 3), row = 64 wb + 32 b2 + l31
    const int l31 = lane & 31, h = lane >> 5, wa = wid / C::WN, wb = wid % C::WN;
    float* const XCH = reinterpret_cast<float*>(gsm);                 // [2 (wa)][256 rows][2] exchange of row partials
    _Float16* const TT = gsm + 4096;                                   // [256 rows][TTP] halfs: one G plane at a time
    constexpr int TTP = 256 + 4;
    const float w = p.w ? *p.w : p.w_imm, bias = p.b ? *p.b : p.b_imm;
    const float eps = p.eps, log_eps = p.log_eps;
    const float inv_m1 = 1.0f / (float)(M - 1);
    const int soff = 128 * wa + 4 * h;                                 // slot of (a2 = 0, v = 0)

    float rne[2], ke[2], cosd[2], sjj[2], rnu[2], ku[2], xo[2], csx[2], csy[2], csz[2];
    int jl[2];          // own-speaker slot relative to soff (matches 32 a2 + 8 (v >> 2) + (v & 3) of at most one register)
    bool rv[2];
#pragma unroll
    for (int b2 = 0; b2 < C::B2; ++b2) {
        const int rloc = 64 * wb + 32 * b2 + l31;
        const int r = rtile * C::TN + rloc;
        rv[b2] = r < NM;
        const int rc = rv[b2] ? r : NM - 1;
        const int j = rc / M;
        const float4 rst = *reinterpret_cast<const float4*>(p.ws + L.rst + ((size_t)bi * NM + rc) * 4);   // rne ke ee xo
        const float4 cs = *reinterpret_cast<const float4*>(p.ws + L.cst + ((size_t)bi * N + j) * 4);       // rn kap |s| |s|^2
        rne[b2] = rst.x; ke[b2] = rst.y; xo[b2] = rst.w;
        csx[b2] = cs.x; csy[b2] = cs.y; csz[b2] = cs.z;
        const OwnCos oc = own_column_cos(rst, cs, rst.w, inv_m1, p.eps_cos);
        cosd[b2] = oc.cosd; rnu[b2] = oc.rnu; ku[b2] = oc.ku;
        sjj[b2] = w * (cosd[b2] + eps) + bias;
        jl[b2] = j - soff;
    }
    const int nl = N - soff;        // slots of this lane with (32 a2 + 8 (v >> 2) + (v & 3)) < nl exist
    const float ws = w * kSplitInv2, bs = w * eps + bias;       // S = ws acc + bs

    // ---- row maximum over the other speakers' columns (the own column enters with its leave-one-out value) ----------
    // (jl and nl are re-read through an opaque copy in every phase: compared once, hipcc keeps all 128 (exists, own-column)
    // lane masks of the three loops below in SGPRs -- 250 spilled scalars)
#define GE2E_SR_OPAQUE() int jq[2] = {jl[0], jl[1]}, nq = nl; asm volatile("" : "+v"(jq[0]), "+v"(jq[1]), "+v"(nq))
    float best[2]; int besti[2];
    float mx[2];
    {
    GE2E_SR_OPAQUE();
#pragma unroll
    for (int b2 = 0; b2 < C::B2; ++b2) {
        float m = -INFINITY;
        best[b2] = -INFINITY; besti[b2] = 0x7fffffff;
        if (!CONTRAST) {       // (the two variants as separate straight-line loops: no per-element control flow)
#pragma unroll
            for (int a2 = 0; a2 < C::A2; ++a2)
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int c = 32 * a2 + 8 * (v >> 2) + (v & 3);
                    const float sv = fmaf(ws, acc[a2][b2][v], bs);
                    m = ((FULL || c < nq) && c != jq[b2]) ? fmaxf(m, sv) : m;
                }
        } else {
            float bv = -INFINITY; int bi_ = 0x7fffffff;
#pragma unroll
            for (int a2 = 0; a2 < C::A2; ++a2)
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int c = 32 * a2 + 8 * (v >> 2) + (v & 3);     // ascending slot order: ties keep the lower slot
                    const float sv = fmaf(ws, acc[a2][b2][v], bs);
                    const bool better = (FULL || c < nq) && c != jq[b2] && sv > bv;
                    bv = better ? sv : bv;
                    bi_ = better ? soff + c : bi_;
                }
            best[b2] = bv; besti[b2] = bi_;
        }
        {   // the two half-rows of the wave
            auto sw = GE2E_SWAP32(__float_as_uint(m));
            m = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
        }
        mx[b2] = m;
    }
    }
    if (CONTRAST) {
#pragma unroll
        for (int b2 = 0; b2 < C::B2; ++b2) {
            auto a = GE2E_SWAP32(__float_as_uint(best[b2]));
            auto b = GE2E_SWAP32((unsigned)besti[b2]);
            float v0 = __uint_as_float(a[0]); int i0 = (int)b[0];
            argmax_merge(v0, i0, __uint_as_float(a[1]), (int)b[1]);
            best[b2] = v0; besti[b2] = i0;
        }
    }
    if (h == 0) {
#pragma unroll
        for (int b2 = 0; b2 < C::B2; ++b2) {
            const int rloc = 64 * wb + 32 * b2 + l31;
            XCH[(wa * 256 + rloc) * 2] = CONTRAST ? best[b2] : mx[b2];
            XCH[(wa * 256 + rloc) * 2 + 1] = __int_as_float(besti[b2]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int b2 = 0; b2 < C::B2; ++b2) {
        const int rloc = 64 * wb + 32 * b2 + l31;
        const float om = XCH[((wa ^ 1) * 256 + rloc) * 2];
        if (CONTRAST) {
            const int oi = __float_as_int(XCH[((wa ^ 1) * 256 + rloc) * 2 + 1]);
            argmax_merge(best[b2], besti[b2], om, oi);
        } else {
            mx[b2] = fmaxf(fmaxf(fmaxf(mx[b2], om), sjj[b2]), log_eps);
        }
    }
    __syncthreads();

    // ---- exponentials, row sums -> dL/dS in place of the similarities ----------------------------------------------
    float zl[2], al[2];
    {
    GE2E_SR_OPAQUE();
#pragma unroll
    for (int b2 = 0; b2 < C::B2; ++b2) {
        float z = 0.f, a = 0.f;
        if (!CONTRAST) {
            const float tb2 = (bs - mx[b2]) * 1.44269504088896341f, ws2 = ws * 1.44269504088896341f;   // base 2: one instruction per exponential
#pragma unroll
            for (int a2 = 0; a2 < C::A2; ++a2)
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int c = 32 * a2 + 8 * (v >> 2) + (v & 3);
                    const float x = acc[a2][b2][v];
                    float g = __builtin_amdgcn_exp2f(fmaf(ws2, x, tb2));
                    g = ((FULL || c < nq) && c != jq[b2]) ? g : 0.f;
                    z += g;
                    a = fmaf(g, x, a);
                    acc[a2][b2][v] = g;
                }
        } else {
#pragma unroll
            for (int a2 = 0; a2 < C::A2; ++a2)
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int c = 32 * a2 + 8 * (v >> 2) + (v & 3);
                    const bool hit = soff + c == besti[b2] && (FULL || c < nq) && c != jq[b2];
                    a = hit ? acc[a2][b2][v] : a;          // the raw similarity of the best other speaker
                    acc[a2][b2][v] = hit ? 1.0f : 0.f;
                }
        }
        {
            auto s0 = GE2E_SWAP32(__float_as_uint(z));
            z = __uint_as_float(s0[0]) + __uint_as_float(s0[1]);
            auto s1 = GE2E_SWAP32(__float_as_uint(a));
            a = __uint_as_float(s1[0]) + __uint_as_float(s1[1]);
        }
        zl[b2] = z; al[b2] = a;
    }
    }
    if (h == 0) {
#pragma unroll
        for (int b2 = 0; b2 < C::B2; ++b2) {
            const int rloc = 64 * wb + 32 * b2 + l31;
            XCH[(wa * 256 + rloc) * 2] = zl[b2];
            XCH[(wa * 256 + rloc) * 2 + 1] = al[b2];
        }
    }
    __syncthreads();
    float gs[2], og[2];     // scale of the other columns' values, value of the own column (both x 2^8)
#pragma unroll
    for (int b2 = 0; b2 < C::B2; ++b2) {
        const int rloc = 64 * wb + 32 * b2 + l31;
        // fixed order (wa = 0 first): both waves of a row form the same sums
        const float z0 = wa == 0 ? zl[b2] : XCH[rloc * 2], z1 = wa == 1 ? zl[b2] : XCH[(256 + rloc) * 2];
        const float a0 = wa == 0 ? al[b2] : XCH[rloc * 2 + 1], a1 = wa == 1 ? al[b2] : XCH[(256 + rloc) * 2 + 1];
        const float zp = z0 + z1, ap = (a0 + a1) * kSplitInv2;
        float per, ad0, coefsum, db_row, gsc;
        if (!CONTRAST) {
            const float zoff = zp + __expf(log_eps - mx[b2]);
            const float z = zoff + __expf(sjj[b2] - mx[b2]);
            per = (mx[b2] - sjj[b2]) + __logf(z);
            const float rz = 1.0f / z;
            ad0 = -zoff * rz;                         // dL/dS on the own-speaker column: -(1 - p_jj) = -z_off / z
            coefsum = fmaf(ap, rz, ad0 * cosd[b2]);   // sum_k dL/dS_k c0_k
            db_row = fmaf(zp, rz, ad0);
            gsc = rz;
        } else {
            const float pos = 1.0f / (1.0f + __expf(-sjj[b2]));
            const float neg = (N > 1) ? 1.0f / (1.0f + __expf(-best[b2])) : 0.0f;
            per = 1.0f - pos + neg;
            ad0 = -pos * (1.0f - pos);
            const float gn = neg * (1.0f - neg);
            coefsum = fmaf(gn, ap, ad0 * cosd[b2]);   // (a0 + a1) is the raw similarity of the best other speaker
            db_row = gn + ad0;
            gsc = gn;
        }
        if (!rv[b2]) { ad0 = 0.f; gsc = 0.f; }
        // the own-speaker column carries o = c2 |s_j| / (ra w)  (k_rows below)
        og[b2] = row_own_o(rne[b2], rnu[b2], ku[b2], cosd[b2], inv_m1, csz[b2]) * ad0 * kSplitScale;
        gs[b2] = gsc * kSplitScale;
        if (wa == 0 && h == 0 && rv[b2])
            write_row_scalars(p, L, (size_t)bi * NM + rtile * C::TN + rloc, w, w * ad0, w * coefsum, rne[b2], ke[b2],
                              OwnCos{cosd[b2], rnu[b2], ku[b2]}, inv_m1, csz[b2], csy[b2], xo[b2], per,
                              fmaf(eps, db_row, coefsum), db_row);
    }
    if (!p.dE) return;      // forward-only calls: nobody reads the dL/dS planes (a third of this kernel's time and 2.7 MB per tile)
    __syncthreads();        // XCH has been read: the region below it is about to hold the G tile

    // ---- dL/dS -> split fp16 -> LDS tile [row][slot] -> the GH planes as whole rows, one plane at a time ------------
    _Float16* const GHh = reinterpret_cast<_Float16*>(p.ws + L.gh) + (size_t)bi * 2 * NMp * npad + (size_t)rtile * C::TN * npad;
    const int rows_here = min(C::TN, NM - rtile * C::TN);
    // The tile is formed ONCE: the hi halves go to the LDS tile, the lo halves are parked in the accumulator registers they
    // came from (two registers per four values) until the hi plane has left.  (Round 4's first form ran the select, the scale
    // and the whole split once per plane: ~1 000 of the kernel's 4 100 vector instructions per wave.)
    auto write_plane = [&](int plane) {
        __syncthreads();
        _Float16* const G = GHh + (size_t)plane * NMp * npad;
        for (int idx = tid; idx < 256 * 32; idx += C::NT) {          // 32 16-byte pieces per row
            const int row = idx >> 5, c8 = (idx & 31) * 8;
            if (row < rows_here && c8 < npad) {
                const uint2 lo8 = *reinterpret_cast<const uint2*>(TT + row * TTP + c8);
                const uint2 hi8 = *reinterpret_cast<const uint2*>(TT + row * TTP + c8 + 4);
                *reinterpret_cast<uint4*>(G + (size_t)row * npad + c8) = make_uint4(lo8.x, lo8.y, hi8.x, hi8.y);
            }
        }
        __syncthreads();
    };
    {
        GE2E_SR_OPAQUE();
        (void)nq;
#pragma unroll
        for (int b2 = 0; b2 < C::B2; ++b2) {
            const int rloc = 64 * wb + 32 * b2 + l31;
#pragma unroll
            for (int a2 = 0; a2 < C::A2; ++a2)
#pragma unroll
                for (int vg = 0; vg < 4; ++vg) {
                    float gv[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int c = 32 * a2 + 8 * vg + e;
                        gv[e] = c == jq[b2] ? og[b2] : acc[a2][b2][4 * vg + e] * gs[b2];
                    }
                    h4 hi, lo;
                    split4(make_float4(gv[0], gv[1], gv[2], gv[3]), hi, lo);
                    *reinterpret_cast<h4*>(TT + rloc * TTP + soff + 32 * a2 + 8 * vg) = hi;
                    const uint2 lb = __builtin_bit_cast(uint2, lo);
                    acc[a2][b2][4 * vg] = __uint_as_float(lb.x);
                    acc[a2][b2][4 * vg + 1] = __uint_as_float(lb.y);
                }
        }
    }
    write_plane(0);
#pragma unroll
    for (int b2 = 0; b2 < C::B2; ++b2) {
        const int rloc = 64 * wb + 32 * b2 + l31;
#pragma unroll
        for (int a2 = 0; a2 < C::A2; ++a2)
#pragma unroll
            for (int vg = 0; vg < 4; ++vg)
                *reinterpret_cast<uint2*>(TT + rloc * TTP + soff + 32 * a2 + 8 * vg) =
                    make_uint2(__float_as_uint(acc[a2][b2][4 * vg]), __float_as_uint(acc[a2][b2][4 * vg + 1]));
    }
    write_plane(1);
#undef GE2E_SR_OPAQUE
}

// ---------------------------------------------------------------------------------------------
// k_rows: W lanes per row, 256 / W rows per workgroup; the row of X lives in 16 registers per lane: lane l of a row holds
// the 4 consecutive centroid slots 4 W c + 4 l .. + 3 of up to four chunks c (16-byte reads of X and 8-byte writes of the
// two G planes; 2-byte stores cost ~12x per byte).
//   W = 64  one wave per row, up to 1024 centroids
//   W = 16  N <= 256: four rows per wave (a wave per row is latency-bound: one short dependent chain per wave and 655 k
//           waves per launch at cfg4)
// Rows past the end: a whole wave of them leaves (W = 64); inside a wave dead rows recompute the last row and store nothing.
template <int W>
__global__ __launch_bounds__(256) void ge2e_tiled_rows(Problem p, TiledWs L) {
    const int l = threadIdx.x & (W - 1);
    const size_t gr_ = (size_t)blockIdx.x * (256 / W) + threadIdx.x / W;  // global row
    const int N = p.N, M = p.M, NM = N * M, npad = L.npad;
    const size_t rows_total = (size_t)p.B * NM;
    const bool live = gr_ < rows_total;
    if constexpr (W == 64) {
        if (!live) return;
    }
    const size_t gr = live ? gr_ : rows_total - 1;
    const int bi = (int)(gr / NM), r = (int)(gr - (size_t)bi * NM), j = r / M;
    const float w = p.w ? *p.w : p.w_imm, bias = p.b ? *p.b : p.b_imm;
    const float eps = p.eps, log_eps = p.log_eps;
    const float inv_m1 = 1.0f / (float)(M - 1);
    const float* X = p.ws + L.x + ((size_t)bi * NM + r) * npad;
    const float4 rst = *reinterpret_cast<const float4*>(p.ws + L.rst + gr * 4);      // rne ke ee
    const float4 cs = *reinterpret_cast<const float4*>(p.ws + L.cst + ((size_t)bi * N + j) * 4);  // rn kap |s| |s|^2
    const float rne = rst.x, ke = rst.y;
    const float xo = X[j];
    const OwnCos oc = own_column_cos(rst, cs, xo, inv_m1, p.eps_cos);
    const float cosd = oc.cosd;
    const float sjj = w * (cosd + eps) + bias;
    float c0[4][4], g[4][4];
    float mx = -INFINITY, best = -INFINITY;
    int besti = 0x7fffffff;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int kb = 4 * W * c + 4 * l;
        float4 xv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (kb < npad) xv = *reinterpret_cast<const float4*>(X + kb);
        const float xe[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int k = kb + e;
            c0[c][e] = (k == j) ? cosd : xe[e];
            if (k < N) {
                const float sv = w * (c0[c][e] + eps) + bias;
                mx = fmaxf(mx, sv);
                if (k != j && sv > best) { best = sv; besti = k; }
            }
        }
    }
    float per;
    if (p.variant == 0) {
        mx = fmaxf(group_max<W>(mx), log_eps);
        float zoff = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = 4 * W * c + 4 * l + e;
                g[c][e] = (k < N) ? __expf(w * (c0[c][e] + eps) + bias - mx) : 0.f;
                if (k != j) zoff += g[c][e];
            }
        zoff = group_sum<W>(zoff) + __expf(log_eps - mx);
        const float z = zoff + __expf(sjj - mx);
        per = (mx - sjj) + __logf(z);
        const float rz = 1.0f / z;
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) g[c][e] = (4 * W * c + 4 * l + e == j) ? -zoff * rz : g[c][e] * rz;
    } else {
        group_argmax<W>(best, besti);
        const float pos = 1.0f / (1.0f + __expf(-sjj));
        const float neg = (N > 1) ? 1.0f / (1.0f + __expf(-best)) : 0.0f;
        per = 1.0f - pos + neg;
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = 4 * W * c + 4 * l + e;
                g[c][e] = (k == j) ? -pos * (1.0f - pos) : ((k == besti) ? neg * (1.0f - neg) : 0.f);
            }
    }
    float dwv = 0.f, dbv = 0.f, coef = 0.f, ad = 0.f;
    const float own_o = row_own_o(rne, oc.rnu, oc.ku, cosd, inv_m1, cs.z);
    _Float16* GHh = reinterpret_cast<_Float16*>(p.ws + L.gh) + (size_t)bi * 2 * NM * npad + (size_t)r * npad;
    _Float16* GHl = GHh + (size_t)NM * npad;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int kb = 4 * W * c + 4 * l;
        if (kb < npad) {
            float gv[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = kb + e;
                gv[e] = (k < N) ? g[c][e] : 0.f;
                dwv += gv[e] * (c0[c][e] + eps);
                dbv += gv[e];
                coef += gv[e] * c0[c][e];
                // the own-speaker column carries o = c2 |s_j| / (ra w): k_ge's contraction then adds the c2 s_j term of dE
                // by itself, and what o adds to gC_j is, pushed through the centroid norm in k_spk, exactly the
                // leave-one-out speaker row sum_i c3_i e-hat_i minus kap_j (sum_i c3_i xo_i) c-hat_j (ge2e_team.hip, S)
                if (k == j) { ad = gv[e]; gv[e] = own_o * gv[e]; }
            }
            if (live && p.dE) {      // (forward-only calls: nobody reads the dL/dS planes)
                h4 hi, lo;
                split4(make_float4(gv[0] * kSplitScale, gv[1] * kSplitScale, gv[2] * kSplitScale, gv[3] * kSplitScale), hi, lo);
                *reinterpret_cast<h4*>(GHh + kb) = hi;
                *reinterpret_cast<h4*>(GHl + kb) = lo;
            }
        }
    }
    dwv = group_sum<W>(dwv); dbv = group_sum<W>(dbv);
    coef = w * group_sum<W>(coef); ad = w * group_sum<W>(ad);
    if (l == 0 && live) write_row_scalars(p, L, gr, w, ad, coef, rne, ke, oc, inv_m1, cs.z, cs.y, xo, per, dwv, dbv);
}

// ---------------------------------------------------------------------------------------------
// k_gc: gC[k][d] = sum_r GH[r][k] EH[r][d].  One workgroup per (TM centroids x TN d) tile over all rows of the batch
// (both operands with K along their rows -> transposing reads).
template <class C>
__global__ __launch_bounds__(C::NT, 2) void ge2e_tiled_gc(Problem p, TiledWs L) {
    extern __shared__ __attribute__((aligned(16))) _Float16 gsm[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int N = p.N, D = p.D, NM = p.N * p.M, npad = L.npad;
    const int dtiles = (D + C::TN - 1) / C::TN, ct = (N + C::TM - 1) / C::TM;
    const int S = L.gc_split, steps = NM / 32;
    struct Ix { int dt, kt, sp, bi; };
    auto decode = [&](int t, Opnd& A, Opnd& Bo, Ix& ix, int& ktotal) {
        ix.dt = t % dtiles; t /= dtiles;
        ix.kt = t % ct; t /= ct;
        ix.sp = t % S;
        ix.bi = t / S;
        // rows [r0, r1) of the batch: piece sp of S (whole 32-row K-steps when S > 1 -- the launcher splits only then)
        const int r0 = S > 1 ? (int)((long long)steps * ix.sp / S) * 32 : 0;
        const int r1 = S > 1 ? (int)((long long)steps * (ix.sp + 1) / S) * 32 : NM;
        A.hi = reinterpret_cast<const _Float16*>(p.ws + L.gh) + (size_t)ix.bi * 2 * NM * npad + (size_t)r0 * npad + ix.kt * C::TM;
        A.lo = A.hi + (size_t)NM * npad;
        A.ld = npad; A.valid = min(C::TM, npad - ix.kt * C::TM);
        Bo.hi = reinterpret_cast<const _Float16*>(p.ws + L.eh) + (size_t)ix.bi * 2 * NM * D + (size_t)r0 * D + ix.dt * C::TN;
        Bo.lo = Bo.hi + (size_t)NM * D;
        Bo.ld = D; Bo.valid = min(C::TN, D - ix.dt * C::TN);
        ktotal = r1 - r0;
    };
    auto epilogue = [&](const Ix& ix, f32x16 (&acc)[C::A2][C::B2]) {
        float* GC = S > 1 ? p.ws + L.x + ((size_t)ix.bi * S + ix.sp) * N * D : p.ws + L.gc + (size_t)ix.bi * N * D;
        store_tile<C>(acc, lane, wid, GC, D, ix.kt * C::TM, ix.dt * C::TN, N, D);
    };
    walk_tiles<C, false, false, Ix>(p, 8, p.B * S * ct * dtiles, gsm, tid, decode, epilogue);
}

// ---------------------------------------------------------------------------------------------
// k_spk: one wave per speaker: dc_j / M (gC through the centroid norm) + the leave-one-out sums.
__global__ __launch_bounds__(256) void ge2e_tiled_spk(Problem p, TiledWs L) {
    const int lane = threadIdx.x & 63;
    const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int N = p.N, M = p.M, D = p.D, NM = N * M;
    if (gw >= p.B * N) return;
    const int bi = gw / N, j = gw - bi * N;
    const float w = p.w ? *p.w : p.w_imm;
    const float fM = (float)M;
    const int S = L.gc_split;
    const float* GC = S > 1 ? p.ws + L.x + ((size_t)bi * S * N + j) * D : p.ws + L.gc + ((size_t)bi * N + j) * D;
    const float* CHf = p.ws + L.chf + ((size_t)bi * N + j) * D;
    const float4 cs = *reinterpret_cast<const float4*>(p.ws + L.cst + ((size_t)bi * N + j) * 4);
    const float* RS = p.ws + L.rs + ((size_t)bi * NM + (size_t)j * M) * 8;
    float* KJ = p.ws + L.kj + ((size_t)bi * N + j) * D;
    const int npass = (D + 255) >> 8;
    float4 g[4], c[4];
    float coef = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int d = 256 * q + 4 * lane;
        g[q] = c[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q < npass && d < D) {
            float4 gs = *reinterpret_cast<const float4*>(GC + d);
            for (int sp = 1; sp < S; ++sp) {       // k_gc's partial sums, in a fixed order
                const float4 gp = *reinterpret_cast<const float4*>(GC + (size_t)sp * N * D + d);
                gs.x += gp.x; gs.y += gp.y; gs.z += gp.z; gs.w += gp.w;
            }
            g[q] = scale4(gs, w);
            c[q] = *reinterpret_cast<const float4*>(CHf + d);
            coef += dot4(g[q], c[q]);
        }
    }
    coef = wave_sum(coef);
    const float f = cs.y * coef, sc = cs.x / fM;
    // sum_i c4'_i: the whole speaker row KJP_j is a multiple of c-hat_j (the e-hat part rides in gC).  Lane i reads row i's
    // coefficient and the wave adds them (as a loop over i this was M dependent round trips per wave: a run-time M is not unrolled)
    float bsum = 0.f;
    for (int i = lane; i < M; i += kWave) bsum += RS[i * 8 + 4];
    const float bs = wave_sum(bsum);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int d = 256 * q + 4 * lane;
        if (q < npass && d < D) {
            *reinterpret_cast<float4*>(KJ + d) =
                make_float4((g[q].x - f * c[q].x) * sc + bs * c[q].x, (g[q].y - f * c[q].y) * sc + bs * c[q].y,
                            (g[q].z - f * c[q].z) * sc + bs * c[q].z, (g[q].w - f * c[q].w) * sc + bs * c[q].w);
        }
    }
    // the batch's loss / dw / db: fixed-order sums of the per-row values (k_rows wrote them two launches ago), taken by
    // the wave of speaker 0 -- one launch fewer than a reduction kernel of its own (forward-only calls keep k_reduce)
    if (j == 0) {
        const float* RSb = p.ws + L.rs + (size_t)bi * NM * 8;
        float red[3] = {0.f, 0.f, 0.f};
#pragma unroll 8     // (eight loads in flight: this wave has NM / 64 of them in a row while its 4 N - 1 siblings have one round trip)
        for (int r = lane; r < NM; r += kWave) {
            const float4 v = *reinterpret_cast<const float4*>(RSb + (size_t)r * 8 + 4);   // . loss dw db
            red[0] += v.y; red[1] += v.z; red[2] += v.w;
        }
        wave_sum_n<3>(red);
        if (lane == 0) {
            if (p.loss) p.loss[bi] = red[0];
            if (p.dw) p.dw[bi] = red[1];
            if (p.db) p.db[bi] = red[2];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// k_ge: gE[r][d] = sum_k GH[r][k] CH[k][d] per (TM rows x TN d) tile (A K-contiguous, B K-rows), then the epilogue
// dE = ra gE + c1e e + KJ_j (the c2 s_j term rides in GH's own-speaker column).
template <class C>
__global__ __launch_bounds__(C::NT, 2) void ge2e_tiled_ge(Problem p, TiledWs L) {
    extern __shared__ __attribute__((aligned(16))) _Float16 gsm[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int N = p.N, M = p.M, D = p.D, NM = N * M, npad = L.npad;
    const int dtiles = (D + C::TN - 1) / C::TN, rt = (NM + C::TM - 1) / C::TM;
    struct Ix { int dt, rtile, bi; };
    auto decode = [&](int t, Opnd& A, Opnd& Bo, Ix& ix, int& ktotal) {
        ix.dt = t % dtiles; t /= dtiles;
        ix.rtile = t % rt;
        ix.bi = t / rt;
        A.hi = reinterpret_cast<const _Float16*>(p.ws + L.gh) + (size_t)ix.bi * 2 * NM * npad + (size_t)ix.rtile * C::TM * npad;
        A.lo = A.hi + (size_t)NM * npad;
        A.ld = npad; A.valid = min(C::TM, NM - ix.rtile * C::TM);
        Bo.hi = reinterpret_cast<const _Float16*>(p.ws + L.ch) + (size_t)ix.bi * 2 * N * D + ix.dt * C::TN;
        Bo.lo = Bo.hi + (size_t)N * D;
        Bo.ld = D; Bo.valid = min(C::TN, D - ix.dt * C::TN);
        ktotal = N;      // K = the N real centroid slots (pad columns of GH are zero)
    };
    auto epilogue = [&](const Ix& ix, f32x16 (&acc)[C::A2][C::B2]) {
        const int rtile = ix.rtile, dt = ix.dt;
        const float* E = p.E + (size_t)ix.bi * NM * D;
        float* dE = p.dE + (size_t)ix.bi * NM * D;
        const float* KJ = p.ws + L.kj + (size_t)ix.bi * N * D;
        const float* RS = p.ws + L.rs + (size_t)ix.bi * NM * 8;
        // in-quad transposes turn four accumulator registers (4 rows x this lane's column) into one row x 4 consecutive
        // columns: every global access of the epilogue is 16 bytes wide (8 rows x 128 B per wave-instruction)
        const int l31 = lane & 31, h = lane >> 5, wa = wid / C::WN, wb = wid % C::WN, pq = lane & 3, cq = l31 >> 2;
        // The loads of a 32-row block (4 row scalars, 8 x 16 B of e, 8 x 16 B of KJ per lane: 72 VGPRs, free now that the
        // fragments are dead) are all requested before the first is used, on clamped addresses so that no branch separates
        // them: one memory round trip per block instead of one per 16 bytes (stamped build, config 5, round 4: the epilogue
        // was 35 % of the workgroup's time at 12 GB/s per CU -- latency, not bandwidth).
#pragma unroll
        for (int a2 = 0; a2 < C::A2; ++a2) {
            float2 rs[4];
            float4 e[4][C::B2], kj[4][C::B2];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int r = rtile * C::TM + wa * (32 * C::A2) + 32 * a2 + 8 * g + 4 * h + pq;
                const int rc = r < NM ? r : NM - 1;
                rs[g] = *reinterpret_cast<const float2*>(RS + (size_t)rc * 8);  // ra c1e
                const int j = rc / M;
#pragma unroll
                for (int b2 = 0; b2 < C::B2; ++b2) {
                    const int d = dt * C::TN + wb * (32 * C::B2) + 32 * b2 + 4 * cq;
                    const int dc = d < D ? d : 0;
                    e[g][b2] = *reinterpret_cast<const float4*>(E + (size_t)rc * D + dc);
                    kj[g][b2] = *reinterpret_cast<const float4*>(KJ + (size_t)j * D + dc);
                }
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int r = rtile * C::TM + wa * (32 * C::A2) + 32 * a2 + 8 * g + 4 * h + pq;
#pragma unroll
                for (int b2 = 0; b2 < C::B2; ++b2) {
                    float x[4] = {acc[a2][b2][4 * g], acc[a2][b2][4 * g + 1], acc[a2][b2][4 * g + 2], acc[a2][b2][4 * g + 3]};
                    quad_transpose4(x, lane);
                    const int d = dt * C::TN + wb * (32 * C::B2) + 32 * b2 + 4 * cq;
                    if (r < NM && d < D)
                        *reinterpret_cast<float4*>(dE + (size_t)r * D + d) =
                            make_float4(x[0] * rs[g].x + e[g][b2].x * rs[g].y + kj[g][b2].x, x[1] * rs[g].x + e[g][b2].y * rs[g].y + kj[g][b2].y,
                                        x[2] * rs[g].x + e[g][b2].z * rs[g].y + kj[g][b2].z, x[3] * rs[g].x + e[g][b2].w * rs[g].y + kj[g][b2].w);
                }
            }
        }
    };
    walk_tiles<C, true, false, Ix>(p, 16, p.B * rt * dtiles, gsm, tid, decode, epilogue);
}

// ---------------------------------------------------------------------------------------------
// k_reduce: one workgroup per batch, fixed-order sums of the per-row loss / dw / db.
// get_cos_sim's output from the similarity contraction (s3:42-80): cos[r][k] = X[r][k] + eps, the own column replaced by the
// cosine with the leave-one-out centroid, which follows from X's own column and the row / speaker scalars of the
// preparation pass exactly as in the row kernels above.  One wave per row, lanes along the slots: coalesced both ways.
__global__ __launch_bounds__(256) void ge2e_tiled_cos(Problem p, TiledWs L) {
    const int lane = threadIdx.x & 63;
    const size_t gr = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // global row
    const int N = p.N, M = p.M, NM = N * M, npad = L.npad;
    if (gr >= (size_t)p.B * NM) return;
    const int bi = (int)(gr / NM), r = (int)(gr - (size_t)bi * NM), j = r / M;
    const float* X = p.ws + L.x + ((size_t)bi * NM + r) * npad;
    const float4 rst = *reinterpret_cast<const float4*>(p.ws + L.rst + gr * 4);                   // rne ke ee
    const float4 cs = *reinterpret_cast<const float4*>(p.ws + L.cst + ((size_t)bi * N + j) * 4);  // rn kap |s| |s|^2
    const float inv_m1 = 1.0f / (float)(M - 1);
    const float cosd = own_column_cos(rst, cs, X[j], inv_m1, p.eps_cos).cosd;
    float* out = p.cos_out + gr * N;
    for (int k = lane; k < N; k += 64) out[k] = (k == j ? cosd : X[k]) + p.eps;
}

__global__ __launch_bounds__(256) void ge2e_tiled_reduce(Problem p, TiledWs L) {
    __shared__ float red[3][256];
    const int bi = blockIdx.x, tid = threadIdx.x, NM = p.N * p.M;
    const float* RS = p.ws + L.rs + (size_t)bi * NM * 8;
    float l = 0.f, a = 0.f, c = 0.f;
    for (int r = tid; r < NM; r += 256) { l += RS[(size_t)r * 8 + 5]; a += RS[(size_t)r * 8 + 6]; c += RS[(size_t)r * 8 + 7]; }
    red[0][tid] = l; red[1][tid] = a; red[2][tid] = c;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) { red[0][tid] += red[0][tid + s]; red[1][tid] += red[1][tid + s]; red[2][tid] += red[2][tid + s]; }
        __syncthreads();
    }
    if (tid == 0) {
        if (p.loss) p.loss[bi] = red[0][0];
        if (p.dw) p.dw[bi] = red[1][0];
        if (p.db) p.db[bi] = red[2][0];
    }
}

// ---------------------------------------------------------------------------------------------
bool tiled_supports(int N, int M, int D) {
    return N >= 1 && N <= 1024 && M >= 2 && D >= 8 && D <= 1024 && (D % 8) == 0;     // rows of the fp16 planes 16-byte aligned
}

TiledWs tiled_layout(int B, int N, int M, int D) {
    TiledWs L;
    const size_t NM = (size_t)N * M;
    L.npad = (N + 63) / 64 * 64;
    L.row_tiles = (int)((NM + 63) / 64);
    L.cen_tiles = L.npad / 64;
    size_t off = 0;  // offsets in floats; fp16 planes take half a float per element
    auto take = [&](size_t floats) { const size_t o = off; off = align_up(off + floats, 64); return o; };
    L.ch = take((size_t)B * N * D);          // 2 planes x [N][D] halfs
    L.eh = take((size_t)B * NM * D);         // 2 planes x [NM][D] halfs
    L.gh = take((size_t)B * NM * L.npad);    // 2 planes x [NM][npad] halfs
    L.chf = take((size_t)B * N * D);
    L.x = take((size_t)B * NM * L.npad);
    L.gc = take((size_t)B * N * D);
    L.kj = take((size_t)B * N * D);
    L.cst = take((size_t)B * N * 4);
    L.rst = take((size_t)B * NM * 4);
    L.rs = take((size_t)B * NM * 8);
    L.total = off;
    return L;
}

size_t tiled_workspace_bytes(int B, int N, int M, int D) { return tiled_layout(B, N, M, D).total * sizeof(float); }

typedef GemmCfg<128, 128> C1;
typedef GemmCfg<256, 256> C2;
typedef GemmCfgDma C3;   // the same tile, operands by LDS-DMA: the contraction's K must be a multiple of 32

static unsigned tiles(int n, int t) { return (unsigned)((n + t - 1) / t); }
// the DMA-fed contractions walk their tiles with one workgroup per CU (160 KB of LDS: one fits)
static dim3 walk_grid(unsigned ntiles) {
    int ncu = device_cu_count();
    if (ncu < 8) ncu = 8;
    ncu = ncu / 8 * 8;    // a workgroup's tiles b, b + grid, ... stay on one XCD when the grid is a multiple of 8
    return dim3(ntiles < (unsigned)ncu ? ntiles : (unsigned)ncu);
}

// Every kernel with a tile core, with what a launch needs to know of its configuration: kTileKernels[3 k + cfg - kTileC1]
// for the contraction k (kSim, kGc, kGe) in tile configuration cfg, then simrows by (contrast, full).  The launches and the
// LDS attributes both go through this table, so no instantiation is launched without its attribute.
struct TileKernel {
    void (*fn)(Problem, TiledWs);
    int tile;            // TM = TN
    unsigned threads;
    size_t lds_bytes;
    bool walks;          // at most one workgroup per CU, each walking its tiles
};
template <class C>
static constexpr TileKernel tile_kernel(void (*fn)(Problem, TiledWs), bool walks = C::DMA) {
    return {fn, C::TM, (unsigned)C::NT, C::LDS_BYTES, walks};
}
enum { kSim = 0, kGc = 1, kGe = 2, kSimrows = 9, kTileKernelCount = 13 };
static const TileKernel kTileKernels[kTileKernelCount] = {
    tile_kernel<C1>(ge2e_tiled_sim<C1>), tile_kernel<C2>(ge2e_tiled_sim<C2>), tile_kernel<C3>(ge2e_tiled_sim<C3>),
    tile_kernel<C1>(ge2e_tiled_gc<C1>), tile_kernel<C2>(ge2e_tiled_gc<C2>), tile_kernel<C3>(ge2e_tiled_gc<C3>),
    tile_kernel<C1>(ge2e_tiled_ge<C1>), tile_kernel<C2>(ge2e_tiled_ge<C2>), tile_kernel<C3>(ge2e_tiled_ge<C3>),
    // one tile per workgroup, fed by LDS-DMA
    tile_kernel<C3>(ge2e_tiled_simrows<C3, false, false>, false), tile_kernel<C3>(ge2e_tiled_simrows<C3, false, true>, false),
    tile_kernel<C3>(ge2e_tiled_simrows<C3, true, false>, false), tile_kernel<C3>(ge2e_tiled_simrows<C3, true, true>, false),
};
static const TileKernel& contraction(int k, int cfg) { return kTileKernels[3 * k + cfg - kTileC1]; }
// Allow kernels [first, first + count) of the table their dynamic LDS.  Every launch, like the fused kernels: the attribute
// is per device and a process may drive several.
static hipError_t allow_lds(int first, int count) {
    for (const TileKernel* k = kTileKernels + first; k != kTileKernels + first + count; ++k) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k->fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)k->lds_bytes);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
// `units` x (rows x cols of output, in the kernel's tiles) tiles
static void launch_tiles(const TileKernel& k, unsigned units, int rows, int cols, const Problem& p, const TiledWs& L,
                         hipStream_t stream) {
    const unsigned n = units * tiles(rows, k.tile) * tiles(cols, k.tile);
    hipLaunchKernelGGL(k.fn, k.walks ? walk_grid(n) : dim3(n), dim3(k.threads), k.lds_bytes, stream, p, L);
}
// the 256 x 256 tile where both extents of a contraction's output reach it AND its grid still gives most of the CUs a
// workgroup (a single batch of cfg5 has 160 big tiles), else 128 x 128
constexpr unsigned kFill = 192;   // (measured: the long-K gC contraction gains from the big tile even at one workgroup per CU)
// ... fed by LDS-DMA where the contraction's K is a multiple of 32, from registers where not
static int plan_tile(int B, int rows, int cols, int K) {
    if (!(rows >= 256 && cols >= 256 && (unsigned)B * tiles(rows, 256) * tiles(cols, 256) >= kFill)) return kTileC1;
    return K % 32 == 0 ? kTileC3 : kTileC2;
}

// ---- the decisions: every shape-dependent choice of launch_tiled / launch_tiled_cos, and nothing else ---------------------
TiledCosPlan plan_tiled_cos(int B, int N, int M, int D) { return {plan_prep(M, D), plan_tile(B, N * M, N, D)}; }

TiledPlan plan_tiled(int B, int N, int M, int D, int variant, bool want_grad) {
    const int NM = N * M, npad = (N + 63) / 64 * 64;
    TiledPlan t{};
    t.prep = plan_prep(M, D);
    // one 256-slot tile holds a whole similarity row: similarity contraction + row pass in one kernel (config 4)
    t.simrows = npad <= 256 && N > 128 && NM >= 256 && D % 32 == 0 && (unsigned)B * tiles(NM, 256) >= kFill;
    t.simrows_contrast = t.simrows && variant == 1;
    t.simrows_full = t.simrows && N == 256;
    t.sim = t.simrows ? kTileNone : plan_tile(B, NM, N, D);
    t.rows = t.simrows ? 0 : npad <= 256 ? 16 : 64;
    t.gc_split = 1;
    t.reduce = !want_grad;      // forward only: nothing runs after k_rows that could carry the sums
    if (!want_grad) return t;
    t.gc = plan_tile(B, N, D, NM);
    t.ge = plan_tile(B, NM, D, N);
    // k_gc has B ct dtiles tiles, each over ALL rows of its batch: at config 5 that is 192 workgroups for 256 CUs, one
    // round.  Cut the rows into S pieces when that fills the last round better (S = 4 there: three full rounds); the
    // partial sums go to the similarity block, dead once the row pass has run, and k_spk adds them in a fixed order.
    if (t.gc == kTileC3) {
        const unsigned tiles_gc = (unsigned)B * tiles(N, 256) * tiles(D, 256);
        auto fillq = [](unsigned wg) { return (double)wg / (double)((wg + 255) / 256 * 256); };
        for (int sp : {2, 4, 8})
            if (NM / 32 >= 8 * sp && (size_t)sp * N * D <= (size_t)NM * npad && fillq(tiles_gc * sp) > fillq(tiles_gc * t.gc_split) + 0.1) t.gc_split = sp;
    }
    return t;
}

hipError_t launch_tiled(const Problem& p, hipStream_t stream) {
    TiledWs L = tiled_layout(p.B, p.N, p.M, p.D);
    const TiledPlan plan = plan_tiled(p.B, p.N, p.M, p.D, p.variant, p.dE != nullptr);
    const int NM = p.N * p.M;
    const unsigned spk_blocks = (unsigned)((p.B * p.N + 3) / 4);
    const unsigned row_blocks = (unsigned)(((size_t)p.B * NM + 3) / 4);
    const hipError_t e = allow_lds(0, kTileKernelCount);
    if (e != hipSuccess) return e;
    L.gc_split = plan.gc_split;
    launch_prep(p, L, plan.prep, stream);
    if (plan.simrows)
        launch_tiles(kTileKernels[kSimrows + 2 * plan.simrows_contrast + plan.simrows_full], p.B, NM, 1, p, L, stream);
    else
        launch_tiles(contraction(kSim, plan.sim), p.B, NM, p.N, p, L, stream);
    switch (plan.rows) {
        case 16: hipLaunchKernelGGL(ge2e_tiled_rows<16>, dim3((unsigned)(((size_t)p.B * NM + 15) / 16)), dim3(256), 0, stream, p, L); break;
        case 64: hipLaunchKernelGGL(ge2e_tiled_rows<64>, dim3(row_blocks), dim3(256), 0, stream, p, L); break;
        default: break;     // the row pass ran inside simrows
    }
    if (plan.gc != kTileNone) {     // kTileNone: forward only
        launch_tiles(contraction(kGc, plan.gc), (unsigned)p.B * L.gc_split, p.N, p.D, p, L, stream);
        hipLaunchKernelGGL(ge2e_tiled_spk, dim3(spk_blocks), dim3(256), 0, stream, p, L);
    }
    if (plan.ge != kTileNone) launch_tiles(contraction(kGe, plan.ge), p.B, NM, p.D, p, L, stream);
    if (plan.reduce)   // forward only: nothing ran after k_rows that could carry the sums
        hipLaunchKernelGGL(ge2e_tiled_reduce, dim3((unsigned)p.B), dim3(256), 0, stream, p, L);
    return hipGetLastError();
}

// Forward half only, for ge2e_cos_sim: preparation, similarity contraction on the matrix cores, cos output.
hipError_t launch_tiled_cos(const Problem& p, hipStream_t stream) {
    const TiledWs L = tiled_layout(p.B, p.N, p.M, p.D);
    const TiledCosPlan plan = plan_tiled_cos(p.B, p.N, p.M, p.D);
    const int NM = p.N * p.M;
    const hipError_t e = allow_lds(3 * kSim, 3);
    if (e != hipSuccess) return e;
    launch_prep(p, L, plan.prep, stream);
    launch_tiles(contraction(kSim, plan.sim), p.B, NM, p.N, p, L, stream);
    hipLaunchKernelGGL(ge2e_tiled_cos, dim3((unsigned)(((size_t)p.B * NM + 3) / 4)), dim3(256), 0, stream, p, L);
    return hipGetLastError();
}

}  // namespace ge2e
