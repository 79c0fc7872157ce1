// The split-fp16 tile GEMM core of GE2E_IMPL_TILED (ge2e_tiled.hip holds the kernels and the plan): acc += A . B^T per
// TM x TN tile of a workgroup over operand images that are fp16 hi / lo planes in global memory.
//   GemmCfg<128,128>   128 x 128 x 64 on four waves, one LDS stage + register prefetch, two workgroups per CU
//   GemmCfg<256,256>   256 x 256 x 32 on eight waves, two LDS stages, register-staged (gemm_tile)
//   GemmCfgDma         the same tile fed by buffer_load ... lds when K is a multiple of 32 (dma_begin / dma_run), one
//                      workgroup per CU walking its tiles (walk_tiles)
// and what a kernel needs around a contraction: the walk over a workgroup's tiles with its GE2E_PROFILE stamps, and the map
// from a wave's accumulators to (row, column) of the tile (acc_quads, store_tile).
// The configurations are types of an unnamed namespace: they are template arguments of the kernels of the one source that
// includes this header, and the kernels' names carry them.
#pragma once
#include "ge2e_common.hpp"
#include "ge2e_split_gemm.hpp"

namespace ge2e {

namespace {

// ---- tile contraction TM x TN x 64 on the split-fp16 MFMA (one LDS stage + register prefetch) ----------------------
// Two shapes: <128,128> = 4 waves as 2 x 2, each 64 x 64 (74 KB of LDS -> two workgroups per CU), and <256,256> =
// 8 waves as 2 x 4, each 128 x 64 (147 KB, one workgroup per CU).  A 64 x 64 wave tile re-reads 682 B of fragments
// per MFMA (8 waves ask ~170 B/clk of a 128 B/clk LDS); 128 x 64 needs 512 B and the 256 x 256 stage halves the LDS
// WRITE bytes per MFMA, which cost 3-4x a read -- the big shape is for contractions with both extents >= 256.
// The global loads of K-step s + 1 are in flight while the MFMAs of K-step s issue.  An operand is either
// "K-contiguous" (global [row][K], LDS [T][KS + 8], fragments by ds_read_b128) or "K-rows" (global [K][col],
// LDS [KS][T + 16], fragments by the transposing read); KS = 64 (small tile) or 32 (big tile: its prefetch must fit
// in registers next to 128 accumulator VGPRs).
template <int TM_, int TN_>
struct GemmCfg {
    static constexpr int TM = TM_, TN = TN_;
    static constexpr int NT = TM_ == 256 ? 512 : 256;              // threads
    static constexpr int WN = TM_ == 256 ? 4 : 2;                  // waves along N (2 along M)
    static constexpr int A2 = TM_ / 64, B2 = TN_ / (32 * WN);      // 32-row / 32-column blocks per wave
    static constexpr int KS = TM_ == 256 ? 32 : 64;                // K per stage (the big tile's prefetch must fit in registers)
    static constexpr int KP = KS + 8;                              // K-contiguous tile pitch (halfs)
    static constexpr int NP = KS / 16;                             // 16-byte pieces per plane per thread (= T * KS / 8 / NT)
    static constexpr int PLANE_A = TM_ * KP > KS * (TM_ + 16) ? TM_ * KP : KS * (TM_ + 16);
    static constexpr int PLANE_B = TN_ * KP > KS * (TN_ + 16) ? TN_ * KP : KS * (TN_ + 16);
    // The big tile runs with TWO LDS stages (2 x 80 KB = the whole 160 KB, one workgroup per CU either way): the operands of
    // K-step s + 1 are written to the other stage behind the MFMAs of step s -- one barrier per K-step and no write phase in
    // which the matrix pipe idles.  The small tile keeps one stage (74 KB) so that two workgroups share a CU.
    static constexpr int STAGES = TM_ == 256 ? 2 : 1;
    static constexpr int STAGE_HALFS = 2 * (PLANE_A + PLANE_B);
    static constexpr size_t LDS_BYTES = (size_t)STAGES * STAGE_HALFS * sizeof(_Float16);
    static constexpr bool DMA = false;
};
// the big tile with its operands brought in by buffer_load ... lds (gemm_tile_dma below; K a multiple of 32)
struct GemmCfgDma : GemmCfg<256, 256> {
    static constexpr bool DMA = true;
};

struct Opnd {
    const _Float16* hi;   // plane pointers already offset to the tile's first row (K-contig) / first column (K-rows)
    const _Float16* lo;
    size_t ld;            // leading dimension of the global image (halfs)
    int valid;            // K-contig: valid tile rows; K-rows: valid tile columns
};

// T = tile extent of this operand (rows if K-contiguous, columns if K-rows)
template <class C, bool KC, int T>
__device__ __forceinline__ void gemm_fetch(const Opnd& o, int k0, int kvalid, int tid, uint4 (&rh)[C::NP], uint4 (&rl)[C::NP]) {
    static_assert(T * (C::KS / 8) == C::NP * C::NT, "pieces per plane per thread");
#pragma unroll
    for (int i = 0; i < C::NP; ++i) {
        const int idx = tid + C::NT * i;
        uint4 vh = make_uint4(0, 0, 0, 0), vl = vh;
        if (KC) {   // tile [T rows][KS K]
            const int row = idx / (C::KS / 8), c8 = (idx % (C::KS / 8)) * 8;
            if (row < o.valid && c8 < kvalid) {
                vh = *reinterpret_cast<const uint4*>(o.hi + (size_t)row * o.ld + k0 + c8);
                vl = *reinterpret_cast<const uint4*>(o.lo + (size_t)row * o.ld + k0 + c8);
            }
        } else {    // tile [KS K-rows][T cols]
            const int row = idx / (T / 8), c8 = (idx % (T / 8)) * 8;
            if (row < kvalid && c8 < o.valid) {
                vh = *reinterpret_cast<const uint4*>(o.hi + (size_t)(k0 + row) * o.ld + c8);
                vl = *reinterpret_cast<const uint4*>(o.lo + (size_t)(k0 + row) * o.ld + c8);
            }
        }
        rh[i] = vh; rl[i] = vl;
    }
}
// ---- the same fetch with everything that does not change along K taken out of the K loop -----------------------------
// (rocprofv3 SQ counters at config 5, round 4: 5.0 k VALU instructions per wave and tile against 1.5 k MFMAs -- the piece
// index -> (row, column) divisions, the 64-bit address arithmetic and the bounds tests of gemm_fetch, redone every K-step.)
// A plane is a buffer resource whose base is the tile's first element; a piece's lane offset is formed once (an invalid
// row / column gets an out-of-range offset and reads zeros), a K-step only moves the SCALAR offset.
typedef unsigned int tu32x4 __attribute__((ext_vector_type(4)));
struct OpndRs {
    __amdgpu_buffer_rsrc_t hi, lo;
    unsigned kstep_bytes;      // bytes one K-step advances
};
template <class C, bool KC, int T>
__device__ __forceinline__ OpndRs gemm_rsrc(const Opnd& o, int ktotal) {
    OpndRs r;
    // the furthest byte any piece touches: K-contiguous (valid rows - 1) ld + ktotal; K-rows (ktotal - 1) ld + valid columns
    // (K-rows: up to the end of the last piece that starts inside the valid columns -- ld is a multiple of 8, the row has it)
    const size_t span = KC ? ((size_t)(o.valid - 1) * o.ld + (size_t)ktotal) * 2
                           : ((size_t)(ktotal - 1) * o.ld + (size_t)((o.valid + 7) / 8 * 8)) * 2;
    r.hi = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(o.hi), 0, (int)span, 0x00020000);
    r.lo = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(o.lo), 0, (int)span, 0x00020000);
    r.kstep_bytes = KC ? (unsigned)C::KS * 2u : (unsigned)((size_t)C::KS * o.ld * 2);
    return r;
}
template <class C, bool KC, int T>
__device__ __forceinline__ void gemm_piece_offsets(const Opnd& o, int tid, unsigned (&voff)[C::NP]) {
#pragma unroll
    for (int i = 0; i < C::NP; ++i) {
        const int idx = tid + C::NT * i;
        if (KC) {   // tile [T rows][KS K]: a row beyond the tile's valid rows reads zeros
            const int row = idx / (C::KS / 8), c8 = (idx % (C::KS / 8)) * 8;
            voff[i] = row < o.valid ? (unsigned)(((size_t)row * o.ld + c8) * 2) : 0x7FFFFF00u;
        } else {    // tile [KS K-rows][T cols]: a column beyond the valid ones reads zeros
            const int row = idx / (T / 8), c8 = (idx % (T / 8)) * 8;
            voff[i] = c8 < o.valid ? (unsigned)(((size_t)row * o.ld + c8) * 2) : 0x7FFFFF00u;
        }
    }
}
// K-step kstep (whole: the buffer's range check covers a ragged last step -- K-contiguous pieces past ktotal lie beyond
// `span` only in the LAST valid row, so ragged K is handled by the caller falling back to gemm_fetch for that step)
template <class C>
__device__ __forceinline__ void gemm_fetch_rs(const OpndRs& r, const unsigned (&voff)[C::NP], unsigned koff,
                                              uint4 (&rh)[C::NP], uint4 (&rl)[C::NP]) {
#pragma unroll
    for (int i = 0; i < C::NP; ++i) {
        rh[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(r.hi, voff[i], koff, 0));
        rl[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(r.lo, voff[i], koff, 0));
    }
}
template <class C, bool KC, int T>
__device__ __forceinline__ void gemm_stash_offsets(int tid, int (&soff)[C::NP]) {
#pragma unroll
    for (int i = 0; i < C::NP; ++i) {
        const int idx = tid + C::NT * i;
        soff[i] = KC ? (idx / (C::KS / 8)) * C::KP + (idx % (C::KS / 8)) * 8 : (idx / (T / 8)) * (T + 16) + (idx % (T / 8)) * 8;
    }
}
template <class C>
__device__ __forceinline__ void gemm_stash_at(_Float16* th, _Float16* tl, const int (&soff)[C::NP], const uint4 (&rh)[C::NP],
                                              const uint4 (&rl)[C::NP]) {
#pragma unroll
    for (int i = 0; i < C::NP; ++i) {
        *reinterpret_cast<uint4*>(th + soff[i]) = rh[i];
        *reinterpret_cast<uint4*>(tl + soff[i]) = rl[i];
    }
}
template <class C, bool KC, int T>
__device__ __forceinline__ void gemm_stash(_Float16* th, _Float16* tl, int tid, const uint4 (&rh)[C::NP], const uint4 (&rl)[C::NP]) {
#pragma unroll
    for (int i = 0; i < C::NP; ++i) {
        const int idx = tid + C::NT * i;
        const int off = KC ? (idx / (C::KS / 8)) * C::KP + (idx % (C::KS / 8)) * 8
                           : (idx / (T / 8)) * (T + 16) + (idx % (T / 8)) * 8;
        *reinterpret_cast<uint4*>(th + off) = rh[i];
        *reinterpret_cast<uint4*>(tl + off) = rl[i];
    }
}
template <class C, bool KC, int T>
__device__ __forceinline__ h8 gemm_frag(const _Float16* t, int blk0, int s, int lane) {
    if (KC) return frag_row(t + (blk0 + (lane & 31)) * C::KP + 8 * (lane >> 5) + 16 * s);
    return frag_tr(t, T + 16, 16 * s, blk0, lane);
}

// ---- the 256 x 256 tile with the operands brought into LDS by the memory pipe itself (buffer_load ... lds) ---------------
// Round 4, SQ counters of the register-staged loop at config 5: the matrix pipe busy a third of the time, LDS cycles about
// equal to MFMA cycles (every K-step each wave spends 16 ds_write_b128 = 208 cycles on the store path and the transposing
// reads of the [KS][T + 16] image collide two-way), 64 VGPRs of prefetch next to 128 accumulators.  Here a K-step's four
// planes (A hi/lo, B hi/lo: 4 x 16 KB) arrive as 64 one-KiB pieces, eight per wave, with no register in between; a piece's
// LDS bytes are lane-linear (that is what the instruction does), so the images are unpadded and the bank spread comes
// from which GLOBAL 16 bytes a lane fetches (the read side applies the same exclusive-or):
//   K-rows plane  [32 K-rows][256 cols]: 512-byte rows; 64-byte column chunk c of row r sits at chunk position c ^ (r & 3)
//                 and the two 32-byte halves of a chunk are exchanged in K-rows 8-15 and 24-31 -- a half-wave of the 16-lane
//                 transposing read covers K-rows {q, 8 + q}, q = 0..3: eight different 32-byte slots of a bank row;
//   K-contig plane [256 rows][32 K]:     64-byte rows; 16-byte piece p of row r sits at piece position p ^ kc_swizzle(r % 16)
//                 = p ^ (bit 2 of r, bit 1 of r).  ds_read_b128 does not take its lanes sixteen consecutive ones at a time:
//                 with the first form's (bit 3, bit 2) the 16-row fragments of the 16x16x32 MFMA (lane = row i, K group kg:
//                 piece kg ^ f(i)) collided two-way although sixteen consecutive lanes hit sixteen different slots
//                 (SQ_LDS_BANK_CONFLICT = half of k_sim's LDS cycles); tools/ubench/lds_b128_banks.hip times all 256
//                 linear choices of f -- this one is among the conflict-free ones, and the counter is 0 again.
// Needs ktotal % 32 == 0 (a K-contiguous piece past the end of K would read the next row); other shapes keep the loop above.
constexpr int DMA_PL = 32 * 256;            // halfs per plane
constexpr int DMA_ST = 4 * DMA_PL;          // halfs per stage (64 KB)
typedef __attribute__((address_space(3))) void* lds_void_p;
typedef float acc4 __attribute__((ext_vector_type(4)));   // a 16 x 16 accumulator block

// K-contiguous plane: the piece position of row r's piece p is p ^ kc_swizzle(r % 16)
__device__ __forceinline__ int kc_swizzle(int r) { return (r >> 1) & 3; }
// per-lane byte offsets of this wave's two pieces (j = wave, wave + 8) of one operand's planes
template <bool KC>
__device__ __forceinline__ void dma_piece_offsets(const Opnd& o, int lane, int wid, unsigned (&vo)[2]) {
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
        const int j = wid + 8 * jj;
        if (KC) {   // piece = 16 rows x 64 B; lane -> row 16 j + lane / 4, LDS piece position lane & 3
            const int row = 16 * j + (lane >> 2), pc = (lane & 3) ^ kc_swizzle(lane >> 2);
            vo[jj] = row < o.valid ? (unsigned)(((size_t)row * o.ld + 8 * pc) * 2) : 0x7FFFFF00u;
        } else {    // piece = 2 K-rows x 512 B; lane -> row 2 j + lane / 32, LDS chunk position (lane & 31) / 4
            const int row = 2 * j + (lane >> 5), ch = ((lane & 31) >> 2) ^ (row & 3);
            const int c8 = 32 * ch + 8 * ((lane & 3) ^ ((row >> 2) & 2));
            vo[jj] = c8 < o.valid ? (unsigned)(((size_t)row * o.ld + c8) * 2) : 0x7FFFFF00u;
        }
    }
}
// The pieces are issued from inline asm: hipcc counts a `buffer_load ... lds` it knows about as a store to every LDS
// address and puts s_waitcnt vmcnt(0) in front of the next ds_read -- the fetch of K-step s + 1 would be drained before
// the first fragment of step s is read (seen in the ISA of the builtin form).  M0 (the piece's LDS byte address) is written
// in the statement that uses it; the wait is ours (dma_wait), in front of the barrier that hands the stage over.
struct DmaRs { tu32x4 hi, lo; unsigned kstep_bytes; };
template <class C, bool KC, int T>
__device__ __forceinline__ DmaRs dma_rsrc(const Opnd& o, int ktotal) {
    const size_t span = KC ? ((size_t)(o.valid - 1) * o.ld + (size_t)ktotal) * 2
                           : ((size_t)(ktotal - 1) * o.ld + (size_t)((o.valid + 7) / 8 * 8)) * 2;
    const unsigned long long ah = (unsigned long long)o.hi, al = (unsigned long long)o.lo;
    DmaRs r;
    r.hi = tu32x4{(unsigned)ah, (unsigned)(ah >> 32) & 0xFFFFu, (unsigned)span, 0x00020000u};
    r.lo = tu32x4{(unsigned)al, (unsigned)(al >> 32) & 0xFFFFu, (unsigned)span, 0x00020000u};
    r.kstep_bytes = KC ? (unsigned)C::KS * 2u : (unsigned)((size_t)C::KS * o.ld * 2);
    return r;
}
__device__ __forceinline__ void dma_piece(const tu32x4& rs, unsigned lds_byte, unsigned voff, unsigned soff) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
                 :: "s"(lds_byte), "v"(voff), "s"(rs), "s"(soff) : "memory");
}
__device__ __forceinline__ void dma_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void dma_issue(const DmaRs& rA, const DmaRs& rB, const unsigned (&voA)[2], const unsigned (&voB)[2],
                                          unsigned kA, unsigned kB, unsigned stage_byte, int wid) {
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
        const unsigned d = stage_byte + (unsigned)(wid + 8 * jj) * 1024u;
        dma_piece(rA.hi, d, voA[jj], kA);
        dma_piece(rA.lo, d + 2u * DMA_PL, voA[jj], kA);
        dma_piece(rB.hi, d + 4u * DMA_PL, voB[jj], kB);
        dma_piece(rB.lo, d + 6u * DMA_PL, voB[jj], kB);
    }
}
// all but the n most recent memory instructions of this wave have completed (they complete in issue order)
__device__ __forceinline__ void dma_wait_but(int n) {
    if (n >= 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
// fragment of 16-row / 16-column block `blk` (0..15 inside the tile) of a plane for v_mfma_f32_16x16x32_f16: lane
// (i = lane % 16, kg = lane / 16) gets row / column i of the block, K = 8 kg .. 8 kg + 7 of the K-step
template <bool KC>
__device__ __forceinline__ h8 dma_frag(const _Float16* pl, int blk, int lane) {
    const int i = lane & 15, kg = lane >> 4;
    if (KC) return frag_row(pl + (16 * blk + i) * 32 + 8 * (kg ^ kc_swizzle(i)));
    const int q = i >> 2, pp = i & 3;     // the transposing read: lane 4 q + pp names K-row q, columns 4 pp .. 4 pp + 3
    const _Float16* p = pl + (8 * kg + q) * 256 + 32 * ((blk >> 1) ^ q) + 16 * ((blk ^ kg) & 1) + 4 * pp;
    const h4 t0 = tr_read4(p);
    const h4 t1 = tr_read4(p + 4 * 256);
    return __builtin_shufflevector(t0, t1, 0, 1, 2, 3, 4, 5, 6, 7);
}
#ifdef GE2E_PROFILE
#define DMA_STAMP(i)                                                          \
    do {                                                                      \
        __builtin_amdgcn_sched_barrier(0);                                    \
        const unsigned long long now_ = __builtin_amdgcn_s_memtime();         \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                    \
        if (t_first) t_first[i] += now_ - last_;                              \
        last_ = now_;                                                         \
        __builtin_amdgcn_sched_barrier(0);                                    \
    } while (0)
#else
#define DMA_STAMP(i)
#endif
// A contraction in two calls, so that a workgroup that walks several tiles can ask for the NEXT tile's first two stages
// before it writes the current tile out (dma_begin ... epilogue ... dma_run): the ~5 k cycles in which a fresh workgroup
// waits for its first stage, and the launch of a workgroup per tile, go away.
struct DmaJob {
    DmaRs rA, rB;
    unsigned voA[2], voB[2];
    int nk;
};
template <class C, bool AKC, bool BKC>
__device__ __forceinline__ void dma_begin(DmaJob& j, const Opnd& A, const Opnd& B, int ktotal, _Float16* sm, int tid) {
    static_assert(C::TM == 256 && C::TN == 256 && C::KS == 32 && (size_t)2 * DMA_ST * 2 <= C::LDS_BYTES, "big tile only");
    const int lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    j.rA = dma_rsrc<C, AKC, C::TM>(A, ktotal);
    j.rB = dma_rsrc<C, BKC, C::TN>(B, ktotal);
    dma_piece_offsets<AKC>(A, lane, wid, j.voA);
    dma_piece_offsets<BKC>(B, lane, wid, j.voB);
    j.nk = ktotal / 32;
    const unsigned sm_byte = (unsigned)(unsigned long long)(lds_void_p)sm;
    dma_issue(j.rA, j.rB, j.voA, j.voB, 0u, 0u, sm_byte, wid);
    if (j.nk > 1) dma_issue(j.rA, j.rB, j.voA, j.voB, j.rA.kstep_bytes, j.rB.kstep_bytes, sm_byte + 2u * DMA_ST, wid);
}
// drain_all: memory instructions younger than the job's pieces may be outstanding (the previous tile's epilogue) -- wait
// for everything instead of "all but the second stage's eight pieces".
template <class C, bool AKC, bool BKC>
__device__ __forceinline__ void dma_run(const DmaJob& j, _Float16* sm, int tid, f32x16 (&acc)[C::A2][C::B2], bool drain_all,
                                        unsigned long long* t_first = nullptr) {
    const int lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6), wa = wid / C::WN, wb = wid % C::WN;
    const int ablk0 = wa * C::A2, bblk0 = wb * C::B2;
    const DmaRs& rA = j.rA;
    const DmaRs& rB = j.rB;
    const unsigned (&voA)[2] = j.voA;
    const unsigned (&voB)[2] = j.voB;
    const unsigned sm_byte = (unsigned)(unsigned long long)(lds_void_p)sm;
    // The products run on v_mfma_f32_16x16x32_f16 (one MFMA = a whole K-step of a 16 x 16 block; tools/ubench/mfma_shapes.hip:
    // with fragments coming from LDS it sustains 16-22 % more than 32x32x16, which needs the same fragment bytes but clocks
    // ~250 MHz lower under the power cap).  A wave's 128 x 64 block = 8 A blocks x 4 B blocks, 96 MFMAs per K-step.
    // Schedule of one K-step k (fragments: A 8 x (hi, lo), B 4 x (hi, lo) = 96 VGPRs, each register read once per K-step):
    //     first half : A blocks 0-3 x B, A-major   |  behind group a: read A block 4 + a of stage k
    //     wait: own pieces of stage k + 1 landed; barrier  -- everybody has read all of stage k, stage k + 1 is whole
    //     second half: A blocks 4-7 x B, B-major   |  behind group b: the pieces of K-step k + 2 into stage k's buffer, and
    //                                                 B block b, A block b of stage k + 1 (B block b is done after group b)
    // A piece has a whole K-step (~1.3 us of MFMAs) to land, no fragment read is waited for with the matrix pipe idle, one
    // barrier per K-step.  The sched_barriers pin the order (left alone hipcc moves the barrier up to the first MFMA).
    constexpr int A16 = 2 * C::A2, B16 = 2 * C::B2;
    static_assert(A16 == 8 && B16 == 4, "schedule written for the 128 x 64 wave block");
    const int a16 = 2 * ablk0, b16 = 2 * bblk0;
    const int nk = j.nk;
    unsigned kA = nk > 1 ? rA.kstep_bytes : 0u, kB = nk > 1 ? rB.kstep_bytes : 0u;
    if (nk > 1 && !drain_all) dma_wait_but(8);       // the eight pieces of step 0 (pieces land in issue order)
    else dma_wait();
    __syncthreads();
#ifdef GE2E_PROFILE
    unsigned long long last_ = 0;
    if (t_first) {   // diagnostic build: when the first stage had landed; [1..4]: the K-step's four parts, summed
        __builtin_amdgcn_sched_barrier(0);
        t_first[0] = last_ = __builtin_amdgcn_s_memtime();
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_sched_barrier(0);
    }
#endif
    acc4 c16[A16][B16];
#pragma unroll
    for (int a = 0; a < A16; ++a)
#pragma unroll
        for (int b = 0; b < B16; ++b) c16[a][b] = acc4{0.f, 0.f, 0.f, 0.f};
    h8 fa[A16][2], fb[B16][2];
    auto read_a = [&](const _Float16* st, int a) {
        fa[a][0] = dma_frag<AKC>(st, a16 + a, lane);
        fa[a][1] = dma_frag<AKC>(st + DMA_PL, a16 + a, lane);
    };
    auto read_b = [&](const _Float16* st, int b) {
        fb[b][0] = dma_frag<BKC>(st + 2 * DMA_PL, b16 + b, lane);
        fb[b][1] = dma_frag<BKC>(st + 3 * DMA_PL, b16 + b, lane);
    };
    auto mfma = [&](int a, int b) {
        c16[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[a][0], fb[b][0], c16[a][b], 0, 0, 0);
        c16[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[a][0], fb[b][1], c16[a][b], 0, 0, 0);
        c16[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[a][1], fb[b][0], c16[a][b], 0, 0, 0);
    };
#pragma unroll
    for (int b = 0; b < B16; ++b) read_b(sm, b);
#pragma unroll
    for (int a = 0; a < 4; ++a) read_a(sm, a);
    int cur = 0;
    for (int k = 0; k < nk; ++k, cur ^= 1) {
        const _Float16* const st = sm + cur * DMA_ST;
        const _Float16* const nx = sm + (cur ^ 1) * DMA_ST;
        const unsigned stage_byte = sm_byte + (unsigned)cur * (2u * DMA_ST);
#pragma unroll
        for (int a = 0; a < 4; ++a) {                 // A blocks 0-3 on the matrix pipe, A blocks 4-7 read behind them
            if (a == 0) __builtin_amdgcn_s_setprio(1);
            if (a == 2) __builtin_amdgcn_s_setprio(0);
#pragma unroll
            for (int b = 0; b < B16; ++b) mfma(a, b);
            __builtin_amdgcn_sched_barrier(0);
            read_a(st, 4 + a);
            __builtin_amdgcn_sched_barrier(0);
        }
        DMA_STAMP(1);      // the reads of A blocks 4-7 + 48 MFMAs issued (the reads have returned)
        dma_wait();        // this wave's pieces of stage k + 1 have landed ...
        DMA_STAMP(2);
        __syncthreads();   // ... and so have everybody else's; everybody has read all of stage k
        __builtin_amdgcn_sched_barrier(0);
        DMA_STAMP(3);      // the barrier
        const bool more2 = k + 2 < nk, more1 = k + 1 < nk;
        if (more2) { kA += rA.kstep_bytes; kB += rB.kstep_bytes; }
        // Issue priority falls from barrier to barrier (3, 2 | 1, 0 over the eight MFMA groups of a K-step): of the two waves
        // that share a SIMD the one that is BEHIND wins the arbiter.  With equal priorities the older wave wins every tie,
        // finishes its K-step ~1200 cycles early and sits at the barrier while the other runs alone with every read and
        // piece it issues exposed (stamped build, views of waves 0 and 4, round 4).
#pragma unroll
        for (int b = 0; b < B16; ++b) {               // A blocks 4-7 on the matrix pipe, B-major; behind group b two pieces of
            if (b == 0) __builtin_amdgcn_s_setprio(3);    // K-step k + 2 (into stage k's buffer) and B block b, A block b of step k + 1
            if (b == 2) __builtin_amdgcn_s_setprio(2);
#pragma unroll
            for (int a = 4; a < A16; ++a) mfma(a, b);
            __builtin_amdgcn_sched_barrier(0);
            if (more2) {
                const unsigned d = stage_byte + (unsigned)(wid + 8 * (b >> 1)) * 1024u;
                if ((b & 1) == 0) {
                    dma_piece(rA.hi, d, voA[b >> 1], kA);
                    dma_piece(rA.lo, d + 2u * DMA_PL, voA[b >> 1], kA);
                } else {
                    dma_piece(rB.hi, d + 4u * DMA_PL, voB[b >> 1], kB);
                    dma_piece(rB.lo, d + 6u * DMA_PL, voB[b >> 1], kB);
                }
            }
            if (more1) { read_b(nx, b); read_a(nx, b); }
            __builtin_amdgcn_sched_barrier(0);
        }
#ifdef GE2E_PROFILE
        {   // 48 MFMAs + pieces + next step's reads issued; NOT waiting for the reads (they belong to the next step)
            __builtin_amdgcn_sched_barrier(0);
            const unsigned long long now_ = __builtin_amdgcn_s_memtime();
            if (t_first) t_first[4] += now_ - last_;
            last_ = now_;
            __builtin_amdgcn_sched_barrier(0);
        }
#endif
    }
    __builtin_amdgcn_s_setprio(0);
    // The epilogues (and the register-staged loop) speak the 32 x 32 accumulator layout -- lane (h = lane / 32, c = lane % 32),
    // register 4 g + j = row 8 g + 4 h + j, column c of the block.  A 16 x 16 accumulator has lane (r4 = lane / 16, c), register
    // j = row 4 r4 + j.  Two gfx950 row swaps per register pair turn the four 16 x 16 blocks X[ar][bc] of a 32 x 32 block into
    // it: v_permlane16_swap (X[ar][0], X[ar][1]) collects "h = 0 | h = 1" with lane rows (x, bc), v_permlane32_swap then
    // collects "x = 0 | x = 1" (x = g % 2) with lane rows (h, bc).  128 swaps per wave and tile, no LDS, no barrier.
#pragma unroll
    for (int a2 = 0; a2 < C::A2; ++a2)
#pragma unroll
        for (int b2 = 0; b2 < C::B2; ++b2)
#pragma unroll
            for (int ar = 0; ar < 2; ++ar)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const float pv = c16[2 * a2 + ar][2 * b2][jj], qv = c16[2 * a2 + ar][2 * b2 + 1][jj];
                    // (element copies first: __builtin_bit_cast applied to a vector ELEMENT reads element 0, hipcc 7.2)
                    const auto s1 = __builtin_amdgcn_permlane16_swap(__float_as_uint(pv), __float_as_uint(qv), false, false);
                    const auto s2 = __builtin_amdgcn_permlane32_swap(s1[0], s1[1], false, false);
                    acc[a2][b2][4 * (2 * ar) + jj] = __uint_as_float(s2[0]);
                    acc[a2][b2][4 * (2 * ar + 1) + jj] = __uint_as_float(s2[1]);
                }
}
template <class C, bool AKC, bool BKC>
__device__ __forceinline__ void gemm_tile_dma(const Opnd& A, const Opnd& B, int ktotal, _Float16* sm, int tid,
                                              f32x16 (&acc)[C::A2][C::B2], unsigned long long* t_first = nullptr) {
    DmaJob j;
    dma_begin<C, AKC, BKC>(j, A, B, ktotal, sm, tid);
    dma_run<C, AKC, BKC>(j, sm, tid, acc, false, t_first);
}

// One K-step of the register-staged loops: the KS / 16 MFMA steps of a stage whose four planes are in LDS, the B fragments
// of a step held over its A blocks.  (dma_run keeps a nest of its own: 16 x 16 x 32 MFMAs on other fragments, cut in two
// halves with the reads and pieces of the next steps placed between the groups.)
template <class C, bool AKC, bool BKC>
__device__ __forceinline__ void gemm_kstep(const _Float16* Ah, const _Float16* Al, const _Float16* Bh, const _Float16* Bl,
                                           int arow0, int bcol0, int lane, f32x16 (&acc)[C::A2][C::B2]) {
#pragma unroll
    for (int s = 0; s < C::KS / 16; ++s) {
        h8 bh[C::B2], bl[C::B2];
#pragma unroll
        for (int u = 0; u < C::B2; ++u) {
            bh[u] = gemm_frag<C, BKC, C::TN>(Bh, bcol0 + 32 * u, s, lane);
            bl[u] = gemm_frag<C, BKC, C::TN>(Bl, bcol0 + 32 * u, s, lane);
        }
#pragma unroll
        for (int a2 = 0; a2 < C::A2; ++a2) {
            const h8 ah = gemm_frag<C, AKC, C::TM>(Ah, arow0 + 32 * a2, s, lane);
            const h8 al = gemm_frag<C, AKC, C::TM>(Al, arow0 + 32 * a2, s, lane);
#pragma unroll
            for (int b2 = 0; b2 < C::B2; ++b2) acc[a2][b2] = mfma3(ah, al, bh[b2], bl[b2], acc[a2][b2]);
        }
    }
}

// acc[a2][b2] += A[wave rows + 32 a2 ..][K] . B[wave cols + 32 b2 ..][K]  over K = [0, ktotal)
template <class C, bool AKC, bool BKC>
__device__ __forceinline__ void gemm_tile(const Opnd& A, const Opnd& B, int ktotal, _Float16* sm, int tid,
                                          f32x16 (&acc)[C::A2][C::B2], unsigned long long* t_first = nullptr) {
    constexpr int KS = C::KS;
    const int lane = tid & 63, wid = tid >> 6, wa = wid / C::WN, wb = wid % C::WN;
    const int arow0 = wa * (32 * C::A2), bcol0 = wb * (32 * C::B2);
    if constexpr (C::DMA) {   // (a kernel holds ONE of the two loops: with both, the waits hipcc places for the register
        gemm_tile_dma<C, AKC, BKC>(A, B, ktotal, sm, tid, acc, t_first);   // prefetch of the other loop drain the pieces in flight)
        return;
    }
    uint4 pah[C::NP], pal[C::NP], pbh[C::NP], pbl[C::NP];
    gemm_fetch<C, AKC, C::TM>(A, 0, min(KS, ktotal), tid, pah, pal);
    gemm_fetch<C, BKC, C::TN>(B, 0, min(KS, ktotal), tid, pbh, pbl);
    if constexpr (C::STAGES == 2) {
        const OpndRs rA = gemm_rsrc<C, AKC, C::TM>(A, ktotal), rB = gemm_rsrc<C, BKC, C::TN>(B, ktotal);
        unsigned voA[C::NP], voB[C::NP];
        int soA[C::NP], soB[C::NP];
        gemm_piece_offsets<C, AKC, C::TM>(A, tid, voA);
        gemm_piece_offsets<C, BKC, C::TN>(B, tid, voB);
        gemm_stash_offsets<C, AKC, C::TM>(tid, soA);
        gemm_stash_offsets<C, BKC, C::TN>(tid, soB);
        gemm_stash_at<C>(sm, sm + C::PLANE_A, soA, pah, pal);
        gemm_stash_at<C>(sm + 2 * C::PLANE_A, sm + 2 * C::PLANE_A + C::PLANE_B, soB, pbh, pbl);
        __syncthreads();
        int cur = 0;
        unsigned kA = 0, kB = 0;
        for (int k0 = 0; k0 < ktotal; k0 += KS, cur ^= 1) {
            const _Float16* const Ah = sm + cur * C::STAGE_HALFS;
            const _Float16* const Al = Ah + C::PLANE_A;
            const _Float16* const Bh = Ah + 2 * C::PLANE_A;
            const _Float16* const Bl = Bh + C::PLANE_B;
            const bool more = k0 + KS < ktotal;
            if (more) {   // next K-step's operands: in flight under the MFMAs below
                kA += rA.kstep_bytes; kB += rB.kstep_bytes;
                if (k0 + 2 * KS <= ktotal) {     // a whole step: scalar K offset, no per-piece arithmetic
                    gemm_fetch_rs<C>(rA, voA, kA, pah, pal);
                    gemm_fetch_rs<C>(rB, voB, kB, pbh, pbl);
                } else {                          // the ragged last step of a K that is no multiple of KS
                    gemm_fetch<C, AKC, C::TM>(A, k0 + KS, ktotal - k0 - KS, tid, pah, pal);
                    gemm_fetch<C, BKC, C::TN>(B, k0 + KS, ktotal - k0 - KS, tid, pbh, pbl);
                }
            }
            gemm_kstep<C, AKC, BKC>(Ah, Al, Bh, Bl, arow0, bcol0, lane, acc);
            if (more) {   // ... and into the OTHER stage, which nobody has read since the barrier of the previous step
                _Float16* const nA = sm + (cur ^ 1) * C::STAGE_HALFS;
                gemm_stash_at<C>(nA, nA + C::PLANE_A, soA, pah, pal);
                gemm_stash_at<C>(nA + 2 * C::PLANE_A, nA + 2 * C::PLANE_A + C::PLANE_B, soB, pbh, pbl);
            }
            __syncthreads();
        }
        return;
    }
    _Float16* const Ah = sm;
    _Float16* const Al = sm + C::PLANE_A;
    _Float16* const Bh = sm + 2 * C::PLANE_A;
    _Float16* const Bl = Bh + C::PLANE_B;
    for (int k0 = 0; k0 < ktotal; k0 += KS) {
        gemm_stash<C, AKC, C::TM>(Ah, Al, tid, pah, pal);
        gemm_stash<C, BKC, C::TN>(Bh, Bl, tid, pbh, pbl);
        __syncthreads();
        if (k0 + KS < ktotal) {   // next K-step's operands: in flight under the MFMAs below
            gemm_fetch<C, AKC, C::TM>(A, k0 + KS, min(KS, ktotal - k0 - KS), tid, pah, pal);
            gemm_fetch<C, BKC, C::TN>(B, k0 + KS, min(KS, ktotal - k0 - KS), tid, pbh, pbl);
        }
        gemm_kstep<C, AKC, BKC>(Ah, Al, Bh, Bl, arow0, bcol0, lane, acc);
        __syncthreads();
    }
}
template <class C>
__device__ __forceinline__ void gemm_zero(f32x16 (&acc)[C::A2][C::B2]) {
#pragma unroll
    for (int a2 = 0; a2 < C::A2; ++a2)
#pragma unroll
        for (int b2 = 0; b2 < C::B2; ++b2)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[a2][b2][i] = 0.f;
}

// ---- a wave's accumulators as the tile's rows and columns ------------------------------------------------------------------
// acc[a2][b2][4 g + i] of lane (h = lane / 32, c = lane % 32) is row 32 a2 + 8 g + 4 h + i, column 32 b2 + c of the wave's
// block.  An in-quad transpose turns the four registers of a g (4 rows x this lane's column) into one row x 4 consecutive
// columns, so every global access of an epilogue is 16 bytes wide (8 rows x 128 B per wave-instruction): after it the lane
// holds one row and four consecutive columns of the tile.
// acc_quads: f(row, col, x) for every quad of the wave, rows ascending, x its four values after the transpose, (row, col)
// where it lies in an image in which the tile starts at (row0, col0); the sums keep this operand order.  lane and wid
// (= tid >> 6) are the caller's, formed at the top of its kernel: formed here, behind the contraction, they cost k_gc up to
// 16 VGPRs.  (k_ge's epilogue walks the same map in its own text: it requests all loads of a 32-row block before the first
// transpose, and on this visitor, in three forms, its DMA-fed instantiation took a 256th VGPR or spilled.)
template <class C, class F>
__device__ __forceinline__ void acc_quads(const f32x16 (&acc)[C::A2][C::B2], int row0, int col0, int lane, int wid, F f) {
#pragma unroll
    for (int a2 = 0; a2 < C::A2; ++a2)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int row = row0 + (wid / C::WN) * (32 * C::A2) + 32 * a2 + 8 * g + 4 * (lane >> 5) + (lane & 3);
#pragma unroll
            for (int b2 = 0; b2 < C::B2; ++b2) {
                float x[4] = {acc[a2][b2][4 * g], acc[a2][b2][4 * g + 1], acc[a2][b2][4 * g + 2], acc[a2][b2][4 * g + 3]};
                quad_transpose4(x, lane);
                f(row, col0 + (wid % C::WN) * (32 * C::B2) + 32 * b2 + 4 * ((lane & 31) >> 2), x);
            }
        }
}
// out[row][col] = 2^-16 acc over the tile at (row0, col0), inside (rows, cols) of an image with leading dimension ld
template <class C>
__device__ __forceinline__ void store_tile(const f32x16 (&acc)[C::A2][C::B2], int lane, int wid, float* out, int ld, int row0,
                                           int col0, int rows, int cols) {
    acc_quads<C>(acc, row0, col0, lane, wid, [&](int r, int c, const float (&x)[4]) {
        if (r < rows && c < cols)
            *reinterpret_cast<float4*>(out + (size_t)r * ld + c) =
                make_float4(x[0] * kSplitInv2, x[1] * kSplitInv2, x[2] * kSplitInv2, x[3] * kSplitInv2);
    });
}

// Workgroups go to the XCDs round-robin (workgroup b runs on XCD b % 8), each XCD with an L2 of its own.  Tiles are
// numbered batch-major with the tiles of one batch adjacent, so in launch order a batch's tiles -- which share an operand
// (the centroid planes in k_sim / k_ge) -- land on eight different L2s and the shared operand is fetched eight times.
// This gives the workgroups of ONE XCD a contiguous range of tile numbers instead.
__device__ __forceinline__ int xcd_major_tile(unsigned b, unsigned grid) {
    const unsigned per = grid / 8;
    return b < per * 8 ? (int)((b % 8) * per + b / 8) : (int)b;
}

// One workgroup, several tiles (the DMA configuration only; launched with min(tiles, CUs) workgroups): `decode(t, A, B, ix)`
// sets a tile's operands and indices, `epilogue(ix, acc)` writes it out.  The next tile's first two stages are requested
// before the current tile's epilogue; virtual workgroup numbers b, b + grid, ... keep a workgroup on one XCD's contiguous
// range of tiles (xcd_major_tile above; grid is a multiple of 8 or a single pass).
// GE2E_PROFILE builds: eight cycle sums of the workgroup at p.prof + prof_base -- [0] up to the first stage of a tile having
// landed, [1] the contraction, [2] the epilogue, [4..7] the four parts of dma_run's K-step.
template <class C, bool AKC, bool BKC, class Ix, class Decode, class Epilogue>
__device__ __forceinline__ void walk_tiles(const Problem& p, int prof_base, int ntiles, _Float16* sm, int tid, Decode decode,
                                           Epilogue epilogue_) {
    GE2E_PROF_DECL(8)
    unsigned long long t_first[5] = {0, 0, 0, 0, 0};
    auto epilogue = [&](const Ix& ix, f32x16 (&acc)[C::A2][C::B2]) {
        GE2E_PROF_AT(0, t_first[0]);
        GE2E_PROF(1);
        epilogue_(ix, acc);
        GE2E_PROF(2);
    };
    f32x16 acc[C::A2][C::B2];
    if constexpr (!C::DMA) {    // one tile per workgroup
        Opnd A, Bo; Ix ix; int ktotal;
        decode(xcd_major_tile(blockIdx.x, gridDim.x), A, Bo, ix, ktotal);
        gemm_zero<C>(acc);
        gemm_tile<C, AKC, BKC>(A, Bo, ktotal, sm, tid, acc);
        epilogue(ix, acc);
    } else {
        int lin = blockIdx.x;
        Opnd A, Bo; Ix ix; int ktotal;
        decode(xcd_major_tile(lin, ntiles), A, Bo, ix, ktotal);
        DmaJob j;
        dma_begin<C, AKC, BKC>(j, A, Bo, ktotal, sm, tid);
        bool first = true;
        for (;;) {
            gemm_zero<C>(acc);
            dma_run<C, AKC, BKC>(j, sm, tid, acc, !first, t_first);
            first = false;
            const int nlin = lin + (int)gridDim.x;
            const Ix cur = ix;
            if (nlin < ntiles) {   // (every wave is past the last barrier of the loop: nobody reads the stages any more)
                decode(xcd_major_tile(nlin, ntiles), A, Bo, ix, ktotal);
                dma_begin<C, AKC, BKC>(j, A, Bo, ktotal, sm, tid);
            }
            epilogue(cur, acc);
            if (nlin >= ntiles) break;
            lin = nlin;
        }
    }
#ifdef GE2E_PROFILE
    for (int i = 0; i < 4; ++i) prof_acc[4 + i] = t_first[1 + i];
#endif
    GE2E_PROF_FLUSH_AT(prof_base, 8)
}

}  // namespace

}  // namespace ge2e
