// extern "C" boundary of libge2e_hip.so (include/ge2e_hip.h): argument checks,
// implementation choice, workspace sizing, launches.  No allocation, no sync, no state.
#include "../../include/ge2e_hip.h"

#include <cmath>
#include <stdlib.h>

#include "ge2e_common.hpp"
#include "ge2e_generic.hpp"
#include "ge2e_f64.hpp"
#include "ge2e_ragged.hpp"
#include "ge2e_labels.hpp"
#include "ge2e_labeled_eval.hpp"
#include "ge2e_labeled_wide.hpp"
#include "ge2e_labeled_helpers.hpp"
#include "ge2e_enroll.hpp"
#include "ge2e_encoder.hpp"
#include "ge2e_encoder_train.hpp"
#include "ge2e_melspec.hpp"
#include "ge2e_resample.hpp"
#include "ge2e_vad.hpp"
#include "ge2e_optim.hpp"
#include "ge2e_identify.hpp"
#include "ge2e_snorm.hpp"
#include "ge2e_helpers.hpp"
#include "ge2e_fused.hpp"
#include "ge2e_selftest.hpp"
#include "ge2e_tiled.hpp"
#include "ge2e_team_kernel.hpp"
#include "ge2e_tail.hpp"
#include "ge2e_wave.hpp"
#include "ge2e_plan.hpp"

using namespace ge2e;

namespace {

#ifdef GE2E_PROFILE
unsigned long long* g_prof = nullptr;  // diagnostic build only
#endif

bool shape_ok(int B, int N, int M, int D) { return B >= 1 && N >= 1 && M >= 2 && D >= 1; }

// The ragged entry point's shape: R rows shared by N speakers of at least two rows each.
bool ragged_shape_ok(int B, int N, int R, int D) { return B >= 1 && N >= 1 && D >= 1 && (long long)R >= 2LL * N; }

// The masked entries' shape: N is a bound there, so R >= 2 N is not asked for.
bool masked_shape_ok(int B, int N, int R, int D) { return B >= 1 && N >= 1 && R >= 1 && D >= 1; }

// The index entry points' shape.
bool index_shape_ok(int B, int N, int R) { return B >= 1 && N >= 1 && R >= 1; }

bool variant_ok(int v) { return v == GE2E_VARIANT_SOFTMAX || v == GE2E_VARIANT_CONTRAST; }

// The NULL rule of every loss entry point: inputs and the loss always, and whoever asks for dE takes dw and db with it.
bool loss_ptrs_ok(const void* E, const void* w, const void* b, const void* loss, const void* dE, const void* dw,
                  const void* db) {
    return E && w && b && loss && (!dE || (dw && db));
}

// A caller's workspace: present, large enough, aligned (256 bytes; the cosine backward's asks for 16).
bool workspace_ok(const void* workspace, size_t workspace_bytes, size_t need, uintptr_t align = 256) {
    return workspace && workspace_bytes >= need && !((uintptr_t)workspace & (align - 1));
}

// The kernels move 16 bytes per lane to and from E / dE.  (A null pointer -- no dE -- is aligned.)
bool aligned16(const void* p) { return !((uintptr_t)p & 15); }
// The audio entries read and write single words: float32 and int32 (aligned4), int64 (aligned8).
bool aligned4(const void* p) { return !((uintptr_t)p & 3); }
bool aligned8(const void* p) { return !((uintptr_t)p & 7); }

// The checks of every loss entry point behind its NULL rule, in the order that is part of the ABI: shape, variant,
// [implementation], workspace, alignment of E and dE; GE2E_OK (0) when all hold.  `shape_good` is the entry's own shape
// predicate.  `impl` and `need` run only once shape and variant hold, in this order: `impl` answers GE2E_OK or the code
// of an implementation that cannot run the shape, `need` the workspace bytes of the call (0: it takes none, and the
// workspace is not looked at).
template <class Need, class Impl = int (*)()>
int loss_checks(bool shape_good, int variant, Need need, const void* workspace, size_t workspace_bytes, const void* E,
                const void* dE, Impl impl = [] { return GE2E_OK; }) {
    if (!shape_good) return GE2E_ERR_SHAPE;
    if (!variant_ok(variant)) return GE2E_ERR_VARIANT;
    if (const int code = impl()) return code;
    const size_t bytes = need();
    if (bytes > 0 && !workspace_ok(workspace, workspace_bytes, bytes)) return GE2E_ERR_WORKSPACE;
    if (!aligned16(E) || !aligned16(dE)) return GE2E_ERR_ALIGN;
    return GE2E_OK;
}

template <class T>
T log_eps_of(T eps) { return eps > T(0) ? std::log(eps) : T(-INFINITY); }   // std::log(float) is logf

// The launch description of a loss entry point's argument list (P = Problem with T = float, ProblemF64 with T = double,
// ProblemRagged with T = float), without its shape.  Everything else starts as zero: no cos_out, no grid cap, no test
// abort, not raw; ws and log_eps are the caller's.
template <class P, class T>
P make_problem_io(const T* E, const T* w, const T* b, T eps_cos, T eps, int variant, T* loss, T* per_emb_loss, T* dE, T* dw,
                  T* db) {
    P p{};
    p.E = E; p.w = w; p.b = b; p.loss = loss; p.per = per_emb_loss;
    p.dE = dE; p.dw = dw; p.db = db;
    p.variant = variant; p.eps_cos = eps_cos; p.eps = eps;
    return p;
}

// ... and with the dense (B, N, M, D) shape.
template <class P, class T>
P make_problem(const T* E, int B, int N, int M, int D, const T* w, const T* b, T eps_cos, T eps, int variant, T* loss,
               T* per_emb_loss, T* dE, T* dw, T* db) {
    P p = make_problem_io<P>(E, w, b, eps_cos, eps, variant, loss, per_emb_loss, dE, dw, db);
    p.B = B; p.N = N; p.M = M; p.D = D;
    return p;
}

// ... and with what the ragged kernel's three entry points add, on their checked workspace: they differ in `order` (null:
// the rows lie speaker after speaker), `active` (null: every row and speaker counts) and NA (read with `active` only).
ProblemRagged ragged_problem(ProblemRagged p, const int* off, const int* order, const int* active, int NA, int B, int N, int R,
                             int D, void* workspace) {
    p.off = off; p.order = order; p.active = active; p.NA = NA;
    p.B = B; p.N = N; p.R = R; p.D = D;
    p.ws = (float*)workspace;
    p.log_eps = log_eps_of(p.eps);
    return p;
}

// The labelled loss entries' workspace: the ragged kernel's slices -- with masking for speaker_capacity speakers, N being
// a bound there -- then the index tables (ge2e_labels.hpp).
IndexTables labeled_tables(int B, int N, int R, int D, bool masked) {
    return index_tables(ragged_workspace_bytes(B, masked ? speaker_capacity(N, R) : N, R, D), B, N, R, masked);
}

// The prologue of every entry that starts with an index kernel, behind the entry's own checks: the four tables inside the
// call's checked workspace (L: where; the plain form has no speakers and no active) and the launch.  The masked forms write
// speakers and active into the caller's buffers where the caller gives some.  Handed back: the tables the kernels behind
// read, and the launch's error.
enum IndexForm { INDEX_PLAIN, INDEX_MASKED, INDEX_LONE_SPEAKERS };
struct IndexPtrs { int *offsets, *order, *speakers, *active; hipError_t err; };
IndexPtrs run_label_index(IndexForm form, const int* labels, int B, int N, int R, const IndexTables& L, void* workspace,
                          int* speakers, int* active, void* stream) {
    char* ws = (char*)workspace;
    IndexPtrs t = {(int*)(ws + L.off), (int*)(ws + L.order), nullptr, nullptr, hipSuccess};
    if (form == INDEX_PLAIN) {
        t.err = launch_label_index(labels, B, N, R, t.offsets, t.order, (int*)(ws + L.index), (hipStream_t)stream);
        return t;
    }
    t.speakers = speakers ? speakers : (int*)(ws + L.speakers);
    t.active = active ? active : (int*)(ws + L.active);
    t.err = launch_label_index_masked(labels, B, N, R, t.offsets, t.order, t.speakers, t.active, (int*)(ws + L.index),
                                      (hipStream_t)stream, form == INDEX_LONE_SPEAKERS);
    return t;
}

// What the wide loss and the cosine backward share of a ProblemLabeledWide: the tables, the planes of the layout on the
// checked workspace (`partials`: with the tile partials, which the cosine backward has no room for) and the shape.
void wide_problem_tables(ProblemLabeledWide& p, const IndexPtrs& t, void* workspace, const LabeledWideLayout& L, bool partials,
                         int B, int N, int R, int D) {
    char* ws = (char*)workspace;
    p.off = t.offsets; p.order = t.order; p.active = t.active;
    p.CH = (float*)(ws + L.ch); p.SS = (float*)(ws + L.ss); p.GC = (float*)(ws + L.gc); p.DUS = (float*)(ws + L.dus);
    p.GCP = (float*)(ws + L.gcp); p.CST = (float*)(ws + L.cstat); p.A = (float*)(ws + L.a);
    p.RST = (float*)(ws + L.rowstat); p.spk = (int*)(ws + L.spk);
    if (partials) p.PART = (float*)(ws + L.part);
    p.B = B; p.N = N; p.R = R; p.D = D;
    p.NA = speaker_capacity(N, R);
}

// AUTO at shapes both accept (measured at N=64, M=10, D=256, interleaved in one process, tools/compare_impls.py,
// profiles/r02_team_vs_fused_split_by_B.txt): the eight-CU team kernel wins everywhere (28 us vs 117 us at B = 1,
// 96 vs 133 us at B = 128, 245 vs 298 us at B = 384, 612 vs 619 us at B = 1024, 2.32 vs 2.40 ms at B = 4096, and it moves
// 1.4x instead of 2.5x the algorithmic bytes) except where the one-workgroup-per-batch kernel just fills the chip
// once: B = 256, 166 vs 173 us.
constexpr int kSplitMinB = 208, kSplitMaxB = 256;

// The team kernel wants its workgroups co-resident.  It survives a busy device (waits bounded to milliseconds, then the
// workgroups of the same launch redo the call without teams), but a caller that KNOWS it shares the GPU -- overlapped collectives, several
// processes -- asks for GE2E_IMPL_AUTO_NO_TEAM (the only switch: the GE2E_AUTO_NO_TEAM environment override of rounds 2-3
// is gone, an implementation choice is an argument of the call).

int resolve(int B, int N, int M, int D, int variant, int impl) {
    (void)variant;
    switch (impl) {
        case GE2E_IMPL_AUTO_NO_TEAM:
        case GE2E_IMPL_AUTO:  // split-fp16 MFMA is fp32-grade (tests hold it to 2e-5) and the fastest
            // a few dozen rows: one wave per batch, exact fp32 (31..64 rows: from a few hundred batches per launch on --
            // 117-277 us against 262-408 us at B = 4096, but 30-44 us against 20-28 us for a single batch)
            if (wave_supports(N, M, D) && (!wave_is_large(N, M) || B >= 384)) return GE2E_IMPL_WAVE;
            if (impl == GE2E_IMPL_AUTO && !(B >= kSplitMinB && B <= kSplitMaxB) && N >= 16 && team_supports(N, M, D)) return GE2E_IMPL_TEAM;
            if (fused_split_supports(N, M, D)) return GE2E_IMPL_FUSED_SPLIT;
            return tiled_supports(N, M, D) ? GE2E_IMPL_TILED : GE2E_IMPL_GENERIC;
        case GE2E_IMPL_GENERIC: return GE2E_IMPL_GENERIC;
        case GE2E_IMPL_FUSED_F32: return fused_f32_supports(N, M, D) ? GE2E_IMPL_FUSED_F32 : GE2E_ERR_IMPL;
        case GE2E_IMPL_FUSED_SPLIT: return fused_split_supports(N, M, D) ? GE2E_IMPL_FUSED_SPLIT : GE2E_ERR_IMPL;
        case GE2E_IMPL_TILED: return tiled_supports(N, M, D) ? GE2E_IMPL_TILED : GE2E_ERR_IMPL;
        case GE2E_IMPL_TEAM: return team_supports(N, M, D) ? GE2E_IMPL_TEAM : GE2E_ERR_IMPL;
        case GE2E_IMPL_WAVE: return wave_supports(N, M, D) ? GE2E_IMPL_WAVE : GE2E_ERR_IMPL;
        default: return GE2E_ERR_IMPL;
    }
}

// The first team_head_bytes() of EVERY loss workspace are the team kernel's control block (ge2e_team.hpp), whichever
// implementation runs: the others put their scratch behind it.  A workspace that callers reuse across shapes and
// implementations (the Python module path caches one per stream) therefore keeps a clean block, and a team call is never
// pushed onto its fall-back -- with that kernel's last-bit-different results -- by what ran on the workspace before.
size_t ws_bytes(int B, int N, int M, int D, int impl) {
    size_t own = 0;
    switch (impl) {
        case GE2E_IMPL_GENERIC: own = generic_workspace_bytes(B, N, M, D); break;
        case GE2E_IMPL_FUSED_F32: own = fused_f32_workspace_bytes(B, N, M, D); break;
        case GE2E_IMPL_FUSED_SPLIT: own = fused_split_workspace_bytes(B, N, M, D); break;
        case GE2E_IMPL_TILED: own = tiled_workspace_bytes(B, N, M, D); break;
        case GE2E_IMPL_TEAM: return team_workspace_bytes(B, N, M, D);      // its layout starts with the block
        case GE2E_IMPL_WAVE: return 0;
        default: return 0;
    }
    return own > 0 ? own + team_head_bytes() : 0;
}

int run(Problem& p, int impl, void* workspace, size_t workspace_bytes, void* stream) {
    int chosen = 0;
    size_t need = 0;
    if (const int code = loss_checks(shape_ok(p.B, p.N, p.M, p.D), p.variant,
                                     [&] { return need = ws_bytes(p.B, p.N, p.M, p.D, chosen); }, workspace, workspace_bytes, p.E, p.dE,
                                     [&] { return (chosen = resolve(p.B, p.N, p.M, p.D, p.variant, impl)) < 0 ? chosen : GE2E_OK; }))
        return code;
    p.ws = (float*)((char*)workspace + (need > 0 && chosen != GE2E_IMPL_TEAM ? team_head_bytes() : 0));
#ifdef GE2E_PROFILE
    p.prof = g_prof;
#endif
    p.log_eps = log_eps_of(p.eps);
    hipError_t err = hipSuccess;
    switch (chosen) {
        case GE2E_IMPL_GENERIC: err = launch_generic(p, (hipStream_t)stream); break;
        case GE2E_IMPL_FUSED_F32: err = launch_fused_f32(p, (hipStream_t)stream); break;
        case GE2E_IMPL_FUSED_SPLIT: err = launch_fused_split(p, (hipStream_t)stream); break;
        case GE2E_IMPL_TILED: err = launch_tiled(p, (hipStream_t)stream); break;
        case GE2E_IMPL_TEAM: err = launch_team(p, (hipStream_t)stream); break;
        case GE2E_IMPL_WAVE: err = launch_wave(p, (hipStream_t)stream); break;
        default: return GE2E_ERR_IMPL;
    }
    return (int)err;
}

}  // namespace

extern "C" {

#ifdef GE2E_PROFILE
// diagnostic build only (tools/profile_phases.py): where the kernels add their phase stamps
void ge2e_debug_set_prof(void* device_u64_buffer) { g_prof = (unsigned long long*)device_u64_buffer; }
#endif

int ge2e_abi_version(void) { return GE2E_ABI_VERSION; }

const char* ge2e_strerror(int code) {
    switch (code) {
        case GE2E_OK: return "ok";
        case GE2E_ERR_NULL: return "required pointer is NULL";
        case GE2E_ERR_SHAPE: return "bad shape: need B,N,D >= 1 and M >= 2";
        case GE2E_ERR_WORKSPACE: return "workspace missing, too small or not 256-byte aligned";
        case GE2E_ERR_VARIANT: return "unknown loss variant";
        case GE2E_ERR_IMPL: return "requested implementation cannot run this shape";
        case GE2E_ERR_ALIGN: return "E / dE must be 16-byte aligned";
        default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown error";
    }
}

int ge2e_resolve_impl(int B, int N, int M, int D, int variant, int impl) {
    if (!shape_ok(B, N, M, D)) return GE2E_ERR_SHAPE;
    return resolve(B, N, M, D, variant, impl);
}

size_t ge2e_workspace_bytes(int B, int N, int M, int D, int variant, int impl) {
    if (!shape_ok(B, N, M, D)) return 0;
    const int chosen = resolve(B, N, M, D, variant, impl);
    return chosen < 0 ? 0 : ws_bytes(B, N, M, D, chosen);
}

int ge2e_workspace_init(void* workspace, size_t workspace_bytes, void* stream) {
    if (!workspace) return GE2E_ERR_NULL;
    if (workspace_bytes < team_head_bytes()) return GE2E_OK;      // too small for any team launch: nothing to prepare
    return (int)launch_team_head_init(workspace, team_head_bytes(), false, (hipStream_t)stream);   // > 0: a hipError_t, like every launch
}

int ge2e_loss_fwd_bwd(const float* E, int B, int N, int M, int D, const float* w, const float* b,
                      float eps_cos, float eps, int variant, int impl, float* loss,
                      float* per_emb_loss, float* dE, float* dw, float* db, void* workspace,
                      size_t workspace_bytes, void* stream) {
    if (!loss_ptrs_ok(E, w, b, loss, dE, dw, db)) return GE2E_ERR_NULL;
    Problem p = make_problem<Problem>(E, B, N, M, D, w, b, eps_cos, eps, variant, loss, per_emb_loss, dE, dw, db);
    return run(p, impl, workspace, workspace_bytes, stream);
}

// The double-precision loss: a kernel of its own (ge2e_f64.hip), a workspace of its own (no team control block: nothing
// else runs on it).  Same checks, in the same order, as ge2e_loss_fwd_bwd.
size_t ge2e_workspace_bytes_f64(int B, int N, int M, int D, int variant) {
    (void)variant;
    return shape_ok(B, N, M, D) ? f64_workspace_bytes(B, N, M, D) : 0;
}

int ge2e_loss_fwd_bwd_f64(const double* E, int B, int N, int M, int D, const double* w, const double* b, double eps_cos,
                          double eps, int variant, double* loss, double* per_emb_loss, double* dE, double* dw, double* db,
                          void* workspace, size_t workspace_bytes, void* stream) {
    if (!loss_ptrs_ok(E, w, b, loss, dE, dw, db)) return GE2E_ERR_NULL;
    if (const int code = loss_checks(shape_ok(B, N, M, D), variant, [&] { return f64_workspace_bytes(B, N, M, D); }, workspace,
                                     workspace_bytes, E, dE))
        return code;
    ProblemF64 p = make_problem<ProblemF64>(E, B, N, M, D, w, b, eps_cos, eps, variant, loss, per_emb_loss, dE, dw, db);
    p.ws = (double*)workspace;
    p.log_eps = log_eps_of(eps);
    return (int)launch_f64(p, (hipStream_t)stream);
}

// The ragged loss (every speaker its own utterance count): a kernel of its own (ge2e_ragged.hip) on a workspace of its own,
// like the double-precision one.  Same checks, in the same order.  What the offsets HOLD is the caller's word: reading
// them here would take a synchronisation; the kernel clamps them, so a broken table cannot reach outside the buffers.
size_t ge2e_workspace_bytes_ragged(int B, int N, int R, int D, int variant) {
    (void)variant;
    return ragged_shape_ok(B, N, R, D) ? ragged_workspace_bytes(B, N, R, D) : 0;
}

int ge2e_loss_fwd_bwd_ragged(const float* E, const int* offsets, int B, int N, int R, int D, const float* w, const float* b,
                             float eps_cos, float eps, int variant, float* loss, float* per_row_loss, float* dE, float* dw,
                             float* db, void* workspace, size_t workspace_bytes, void* stream) {
    if (!offsets || !loss_ptrs_ok(E, w, b, loss, dE, dw, db)) return GE2E_ERR_NULL;
    if (const int code = loss_checks(ragged_shape_ok(B, N, R, D), variant, [&] { return ragged_workspace_bytes(B, N, R, D); },
                                     workspace, workspace_bytes, E, dE))
        return code;
    const ProblemRagged p = ragged_problem(make_problem_io<ProblemRagged>(E, w, b, eps_cos, eps, variant, loss, per_row_loss, dE, dw, db),
                                           offsets, nullptr, nullptr, 0, B, N, R, D, workspace);
    return (int)launch_ragged(p, (hipStream_t)stream);
}

// The ragged loss from one speaker label per row, rows in any order: the index kernel (ge2e_labels.hip) writes the offset
// table and the row order into this entry's own workspace, the ragged kernel's gathering instantiation reads them.  Same
// checks, in the same order.  What the labels HOLD is the caller's word: reading them here would take a synchronisation;
// the index kernel clamps them, so the order is a permutation whatever they hold and nothing reaches outside the buffers.
// The masked form (labels of ANY content, include/ge2e_hip.h) decides on the device which rows and speakers count and
// leaves their numbers in `active`.
size_t ge2e_label_index_workspace_bytes(int B, int N, int R) {
    return index_shape_ok(B, N, R) ? label_index_workspace_bytes(B, N, R) : 0;
}

size_t ge2e_label_index_masked_workspace_bytes(int B, int N, int R) {
    return index_shape_ok(B, N, R) ? label_index_masked_workspace_bytes(B, N, R) : 0;
}

namespace {
// Both index entry points: `masked` adds speakers and active to the required pointers and picks the kernel.
int label_index(bool masked, const int* labels, int B, int N, int R, int* offsets, int* order, int* speakers, int* active,
                void* workspace, size_t workspace_bytes, void* stream) {
    if (!labels || !offsets || !order || (masked && (!speakers || !active))) return GE2E_ERR_NULL;
    if (!index_shape_ok(B, N, R)) return GE2E_ERR_SHAPE;
    const size_t need = masked ? label_index_masked_workspace_bytes(B, N, R) : label_index_workspace_bytes(B, N, R);
    if (need > 0 && !workspace_ok(workspace, workspace_bytes, need)) return GE2E_ERR_WORKSPACE;
    if (masked) return (int)launch_label_index_masked(labels, B, N, R, offsets, order, speakers, active, (int*)workspace,
                                                      (hipStream_t)stream);
    return (int)launch_label_index(labels, B, N, R, offsets, order, (int*)workspace, (hipStream_t)stream);
}
}  // namespace

int ge2e_label_index(const int* labels, int B, int N, int R, int* offsets, int* order, void* workspace, size_t workspace_bytes,
                     void* stream) {
    return label_index(false, labels, B, N, R, offsets, order, nullptr, nullptr, workspace, workspace_bytes, stream);
}

int ge2e_label_index_masked(const int* labels, int B, int N, int R, int* offsets, int* order, int* speakers, int* active,
                            void* workspace, size_t workspace_bytes, void* stream) {
    return label_index(true, labels, B, N, R, offsets, order, speakers, active, workspace, workspace_bytes, stream);
}

size_t ge2e_workspace_bytes_labeled(int B, int N, int R, int D, int variant) {
    (void)variant;
    return ragged_shape_ok(B, N, R, D) ? labeled_tables(B, N, R, D, false).total : 0;
}

// Both labelled losses on the ragged kernel.  `masked` (labels of ANY content, include/ge2e_hip.h): N is a bound in the shape
// rule, the masked index kernel runs, and its `active` gives the ragged kernel's masked instantiation its extents.
static int labeled_loss(bool masked, const float* E, const int* labels, int B, int N, int R, int D, const float* w,
                        const float* b, float eps_cos, float eps, int variant, float* loss, float* per_row_loss, float* dE,
                        float* dw, float* db, int* active, void* workspace, size_t workspace_bytes, void* stream) {
    if (!labels || !loss_ptrs_ok(E, w, b, loss, dE, dw, db)) return GE2E_ERR_NULL;
    IndexTables L{};
    if (const int code = loss_checks(masked ? masked_shape_ok(B, N, R, D) : ragged_shape_ok(B, N, R, D), variant,
                                     [&] { return (L = labeled_tables(B, N, R, D, masked)).total; }, workspace, workspace_bytes, E, dE))
        return code;
    const IndexPtrs t = run_label_index(masked ? INDEX_MASKED : INDEX_PLAIN, labels, B, N, R, L, workspace, nullptr, active, stream);
    if (t.err != hipSuccess) return (int)t.err;
    const ProblemRagged p = ragged_problem(make_problem_io<ProblemRagged>(E, w, b, eps_cos, eps, variant, loss, per_row_loss, dE, dw, db),
                                           t.offsets, t.order, t.active, masked ? speaker_capacity(N, R) : 0, B, N, R, D, workspace);
    return (int)launch_ragged(p, (hipStream_t)stream);
}

int ge2e_loss_fwd_bwd_labeled(const float* E, const int* labels, int B, int N, int R, int D, const float* w, const float* b,
                              float eps_cos, float eps, int variant, float* loss, float* per_row_loss, float* dE, float* dw,
                              float* db, void* workspace, size_t workspace_bytes, void* stream) {
    return labeled_loss(false, E, labels, B, N, R, D, w, b, eps_cos, eps, variant, loss, per_row_loss, dE, dw, db, nullptr, workspace,
                        workspace_bytes, stream);
}

size_t ge2e_workspace_bytes_labeled_masked(int B, int N, int R, int D, int variant) {
    (void)variant;
    return masked_shape_ok(B, N, R, D) ? labeled_tables(B, N, R, D, true).total : 0;
}

int ge2e_loss_fwd_bwd_labeled_masked(const float* E, const int* labels, int B, int N, int R, int D, const float* w,
                                     const float* b, float eps_cos, float eps, int variant, float* loss, float* per_row_loss,
                                     float* dE, float* dw, float* db, int* active, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    return labeled_loss(true, E, labels, B, N, R, D, w, b, eps_cos, eps, variant, loss, per_row_loss, dE, dw, db, active, workspace,
                        workspace_bytes, stream);
}

// The masked labelled loss on many workgroups per batch (include/ge2e_hip.h, csrc/ge2e_labeled_wide.hip): the masked
// entry's checks, the masked index kernel, then the chain of wide kernels on a workspace laid out per batch.
size_t ge2e_workspace_bytes_labeled_wide(int B, int N, int R, int D, int variant) {
    (void)variant;
    return masked_shape_ok(B, N, R, D) ? labeled_wide_layout(B, N, R, D).t.total : 0;
}

int ge2e_loss_fwd_bwd_labeled_wide(const float* E, const int* labels, int B, int N, int R, int D, const float* w,
                                   const float* b, float eps_cos, float eps, int variant, float* loss, float* per_row_loss,
                                   float* dE, float* dw, float* db, int* active, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    if (!labels || !loss_ptrs_ok(E, w, b, loss, dE, dw, db)) return GE2E_ERR_NULL;
    LabeledWideLayout L{};
    if (const int code = loss_checks(masked_shape_ok(B, N, R, D), variant, [&] { return (L = labeled_wide_layout(B, N, R, D)).t.total; },
                                     workspace, workspace_bytes, E, dE))
        return code;
    const IndexPtrs t = run_label_index(INDEX_MASKED, labels, B, N, R, L.t, workspace, nullptr, active, stream);
    if (t.err != hipSuccess) return (int)t.err;
    ProblemLabeledWide p = make_problem_io<ProblemLabeledWide>(E, w, b, eps_cos, eps, variant, loss, per_row_loss, dE, dw, db);
    wide_problem_tables(p, t, workspace, L, true, B, N, R, D);
    p.log_eps = log_eps_of(p.eps);
    return (int)launch_labeled_wide(p, (hipStream_t)stream);
}

// The labelled EVALUATION calls (include/ge2e_hip.h, csrc/ge2e_labeled_eval.hip): the masked index kernel, unchanged, then
// the centroid kernel and the row kernel, all on the stream.  Checks on the host in the labelled entry's order (no loss:
// no variant step, and no dE).
size_t ge2e_cos_sim_labeled_workspace_bytes(int B, int N, int R, int D) {
    return masked_shape_ok(B, N, R, D) ? labeled_eval_layout(B, N, R, D).t.total : 0;
}

int ge2e_cos_sim_labeled(const float* E, const int* labels, int B, int N, int R, int D, float eps_cos, float eps,
                         const float* thresholds, int T, float* cos, int* col, int* speakers, int* active, int* counts,
                         void* workspace, size_t workspace_bytes, void* stream) {
    if (!E || !labels || (!cos && !counts)) return GE2E_ERR_NULL;
    if (!masked_shape_ok(B, N, R, D) || T < 0 || T > 4096 || (counts && (!thresholds || T == 0))) return GE2E_ERR_SHAPE;
    const LabeledEvalLayout L = labeled_eval_layout(B, N, R, D);
    if (!workspace_ok(workspace, workspace_bytes, L.t.total)) return GE2E_ERR_WORKSPACE;
    if (!aligned16(E)) return GE2E_ERR_ALIGN;
    const IndexPtrs t = run_label_index(INDEX_MASKED, labels, B, N, R, L.t, workspace, speakers, active, stream);
    if (t.err != hipSuccess) return (int)t.err;
    char* ws = (char*)workspace;
    ProblemLabeledEval p{};
    p.E = E;
    p.off = t.offsets;
    p.order = t.order;
    p.active = t.active;
    p.thr = counts ? thresholds : nullptr;
    p.cos = cos; p.col = col ? col : (int*)(ws + L.t.extra); p.counts = counts;
    p.CH = (float*)(ws + L.ch); p.SS = (float*)(ws + L.ss); p.CST = (float*)(ws + L.cstat); p.spk = (int*)(ws + L.spk);
    p.B = B; p.N = N; p.R = R; p.D = D;
    p.NA = speaker_capacity(N, R);
    p.T = counts ? T : 0;
    p.eps_cos = eps_cos; p.eps = eps;
    return (int)launch_labeled_eval(p, (hipStream_t)stream);
}

int ge2e_eer_counts_labeled(const float* sim, const int* col, const int* active, int B, int N, int R,
                            const float* thresholds, int T, int* counts, void* stream) {
    if (!sim || !col || !active || !thresholds || !counts) return GE2E_ERR_NULL;
    if (B < 1 || N < 1 || R < 1 || T < 1 || T > 4096) return GE2E_ERR_SHAPE;
    return (int)launch_eer_counts_labeled(sim, col, active, B, N, R, thresholds, T, counts, (hipStream_t)stream);
}

// ENROLMENT AND VERIFICATION (include/ge2e_hip.h, csrc/ge2e_enroll.hip).  The bank has no batch dimension: the index kernel
// runs on one batch, with the activity threshold 1.
size_t ge2e_enroll_workspace_bytes(int K, int R, int D) {
    return (K >= 1 && R >= 1 && D >= 1) ? enroll_layout(K, R).total : 0;
}

int ge2e_enroll_accumulate(const float* E, const int* labels, int K, int R, int D, float* sums, int* cnt, void* workspace,
                           size_t workspace_bytes, void* stream) {
    if (!E || !labels || !sums || !cnt) return GE2E_ERR_NULL;
    if (K < 1 || R < 1 || D < 1) return GE2E_ERR_SHAPE;
    const IndexTables L = enroll_layout(K, R);
    if (!workspace_ok(workspace, workspace_bytes, L.total)) return GE2E_ERR_WORKSPACE;
    if (!aligned16(E) || !aligned16(sums)) return GE2E_ERR_ALIGN;
    const IndexPtrs t = run_label_index(INDEX_LONE_SPEAKERS, labels, 1, K, R, L, workspace, nullptr, nullptr, stream);
    if (t.err != hipSuccess) return (int)t.err;
    return (int)launch_enroll_accumulate(E, t.offsets, t.order, t.speakers, t.active, K, R, D, sums, cnt, (hipStream_t)stream);
}

int ge2e_enroll_finalize(const float* sums, const int* cnt, int K, int D, float eps_cos, float* models, void* stream) {
    if (!sums || !cnt || !models) return GE2E_ERR_NULL;
    if (K < 1 || D < 1) return GE2E_ERR_SHAPE;
    return (int)launch_enroll_finalize(sums, cnt, K, D, eps_cos, models, (hipStream_t)stream);
}

// The checks, the launch description and the launch of every verification call: ge2e_verify_scores[_normed] and the selftest
// entry.  `normed`: the two tables of {mean, spread} are wanted (and the streamed form is taken).
static int verify_call(const float* E, const int* labels, const float* models, const int* cnt, int K, int R, int D,
                       float eps_cos, float eps, bool normed, const float* row_stats, const float* model_stats,
                       const float* thresholds, int T, float* scores, int* counts, int* trials, void* stream, int form) {
    if (!E || !models || !cnt || (normed && (!row_stats || !model_stats)) || (!scores && !counts) ||
        (!labels && (counts || trials)))
        return GE2E_ERR_NULL;
    if (K < 1 || R < 1 || D < 1 || T < 0 || T > 4096 || (counts && (!thresholds || T == 0)) ||
        ((counts || trials) && (long long)R * K > 2147483647LL) || form < VERIFY_AUTO || form > VERIFY_STREAMED)
        return GE2E_ERR_SHAPE;
    if (!aligned16(E) || !aligned16(models)) return GE2E_ERR_ALIGN;
    ProblemVerify p{};
    p.E = E; p.labels = labels; p.models = models; p.cnt = cnt;
    p.thr = counts ? thresholds : nullptr;
    p.scores = scores; p.counts = counts; p.trials = trials;
    if (normed) { p.row_stats = row_stats; p.model_stats = model_stats; }
    p.K = K; p.R = R; p.D = D;
    p.T = counts ? T : 0;
    p.eps_cos = eps_cos; p.eps = eps;
    return (int)launch_verify_scores(p, (VerifyForm)form, (hipStream_t)stream);
}

int ge2e_selftest_verify_form(const float* E, const int* labels, const float* models, const int* cnt, int K, int R, int D,
                              float eps_cos, float eps, const float* thresholds, int T, float* scores, int* counts, int* trials,
                              void* stream, int form) {
    return verify_call(E, labels, models, cnt, K, R, D, eps_cos, eps, false, nullptr, nullptr, thresholds, T, scores, counts,
                       trials, stream, form);
}

int ge2e_verify_scores(const float* E, const int* labels, const float* models, const int* cnt, int K, int R, int D, float eps_cos,
                       float eps, const float* thresholds, int T, float* scores, int* counts, int* trials, void* stream) {
    return ge2e_selftest_verify_form(E, labels, models, cnt, K, R, D, eps_cos, eps, thresholds, T, scores, counts, trials, stream,
                                     VERIFY_AUTO);
}

// SPEAKER IDENTIFICATION (include/ge2e_hip.h, csrc/ge2e_identify.hip).  The product call is the selftest entry with the
// split left to identify_split.
size_t ge2e_selftest_identify_workspace_bytes(int K, int R, int D, int k_top, int slices) {
    if (K < 1 || R < 1 || D < 1 || k_top < 1 || k_top > GE2E_IDENTIFY_MAX_TOP) return 0;
    return identify_workspace_bytes(R, k_top, identify_split(K, R, slices).slices);
}

size_t ge2e_identify_workspace_bytes(int K, int R, int D, int k_top) {
    return ge2e_selftest_identify_workspace_bytes(K, R, D, k_top, 0);
}

int ge2e_selftest_identify_slices(const float* E, const int* labels, const float* models, const int* cnt, int K, int R, int D,
                                  int k_top, float eps_cos, float eps, int* idx, float* score, int* rank, int* hist,
                                  void* workspace, size_t workspace_bytes, void* stream, int slices) {
    if (!E || !models || !cnt || !idx || (!labels && (rank || hist))) return GE2E_ERR_NULL;
    if (K < 1 || R < 1 || D < 1 || k_top < 1 || k_top > GE2E_IDENTIFY_MAX_TOP) return GE2E_ERR_SHAPE;
    const IdentifySplit split = identify_split(K, R, slices);
    if (!workspace_ok(workspace, workspace_bytes, identify_workspace_bytes(R, k_top, split.slices))) return GE2E_ERR_WORKSPACE;
    if (!aligned16(E) || !aligned16(models)) return GE2E_ERR_ALIGN;
    ProblemIdentify p{};
    p.E = E; p.labels = labels; p.models = models; p.cnt = cnt;
    p.idx = idx; p.score = score; p.rank = rank; p.hist = hist;
    p.part = (unsigned long long*)workspace;
    p.K = K; p.R = R; p.D = D; p.k_top = k_top;
    p.eps_cos = eps_cos; p.eps = eps;
    return (int)launch_identify(p, split, (hipStream_t)stream);
}

int ge2e_identify(const float* E, const int* labels, const float* models, const int* cnt, int K, int R, int D, int k_top,
                  float eps_cos, float eps, int* idx, float* score, int* rank, int* hist, void* workspace,
                  size_t workspace_bytes, void* stream) {
    return ge2e_selftest_identify_slices(E, labels, models, cnt, K, R, D, k_top, eps_cos, eps, idx, score, rank, hist, workspace,
                                         workspace_bytes, stream, 0);
}

// SCORE NORMALISATION (include/ge2e_hip.h, csrc/ge2e_snorm.hip).  The product call is the selftest entry with the chunk
// left to cohort_chunk_rows.
size_t ge2e_selftest_cohort_stats_workspace_bytes(int C, int R, int D, int n_top, int chunk_rows) {
    if (C < 1 || C > GE2E_COHORT_MAX || R < 1 || D < 1 || n_top < 1) return 0;
    return cohort_workspace_bytes(C, R, cohort_chunk_rows(C, chunk_rows));
}

size_t ge2e_cohort_stats_workspace_bytes(int C, int R, int D, int n_top) {
    return ge2e_selftest_cohort_stats_workspace_bytes(C, R, D, n_top, 0);
}

int ge2e_selftest_cohort_stats_chunk(const float* X, const int* sel, int sel_min, const float* cohort, const int* ccnt, int C,
                                     int R, int D, int n_top, float eps_cos, float eps, float eps_std, float* stats,
                                     void* workspace, size_t workspace_bytes, void* stream, int chunk_rows) {
    if (!X || !cohort || !ccnt || !stats) return GE2E_ERR_NULL;
    if (C < 1 || C > GE2E_COHORT_MAX || R < 1 || D < 1 || n_top < 1) return GE2E_ERR_SHAPE;
    const int chunk = cohort_chunk_rows(C, chunk_rows);
    if (!workspace_ok(workspace, workspace_bytes, cohort_workspace_bytes(C, R, chunk))) return GE2E_ERR_WORKSPACE;
    if (!aligned16(X) || !aligned16(cohort)) return GE2E_ERR_ALIGN;
    ProblemCohort p{};
    p.X = X; p.sel = sel; p.cohort = cohort; p.ccnt = ccnt;
    p.stats = stats;
    p.keys = (unsigned*)workspace;
    p.C = C; p.R = R; p.D = D; p.n_top = n_top; p.sel_min = sel_min;
    p.eps_cos = eps_cos; p.eps = eps; p.eps_std = eps_std;
    return (int)launch_cohort_stats(p, chunk, (hipStream_t)stream);
}

int ge2e_cohort_stats(const float* X, const int* sel, int sel_min, const float* cohort, const int* ccnt, int C, int R, int D,
                      int n_top, float eps_cos, float eps, float eps_std, float* stats, void* workspace, size_t workspace_bytes,
                      void* stream) {
    return ge2e_selftest_cohort_stats_chunk(X, sel, sel_min, cohort, ccnt, C, R, D, n_top, eps_cos, eps, eps_std, stats, workspace,
                                            workspace_bytes, stream, 0);
}

int ge2e_verify_scores_normed(const float* E, const int* labels, const float* models, const int* cnt, int K, int R, int D,
                              float eps_cos, float eps, const float* row_stats, const float* model_stats,
                              const float* thresholds, int T, float* scores, int* counts, int* trials, void* stream) {
    return verify_call(E, labels, models, cnt, K, R, D, eps_cos, eps, true, row_stats, model_stats, thresholds, T, scores,
                       counts, trials, stream, VERIFY_STREAMED);
}

// The DIFFERENTIABLE labelled helpers (include/ge2e_hip.h).  ge2e_cos_sim_labeled_bwd: stateless like every entry -- the
// masked index kernel and the centroid kernel run again from E and labels, the cosines are recomputed -- then the cos-grad
// rows kernel and the wide route's backward (csrc/ge2e_labeled_wide.hip), on the wide layout without its tile partials.
size_t ge2e_cos_sim_labeled_bwd_workspace_bytes(int B, int N, int R, int D) {
    return masked_shape_ok(B, N, R, D) ? labeled_wide_layout(B, N, R, D, false).t.total : 0;
}

int ge2e_cos_sim_labeled_bwd(const float* E, const int* labels, const float* g_cos, int B, int N, int R, int D, float eps_cos,
                             float* dE, int* active, void* workspace, size_t workspace_bytes, void* stream) {
    if (!E || !labels || !g_cos || !dE) return GE2E_ERR_NULL;
    if (!masked_shape_ok(B, N, R, D)) return GE2E_ERR_SHAPE;
    const LabeledWideLayout L = labeled_wide_layout(B, N, R, D, false);
    if (!workspace_ok(workspace, workspace_bytes, L.t.total)) return GE2E_ERR_WORKSPACE;
    if (!aligned16(E) || !aligned16(dE)) return GE2E_ERR_ALIGN;
    const IndexPtrs t = run_label_index(INDEX_MASKED, labels, B, N, R, L.t, workspace, nullptr, active, stream);
    if (t.err != hipSuccess) return (int)t.err;
    ProblemLabeledWide p{};
    p.E = E; p.dE = dE;
    wide_problem_tables(p, t, workspace, L, false, B, N, R, D);
    p.eps_cos = eps_cos;
    return (int)launch_labeled_cos_grad(p, g_cos, (hipStream_t)stream);
}

int ge2e_calc_loss_labeled(const float* sim, const int* col, const int* active, int B, int N, int R, float eps, int variant,
                           float* loss, float* per_row_loss, void* stream) {
    if (!sim || !col || !active || !per_row_loss) return GE2E_ERR_NULL;
    if (B < 1 || N < 1 || R < 1) return GE2E_ERR_SHAPE;
    if (!variant_ok(variant)) return GE2E_ERR_VARIANT;
    return (int)launch_calc_loss_labeled(sim, col, active, B, N, R, eps, variant, loss, per_row_loss, (hipStream_t)stream);
}

int ge2e_calc_loss_labeled_bwd(const float* sim, const int* col, const int* active, int B, int N, int R, float eps, int variant,
                               const float* g_loss, const float* g_per, float* d_sim, void* stream) {
    if (!sim || !col || !active || !d_sim) return GE2E_ERR_NULL;
    if (B < 1 || N < 1 || R < 1) return GE2E_ERR_SHAPE;
    if (!variant_ok(variant)) return GE2E_ERR_VARIANT;
    return (int)launch_calc_loss_labeled_bwd(sim, col, active, B, N, R, eps, variant, g_loss, g_per, d_sim, (hipStream_t)stream);
}

// ENCODER INFERENCE (include/ge2e_hip.h, csrc/ge2e_encoder.hip): the weights packed once, then mel windows to d-vectors in
// one launch.
// The shape-and-implementation step of every encoder entry, inference and training; the packs have no rows or frames and
// pass R = T = 1.
static int encoder_checks(int R, int T, int n_mels, int H, int L, int D) {
    if (R < 1 || T < 1 || n_mels < 1 || D < 1 || L < 1) return GE2E_ERR_SHAPE;
    return encoder_supported(n_mels, H, L, D) ? GE2E_OK : GE2E_ERR_IMPL;
}
// ... and all four steps of the two packs.
static int encoder_pack_checks(const float* flat_params, const float* packed, int n_mels, int H, int L, int D) {
    if (!flat_params || !packed) return GE2E_ERR_NULL;
    if (const int code = encoder_checks(1, 1, n_mels, H, L, D)) return code;
    return aligned16(packed) ? GE2E_OK : GE2E_ERR_ALIGN;
}

size_t ge2e_encoder_packed_bytes(int n_mels, int H, int L, int D) {
    return encoder_checks(1, 1, n_mels, H, L, D) == GE2E_OK ? encoder_packed_floats(n_mels, H, L, D) * sizeof(float) : 0;
}

int ge2e_encoder_pack(const float* flat_params, int n_mels, int H, int L, int D, float* packed, void* stream) {
    if (const int code = encoder_pack_checks(flat_params, packed, n_mels, H, L, D)) return code;
    return (int)launch_encoder_pack(flat_params, n_mels, H, L, D, packed, (hipStream_t)stream);
}

int ge2e_encode(const float* packed, const float* mel, const long long* row_start, int R, int T, int n_mels, int H, int L,
                int D, int normalize, float* out, void* stream) {
    if (!packed || !mel || !out) return GE2E_ERR_NULL;
    if (const int code = encoder_checks(R, T, n_mels, H, L, D)) return code;
    if (!aligned16(packed) || !aligned16(mel) || !aligned16(out)) return GE2E_ERR_ALIGN;
    const ProblemEncode p = {packed, mel, row_start, out, R, T, n_mels, L, D, normalize != 0, nullptr};
    return (int)launch_encode(p, H, (hipStream_t)stream);
}

int ge2e_encode_plan(int R, int T, int n_mels, int H, int L, int D, char* buf, size_t buf_bytes) {
    if (const int code = encoder_checks(R, T, n_mels, H, L, D)) return code;
    return plan_string_encode(R, H, buf, buf_bytes);
}

// ENCODER TRAINING (include/ge2e_hip.h, csrc/ge2e_encoder_train.hip): the forward that leaves a tape, the transposed pack,
// the backward through time into one flat gradient buffer.
size_t ge2e_encoder_packed_bwd_bytes(int n_mels, int H, int L, int D) {
    return encoder_checks(1, 1, n_mels, H, L, D) == GE2E_OK ? encoder_packed_bwd_floats(H, L, D) * sizeof(float) : 0;
}

int ge2e_encoder_pack_bwd(const float* flat_params, int n_mels, int H, int L, int D, float* packed_bwd, void* stream) {
    if (const int code = encoder_pack_checks(flat_params, packed_bwd, n_mels, H, L, D)) return code;
    return (int)launch_encoder_pack_bwd(flat_params, n_mels, H, L, D, packed_bwd, (hipStream_t)stream);
}

size_t ge2e_encode_train_tape_bytes(int R, int T, int n_mels, int H, int L, int D) {
    return encoder_checks(R, T, n_mels, H, L, D) == GE2E_OK ? encoder_tape_floats(R, T, H, L, D) * sizeof(float) : 0;
}

int ge2e_encode_train(const float* packed, const float* mel, const long long* row_start, int R, int T, int n_mels, int H, int L,
                      int D, int normalize, float* out, float* tape, void* stream) {
    if (!packed || !mel || !out || !tape) return GE2E_ERR_NULL;
    if (const int code = encoder_checks(R, T, n_mels, H, L, D)) return code;
    if (!aligned16(packed) || !aligned16(mel) || !aligned16(out) || !aligned16(tape)) return GE2E_ERR_ALIGN;
    const ProblemEncode p = {packed, mel, row_start, out, R, T, n_mels, L, D, normalize != 0, tape};
    return (int)launch_encode_train(p, H, (hipStream_t)stream);
}

size_t ge2e_encode_bwd_workspace_bytes(int R, int T, int n_mels, int H, int L, int D) {
    return encoder_checks(R, T, n_mels, H, L, D) == GE2E_OK
               ? encoder_bwd_workspace(R, T, n_mels, H, L, D).total * sizeof(float) : 0;
}

int ge2e_encode_bwd(const float* packed_bwd, const float* mel, const long long* row_start, int R, int T, int n_mels, int H,
                    int L, int D, int normalize, const float* tape, const float* d_out, float* d_flat_params, void* workspace,
                    void* stream) {
    if (!packed_bwd || !mel || !tape || !d_out || !d_flat_params || !workspace) return GE2E_ERR_NULL;
    if (const int code = encoder_checks(R, T, n_mels, H, L, D)) return code;
    if (!aligned16(packed_bwd) || !aligned16(mel) || !aligned16(tape) || !aligned16(d_out) || !aligned16(d_flat_params) ||
        !aligned16(workspace))
        return GE2E_ERR_ALIGN;
    const ProblemEncodeBwd p = {packed_bwd, mel, row_start, tape, d_out, d_flat_params, (float*)workspace,
                                R, T, n_mels, L, D, normalize != 0, nullptr, nullptr};
    return (int)launch_encode_bwd(p, H, (hipStream_t)stream);
}

int ge2e_encode_train_plan(int R, int T, int n_mels, int H, int L, int D, char* buf, size_t buf_bytes) {
    if (const int code = encoder_checks(R, T, n_mels, H, L, D)) return code;
    return plan_string_encode_train(R, H, buf, buf_bytes);
}

int ge2e_encode_bwd_plan(int R, int T, int n_mels, int H, int L, int D, char* buf, size_t buf_bytes) {
    if (const int code = encoder_checks(R, T, n_mels, H, L, D)) return code;
    return plan_string_encode_bwd(R, T, n_mels, H, L, D, buf, buf_bytes);
}

// MEL FRONT END (include/ge2e_hip.h, csrc/ge2e_melspec.hip): window, twiddles and basis packed once, then waveforms to
// (log-)mel frames in one launch.
size_t ge2e_melspec_packed_bytes(int n_fft, int n_mels) {
    return melspec_supported(n_fft, n_mels) ? melspec_packed_floats(n_fft, n_mels) * sizeof(float) : 0;
}

int ge2e_melspec_pack(const float* window, const float* basis, int n_fft, int n_mels, float* packed, void* stream) {
    if (!window || !basis || !packed) return GE2E_ERR_NULL;
    if (n_mels < 1) return GE2E_ERR_SHAPE;
    if (!melspec_supported(n_fft, n_mels)) return GE2E_ERR_IMPL;
    if (!aligned16(packed)) return GE2E_ERR_ALIGN;
    return (int)launch_melspec_pack(window, basis, n_fft, n_mels, packed, (hipStream_t)stream);
}

static int melspec_shape_check(int U, long long total_frames, int n_fft, int hop, int n_mels) {
    if (U < 1 || hop < 1 || n_mels < 1 || total_frames < 1) return GE2E_ERR_SHAPE;
    // (a grid of more than 2^31 - 1 tiles has no launch)
    if (!melspec_supported(n_fft, n_mels) || (total_frames + kMelTile - 1) / kMelTile > 0x7fffffffLL) return GE2E_ERR_IMPL;
    return GE2E_OK;
}

int ge2e_melspec(const float* packed, const float* wav, const long long* utt_start, const long long* utt_len,
                 const long long* utt_padded_len, const float* gain, const long long* frame_start, int U,
                 long long total_frames, int n_fft, int hop, int n_mels, int mode, float min_level_db, float ref_level_db,
                 float* out, void* stream) {
    if (!packed || !wav || !utt_start || !utt_len || !frame_start || !out) return GE2E_ERR_NULL;
    if (U < 1 || hop < 1 || n_mels < 1 || total_frames < 1 || (mode != 0 && mode != 1) || !(min_level_db < 0.f))
        return GE2E_ERR_SHAPE;
    const int rc = melspec_shape_check(U, total_frames, n_fft, hop, n_mels);
    if (rc != GE2E_OK) return rc;
    if (!aligned16(packed) || !aligned16(out) || !aligned4(wav)) return GE2E_ERR_ALIGN;
    const ProblemMelspec p = {packed, wav, utt_start, utt_len, utt_padded_len, gain, frame_start, out, total_frames,
                              U, hop, n_mels, mode, (float)pow(10.0, (double)min_level_db / 20.0), min_level_db, ref_level_db};
    return (int)launch_melspec(p, n_fft, (hipStream_t)stream);
}

int ge2e_melspec_plan(int U, long long total_frames, int n_fft, int hop, int n_mels, char* buf, size_t buf_bytes) {
    const int rc = melspec_shape_check(U, total_frames, n_fft, hop, n_mels);
    if (rc != GE2E_OK) return rc;
    return plan_string_melspec(total_frames, n_fft, buf, buf_bytes);
}

// RESAMPLING AND GAIN (include/ge2e_hip.h, csrc/ge2e_resample.hip): the bank packed once per (rates, filter), then recordings
// to the model's rate in one launch; the per-utterance gain of normalize_volume in two.
size_t ge2e_resample_packed_bytes(int L, int M, int W) {
    return resample_supported(L, M, W) ? resample_packed_floats(L, W) * sizeof(float) : 0;
}

int ge2e_resample_pack(const float* taps, int L, int M, int lead, float* packed, void* stream) {
    if (!taps || !packed) return GE2E_ERR_NULL;
    if (L < 1 || M < 1 || lead < 0) return GE2E_ERR_SHAPE;
    if (!resample_supported(L, M, 2LL * lead + 1)) return GE2E_ERR_IMPL;
    if (!aligned16(packed)) return GE2E_ERR_ALIGN;
    return (int)launch_resample_pack(taps, L, M, 2 * lead + 1, packed, (hipStream_t)stream);
}

static int resample_shape_check(int U, long long total_out, int L, int M, int lead) {
    if (U < 1 || L < 1 || M < 1 || total_out < 1 || lead < 0) return GE2E_ERR_SHAPE;
    if (!resample_supported(L, M, 2LL * lead + 1)) return GE2E_ERR_IMPL;
    // (a grid of more than 2^31 - 1 tiles has no launch)
    if (resample_grid(total_out, U, resample_plan(L, M, 2 * lead + 1).tile) > 0x7fffffffLL) return GE2E_ERR_IMPL;
    return GE2E_OK;
}

int ge2e_resample(const float* packed, const float* wav, const long long* in_start, const long long* in_len,
                  const long long* out_start, int U, long long total_out, int L, int M, int lead, float* out, void* stream) {
    if (!packed || !wav || !in_start || !in_len || !out_start || !out) return GE2E_ERR_NULL;
    const int rc = resample_shape_check(U, total_out, L, M, lead);
    if (rc != GE2E_OK) return rc;
    if (!aligned16(packed) || !aligned16(out) || !aligned4(wav)) return GE2E_ERR_ALIGN;
    const int W = 2 * lead + 1;
    const ResamplePlan plan = resample_plan(L, M, W);
    const ProblemResample p = {packed, wav, in_start, in_len, out_start, out, U, L, M, lead, W, resample_lpad(L), plan.B,
                               plan.tile, plan.span};
    return (int)launch_resample(p, plan, resample_grid(total_out, U, plan.tile), (hipStream_t)stream);
}

int ge2e_resample_plan(int U, long long total_out, int L, int M, int lead, char* buf, size_t buf_bytes) {
    const int rc = resample_shape_check(U, total_out, L, M, lead);
    if (rc != GE2E_OK) return rc;
    return plan_string_resample(total_out, U, L, M, 2 * lead + 1, buf, buf_bytes);
}

size_t ge2e_volume_gain_workspace_bytes(long long total_samples, int U) {
    return (total_samples < 0 || U < 1) ? 0 : volume_gain_workspace_bytes(U);
}

int ge2e_volume_gain(const float* wav, const long long* utt_start, const long long* utt_len, int U, float target_dbfs,
                     int increase_only, float* gain_out, void* workspace, void* stream) {
    if (!wav || !utt_start || !utt_len || !gain_out || !workspace) return GE2E_ERR_NULL;
    if (U < 1) return GE2E_ERR_SHAPE;
    if (!aligned16(workspace) || !aligned4(wav) || !aligned4(gain_out)) return GE2E_ERR_ALIGN;
    return (int)launch_volume_gain(wav, utt_start, utt_len, U, (double)target_dbfs, increase_only != 0, gain_out,
                                   (double*)workspace, (hipStream_t)stream);
}

// SILENCE TRIMMING (include/ge2e_hip.h, csrc/ge2e_vad.hip): window energies and voice flags in two launches, the mask and the
// ranks of the kept windows in one, the compaction in one.
size_t ge2e_vad_workspace_bytes(long long total_windows, int U) {
    return (total_windows < 0 || U < 1) ? 0 : vad_workspace_bytes(total_windows);
}

// the window, the window count and the grids every entry shares: SHAPE before IMPL
static int vad_shape_check(int U, long long total_windows, int S) {
    if (U < 1 || S < 1 || total_windows < 0) return GE2E_ERR_SHAPE;
    if (!vad_window_supported(S) || total_windows > 0x7fffffffLL) return GE2E_ERR_IMPL;
    return GE2E_OK;
}

static int vad_mask_check(int avg_width, int max_silence) {
    if (avg_width < 1 || max_silence < 0) return GE2E_ERR_SHAPE;
    return (avg_width > kVadMaxWidth || max_silence + 1 > kVadMaxWidth) ? GE2E_ERR_IMPL : GE2E_OK;
}

int ge2e_vad_flags(const float* wav, const long long* utt_start, const long long* utt_len, const float* gain,
                   const long long* win_start, int U, long long total_windows, int S, int floor_span, long long ratio_q8,
                   long long min_energy, unsigned char* flags, void* workspace, void* stream) {
    if (!wav || !utt_start || !utt_len || !win_start || !flags) return GE2E_ERR_NULL;
    if (floor_span < 0 || ratio_q8 < 0 || min_energy < 0) return GE2E_ERR_SHAPE;
    const int rc = vad_shape_check(U, total_windows, S);
    if (rc != GE2E_OK) return rc;
    if (floor_span > kVadMaxSpan) return GE2E_ERR_IMPL;
    if (!workspace || !aligned16(workspace)) return GE2E_ERR_WORKSPACE;
    if (!aligned4(wav) || !aligned4(gain)) return GE2E_ERR_ALIGN;
    if (total_windows == 0) return GE2E_OK;
    const ProblemVad p = {wav, utt_start, gain, win_start, U, S, total_windows};
    return (int)launch_vad_flags(p, floor_span, (unsigned long long)ratio_q8, min_energy, flags, (long long*)workspace,
                                 (hipStream_t)stream);
}

int ge2e_vad_mask(const unsigned char* flags, const long long* win_start, int U, long long total_windows, int S, int avg_width,
                  int max_silence, int* dst, long long* out_len, void* stream) {
    if (!flags || !win_start || !dst || !out_len) return GE2E_ERR_NULL;
    if (vad_mask_check(avg_width, max_silence) == GE2E_ERR_SHAPE) return GE2E_ERR_SHAPE;
    int rc = vad_shape_check(U, total_windows, S);
    if (rc == GE2E_OK) rc = vad_mask_check(avg_width, max_silence);
    if (rc != GE2E_OK) return rc;
    if (!aligned4(dst) || !aligned8(out_len)) return GE2E_ERR_ALIGN;
    // (an utterance without windows still gets its out_len = 0: the launch is per utterance)
    return (int)launch_vad_mask(flags, win_start, U, S, avg_width, max_silence, dst, out_len, (hipStream_t)stream);
}

int ge2e_vad_trim(const float* wav, const long long* utt_start, const long long* win_start, const int* dst,
                  const long long* out_start, int U, long long total_windows, int S, float* out, void* stream) {
    if (!wav || !utt_start || !win_start || !dst || !out_start || !out) return GE2E_ERR_NULL;
    const int rc = vad_shape_check(U, total_windows, S);
    if (rc != GE2E_OK) return rc;
    if (!aligned4(wav) || !aligned4(out) || !aligned4(dst)) return GE2E_ERR_ALIGN;
    if (total_windows == 0) return GE2E_OK;
    const ProblemVad p = {wav, utt_start, nullptr, win_start, U, S, total_windows};
    return (int)launch_vad_trim(p, dst, out_start, out, (hipStream_t)stream);
}

int ge2e_vad_plan(int U, long long total_windows, int S, int floor_span, int avg_width, int max_silence, char* buf,
                  size_t buf_bytes) {
    if (floor_span < 0 || vad_mask_check(avg_width, max_silence) == GE2E_ERR_SHAPE) return GE2E_ERR_SHAPE;
    int rc = vad_shape_check(U, total_windows, S);
    if (rc == GE2E_OK && floor_span > kVadMaxSpan) rc = GE2E_ERR_IMPL;
    if (rc == GE2E_OK) rc = vad_mask_check(avg_width, max_silence);
    if (rc != GE2E_OK) return rc;
    return plan_string_vad(total_windows, U, S, buf, buf_bytes);
}

// OPTIMIZER STEP (include/ge2e_hip.h, csrc/ge2e_optim.hip): both gradient clips and SGD over the flat bucket in two launches.
static_assert(kSgdMaxGroups == GE2E_SGD_MAX_GROUPS && kSgdChunk == GE2E_SGD_CHUNK && kSgdFlagZeroGrad == GE2E_SGD_FLAG_ZERO_GRAD &&
                  kSgdFlagSkipNonfinite == GE2E_SGD_FLAG_SKIP_NONFINITE, "the header's constants are the kernels'");
size_t ge2e_sgd_clip_workspace_bytes(int C) { return C < 1 ? 0 : sgd_workspace_bytes(C); }

static int sgd_shape_check(int S, int C, int G, int flags) {
    if (S < 1 || C < 1 || G < 1 || C < S || G > kSgdMaxGroups) return GE2E_ERR_SHAPE;
    return (flags & ~(kSgdFlagZeroGrad | kSgdFlagSkipNonfinite)) ? GE2E_ERR_SHAPE : GE2E_OK;
}

int ge2e_sgd_clip_step(const long long* seg, const int* chunk_start, int S, int C, int G, float* grad, float* momentum,
                       const float* hyper, float grad_scale, int flags, float* stats, int* skipped, void* workspace,
                       size_t workspace_bytes, void* stream) {
    if (!seg || !chunk_start || !grad || !hyper) return GE2E_ERR_NULL;
    if ((flags & kSgdFlagSkipNonfinite) && !skipped) return GE2E_ERR_NULL;
    const int rc = sgd_shape_check(S, C, G, flags);
    if (rc != GE2E_OK) return rc;
    if (!workspace_ok(workspace, workspace_bytes, sgd_workspace_bytes(C))) return GE2E_ERR_WORKSPACE;
    if (!aligned8(seg) || !aligned4(chunk_start) || !aligned4(grad) || !aligned4(momentum) || !aligned4(hyper) ||
        !aligned4(stats) || !aligned4(skipped))
        return GE2E_ERR_ALIGN;
    const ProblemSgd p = {seg, chunk_start, S, C, G, grad, momentum, hyper, grad_scale, flags, stats, skipped, (float*)workspace};
    return (int)launch_sgd_clip_step(p, (hipStream_t)stream);
}

int ge2e_sgd_clip_plan(int S, int C, int G, int has_momentum, int flags, char* buf, size_t buf_bytes) {
    const int rc = sgd_shape_check(S, C, G, flags);
    if (rc != GE2E_OK) return rc;
    return plan_string_sgd(C, has_momentum != 0, buf, buf_bytes);
}

// ---- diagnostics: the launch plan of a call, from the launchers' own decision functions (ge2e_plan.hpp); no GPU needed ----
int ge2e_loss_plan(int B, int N, int M, int D, int variant, int impl, int want_grad, int raw, char* buf, size_t buf_bytes) {
    if (!shape_ok(B, N, M, D)) return GE2E_ERR_SHAPE;
    if (!variant_ok(variant)) return GE2E_ERR_VARIANT;
    if (raw) return wave_supports_raw(N, M, D) ? plan_string_loss(B, N, M, D, variant, GE2E_IMPL_WAVE, want_grad != 0, true, buf, buf_bytes) : GE2E_ERR_IMPL;
    const int chosen = resolve(B, N, M, D, variant, impl);
    return chosen < 0 ? chosen : plan_string_loss(B, N, M, D, variant, chosen, want_grad != 0, false, buf, buf_bytes);
}

int ge2e_plan_atoms(char* buf, size_t buf_bytes) { return plan_string_atoms(buf, buf_bytes); }

int ge2e_raw_supported(int N, int M, int D) { return (N >= 1 && M >= 2 && D >= 1 && wave_supports_raw(N, M, D)) ? 1 : 0; }

int ge2e_loss_fwd_bwd_raw(const float* Y, const int* src, int B, int N, int M, int D, const float* w, const float* b,
                          float eps_cos, float eps, int variant, float* loss, float* per_emb_loss, float* dY, float* dw,
                          float* db, void* stream) {
    if (!loss_ptrs_ok(Y, w, b, loss, dY, dw, db)) return GE2E_ERR_NULL;
    if (const int code = loss_checks(shape_ok(B, N, M, D), variant, [] { return (size_t)0; }, nullptr, 0, Y, dY,   // (no workspace)
                                     [&] { return wave_supports_raw(N, M, D) ? GE2E_OK : GE2E_ERR_IMPL; }))
        return code;
    Problem p = make_problem<Problem>(Y, B, N, M, D, w, b, eps_cos, eps, variant, loss, per_emb_loss, dY, dw, db);
    p.log_eps = log_eps_of(eps);
    p.raw = 1; p.src = src;
    return (int)launch_wave(p, (hipStream_t)stream);
}

// Forward-only similarity matrix; w and b are not applied (s5:44 applies its own).
// get_cos_sim runs on the matrix cores (TILED's preparation pass + split-fp16 similarity contraction + a row pass for the
// leave-one-out column) where that kernel takes the shape and the contraction is big enough to pay for three launches;
// tiny shapes (the reference's N = 2..6) stay on the exact-fp32 VALU kernel.
static bool cos_on_mfma(int N, int M, int D) { return N >= 16 && tiled_supports(N, M, D); }

size_t ge2e_cos_sim_workspace_bytes(int B, int N, int M, int D) {
    if (!shape_ok(B, N, M, D)) return 0;
    const size_t g = ws_bytes(B, N, M, D, GE2E_IMPL_GENERIC);      // what run() asks for (the control block's room included)
    const size_t t = cos_on_mfma(N, M, D) ? tiled_workspace_bytes(B, N, M, D) : 0;
    return g > t ? g : t;
}

int ge2e_cos_sim_plan(int B, int N, int M, int D, char* buf, size_t buf_bytes) {
    if (!shape_ok(B, N, M, D)) return GE2E_ERR_SHAPE;
    return plan_string_cos(B, N, M, D, cos_on_mfma(N, M, D), buf, buf_bytes);
}

int ge2e_cos_sim(const float* E, int B, int N, int M, int D, float eps_cos, float eps, float* cos,
                 void* workspace, size_t workspace_bytes, void* stream) {
    if (!E || !cos) return GE2E_ERR_NULL;
    Problem p{};
    p.E = E; p.w = nullptr; p.b = nullptr; p.w_imm = 1.0f; p.b_imm = 0.0f; p.cos_out = cos;
    p.B = B; p.N = N; p.M = M; p.D = D; p.variant = GE2E_VARIANT_SOFTMAX; p.eps_cos = eps_cos; p.eps = eps;
    // (a caller that sized the workspace for the VALU kernel only -- ge2e_workspace_bytes(.., GE2E_IMPL_GENERIC), ABI 1's
    // rule -- gets the VALU kernel)
    if (shape_ok(B, N, M, D) && cos_on_mfma(N, M, D) && workspace_ok(workspace, workspace_bytes, tiled_workspace_bytes(B, N, M, D)) &&
        aligned16(E)) {
        p.ws = (float*)workspace;
        p.log_eps = log_eps_of(eps);
        return (int)launch_tiled_cos(p, (hipStream_t)stream);
    }
    return run(p, GE2E_IMPL_GENERIC, workspace, workspace_bytes, stream);
}

// get_cos_sim with the caller's centroids (the reference's second argument), forward only.
int ge2e_cos_sim_centroids(const float* E, const float* C, int B, int N, int M, int D, float eps_cos, float eps,
                           float* cos, void* stream) {
    if (!E || !C || !cos) return GE2E_ERR_NULL;
    if (!shape_ok(B, N, M, D)) return GE2E_ERR_SHAPE;
    return (int)launch_cos_centroids(E, C, B, N, N, 0, M, D, eps_cos, eps, cos, (hipStream_t)stream);
}

int ge2e_calc_loss(const float* sim, int B, int N, int M, float eps, int variant, float* loss,
                   float* per_emb_loss, void* stream) {
    if (!sim || !loss) return GE2E_ERR_NULL;
    if (B < 1 || N < 1 || M < 1) return GE2E_ERR_SHAPE;
    if (!variant_ok(variant)) return GE2E_ERR_VARIANT;
    return (int)launch_calc_loss(sim, B, N, N, 0, M, eps, variant, loss, per_emb_loss, (hipStream_t)stream);
}

int ge2e_centroids(const float* E, int B, int N, int M, int D, float* cent, void* stream) {
    if (!E || !cent) return GE2E_ERR_NULL;
    if (B < 1 || N < 1 || M < 1 || D < 1) return GE2E_ERR_SHAPE;
    return (int)launch_centroids(E, B, N, M, D, cent, (hipStream_t)stream);
}

int ge2e_utterance_centroids(const float* E, int B, int N, int M, int D, float* U, void* stream) {
    if (!E || !U) return GE2E_ERR_NULL;
    if (B < 1 || N < 1 || M < 2 || D < 1) return GE2E_ERR_SHAPE;
    return (int)launch_utt_centroids(E, B, N, M, D, U, (hipStream_t)stream);
}

int ge2e_centroids_bwd(const float* g_cent, int B, int N, int M, int D, float* dE, void* stream) {
    if (!g_cent || !dE) return GE2E_ERR_NULL;
    if (B < 1 || N < 1 || M < 1 || D < 1) return GE2E_ERR_SHAPE;
    return (int)launch_centroids_bwd(g_cent, B, N, M, D, dE, (hipStream_t)stream);
}

size_t ge2e_cos_sim_bwd_workspace_bytes(int B, int N, int M, int D) {
    return shape_ok(B, N, M, D) ? cos_bwd_workspace_bytes(B, N, N, M, D) : 0;
}

int ge2e_cos_sim_bwd(const float* E, const float* C, const float* cos, const float* g_cos, int B, int N, int M, int D,
                     float eps_cos, float eps, float* dE, float* dC, void* workspace, size_t workspace_bytes,
                     void* stream) {
    if (!E || !C || !cos || !g_cos || !dE || !dC) return GE2E_ERR_NULL;
    if (!shape_ok(B, N, M, D)) return GE2E_ERR_SHAPE;
    if (!workspace_ok(workspace, workspace_bytes, cos_bwd_workspace_bytes(B, N, N, M, D), 16)) return GE2E_ERR_WORKSPACE;
    return (int)launch_cos_bwd(E, C, cos, g_cos, B, N, N, 0, M, D, eps_cos, eps, dE, dC, (float*)workspace, (hipStream_t)stream);
}

int ge2e_calc_loss_bwd(const float* sim, int B, int N, int M, float eps, int variant, const float* g_loss,
                       const float* g_per, float* d_sim, void* stream) {
    if (!sim || !d_sim || (!g_loss && !g_per)) return GE2E_ERR_NULL;
    if (B < 1 || N < 1 || M < 1) return GE2E_ERR_SHAPE;
    if (!variant_ok(variant)) return GE2E_ERR_VARIANT;
    return (int)launch_calc_loss_bwd(sim, B, N, N, 0, M, eps, variant, g_loss, g_per, d_sim, (hipStream_t)stream);
}

// ---- the same helpers on LOCAL ROWS (the speaker-sharded loss, s3:42-80 / s3:114-127 semantics) --------------
static bool rows_ok(int B, int n, int N, int j0, int M, int D) {
    return B >= 1 && n >= 1 && N >= 1 && M >= 2 && D >= 1 && j0 >= 0 && j0 + n <= N;
}
int ge2e_cos_sim_rows(const float* E, const float* C, int B, int n, int N, int j0, int M, int D, float eps_cos, float eps,
                      float* cos, void* stream) {
    if (!E || !C || !cos) return GE2E_ERR_NULL;
    if (!rows_ok(B, n, N, j0, M, D)) return GE2E_ERR_SHAPE;
    return (int)launch_cos_centroids(E, C, B, n, N, j0, M, D, eps_cos, eps, cos, (hipStream_t)stream);
}
size_t ge2e_cos_sim_rows_bwd_workspace_bytes(int B, int n, int N, int M, int D) {
    return rows_ok(B, n, N, 0, M, D) ? cos_bwd_workspace_bytes(B, n, N, M, D) : 0;
}
int ge2e_cos_sim_rows_bwd(const float* E, const float* C, const float* cos, const float* g_cos, int B, int n, int N, int j0,
                          int M, int D, float eps_cos, float eps, float* dE, float* dC, void* workspace,
                          size_t workspace_bytes, void* stream) {
    if (!E || !C || !cos || !g_cos || !dE || !dC) return GE2E_ERR_NULL;
    if (!rows_ok(B, n, N, j0, M, D)) return GE2E_ERR_SHAPE;
    if (!workspace_ok(workspace, workspace_bytes, cos_bwd_workspace_bytes(B, n, N, M, D), 16)) return GE2E_ERR_WORKSPACE;
    return (int)launch_cos_bwd(E, C, cos, g_cos, B, n, N, j0, M, D, eps_cos, eps, dE, dC, (float*)workspace, (hipStream_t)stream);
}
int ge2e_calc_loss_rows(const float* sim, int B, int n, int N, int j0, int M, float eps, int variant, float* loss,
                        float* per_emb_loss, void* stream) {
    if (!sim || !loss) return GE2E_ERR_NULL;
    if (!rows_ok(B, n, N, j0, M, 1)) return GE2E_ERR_SHAPE;
    if (!variant_ok(variant)) return GE2E_ERR_VARIANT;
    return (int)launch_calc_loss(sim, B, n, N, j0, M, eps, variant, loss, per_emb_loss, (hipStream_t)stream);
}
int ge2e_calc_loss_rows_bwd(const float* sim, int B, int n, int N, int j0, int M, float eps, int variant, const float* g_loss,
                            const float* g_per, float* d_sim, void* stream) {
    if (!sim || !d_sim || (!g_loss && !g_per)) return GE2E_ERR_NULL;
    if (!rows_ok(B, n, N, j0, M, 1)) return GE2E_ERR_SHAPE;
    if (!variant_ok(variant)) return GE2E_ERR_VARIANT;
    return (int)launch_calc_loss_bwd(sim, B, n, N, j0, M, eps, variant, g_loss, g_per, d_sim, (hipStream_t)stream);
}

int ge2e_scale_grads(const float* dE, const float* dw, const float* db, const float* g, int g_count, int B, int N, int M,
                     int D, float* gE, float* gw, float* gb, void* stream) {
    if (!g || (gE && !dE) || (gw && !dw) || (gb && !db) || (!gE && !gw && !gb)) return GE2E_ERR_NULL;
    if (B < 1 || N < 1 || M < 1 || D < 1 || (g_count != 1 && g_count != B)) return GE2E_ERR_SHAPE;
    return (int)launch_scale_grads(dE, dw, db, g, g_count, B, (size_t)N * M * D, gE, gw, gb, (hipStream_t)stream);
}

int ge2e_normalize_unperm(const float* y, const int* src, int rows, int D, float* e, float* rnorm, void* stream) {
    if (!y || !e || !rnorm) return GE2E_ERR_NULL;
    if (rows < 1 || D < 1) return GE2E_ERR_SHAPE;
    return (int)launch_tail_fwd(y, src, rows, D, e, rnorm, (hipStream_t)stream);
}

int ge2e_normalize_unperm_bwd(const float* g, const float* e, const float* rnorm, const int* src, int rows, int D,
                              float* dy, void* stream) {
    if (!g || !e || !rnorm || !dy) return GE2E_ERR_NULL;
    if (rows < 1 || D < 1) return GE2E_ERR_SHAPE;
    return (int)launch_tail_bwd(g, e, rnorm, src, rows, D, dy, (hipStream_t)stream);
}

int ge2e_eer_counts(const float* sim, int B, int N, int M, const float* thresholds, int T, int* counts, void* stream) {
    if (!sim || !thresholds || !counts) return GE2E_ERR_NULL;
    if (B < 1 || N < 1 || M < 1 || T < 1 || T > 4096) return GE2E_ERR_SHAPE;
    return (int)launch_eer_counts(sim, B, N, M, thresholds, T, counts, (hipStream_t)stream);
}

int ge2e_sample_batch(const void* store, int store_is_f64, const long long* spk_offsets, const int* utter_idx,
                      const int* clip_start, int N, int M, int T, int L, int F, float* out, void* stream) {
    if (!store || !spk_offsets || !utter_idx || !clip_start || !out) return GE2E_ERR_NULL;
    if (N < 1 || M < 1 || T < 1 || L < 1 || L > T || F < 1 || (long long)N * M > 65535) return GE2E_ERR_SHAPE;
    return (int)launch_sample_batch(store, store_is_f64, spk_offsets, utter_idx, clip_start, N, M, T, L, F, out,
                                    (hipStream_t)stream);
}

// The three launches of GE2E_IMPL_TEAM under test conditions: ge2e_loss_fwd_bwd's argument list, and the one field of the
// problem that each of them sets.  `arg_ok`: the wrapper's own argument check, answered as a shape error behind the NULL rule.
namespace {
int selftest_team_run(int Problem::*field, int value, bool arg_ok, const float* E, int B, int N, int M, int D, const float* w,
                      const float* b, float eps_cos, float eps, int variant, float* loss, float* per_emb_loss, float* dE,
                      float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream) {
    if (!loss_ptrs_ok(E, w, b, loss, dE, dw, db)) return GE2E_ERR_NULL;
    if (!arg_ok) return GE2E_ERR_SHAPE;
    Problem p = make_problem<Problem>(E, B, N, M, D, w, b, eps_cos, eps, variant, loss, per_emb_loss, dE, dw, db);
    p.*field = value;
    return run(p, GE2E_IMPL_TEAM, workspace, workspace_bytes, stream);
}
}  // namespace

// The abort word raised before the launch: no team forms, the launch redoes the call with one workgroup per batch.
int ge2e_selftest_team_fallback(const float* E, int B, int N, int M, int D, const float* w, const float* b,
                                float eps_cos, float eps, int variant, float* loss, float* per_emb_loss, float* dE,
                                float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream) {
    return selftest_team_run(&Problem::test_abort, 1, true, E, B, N, M, D, w, b, eps_cos, eps, variant, loss, per_emb_loss, dE,
                             dw, db, workspace, workspace_bytes, stream);
}

// The abort word raised by one workgroup in the middle of the grid's finish (some leave, some stay)
int ge2e_selftest_team_abort_midgrid(const float* E, int B, int N, int M, int D, const float* w, const float* b,
                                     float eps_cos, float eps, int variant, float* loss, float* per_emb_loss, float* dE,
                                     float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream) {
    return selftest_team_run(&Problem::test_abort, 2, true, E, B, N, M, D, w, b, eps_cos, eps, variant, loss, per_emb_loss, dE,
                             dw, db, workspace, workspace_bytes, stream);
}

// At most `max_workgroups` workgroups (a multiple of 64: eight per XCD form one team): many batches through few teams, so
// that the hand-off counters of a team run far beyond what a full-size launch reaches.
int ge2e_selftest_team_grid(const float* E, int B, int N, int M, int D, const float* w, const float* b, float eps_cos,
                            float eps, int variant, float* loss, float* per_emb_loss, float* dE, float* dw, float* db,
                            void* workspace, size_t workspace_bytes, void* stream, int max_workgroups) {
    return selftest_team_run(&Problem::grid_cap, max_workgroups, max_workgroups >= 64, E, B, N, M, D, w, b, eps_cos, eps, variant,
                             loss, per_emb_loss, dE, dw, db, workspace, workspace_bytes, stream);
}

int ge2e_selftest_split_gemm(const float* A, const float* Bm, const float* G, float* X, float* GE, float* GC,
                             void* stream) {
    if (!A || !Bm || !G || !X || !GE || !GC) return GE2E_ERR_NULL;
    return (int)launch_selftest_split(A, Bm, G, X, GE, GC, (hipStream_t)stream);
}

int ge2e_selftest_wave_ops(const float* x, float* out, void* stream) {
    if (!x || !out) return GE2E_ERR_NULL;
    return (int)launch_selftest_wave(x, out, (hipStream_t)stream);
}

int ge2e_selftest_rows16(const float* CH, const float* R, float* XT, float* GE, float* GT, void* stream) {
    if (!CH || !R || !XT || !GE || !GT) return GE2E_ERR_NULL;
    return (int)launch_selftest_rows16(CH, R, XT, GE, GT, (hipStream_t)stream);
}

size_t ge2e_selftest_team_bytes(int payload_f4) { return payload_f4 > 0 ? selftest_team_bytes(payload_f4) : 0; }

int ge2e_selftest_team(void* ws, size_t ws_bytes, int grid, int rounds, int payload_f4, unsigned* out, void* stream) {
    if (!ws || !out) return GE2E_ERR_NULL;
    if (rounds < 1 || payload_f4 < 1) return GE2E_ERR_SHAPE;
    return (int)launch_selftest_team(ws, ws_bytes, grid, rounds, payload_f4, out, (hipStream_t)stream);
}

}  // extern "C"
