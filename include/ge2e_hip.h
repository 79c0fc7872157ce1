/*
 * ge2e_hip.h -- C ABI of libge2e_hip.so: the GE2E speaker-verification loss
 * (forward + full gradient) as hand-written HIP kernels for gfx950 (MI355X).
 *
 * This is the drop-in boundary for the hot path of
 * gkv856/speaker_embedding_GE2E_loss:
 *     embedding_model_GE2E/s3_loss_function_GE2E.py:19-30   GE2ELoss.forward
 *     embedding_model_GE2E/s3_loss_function_GE2E.py:34-127  get_centroids,
 *         get_cos_sim, get_utterance_centroids, calc_loss
 *     embedding_model_GE2E/s4_train_embed_model.py:200      loss.backward()
 * The reference has no native layer; these entry points are what a ctypes /
 * torch binding for that path binds (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - plain C types only; every pointer is a DEVICE pointer unless it says host;
 *   - all tensors are dense, row-major, float32;  E is [B][N][M][D]
 *     (B independent (speakers x utterances) batches, N speakers, M utterances
 *     per speaker, D embedding size); B = 1 is the reference's single batch;
 *   - the caller owns every buffer including the workspace; the library
 *     allocates nothing, keeps no state and never synchronises: calls only
 *     enqueue work on `stream` (a hipStream_t passed as void*, NULL = default);
 *   - a loss workspace (ge2e_workspace_bytes) begins with a 26 KB control block
 *     of the eight-CU team kernel, whichever implementation runs on it; the
 *     block cleans itself after every call (see ge2e_workspace_init);
 *   - w and b (s3:16-17) are read from device memory, no host sync;
 *   - return value: 0 = ok, < 0 = argument error (GE2E_ERR_*), > 0 = hipError_t
 *     of a failed launch.  Nothing is thrown across the boundary.
 */
#ifndef GE2E_HIP_H
#define GE2E_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GE2E_ABI_VERSION 2   /* 2: ge2e_workspace_init, the *_rows helpers; every loss workspace starts with the control block */

/* loss variants: eq. (6) softmax is the reference's (s3:115-127); eq. (7)
 * contrast is defined from arXiv:1710.10467 (absent from the reference). */
#define GE2E_VARIANT_SOFTMAX 0
#define GE2E_VARIANT_CONTRAST 1

/* kernel selection */
#define GE2E_IMPL_AUTO 0        /* fastest implementation valid for the shape   */
#define GE2E_IMPL_GENERIC 1     /* one workgroup per batch, fp32 VALU, any shape */
#define GE2E_IMPL_FUSED_F32 2   /* one workgroup per batch, LDS-resident centroids,
                                   exact-fp32 MFMA (v_mfma_f32_32x32x2_f32)      */
#define GE2E_IMPL_FUSED_SPLIT 3 /* as FUSED_F32 with fp16 hi+lo split operands on
                                   v_mfma_f32_32x32x16_f16, fp32 accumulate      */
#define GE2E_IMPL_TILED 4       /* many workgroups per batch (large N / D, small B); D any multiple of 8 up to 1024 */
#define GE2E_IMPL_TEAM 5        /* eight workgroups of one XCD per batch, the member's rows resident in LDS: E is
                                   read once.  ONE launch per call: if the teams cannot form or a hand-off times
                                   out, the same workgroups redo the call with FUSED_SPLIT's one-workgroup-per-batch
                                   body before the launch ends (see GE2E_IMPL_AUTO_NO_TEAM).  D: any multiple of 4
                                   up to 256 (padded to the next multiple of 64 inside the kernel)               */

#define GE2E_IMPL_WAVE 6        /* one WAVE per batch, the batch in registers, exact fp32, no workspace: the reference's
                                   own shapes (up to 64 rows: N <= 3..12 depending on M in {2,3,4,5,6,8,10,16},
                                   D <= 256, D % 4 == 0)                                                        */
#define GE2E_IMPL_AUTO_NO_TEAM 7 /* AUTO without GE2E_IMPL_TEAM: for callers that KNOW other streams or processes keep
                                   CUs busy while the loss runs (overlapped collectives, a shared GPU).  The team kernel
                                   wants its workgroups co-resident; it survives a busy device (waits bounded to a few
                                   milliseconds, then the in-launch redo), but not choosing it saves those waits.  */

#define GE2E_OK 0
#define GE2E_ERR_NULL (-1)      /* a required pointer is NULL                    */
#define GE2E_ERR_SHAPE (-2)     /* B,N,D < 1 or M < 2 (M = 1 divides by zero in
                                   the reference, s3:110-111)                    */
#define GE2E_ERR_WORKSPACE (-3) /* workspace NULL/too small/misaligned (256 B)   */
#define GE2E_ERR_VARIANT (-4)
#define GE2E_ERR_IMPL (-5)      /* requested impl cannot run this shape          */
#define GE2E_ERR_ALIGN (-6)     /* E / dE not 16-byte aligned                    */

int ge2e_abi_version(void);
const char* ge2e_strerror(int code);

/* Which implementation GE2E_IMPL_AUTO resolves to for a shape (or `impl`
 * itself if it is valid for the shape, GE2E_ERR_IMPL if not). */
int ge2e_resolve_impl(int B, int N, int M, int D, int variant, int impl);

/* Bytes of scratch ge2e_loss_fwd_bwd / ge2e_cos_sim need for this shape. */
size_t ge2e_workspace_bytes(int B, int N, int M, int D, int variant, int impl);

/* OPTIONAL, once per workspace allocation (enqueue-only, one 2-us launch): writes the clean control block GE2E_IMPL_TEAM
 * expects at the head of its workspace.  The block is self-cleaning -- every call hands it back the way it found it, so
 * the steady state has no zeroing launch in front of the kernel -- and a workspace that was NOT initialised (or that another
 * implementation has used in between) is still safe: the first call on it is computed without teams (one workgroup
 * per batch, inside the same launch), which leaves a clean block behind.  Calling this just makes the first call already run the team kernel.  Workspaces
 * smaller than the block (26 KB, the first bytes of every loss workspace whichever implementation runs) are left alone.  (The reference has no counterpart: s3's module allocates nothing.) */
int ge2e_workspace_init(void* workspace, size_t workspace_bytes, void* stream);

/*
 * GE2ELoss.forward + its autograd backward in one call (s3:19-30 + s4:200).
 *   loss          [B]        sum over the (N,M) per-utterance losses (s3:126)
 *   per_emb_loss  [B][N][M]  calc_loss()'s second return value, or NULL
 *   dE            [B][N][M][D] dLoss/dE, or NULL for forward only
 *   dw, db        [B]        dLoss/dw, dLoss/db (NULL allowed when dE is NULL)
 * eps_cos = F.cosine_similarity's eps (1e-8); eps = hp.general.small_err (1e-6).
 */
int ge2e_loss_fwd_bwd(const float* E, int B, int N, int M, int D,
                      const float* w, const float* b, float eps_cos, float eps,
                      int variant, int impl,
                      float* loss, float* per_emb_loss,
                      float* dE, float* dw, float* db,
                      void* workspace, size_t workspace_bytes, void* stream);

/*
 * The same in DOUBLE precision (the reference's forward is dtype-generic, s3:19-30: float64 embeddings are computed in
 * float64): every tensor, w, b and every result is float64, every operation of the kernel is fp64 (contractions on
 * v_mfma_f64_16x16x4_f64).  Any shape ge2e_loss_fwd_bwd takes, both variants, forward only with dE = NULL.  One kernel,
 * no implementation choice; deterministic.  The workspace is this entry point's own (ge2e_workspace_bytes_f64, 256-byte
 * aligned, no control block, no initialisation).  Same error codes, checked on the host before anything is launched.
 */
size_t ge2e_workspace_bytes_f64(int B, int N, int M, int D, int variant);
int ge2e_loss_fwd_bwd_f64(const double* E, int B, int N, int M, int D,
                          const double* w, const double* b, double eps_cos, double eps, int variant,
                          double* loss, double* per_emb_loss, double* dE, double* dw, double* db,
                          void* workspace, size_t workspace_bytes, void* stream);

/*
 * The RAGGED loss: every speaker has its own utterance count.  E [B][R][D] holds the rows of speaker j of batch bi
 * contiguously at offsets[bi][j] .. offsets[bi][j+1]-1; offsets [B][N+1] is int32 ON THE DEVICE.  The B batches share N
 * and R (a fixed row budget) and differ in their offsets.  Semantics: ge2e_loss_fwd_bwd's with M replaced by
 * m_j = offsets[j+1] - offsets[j] wherever it appears (centroid = mean of the speaker's m_j rows, leave-one-out centroid
 * = (sum_j - e_r) / (m_j - 1)); with all counts equal to M it is that loss.  per_row_loss [B][R] or NULL, dE [B][R][D] or
 * NULL for forward only.  fp32, exact (contractions on v_mfma_f32_16x16x4_f32), any N >= 1, D >= 1, R >= 2 N, both
 * variants; one kernel, no implementation choice; deterministic.  The workspace is this entry point's own
 * (ge2e_workspace_bytes_ragged, 256-byte aligned, no control block, no initialisation).  Same error codes, checked on
 * the host before anything is launched: GE2E_ERR_SHAPE for B, N, D < 1 or R < 2 N.
 * THE CALLER GUARANTEES THE OFFSETS' CONTENTS -- offsets[0] = 0, offsets[N] = R, every step >= 2 -- which cannot be
 * checked here without a synchronisation.  The kernel clamps every offset it reads into [0, R]: a table that breaks the
 * contract yields wrong or non-finite numbers, never an access outside the buffers (a step of 1 divides by zero, like
 * M = 1 in the reference).
 */
size_t ge2e_workspace_bytes_ragged(int B, int N, int R, int D, int variant);      /* 0 for a bad shape */
int ge2e_loss_fwd_bwd_ragged(const float* E, const int* offsets, int B, int N, int R, int D,
                             const float* w, const float* b, float eps_cos, float eps, int variant,
                             float* loss, float* per_row_loss, float* dE, float* dw, float* db,
                             void* workspace, size_t workspace_bytes, void* stream);

/*
 * The ragged loss FROM SPEAKER LABELS: the rows of E [B][R][D] come in any order and labels [B][R] (int32 ON THE DEVICE)
 * names the speaker of each, 0 .. N-1.  ge2e_label_index builds, per batch and without leaving the device,
 *   offsets [B][N+1]  offsets[j] = number of rows with a label < j          (offsets[0] = 0, offsets[N] = R)
 *   order   [B][R]    order[p] = the original row that stands at sorted position p; STABLE: the rows of one speaker keep
 *                     their original relative order, so order == numpy.argsort(labels, kind="stable")
 * (one 256-thread workgroup per batch: histogram, scan, stable placement; exact and the same bits every launch, for any
 * N >= 1 and R >= 1).  Its workspace, ge2e_label_index_workspace_bytes (256-byte aligned; 0 for few speakers, then it may
 * be NULL), needs no initialisation.
 * ge2e_loss_fwd_bwd_labeled computes ge2e_loss_fwd_bwd_ragged on the rows E[order[0]], E[order[1]], ... with those
 * offsets, gathering as it loads -- nothing is materialised in sorted order -- and returns per_row_loss [B][R] and
 * dE [B][R][D] in the CALLER'S row order (the same bits as the ragged entry on gathered rows, scattered back; with labels
 * already sorted it is the ragged entry).  per_row_loss or dE may be NULL (dE = NULL: forward only, dw / db may then be
 * NULL).  Two launches, the index kernel and the loss kernel; enqueue-only, deterministic, no allocation, no state.  Any
 * N >= 1, D >= 1, R >= 2 N, both variants.  The workspace is this entry point's own (ge2e_workspace_bytes_labeled,
 * 256-byte aligned, no control block, no initialisation): the ragged workspace, offsets and order of all B batches and
 * the index kernel's counters.  Same error codes, checked on the host before anything is launched, in the ragged
 * entry's order: GE2E_ERR_NULL, GE2E_ERR_SHAPE for B, N, D < 1 or R < 2 N, GE2E_ERR_VARIANT, GE2E_ERR_WORKSPACE,
 * GE2E_ERR_ALIGN.
 * THE CALLER GUARANTEES THE LABELS' CONTENTS -- every label in [0, N), every speaker at least 2 rows -- which cannot be
 * checked here without a synchronisation.  Every label is clamped into [0, N-1] where it is read, so order is a
 * permutation of 0..R-1 whatever the labels hold: labels that break the contract yield wrong or non-finite numbers, never
 * an access outside the buffers (a speaker with 1 row divides by zero, like M = 1 in the reference).
 */
size_t ge2e_label_index_workspace_bytes(int B, int N, int R);                     /* may be 0 */
int ge2e_label_index(const int* labels, int B, int N, int R, int* offsets, int* order,
                     void* workspace, size_t workspace_bytes, void* stream);
size_t ge2e_workspace_bytes_labeled(int B, int N, int R, int D, int variant);     /* 0 for a bad shape */
int ge2e_loss_fwd_bwd_labeled(const float* E, const int* labels, int B, int N, int R, int D,
                              const float* w, const float* b, float eps_cos, float eps, int variant,
                              float* loss, float* per_row_loss, float* dE, float* dw, float* db,
                              void* workspace, size_t workspace_bytes, void* stream);

/*
 * The labelled loss WITH MASKING: the labels' contents need no guarantee any more.  labels [B][R] (int32 on the device)
 * may hold anything and N is only an upper bound of the speaker ids (the data set's speaker count works).  Per batch,
 * decided on the device without a synchronisation:
 *   valid row       0 <= labels[r] < N (nothing is clamped); every other row is ignored -- e.g. padding labelled -1
 *   active speaker  at least 2 valid rows carry its label; a speaker with 1 row (no leave-one-out centroid) or none is
 *                   left out, rows and centroid alike
 *   active row      valid, and its speaker is active; n_act / r_act count the active speakers / rows
 * ge2e_label_index_masked writes (any N >= 1 and R >= 1, N may be far above R):
 *   order    [B][R]    order[0 .. r_act) = the active rows sorted by (label, original index), then every other row in
 *                      ascending original index: always a permutation of 0..R-1, and
 *                      numpy.argsort(numpy.where(active_row, labels, N), kind="stable")
 *   offsets  [B][N+1]  offsets[k] = number of active rows of the active speakers before the k-th one (ascending label),
 *                      k <= n_act; offsets[k] = r_act for n_act < k <= N
 *   speakers [B][N]    speakers[k] = the label of the k-th active speaker, k < n_act; -1 beyond
 *   active   [B][2]    {n_act, r_act}
 * with the same bits every launch and at every position of the stack.  Its workspace
 * (ge2e_label_index_masked_workspace_bytes) follows ge2e_label_index's rule.
 * ge2e_loss_fwd_bwd_labeled_masked computes ge2e_loss_fwd_bwd_ragged of the n_act active speakers on the rows
 * E[order[0 .. r_act)] with offsets[0 .. n_act] -- the ragged entry's bits on that compacted batch; with every row
 * active and n_act = N the bits of ge2e_loss_fwd_bwd_labeled -- and returns per_row_loss [B][R] and dE [B][R][D] in the
 * CALLER'S row order, WRITTEN AS 0 FOR EVERY ROW THAT IS NOT ACTIVE.  Such rows of E are never read: they may hold NaN.
 * A batch without active speakers has loss = dw = db = 0 and all of dE and per_row_loss 0.  active [B][2] receives
 * {n_act, r_act} (NULL: not wanted); the other arguments are ge2e_loss_fwd_bwd_labeled's.  B, N, R, D >= 1 (R >= 2 N is
 * NOT required: N is a bound), both variants.  The workspace is this entry point's own
 * (ge2e_workspace_bytes_labeled_masked, 256-byte aligned, no control block, no initialisation, and the result does not
 * depend on what it held): the ragged slices -- laid out for max(1, min(N, R / 2)) speakers, all that R rows can hold --
 * offsets, order, speakers and active of all B batches, and the index kernel's counters.  Same error codes, checked on
 * the host before anything is launched, in the labelled entry's order.  Two launches, enqueue-only, no allocation, no
 * state: a fixed row budget R with padding rows makes a batch of varying size a static-shape call, fit for a HIP graph.
 */
size_t ge2e_label_index_masked_workspace_bytes(int B, int N, int R);              /* may be 0 */
int ge2e_label_index_masked(const int* labels, int B, int N, int R, int* offsets, int* order, int* speakers, int* active,
                            void* workspace, size_t workspace_bytes, void* stream);
size_t ge2e_workspace_bytes_labeled_masked(int B, int N, int R, int D, int variant);   /* 0 for a bad shape */
int ge2e_loss_fwd_bwd_labeled_masked(const float* E, const int* labels, int B, int N, int R, int D,
                                     const float* w, const float* b, float eps_cos, float eps, int variant,
                                     float* loss, float* per_row_loss, float* dE, float* dw, float* db, int* active,
                                     void* workspace, size_t workspace_bytes, void* stream);

/*
 * The masked labelled loss on MANY WORKGROUPS PER BATCH: the wide route.  Arguments, semantics, error codes and the order
 * of the host checks are ge2e_loss_fwd_bwd_labeled_masked's: a row is valid iff 0 <= label < N, a speaker active iff at
 * least 2 valid rows carry its label, the loss is the ragged loss of the n_act active speakers on the r_act active rows,
 * per_row_loss and dE come back in the caller's row order and are written as 0 on every row that does not count, such rows
 * are never read, n_act = 0 gives zeros everywhere, dE = NULL is forward only; both variants, any B, N, R, D >= 1.
 * What differs is the work decomposition: behind the index kernel come the centroids (one wave per speaker), the rows
 * (one workgroup per 64 sorted rows), the final sums and, with dE, GC, the speakers and dE, each on many workgroups --
 * 7 launches with a gradient, 4 without, one linear chain, enqueue-only, no allocation, no state, no synchronisation,
 * grids sized from the shapes alone: fit for a HIP graph.  The low bits are therefore NOT the masked entry's; the result
 * has the same bits on every launch, at every position of the stack and whatever the workspace held.
 * Workspace (ge2e_workspace_bytes_labeled_wide; 256-byte aligned parts, no control block, no initialisation), with
 * NA = max(1, min(N, R / 2)), NAp = NA rounded up to a multiple of 4, S = min(8, ceil(R / 128)) pieces of GC's K loop:
 *   4 B (  4 NA D           CH, SS, GC, DUS
 *        + S NA D           GC's pieces (S > 1 only)
 *        + 4 NA             CST
 *        + R NAp            A
 *        + 8 R + R          row statistics, spk
 *        + 4 ceil(R / 64) ) tile partials
 *   + offsets, order, speakers, active of all B batches + the index kernel's counters, every part rounded up to 256 bytes.
 * It GROWS WITH B -- 164 KB of A per batch at R = 640, N = 64: the route is meant for few, large batches.  The masked
 * entry, one workgroup per batch, remains the choice when B fills the chip; nothing picks between the two.
 */
size_t ge2e_workspace_bytes_labeled_wide(int B, int N, int R, int D, int variant);   /* 0 for a bad shape */
int ge2e_loss_fwd_bwd_labeled_wide(const float* E, const int* labels, int B, int N, int R, int D,
                                   const float* w, const float* b, float eps_cos, float eps, int variant,
                                   float* loss, float* per_row_loss, float* dE, float* dw, float* db, int* active,
                                   void* workspace, size_t workspace_bytes, void* stream);

/*
 * LABELLED EVALUATION: the cosines (and the EER counts) of the masked labelled loss, forward only, for rows in any order.
 * Semantics per batch: ge2e_loss_fwd_bwd_labeled_masked's -- a row is valid iff 0 <= label < N, a speaker active iff at
 * least 2 valid rows carry its label, a row active iff it is valid and its speaker is active; the active speakers get the
 * compact ids 0 .. n_act-1 by ascending label (ge2e_label_index_masked's speakers / active).  For an active row r of
 * compact speaker j and k < n_act:
 *   cos[r][k] = cossim(e_r, c_k) + eps  (k != j),   cos[r][j] = cossim(e_r, (sum_j - e_r) / (m_j - 1)) + eps
 * with c_k the mean of speaker k's active rows and F.cosine_similarity's eps_cos clamp.  Outputs, in the CALLER'S row order:
 *   cos      [B][R][N]  column k = compact speaker k; WRITTEN AS 0 on every row that is not active and on every column
 *                       k >= n_act: every element is written.  NULL: the matrix is never materialised (counts only)
 *   col      [B][R]     the row's own column (its compact speaker id), -1 for a row that is not active; or NULL
 *   speakers [B][N], active [B][2]   as ge2e_label_index_masked writes them; or NULL
 *   counts   [B][T][2]  the calculate_ERR sweep (s5_eval_model.py:57-98 with w = 1, b = 0, s5:44) on cos itself, over the
 *                       active rows and the columns < n_act:  [t][0] = #{(r,k), k != col[r] : cos[r][k] > thr[t]},
 *                       [t][1] = #{r : cos[r][col[r]] > thr[t]}.  fp32 strict `>`, NaN accepts nothing; thresholds
 *                       non-decreasing, T <= 4096, as for ge2e_eer_counts.  NULL (with thresholds NULL / T = 0): no counts
 * At least one of cos and counts must be given.  Rows that are not active are never read: they may hold NaN.  n_act = 0:
 * all of cos and counts 0.  Three launches (the index kernel, one wave per speaker for the centroids, one workgroup per
 * 64 rows for the cosines: a single batch spreads over the chip), enqueue-only, no allocation, no state, static shapes:
 * fit for a HIP graph.  The counts are accumulated with integer atomics only: the same bits every launch.  The
 * workspace is this entry's own (ge2e_cos_sim_labeled_workspace_bytes, 256-byte aligned, per batch: centroids and sums for
 * max(1, min(N, R / 2)) speakers, the index tables, the index kernel's counters; no control block, no initialisation, and
 * the result does not depend on what it held).  Checked on the host before anything is launched, in this order:
 * GE2E_ERR_NULL (E, labels, or both cos and counts NULL), GE2E_ERR_SHAPE (B, N, R, D < 1, T < 0, T > 4096, counts without
 * thresholds or with T = 0), GE2E_ERR_WORKSPACE, GE2E_ERR_ALIGN (E not 16-byte aligned).
 * ge2e_eer_counts_labeled: the same count on a CALLER-MADE sim [B][R][N] (e.g. w cos + b) with the col and active the
 * first call returned; columns >= n_act and rows with col < 0 are never read.  Two launches (zeroing, counting).
 */
size_t ge2e_cos_sim_labeled_workspace_bytes(int B, int N, int R, int D);   /* 0 for a bad shape */
int ge2e_cos_sim_labeled(const float* E, const int* labels, int B, int N, int R, int D,
                         float eps_cos, float eps,
                         const float* thresholds, int T,       /* NULL / 0: no counts */
                         float* cos,      /* [B][R][N] or NULL */
                         int* col,        /* [B][R]    or NULL */
                         int* speakers,   /* [B][N]    or NULL */
                         int* active,     /* [B][2]    or NULL */
                         int* counts,     /* [B][T][2] or NULL */
                         void* workspace, size_t workspace_bytes, void* stream);

int ge2e_eer_counts_labeled(const float* sim, const int* col, const int* active,
                            int B, int N, int R,
                            const float* thresholds, int T, int* counts, void* stream);

/*
 * DIFFERENTIABLE LABELLED HELPERS: the backward of ge2e_cos_sim_labeled's cosines, and the labelled counterpart of
 * ge2e_calc_loss / ge2e_calc_loss_bwd, so that a caller can put a head of its own between the two (the reference's
 * get_cos_sim / calc_loss recombined, for rows in any order).
 *
 * ge2e_cos_sim_labeled_bwd.  Semantics are ge2e_cos_sim_labeled's (valid row, active speaker, active row, compact columns
 * by ascending label).  g_cos [B][R][N] is dL/dcos in the layout cos was returned in: the caller's row order, column k =
 * compact speaker k.  dE [B][R][D] is dL/dE through all three paths of cos: the row's own normalisation; the other
 * speakers' centroids, into every row of those speakers; the leave-one-out centroid on the own column, into the speaker's
 * other rows.  The eps_cos clamps of F.cosine_similarity act as in the wide loss (the `+ eps` of cos is a constant and has
 * no gradient).  dE comes back in the caller's row order, EVERY element is written, and it is 0 on every row that is not
 * active.  Rows of E and g_cos that are not active and columns >= n_act of g_cos are never read: they may hold NaN.
 * n_act = 0: dE all zero.  active [B][2] as ge2e_label_index_masked writes it, or NULL.
 * The call is stateless: it runs the masked index kernel and the centroid kernel again from E and labels and recomputes
 * the cosines it needs; it does not take the forward's cos.  Six launches, one linear chain -- index, centroids, the
 * cos-grad rows kernel (one workgroup per 64 sorted rows: row statistics, the cosines on the matrix core, g_cos into the
 * wide route's A / row statistics), then the wide loss's own GC, speakers and dE kernels -- enqueue-only, no allocation,
 * no synchronisation, grids sized from the shapes alone: fit for a HIP graph.  No atomics; every sum has an order fixed
 * by the shapes and the batch's labels: the same bits on every launch, at every position of the stack, whatever the
 * workspace held.  Workspace (ge2e_cos_sim_labeled_bwd_workspace_bytes, 256-byte aligned, no initialisation): the wide
 * entry's layout without the tile partials.  Checked on the host before anything is launched, in this order:
 * GE2E_ERR_NULL (E, labels, g_cos or dE), GE2E_ERR_SHAPE (B, N, R, D < 1), GE2E_ERR_WORKSPACE, GE2E_ERR_ALIGN (E or dE not
 * 16-byte aligned; g_cos needs float alignment only).
 *
 * ge2e_calc_loss_labeled / _bwd, on a CALLER-MADE sim [B][R][N] (e.g. w cos + b) with the col [B][R] and active [B][2] that
 * ge2e_cos_sim_labeled returned.  A row counts iff 0 <= col[r] < n_act, n_act = clamp(active[0], 0, N); only the columns
 * < n_act of a counting row are read.  With j = col[r]:
 *   softmax   per_r = -sim[r][j] + log(sum_{k < n_act} exp sim[r][k] + eps)
 *   contrast  per_r = 1 - sigmoid(sim[r][j]) + max_{k != j, k < n_act} sigmoid(sim[r][k])   (the max is 0 when n_act = 1;
 *             ties go to the lowest index)
 * in the stabilised arithmetic of the loss kernels.  per_row_loss [B][R] (required) is 0 on rows that do not count;
 * loss [B] (or NULL) is the batch's sum of per_row_loss in a fixed order (a second small launch).
 * d_sim[r][k] = (g_loss[b] + g_per[b][r]) d per_r / d sim[r][k], a NULL gradient counting as 0; EVERY element of d_sim is
 * written: 0 on rows that do not count and on columns >= n_act.  No workspace.  Checks: GE2E_ERR_NULL (sim, col, active,
 * per_row_loss / d_sim), GE2E_ERR_SHAPE (B, N, R < 1), GE2E_ERR_VARIANT.
 */
size_t ge2e_cos_sim_labeled_bwd_workspace_bytes(int B, int N, int R, int D);   /* 0 for a bad shape */
int ge2e_cos_sim_labeled_bwd(const float* E, const int* labels, const float* g_cos,
                             int B, int N, int R, int D, float eps_cos,
                             float* dE, int* active /* [B][2] or NULL */,
                             void* workspace, size_t workspace_bytes, void* stream);
int ge2e_calc_loss_labeled(const float* sim, const int* col, const int* active, int B, int N, int R,
                           float eps, int variant,
                           float* loss /* [B] or NULL */, float* per_row_loss /* [B][R], required */, void* stream);
int ge2e_calc_loss_labeled_bwd(const float* sim, const int* col, const int* active, int B, int N, int R,
                               float eps, int variant,
                               const float* g_loss /* [B] or NULL */, const float* g_per /* [B][R] or NULL */,
                               float* d_sim /* [B][R][N] */, void* stream);

/*
 * ENROLMENT AND VERIFICATION: a speaker bank filled from one set of rows, and other rows scored against it.  Every cosine
 * above is the training-time similarity: the centroids come from the very rows that are scored and the own column is the
 * leave-one-out centroid.  A held-out trial row is no part of the model it is compared with: nothing here leaves one out.
 * A BANK is two caller-owned device buffers for the speaker ids 0 .. K-1, sums [K][D] float32 and cnt [K] int32, zeroed
 * once by the caller.  Rows are taken as given (the encoder's output is L2-normalised, s2:34; nothing is normalised on the
 * way in).  No batch dimension.
 *
 * ge2e_enroll_accumulate.  E [R][D], labels [R] int32, rows in any order, labels of ANY content.  A row is valid iff
 * 0 <= label < K; every other row is ignored and never read: it may hold NaN.  For a speaker s with m >= 1 valid rows in
 * this call (ONE row enrols: not the masked loss's "at least 2") the partial sum starts from 0 and adds the speaker's rows
 * in ascending row index; then, once, sums[s] = sums[s] + partial and cnt[s] += m.  A speaker without a valid row in this
 * call is not touched: its sums row keeps its bits, whatever they are.  Two launches: the masked index kernel with the
 * activity threshold 1, then one wave per active speaker (up to min(K, R) of them).  Exactly one wave touches a speaker per
 * launch, no floating-point atomics, every sum has a fixed order: the same bits on every launch, and the same for every
 * row order that keeps each speaker's own rows in their order.  Workspace (ge2e_enroll_workspace_bytes, 256-byte aligned):
 * the index tables of one batch -- offsets [K+1], order [R], speakers [K], active [2] -- and, above 1024 speakers, the
 * index kernel's K counters, each part 256-byte aligned; no initialisation, and the result does not depend on what it held.
 * Checked on the host before anything is launched, in this order: GE2E_ERR_NULL (E, labels, sums or cnt), GE2E_ERR_SHAPE
 * (K, R or D < 1), GE2E_ERR_WORKSPACE, GE2E_ERR_ALIGN (E or sums not 16-byte aligned).
 *
 * ge2e_enroll_finalize.  models [K][D]: for cnt[s] > 0 the unit centroid c / max(|c|, eps_cos), c = sums[s] / cnt[s], in
 * the centroid kernels' arithmetic; for cnt[s] <= 0 the row is written as +0 and sums[s] is never read.  EVERY element is
 * written.  One launch (one wave per speaker), no workspace.  Checks: GE2E_ERR_NULL (sums, cnt or models), GE2E_ERR_SHAPE
 * (K or D < 1).
 *
 * ge2e_verify_scores.  E [R][D] the trial rows, models [K][D] and cnt [K] as above.  A speaker k is ENROLLED iff cnt[k] > 0.
 * labels NULL: every row is scored; scores is required, counts and trials must be NULL.  With labels [R]: a row with
 * label < 0 is ignored (never read: it may hold NaN; its score row is +0), every other row is scored, and its TARGET is
 * `label` if label < K and that speaker is enrolled; otherwise it has none (an unknown speaker: an impostor against
 * everybody).  Outputs:
 *   scores [R][K]   (e_r . models[k]) / max(|e_r|, eps_cos) + eps for an enrolled k, +0 for any other: every element is
 *                   written.  NULL: the matrix is never materialised (counts only)
 *   counts [T][2]   [t][0] = #{(r, k) : r scored, k enrolled, k != target(r), scores[r][k] > thr[t]},
 *                   [t][1] = #{r : r has a target, scores[r][target(r)] > thr[t]}.  fp32 strict `>`, NaN accepts nothing;
 *                   thresholds non-decreasing, T <= 4096, as for ge2e_eer_counts.  Or NULL
 *   trials [2]      {impostor scores counted, target scores counted}: the denominators of FAR and FRR, tallied where
 *                   the values are binned, NaN included.  Or NULL
 * A zeroing launch when counts or trials are wanted, then one rows kernel (one workgroup per 64 rows in the caller's
 * order; exact fp32 on the matrix core; every wave streams the model tiles from L2).  No workspace, enqueue-only, static shapes: fit for a HIP
 * graph.  Integer atomics only: the same bits every launch, and a row's scores do not depend on where it stands in E.
 * Checked on the host before anything is launched, in this order: GE2E_ERR_NULL (E, models or cnt NULL; both scores and
 * counts NULL; counts or trials without labels), GE2E_ERR_SHAPE (K, R or D < 1; T < 0 or T > 4096; counts without
 * thresholds or with T = 0; counts or trials with R * K > 2^31 - 1), GE2E_ERR_ALIGN (E or models not 16-byte aligned).
 */
size_t ge2e_enroll_workspace_bytes(int K, int R, int D);   /* 0 for a bad shape */
int ge2e_enroll_accumulate(const float* E, const int* labels, int K, int R, int D,
                           float* sums /* [K][D] */, int* cnt /* [K] */,
                           void* workspace, size_t workspace_bytes, void* stream);
int ge2e_enroll_finalize(const float* sums, const int* cnt, int K, int D, float eps_cos,
                         float* models /* [K][D] */, void* stream);
int ge2e_verify_scores(const float* E, const int* labels /* [R] or NULL */, const float* models, const int* cnt,
                       int K, int R, int D, float eps_cos, float eps,
                       const float* thresholds, int T,       /* NULL / 0: no counts */
                       float* scores,   /* [R][K] or NULL */
                       int* counts,     /* [T][2] or NULL */
                       int* trials,     /* [2]    or NULL */
                       void* stream);

/*
 * SPEAKER IDENTIFICATION (csrc/ge2e_identify.hip): "who is this row?" -- the best k_top enrolled speakers of every trial
 * row, without the score matrix [R][K] ever being materialised.  Inputs as for ge2e_verify_scores: E [R][D] the trial rows,
 * models [K][D] and cnt [K] (speaker k is ENROLLED iff cnt[k] > 0), optional labels [R] int32, and k_top with
 * 1 <= k_top <= GE2E_IDENTIFY_MAX_TOP.
 * Which rows are scored, and their targets: without labels every row is scored and no row has a target.  With labels a row
 * with label < 0 is ignored: it is never read and may hold NaN.  Every other row is scored; its TARGET is `label` if
 * label < K and that speaker is enrolled; otherwise it has none.
 * The score of (r, k) for an enrolled k is ge2e_verify_scores' score, (e_r . models[k]) / max(|e_r|, eps_cos) + eps, with
 * the same bits (the same fmaf chain).  A speaker that is not enrolled is never a candidate.
 * The order of candidates is total: candidate a stands before b iff score_a > score_b as fp32 values; -0 and +0 are equal;
 * a NaN score stands behind every number; where the scores are equal, or both NaN, the lower speaker index stands first.
 * Outputs:
 *   idx [R][k_top]    int32, required: the first k_top candidates of the row in that order.  Positions past the number of
 *                     enrolled speakers hold -1; ignored rows hold all -1.  Every element is written
 *   score [R][k_top]  float32 or NULL: the candidates' scores; -inf wherever idx is -1.  Every element is written.  (A
 *                     NaN score comes back as the quiet NaN 0x7fc00000 and a -0 score as +0.)
 *   rank [R]          int32 or NULL (needs labels): the target's position 0 .. k_top-1 in the row's list, k_top when the
 *                     row has a target that is not in the list, -1 for a row without target and for an ignored row
 *   hist [k_top + 1]  int32 or NULL (needs labels): hist[j] = number of rows whose rank is j, hist[k_top] = rows whose
 *                     target is outside the list; its sum is the number of rows with a target.  Integer atomics only
 * The result is a function of the inputs alone: the same bits on every launch and whatever the workspace held, and it does
 * not depend on how the bank axis was split.
 * Launches: [a zeroing launch for hist,] the rows kernel -- one workgroup per (64 trial rows, slice of the bank); the number
 * of slices S = clamp(ceil(W / ceil(R / 64)), 1, ceil(K / 64)) is a function of (K, R) alone, W = 512, a slice being
 * ceil(ceil(K / 64) / S) groups of 64 speakers -- and the merge kernel, one wave per row.  Enqueue-only, no allocation, no
 * state, grids from the shapes alone: fit for a HIP graph.  Workspace (ge2e_identify_workspace_bytes, 256-byte aligned):
 * the rows' partial lists [S][R][k_top] of 8 bytes and nothing else; no initialisation.
 * Checked on the host before anything is launched, in this order: GE2E_ERR_NULL (E, models, cnt or idx NULL; rank or hist
 * without labels), GE2E_ERR_SHAPE (K, R or D < 1; k_top < 1 or > GE2E_IDENTIFY_MAX_TOP), GE2E_ERR_WORKSPACE (NULL, too
 * small, or not 256-byte aligned), GE2E_ERR_ALIGN (E or models not 16-byte aligned).
 */
#define GE2E_IDENTIFY_MAX_TOP 32
size_t ge2e_identify_workspace_bytes(int K, int R, int D, int k_top);     /* 0 for a bad shape */
int ge2e_identify(const float* E, const int* labels /* [R] or NULL */, const float* models, const int* cnt,
                  int K, int R, int D, int k_top, float eps_cos, float eps,
                  int* idx /* [R][k_top] */, float* score /* [R][k_top] or NULL */,
                  int* rank /* [R] or NULL */, int* hist /* [k_top+1] or NULL */,
                  void* workspace, size_t workspace_bytes, void* stream);

/*
 * ADAPTIVE SCORE NORMALISATION, AS-norm (csrc/ge2e_snorm.hip): verification scores normalised with statistics of the
 * enrolment model and of the trial row, each taken against a COHORT of impostor models.  A cohort is a bank's finalised
 * form: cohort [C][D] float32 and ccnt [C] int32, 1 <= C <= GE2E_COHORT_MAX; cohort speaker c is a MEMBER iff ccnt[c] > 0,
 * and the model row of a non-member is never used: it may hold NaN.  The score of (row x, member c) is ge2e_verify_scores'
 * score, (x . cohort[c]) / max(|x|, eps_cos) + eps, with the same bits.
 *
 * ge2e_cohort_stats.  X [R][D]; sel [R] int32 or NULL with sel_min: a row is SCORED iff sel == NULL or sel[r] >= sel_min
 * (trial rows pass (labels, 0), a bank's own models pass (cnt, 1)).  A row that is not scored is never read and gets
 * {+0, 1}.  n = min(n_top, number of members); for n = 0 the row gets {+0, 1} as well, with which normalising is the
 * identity.  Otherwise the n largest member scores are taken, in ge2e_identify's order (fp32 `>`, -0 equal to +0, a NaN
 * behind every number).  Only the MULTISET of those n values matters -- with v the n-th largest value: every score > v and
 * n - #{> v} copies of v -- so ties at the boundary need no index rule.
 *   stats [R][2]   {mean, max(std, eps_std)}: mean = sum / n; std the population one (ddof = 0), two-pass, from the
 *                  deviations from that mean.  A NaN among the n gives NaN for both.  Every element is written
 * Launches: per chunk of chunk_rows(C) rows -- a multiple of 64 and a function of C alone, floor(32 MiB / (4 C)) rounded
 * down to 64 rows and at least 64 -- a rows kernel (the verify rows kernel's shape, the cohort axis split over workgroups as
 * ge2e_identify splits its bank -- a function of C and the chunk's rows alone; the chunk's scores go into the workspace
 * as 32-bit keys, [chunk][C]) and a select kernel (one workgroup per row: an exact radix selection of the n-th largest key,
 * then the sum and the deviations in a fixed order).  The matrix [R][C] is never materialised.  Enqueue-only, no allocation,
 * no state, no synchronisation, grids from the shapes alone: fit for a HIP graph.  LDS integer atomics only, every sum in
 * an order fixed by the shapes: the same bits on every launch and whatever the workspace held, a row's statistics do not
 * depend on where it stands in X, and the chunking does not change them.  Workspace (ge2e_cohort_stats_workspace_bytes,
 * 256-byte aligned): the keys of one chunk, min(chunk_rows(C), R rounded up to 64) x C x 4 bytes -- at most 32 MiB plus
 * rounding whatever R is; no initialisation.
 * Checked on the host before anything is launched, in this order: GE2E_ERR_NULL (X, cohort, ccnt or stats), GE2E_ERR_SHAPE
 * (C < 1 or > GE2E_COHORT_MAX; R, D or n_top < 1), GE2E_ERR_WORKSPACE (NULL, too small, or not 256-byte aligned),
 * GE2E_ERR_ALIGN (X or cohort not 16-byte aligned).
 *
 * ge2e_verify_scores_normed.  ge2e_verify_scores with row_stats [R][2] and model_stats [K][2] ({mean, spread}, as
 * ge2e_cohort_stats writes them): the same rules for which rows are scored, their targets, +0 on ignored rows and on
 * columns that are not enrolled, counts, trials.  The statistics of an ignored row and of a speaker that is not enrolled
 * are never read and may hold NaN.  With v the verify score of (r, k),
 *   out = 0.5f * ( fl(fl(v - mu_k) * fl(1 / sd_k)) + fl(fl(v - mu_r) * fl(1 / sd_r)) ),
 * every operation rounded on its own in fp32, the reciprocal correctly rounded, nothing contracted into an fma.  counts are
 * taken on `out` (fp32 strict `>`; a NaN accepts nothing and is still tallied in trials).  Nothing is clamped here:
 * ge2e_cohort_stats did.  With both tables {0, 1} the output has ge2e_verify_scores' bits.  A zeroing launch when counts
 * or trials are wanted, then one rows kernel (streamed form); no workspace; fit for a HIP graph.
 * Checks, in this order: GE2E_ERR_NULL (E, models, cnt, row_stats or model_stats NULL; both scores and counts NULL; counts
 * or trials without labels), GE2E_ERR_SHAPE and GE2E_ERR_ALIGN as for ge2e_verify_scores.
 */
#define GE2E_COHORT_MAX 65536
size_t ge2e_cohort_stats_workspace_bytes(int C, int R, int D, int n_top);   /* 0 for a bad shape */
int ge2e_cohort_stats(const float* X, const int* sel /* [R] or NULL */, int sel_min, const float* cohort, const int* ccnt,
                      int C, int R, int D, int n_top, float eps_cos, float eps, float eps_std,
                      float* stats /* [R][2] */, void* workspace, size_t workspace_bytes, void* stream);
int ge2e_verify_scores_normed(const float* E, const int* labels /* [R] or NULL */, const float* models, const int* cnt,
                              int K, int R, int D, float eps_cos, float eps,
                              const float* row_stats /* [R][2] */, const float* model_stats /* [K][2] */,
                              const float* thresholds, int T,       /* NULL / 0: no counts */
                              float* scores,   /* [R][K] or NULL */
                              int* counts,     /* [T][2] or NULL */
                              int* trials,     /* [2]    or NULL */
                              void* stream);

/*
 * The same, fed with the encoder's RAW output (s2_model_GE2E_loss_speach_embed.py:34 +
 * s4_train_embed_model.py:186-192 folded into the loss kernel's load and store stages):
 *   Y   [B][N*M][D]  the encoder's projection BEFORE its L2-normalisation, rows in the encoder's own (permuted) order
 *   src [B][N*M] int32 or NULL: row r of the (N,M,D) block is Y[src[r]] / |Y[src[r]]|  (the reference's `unperm`; NULL =
 *       identity).  Each batch's src must be a permutation of 0..N*M-1.
 *   dY  [B][N*M][D]  dLoss/dY, through the normalisation's backward (g - e (e . g)) / |y|, in Y's row order; or NULL.
 * One launch instead of normalise + gather, loss, and the normalisation's backward + scatter; no (N,M,D) intermediate.
 * Shapes: ge2e_raw_supported(N, M, D) != 0 (the one-wave-per-batch kernel's register-only shapes: the reference's training
 * shapes N=2 M=16, N=4 M=5, ...); otherwise GE2E_ERR_IMPL and the caller uses ge2e_normalize_unperm + ge2e_loss_fwd_bwd.
 */
int ge2e_raw_supported(int N, int M, int D);
int ge2e_loss_fwd_bwd_raw(const float* Y, const int* src, int B, int N, int M, int D,
                          const float* w, const float* b, float eps_cos, float eps, int variant,
                          float* loss, float* per_emb_loss, float* dY, float* dw, float* db, void* stream);

/* GE2ELoss.get_cos_sim (s3:42-80): cos [B][N][M][N], leave-one-out centroid on
 * the own-speaker column, eps added to every entry.  Forward-only consumer:
 * s5_eval_model.py:42-44.
 * Workspace: ge2e_cos_sim_workspace_bytes(B, N, M, D).  With it, shapes the tiled kernel takes (N >= 16, D % 64 == 0) run
 * the N x (N M) x D contraction on the matrix cores (split-fp16 x3, fp32 accumulate: cosines to ~1e-6); with the smaller
 * ge2e_workspace_bytes(.., GE2E_IMPL_GENERIC) of ABI 1's rule, or any other shape, the exact-fp32 VALU kernel runs. */
size_t ge2e_cos_sim_workspace_bytes(int B, int N, int M, int D);
int ge2e_cos_sim(const float* E, int B, int N, int M, int D,
                 float eps_cos, float eps, float* cos,
                 void* workspace, size_t workspace_bytes, void* stream);

/* GE2ELoss.calc_loss (s3:115-127) on a caller-made similarity matrix
 * sim [B][N][M][N]:  loss [B], per_emb_loss [B][N][M] (or NULL).  Forward only. */
int ge2e_calc_loss(const float* sim, int B, int N, int M, float eps, int variant,
                   float* loss, float* per_emb_loss, void* stream);

/* GE2ELoss.get_cos_sim(embeddings, centroids, hp) (s3:42-80) with the CALLER'S centroids C [B][N][D]: other-speaker
 * columns use C, the own-speaker column the leave-one-out centroid of E; + eps on every entry.  cos [B][N][M][N].
 * (ge2e_cos_sim above is the special case C = get_centroids(E), the only one the reference's callers use.) */
int ge2e_cos_sim_centroids(const float* E, const float* C, int B, int N, int M, int D, float eps_cos,
                           float eps, float* cos, void* stream);

/* GE2ELoss.get_centroids (s3:34-38): cent [B][N][D] = mean over M. */
int ge2e_centroids(const float* E, int B, int N, int M, int D, float* cent, void* stream);

/* GE2ELoss.get_utterance_centroids (s3:95-112): U [B][N][M][D], u_ji = (sum_i' e_ji' - e_ji) / (M - 1).  The map is
 * linear and symmetric, so its backward is the same call on the incoming gradient. */
int ge2e_utterance_centroids(const float* E, int B, int N, int M, int D, float* U, void* stream);

/* ---- backward passes of the static helpers (the reference's are plain autograd code: s3:33-38, 41-80, 114-127) ----
 * get_centroids:  dE [B][N][M][D] = g_cent [B][N][D] / M */
int ge2e_centroids_bwd(const float* g_cent, int B, int N, int M, int D, float* dE, void* stream);
/* get_cos_sim(E, C): from the forward result `cos` and its incoming gradient g_cos (both [B][N][M][N]) the gradients
 * with respect to the embeddings, dE [B][N][M][D] (a-slot + leave-one-out slot), and to the caller's centroids,
 * dC [B][N][D].  Scratch: ge2e_cos_sim_bwd_workspace_bytes, 16-byte aligned. */
size_t ge2e_cos_sim_bwd_workspace_bytes(int B, int N, int M, int D);
int ge2e_cos_sim_bwd(const float* E, const float* C, const float* cos, const float* g_cos, int B, int N, int M, int D,
                     float eps_cos, float eps, float* dE, float* dC, void* workspace, size_t workspace_bytes,
                     void* stream);
/* calc_loss(sim): d_sim [B][N][M][N] from g_loss [B] (gradient of the summed loss, or NULL) and g_per [B][N][M]
 * (gradient of per_embedding_loss, or NULL). */
int ge2e_calc_loss_bwd(const float* sim, int B, int N, int M, float eps, int variant, const float* g_loss,
                       const float* g_per, float* d_sim, void* stream);

/*
 * The static helpers on LOCAL ROWS -- the speaker-sharded exact loss: a rank holds the rows of the n
 * speakers j0 .. j0 + n - 1 of a batch of N speakers and has gathered all N centroids.  Same semantics as
 * get_cos_sim(embeddings, centroids) (s3:42-80: the caller's centroids on every other-speaker column, the leave-one-out
 * centroid of the LOCAL rows on the own column j0 + jl) and calc_loss (s3:114-127), restricted to those rows:
 *   E   [B][n][M][D]   C [B][N][D]   cos / sim / g_cos / d_sim [B][n][M][N]   loss [B]   per_emb_loss [B][n][M]
 *   dE  [B][n][M][D]   dC [B][N][D] = this shard's PARTIAL centroid gradient (summed over the shards by the caller)
 * n = N, j0 = 0 is exactly ge2e_cos_sim_centroids / ge2e_cos_sim_bwd / ge2e_calc_loss / ge2e_calc_loss_bwd.
 */
int ge2e_cos_sim_rows(const float* E, const float* C, int B, int n, int N, int j0, int M, int D, float eps_cos, float eps,
                      float* cos, void* stream);
size_t ge2e_cos_sim_rows_bwd_workspace_bytes(int B, int n, int N, int M, int D);
int ge2e_cos_sim_rows_bwd(const float* E, const float* C, const float* cos, const float* g_cos, int B, int n, int N, int j0,
                          int M, int D, float eps_cos, float eps, float* dE, float* dC, void* workspace,
                          size_t workspace_bytes, void* stream);
int ge2e_calc_loss_rows(const float* sim, int B, int n, int N, int j0, int M, float eps, int variant, float* loss,
                        float* per_emb_loss, void* stream);
int ge2e_calc_loss_rows_bwd(const float* sim, int B, int n, int N, int j0, int M, float eps, int variant, const float* g_loss,
                            const float* g_per, float* d_sim, void* stream);

/* What `loss.backward()` (s4:200) does with the results of ge2e_loss_fwd_bwd: scale by the incoming gradient g (device;
 * g_count = 1 for a scalar loss or B for a per-batch loss vector) in ONE launch:
 *   gE [B][N][M][D] = g[b] dE[b]   (NULL: skip);   gw [1] = sum_b g[b] dw[b];   gb [1] = sum_b g[b] db[b]   (NULL: skip)
 * dE and gE need only float alignment: 16-byte loads are used when N*M*D % 4 == 0 and both are 16-byte aligned. */
int ge2e_scale_grads(const float* dE, const float* dw, const float* db, const float* g, int g_count, int B, int N, int M,
                     int D, float* gE, float* gw, float* gb, void* stream);

/* ---- the callers either side of the loss ---------------------------------------------------------
 * Encoder tail: the L2-normalisation that ends the encoder's forward (s2_model_GE2E_loss_speach_embed.py:34), the
 * un-permute gather `embeddings[unperm]` (s4_train_embed_model.py:186) and the (N,M,D) reshape (s4:189) in one pass:
 *   e[i][:] = y[src[i]][:] / |y[src[i]]|,  rnorm[i] = 1 / |y[src[i]]|      y, e [rows][D]; src [rows] int32 or NULL (identity)
 * src must be a permutation of 0..rows-1 (the reference's `unperm`); no epsilon, like s2:34. */
int ge2e_normalize_unperm(const float* y, const int* src, int rows, int D, float* e, float* rnorm, void* stream);
/* its backward: dy[src[i]][:] = (g[i] - e[i] (e[i] . g[i])) * rnorm[i]  (every row of dy is written exactly once). */
int ge2e_normalize_unperm_bwd(const float* g, const float* e, const float* rnorm, const int* src, int rows, int D,
                              float* dy, void* stream);
/* Threshold sweep of calculate_ERR (s5_eval_model.py:57-98) on a similarity matrix sim [B][N][M][N]: for every threshold
 * (non-decreasing fp32 table, T <= 4096; the reference's is 0.5 + 0.01 i, i < 50, s5:57) the two integer counts the
 * reference derives FAR and FRR from, counts [B][T][2] int32:
 *   [0] = #{(j,i,k), k != j : sim[j][i][k] > thr}   (s5:82)      [1] = #{(j,i) : sim[j][i][j] > thr}   (s5:89)
 * The comparison is the reference's fp32 `S > thres`; the counts are exact.  FAR/FRR, with the reference's own
 * denominators (s5:81,88), and the argmin over thresholds (s5:93-98) are a few dozen scalar operations on the host. */
int ge2e_eer_counts(const float* sim, int B, int N, int M, const float* thresholds, int T, int* counts, void* stream);

/* Batch sampler (s1_dataset_loader.py:65-77, EmbeddingModelTTDataset.__getitem__ for the N speakers of a batch): the
 * per-speaker spectrogram arrays (U_j, T, F), float64 as the reference stores them on disk (sv_<speaker>.npy) or float32,
 * stay resident in ONE device buffer `store`; spk_offsets [N] (device, int64, in ELEMENTS) locate the arrays of the batch's
 * speakers, utter_idx [N][M] and clip_start [N] (device, int32) are the draws s1:65 and s1:71 make on the host.
 *   out [N][M][L][F] float32 = (float) array_n[utter_idx[n][m]][clip_start[n] .. + L][:]      (s1:68, 74; the cast of s2:28)
 * The caller guarantees 0 <= utter_idx < U_n and 0 <= clip_start <= T - L (the reference's draws do); N * M <= 65535. */
int ge2e_sample_batch(const void* store, int store_is_f64, const long long* spk_offsets, const int* utter_idx,
                      const int* clip_start, int N, int M, int T, int L, int F, float* out, void* stream);

/*
 * ENCODER INFERENCE (csrc/ge2e_encoder.hip): the forward pass of the d-vector encoder (s2:7-35) for inference -- L stacked
 * LSTM layers of H units over the T frames of a window of n_mels mel channels, the LAST frame's top hidden state through one
 * Linear [D][H], divided by its L2 norm -- from mel windows to embeddings in ONE launch.  Forward only, float32, exact fp32
 * on the matrix core (v_mfma_f32_16x16x4_f32).  Supported: H = 128 or 256, 1 <= L <= 4, 1 <= n_mels <= 256, 1 <= D <= 256,
 * any T >= 1 and R >= 1; everything else is GE2E_ERR_IMPL and nothing is launched.
 *
 * ge2e_encoder_pack, once per set of weights.  flat_params: the parameters in torch's own layout as one float32 buffer --
 * per layer l, in order, weight_ih [4H][I_l] (I_0 = n_mels, I_l = H above), weight_hh [4H][H], bias_ih [4H], bias_hh [4H],
 * gate order i, f, g, o; then projection.weight [D][H] and projection.bias [D].  packed (ge2e_encoder_packed_bytes, 16-byte
 * aligned; every byte is written): per layer the matrix [pad16(I_l) + H][4H] in the MFMA's B-fragment order -- the input's k
 * zero-padded to a multiple of 16, i.e. to whole groups of four K-steps, of which a lane fetches 16 contiguous bytes -- with
 * the gate columns permuted so that i, f, g, o of one hidden unit fall into the same lane and register slot of four
 * accumulator tiles, followed by the 4H sums bias_ih + bias_hh in the same column order; then the projection likewise,
 * [H][pad16(D)] and pad16(D) biases, zero past D.  One launch.  Checks, in this order: GE2E_ERR_NULL (flat_params or
 * packed), GE2E_ERR_SHAPE (n_mels, D or L < 1), GE2E_ERR_IMPL, GE2E_ERR_ALIGN (packed not 16-byte aligned).
 *
 * ge2e_encode.  mel [frames][n_mels] float32; row r is the T frames from frame row_start[r] (int64, device) on, or from
 * frame r T where row_start is NULL (mel is then [R][T][n_mels]).  Rows may overlap: the sliding windows of a long utterance
 * are encoded without being materialised.  0 <= row_start[r] and row_start[r] + T <= frames are the caller's guarantee;
 * frames outside every row are never read.  out [R][D]: y / |y| of the projection y for normalize != 0 -- no epsilon, as
 * s2:34: a zero y gives NaN -- and y itself for normalize == 0.  Exactly the R D elements of out are written.
 * One launch of ceil(R / 32) workgroups of 512 threads; a workgroup owns 32 rows for all T steps and all L layers (time
 * outside, layers inside), c in registers, h in LDS (4 L 32 H bytes), the weights streamed from L2 every step; rows past R
 * in the last tile compute on zeros and are never stored.  No workspace, no allocation, no synchronisation, everything on
 * `stream`, grid from the shape alone: fit for a HIP graph.  The bits of an output row depend on that row's frames and the
 * weights ALONE: not on R, on the row's position, or on the tile it fell into.
 * Checked on the host before anything is launched, in this order: GE2E_ERR_NULL (packed, mel or out), GE2E_ERR_SHAPE (R, T,
 * n_mels, D or L < 1), GE2E_ERR_IMPL (H, L, n_mels or D unsupported), GE2E_ERR_ALIGN (packed, mel or out not 16-byte aligned).
 *
 * ge2e_encode_plan (diagnostics, no GPU): "encode<H>/tiles", the instantiation and its grid ceil(R / 32), snprintf-style as
 * ge2e_loss_plan; < 0: GE2E_ERR_SHAPE or GE2E_ERR_IMPL as the call itself.  (These names are no part of ge2e_plan_atoms.)
 */
size_t ge2e_encoder_packed_bytes(int n_mels, int H, int L, int D);   /* 0 for an unsupported shape */
int ge2e_encoder_pack(const float* flat_params, int n_mels, int H, int L, int D, float* packed, void* stream);
int ge2e_encode(const float* packed, const float* mel, const long long* row_start /* [R] or NULL */,
                int R, int T, int n_mels, int H, int L, int D, int normalize,
                float* out /* [R][D] */, void* stream);
int ge2e_encode_plan(int R, int T, int n_mels, int H, int L, int D, char* buf, size_t buf_bytes);

/*
 * ENCODER TRAINING (csrc/ge2e_encoder_train.hip; the forward is csrc/ge2e_encoder.hip's kernel in a second instantiation):
 * the same encoder with gradients -- a forward that keeps what the backward needs, and the backward through time, the
 * projection's and the norm's backward in hand-written HIP, float32, exact fp32 on the matrix core.  Shapes as
 * ge2e_encode: H = 128 or 256, 1 <= L <= 4, 1 <= n_mels <= 256, 1 <= D <= 256, any T >= 1 and R >= 1, dense rows or
 * row_start; everything else is GE2E_ERR_IMPL and nothing is launched.  No gradient with respect to the mels.
 *
 * ge2e_encode_train: ge2e_encode's arguments plus `tape` (ge2e_encode_train_tape_bytes, 16-byte aligned, the caller's).
 * `out` has the bits ge2e_encode writes for the same inputs.  The tape holds EVERYTHING the backward reads, nothing is
 * recomputed but tanh(c): per layer six planes [T][R][H] -- the gate activations i, f, g, o, the cell c, the hidden state h
 * -- then the raw projection [R][D]: 4 (6 L T R H + R D) bytes, i.e. 6 L H T 4 bytes a window: 2.9 MB a window for
 * 3 x 256 at T = 160, 24 GB at R = 8192.  Its layout is private to the two kernels.  Rows past R in the last tile write
 * nothing.  One launch of ceil(R / 32) workgroups, as ge2e_encode.
 *
 * ge2e_encoder_pack_bwd, once per set of weights: flat_params (ge2e_encoder_pack's) -> packed_bwd
 * (ge2e_encoder_packed_bwd_bytes, 16-byte aligned; every byte is written): per layer [4H][I_l + H] -- layer 0: [4H][H],
 * weight_hh alone -- in the fragment order of d[input | h_prev] = dz W, then the projection [pad16(D)][H], zero past D.
 *
 * ge2e_encode_bwd: d_out [R][D], the gradient with respect to ge2e_encode_train's `out` (of y / |y| for normalize != 0:
 * dy = (g - e (e.g)) / |y|, no epsilon; of y itself otherwise) -> d_flat_params, the gradient of every parameter in ONE flat
 * buffer in flat_params' own layout (bias_ih and bias_hh of a layer get the same values).  Written, not accumulated; every
 * element exactly once; nothing outside it is touched.  mel, row_start, the shape and normalize are those of the forward
 * call that filled `tape`.  workspace (ge2e_encode_bwd_workspace_bytes, 16-byte aligned): dZ [L][T][R][4H] in torch's gate
 * order -- the pre-activation gradients, at offset 0 --, dy [R][D], and the K-slice partials of the weight gradients; it
 * needs no initialisation and every byte the call reads it has written itself.
 * Launches: the recurrence, ceil(R / 16) workgroups of 512 threads (a workgroup owns 16 rows for all frames and layers,
 * frames downwards, dc in registers, dh and dz in LDS: 4 (16 L H + 16 (4H + 4)) bytes, 128.25 KiB at H = 256, L = 4); L + 1
 * weight-gradient GEMMs over K = R T (the projection's: K = R), each a grid of 64 x 64 output blocks times K-slices; one
 * reduction that sums the slices in ascending order.  The slices of K pairs are min(ceil(K / 512), 32) equal parts rounded
 * up to a multiple of 4: grids and slice counts come from the shape alone, there are no atomics, and two calls on the same
 * inputs give the same bits.  No allocation, no synchronisation, everything on `stream`: fit for a HIP graph.
 * A row whose d_out is zero contributes exact zeros to every dz.
 * Checks of all of these, in this order: GE2E_ERR_NULL (any pointer but row_start and stream), GE2E_ERR_SHAPE (R, T,
 * n_mels, D or L < 1; the pack: n_mels, D or L < 1), GE2E_ERR_IMPL, GE2E_ERR_ALIGN (any buffer not 16-byte aligned;
 * flat_params is read four bytes at a time and may lie anywhere).  The size queries return 0 where the call would refuse.
 *
 * ge2e_encode_train_plan / ge2e_encode_bwd_plan (diagnostics, no GPU): "encode_train<H>/tiles" and
 * "encode_bwd<H>/tiles,encode_wgrad/NxMxS" (L + 1 times: column blocks x row blocks x slices) ",encode_reduce/blocks",
 * snprintf-style as ge2e_encode_plan.  (These names are no part of ge2e_plan_atoms.)
 */
size_t ge2e_encoder_packed_bwd_bytes(int n_mels, int H, int L, int D);   /* 0 for an unsupported shape */
int ge2e_encoder_pack_bwd(const float* flat_params, int n_mels, int H, int L, int D, float* packed_bwd, void* stream);
size_t ge2e_encode_train_tape_bytes(int R, int T, int n_mels, int H, int L, int D);
int ge2e_encode_train(const float* packed, const float* mel, const long long* row_start /* [R] or NULL */,
                      int R, int T, int n_mels, int H, int L, int D, int normalize,
                      float* out /* [R][D] */, float* tape, void* stream);
size_t ge2e_encode_bwd_workspace_bytes(int R, int T, int n_mels, int H, int L, int D);
int ge2e_encode_bwd(const float* packed_bwd, const float* mel, const long long* row_start /* [R] or NULL */,
                    int R, int T, int n_mels, int H, int L, int D, int normalize, const float* tape,
                    const float* d_out /* [R][D] */, float* d_flat_params, void* workspace, void* stream);
int ge2e_encode_train_plan(int R, int T, int n_mels, int H, int L, int D, char* buf, size_t buf_bytes);
int ge2e_encode_bwd_plan(int R, int T, int n_mels, int H, int L, int D, char* buf, size_t buf_bytes);

/*
 * MEL FRONT END (csrc/ge2e_melspec.hip): waveforms to the frames ge2e_encode reads -- reflect pad, overlapping frames, a
 * window, |rfft|, a mel basis, 20 log10 and a clip (s0:29-66 with pySTFT, s0:201-219) -- in ONE launch.  float32, the mel
 * product exact fp32 on the matrix core (v_mfma_f32_16x16x4_f32).  Supported: n_fft 256, 512, 1024 or 2048, 1 <= n_mels <=
 * 128, any hop >= 1 (it need not divide n_fft and may exceed it), any U >= 1; everything else is GE2E_ERR_IMPL and nothing
 * is launched.
 *
 * ge2e_melspec_pack, once per (window, basis).  window [n_fft] and basis [n_fft/2 + 1][n_mels], float32 on the device, any
 * values: the kernel does not know what a Hann window or a mel scale is.  packed (ge2e_melspec_packed_bytes, 16-byte
 * aligned; every byte is written): the window; the transform's twiddles exp(-2 pi i k / n_fft), k < n_fft, as (cos, sin),
 * computed in double and rounded once; the basis in the MFMA's B-fragment order [column tile][K-step][lane], its n_fft/2 + 1
 * rows zero-padded to a multiple of 4 and its n_mels columns to a multiple of 16.  One launch.  Checks, in this order:
 * GE2E_ERR_NULL (window, basis or packed), GE2E_ERR_SHAPE (n_mels < 1), GE2E_ERR_IMPL, GE2E_ERR_ALIGN (packed not 16-byte
 * aligned).
 *
 * ge2e_melspec.  Utterance u is wav[utt_start[u] .. + utt_len[u]) (int64, in samples, on the device), every sample times
 * gain[u] (1 where gain is NULL), logically extended with zeros to P_u = utt_padded_len[u] (utt_len[u] where NULL; P_u >=
 * utt_len[u] is the caller's guarantee): the reference's zero pad to the last partial slice without a copy.  Samples at or
 * past utt_len[u] are never read.  The extended signal is reflect-padded by n_fft/2 on both sides (numpy's mode='reflect',
 * the edge sample not repeated: this needs P_u > n_fft/2), frame f is samples f hop .. f hop + n_fft of that, and there are
 * F_u = P_u / hop + 1 frames (integer division).  frame_start [U + 1] (int64, device) is the prefix sum of F_u and
 * total_frames its last entry: host arithmetic on lengths, the caller's.  out[frame_start[u] + f][n_mels], float32:
 *   m = |rfft(window . frame)| . basis
 *   mode 0   m, the linear mel
 *   mode 1   clip((20 log10(max(10^(min_level_db / 20), m)) - ref_level_db - min_level_db) / -min_level_db, 0, 1), computed
 *            from the very bits mode 0 stores; min_level_db = -100 and ref_level_db = 16 are s0:47-50
 * A NaN or Inf sample makes EVERY element of the frames that contain it NaN, in both modes (numpy's maximum and clip keep a
 * NaN; nothing is clamped away), and no other frame changes by a bit.  Exactly total_frames n_mels elements are written.
 * One launch of ceil(total_frames / 16) workgroups of 512 threads.  A workgroup owns 16 consecutive rows of out, which may
 * belong to different utterances: each row finds its own by a binary search of frame_start.  One wave per frame gathers it
 * (reflection and zero extension are address arithmetic), applies gain and window, and runs the real transform as an
 * n_fft/2-point complex FFT -- radix-8 and radix-4 butterflies in registers, the points exchanged through LDS between the
 * passes -- plus the real-input post-pass; the 16 x (n_fft/2 + 1) magnitudes in LDS then meet the packed basis, streamed
 * from L2, on the matrix core, one 16-column tile per wave.  No workspace, no allocation, no synchronisation, everything on
 * `stream`, grid from the arguments alone: fit for a HIP graph.  The bits of an output row depend on that frame's samples,
 * its gain and `packed` ALONE: not on U, on the row's position in its tile, or on its neighbours.
 * Checked on the host before anything is launched, in this order: GE2E_ERR_NULL (packed, wav, utt_start, utt_len,
 * frame_start or out), GE2E_ERR_SHAPE (U, hop, n_mels or total_frames < 1, mode not 0 or 1, min_level_db not below 0),
 * GE2E_ERR_IMPL (n_fft or n_mels unsupported), GE2E_ERR_ALIGN (packed or out not 16-byte aligned, wav not aligned to a float).
 *
 * ge2e_melspec_plan (diagnostics, no GPU): "melspec<n_fft>/tiles", the instantiation and its grid ceil(total_frames / 16),
 * snprintf-style as ge2e_loss_plan; < 0: GE2E_ERR_SHAPE or GE2E_ERR_IMPL as the call itself.  (No part of ge2e_plan_atoms.)
 */
size_t ge2e_melspec_packed_bytes(int n_fft, int n_mels);   /* 0 for an unsupported shape */
int ge2e_melspec_pack(const float* window /* [n_fft] */, const float* basis /* [n_fft/2+1][n_mels] */,
                      int n_fft, int n_mels, float* packed, void* stream);
int ge2e_melspec(const float* packed, const float* wav,
                 const long long* utt_start, const long long* utt_len,      /* [U], device, in samples */
                 const long long* utt_padded_len /* [U] or NULL */, const float* gain /* [U] or NULL */,
                 const long long* frame_start /* [U+1], device */, int U, long long total_frames,
                 int n_fft, int hop, int n_mels, int mode, float min_level_db, float ref_level_db,
                 float* out /* [total_frames][n_mels] */, void* stream);
int ge2e_melspec_plan(int U, long long total_frames, int n_fft, int hop, int n_mels, char* buf, size_t buf_bytes);

/*
 * RESAMPLING AND GAIN (csrc/ge2e_resample.hip): the stage in front of ge2e_melspec -- recordings at another rate to the
 * model's (the reference's librosa.resample, utils/audio_utils.py:83-85) in ONE launch, and the per-utterance gain of its
 * normalize_volume (s0:94-105) in two.  float32 in and out.
 *
 * The definition.  Rates sr_in -> sr_out with g = gcd: L = sr_out / g (up), M = sr_in / g (down); a bank taps[L][W] with
 * W = 2 lead + 1, float32 on the device, ANY values: the kernel does not know what a Kaiser window is
 * (audio.resample_bank makes the project's).  Utterance u is x = wav[in_start[u] .. + in_len[u]) (int64, in samples, on
 * the device), taken as zero outside its own extent; samples outside it are never read.  It has
 * n_out = (in_len L + M - 1) div M outputs; output n, with t = n M in 64-bit, i0 = t div L and p = t mod L, is
 *     y[n] = sum_{k=0}^{W-1} taps[p][k] x[i0 + lead - k]
 * Supported: 1 <= L <= 640, 1 <= M <= 640, odd W <= 1025 ({8000, 11025, 22050, 24000, 32000, 44100, 48000, 96000} -> 16000
 * under both presets of audio.resample_bank); everything else is GE2E_ERR_IMPL and nothing is launched.
 *
 * ge2e_resample_pack, once per bank.  packed (ge2e_resample_packed_bytes, 16-byte aligned; every byte is written):
 * [W][pad4(L)] floats, packed[k][q] = taps[(q M) mod L][k] -- the phases in the order consecutive outputs meet them -- and
 * zero in the pad columns.  One launch.  Checks, in this order: GE2E_ERR_NULL (taps or packed), GE2E_ERR_SHAPE (L or M < 1,
 * lead < 0), GE2E_ERR_IMPL, GE2E_ERR_ALIGN (packed not 16-byte aligned).
 *
 * ge2e_resample.  out[out_start[u] + n], n < out_start[u + 1] - out_start[u]; out_start [U + 1] (int64, device) is the
 * prefix sum of n_out and total_out its last entry: host arithmetic on the lengths, the caller's, as frame_start is for
 * ge2e_melspec.  An utterance of length 0 has no outputs and is legal among others.  Exactly total_out elements are written.
 * One launch of floor(total_out / tile) + U workgroups of 256 threads, no workspace, no allocation, no synchronisation,
 * everything on `stream`, grid from the arguments alone: fit for a HIP graph.  A workgroup owns `tile` consecutive outputs of
 * ONE utterance (it finds the utterance by a bisection of out_start) and stages their input span in LDS, the zeros of the
 * extent filled in there; the bank is read from L2.  Accumulation order: one fp32 accumulator per output, started at -0,
 * acc = fma(taps[p][k], x[i0 + lead - k], acc) for k = 0, 1, ..., W - 1 in this order, the zeros outside the extent included.
 * So the bits of y[n] depend on that utterance's samples, on n and on `packed` ALONE: not on U, on the utterance's place in
 * the buffer or on the output's place in its tile.  A NaN sample makes exactly the outputs whose window
 * [i0 + lead - W + 1, i0 + lead] holds it NaN.
 * Checked on the host before anything is launched, in this order: GE2E_ERR_NULL (packed, wav, in_start, in_len, out_start or
 * out), GE2E_ERR_SHAPE (U, L, M or total_out < 1, lead < 0), GE2E_ERR_IMPL (the shape, or more than 2^31 - 1 workgroups),
 * GE2E_ERR_ALIGN (packed or out not 16-byte aligned, wav not aligned to a float).
 *
 * ge2e_resample_plan (diagnostics, no GPU): "resample<lds,R>/tile/grid" -- the instantiation (R outputs a thread, their
 * samples staged in LDS; "global": a span too long for LDS, read from global memory), the outputs of a tile and the grid --
 * snprintf-style as ge2e_melspec_plan; < 0: GE2E_ERR_SHAPE or GE2E_ERR_IMPL as the call itself.  (No part of ge2e_plan_atoms.)
 *
 * ge2e_volume_gain.  gain_out[u] (float32, device) for utterance u = wav[utt_start[u] .. + utt_len[u]):
 *     S = sum x^2, rms = sqrt(S / utt_len), change = target_dbfs - 20 log10(rms), gain = 10^(change / 20),
 * and with increase_only != 0 gain = 1 where change < 0; all in double, rounded once to float32.  A silent utterance gives
 * +inf and a length of 0 NaN, as audio.volume_gain does.  S has a fixed order: tiles of 2048 samples counted from the
 * utterance's start; tile j belongs to slice j mod 128; thread t of a slice's 256 adds the squares of samples
 * 2048 j + t + 256 i, i = 0 .. 7, tile after tile in index order; the 256 sums are added by a butterfly over each wave of 64,
 * then the four waves in order; a second launch adds the utterance's 128 slices in index order.  No atomics: the same bits
 * on every call, and the gain of an utterance does not depend on the others.  Two launches, grid from U alone.  workspace:
 * ge2e_volume_gain_workspace_bytes(total_samples, U) bytes (0 for U < 1 or total_samples < 0), 16-byte aligned; its
 * contents need not be kept.  Checks, in this order: GE2E_ERR_NULL (wav, utt_start, utt_len, gain_out or workspace),
 * GE2E_ERR_SHAPE (U < 1), GE2E_ERR_ALIGN (workspace not 16-byte aligned, wav or gain_out not aligned to a float).
 */
size_t ge2e_resample_packed_bytes(int L, int M, int W);   /* 0 for an unsupported shape */
int ge2e_resample_pack(const float* taps /* [L][2 lead + 1] */, int L, int M, int lead, float* packed, void* stream);
int ge2e_resample(const float* packed, const float* wav,
                  const long long* in_start, const long long* in_len,       /* [U], device, in samples */
                  const long long* out_start /* [U+1], device */, int U, long long total_out,
                  int L, int M, int lead, float* out /* [total_out] */, void* stream);
int ge2e_resample_plan(int U, long long total_out, int L, int M, int lead, char* buf, size_t buf_bytes);
size_t ge2e_volume_gain_workspace_bytes(long long total_samples, int U);
int ge2e_volume_gain(const float* wav, const long long* utt_start, const long long* utt_len /* [U], device */, int U,
                     float target_dbfs, int increase_only, float* gain_out /* [U] */, void* workspace, void* stream);

/*
 * SILENCE TRIMMING (csrc/ge2e_vad.hip): the reference's trim_long_silences (utils/audio_utils.py:107-148), which runs between
 * normalize_volume and the spectrogram.  Everything there that is the reference's own code is reproduced exactly -- window
 * arithmetic, int16 quantisation, moving average, rounding, dilation, selection of samples; the per-window voice decision,
 * which the reference takes from webrtcvad, is the PROJECT'S OWN detector (below), all in integers.  A caller who has flags
 * from elsewhere passes them to ge2e_vad_mask in place of ge2e_vad_flags' and gets the reference's trimming of them.
 *
 * The definition.  Utterance u is wav[utt_start[u] .. + utt_len[u]) (int64, in samples, on the device), float32.  With S
 * samples a window (vad_window_length * sampling_rate div 1000; 480 for the reference) it has W_u = utt_len[u] div S windows;
 * the utt_len[u] mod S samples left over are dropped (s0:118) and never read.  win_start [U + 1] (int64, device) is the prefix
 * sum of W_u and total_windows its last entry: host arithmetic on lengths, the caller's, as frame_start is for ge2e_melspec.
 * gain [U] (float32, device) may be NULL, which means 1.
 *   quantise  q = sat16(rint(fl32(fl32(x * gain[u]) * 32767.0f))) (s0:121 in numpy's float32 arithmetic: two roundings, no
 *             fused multiply-add), rint to nearest, halves to even; NaN gives 0; values past the int16 range saturate (the
 *             reference's astype(np.int16) wraps there: the one deliberate departure).
 *   energy    e = S sum(q^2) - (sum q)^2 over the window's S samples, in int64: S^2 times the variance (DC does not count),
 *             exact, independent of the order of summation, at most 2^54 for S <= 4096.
 *   flag      floor[w] = min e[v] over |v - w| <= floor_span, v in the same utterance;
 *             flag[w] = (e[w] >= min_energy) and (e[w] * 256 > floor[w] * ratio_q8), compared exactly (128-bit products).
 *   mask      m[w] = 2 sum(flag[w - (A - 1) div 2 .. w + A div 2]) > A, A = avg_width, flags outside the utterance zero: the
 *             reference's moving_average and np.round (a mean of exactly 0.5 rounds to 0: the `>`);
 *             keep[i] = any m[i - (n - 1) div 2 .. i + n div 2], n = max_silence + 1: scipy's binary_dilation with np.ones(n).
 *   outputs   dst[w] (int32): the rank of window w among its utterance's kept windows, or -1; out_len[u] = S kept_u (int64).
 *   trim      kept window w of utterance u goes, bits unchanged, to out[out_start[u] + S dst[w] ..]; no arithmetic touches
 *             the samples.  The gain stays a separate factor (ge2e_melspec applies it): select(x) g == select(x g).
 * Supported: 2 <= S <= 4096, 0 <= floor_span <= 1024, avg_width and max_silence + 1 in 1 .. 64, total_windows < 2^31;
 * everything else is GE2E_ERR_IMPL and nothing is launched.  total_windows = 0 is legal and launches nothing.
 *
 * ge2e_vad_flags: two launches.  flags [total_windows] uint8 (0 / 1).  workspace: ge2e_vad_workspace_bytes(total_windows, U)
 * bytes (the int64 energies; 0 for total_windows < 0 or U < 1), 16-byte aligned; it holds e[w] afterwards.  Launch 1 reads
 * every sample once: 16 (S >= 64; S below: 128) consecutive windows a workgroup of 256 threads, 64 (8) lanes a window reading
 * consecutive words, integer sums added by a butterfly.  Launch 2: 256 consecutive windows a workgroup, their energies and
 * floor_span either side staged in LDS, one thread per window.  A window finds its utterance by a bisection of win_start.
 * Checks, in this order: GE2E_ERR_NULL (wav, utt_start, utt_len, win_start or flags), GE2E_ERR_SHAPE (U or S < 1,
 * total_windows, floor_span, ratio_q8 or min_energy < 0), GE2E_ERR_IMPL, GE2E_ERR_WORKSPACE (NULL or not 16-byte aligned),
 * GE2E_ERR_ALIGN (wav or gain not aligned to a float).
 *
 * ge2e_vad_mask: one launch of U workgroups of 1024 threads.  A workgroup walks its utterance in chunks of 4096 windows
 * with the count of kept windows carried from chunk to chunk; integers only, no atomics: the result does not depend on the
 * chunk.  Checks: GE2E_ERR_NULL (flags, win_start, dst or out_len), GE2E_ERR_SHAPE (U, S or avg_width < 1, total_windows
 * or max_silence < 0), GE2E_ERR_IMPL, GE2E_ERR_ALIGN (dst not aligned to an int, out_len not to 8 bytes).
 *
 * ge2e_vad_trim: one launch over the input windows, tiled as launch 1 of ge2e_vad_flags.  A dropped window is not read; a
 * kept one moves in 16-byte pieces where its source and destination are both 16-byte aligned and word by word otherwise.
 * out_start [U] (int64, device) is the caller's: the utterances' own starts for an in-slot form without a read-back, or a
 * dense prefix once out_len is known.  out must not overlap wav.  Exactly sum(out_len) elements are written.  Checks:
 * GE2E_ERR_NULL (wav, utt_start, win_start, dst, out_start or out), GE2E_ERR_SHAPE (U or S < 1, total_windows < 0),
 * GE2E_ERR_IMPL, GE2E_ERR_ALIGN (wav or out not aligned to a float, dst not to an int).
 *
 * Every entry: no allocation, no synchronisation, everything on `stream`, grid from the arguments alone: fit for a HIP graph.
 *
 * ge2e_vad_plan (diagnostics, no GPU): "vad_energy<G>/T/grid,vad_flag/256/grid,vad_mask/4096/U,vad_trim<G>/T/grid" -- G lanes
 * a window and T windows a workgroup, the mask kernel's chunk, the grids -- snprintf-style as ge2e_resample_plan; < 0:
 * GE2E_ERR_SHAPE or GE2E_ERR_IMPL as the calls themselves; total_windows = 0: the empty string.  (No part of ge2e_plan_atoms.)
 */
size_t ge2e_vad_workspace_bytes(long long total_windows, int U);
int ge2e_vad_flags(const float* wav, const long long* utt_start, const long long* utt_len /* [U], device, in samples */,
                   const float* gain /* [U] or NULL */, const long long* win_start /* [U+1], device */, int U,
                   long long total_windows, int S, int floor_span, long long ratio_q8, long long min_energy,
                   unsigned char* flags /* [total_windows] */, void* workspace, void* stream);
int ge2e_vad_mask(const unsigned char* flags /* [total_windows] */, const long long* win_start /* [U+1], device */, int U,
                  long long total_windows, int S, int avg_width, int max_silence, int* dst /* [total_windows] */,
                  long long* out_len /* [U] */, void* stream);
int ge2e_vad_trim(const float* wav, const long long* utt_start /* [U], device */, const long long* win_start /* [U+1] */,
                  const int* dst /* [total_windows] */, const long long* out_start /* [U], device */, int U,
                  long long total_windows, int S, float* out, void* stream);
int ge2e_vad_plan(int U, long long total_windows, int S, int floor_span, int avg_width, int max_silence, char* buf,
                  size_t buf_bytes);

/*
 * OPTIMIZER STEP (csrc/ge2e_optim.hip): the training step's last statements (s4:201-203) -- torch.nn.utils.clip_grad_norm_
 * once per parameter group, then torch.optim.SGD.step -- over a flat gradient bucket in TWO launches, whatever the number
 * of tensors.  Fixed-order sums, no atomics: the same bits on every call.
 *
 * The tables (device memory, the caller's; functional.sgd_layout builds them).  A SEGMENT is one parameter tensor:
 * seg[s] = (address of its first element, its element offset in grad (and in momentum), numel >= 1, group g in [0, G)),
 * four int64; segments are SORTED BY GROUP.  A CHUNK is at most GE2E_SGD_CHUNK consecutive elements of one segment;
 * chunk_start [S + 1] (int32) is the prefix sum of ceil(numel / GE2E_SGD_CHUNK) and C its last entry.  hyper [G][4]
 * (float32) holds lr, max_norm, weight_decay, momentum of each group and is read by the launches themselves: a new
 * learning rate is a device write, and a captured launch stays valid.  The addresses in seg are raw: a parameter whose
 * storage moved needs a new table (functional.sgd_clip_step compares data_ptr() on every call; nothing else can notice).
 *
 * The definition, all in float32 with every operation rounded on its own (no fused multiply-add):
 *   partial[c] = sum over chunk c of fl(fl(g grad_scale)^2); thread t of 256 adds its elements in index order -- single
 *                elements up to the first 16-byte boundary of the gradient, then 16-byte pieces t, t + 256, ..., then at
 *                most 3 single elements -- then a butterfly over each wave of 64, then (w0 + w1) + (w2 + w3).
 *   norm[g]    = sqrtf(sum of the group's partials): thread t adds partial[b + t], partial[b + t + 256], ... of the group's
 *                chunk range in that order, then the same two trees.  EVERY workgroup of launch 2 does this for every
 *                group, with the same code, and holds the same bits.
 *   coef[g]    = c > 1 ? 1 : c with c = max_norm[g] / (norm[g] + 1e-6f): clip_grad_norm_'s formula; a NaN norm gives a NaN
 *                coef (torch.clamp passes it on), an infinite norm 0.
 *   g1 = g grad_scale;  g2 = g1 coef[group]                  (what clip_grad_norm_ leaves in .grad)
 *   g3 = weight_decay != 0 ? g2 + weight_decay p : g2         (SGD's weight decay, after the clip)
 *   m' = momentum != 0 ? momentum m + g3 : g3                 (the buffer starts as zeros, which is torch's "buf = g" at the
 *                                                              first step; dampening 0, no Nesterov)
 *   p' = p - lr[group] m'
 * Stores: p' to the parameter; m' to momentum[offset ..] where momentum is not NULL (also in a group whose momentum is 0,
 * whose m is not read); g2 to grad, or +0 with GE2E_SGD_FLAG_ZERO_GRAD; stats[g] = (norm, coef) where stats is not NULL.
 * GE2E_SGD_FLAG_SKIP_NONFINITE: if the norm of ANY group is not finite, no parameter and no momentum element is written
 * (they keep their bits), grad is written as above, and *skipped is incremented by one workgroup (a plain read and
 * write on the stream; *skipped is the caller's to zero).
 * A segment whose parameter, gradient and momentum addresses are congruent mod 16 moves in 16-byte pieces behind the
 * boundary; any other a word at a time.  Any 4-byte boundary is legal; nothing outside [0, numel) of a segment is touched.
 * A group without segments is legal (norm 0, coef 1 or max_norm / 1e-6f).
 *
 * workspace: ge2e_sgd_clip_workspace_bytes(C) = 4 C rounded up to 256 bytes (0 for C < 1), 256-byte aligned; it holds the
 * partials afterwards.  No allocation, no synchronisation, everything on `stream`, grids from C alone: fit for a HIP graph.
 * Checked on the host before anything is launched, in this order: GE2E_ERR_NULL (seg, chunk_start, grad or hyper;
 * GE2E_SGD_FLAG_SKIP_NONFINITE without skipped), GE2E_ERR_SHAPE (S, C or G < 1, C < S, G > GE2E_SGD_MAX_GROUPS, a flag bit
 * that is not defined), GE2E_ERR_WORKSPACE (NULL, too small, or not 256-byte aligned), GE2E_ERR_ALIGN (grad, momentum or
 * another float32 / int32 buffer not 4-byte aligned, seg not 8-byte aligned).
 *
 * ge2e_sgd_clip_plan (diagnostics, no GPU): "sgd_sqsum/4096/C,sgd_update<mom>/4096/C" -- the chunk and the grid of either
 * launch; <plain> without a momentum buffer -- snprintf-style as ge2e_vad_plan; < 0: GE2E_ERR_SHAPE as the call itself.
 * (No part of ge2e_plan_atoms.)
 */
#define GE2E_SGD_MAX_GROUPS 8
#define GE2E_SGD_CHUNK 4096
#define GE2E_SGD_FLAG_ZERO_GRAD 1
#define GE2E_SGD_FLAG_SKIP_NONFINITE 2
size_t ge2e_sgd_clip_workspace_bytes(int C);                     /* 0 for C < 1 */
int ge2e_sgd_clip_step(const long long* seg /* [S][4] device: address, grad offset, numel, group */,
                       const int* chunk_start /* [S+1] device */, int S, int C, int G,
                       float* grad, float* momentum /* or NULL */, const float* hyper /* [G][4] device */,
                       float grad_scale, int flags, float* stats /* [G][2] or NULL */, int* skipped /* or NULL */,
                       void* workspace, size_t workspace_bytes, void* stream);
int ge2e_sgd_clip_plan(int S, int C, int G, int has_momentum, int flags, char* buf, size_t buf_bytes);

/* ---- diagnostics (tests only): which kernels a call launches ---------------------------------------------------------
 * Below ge2e_resolve_impl every launcher chooses again among kernels and template instantiations.  These queries print
 * that choice -- made by the very functions the launchers switch on -- without a GPU and without launching anything:
 * the names of the kernels the call would launch, in launch order, separated by commas, e.g.
 *     tiled_prep<10,2>,tiled_sim<C3>,tiled_rows<64>,tiled_gc<C3>/4,tiled_spk,tiled_ge<C2>
 * One name ("atom") per kernel instantiation; tiled_gc<C3> carries its row split (/1, /2, /4, /8) because the row
 * pieces and the order of the final add differ per split.  Commas inside <> belong to a name.  Names are stable.
 * snprintf-style: at most buf_bytes - 1 characters and a NUL are written to buf (host memory; NULL with buf_bytes = 0
 * just measures), the full length is returned; < 0: the code the call itself would fail with for these arguments
 * (GE2E_ERR_SHAPE, GE2E_ERR_VARIANT, GE2E_ERR_IMPL).  Grid sizes depend on the device and are no part of a plan.
 *   ge2e_loss_plan     ge2e_loss_fwd_bwd(B, N, M, D, variant, impl) with dE != NULL (want_grad != 0) or dE == NULL;
 *                      raw != 0: ge2e_loss_fwd_bwd_raw instead (impl is ignored)
 *   ge2e_cos_sim_plan  ge2e_cos_sim on a workspace of ge2e_cos_sim_workspace_bytes (shapes off the matrix-core route: "generic")
 *   ge2e_plan_atoms    every name the two queries above can print */
int ge2e_loss_plan(int B, int N, int M, int D, int variant, int impl, int want_grad, int raw, char* buf, size_t buf_bytes);
int ge2e_cos_sim_plan(int B, int N, int M, int D, char* buf, size_t buf_bytes);
int ge2e_plan_atoms(char* buf, size_t buf_bytes);

/* ---- diagnostics (tests only): device building blocks on caller data ------------------- */
/* A,Bm [64][256], G [64][64] (|x| <= 1) -> X [64][64] = A.Bm^T, GE [64][256] = G.A,
 * GC [64][256] = G^T.Bm through the split-fp16 MFMA tile contractions. */
int ge2e_selftest_split_gemm(const float* A, const float* Bm, const float* G,
                             float* X, float* GE, float* GC, void* stream);
/* x [64] -> out [384]: wave_sum, wave_max, row16_sum, quad_sum, wave_argmax idx, quad_argmax idx. */
int ge2e_selftest_wave_ops(const float* x, float* out, void* stream);

/* One wave of the team kernel's per-speaker chain on caller data: CH [64][256], R [16][256] (unit rows)
 * -> XT [64][16] = CH.R^T (16x16x32 tiles), GE [16][256] = XT^T.CH with XT taken straight from the
 * accumulators, GT = GE stored through the in-quad register transpose. */
int ge2e_selftest_rows16(const float* CH, const float* R, float* XT, float* GE, float* GT, void* stream);
/* Team formation (8 workgroups of one XCD) + the L2 hand-off protocol under load: `grid` workgroups
 * (all resident), `rounds` publish/consume rounds of `payload_f4` float4 per member.
 * out [16] (device): [0] complete teams, [1] mismatching float4 read back, [2..9] workgroups per XCD,
 * [10] abort word.  ws: ge2e_selftest_team_bytes(payload_f4) bytes, 256-byte aligned. */
size_t ge2e_selftest_team_bytes(int payload_f4);
int ge2e_selftest_team(void* ws, size_t ws_bytes, int grid, int rounds, int payload_f4, unsigned* out,
                       void* stream);

/* ge2e_loss_fwd_bwd with impl = GE2E_IMPL_TEAM and the team kernel's abort word raised before the launch: exercises the
 * in-launch redo (the same workgroups, one per batch) deterministically.  Same arguments and results. */
int ge2e_selftest_team_fallback(const float* E, int B, int N, int M, int D, const float* w, const float* b,
                                float eps_cos, float eps, int variant, float* loss, float* per_emb_loss, float* dE,
                                float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream);

/* The same with the abort word raised by ONE workgroup (block index grid / 2) when it reaches the end of the launch: the
 * workgroups that finished before leave, the later ones stay, and the redo must agree on its size (TeamCtl::go).  dE may be
 * NULL (the forward-only team kernel).  Same arguments and results. */
int ge2e_selftest_team_abort_midgrid(const float* E, int B, int N, int M, int D, const float* w, const float* b,
                                     float eps_cos, float eps, int variant, float* loss, float* per_emb_loss, float* dE,
                                     float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream);

/* ge2e_loss_fwd_bwd with impl = GE2E_IMPL_TEAM on at most max_workgroups workgroups (>= 64, rounded down to a multiple
 * of 64 = one team per XCD): the same results from fewer teams, i.e. many more batches through each team's hand-off
 * counters than a full-size launch reaches. */
int ge2e_selftest_team_grid(const float* E, int B, int N, int M, int D, const float* w, const float* b,
                            float eps_cos, float eps, int variant, float* loss, float* per_emb_loss, float* dE,
                            float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream,
                            int max_workgroups);

/* ge2e_verify_scores with the form of its rows kernel chosen by the caller: 0 = as the product call chooses (2), 1 = the
 * model tiles staged in LDS once per workgroup (up to T = 2730; above that there is no room beside the histograms and the
 * call streams), 2 = every wave streams them from L2.  Same arguments, checks and results (bit for bit); for the tests of
 * both forms and for tools/bench_enroll_verify.py, which measured 2 faster than 1. */
int ge2e_selftest_verify_form(const float* E, const int* labels, const float* models, const int* cnt, int K, int R, int D,
                              float eps_cos, float eps, const float* thresholds, int T, float* scores, int* counts,
                              int* trials, void* stream, int form);

/* ge2e_identify with the number of bank slices forced to `slices` (clamped to 1 .. ceil(K / 64), and so that tiles x slices
 * stays a launchable grid; slices that would start past the bank are not made); 0 = the product's choice.  The workspace
 * must be ge2e_selftest_identify_workspace_bytes(K, R, D, k_top, slices).  Same checks and results (bit for bit): for the
 * tests of the split and for tools/bench_identify.py. */
size_t ge2e_selftest_identify_workspace_bytes(int K, int R, int D, int k_top, int slices);
int ge2e_selftest_identify_slices(const float* E, const int* labels, const float* models, const int* cnt, int K, int R, int D,
                                  int k_top, float eps_cos, float eps, int* idx, float* score, int* rank, int* hist,
                                  void* workspace, size_t workspace_bytes, void* stream, int slices);

/* ge2e_cohort_stats with the chunk forced to `chunk_rows` rows (rounded up to a multiple of 64; <= 0 = the product's choice),
 * so that a small R crosses chunk boundaries.  The workspace must be ge2e_selftest_cohort_stats_workspace_bytes(C, R, D,
 * n_top, chunk_rows).  Same checks and results (bit for bit): for the tests of the chunking and for tools/bench_snorm.py. */
size_t ge2e_selftest_cohort_stats_workspace_bytes(int C, int R, int D, int n_top, int chunk_rows);
int ge2e_selftest_cohort_stats_chunk(const float* X, const int* sel, int sel_min, const float* cohort, const int* ccnt, int C,
                                     int R, int D, int n_top, float eps_cos, float eps, float eps_std, float* stats,
                                     void* workspace, size_t workspace_bytes, void* stream, int chunk_rows);

#ifdef __cplusplus
}
#endif
#endif /* GE2E_HIP_H */
