// Workspace layout + launchers of enrolment and verification (see ge2e_enroll.hip): a speaker bank filled from labelled
// rows, its unit models, and held-out trial rows scored against them.
#pragma once
#include "ge2e_common.hpp"
#include "ge2e_labels.hpp"

namespace ge2e {

// Enrolment can activate a speaker with a single row: the tables behind the index kernel's lone-speaker instantiation are
// read for min(K, R) speakers.
inline int enroll_capacity(int K, int R) { return K < R ? K : R; }

// ge2e_enroll_accumulate's workspace: the index tables (ge2e_labels.hpp) of one batch and nothing else.
inline IndexTables enroll_layout(int K, int R) { return index_tables(0, 1, K, R, true); }

// One wave per compact speaker behind the index kernel: sums[speakers[k]] += the speaker's rows, cnt[speakers[k]] += m.
hipError_t launch_enroll_accumulate(const float* E, const int* off, const int* order, const int* speakers, const int* active,
                                    int K, int R, int D, float* sums, int* cnt, hipStream_t stream);
// One wave per speaker: models[s] = the unit centroid, or +0 where cnt[s] <= 0.
hipError_t launch_enroll_finalize(const float* sums, const int* cnt, int K, int D, float eps_cos, float* models,
                                  hipStream_t stream);

// Launch-time description of ge2e_verify_scores and ge2e_verify_scores_normed.  Every pointer is a device pointer.
struct ProblemVerify {
    const float* E;        // [R][D] trial rows, in the caller's order
    const int* labels;     // [R] or null
    const float* models;   // [K][D]
    const int* cnt;        // [K]
    const float* thr;      // [T] non-decreasing, or null
    float* scores;         // [R][K] or null
    int* counts;           // [T][2] or null
    int* trials;           // [2] or null
    const float* row_stats;     // [R][2] {mean, spread} of the trial rows, or null: the plain call
    const float* model_stats;   // [K][2] of the models; with row_stats
    int K, R, D, T;
    float eps_cos, eps;
};
// Which form the rows kernel takes: the model tiles streamed from L2 by every wave (AUTO: the faster one where it was
// measured), or staged in LDS once per workgroup (where T leaves room for the buffers beside the histograms).
enum VerifyForm { VERIFY_AUTO = 0, VERIFY_STAGED = 1, VERIFY_STREAMED = 2 };
bool verify_staged_fits(int T);   // the staging buffers and the histograms fit the LDS of one launch
// A zeroing launch where counts or trials are wanted, then the rows kernel.  With row_stats the scores are normalised
// (ge2e_verify_scores_normed), in the streamed form whatever `form` says.
hipError_t launch_verify_scores(const ProblemVerify& p, VerifyForm form, hipStream_t stream);

}  // namespace ge2e
