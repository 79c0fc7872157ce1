// Launch plans: which kernel instantiations a call launches, decided from the shape alone.
// Every launcher with a choice has ONE decision function (plan_*, defined next to its launcher); the launcher only
// switches on the plan it returns, and the plan queries of include/ge2e_hip.h (ge2e_plan.hip) print the same plan
// without a GPU.  Device-dependent values -- grid sizes, occupancy -- are no part of a plan.
#pragma once
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>

namespace ge2e {

// snprintf-style accumulation of a plan into a caller's buffer: writes what fits, counts everything.  (Hidden: the
// variadic member is never inlined and would be an exported symbol of the library otherwise.)
struct __attribute__((visibility("hidden"))) Out {
    char* buf;
    size_t cap;
    int len = 0;
    void add(const char* fmt, ...) __attribute__((format(printf, 2, 3))) {
        char atom[64];
        va_list ap;
        va_start(ap, fmt);
        const int n = vsnprintf(atom, sizeof atom, fmt, ap);
        va_end(ap);
        for (int i = -(len > 0); i < n; ++i, ++len)         // (a comma in front of every name but the first)
            if (buf && (size_t)len + 1 < cap) buf[len] = i < 0 ? ',' : atom[i];
    }
    int done() {
        if (buf && cap > 0) buf[(size_t)len < cap ? (size_t)len : cap - 1] = '\0';
        return len;
    }
};

// tile configurations of the tiled contractions (ge2e_tiled.hip: C1 = 128 x 128, C2 = 256 x 256 fed from registers,
// C3 = 256 x 256 fed by LDS-DMA); 0 = that kernel does not run
enum { kTileNone = 0, kTileC1 = 1, kTileC2 = 2, kTileC3 = 3 };

struct PrepPlan { int rm, np; };                 // ge2e_tiled_prep<RM, NP>
struct TiledPlan {
    PrepPlan prep;
    int sim;                 // ge2e_tiled_sim<C>, or kTileNone where simrows runs instead
    bool simrows;            // ge2e_tiled_simrows<C3, contrast, full>: similarity + row pass in one kernel
    bool simrows_contrast, simrows_full;
    int rows;                // ge2e_tiled_rows<16 | 64>, 0 after simrows
    int gc, gc_split, ge;    // kTileNone for a forward-only call; gc_split > 1 only with gc == kTileC3
    bool reduce;             // ge2e_tiled_reduce: forward-only calls
};
struct TiledCosPlan { PrepPlan prep; int sim; };             // ge2e_cos_sim on the matrix cores: prep, sim, ge2e_tiled_cos
struct TeamPlan { int nch, mr, rbt; bool contrast; };        // ge2e_team_kernel / ge2e_team_fwd_kernel<NCH, MR, RBT, CONTRAST>
struct WavePlan { int m, nx; bool raw; };                    // ge2e_wave_kernel<M, NX, RAW>; m = 0: no instantiation takes the call
struct FusedPlan { int nch; };                               // ge2e_fused_{f32,split}_kernel<NCH>

TiledPlan plan_tiled(int B, int N, int M, int D, int variant, bool want_grad);
TiledCosPlan plan_tiled_cos(int B, int N, int M, int D);
TeamPlan plan_team(int N, int M, int D, int variant);        // launch_team and launch_team_fwd: the same grid of instantiations
WavePlan plan_wave(int N, int M, bool raw);
FusedPlan plan_fused_split(int D);
FusedPlan plan_fused_f32(int D);

// ge2e_plan.hip: the plan of a loss call that `impl` (already resolved: one of GE2E_IMPL_GENERIC .. GE2E_IMPL_WAVE) runs, of a
// raw call and of ge2e_cos_sim's matrix-core route as comma-separated kernel names, and every name there is.
// snprintf-style: at most cap - 1 characters and a NUL are written, the full length is returned.
int plan_string_loss(int B, int N, int M, int D, int variant, int impl, bool want_grad, bool raw, char* buf, size_t cap);
int plan_string_cos(int B, int N, int M, int D, bool matrix_cores, char* buf, size_t cap);
int plan_string_atoms(char* buf, size_t cap);

}  // namespace ge2e
