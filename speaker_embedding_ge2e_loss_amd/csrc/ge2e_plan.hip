// The launch plans (ge2e_plan.hpp) as text: the diagnostics ge2e_loss_plan, ge2e_cos_sim_plan and ge2e_plan_atoms of
// include/ge2e_hip.h.  Host code only: one name per kernel instantiation ("atom"), the names of a call in launch order.
// The names are stable (tests keep the plan of every case they run):
//   generic   fused_f32<NCH>   fused_split<NCH>   wave<M,NX>   wave<M,NX,raw>
//   team<NCH,MR,RBT,softmax|contrast>   team_fwd<NCH,MR,RBT,softmax|contrast>
//   tiled_prep<RM,NP>   tiled_sim<C>   tiled_simrows<C3,softmax|contrast,N256|Nany>   tiled_rows<W>   tiled_gc<C1|C2>
//   tiled_gc<C3>/S (S = gc_split: the row pieces differ per split)   tiled_spk   tiled_ge<C>   tiled_reduce   tiled_cos
#include "../../include/ge2e_hip.h"
#include "ge2e_plan.hpp"

namespace ge2e {
namespace {

const char* var_name(bool contrast) { return contrast ? "contrast" : "softmax"; }

void add_prep(Out& o, const PrepPlan& p) { o.add("tiled_prep<%d,%d>", p.rm, p.np); }
void add_gc(Out& o, int cfg, int split) {
    if (cfg == kTileC3) o.add("tiled_gc<C3>/%d", split);
    else o.add("tiled_gc<C%d>", cfg);
}
void add_team(Out& o, const char* kernel, const TeamPlan& t) {
    o.add("%s<%d,%d,%d,%s>", kernel, t.nch, t.mr, t.rbt, var_name(t.contrast));
}
void add_wave(Out& o, const WavePlan& w) {
    if (w.raw) o.add("wave<%d,%d,raw>", w.m, w.nx);
    else o.add("wave<%d,%d>", w.m, w.nx);
}
void add_simrows(Out& o, bool contrast, bool full) { o.add("tiled_simrows<C3,%s,%s>", var_name(contrast), full ? "N256" : "Nany"); }

}  // namespace

int plan_string_loss(int B, int N, int M, int D, int variant, int impl, bool want_grad, bool raw, char* buf, size_t cap) {
    Out o{buf, cap};
    if (raw || impl == GE2E_IMPL_WAVE) {
        const WavePlan w = plan_wave(N, M, raw);
        if (w.m == 0) return GE2E_ERR_IMPL;
        add_wave(o, w);
        return o.done();
    }
    switch (impl) {
        case GE2E_IMPL_GENERIC: o.add("generic"); break;
        case GE2E_IMPL_FUSED_F32: o.add("fused_f32<%d>", plan_fused_f32(D).nch); break;
        case GE2E_IMPL_FUSED_SPLIT: o.add("fused_split<%d>", plan_fused_split(D).nch); break;
        case GE2E_IMPL_TEAM: add_team(o, want_grad ? "team" : "team_fwd", plan_team(N, M, D, variant)); break;
        case GE2E_IMPL_TILED: {
            const TiledPlan t = plan_tiled(B, N, M, D, variant, want_grad);
            add_prep(o, t.prep);
            if (t.simrows) add_simrows(o, t.simrows_contrast, t.simrows_full);
            else o.add("tiled_sim<C%d>", t.sim);
            if (t.rows) o.add("tiled_rows<%d>", t.rows);
            if (t.gc != kTileNone) {
                add_gc(o, t.gc, t.gc_split);
                o.add("tiled_spk");
                o.add("tiled_ge<C%d>", t.ge);
            }
            if (t.reduce) o.add("tiled_reduce");
            break;
        }
        default: return GE2E_ERR_IMPL;
    }
    return o.done();
}

int plan_string_cos(int B, int N, int M, int D, bool matrix_cores, char* buf, size_t cap) {
    Out o{buf, cap};
    if (!matrix_cores) {
        o.add("generic");
        return o.done();
    }
    const TiledCosPlan t = plan_tiled_cos(B, N, M, D);
    add_prep(o, t.prep);
    o.add("tiled_sim<C%d>", t.sim);
    o.add("tiled_cos");
    return o.done();
}

// Every instantiation the launchers' switches hold, written out by hand from those switches (NOT collected from the
// plan functions: tests scan shapes through the queries above and hold the union of what they see to this list).
int plan_string_atoms(char* buf, size_t cap) {
    Out o{buf, cap};
    o.add("generic");
    for (int nch = 1; nch <= 4; ++nch) o.add("fused_f32<%d>", nch);
    for (int nch = 1; nch <= 4; ++nch) o.add("fused_split<%d>", nch);
    static const int wave[8][3] = {{2, 6, 12}, {3, 5, 10}, {4, 4, 10}, {5, 4, 8}, {6, 3, 8}, {8, 3, 8}, {10, 2, 6}, {16, 2, 3}};
    for (const auto& w : wave) {
        add_wave(o, {w[0], w[1], false});
        add_wave(o, {w[0], w[2], false});
        add_wave(o, {w[0], w[1], true});
    }
    for (const char* kernel : {"team", "team_fwd"})
        for (int contrast = 0; contrast < 2; ++contrast) {
            for (int mr : {10, 16})
                for (int nch = 1; nch <= 4; ++nch) add_team(o, kernel, {nch, mr, 0, contrast != 0});
            add_team(o, kernel, {4, 10, 5, contrast != 0});
        }
    for (int np = 1; np <= 3; ++np) add_prep(o, {10, np});
    add_prep(o, {0, 4});
    for (int c = kTileC1; c <= kTileC3; ++c) o.add("tiled_sim<C%d>", c);
    for (int contrast = 0; contrast < 2; ++contrast)
        for (int full = 0; full < 2; ++full) add_simrows(o, contrast != 0, full != 0);
    o.add("tiled_rows<16>");
    o.add("tiled_rows<64>");
    add_gc(o, kTileC1, 1);
    add_gc(o, kTileC2, 1);
    for (int split : {1, 2, 4, 8}) add_gc(o, kTileC3, split);
    o.add("tiled_spk");
    for (int c = kTileC1; c <= kTileC3; ++c) o.add("tiled_ge<C%d>", c);
    o.add("tiled_reduce");
    o.add("tiled_cos");
    return o.done();
}

}  // namespace ge2e
