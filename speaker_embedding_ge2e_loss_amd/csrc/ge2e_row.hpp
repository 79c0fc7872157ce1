// The coefficients of a row's gradient in the fp32 loss kernels, written once (row_coeffs, row_own_o, row_c4_share): the two
// one-workgroup-per-batch kernels and the three row kernels of ge2e_tiled.hip, which also take their leave-one-out own-column
// cosine from here (own_column_cos).  Algebra: oracle/ge2e_oracle.py:closed_form
// and the header of ge2e_fused_f32.hip.  The operand order and the parentheses of every expression are part of the
// results: the kernels agree bit for bit with what they computed when each carried its own copy.
#pragma once
#include "ge2e_common.hpp"
#include "ge2e_dev.hpp"

namespace ge2e {

// dE_r = w gE rne + c1 e-hat + c2 s_j + KJ_j: the coefficients of a row from ad = dL/dcos on its own-speaker column,
// coef = (dL/d e-hat) . e-hat, the norm bookkeeping of e (rne, ke) and of the leave-one-out centroid u (rnu, ku) and
// cosd = cos(e, u); alpha and beta are the row's e-hat and s_j terms of its speaker's KJ row.  (A caller with pad rows
// passes an rne that is 1 there.)
struct RowCoeffs { float c1, c2, alpha, beta; };
__device__ __forceinline__ RowCoeffs row_coeffs(float ad, float coef, float rne, float ke, float rnu, float ku, float cosd,
                                                float inv_m1) {
    RowCoeffs rc;
    const float rho = rnu * inv_m1;
    rc.c2 = rho * (ad * rne + ad * ku * cosd * rnu * inv_m1);
    rc.c1 = (-ke * coef * rne - ad * rnu * inv_m1) - rc.c2 / rne;
    rc.alpha = ad * rnu * (1.0f + ku * cosd * rho / rne);
    rc.beta = -ad * rnu * ku * cosd * rho;
    return rc;
}
// o / (dL/dS on the own column): the factor that turns the own-speaker column of dL/dS into o = c2 |s_j| / (ra w), the
// value it carries into the gradient contractions (sj = |s_j| scale).  Needed while dL/dS is still being formed, before
// the reductions that give ad and coef -- hence not a member of RowCoeffs.
__device__ __forceinline__ float row_own_o(float rne, float rnu, float ku, float cosd, float inv_m1, float sj) {
    const float rho = rnu * inv_m1;
    return rho * (rne + ku * cosd * rho) * sj / rne;
}
// The own-speaker column of a row without a second pass over the speaker's rows (ge2e_tiled.hip): the cosine with the
// leave-one-out centroid u = (s_j - e) / (M - 1) from the row scalars rst = (1/|e|, kappa_e, |e|^2, .), the speaker scalars
// cs = (., ., |s_j| scale, |s_j|^2) of the preparation pass and xo = e-hat . c-hat_j, the own column of the similarity.
struct OwnCos { float cosd, rnu, ku; };
__device__ __forceinline__ OwnCos own_column_cos(const float4& rst, const float4& cs, float xo, float inv_m1, float eps_cos) {
    OwnCos o;
    const float rne = rst.x, ee = rst.z;
    const float es = xo * cs.z / rne;
    const float eu = (es - ee) * inv_m1;
    const float uu = fmaxf((cs.w - 2.0f * es + ee) * (inv_m1 * inv_m1), 0.0f);
    unit_stats_fast(uu, eps_cos, o.rnu, o.ku);
    o.cosd = eu * rne * o.rnu;
    return o;
}
// c4': the row's share of the c-hat_j coefficient of the speaker's KJ row, (beta |s_j| + kap_j alpha xo) / (M - 1)
__device__ __forceinline__ float row_c4_share(const RowCoeffs& rc, float inv_m1, float sj, float kap, float xo) {
    return inv_m1 * (rc.beta * sj + kap * rc.alpha * xo);
}

}  // namespace ge2e
