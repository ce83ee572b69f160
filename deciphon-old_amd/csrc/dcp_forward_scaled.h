// dcp_forward_scaled.h -- the scaled probability-space Forward recursion's one rule, as the kernels
// (dcp_forward_scaled.hip) and the host twin (dcp_forward_scaled_tables, dcp_model.cpp) both evaluate it.  DESIGN 24.
//
// The recursion is dcp_forward.h's with every value v held as a double u beside an integer exponent s, v = u 2^s:
//   * a table value t (a log-probability) enters as a factor f(t) >= 0, f(-inf) = 0 exactly;
//   * a candidate is predecessor x factor, a combination is a sum in index order, written as a chain of fused
//     multiply-adds from 0:  acc = fma(p_1, f_1, 0), acc = fma(p_2, f_2, acc), ..  (dcp_fws_fma: explicit, so no unit
//     depends on contraction);
//   * the delete chain is D_k = fma(dd_k, D_{k-1}, M_{k-1} md_k);
//   * all history rows of P, Q, PN, PJ, PC of a pair share one exponent; the null state R has one of its own.  After a
//     row, ref = max(PN, PJ, PC, E, B) of that row; if ref != 0 lies outside [2^-band, 2^band], every ring value (and
//     the carried E and C) is multiplied by the power of two that brings ref into [1, 2) -- exact -- and the exponent
//     follows.  R's ring does the same on PR.  Row 0 is a row: its ref is max(PN, B) = max(SN, SB), and the rule applies
//     before P(0) = B ENT is formed, so that special transitions near e^-708 do not leave rows 0 and 1 in the subnormals;
//   * at the finish the last row's E and C are multiplied by the power of two that brings the larger of them into
//     [1, 2) (dcp_fws_rescale_by with band 0), then alt = fma(C, ct, E et): with et, ct near e^-708 the sum stays normal
//     and does not depend on where the band left E;
//   * a score is formed once, at the end: u 2^s = m 2^e with m in [0.5, 1), score = log(m) + e ln 2; 0 gives -inf.
//
// Factors.  A double DB: f(t) = exp(t) in double, each side its own exp.  A float DB: dcp_fws_factor_f32 below (exported as dcp_fwd_factor_f32), the
// same bits on both sides.
#ifndef DCP_FORWARD_SCALED_H
#define DCP_FORWARD_SCALED_H

#include "dcp_forward.h"

enum
{
    DCP_FWS_BAND = 64, // ref stays within [2^-band, 2^band] between rescalings
    // rows of ldk doubles in a wavefront's work area of the scaled wide sweep: the log-space sweep's thirteen (the rings
    // of P and Q, the row's M, I, D), then the profile's eight rows of transition factors
    DCP_FWS_WORK_ROWS = DCP_FWD_WORK_ROWS + 8
};

DCP_FWD_HD inline double dcp_fws_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// ---- the float DB's factor ----------------------------------------------------------------------------------------
// exp(t) of a float t as a double: n = round(t log2 e) by the 1.5 2^23 trick, r = t - n ln 2 in two fused steps (ln 2
// split so that n hi is exact), exp(r) = 1 + r + r^2 q(r) with a degree-5 q in float Horner steps (the coefficients of
// the Cephes expf), and an exact scaling by 2^n in double.  Float and double arithmetic and explicit fmaf only: no
// libm function, nothing a contraction could change.
//
// Supported range: -708 <= t <= 708.  Below -708 (and -inf) the result is an exact 0: e^-708 = 2^-1021.4 is the last
// point at which the double result is still normal for every r.  Above 708 the result is +inf, which the sweeps flag.
// Its largest relative error against exp in double over every float of the range: tests/c/fwd_factor_exhaustive.c,
// recorded in profiles/forward_scaled/factor_delta.txt.
#define DCP_FWS_T_MIN (-708.0f)
#define DCP_FWS_T_MAX (708.0f)

DCP_FWD_HD inline double dcp_fws_factor_f32(float t)
{
    if (!(t >= DCP_FWS_T_MIN)) return 0.0; // -inf and NaN too
    if (t > DCP_FWS_T_MAX) return __builtin_inf();
    float const magic = 12582912.0f; // 1.5 2^23: the sum's low bits are round(t log2 e)
    float const z = __builtin_fmaf(t, 1.44269504088896341f, magic);
    float const n = z - magic; // |n| <= 1022
    float r = __builtin_fmaf(n, -0.693145751953125f, t);
    r = __builtin_fmaf(n, -1.428606765330187e-6f, r);
    float q = 1.9875691500e-4f;
    q = __builtin_fmaf(q, r, 1.3981999507e-3f);
    q = __builtin_fmaf(q, r, 8.3334519073e-3f);
    q = __builtin_fmaf(q, r, 4.1665795894e-2f);
    q = __builtin_fmaf(q, r, 1.6666665459e-1f);
    q = __builtin_fmaf(q, r, 5.0000001201e-1f);
    float const rr = r * r;
    float const p = __builtin_fmaf(q, rr, r) + 1.0f; // in (0.70, 1.42)
    // 2^n as a double, n + 1023 in 1 .. 2045: p 2^n is normal, the product exact
    uint64_t const sb = (uint64_t)((int)n + 1023) << 52;
    return (double)p * __builtin_bit_cast(double, sb);
}

// the factor of a table value: Real is the DB's scalar
DCP_FWD_HD inline double dcp_fws_factor(float t) { return dcp_fws_factor_f32(t); }
DCP_FWD_HD inline double dcp_fws_factor(double t) { return exp(t); }

// ---- exponents ----------------------------------------------------------------------------------------------------
// 2^k, k in -1022 .. 1023
DCP_FWD_HD inline double dcp_fws_pow2(int k) { return __builtin_bit_cast(double, (uint64_t)(k + 1023) << 52); }

// The rescaling of a ring whose reference value is ref (finite, >= 0): 0 if ref is 0 or within the band, else the k
// (clamped to -1022 .. 1022) with ref 2^-k in [1, 2) -- a subnormal ref gets the largest step, the next row the rest.
// The ring is multiplied by dcp_fws_pow2(-k) and k is added to its exponent.
DCP_FWD_HD inline int dcp_fws_rescale_by(double ref, int band)
{
    if (ref == 0.0) return 0;
    int biased = (int)((__builtin_bit_cast(uint64_t, ref) >> 52) & 0x7ffu);
    if (biased == 0) biased = 1;
    int k = biased - 1023;
    if (k >= -band && k < band) return 0; // (2^band itself rescales too: harmless, and one compare less)
    if (k > 1022) k = 1022;
    return k;
}

DCP_FWD_HD inline int dcp_fws_finite(double v) { return v < __builtin_inf() && v == v; }

// the score of u 2^s, u >= 0 finite: the canonical split, so the bits do not depend on where rescalings happened
DCP_FWD_HD inline double dcp_fws_score(double u, int s)
{
    if (u == 0.0) return dcp_fwd_ninf();
    int e;
    double const m = frexp(u, &e);
    double const shift = (double)(e + s) * 0.693147180559945309417232121458;
    return log(m) + shift;
}

#ifdef __cplusplus
extern "C" {
#endif
// The scaled Forward sweep (dcp_forward_scaled.hip): dcp_forward_launch's classes (R = 1, 2, 4, or 0: the wide sweep),
// scores only (store = DCP_FWD_STORE_NONE) or with every row's record as logs (DCP_FWD_STORE_ROWS).  A pair whose values left the double range is appended to redo[atomicAdd(nredo, 1)] (while that is below
// redo_cap: give the launches that share a counter room for all their pairs) and its scores are -inf and mean nothing:
// the caller reruns it by dcp_forward_launch.  band: DCP_FWS_BAND, or the hooks build's.  != 0: no such kernel, no redo
// list, a band outside 1 .. 500, a wide sweep whose work_stride is no multiple of DCP_FWS_WORK_ROWS, or
// dcp_fwd_args_refused.
int dcp_forward_scaled_launch(int precision, int R, int store, struct dcp_fwd_args const *a, struct dcp_fwd_pair *redo,
                              uint32_t *nredo, uint32_t redo_cap, int band, void *stream);
#ifdef __cplusplus
}
#endif

#endif
