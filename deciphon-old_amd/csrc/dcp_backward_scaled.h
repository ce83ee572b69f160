// dcp_backward_scaled.h -- the scaled probability-space Backward recursion's one rule, as the kernels
// (dcp_backward_scaled.hip) and the host twin (dcp_posterior_scaled_tables, dcp_model.cpp) both evaluate it.  DESIGN 25.
//
// The recursion is dcp_posterior.h's with dcp_forward_scaled.h's conventions: every value v is a double u beside an
// integer exponent s, v = u 2^s; a table value t enters as the factor dcp_fws_factor(t); every combination is a chain of
// dcp_fws_fma from 0 in the order dcp_posterior.h lists the terms, a term that does not exist being a factor 0:
//
//   bP_k(j) = sum_{l=1..5} bM_k(j+l) fM_k(x[j..j+l))          bQ_k(j) = sum_l bI_k(j+l) fI(x[j..j+l))
//   bPX(j)  = sum_l bX(j+l) fN(x[j..j+l))                     X in N, J, C
//   bB(j)   = sum_k ent_k bP_k(j)                             products added in rising k: a plain sum
//   bC(j)   = fma(CC, bPC, [j = L] CT)
//   bJ(j)   = fma(JJ, bPJ, JB bB)                             bN(j) = fma(NN, bPN, NB bB)
//   bE(j)   = [j = L] ET, then fma(EB, bB, .), fma(EJ, bPJ, .), fma(EC, bPC, .)
//   g_k     = fma(DM_{k+1}, bP_{k+1}, bE)                     bD_k = fma(DD_{k+1}, bD_{k+1}, g_k)
//   bM_k(j) = bE, then fma(MD_{k+1}, bD_{k+1}, .), fma(MM_{k+1}, bP_{k+1}, .), fma(MI_k, bQ_k, .)
//   bI_k(j) = fma(II_k, bQ_k, IM_{k+1} bP_{k+1})
//
// Exponents.  The rings of bM and bI (rows j + 1 .. j + 5) and of bN, bJ, bC share one exponent per pair.  After a row,
// ref = max(bN, bJ, bC, bB, bE) of that row, and dcp_fws_rescale_by decides as in the Forward sweep: every ring value
// (and the carried bB and bPN) is multiplied by an exact power of two and the exponent follows.  Row L is a row: its ref
// is max(ET, CT), and the rule applies to those two factors before anything reads the ring, so that ET, CT near e^-708
// do not leave rows L and L - 1 in the subnormals.  At the finish row 0's bB and bPN are multiplied by the power of two
// that brings the larger into [1, 2) (band 0), then alt_bwd = fma(SN, bPN, SB bB) and the score is dcp_fws_score's.
//
// Row records.  A row's five values (bN, bJ, bC, bB, bE; PN, PJ, PC, B, E in the row-storing Forward) are written as
// logs, dcp_fws_score(u, s) with the exponent in force: dcp_posterior_row and the combining kernel read them unchanged.
//
// Overflow.  A non-finite bB, bE or new ring value ends the pair (out of range: the log-space sweeps rerun it).
//
// Underflow.  A record value more than 2^(1022 - band) below its row's ref is rounded in the subnormals or flushed to 0,
// and its posterior term exp(f + b - a) is lost.  With F and Bk the largest record values of the two sweeps at row j and
// a the Forward alt score, such a term is below exp(F + Bk - a) 2^-(1022 - band): a pair with
//   F + Bk - a > (958 - band) ln 2                                      (dcp_bws_lossy)
// at any row is out of range too, and for every other pair a lost term is under 2^-64.  DESIGN 25 has the derivation.
#ifndef DCP_BACKWARD_SCALED_H
#define DCP_BACKWARD_SCALED_H

#include "dcp_forward_scaled.h"
#include "dcp_posterior.h"

enum
{
    // rows of ldk doubles in a wavefront's work area of the scaled wide Backward sweep: the log-space sweep's twelve
    // (the rings of bM and bI, the row's bP, bQ), then the profile's eight rows of transition factors
    DCP_BWS_WORK_ROWS = DCP_POST_WORK_ROWS + 8
};

// the largest of a row record's five logs (-inf: the row has no weight at all)
DCP_FWD_HD inline double dcp_bws_rec_max(double const *r)
{
    return dcp_fwd_max(dcp_fwd_max(dcp_fwd_max(r[0], r[1]), dcp_fwd_max(r[2], r[3])), r[4]);
}

// whether a record value that the scaled representation lost at this row could add 2^-64 or more to a posterior
DCP_FWD_HD inline int dcp_bws_lossy(double F, double Bk, double a, int band)
{
    double const ninf = dcp_fwd_ninf();
    if (F == ninf || Bk == ninf || a == ninf) return 0; // nothing passes through this row, or there is no path at all
    return F + Bk - a > (double)(958 - band) * 0.693147180559945309417232121458;
}

#ifdef __cplusplus
extern "C" {
#endif
// The scaled Backward sweep (dcp_backward_scaled.hip): dcp_backward_launch's classes, always with row records (a->rows),
// alt_bwd into a->out_alt.  rows_f: the round's Forward records (the row-storing scaled Forward wrote them), alt_fwd: the
// list's Forward alt scores by pos -- what the underflow check reads.  redo, nredo, redo_cap, band: as
// dcp_forward_scaled_launch.  != 0: no such kernel, a null pointer, a band outside 1 .. 500, a wide sweep whose
// work_stride is no multiple of DCP_BWS_WORK_ROWS, or dcp_fwd_args_refused.
int dcp_backward_scaled_launch(int precision, int R, struct dcp_fwd_args const *a, double const *rows_f, double const *alt_fwd,
                               struct dcp_fwd_pair *redo, uint32_t *nredo, uint32_t redo_cap, int band, void *stream);
#ifdef __cplusplus
}
#endif

#endif
