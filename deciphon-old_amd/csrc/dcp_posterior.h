// dcp_posterior.h -- what the Backward sweep and the posterior rows of a pair list (dcp_gpu_posterior_pairs) share
// between the kernels (dcp_posterior.hip, dcp_forward.hip's row-storing variant) and the host twin
// (dcp_posterior_tables, dcp_model.cpp): the row records, the word codes read forward, and the one rule that turns the
// two sweeps' special-state rows into begin[j], end[j], core[j].  Every combiner is the lse of dcp_forward.h.
//
// Notation (DESIGN sections 2, 19, 20): M_k(j), I_k(j), D_k(j), N, J, C, E, B are values after emission at row j;
// P_k(j), Q_k(j), PN(j), PJ(j), PC(j) the pre-emission values a word starting after row j leaves from.  beta of a state
// at row j is the log of the summed weight of all path suffixes from it to T at row L; rows run j = L .. 0:
//
//   bP_k(j) = lse_{l=1..5} eM_k(x[j..j+l)) + bM_k(j+l)        bQ_k(j) = lse_l eI(x[j..j+l)) + bI_k(j+l)
//   bPX(j)  = lse_l eN(x[j..j+l)) + bX(j+l)                   X in N, J, C
//   bB(j)   = lse_k entry_k + bP_k(j)
//   bC(j)   = lse([j = L] CT, CC + bPC(j))
//   bJ(j)   = lse(JB + bB(j), JJ + bPJ(j))                    bN(j) = lse(NB + bB(j), NN + bPN(j))
//   bE(j)   = lse([j = L] ET, EB + bB(j), EJ + bPJ(j), EC + bPC(j))
//   bD_k(j) = lse(bE(j), DD_{k+1} + bD_{k+1}(j), DM_{k+1} + bP_{k+1}(j))
//   bM_k(j) = lse(bE(j), MD_{k+1} + bD_{k+1}(j), MM_{k+1} + bP_{k+1}(j), MI_k + bQ_k(j))
//   bI_k(j) = lse(IM_{k+1} + bP_{k+1}(j), II_k + bQ_k(j))
//   alt_bwd = lse(SB + bB(0), SN + bPN(0))
//
// A term that does not exist is -inf: a word that would end past L, node k + 1 = M, ET and CT at j < L.
#ifndef DCP_POSTERIOR_H
#define DCP_POSTERIOR_H

#include "dcp_forward.h"

enum
{
    DCP_POST_REC = 5,       // doubles of a row record.  Forward: PN, PJ, PC, B, E; Backward: bN, bJ, bC, bB, bE
    DCP_POST_WORK_ROWS = 12 // the wide Backward sweep's work area: the rings of bM and bI (5 each), the row's bP, bQ
};

// exp(f + b - a): the posterior of passing through a state whose Forward value is f and whose Backward value is b, a
// the Forward alt score.  No operand is +inf or NaN; an empty sum (or a = -inf: no path at all) is 0, never NaN.
DCP_FWD_HD inline double dcp_post_prob(double f, double b, double a)
{
    double const s = f + b;
    if (a == dcp_fwd_ninf() || s == dcp_fwd_ninf()) return 0.0;
    return exp(s - a);
}

// Code of the word x[s .. s+l) among the nine bases x[j-5 .. j+4) around row j, packed in `win` first base most
// significant (base j - 5 + i in bits 2 (8 - i)); j - 5 <= s, s + l <= j + 4.
DCP_FWD_HD inline unsigned dcp_post_word(unsigned win, unsigned i0, unsigned l)
{
    unsigned const off = l == 1u ? 0u : l == 2u ? 4u : l == 3u ? 20u : l == 4u ? 84u : 340u;
    return off + ((win >> (2u * (9u - i0 - l))) & ((1u << (2u * l)) - 1u));
}

// Row j = 0 .. L of one pair.  fr, br: the pair's Forward and Backward records from row 0 on; en: the null table.
//   begin[j] = exp(B(j) + bB(j) - a)      end[j] = exp(E(j) + bE(j) - a)
//   wX(s,l)  = exp(PX(s) + eN(x[s..s+l)) + bX(s+l) - a)
//   core[j]  = 1 - sum_X sum_{(s,l): s < j <= s+l} wX(s,l),  X = N, J, C, then s rising, then l rising;  core[0] = 0
// the posterior that base j - 1 is emitted by a core state: every base is emitted by exactly one word of one state.
template <class Real>
DCP_FWD_HD inline void dcp_posterior_row(double const *fr, double const *br, Real const *en, unsigned win, unsigned j,
                                         unsigned L, double a, double *begin, double *end, double *core)
{
    double const *f = fr + (uint64_t)DCP_POST_REC * j, *b = br + (uint64_t)DCP_POST_REC * j;
    *begin = dcp_post_prob(f[3], b[3], a);
    *end = j ? dcp_post_prob(f[4], b[4], a) : 0.0;
    if (j == 0u || a == dcp_fwd_ninf())
    {
        *core = 0.0;
        return;
    }
    double sum = 0.0;
    for (unsigned X = 0; X < 3u; ++X)
        for (unsigned s = j > 5u ? j - 5u : 0u; s < j; ++s)
            for (unsigned l = j - s; l <= 5u && s + l <= L; ++l)
            {
                double const eN = (double)en[dcp_post_word(win, s + 5u - j, l)];
                sum += dcp_post_prob(fr[(uint64_t)DCP_POST_REC * s + X] + eN, br[(uint64_t)DCP_POST_REC * (s + l) + X], a);
            }
    *core = 1.0 - sum;
}

// ---- the kernels' arguments (dcp_posterior.hip, driven by dcp_gpu_posterior_pairs in dcp_gpu.hip) -------------------
// The Backward launches take the Forward launches' dcp_fwd_args: out_alt receives alt_bwd (out_null is not written),
// rows the Backward records.  The combining kernel: one thread per row of the round's pairs in list order.
struct dcp_post_args
{
    dcp_fwd_prof const *profs;
    void const *en;            // null tables, the DB's scalar
    uint32_t const *seq_words, *seq_woff, *seq_len;
    dcp_fwd_pair const *list;  // the round's pairs in list order
    uint64_t const *row_off;   // [nlist + 1] from the round's first pair on: pair i's rows start at row_off[i] - row_off[0]
    unsigned nlist;
    double const *rows_f, *rows_b; // the round's records
    double const *alt_fwd;         // [the caller's list], by the pair's pos
    double *begin, *end, *core;    // the round's rows
};

#ifdef __cplusplus
extern "C" {
#endif
// (the two sweeps: dcp_forward_launch and dcp_backward_launch with DCP_FWD_STORE_ROWS, dcp_forward.h)
// precision 32 / 64 as there; total_rows: the round's rows, row_off[nlist] - row_off[0].  != 0: no such kernel.
int dcp_posterior_combine_launch(int precision, struct dcp_post_args const *a, uint64_t total_rows, void *stream);
#ifdef __cplusplus
}
#endif

#endif
