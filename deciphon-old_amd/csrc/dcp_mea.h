// dcp_mea.h -- the posterior-decoded (maximum expected accuracy) alignment of a pair list (dcp_gpu_mea_pairs): what the
// kernels (dcp_mea.hip) and the host twin (dcp_mea_tables, dcp_mea_path_gain; dcp_model.cpp) share -- the word
// posteriors, the order of the candidates of every state, the choice codes the sweep parks and the walk that reads them.
//
// Notation: dcp_posterior.h's.  a is the Forward alt score.  For a word x[s .. s+l), 1 <= l <= 5, s + l <= L:
//
//   wM_k(s,l) = exp(P_k(s) + eM_k(x[s..s+l)) + bM_k(s+l) - a)      wI_k(s,l) = exp(Q_k(s) + eI(..) + bI_k(s+l) - a)
//   wX(s,l)   = exp(PX(s)  + eN(x[s..s+l))   + bX(s+l)   - a)      X = N, J, C
//
// each by dcp_post_prob.  The gain of a path is the sum of l w over its emitting steps; the decoded path is an S .. T
// path over finite transitions and emissions only that emits L bases and has the largest gain.  The sweep runs in the
// Backward direction: g of a state at row j is the best gain of a path suffix from it to T at row L (-inf: none).
// A transition t is a link: it passes g if t is finite, -inf otherwise.  A word's candidate is g(s + l) + l w, formed
// once, -inf if its emission is -inf.  Candidates are taken in the order written, by strict >, from (-inf, code 0):
//
//   gP_k(j) = max_l   l = 1 .. 5:  gM_k(j+l) + l wM_k(j,l)                                   code l
//   gQ_k(j), gPX(j)   the same over gI_k, wI_k and gX, wX
//   gB(j)   = max_k   k rising:    [entry_k] gP_k(j)                                         code k + 1
//   gC(j)   = max([j = L][CT] 0, [CC] gPC(j))                                                codes 1, 2
//   gJ(j)   = max([JB] gB(j), [JJ] gPJ(j))          gN(j) = max([NB] gB(j), [NN] gPN(j))     codes 1, 2
//   gE(j)   = max([j = L][ET] 0, [EB] gB(j), [EJ] gPJ(j), [EC] gPC(j))                       codes 1 .. 4
//   gD_k(j) = max(gE(j), [DD_{k+1}] gD_{k+1}(j), [DM_{k+1}] gP_{k+1}(j))                     codes 1 .. 3
//   gM_k(j) = max(gE(j), [MD_{k+1}] gD_{k+1}(j), [MM_{k+1}] gP_{k+1}(j), [MI_k] gQ_k(j))     codes 1 .. 4
//   gI_k(j) = max([IM_{k+1}] gP_{k+1}(j), [II_k] gQ_k(j))                                    codes 1, 2
//   gain    = max([SB] gB(0), [SN] gPN(0))                                                   codes 1, 2
//
// max is exact, so host and device differ only in the posteriors they start from (exp, log and the association of the
// two sweeps' sums); among near-equal candidates they may choose differently.
#ifndef DCP_MEA_H
#define DCP_MEA_H

#include "dcp_posterior.h"

enum
{
    DCP_MEA_WORK_ROWS = 12, // the sweep's work area: the rings of gM and gI (5 each), the row's gP, gQ
    DCP_MEA_ROWC = 2        // 32-bit words of a row's choices
};

// A cell's choices, 13 bits: P's word (3), Q's word (3), then M (3), I (2), D (2).
// A row's: word 0 = PN's, PJ's, PC's words (3 bits each), then N, J, C (2 each), E (3); word 1 = B's code.
enum
{
    DCP_MEA_SH_P = 0, DCP_MEA_SH_Q = 3, DCP_MEA_SH_M = 6, DCP_MEA_SH_I = 9, DCP_MEA_SH_D = 11,
    DCP_MEA_SH_PN = 0, DCP_MEA_SH_PJ = 3, DCP_MEA_SH_PC = 6, DCP_MEA_SH_N = 9, DCP_MEA_SH_J = 11, DCP_MEA_SH_C = 13,
    DCP_MEA_SH_E = 15
};

struct dcp_mea_best
{
    double g;
    unsigned c;
};
DCP_FWD_HD inline dcp_mea_best dcp_mea_none() { return dcp_mea_best{dcp_fwd_ninf(), 0u}; }
DCP_FWD_HD inline void dcp_mea_take(dcp_mea_best &b, double cand, unsigned code)
{
    if (cand > b.g) b.g = cand, b.c = code;
}
DCP_FWD_HD inline double dcp_mea_link(double t, double g) { return t == dcp_fwd_ninf() ? dcp_fwd_ninf() : g; }

// the candidate of the word of l bases: f the Forward value it leaves from, e its emission, b the Backward value and g
// the suffix gain of where it arrives
DCP_FWD_HD inline double dcp_mea_word(double f, double e, double b, double a, unsigned l, double g)
{
    if (e == dcp_fwd_ninf()) return dcp_fwd_ninf();
    double const lw = (double)l * dcp_post_prob(f + e, b, a);
    return g + lw;
}

// the states but the words and B, whose candidates each side forms in its own loops
DCP_FWD_HD inline dcp_mea_best dcp_mea_c(bool last, double CT, double CC, double gPC)
{
    dcp_mea_best b = dcp_mea_none();
    if (last) dcp_mea_take(b, dcp_mea_link(CT, 0.0), 1u);
    dcp_mea_take(b, dcp_mea_link(CC, gPC), 2u);
    return b;
}
DCP_FWD_HD inline dcp_mea_best dcp_mea_nj(double XB, double XX, double gB, double gPX) // N and J; S with SB, SN
{
    dcp_mea_best b = dcp_mea_none();
    dcp_mea_take(b, dcp_mea_link(XB, gB), 1u);
    dcp_mea_take(b, dcp_mea_link(XX, gPX), 2u);
    return b;
}
DCP_FWD_HD inline dcp_mea_best dcp_mea_e(bool last, double ET, double EB, double EJ, double EC, double gB, double gPJ, double gPC)
{
    dcp_mea_best b = dcp_mea_none();
    if (last) dcp_mea_take(b, dcp_mea_link(ET, 0.0), 1u);
    dcp_mea_take(b, dcp_mea_link(EB, gB), 2u);
    dcp_mea_take(b, dcp_mea_link(EJ, gPJ), 3u);
    dcp_mea_take(b, dcp_mea_link(EC, gPC), 4u);
    return b;
}
DCP_FWD_HD inline dcp_mea_best dcp_mea_d(double gE, double DDn, double DMn, double gDn, double gPn)
{
    dcp_mea_best b = dcp_mea_none();
    dcp_mea_take(b, gE, 1u);
    dcp_mea_take(b, dcp_mea_link(DDn, gDn), 2u);
    dcp_mea_take(b, dcp_mea_link(DMn, gPn), 3u);
    return b;
}
DCP_FWD_HD inline dcp_mea_best dcp_mea_m(double gE, double MDn, double MMn, double MI, double gDn, double gPn, double gQ)
{
    dcp_mea_best b = dcp_mea_none();
    dcp_mea_take(b, gE, 1u);
    dcp_mea_take(b, dcp_mea_link(MDn, gDn), 2u);
    dcp_mea_take(b, dcp_mea_link(MMn, gPn), 3u);
    dcp_mea_take(b, dcp_mea_link(MI, gQ), 4u);
    return b;
}
DCP_FWD_HD inline dcp_mea_best dcp_mea_i(double IMn, double II, double gPn, double gQ)
{
    dcp_mea_best b = dcp_mea_none();
    dcp_mea_take(b, dcp_mea_link(IMn, gPn), 1u);
    dcp_mea_take(b, dcp_mea_link(II, gQ), 2u);
    return b;
}

// ---- the walk ---------------------------------------------------------------------------------------------------------
// One pair's matrices and choices, rows j = 0 .. L of ldm cells each (node k at column k - 1), the two sweeps' records
// and the profile's tables.  Seq: base i of the sequence by operator().
template <class Real> struct dcp_mea_view
{
    unsigned M, L;
    uint64_t ldm;
    double const *P, *Q, *bM, *bI; // the Forward sweep's P, Q and the Backward sweep's bM, bI
    uint16_t const *cell;
    uint32_t const *rowc;          // DCP_MEA_ROWC words a row
    double const *fr, *br;         // DCP_POST_REC doubles a row
    Real const *em, *ei, *en;      // match table (row `code` is ld further each), insert and null tables
    uint64_t ld;
};

template <class Seq> DCP_FWD_HD inline unsigned dcp_mea_code(Seq const &x, unsigned s, unsigned l)
{
    unsigned v = 0;
    for (unsigned i = 0; i < l; ++i)
        v = (v << 2) | (unsigned)x(s + i);
    return (l == 1u ? 0u : l == 2u ? 4u : l == 3u ? 20u : l == 4u ? 84u : 340u) + v;
}

// The path from S (start: S's code) to T in the step format dcp_gpu_trace_paths writes: steps[i] = state_id |
// seqlen << 16 and post[i] (may be null) the word posterior of an emitting step, -1 of a silent one, for i < cap.
// Returns the number of steps, counted past cap; 0 if start is 0 or a choice is missing where one is needed.
template <class Real, class Seq>
DCP_FWD_HD inline uint64_t dcp_mea_walk(dcp_mea_view<Real> const &v, Seq const &x, double a, unsigned start, uint32_t *steps,
                                        double *post, uint64_t cap)
{
    enum { PN, PJ, PC, XN, XJ, XC, SB, SP, SQ, SM, SI, SD, SE, ST, STOP };
    unsigned const EXT = 3u << 14;
    uint64_t n = 0;
    auto push = [&](unsigned id, unsigned len, double w) {
        if (n < cap)
        {
            steps[n] = id | (len << 16);
            if (post) post[n] = w;
        }
        ++n;
    };
    if (start == 0u) return 0u;
    push(EXT | 1u, 0u, -1.0);
    int st = start == 1u ? SB : PN;
    unsigned j = 0, k = 0;
    bool ok = true;
    // a path has at most L emitting steps and, per domain (at most L of them), M + 1 silent core steps and B, E
    uint64_t const max_steps = ((uint64_t)v.L + 1u) * (v.M + 4u) + 64u;
    while (st != STOP && n <= max_steps)
    {
        uint32_t const rc = v.rowc[(uint64_t)DCP_MEA_ROWC * j];
        unsigned const cc = st >= SP && st <= SD ? v.cell[(uint64_t)j * v.ldm + k] : 0u;
        if (st == PN || st == PJ || st == PC)
        {
            unsigned const X = (unsigned)(st - PN), l = (rc >> (3u * X)) & 7u;
            if (l == 0u || j + l > v.L) { ok = false; break; }
            double const f = v.fr[(uint64_t)DCP_POST_REC * j + X] + (double)v.en[dcp_mea_code(x, j, l)];
            push(EXT | (X == 0u ? 2u : X == 1u ? 5u : 6u), l, dcp_post_prob(f, v.br[(uint64_t)DCP_POST_REC * (j + l) + X], a));
            j += l;
            st = XN + (int)X;
        }
        else if (st == XN || st == XJ)
        {
            unsigned const c = (rc >> (st == XN ? DCP_MEA_SH_N : DCP_MEA_SH_J)) & 3u;
            if (c == 0u || c > 2u) { ok = false; break; }
            st = c == 1u ? SB : st == XN ? PN : PJ;
        }
        else if (st == XC)
        {
            unsigned const c = (rc >> DCP_MEA_SH_C) & 3u;
            if (c == 0u || c > 2u) { ok = false; break; }
            st = c == 1u ? ST : PC;
        }
        else if (st == SB)
        {
            push(EXT | 3u, 0u, -1.0);
            unsigned const c = v.rowc[(uint64_t)DCP_MEA_ROWC * j + 1u];
            if (c == 0u || c > v.M) { ok = false; break; }
            k = c - 1u;
            st = SP;
        }
        else if (st == SP || st == SQ)
        {
            bool const m = st == SP;
            unsigned const l = (cc >> (m ? DCP_MEA_SH_P : DCP_MEA_SH_Q)) & 7u;
            if (l == 0u || j + l > v.L) { ok = false; break; }
            unsigned const code = dcp_mea_code(x, j, l);
            uint64_t const from = (uint64_t)j * v.ldm + k, to = (uint64_t)(j + l) * v.ldm + k;
            double const f = m ? v.P[from] + (double)v.em[(uint64_t)code * v.ld + k] : v.Q[from] + (double)v.ei[code];
            push((m ? 0u : 1u << 14) | (k + 1u), l, dcp_post_prob(f, m ? v.bM[to] : v.bI[to], a));
            j += l;
            st = m ? SM : SI;
        }
        else if (st == SM)
        {
            unsigned const c = (cc >> DCP_MEA_SH_M) & 7u;
            if (c == 0u || c > 4u || (c != 1u && c != 4u && k + 1u >= v.M)) { ok = false; break; }
            if (c == 2u || c == 3u) ++k;
            st = c == 1u ? SE : c == 2u ? SD : c == 3u ? SP : SQ;
        }
        else if (st == SI)
        {
            unsigned const c = (cc >> DCP_MEA_SH_I) & 3u;
            if (c == 0u || c > 2u || (c == 1u && k + 1u >= v.M)) { ok = false; break; }
            if (c == 1u) ++k;
            st = c == 1u ? SP : SQ;
        }
        else if (st == SD)
        {
            push((2u << 14) | (k + 1u), 0u, -1.0);
            unsigned const c = (cc >> DCP_MEA_SH_D) & 3u;
            if (c == 0u || (c != 1u && k + 1u >= v.M)) { ok = false; break; }
            if (c != 1u) ++k;
            st = c == 1u ? SE : c == 2u ? SD : SP;
        }
        else if (st == SE)
        {
            push(EXT | 4u, 0u, -1.0);
            unsigned const c = (rc >> DCP_MEA_SH_E) & 7u;
            if (c == 0u || c > 4u) { ok = false; break; }
            st = c == 1u ? ST : c == 2u ? SB : c == 3u ? PJ : PC;
        }
        else // ST
        {
            push(EXT | 7u, 0u, -1.0);
            if (j != v.L) ok = false;
            st = STOP;
        }
    }
    return ok && st == STOP ? n : 0u;
}

// ---- the kernels' arguments (dcp_mea.hip, driven by dcp_gpu_mea_pairs in dcp_gpu.hip) --------------------------------
// The two sweeps' matrix-storing variants take dcp_fwd_args (mat0, mat1, cell_off, cell_base).  The max-plus sweep and
// the walk: the round's pairs in list order, one wavefront striding over them.
struct dcp_mea_args
{
    dcp_fwd_prof const *profs;
    void const *tab, *trans, *ei, *en; // float or double, as the launcher's `precision` says
    uint32_t const *seq_words, *seq_woff, *seq_len;
    double const *xtrans;      // [nseqs][DCP_FWD_XSTRIDE]
    dcp_fwd_pair const *list;  // the round's pairs in list order
    unsigned nlist, nwaves;
    uint64_t const *row_off;   // [nlist + 1] from the round's first pair on: rows, for the records and the row choices
    uint64_t const *cell_off;  // [nlist + 1] likewise: cells, for the matrices and the cell choices
    double const *P, *Q, *bM, *bI; // the round's matrices
    double const *rows_f, *rows_b; // the round's records
    uint16_t *cell;
    uint32_t *rowc;
    double *work;              // the sweep: work_stride doubles per wavefront
    uint64_t work_stride;      // DCP_MEA_WORK_ROWS x the round's widest profile, padded to chunks
    double const *alt_fwd;     // [the caller's list], by the pair's pos
    double *gain;              // [the caller's list], by the pair's pos
    uint32_t *start;           // [nlist]: S's code, the sweep's word to the walk
    // the walk
    uint32_t *steps;           // the round's steps, pair i's from step_at[i] on, at most step_cap[i] of them
    double *post;
    uint64_t const *step_at;   // [nlist]
    uint64_t const *step_cap;  // [nlist]
    uint64_t *nsteps;          // [nlist]: the true counts
};

#ifdef __cplusplus
extern "C" {
#endif
// (the two sweeps: dcp_forward_launch and dcp_backward_launch with DCP_FWD_STORE_MATS, dcp_forward.h)
// precision 32 / 64 as there.  != 0: no such kernel.
int dcp_mea_sweep_launch(int precision, struct dcp_mea_args const *a, void *stream);
int dcp_mea_walk_launch(int precision, struct dcp_mea_args const *a, void *stream);
#ifdef __cplusplus
}
#endif

#endif
