// dcp_forward.h -- the Forward recursion's one rule, log-sum-exp, as the kernel (dcp_forward.hip) and its host twin
// (dcp_forward_tables, dcp_model.cpp) both evaluate it, and the argument blocks of the kernel's launcher.  One source
// for both sides, as dcp_calib.h:
//
//   lse(c_1 .. c_n):  m = max_i c_i,  mm = (m is -inf) ? 0 : m,  lse = mm + log(sum_i exp(c_i - mm))
//
// with the terms added in index order.  All -inf gives 0 + log(0) = -inf and no inf - inf is ever formed; a single
// finite candidate keeps its bits (exp(0) = 1, log(1) = 0).  No input is +inf or NaN.  With no contraction
// (-ffp-contract=off in both units) host and device differ only in exp and log.
#ifndef DCP_FORWARD_H
#define DCP_FORWARD_H

#include <math.h>
#include <stdint.h>

#ifdef __HIP__
#define DCP_FWD_HD __host__ __device__
#else
#define DCP_FWD_HD
#endif

DCP_FWD_HD inline double dcp_fwd_ninf() { return -__builtin_inf(); }
DCP_FWD_HD inline double dcp_fwd_max(double a, double b) { return a > b ? a : b; }
DCP_FWD_HD inline double dcp_fwd_shift(double m) { return m == dcp_fwd_ninf() ? 0.0 : m; }

// Two operands: the larger one's term is exp(0) = 1 and the sum of two terms does not depend on their order, so
// m + log(1 + exp(n - m)), n the smaller one, has the definition's bits with one exp less.  The delete chain, Q and the
// special states' rings are made of these.
DCP_FWD_HD inline double dcp_lse2(double a, double b)
{
    double const m = dcp_fwd_max(a, b), n = a > b ? b : a;
    if (m == dcp_fwd_ninf()) return m;
    return m + log(1.0 + exp(n - m));
}
DCP_FWD_HD inline double dcp_lse3(double a, double b, double c)
{
    double const mm = dcp_fwd_shift(dcp_fwd_max(dcp_fwd_max(a, b), c));
    return mm + log(exp(a - mm) + exp(b - mm) + exp(c - mm));
}
DCP_FWD_HD inline double dcp_lse4(double a, double b, double c, double d)
{
    double const mm = dcp_fwd_shift(dcp_fwd_max(dcp_fwd_max(a, b), dcp_fwd_max(c, d)));
    return mm + log(exp(a - mm) + exp(b - mm) + exp(c - mm) + exp(d - mm));
}
DCP_FWD_HD inline double dcp_lse5(double a, double b, double c, double d, double e)
{
    double const mm = dcp_fwd_shift(dcp_fwd_max(dcp_fwd_max(dcp_fwd_max(a, b), dcp_fwd_max(c, d)), e));
    return mm + log(exp(a - mm) + exp(b - mm) + exp(c - mm) + exp(d - mm) + exp(e - mm));
}

// The running form: (m, s) stands for m + log(s), s scaled by the largest term so far; (-inf, 0) is the empty sum.
// It is what carries E(j) from lane to lane and from chunk to chunk on the device; it differs from the definition
// above in where the scaling happens, not in which terms are added.
struct dcp_lse_acc
{
    double m, s;
};
DCP_FWD_HD inline dcp_lse_acc dcp_lse_acc_empty() { return dcp_lse_acc{dcp_fwd_ninf(), 0.0}; }
DCP_FWD_HD inline dcp_lse_acc dcp_lse_acc_add(dcp_lse_acc a, double c)
{
    if (c > a.m)
    {
        a.s = (a.m == dcp_fwd_ninf() ? 0.0 : a.s * exp(a.m - c)) + 1.0;
        a.m = c;
    }
    else if (c != dcp_fwd_ninf()) a.s += exp(c - a.m); // c <= m and finite: m is finite
    return a;
}
DCP_FWD_HD inline dcp_lse_acc dcp_lse_acc_merge(dcp_lse_acc a, dcp_lse_acc b)
{
    if (b.m > a.m)
    {
        dcp_lse_acc const t = a;
        a = b, b = t;
    }
    if (b.m != dcp_fwd_ninf()) a.s += b.s * exp(b.m - a.m);
    return a;
}
DCP_FWD_HD inline double dcp_lse_acc_value(dcp_lse_acc a) { return a.m == dcp_fwd_ninf() ? a.m : a.m + log(a.s); }

// ---- the kernel's arguments (dcp_forward.hip, driven by dcp_gpu_forward_pairs in dcp_gpu.hip) ----------------------
enum
{
    DCP_FWD_XSTRIDE = 16,  // doubles per sequence in the launch's special transitions (DCP_X_* order)
    DCP_FWD_CHUNK = 256,   // columns of one chunk of the wide-profile sweep (64 lanes x 4)
    DCP_FWD_WORK_ROWS = 13 // rows of ldk doubles in a wavefront's work area: P and Q rings (5 each), M, I, D
};

// One resident profile as the kernel addresses it, by the caller's index.  Offsets in table scalars: a float DB's
// small profiles share table rows (dcp_mp_group), so a profile is a base, a row stride and its own core_size columns;
// the kernel never reads a column >= core_size.
struct dcp_fwd_prof
{
    uint64_t tab_off;   // first column of the match table's row 0; row `code` is ld further each
    uint64_t trans_off; // first column of trans8 row 0; the same stride
    uint64_t ei_off, en_off; // insert and null tables [1364]
    uint32_t core_size;
    uint32_t ld;
};

struct dcp_fwd_pair
{
    uint32_t q;    // resident sequence
    uint32_t prof; // caller's profile index
    uint32_t pos;  // position in the caller's list: where the two scores go
};

struct dcp_fwd_args
{
    dcp_fwd_prof const *profs;
    void const *tab, *trans, *ei, *en; // float or double, as the launcher's `precision` says
    uint32_t const *seq_words, *seq_woff, *seq_len;
    double const *xtrans; // [nseqs][DCP_FWD_XSTRIDE]
    dcp_fwd_pair const *pairs;
    unsigned npairs;
    unsigned nwaves;      // wavefronts striding over the pairs
    double *work;         // the wide sweep: work_stride doubles per wavefront
    uint64_t work_stride; // DCP_FWD_WORK_ROWS x the widest listed profile's padded columns
    double *out_null, *out_alt; // [the caller's list]
    // the row-storing Forward variant and the Backward sweep only (dcp_posterior.h): pair `pos` has its DCP_POST_REC
    // doubles per row j = 0 .. L from rows + (row_off[pos] - row_base) * DCP_POST_REC on
    double *rows;
    uint64_t const *row_off; // [the caller's list + 1]
    uint64_t row_base;       // row_off of the round's first pair
    // the matrix-storing variants of the two sweeps only (dcp_mea.h): pair `pos` has rows j = 0 .. L of core_size
    // doubles each from mat0 / mat1 + (cell_off[pos] - cell_base) on -- P and Q of the Forward sweep, bM and bI of the
    // Backward sweep
    double *mat0, *mat1;
    uint64_t const *cell_off; // [the caller's list + 1]
    uint64_t cell_base;       // cell_off of the round's first pair
};

// What a sweep leaves beside its scores: nothing (dcp_gpu_forward_pairs), every row's record (dcp_gpu_posterior_pairs),
// or the records and the two matrices of every row (dcp_gpu_mea_pairs).
enum
{
    DCP_FWD_STORE_NONE = 0,
    DCP_FWD_STORE_ROWS = 1, // rows, row_off, row_base
    DCP_FWD_STORE_MATS = 2  // and mat0, mat1, cell_off, cell_base
};

// What a launch refuses: no work, a wide sweep without its work area, or a pointer missing that `store` writes through.
static inline int dcp_fwd_args_refused(struct dcp_fwd_args const *a, int R, int store)
{
    if (store < DCP_FWD_STORE_NONE || store > DCP_FWD_STORE_MATS) return 1;
    if (!a || a->nwaves == 0 || a->npairs == 0) return 1;
    if (R == 0 && !a->work) return 1;
    if (store >= DCP_FWD_STORE_ROWS && (!a->rows || !a->row_off)) return 1;
    if (store >= DCP_FWD_STORE_MATS && (!a->mat0 || !a->mat1 || !a->cell_off)) return 1;
    return 0;
}

// The dense Forward scan's lists (dcp_gpu_forward_dense): every resident sequence against every resident profile, the
// records written on the device.  The outer product in one line: the profiles' classes one after the other (class k
// holds the profiles prof_order[class_first[k] .. class_first[k + 1]) and the line's positions [nseqs class_first[k],
// nseqs class_first[k + 1])), within a class sequence-major -- position nseqs class_first[k] + s np + i, np the class's
// profiles, is (seq_order[s], prof_order[class_first[k] + i]).  A round is positions [t0, t0 + n) of the line: its
// records go to pairs[0 .. n), so a round's classes lie back to back as the sweeps' launches take them.  pos = q nprof +
// prof, the dense layout; nseqs nprof fits 32 bits (the caller checks), so every index here does.
struct dcp_fwd_dense_args
{
    uint32_t const *seq_order;  // [nseqs]
    uint32_t const *prof_order; // [nprof]
    uint32_t class_first[5];
    uint32_t nseqs, nprof;
    uint32_t t0, n;
    dcp_fwd_pair *pairs; // [n]
};

#ifdef __cplusplus
extern "C" {
#endif
// The records of one round of the dense scan, one thread per record: one launch on `stream`.  != 0: nothing to write, a
// null pointer, or a round that reaches past the line's end.
int dcp_forward_dense_pairs_launch(struct dcp_fwd_dense_args const *a, void *stream);
// The Forward sweep (dcp_forward.hip) and the Backward sweep (dcp_posterior.hip; there is none that stores nothing).
// precision 32 / 64: the tables' scalar.  R = 1, 2 or 4 nodes per lane with the profile in registers (core sizes up to
// 64 R), or R = 0: the wide sweep in chunks of DCP_FWD_CHUNK columns through the work area.  store: DCP_FWD_STORE_*.
// != 0: no such kernel, or dcp_fwd_args_refused.
int dcp_forward_launch(int precision, int R, int store, struct dcp_fwd_args const *a, void *stream);
int dcp_backward_launch(int precision, int R, int store, struct dcp_fwd_args const *a, void *stream);
#ifdef __cplusplus
}
#endif

#endif
