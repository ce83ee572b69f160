// dcp_f64.h -- the double build's device side: the resident f64 DB's frame-table expansion, the f64 row-sweep
// kernel and the traceback (dcp_f64.hip) and the f64 query-lane kernel (dcp_f64_qlane.hip), as dcp_gpu.hip drives
// them.  Internal; the public C-ABI is include/dcp_gpu.h.
#ifndef DCP_F64_H
#define DCP_F64_H

#include "dcp_host.h"

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum
{
    DCP_F64_XSTRIDE = 16, // doubles per sequence in the f64 xtrans array (DCP_X_* order)
    DCP_F64_SEG = 256,    // nodes of one column segment of the wide-profile sweep (64 lanes x 4)
    DCP_F64_QL_KT = 4,    // nodes of one tile of the query-lane kernel (dcp_f64_qlane.hip)
    DCP_F64_QL_LANES = 256, // queries (threads) of one of its blocks
};

// One resident profile of an f64 DB.  Offsets in doubles.
struct dcp_f64_prof
{
    uint64_t tab_off;   // [1364][ldk] match emission table, columns >= core_size are -inf
    uint64_t trans_off; // [8][ldk] trans8 rows (DCP_T_*), columns >= core_size are -inf
    uint64_t xe_off;    // [2][1364]: insert, then null emission table
    uint32_t core_size;
    uint32_t ldk;       // columns: nseg x 64 x R
    uint32_t nseg;      // column segments (1 unless R = 4 and core_size > 256)
    uint32_t pidx;      // caller's index
};

// One column of frame-table expansion: dist (129 doubles at dists + 129 * dist) -> out[code * stride], or a column
// of -inf where dist == ~0u.
struct dcp_f64_expand_job
{
    uint64_t out_off;
    uint32_t dist;
    uint32_t stride;
    double eps;
};

struct dcp_f64_scan_args
{
    dcp_f64_prof const *profs; // this launch's profiles (one nodes-per-lane class)
    unsigned nprof;
    unsigned nprof_total;      // row length of the score matrices
    double const *tab, *trans, *xe;
    uint32_t const *seq_words, *seq_woff, *seq_len; // relative to the scan's first query
    double const *xtrans;                           // [nq][DCP_F64_XSTRIDE]
    unsigned nq, q_base;
    double *out_null, *out_alt; // [nq][nprof_total] from the scan's first query, or NULL
    struct dcp_hit64 *hits;
    unsigned *nhits;
    unsigned hit_cap;
    double lrt_threshold;
    double *col;      // boundary columns of the segmented sweep: col_stride doubles per wavefront of the grid
    uint64_t col_stride;
    unsigned nwaves;  // wavefronts striding over the pairs (set by dcp_f64_launch_scan)
};

void dcp_f64_launch_expand(dcp_f64_expand_job const *jobs, unsigned njobs, double const *dists, double *out,
                           void *stream);
// R = 1, 2 or 4 nodes per lane; nwaves wavefronts stride over the nprof x nq pairs
int dcp_f64_launch_scan(int R, dcp_f64_scan_args const *a, unsigned nwaves, void *stream);

#ifdef __cplusplus
} // extern "C"

// ---- the traceback of the double build -------------------------------------------------------------------------
// One traced pair: its sequence (absolute index) and its entry of the launch's profs[].
struct dcp_f64_pair
{
    uint32_t q;
    uint32_t prof;
};

// The forward pass (viterbi64_kernel<R, TRACE>): the scan's fields, except that seq_woff / seq_len are not offset
// (pairs name absolute queries), xtrans holds one row per pair of the list, and no score, hit or hit count is
// written.  Pair i writes M, I, D of every row j = 0 .. L and column k < ldk as three [L + 1][ldk] double matrices
// at trace_work + trace_woff[i], then N, B, E, J, C as five [L + 1] vectors; its alt score goes to trace_alt[i].
struct dcp_f64_trace_args : dcp_f64_scan_args
{
    dcp_f64_pair const *pairs;
    unsigned npairs;
    double *trace_work;
    uint64_t const *trace_woff;
    double *trace_alt;
};

// The walk back (trace64_kernel): one wavefront per hit of the round, lane 0 walking on the work area the forward
// pass filled; for the null model lane 0 runs the one-state R recursion into the work area itself.
struct dcp_f64_walk_args
{
    dcp_f64_prof const *profs;
    dcp_f64_pair const *pairs; // [nhits]
    unsigned nhits;
    double const *tab, *trans, *xe;
    uint32_t const *seq_words, *seq_woff, *seq_len;
    double const *xtrans;      // [nhits][DCP_F64_XSTRIDE]
    double *work;
    uint64_t const *work_off;  // [nhits] doubles
    struct dcp_step *steps;
    uint32_t const *step_off;  // [nhits + 1]
    uint32_t *nsteps;          // [nhits]: steps of the path (written up to the capacity), or a sentinel below
    double *alt_out;           // [nhits]: the score the walk starts from
    int null_model;
};

enum : uint32_t
{
    DCP_F64_TRACE_NO_PATH = 0xffffffffu, // DCP_TRACE_NO_PATH / DCP_TRACE_TOO_LONG of dcp_kernels.h
    DCP_F64_TRACE_TOO_LONG = 0xfffffffeu,
};

// The pair-list scan (viterbi64_kernel<R, false, true>): the scan's fields with profs the whole resident DB; pair i of
// pairs[0 .. min(*npairs_dev, pair_cap)) names a query relative to the scan's first one and an entry of profs[], and
// is scored, filtered and stored exactly as the grid mode does.  The count is read on the device: the list is the
// query-lane kernel's redo list, filled by the launch before.
struct dcp_f64_pairs_args : dcp_f64_scan_args
{
    dcp_f64_pair const *pairs;
    unsigned const *npairs_dev;
    unsigned pair_cap;
};
int dcp_f64_launch_scan_pairs(int R, dcp_f64_pairs_args const *a, unsigned nwaves, void *stream);

// The query-lane kernel (dcp_f64_qlane.hip): a persistent grid of blocks of DCP_F64_QL_LANES lanes pulling
// (profile, plan block) tasks from *task_counter; task i is profile order[i / nqb] against block i % nqb of the
// batch plan (plan_query_groups, dcp_gpu.hip: the float query-lane kernels' plan with four wavefront slots per
// block).  Wavefront slot s of block b sweeps groups[slot_first[4 b + s] .. slot_first[4 b + s + 1]) one after the
// other per tile, lane l of the slot the query qorder[group.qfirst + l] (relative to the scan's first query,
// ascending length), in rows group.rowbase .. of its own columns of the block's planes.
struct dcp_ql_group; // dcp_kernels.h
struct dcp_f64_qlane_args
{
    dcp_f64_prof const *profs; // the whole resident DB
    uint32_t const *order;     // [nprof] entries of profs, largest core size first
    unsigned nprof_total;
    double const *tab, *trans, *xe;
    uint32_t const *seq_words, *seq_woff, *seq_len; // relative to the scan's first query
    double const *xtrans;                           // [nq][DCP_F64_XSTRIDE]
    uint32_t const *qorder;                         // [nq]
    struct dcp_ql_group const *groups;              // [groups of the plan], in slot order
    uint32_t const *slot_first;                     // [4 nqb + 1]
    unsigned nq, q_base, nqb, ntasks;
    double *out_null, *out_alt;
    struct dcp_hit64 *hits;
    unsigned *nhits;
    unsigned hit_cap;
    double lrt_threshold;
    double *planes;        // plane_stride doubles per block of the grid: [the plan's plane rows][3][DCP_F64_QL_LANES]
    uint64_t plane_stride;
    unsigned *task_counter;
    dcp_f64_pair *redo;    // one list per launch group of the DB, group g at redo_first[g], redo_cap[g] long
    unsigned redo_first[4], redo_cap[4];
    unsigned *redo_n;      // [4] pairs appended (counts on past the capacity), [1] overflow flag
};
void dcp_f64_launch_qlane(dcp_f64_qlane_args const *a, unsigned nblocks, void *stream);

// R = 1, 2 or 4; nwaves wavefronts stride over the a->npairs pairs (one boundary column each where a->col is set)
int dcp_f64_launch_trace_forward(int R, dcp_f64_trace_args const *a, unsigned nwaves, void *stream);
void dcp_f64_launch_walk(dcp_f64_walk_args const *a, void *stream);
#endif

#endif
