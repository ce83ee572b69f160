// dcp_f64.h -- the double build's device side (dcp_f64.hip): the resident f64 DB's frame-table expansion and the
// f64 row-sweep kernel, as dcp_gpu.hip drives them.  Internal; the public C-ABI is include/dcp_gpu.h.
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
}
#endif

#endif
