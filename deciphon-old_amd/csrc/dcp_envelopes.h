// dcp_envelopes.h -- the rule that turns a pair's posterior rows (dcp_posterior.h: begin[j], end[j], core[j], j = 0 .. L,
// base i at core[i + 1]) into envelope records (struct dcp_envelope, include/dcp_gpu.h), shared between the kernels
// (dcp_envelopes.hip, driven by dcp_gpu_envelope_pairs in dcp_gpu.hip) and the host twin
// (dcp_posterior_envelope_records, dcp_model.cpp).
//
// An envelope is a maximal run [b, e) of bases with core[i + 1] >= lo; it is kept if e - b >= min_len and the largest
// core value of the run is >= hi.  A NaN is below every threshold: it is in no run.  What base i adds to its run:
//   core_sum += core[i + 1]     begin_sum += begin[i]     end_sum += end[i + 1]
// so that begin_sum covers rows b .. e - 1 and end_sum rows b + 1 .. e.  peak is the first base of the run whose value
// equals the largest (-0.0 == 0.0), core_max that base's own value: both are decided by comparisons alone, whatever the
// order in which pieces of a run are looked at, as long as a later piece replaces the maximum only where it is greater.
// The host twin takes the bases one by one; a wavefront takes a run in pieces of at most 64 bases, each piece reduced
// over its own lanes (masked reductions: no term of another run enters a sum), the pieces merged in order by
// dcp_env_run_add.  The sums therefore differ in association only.
#ifndef DCP_ENVELOPES_H
#define DCP_ENVELOPES_H

#include "dcp_gpu.h"

#ifdef __HIP__
#define DCP_ENV_HD __host__ __device__
#else
#define DCP_ENV_HD
#endif

// a run while it is open: where it began, its largest value and where that first stood, the three sums so far
struct dcp_env_run
{
    unsigned begin, peak;
    double core_max, core_sum, begin_sum, end_sum;
};

// is a base with this core value part of a run?  (false for NaN)
DCP_ENV_HD inline bool dcp_env_in(double core, double lo) { return core >= lo; }

// (a run opens with its first piece: dcp_env_run{first base, the piece's peak, its largest value, its three sums})
// the next piece of an open run, all of whose bases lie behind the run's so far
DCP_ENV_HD inline void dcp_env_run_add(dcp_env_run &r, unsigned peak, double core_max, double core_sum, double begin_sum,
                                       double end_sum)
{
    if (core_max > r.core_max) r.core_max = core_max, r.peak = peak;
    r.core_sum = r.core_sum + core_sum;
    r.begin_sum = r.begin_sum + begin_sum;
    r.end_sum = r.end_sum + end_sum;
}

// is the run that ends before base `end` kept?
DCP_ENV_HD inline bool dcp_env_kept(unsigned begin, unsigned end, double core_max, double hi, unsigned min_len)
{
    return end - begin >= min_len && core_max >= hi;
}

DCP_ENV_HD inline dcp_envelope dcp_env_record(dcp_env_run const &r, unsigned pair, unsigned end)
{
    return dcp_envelope{pair, r.begin, end, r.peak, r.core_max, r.core_sum, r.begin_sum, r.end_sum};
}

// the thresholds every entry point refuses alike: a NaN, or lo > hi.  (By its bits: dcp_gpu.hip is built with
// -fno-honor-nans, where x != x is folded away.)
inline bool dcp_env_is_nan(double x)
{
    uint64_t b;
    __builtin_memcpy(&b, &x, sizeof b);
    return (b & 0x7fffffffffffffffull) > 0x7ff0000000000000ull;
}
inline bool dcp_env_thresholds_refused(double hi, double lo) { return dcp_env_is_nan(hi) || dcp_env_is_nan(lo) || lo > hi; }

// ---- the kernels' arguments (dcp_envelopes.hip) ----------------------------------------------------------------------
// A round's rows as the combining kernel leaves them (dcp_post_args): three planes, pair i's first row at
// row_off[i] - row_off[0], L_i + 1 rows.  One wavefront per pair, nwaves wavefronts striding over the round's list.
struct dcp_env_args
{
    uint64_t const *row_off;           // [nlist + 1] from the round's first pair on
    unsigned nlist, nwaves;
    double const *begin, *end, *core;  // the round's rows
    double hi, lo;
    unsigned min_len;
    unsigned pair_base;                // the round's first pair in the call's list: a record's pair is pair_base + i
    uint32_t *count;                   // [nlist] the count pass writes them
    uint64_t const *env_at;            // [nlist + 1] the write pass reads them: pair i's records start at env[env_at[i]]
    dcp_envelope *env;                 // the round's records
};

extern "C" {
// The count pass (a->count receives every pair's kept runs) and the write pass (pair i's env_at[i + 1] - env_at[i]
// records, the counts' exclusive scan).  != 0: refused, nothing launched -- an empty list, no wavefront, a null pointer
// the pass needs.
int dcp_envelopes_count_launch(struct dcp_env_args const *a, void *stream);
int dcp_envelopes_write_launch(struct dcp_env_args const *a, void *stream);
}

#endif
