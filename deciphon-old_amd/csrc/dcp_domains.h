// dcp_domains.h -- hit paths split into domains on the device (dcp_domains.hip): one record and two sums per B .. E
// stretch, one total per path.
#ifndef DCP_DOMAINS_H
#define DCP_DOMAINS_H

#include "dcp_host.h"
#include <stdint.h>

// One path of the call.  The list holds npaths + 1 records: the last one is a sentinel whose step_off / dom_off are
// the totals, so that path h's steps are steps[rec[h].step_off .. rec[h + 1].step_off).
struct dcp_dom_path
{
    uint32_t seq;      // resident sequence
    uint32_t slot;     // entry of the resident DB's profile records (dcp_prof_meta / dcp_f64_prof)
    uint32_t step_off; // first step, relative to the call's first
    uint32_t dom_off;  // first domain record
};

struct dcp_domains_args
{
    dcp_dom_path const *paths; // [npaths + 1]
    unsigned npaths;
    struct dcp_step const *steps;
    uint32_t const *words, *woff; // the resident batch: 2-bit words, first word of every sequence
    // the resident DB in its precision.  Float: profs = dcp_prof_meta[], match = emis_match, trans = trans8, insert /
    // null = [nprof][1364] by caller index.  Double: profs = dcp_f64_prof[], match = tab, trans = trans, insert = xe
    // (null follows the insert table inside a profile's xe block; `null_tab` is not read).
    void const *profs, *match, *trans, *insert, *null_tab;
    // special transitions, 16 values per row: one row per resident sequence (xt_per_path == 0) or per path
    void const *xtrans;
    int xt_per_path;
    uint32_t *dom_out;             // [ndomains][12]
    void *core_out, *null_out;     // [ndomains]
    void *total_out;               // [npaths]
    unsigned long long *bad;       // (path << 32 | step) of the first edge that is not in the graph; ~0: none
};

extern "C" {
// f64 != 0: a double DB.  One launch on `stream`; HIP's error code.
int dcp_launch_domains(dcp_domains_args const *args, int f64, void *stream);
}

#endif
