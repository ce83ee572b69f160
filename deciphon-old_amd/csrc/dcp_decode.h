// dcp_decode.h -- the decode of hit paths on the device (dcp_decode.hip): one codon code per emitting step.
#ifndef DCP_DECODE_H
#define DCP_DECODE_H

#include "dcp_host.h"
#include <stdint.h>

// One emitting step of a path, from integers only (the host's work list).
struct dcp_decode_item
{
    uint32_t seq;   // resident sequence
    uint32_t start; // first base of the fragment; start + len <= the sequence's length
    uint32_t prof;  // resident profile (the caller's index)
    uint32_t sel;   // bits 0..2 fragment length 1..5; bits 3..4 the distribution: 0 null, 1 insert, 2 the match dist
                    // of node k; bits 8..19 k (0-based, < core_size)
};

enum
{
    DCP_DECODE_NULL = 0,
    DCP_DECODE_INSERT = 1,
    DCP_DECODE_MATCH = 2,
    DCP_DECODE_EXP = 68,           // b[4], pc[64] of one distribution
    DCP_DECODE_MAX_ITEMS = 1 << 20 // emitting steps per launch
};

struct dcp_decode_args
{
    dcp_decode_item const *items;
    unsigned nitems;
    uint32_t const *words, *woff; // the resident batch: 2-bit words, first word of every sequence
    void const *dists;            // the resident compact dists, [row][129] float or double
    uint32_t const *match_row;    // per profile: the row of its first node's match dist
    double const *exp_ni;         // per profile [2][68]: the host's exp() of the null and the insert dist
    double const *eps;            // per profile: the epsilon dcp_profile_decode uses
    uint8_t *codes;               // [nitems]: 16a + 4b + c
};

extern "C" {
// f64 != 0: `dists` holds doubles.  One launch on `stream`; HIP's error code.
int dcp_launch_decode(dcp_decode_args const *args, int f64, void *stream);
}

#endif
