// dcp_seqs.h -- kernels on the resident sequence batch itself (dcp_seqs.hip): the reverse strand, windows, regions.
#ifndef DCP_SEQS_H
#define DCP_SEQS_H

#include "dcp_host.h"
#include <stdint.h>

extern "C" {
// Sequences n .. 2n - 1 of a batch whose forward half [0, n) is in place: words_out [nwords] (the second half of the
// word array) receives the reverse complements, woff[n + q] = woff[q] + nwords, len[n + q] = len[q].  words_in /
// woff / len: the forward half ([nwords], [n] of [2n], [n] of [2n]).  Two launches on `stream`; HIP's error code.
int dcp_launch_revcomp(uint32_t const *words_in, uint32_t *words_out, uint32_t *woff, uint32_t *len, unsigned nseqs,
                       uint32_t nwords, void *stream);
// Windows: the batch of nwin windows that replaces a resident batch of nsrc sequences (dcp_gpu_seqs_cut_windows; the
// rule is dcp_seq_window_count / _start).  Device pointers throughout.
struct dcp_window_args
{
    uint32_t const *src_words, *src_woff, *src_len; // the resident batch: its words, [nsrc], [nsrc]
    uint32_t const *wfirst, *nwfirst;               // [nsrc]: each source's first window and that window's first word
    uint32_t *words;                                // [nwords]: the new batch's words (no overlap with src_words)
    uint32_t *woff, *len;                           // [nwin]: the new batch's index
    uint32_t *wsrc, *wofs;                          // [nwin]: the map, window -> (source, offset)
    unsigned nsrc, nwin;
    uint32_t nwords, window, step;
};
// Two launches on `stream` (index, then words); HIP's error code.
int dcp_launch_windows(struct dcp_window_args const *, void *stream);
// Regions: the batch of n regions that replaces a resident batch (dcp_gpu_seqs_cut_regions).  The host holds the list,
// so it computes the new index too; device pointers throughout.  Region i is the len[i] bases from rbegin[i] of
// source rsrc[i], reverse-complemented where rminus[i] != 0; the caller has checked rsrc[i] < the resident sequences,
// len[i] >= 1 and rbegin[i] + len[i] <= the source's length.
struct dcp_region_args
{
    uint32_t const *src_words, *src_woff; // the resident batch: its words, each source's first word
    uint32_t *words;                      // [nwords]: the new batch's words (no overlap with src_words)
    uint32_t const *woff, *len;           // [n]: the new batch's index, woff[0] = 0, woff[i + 1] = woff[i] + len[i] / 16 + 3
    uint32_t const *rsrc, *rbegin, *rminus; // [n]: the map
    unsigned n;
    uint32_t nwords;
};
// One launch on `stream`; HIP's error code.
int dcp_launch_regions(struct dcp_region_args const *, void *stream);
#ifdef DCP_TEST_HOOKS
// NOT in the shipped library (libdcp_hip_testhooks.so only; declared here, not in include/dcp_gpu.h).  The raw
// L / 16 + 3 words of resident sequence q as the device holds them: *nwords receives their number, out the words if
// cap holds them (else DCP_ENOMEM).
int dcp_gpu_test_fetch_seq_words(dcp_gpu_ctx *, unsigned q, uint32_t *out, unsigned cap, unsigned *nwords);
#endif
}

#endif
