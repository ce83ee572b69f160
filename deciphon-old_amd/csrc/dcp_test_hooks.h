// dcp_test_hooks.h -- hooks of the tests' own -DDCP_TEST_HOOKS build (libdcp_hip_testhooks.so) that include/dcp_gpu.h
// does not list: read-only ones, and a cap on the Forward launches' wavefronts and a bound on the posterior rounds' memory that must
// change no result.  Only
// dcp_gpu.hip includes it: the DP kernels' objects do not change with it.
#ifndef DCP_TEST_HOOKS_H
#define DCP_TEST_HOOKS_H

#include "dcp_host.h"

// The words of the records below.  Defined in both builds: the shipped library's launch loops name them in calls of
// note_pair_launch / note_rowsweep_plan (dcp_gpu.hip), which are empty there.
// how launch_rowsweep_scan ran a size class
#define DCP_RS_PATH_NONE 0u      // no profile of the class is resident
#define DCP_RS_PATH_PLAIN 1u     // the grid-mode one-profile kernel rowsweep_variant chose (viterbi_rowsweep_kernel)
#define DCP_RS_PATH_MP 2u        // K profiles per wavefront (viterbi_mp_kernel)
#define DCP_RS_PATH_SEGMENTED 3u // one segment per launch (viterbi_segment_kernel), the exact kernel behind it
#define DCP_RS_PLAN_WORDS 9u
// which driver launched a row-sweep kernel in pair mode
#define DCP_PL_SCAN_PAIRS 1u // dcp_gpu_scan_pairs: the host's list of a size class / launch group
#define DCP_PL_QLANE_REDO 2u // a query-lane scan's redo list (launch_qlane_scan; scan64 with kernel 4)
#define DCP_PL_SEG_REDO 3u   // the segmented sweep's seg_redo list (launch_segsweep_class)
#define DCP_PL_WORDS 7u

#ifdef DCP_TEST_HOOKS
extern "C" {
// What the last scan did, if it was a float row-sweep scan (else DCP_EINVAL); waits for it.  *nwords receives
// 2 + DCP_RS_PLAN_WORDS x classes, out -- if cap holds them, else DCP_ENOMEM -- the words
//   [0] 1 if the classes' launches were forked onto their own streams, [1] the number of size classes,
//   then per class {nodes per lane, wavefronts per pair, DCP_RS_PATH_*, plain: rows staged, wavefronts per block,
//   prefetch; segmented: queries per chunk, pairs its last segment handed to the exact kernel (seg_redo; they are
//   not part of dcp_gpu_last_scan_redo_pairs); K profiles per wavefront: 1 if the flagged profiles of the class got
//   a launch of the one-profile kernel}.  Changes nothing.
int dcp_gpu_test_last_rowsweep_plan(dcp_gpu_ctx *, unsigned *out, unsigned cap, unsigned *nwords);
// The pair-mode launches of the last scan or dcp_gpu_scan_pairs call, in launch order; waits for the stream, looks at
// no redo counter (a scan whose lists overflowed is repeated by the next call that completes it -- the repeat is a
// dense row sweep: no pair-mode launch).  *nwords receives 1 + DCP_PL_WORDS x launches, out -- if cap holds them, else
// DCP_ENOMEM -- the words [0] the number of launches, then per launch {DCP_PL_*, 32 | 64 the DB's precision,
//   float: nodes per lane and wavefronts per pair of the size class; double: the launch group 0 .. 3 and its nodes per lane,
//   blocks (float) / wavefronts (double) launched, tasks per block (double: 1 per wavefront), the list capacity the
//   kernel was given (pair_cap)}.  Changes nothing.
int dcp_gpu_test_last_pair_launches(dcp_gpu_ctx *, unsigned *out, unsigned cap, unsigned *nwords);
// Cap on the wavefronts of each of the following dcp_gpu_forward_pairs launches (the stride loop then takes several
// pairs per wavefront, of whatever widths follow each other in the class's list); 0 restores the default.  Results
// must not change with it.
// (dcp_gpu_posterior_pairs' launches take the same cap.)
// (dcp_gpu_forward_dense's launches take it as well.)
int dcp_gpu_test_set_forward_waves(dcp_gpu_ctx *, unsigned nwaves);
// Bound, in pairs, on a round of each of the following dcp_gpu_forward_dense calls: a small one makes the outer product
// run in several rounds, whose boundaries fall inside classes and between them; 0, or more than the default, restores
// the default (2^22 pairs).  Results must not change with it.
int dcp_gpu_test_set_dense_round(dcp_gpu_ctx *, unsigned npairs);
// The band of the scaled Forward sweeps' rescaling rule (dcp_forward_scaled.h), in bits, for the following
// dcp_gpu_forward_pairs_scaled and dcp_gpu_forward_dense_scaled calls: a small one rescales every few rows; 0 restores
// the default (64).  Results must not change with it.  (The scaled launches take dcp_gpu_test_set_forward_waves' cap and
// dcp_gpu_test_set_dense_round's bound too.)
int dcp_gpu_test_set_forward_scale_band(dcp_gpu_ctx *, unsigned bits);
// Bound, in bytes, on the device memory of the row records of each of the following dcp_gpu_posterior_pairs calls: a
// small one makes the list run in several rounds; 0 restores the default (1 GiB).  Results must not change with it.
int dcp_gpu_test_set_posterior_budget(dcp_gpu_ctx *, unsigned long long bytes);
// The same for dcp_gpu_mea_pairs: the bound on the device memory of a round's matrices, choices and row records; 0
// restores the default (8 GiB).  Results must not change with it.  (Its launches take dcp_gpu_test_set_forward_waves'
// cap too.)
int dcp_gpu_test_set_mea_budget(dcp_gpu_ctx *, unsigned long long bytes);
// (dcp_gpu_envelope_pairs takes dcp_gpu_test_set_forward_waves' cap -- its envelope passes' launches too -- and
// dcp_gpu_test_set_posterior_budget's bound.)
// The envelope passes (dcp_envelopes.hip) alone, on rows of the caller's making: pair i's rows are
// [row_off[i], row_off[i + 1]) of begin / end / core, at least one row each, uploaded as one round; the records come back
// as dcp_gpu_envelope_pairs returns them, pair = i, env_off [npairs + 1] written in full.  DCP_ENOMEM past cap (env_off
// is written; after any other error no output is touched), DCP_EINVAL for a null pointer, a pair without rows, NaN thresholds or lo > hi.  Needs no DB and no batch.
int dcp_gpu_test_envelopes_of_rows(dcp_gpu_ctx *, uint64_t const *row_off, double const *begin, double const *end,
                                   double const *core, unsigned npairs, double hi, double lo, unsigned min_len,
                                   struct dcp_envelope *out, uint64_t cap, uint64_t *env_off);
// The envelope kernels' own part of dcp_gpu_envelope_kernel_ms (the two passes of every round, by events of their own) of
// the context's last dcp_gpu_envelope_pairs that ran all its rounds; negative before.  Changes nothing.
float dcp_gpu_test_envelope_records_kernel_ms(dcp_gpu_ctx *);
}
#endif

#endif
