/*
 * dcp_gpu.h -- C-ABI of the MI355X-native profile-HMM scan engine.
 *
 * This is the drop-in boundary for deciphon-old's scan hot path
 * (SURVEY.md §8b). Plain C: pointers, sizes, POD structs; no C++/torch types.
 * Citations are `path:line` in the reference tree (EBI-Metagenomics/deciphon-old).
 *
 * What each group replaces:
 *   dcp_profile_*        protein_profile_{init,sample,absorb,setup} and the model
 *                        builder it calls   src/model/protein_profile.c:134-304,
 *                                           src/model/protein_model.c:49-500
 *   dcp_gpu_db_*         profile_reader_{setup,rewind,next} + protein_profile.unpack:
 *                        the DB is uploaded ONCE and stays resident in HBM instead
 *                        of being re-read per sequence
 *                                           src/db/profile_reader.c:74-168,
 *                                           src/model/protein_profile.c:38-117
 *   dcp_gpu_seqs_*       imm_seq()/imm_task_setup(): sequence encoding, once per
 *                        batch instead of once per (seq, profile) pair
 *                                           src/server/scan.c:229,
 *                                           src/server/scan_thread.c:51-55
 *   dcp_gpu_scan*        thread_run's per-pair body: protein_profile_setup,
 *                        imm_dp_viterbi(null), imm_dp_viterbi(alt), xmath_lrt filter
 *                                           src/server/scan_thread.c:99-123,
 *                                           include/deciphon/core/xmath.h:32-43
 *
 * Errors: every function that can fail returns `enum dcp_rc`, numerically equal
 * to the reference's `enum rc` (include/deciphon/core/rc.h:4-15); HIP failures map
 * to DCP_EFAIL and the message is kept in dcp_gpu_last_error().
 * There is NO CPU fallback: without a HIP device dcp_gpu_ctx_new() fails.
 */
#ifndef DCP_GPU_H
#define DCP_GPU_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

/* include/deciphon/core/rc.h:4-15 */
enum dcp_rc
{
    DCP_OK = 0,
    DCP_END = 1,
    DCP_EFAIL = 2,
    DCP_EINVAL = 3,
    DCP_EIO = 4,
    DCP_ENOMEM = 5,
    DCP_EPARSE = 6,
    DCP_EAPI = 7,
    DCP_EHTTP = 8,
};

/* include/deciphon/model/entry_dist.h:4-9 */
enum dcp_entry_dist
{
    DCP_ENTRY_DIST_NULL = 0,
    DCP_ENTRY_DIST_UNIFORM = 1,
    DCP_ENTRY_DIST_OCCUPANCY = 2,
};

enum
{
    DCP_AMINO_SIZE = 20,          /* IMM_AMINO_SIZE */
    DCP_TRANS_SIZE = 7,           /* PROTEIN_TRANS_SIZE, protein_trans.h:6 */
    DCP_NCODES = 1364,            /* nucleotide words of length 1..5 */
    DCP_NDIST = 129,              /* nuclt_dist: 4 base lprobs + 5x5x5 codon marg */
    DCP_CORE_SIZE_MAX = 4096,     /* PROTEIN_MODEL_CORE_SIZE_MAX, limits.h:11 */
    DCP_PROFILE_ACC_SIZE = 32,    /* limits.h:9 */
    DCP_NUM_THREADS = 64,         /* limits.h:8: max partitions */
    DCP_NXTRANS = 13,
};

/* ------------------------------------------------------------------------ */
/* Host-side compact profile ("dcpx"): everything protein_profile carries     */
/* that the scan needs, without the per-state emission tables (those are      */
/* expanded on the device at upload).                                         */
/* ------------------------------------------------------------------------ */
typedef struct dcp_profile dcp_profile;

/* protein_profile_init + protein_model_init/setup/add_node/add_trans +
 * protein_profile_absorb (protein_profile.c:134-153,218-257;
 * protein_model.c:49-137,155-184).
 *   null_lprobs [20], match_lprobs [core_size][20] amino log-probs in
 *   imm_amino_iupac order "ACDEFGHIKLMNPQRSTVWY"; trans [core_size+1][7] in
 *   protein_trans order MM MI MD IM II DM DD (protein_trans.h:8-27).
 * Returns NULL (and DCP_EINVAL in *rc) for core_size == 0 or > 4096,
 * as protein_model_setup does (protein_model.c:157-160). */
dcp_profile *dcp_profile_new(char const *accession, unsigned core_size,
                             int entry_dist, float epsilon,
                             float const *null_lprobs,
                             float const *match_lprobs, float const *trans,
                             char const *consensus, int *rc);

/* protein_profile_sample (protein_profile.c:259-304): imm_rnd(seed) stream,
 * log-uniform lprobs, normalised; DD=-inf at i=0, MD=DD=-inf at i=core_size. */
dcp_profile *dcp_profile_sample(char const *accession, unsigned seed,
                                unsigned core_size, int entry_dist,
                                float epsilon, int *rc);
/* A profile from its scan-time parts (what a pressed DB stores: protein_profile.c:338-400):
 * trans8 [8][core_size] rows entry(B->Mk), MM, IM, DM, MD, DD (edges INTO node k), MI, II;
 * null / insert dists [129], match dists [core_size][129] (4 base lprobs + 5x5x5 codon marginals).
 * NULL + DCP_EINVAL for core_size outside 1..4096, epsilon outside [0,1] or a NaN value. */
dcp_profile *dcp_profile_from_parts(char const *accession, unsigned core_size, int entry_dist, float epsilon,
                                    char const *consensus, float const *trans8, float const *null_dist,
                                    float const *insert_dist, float const *match_dist, int *rc);
void dcp_profile_del(dcp_profile *);
unsigned dcp_profile_core_size(dcp_profile const *);
int dcp_profile_entry_dist(dcp_profile const *);
float dcp_profile_epsilon(dcp_profile const *);
/* imm_rnd(seed) / its next double in [0,1) (xoshiro256+ seeded by splitmix64: pinned by the
 * reference's golden test/protein_profile.c:41), and imm_lprob_normalize. */
void dcp_rnd_seed(uint64_t state[4], uint64_t seed);
double dcp_rnd_next(uint64_t state[4]);
void dcp_lprob_normalize(unsigned n, float *lprobs);
char const *dcp_profile_accession(dcp_profile const *);

/* ---- HMMER3 ASCII reader: .hmm -> profiles, what protein_h3reader_next +
 * protein_profile_absorb do in hmm_press (src/model/protein_h3reader.c:18-72,
 * src/server/hmm.c:120-178). The reference parses with the third-party `hmr` library (absent);
 * this is an own parser of the published HMMER3/f text format: per profile the node-0 transition
 * line gives trans[0]; every node line gives 20 match -ln(p) values (`*` = probability 0) and its
 * CONS letter, the next line (insert emissions) is ignored as the reference ignores it, the third
 * gives trans[k]. The null model is the hard-coded Swiss-Prot 50.8 amino frequencies
 * (protein_h3reader.c:79-103); the profile's accession is the ACC field (hmm.c:113-117), NAME if
 * there is none. */
typedef struct dcp_h3reader dcp_h3reader;
dcp_h3reader *dcp_h3reader_open(char const *path, int entry_dist, float epsilon);
/* Same over a stream the caller keeps owning (protein_h3reader_init takes a FILE*). */
dcp_h3reader *dcp_h3reader_open_fp(FILE *fp, int entry_dist, float epsilon);
/* The next profile's raw parameters instead of a built profile (what protein_h3reader_next leaves in
 * its protein_model): match_lprobs [core_size][20], trans [core_size+1][7]; pointers stay valid
 * until the next call on this reader. Same return codes as dcp_h3reader_next. */
struct dcp_h3params
{
    unsigned core_size;
    float const *match_lprobs;
    float const *trans;
    char const *consensus;
    char const *name;
    char const *acc;
};
int dcp_h3reader_next_params(dcp_h3reader *, struct dcp_h3params *out);
/* DCP_OK and *out (caller owns it), DCP_END at end of file, DCP_EPARSE on malformed input
 * (message in dcp_h3reader_error), DCP_EINVAL for core sizes outside 1..4096. */
int dcp_h3reader_next(dcp_h3reader *, dcp_profile **out);
char const *dcp_h3reader_error(dcp_h3reader const *);
void dcp_h3reader_close(dcp_h3reader *);
/* log of the Swiss-Prot 50.8 background frequencies, imm_amino_iupac order */
void dcp_swissprot_null_lprobs(float out[DCP_AMINO_SIZE]);
char const *dcp_profile_consensus(dcp_profile const *);

/* ---- dcpx: compact on-disk profile DB (press once, scan many) ------------------------------
 * Own little-endian container for what the scan needs (transitions + nuclt_dists; no per-state
 * emission tables: the device expands them at upload). It is NOT the reference's .dcp: that is
 * MessagePack with opaque imm_dp blobs whose format lives in the absent imm library. The header
 * carries the reference's fields and its checks (src/db/protein_reader.c:40-82, src/db/reader.c:25-79):
 * magic 0xC6F0 (include/deciphon/db/types.h:11), profile_typeid == PROFILE_PROTEIN, float_size == 4,
 * entry_dist in {UNIFORM, OCCUPANCY}, 0 <= epsilon <= 1, alphabets, profile_sizes[] (u32 bytes per
 * profile). One (entry_dist, epsilon) per DB, as protein_db_writer_open fixes it
 * (src/db/protein_writer.c:56-96). */
typedef struct dcp_db dcp_db;
int dcp_db_write(char const *path, dcp_profile *const *profiles, unsigned nprofiles);
/* NULL + *rc: DCP_EIO (cannot open / truncated), DCP_EINVAL (bad magic, typeid, float size,
 * entry_dist, epsilon, too many profiles) */
dcp_db *dcp_db_open(char const *path, int *rc);
void dcp_db_close(dcp_db *);
unsigned dcp_db_nprofiles(dcp_db const *);
int dcp_db_entry_dist(dcp_db const *);
float dcp_db_epsilon(dcp_db const *);
uint32_t const *dcp_db_profile_sizes(dcp_db const *);
/* profile_reader_setup's partition table for this file (src/db/profile_reader.c:45-72): count-balanced
 * contiguous partitions, part_offset[i] = byte offset in the file where partition i starts,
 * the end of the last non-empty partition = end of the profiles. ceil-sized partitions can leave
 * trailing empty ones whose end offset the reference never writes (0): reproduced as is.
 * Returns npart = min(npartitions, nprofiles); 0 on EINVAL. */
unsigned dcp_db_partitions(dcp_db const *, unsigned npartitions, unsigned part_size[DCP_NUM_THREADS],
                           int64_t part_offset[DCP_NUM_THREADS + 1]);
/* Profiles [begin, end) (caller owns them). */
int dcp_db_read(dcp_db *, unsigned begin, unsigned end, dcp_profile **out);

/* Read-only views (host memory owned by the profile):
 *   trans8 [8][core_size]: rows entry(B->Mk), MM, IM, DM, MD, DD (edges INTO
 *   node k from node k-1) and MI, II (node k's own insert edges);
 *   dists: null [129], insert [129], match [core_size][129]. */
float const *dcp_profile_trans8(dcp_profile const *);
float const *dcp_profile_null_dist(dcp_profile const *);
float const *dcp_profile_insert_dist(dcp_profile const *);
float const *dcp_profile_match_dist(dcp_profile const *);

/* ---- The double build (the reference's IMM_DOUBLE_PRECISION) ----------------------------------------------
 * dcp_profile_new64 / dcp_profile_sample64: the same arguments as dcp_profile_new / dcp_profile_sample with
 * lprobs, trans and epsilon in double.  The profile is built in double throughout -- imm's log-domain sums in its
 * order, no rounding to float -- and keeps its scan-time parts in double: trans8 [8][core_size], null / insert
 * dists [129], match dists [core_size][129].  Its float parts (dcp_profile_trans8 ...) hold the same values
 * rounded once, for the float-only consumers (dcp_db_write, decode, product rows); dcp_gpu_db_upload refuses it,
 * dcp_gpu_db_upload64 takes it. */
dcp_profile *dcp_profile_new64(char const *accession, unsigned core_size, int entry_dist, double epsilon,
                               double const *null_lprobs, double const *match_lprobs, double const *trans,
                               char const *consensus, int *rc);
dcp_profile *dcp_profile_sample64(char const *accession, unsigned seed, unsigned core_size, int entry_dist,
                                  double epsilon, int *rc);
/* dcp_profile_from_parts in double: a double profile from its stored scan-time parts (what unpacking a profile of a
 * double .dcp needs).  The float parts are those values rounded once, as dcp_profile_new64 leaves them.  NULL +
 * DCP_EINVAL for core_size outside 1..4096, epsilon outside [0,1] or a NaN value. */
dcp_profile *dcp_profile_from_parts64(char const *accession, unsigned core_size, int entry_dist, double epsilon,
                                      char const *consensus, double const *trans8, double const *null_dist,
                                      double const *insert_dist, double const *match_dist, int *rc);
/* imm_lprob_normalize on doubles, as dcp_profile_sample64 applies it. */
void dcp_lprob_normalize64(unsigned n, double *lprobs);
/* 64 for a profile of the double build, 32 otherwise. */
int dcp_profile_precision(dcp_profile const *);
/* The double parts (same layouts as the float views below); NULL for a float profile. */
double dcp_profile_epsilon64(dcp_profile const *);
double const *dcp_profile_trans8_64(dcp_profile const *);
double const *dcp_profile_null_dist64(dcp_profile const *);
double const *dcp_profile_insert_dist64(dcp_profile const *);
double const *dcp_profile_match_dist64(dcp_profile const *);

/* Frame-state emission table of one nuclt_dist over all 1364 words (host).
 * out[code], code = {0,4,20,84,340}[len-1] + base-4 value of the word, first
 * base most significant. Same formula the device expansion kernel evaluates. */
void dcp_frame_table_host(float const dist[DCP_NDIST], float epsilon,
                          float out[DCP_NCODES]);

/* protein_profile_setup (protein_profile.c:155-216): the 13 length-dependent
 * special transitions RR, SB, SN, NN, NB, ET, EC, CC, CT, EB, EJ, JJ, JB.
 * DCP_EINVAL for seq_size == 0 (:158). */
int dcp_xtrans(unsigned seq_size, int multi_hits, int hmmer3_compat,
               float out[DCP_NXTRANS]);

/* The same 13 values in double (protein_profile_setup of the double build). */
int dcp_xtrans64(unsigned seq_size, int multi_hits, int hmmer3_compat, double out[DCP_NXTRANS]);

/* xmath_lrt_f32 (xmath.h:32-35) */
float dcp_lrt(float null_loglik, float alt_loglik);

/* profile_reader partitioning (profile_reader.c:54-72, xmath.h:24-30):
 * contiguous count-balanced partitions. part_size[npart], returns npart =
 * min(npartitions, nprofiles) or 0 on EINVAL (0 or > 64 partitions). */
unsigned dcp_partition_by_count(unsigned nprofiles, unsigned npartitions,
                                unsigned part_size[DCP_NUM_THREADS]);
/* MI355X shard map: contiguous partitions balanced by sum of core sizes
 * (cells), one per GPU. part_begin[npart+1]. */
void dcp_partition_by_cells(unsigned const *core_sizes, unsigned nprofiles,
                            unsigned npartitions, unsigned *part_begin);

/* ------------------------------------------------------------------------ */
/* Device context                                                            */
/* ------------------------------------------------------------------------ */
typedef struct dcp_gpu_ctx dcp_gpu_ctx;

int dcp_gpu_device_count(void);
/* Fails (NULL) when no HIP device is present: there is no CPU fallback. */
dcp_gpu_ctx *dcp_gpu_ctx_new(int device);
void dcp_gpu_ctx_del(dcp_gpu_ctx *);
char const *dcp_gpu_last_error(dcp_gpu_ctx const *);
/* The HIP stream every launch of this context goes to (hipStream_t). */
void *dcp_gpu_stream(dcp_gpu_ctx *);

/* Upload `nprofiles` profiles; expands every match/insert/null frame-state
 * emission table into HBM (layout: DESIGN.md §3).  `flags` (0 for a server):
 *   DCP_DB_EXPAND_ON_HOST  the tables are computed with dcp_frame_table_host and
 *                          copied (slow; parity tests).  (The argument used to be
 *                          `int expand_on_host`: 0 / 1 keep their meaning.)
 *   DCP_DB_ONE_LAYOUT      keep ONE layout of the match tables resident -- the row
 *                          sweep's [1364][ldk] -- and let the query-lane kernels
 *                          gather their 8-node tile images from it, instead of
 *                          holding those images as a second copy: half the
 *                          footprint (20.6 instead of 40.2 GB per 20 000 Pfam-like
 *                          profiles), same bits.  Chosen by the library itself when
 *                          both layouts would not leave 16 GiB of the device's
 *                          free memory.
 * Replaces any previously uploaded DB.  (The reference re-reads the profiles from
 * the .dcp file for every sequence: src/server/scan.c:227-258, profile_reader.c.) */
#define DCP_DB_EXPAND_ON_HOST 1
#define DCP_DB_ONE_LAYOUT 2
int dcp_gpu_db_upload(dcp_gpu_ctx *, dcp_profile *const *profiles,
                      unsigned nprofiles, int flags);
/* Upload a DB of double-build profiles (dcp_profile_new64 / dcp_profile_sample64): their frame tables are
 * expanded on the device in double, [1364][core_size padded to the kernel's columns] per profile -- one layout.
 * DCP_EINVAL if any profile was built in float.  A context holds ONE resident DB, float or double: either upload
 * replaces the other.  Scans of a double DB run the f64 row sweep (dcp_scan_params.kernel 0 or 1) or the f64
 * query-lane kernel (4: the throughput path for batches, of one length or mixed -- it packs the queries by length as
 * dcp_plan_query_slots says, see dcp_gpu_last_scan_query_plan; same bits); 2 and 3,
 * the float query-lane kernels, are DCP_EINVAL.  They leave double results: dcp_gpu_fetch_hits64 / dcp_gpu_fetch_scores64; their paths come from
 * dcp_gpu_trace_paths64.  The float-only calls (dcp_gpu_trace_paths, dcp_gpu_db_fetch_match_table, float explicit
 * xtrans) return DCP_EINVAL on it; dcp_gpu_hit_buffer answers float scans only and is DCP_EINVAL after a scan of a
 * double DB, whose buffer dcp_gpu_hit_buffer64 returns (a caller's own: dcp_gpu_set_hit_buffer64). */
int dcp_gpu_db_upload64(dcp_gpu_ctx *, dcp_profile *const *profiles, unsigned nprofiles);
/* 32 or 64: the precision of the resident DB; 0 without one. */
int dcp_gpu_db_precision(dcp_gpu_ctx const *);
unsigned dcp_gpu_db_nprofiles(dcp_gpu_ctx const *);
/* 1 when the resident DB holds one table layout (asked for or chosen). */
int dcp_gpu_db_one_layout(dcp_gpu_ctx const *);
/* Bytes of expanded match tables resident now (the row-sweep layout of a
 * two-layout DB appears with the first scan that needs it). */
uint64_t dcp_gpu_db_table_bytes(dcp_gpu_ctx const *);
/* Copy profile p's expanded match table back: out [1364][core_size]. */
int dcp_gpu_db_fetch_match_table(dcp_gpu_ctx *, unsigned p, float *out);
/* The same from a double DB: out [1364][core_size] in double, as expand64_kernel wrote it.  DCP_EINVAL on a
 * float DB. */
int dcp_gpu_db_fetch_match_table64(dcp_gpu_ctx *, unsigned p, double *out);
/* Profile p's insert and null (background) tables of a double DB, [1364] each in double; either pointer may be
 * NULL.  DCP_EINVAL on a float DB. */
int dcp_gpu_db_fetch_insert_null64(dcp_gpu_ctx *, unsigned p, double *insert, double *null_tab);

/* Upload a batch of sequences. seqs: concatenated symbol ids 0..3 (A,C,G,T);
 * seq_off[nseqs+1]. Any id > 3 or an empty sequence -> DCP_EINVAL
 * (protein_profile.c:158; imm rejects symbols outside the alphabet). */
int dcp_gpu_seqs_upload(dcp_gpu_ctx *, uint8_t const *seqs,
                        uint32_t const *seq_off, unsigned nseqs);
/* Same from ASCII "ACGT" text (what scan.c:229 hands to imm_seq). */
int dcp_gpu_seqs_upload_text(dcp_gpu_ctx *, char const *text,
                             uint32_t const *seq_off, unsigned nseqs);
unsigned dcp_gpu_nseqs(dcp_gpu_ctx const *);
/* Both strands.  The frame model absorbs frame shifts inside a read, nothing absorbs the strand: a gene on the minus
 * strand is found only in the read's reverse complement.  After this call the resident batch of n sequences is 2n:
 * sequence n + q is the reverse complement of sequence q -- base i = 3 - base(L - 1 - i), ids A C G T = 0 1 2 3 --
 * with the same length, written on the device from the resident 2-bit words (csrc/dcp_seqs.hip; the forward half is
 * copied device to device, no base goes through the host again).  Everything downstream sees a batch of 2n:
 * dcp_gpu_nseqs, the cells / bytes accounting, every kernel of either precision, hits, scores, traces and gathers carry
 * resident indices 0 .. 2n - 1, and dcp_gpu_scan_range(.., n, 2n) is "minus strand only".  Dependent state is
 * treated as by an upload (the last scan is void).  DCP_EINVAL, with a message and the batch untouched: no batch
 * resident; the batch already holds both strands; explicit special transitions in force (they are per sequence: set
 * them after this call, for 2n rows); 2n sequences or their words would pass 2^32 - 1 (checked before any allocation).
 * A failed allocation leaves the context without a batch, as a failed upload does.  The next sequence upload
 * returns the context to one strand.  Works on float and double DBs alike, and with no DB resident. */
int dcp_gpu_seqs_add_revcomp(dcp_gpu_ctx *);
/* 0 (no batch resident), 1, or 2 after dcp_gpu_seqs_add_revcomp. */
unsigned dcp_gpu_seqs_strands(dcp_gpu_ctx const *);
/* Resident sequence q as symbol ids, unpacked from the device's words: what a caller hands to dcp_prod_format_row /
 * dcp_profile_decode for a minus-strand hit.  *len (may be NULL) receives its length; DCP_ENOMEM (with *len set) if
 * cap is smaller, DCP_EINVAL if q is not resident.  (The tests' build also has dcp_gpu_test_fetch_seq_words, the raw
 * L / 16 + 3 words of a sequence: declared in csrc/dcp_seqs.h, not here.) */
int dcp_gpu_seqs_fetch(dcp_gpu_ctx *, unsigned q, uint8_t *ids, unsigned cap, unsigned *len);
/* The reverse complement of n symbol ids 0..3 on the host: out[i] = 3 - ids[n - 1 - i] (out must not overlap ids).
 * The restatement of the device kernel that the tests and the host layer use. */
void dcp_seq_revcomp(uint8_t const *ids, unsigned n, uint8_t *out);
/* Windows.  A long sequence costs the traceback a work area over all its rows per hit, and a batch is as slow as its
 * longest member: long targets are cut into overlapping windows and the windows scanned.  The rule, for window >= 1 and
 * 1 <= step <= window: a sequence of L bases gives 1 window if L <= window, else 1 + ceil((L - window) / step); window
 * i starts at min(i step, L - window) (0 if L <= window) and has min(L, window) bases -- the last one is anchored at
 * the sequence's end, every window of a longer sequence has exactly `window` bases.  Pure host arithmetic:
 * _count returns 0 and _start 0 for a bad rule; _plan sums over a batch's lengths, *nwindows the windows and *nwords
 * their resident words (wl / 16 + 3 each), both in 64 bits (either may be NULL), and returns DCP_EINVAL for a bad
 * rule or when either total exceeds 2^32 - 1. */
unsigned dcp_seq_window_count(unsigned L, unsigned window, unsigned step);
unsigned dcp_seq_window_start(unsigned L, unsigned window, unsigned step, unsigned i);
int dcp_seq_window_plan(uint32_t const *len, unsigned nseqs, unsigned window, unsigned step, uint64_t *nwindows,
                        uint64_t *nwords);
/* The resident batch of n sequences is REPLACED by its W = sum of counts windows, in source order, then offset order,
 * written on the device from the resident 2-bit words (csrc/dcp_seqs.hip: no base goes through the host again); the
 * sources are no longer resident.  Everything downstream sees a batch of W sequences; a batch in which every L <=
 * window comes out word for word as it was.  Dependent state is treated as dcp_gpu_seqs_add_revcomp treats it (the
 * last scan is void); strands stays 1, and dcp_gpu_seqs_add_revcomp after the cut gives 2 W: resident W + i is the
 * reverse complement of window i.  A window is scored as the sequence it now is: its Viterbi score is that of its
 * bases alone, under special transitions for its own length -- not a share of the source's score -- and a gene in the
 * overlap of two windows is reported from both (merging is the caller's).  DCP_EINVAL, with a message and the batch
 * untouched: no batch resident; a bad window / step; both strands already resident (cut first, then add the reverse
 * strand); the batch already cut; explicit special transitions in force (set them after the cut, one row per
 * window); W or the windows' words would pass 2^32 - 1 (checked before any allocation).  A failed allocation
 * leaves the context without a batch, as a failed upload does.  The next sequence upload returns the context to
 * uncut.  Works on float and double DBs alike, and with no DB resident. */
int dcp_gpu_seqs_cut_windows(dcp_gpu_ctx *, unsigned window, unsigned step);
/* 1 if the resident batch is cut into windows, with the rule in *window / *step (either may be NULL); else 0 / 0 / 0. */
int dcp_gpu_seqs_windows(dcp_gpu_ctx const *, unsigned *window, unsigned *step);
/* For window i < W: src[i] its source's index in the uploaded batch, off[i] its first base there.  After
 * dcp_gpu_seqs_add_revcomp the map still has W entries (resident W + i is window i's reverse complement).  DCP_ENOMEM if
 * cap < W, DCP_EINVAL if the batch is not cut.  dcp_gpu_seqs_fetch serves a window's bases. */
int dcp_gpu_seqs_window_map(dcp_gpu_ctx *, uint32_t *src, uint32_t *off, unsigned cap);
/* Regions.  What windows report of a gene longer than their overlap is pieces: the finish is to cut the
 * stretch the pieces cover out of the source and score it again.  The resident batch of uploaded sequences is REPLACED
 * by n regions: resident i is the bases [begin[i], begin[i] + len[i]) of resident source src[i], and their reverse
 * complement where minus[i] != 0 -- base k = 3 - base(begin + len - 1 - k) -- written on the device from the resident
 * 2-bit words (csrc/dcp_seqs.hip, region_words_kernel); the sources are no longer resident.  Regions may overlap, repeat
 * and come in any order.  Everything downstream sees a batch of n sequences in the resident layout (len / 16 + 3 words
 * each, every bit behind the last base zero); dcp_gpu_seqs_strands stays 1, a region carries its own strand.
 * Dependent state is treated as dcp_gpu_seqs_cut_windows treats it (the last scan is void).  A region is scored as the
 * sequence it now is.  DCP_EINVAL, with a message and the batch untouched, all checked before any allocation: no
 * batch resident; the batch is cut into windows, holds both strands or is already regions; explicit special
 * transitions in force (set them after the cut, one row per region); n == 0 or a null pointer; src >= the resident
 * sequences, len == 0 or begin + len > the source's length (in 64 bits), naming the first bad region; the regions'
 * words would pass 2^32 - 1.  A failed allocation leaves the context without a batch.  After the cut
 * dcp_gpu_seqs_add_revcomp and dcp_gpu_seqs_cut_windows are DCP_EINVAL; the next sequence upload returns the context
 * to normal.  Works on float and double DBs alike, and with no DB resident. */
int dcp_gpu_seqs_cut_regions(dcp_gpu_ctx *, uint32_t const *src, uint32_t const *begin, uint32_t const *len,
                             uint8_t const *minus, unsigned n);
/* The number of regions while the resident batch is one of regions, else 0. */
unsigned dcp_gpu_seqs_regions(dcp_gpu_ctx const *);
/* For region i < n: its source's index in the uploaded batch, its first base there (plus-strand coordinates) and its
 * strand (0 / 1); its length is the resident sequence's.  DCP_ENOMEM if cap < n, DCP_EINVAL if the batch is not one of
 * regions.  dcp_gpu_seqs_fetch serves a region's bases. */
int dcp_gpu_seqs_region_map(dcp_gpu_ctx *, uint32_t *src, uint32_t *begin, uint8_t *minus, unsigned cap);
/* Explicit special transitions for the resident sequences: xt [nseqs][13] in dcp_xtrans order.
 * By default a scan derives them from each sequence's length and the scan's flags (what
 * protein_profile_setup does per pair); imm_dp_viterbi on a profile whose transitions were set some
 * other way -- or never: the LOG1 defaults of protein_model.c:322-340, as test/protein_db.c:73 runs
 * it -- passes them here.  They stay in force until the next sequence upload; the scan flags
 * multi_hits / hmmer3_compat are then ignored.  NaN values are rejected (DCP_EINVAL). */
int dcp_gpu_seqs_set_xtrans(dcp_gpu_ctx *, float const *xt, unsigned nseqs);
/* The same for a double DB: xt [nseqs][13] in dcp_xtrans64 order.  Scans of a double DB (kernel 0, 1 or 4) and
 * dcp_gpu_trace_paths64 then use these rows instead of deriving them from the lengths and the flags; with them the
 * query-lane scan (4) keeps its redo lists whatever multi_hits says, since EB / EJ may be finite.  Until the next
 * sequence upload; a NaN (tested by its bit pattern) is DCP_EINVAL.  One explicit set holds, the last one given, and
 * it must fit the DB: float transitions before a scan of a double DB, or double ones before a scan or a
 * dcp_gpu_trace_paths of a float DB, are DCP_EINVAL with a message -- they are never rounded or widened. */
int dcp_gpu_seqs_set_xtrans64(dcp_gpu_ctx *, double const *xt, unsigned nseqs);

struct dcp_scan_params
{
    int multi_hits;      /* scan_thread.h:17 */
    int hmmer3_compat;   /* scan_thread.h:18 */
    float lrt_threshold; /* scan.c:221 passes 10.0 */
    int keep_scores;     /* also keep dense null/alt score matrices */
    int kernel;          /* 0 = choose by a cost model (DB size x batch size); 1 = row sweep (one wavefront
                          * group per pair: any batch size); 2 = query lane (one lane per query, tiles in
                          * LDS: throughput path); 3 = query lane, two-stage blocks (even / odd tiles of a
                          * profile pipelined through an LDS ring: half the scratch traffic);
                          * 4 = the double DB's query lane (one lane per query in double, the pairs whose
                          * multi-hit feedback it cannot carry re-scored by the f64 row sweep behind it).
                          * 2 and 3 are DCP_EINVAL on a double DB, 4 on a float one; 0 on a double DB is 1 */
};
/* The LRT threshold of the scans of a double DB, in double.  NaN -- the sentinel, and the default -- means
 * "(double) dcp_scan_params.lrt_threshold".  (Not a field of dcp_scan_params: callers that initialise it
 * positionally under -Wextra -Werror would stop compiling.)  Stays in force for the context's later scans. */
int dcp_gpu_set_lrt_threshold64(dcp_gpu_ctx *, double lrt_threshold64);

/* scan_thread.c:121-123 keeps a pair iff lrt is finite and >= threshold */
struct dcp_hit
{
    uint32_t seq_idx;
    uint32_t profile_idx;
    float null_loglik;
    float alt_loglik;
};

/* The hit record of a scan of a double DB: same keep rule, evaluated in double.  24 bytes, 6 uint32 words, no
 * padding (asserted in csrc/dcp_dist.cpp, which sends it as words). */
struct dcp_hit64
{
    uint32_t seq_idx;
    uint32_t profile_idx;
    double null_loglik;
    double alt_loglik;
};

/* Enqueue the scan of all resident sequences against all resident profiles on
 * the context's stream (asynchronous). */
int dcp_gpu_scan(dcp_gpu_ctx *, struct dcp_scan_params const *);
/* One scan is outstanding per context: results are those of the last scan enqueued; enqueueing
 * another one first completes the previous (it does not queue behind unread results).
 * Same for the resident sequences [q_begin, q_end): scan.c:227-258 hands
 * thread_run one sequence at a time; a caller that prefetched N sequences scans
 * them batch by batch without re-uploading. Hits and scores keep the indices
 * of the resident batch. */
int dcp_gpu_scan_range(dcp_gpu_ctx *, struct dcp_scan_params const *,
                       unsigned q_begin, unsigned q_end);
/* Score exactly the npairs pairs (resident sequence seq_idx[i], resident profile profile_idx[i]), on a float or a
 * double DB, without scanning the batch against the whole DB.  The host buckets the pairs by the row sweep's size
 * class (a double DB: by launch group) and the row-sweep kernels run over the lists in their pair mode, as they do over
 * a query-lane scan's redo lists: a pair's scores are the bits of a kernel-1 scan.  Results arrive as a scan's do:
 * asynchronous on the context's stream, one scan outstanding, dcp_gpu_sync, dcp_gpu_fetch_hits / ...64, the caller's
 * hit buffer and the gathers.  The LRT filter of params (dcp_gpu_set_lrt_threshold64 on a double DB) applies: a
 * threshold of -inf reports every pair whose scores are finite.  A pair listed twice is reported twice; the
 * context's own hit buffer holds min(npairs, 2^22) records.  There is no dense score matrix: keep_scores != 0 is
 * DCP_EINVAL, and dcp_gpu_fetch_scores after the call fails as after any scan without keep_scores.  Accounting:
 * dcp_gpu_last_scan_kernel is 1, the redo pairs 0, dcp_gpu_scan_cells the sum of core_size x length over the list
 * (dcp_gpu_scan_algorithmic_bytes likewise), dcp_gpu_last_scan_launch_info one record per non-empty size class with
 * that class's pairs' cells (a double DB keeps no launch records).  Explicit special transitions apply per sequence,
 * as in a scan.  DCP_EINVAL with a message: keep_scores != 0; kernel other than 0 or 1; an index out of range, naming
 * the first bad pair; no DB or no batch resident; explicit transitions of the other precision.  npairs == 0 is
 * DCP_OK with zero hits. */
int dcp_gpu_scan_pairs(dcp_gpu_ctx *, struct dcp_scan_params const *, uint32_t const *seq_idx,
                       uint32_t const *profile_idx, unsigned npairs);
/* Let the scan write its hit records and hit count into caller-owned DEVICE
 * memory (cap records of struct dcp_hit, one uint32 counter) -- e.g. a buffer
 * that RCCL then gathers. NULL, 0, NULL restores the internal
 * buffer. */
int dcp_gpu_set_hit_buffer(dcp_gpu_ctx *, void *hits_dev, unsigned cap,
                           void *nhits_dev);
/* The device memory the last scan wrote its hit records and counter to (the context's own buffer, or the
 * caller's from dcp_gpu_set_hit_buffer) -- what a C host hands to dcp_dist_gather_hits without touching
 * the HIP API itself.  Call dcp_gpu_sync first: a query-lane scan completes its redo pairs there. */
int dcp_gpu_hit_buffer(dcp_gpu_ctx *, void **hits_dev, void **nhits_dev, unsigned *cap);
/* dcp_gpu_set_hit_buffer for the scans of a double DB: hits_dev is cap records of struct dcp_hit64, nhits_dev one
 * uint32 counter.  NULL, 0, NULL restores the context's own buffer; the same argument checks.  The two registrations
 * are independent and both may be set: this one applies to scans of a double DB only, the float one to scans of a
 * float DB only.  Every path of a double scan honours it -- either kernel, kernel 4's redo launches, ranged scans
 * and the repeat with the row sweep after kernel 4's redo lists overflowed (which zeroes the counter again, so no
 * record appears twice).  Overflow as in float: the counter keeps counting past cap, nothing is written at or
 * beyond record cap, and dcp_gpu_fetch_hits64 -- which reads whichever buffer the scan wrote -- returns DCP_ENOMEM
 * with the true count in *nhits. */
int dcp_gpu_set_hit_buffer64(dcp_gpu_ctx *, void *hits_dev, unsigned cap, void *nhits_dev);
/* dcp_gpu_hit_buffer for the last scan of a double DB: what it wrote its struct dcp_hit64 records and counter to,
 * the context's own buffer or the caller's.  DCP_EINVAL with a message before any scan and after a scan of a
 * float DB.  Call dcp_gpu_sync first. */
int dcp_gpu_hit_buffer64(dcp_gpu_ctx *, void **hits_dev, void **nhits_dev, unsigned *cap);
#ifdef DCP_TEST_HOOKS
/* NOT in the shipped library: exists only in libdcp_hip_testhooks.so (the same sources compiled with
 * -DDCP_TEST_HOOKS, loaded by the tests alone).  Shrinks the per-size-class capacity of the redo lists
 * (default 2^26 pairs; 0 restores it) so a test can reach the overflow path.  Results are unaffected:
 * an overflowed scan is repeated with the row-sweep kernel. */
int dcp_gpu_test_set_redo_cap(dcp_gpu_ctx *, unsigned cap);
/* Same build only.  on != 0: in the next two-stage query-lane scans, stage 0 of the first task sits out its first
 * step, so its partner stage runs into the bound of the LDS ring's hand-shake: the kernel must drain and
 * dcp_gpu_sync must return DCP_EFAIL (never a hang). */
int dcp_gpu_test_set_ring_stall(dcp_gpu_ctx *, int on);
/* Same build only.  Cap in bytes on the boundary columns the segmented row sweep keeps per size class (0 restores the
 * default, 6 GiB): a small cap makes it sweep a class's queries chunk by chunk. */
int dcp_gpu_test_set_seg_col_bytes(dcp_gpu_ctx *, unsigned long long bytes);
/* Same build only.  own_forward != 0: dcp_gpu_trace_paths fills the hits' work areas with the trace kernel's own
 * one-wavefront forward loop (rounds 1-3) instead of the row-sweep kernels' -- the tests' second implementation of
 * the same rows; budget_floats != 0: floats of work area per round of launches (default 2^31), so that a handful of
 * hits already takes several rounds.  dcp_gpu_trace_paths64 takes budget_floats as 4-byte units of its double work
 * area and ignores own_forward (the double build has one forward pass). */
int dcp_gpu_test_set_trace_mode(dcp_gpu_ctx *, int own_forward, unsigned long long budget_floats);
/* Same build only.  Forces the grid-mode row-sweep kernel variant -- leading emission rows a block stages in
 * LDS (0, 20 or 84) and, in `block_waves`: bits 0..7 wavefronts per block (0: the default), bits 8..15 KiB of
 * unused LDS per block (an occupancy experiment), bit 16 the two-rows-ahead prefetch variant, bits 20..23 the
 * one size class (nodes per lane) to force, 0 = all, bits 24..25 the segmented sweep of the classes of more than
 * 512 nodes (1 never, 2 always, 0 the library's rule), bits 26..27 likewise the K-profiles-per-wavefront kernel of
 * the classes of at most 128 nodes -- instead of the one the library picks per size class and
 * batch size; stage < 0 restores the automatic choice.  A class without such a kernel keeps the automatic
 * one.  Every variant computes the same scores: tests/test_gpu_parity.py runs them all against the oracle. */
int dcp_gpu_test_set_rowsweep_variant(dcp_gpu_ctx *, int stage_rows, unsigned block_waves);
/* Same build only.  Profile p's raw column span of the row-sweep match tables, padding included: all 1364 rows,
 * each from the profile's first column to the next profile's first column in a shared row, or to the row's end.
 * *span receives that many columns, *ldk the rows' stride on the device, *elem_bytes 4 (float DB) or 8 (double
 * DB).  out (may be NULL: sizes only) receives [1364][span] values if cap_bytes holds them, else DCP_ENOMEM. */
int dcp_gpu_test_fetch_table_span(dcp_gpu_ctx *, unsigned p, void *out, unsigned long long cap_bytes,
                                  unsigned *span, unsigned *ldk, unsigned *elem_bytes);
#endif
/* Wait for the stream (and, after a query-lane scan, check its redo lists:
 * see dcp_gpu_last_scan_redo_pairs). */
int dcp_gpu_sync(dcp_gpu_ctx *);
/* Query-lane scans with multi_hits score a pair under B(j) = N(j) + NB and
 * verify that against the E -> B / J -> B feedback; pairs that fail the check
 * are re-scored exactly by the row-sweep kernel behind it on the same stream.
 * Their number in the last scan (0 for row-sweep and uni-hit scans);
 * synchronises. */
int dcp_gpu_last_scan_redo_pairs(dcp_gpu_ctx *, unsigned *npairs);
/* The batch plan the last scan ran with, if that scan ran kernel 4: plan blocks, rows a tile costs summed over
 * the blocks, rows of a block's planes, the most groups any slot holds.  DCP_EINVAL if the last scan ran another
 * kernel (also after an overflowed kernel-4 scan that was repeated with the row sweep) or none ran.  The plan is
 * dcp_plan_query_slots' for the scanned range's lengths in ascending order, four slots per block; synchronises. */
int dcp_gpu_last_scan_query_plan(dcp_gpu_ctx *, unsigned *nblocks, unsigned long long *sum_block_rows,
                                 unsigned *plane_rows, unsigned *max_groups_per_slot);
/* Milliseconds between HIP events recorded on the context's stream around the
 * kernels of the LAST dcp_gpu_scan (valid after dcp_gpu_sync). */
float dcp_gpu_last_scan_ms(dcp_gpu_ctx *);
/* Number of DP kernel launches of the last scan (row sweep: one per profile
 * size class; query lane: one, plus one redo launch per size class). */
unsigned dcp_gpu_last_scan_launches(dcp_gpu_ctx const *);
/* The kernel the last scan ran with, as dcp_scan_params.kernel names it (1, 2, 3, or 4 on a double DB): what
 * the cost model chose when the scan asked for 0.  A query-lane scan (2, 3 or 4) whose redo list overflowed was
 * repeated with the row sweep by dcp_gpu_sync and reports 1 from then on.  0 before any scan. */
int dcp_gpu_last_scan_kernel(dcp_gpu_ctx const *);
/* Launch i of the last scan: its kernel shape, HIP-event duration on the
 * context's stream, DP cells and algorithmic bytes.  The cells
 * of a query-lane scan are all counted in its launch 0; its redo launches
 * report 0 cells. */
struct dcp_launch_info
{
    int nodes_per_lane; /* row sweep: R; query lane: nodes per tile */
    int waves_per_pair; /* row sweep: W; query lane: 0 */
    unsigned nprofiles;
    float ms;
    uint64_t cells;
    uint64_t algorithmic_bytes;
};
int dcp_gpu_last_scan_launch_info(dcp_gpu_ctx *, unsigned i,
                                  struct dcp_launch_info *out);

/* Results of the last scan (synchronises).
 * scores: null_out/alt_out [nseqs][nprofiles] (need keep_scores).
 * hits: sorted by (seq_idx, profile_idx); returns count in *nhits; DCP_ENOMEM
 * if cap is too small (nhits still set). */
int dcp_gpu_fetch_scores(dcp_gpu_ctx *, float *null_out, float *alt_out);
int dcp_gpu_fetch_hits(dcp_gpu_ctx *, struct dcp_hit *hits, unsigned cap,
                       unsigned *nhits);
/* The same for a scan of a double DB, in double.  A float fetch after a double scan, or a double fetch after a
 * float scan, is DCP_EINVAL (with a message): results are never rounded or widened on the way out. */
int dcp_gpu_fetch_scores64(dcp_gpu_ctx *, double *null_out, double *alt_out);
int dcp_gpu_fetch_hits64(dcp_gpu_ctx *, struct dcp_hit64 *hits, unsigned cap, unsigned *nhits);
/* ------------------------------------------------------------------------ */
/* Hits -> paths -> product rows                           */
/* ------------------------------------------------------------------------ */
/* imm_step {state_id, seqlen}: state ids as include/deciphon/model/protein_state.h:7-21 */
struct dcp_step
{
    uint16_t state_id;
    uint8_t seqlen;
    uint8_t reserved;
};

/* Viterbi paths (what imm_dp_viterbi leaves in prod.path,
 * src/server/scan_thread.c:115-117) of `nhits` (seq_idx, profile_idx) pairs of the
 * resident batch / DB, computed on the device: null_model == 0 -> alt model
 * (S ... T), != 0 -> null model (R steps). Flags as in the scan that found
 * them. steps_out receives the paths back to back; step_off[nhits+1] their
 * offsets; alt_out (may be NULL) the log-likelihood the trace recomputed (equal
 * to the scan's). DCP_ENOMEM if cap_steps is too small (step_off[nhits] then
 * holds the needed total, more than cap_steps: call again with that much; a device allocation's
 * DCP_ENOMEM leaves it 0), DCP_EFAIL if a pair has no finite path or one of more than 2^32 - 3 steps.
 * A path has no bound of the form 2L + cM: in multi-hit mode each domain can cross M + 1 silent states, so a
 * path has up to L emitting steps plus M + 4 per domain.  2L + 2M + 16 per hit is a first estimate only: the call
 * traces a longer hit once more at its exact count.
 * Device work: the rows of every hit are swept once more by its size class's row-sweep kernel, which parks every
 * row's M, I, D, N, B, E, J, C in a work area (12 x 64 R W + 20 bytes per row; at most 8 GiB per round of launches,
 * kept by the context between calls), then one wavefront per hit walks back through it. */
int dcp_gpu_trace_paths(dcp_gpu_ctx *, struct dcp_hit const *hits, unsigned nhits,
                        int multi_hits, int hmmer3_compat, int null_model,
                        struct dcp_step *steps_out, unsigned cap_steps, uint32_t *step_off,
                        float *alt_out);
/* dcp_gpu_trace_paths on a double DB (dcp_gpu_db_upload64), word for word, with dcp_hit64 records and double
 * log-likelihoods: the paths of the double build's recursion on the DB's own tables, special transitions
 * dcp_xtrans64 of each hit's length and the flags (or the rows of dcp_gpu_seqs_set_xtrans64).  DCP_EINVAL on a float DB.
 * Device work: viterbi64_kernel's forward pass per launch group over the round's pairs parks every row's M, I, D
 * (24 bytes per column of the DB's padded width) and N, B, E, J, C (40 bytes) in the context's traceback work area,
 * at most 8 GiB per round of launches; one wavefront per hit walks back through it. */
int dcp_gpu_trace_paths64(dcp_gpu_ctx *, struct dcp_hit64 const *hits, unsigned nhits,
                          int multi_hits, int hmmer3_compat, int null_model,
                          struct dcp_step *steps_out, unsigned cap_steps, uint32_t *step_off,
                          double *alt_out);

/* protein_state_name (src/model/protein_state.c:5-39): "M12", "I3", "N"... */
unsigned dcp_state_name(unsigned state_id, char name[8]);
/* protein_profile_decode (src/model/protein_profile.c:306-331) = imm_frame_cond_decode:
 * most likely codon (ids 0..3) of a 1..5-nt fragment emitted by `state_id`. */
int dcp_profile_decode(dcp_profile const *, uint8_t const *frag, unsigned len,
                       unsigned state_id, uint8_t codon[3]);
/* imm_gc_decode(1, codon): amino acid letter of a codon, '*' for stops */
char dcp_gc_decode(uint8_t const codon[3]);
/* One product row exactly as prod_fwrite + protein_match_write_func write it
 * (src/server/prod.c:13-41,153-181; src/server/protein_match.c:21-56), without
 * the trailing newline handling changed: returns the number of bytes written to
 * buf (incl. the final '\n'), or -1 if cap is too small. seq: symbol ids. */
long dcp_prod_format_row(char *buf, size_t cap, int64_t scan_id, int64_t seq_id,
                         char const *profile_name, char const *abc_name,
                         double alt_loglik, double null_loglik,
                         char const *profile_typeid, char const *version,
                         dcp_profile const *prof, uint8_t const *seq, unsigned seq_len,
                         struct dcp_step const *steps, unsigned nsteps);
/* The header line prod_fclose writes (src/server/prod.c:119-121). */
char const *dcp_prod_header(void);

/* ---- The decode on the device: hits and paths in, one codon code per step out ----------------
 * The last numeric step of a product row -- for every emitting step of a path the arg-max over the 64 codons of
 * p(fragment, codon), protein_profile_decode / imm_frame_cond_decode -- computed by one wavefront per step, lane =
 * codon, from the resident 2-bit words and the profiles' compact distributions (csrc/dcp_decode.hip).
 *
 * dcp_gpu_db_keep_dists: later uploads (dcp_gpu_db_upload with any flags, dcp_gpu_db_upload64) keep the profiles'
 * compact distributions resident for dcp_gpu_decode_paths: 516 B per node (float DB), 1 032 B (double DB), plus
 * 1 104 B per profile.  Default off: uploads behave exactly as before.  A default two-layout float DB keeps them
 * anyway (it expands its row-sweep layout from them on first use) and can decode without the setting. */
int dcp_gpu_db_keep_dists(dcp_gpu_ctx *, int on);
/* 1 if the resident DB can decode (its dists are resident), else 0. */
int dcp_gpu_db_has_dists(dcp_gpu_ctx const *);

#define DCP_CODE_MUTE 0xFFu
/* For npaths (resident sequence, resident profile) pairs and their paths -- steps back to back, step_off[npaths + 1],
 * as dcp_gpu_trace_paths / ...64 leave them; alt or null paths alike -- codes_out[i] for step i = 16a + 4b + c of the
 * codon (a, b, c) dcp_profile_decode returns for that step's fragment and state, DCP_CODE_MUTE for a step that emits
 * nothing.  Amino acid = dcp_gc_decode of the codon.  One call for callers of either hit record: the precision is the
 * resident DB's (a double DB decodes from its double dists and epsilon, as dcp_profile_decode does for a double
 * profile).  I, N, J, C, R steps agree with dcp_profile_decode bit for bit, ties included (their operands are the
 * host's own exp() values, stored at upload); an M step takes exp() of its node's dist on the device and can differ
 * from the host only where two codons' joints agree to about 2^-48 relative.
 * Everything is validated on the host before any launch, and codes_out stays untouched on error.  DCP_EINVAL with a
 * message: no DB or no batch resident; the dists are not resident (see dcp_gpu_db_keep_dists); an index out of range;
 * a state id that is not M / I / D with index 1..core_size or R, S, N, B, E, J, C, T; an emitting state with seqlen
 * outside 1..5 or a mute state with seqlen != 0; a path whose seqlens sum past its sequence's length.  npaths == 0 is
 * DCP_OK.  The emitting steps go to the device in rounds of at most 2^20 (16 MiB work list, 1 MiB of codes); the call
 * runs on the context's stream and returns synchronised; the last scan's results stay valid. */
int dcp_gpu_decode_paths(dcp_gpu_ctx *, uint32_t const *seq_idx, uint32_t const *profile_idx, unsigned npaths,
                         struct dcp_step const *steps, uint32_t const *step_off, uint8_t *codes_out);

/* p(fragment, codon) for ONE given codon: the quantity dcp_profile_decode maximises, by the same arithmetic (double
 * parts for a double profile).  Host only.  DCP_EINVAL as dcp_profile_decode, or for a codon base > 3. */
int dcp_profile_codon_joint(dcp_profile const *, uint8_t const *frag, unsigned len, unsigned state_id,
                            uint8_t const codon[3], double *p);

/* dcp_prod_format_row with the steps' codes given (codes[nsteps], as dcp_gpu_decode_paths wrote them) instead of
 * decoded here.  -1 also for DCP_CODE_MUTE (or any value above 63) on an emitting step, or another value than
 * DCP_CODE_MUTE on a mute one. */
long dcp_prod_format_row_codes(char *buf, size_t cap, int64_t scan_id, int64_t seq_id,
                               char const *profile_name, char const *abc_name,
                               double alt_loglik, double null_loglik,
                               char const *profile_typeid, char const *version,
                               dcp_profile const *prof, uint8_t const *seq, unsigned seq_len,
                               struct dcp_step const *steps, unsigned nsteps, uint8_t const *codes);

/* ---- Domains: hit paths split at B .. E on the device, located on their sources, merged --------
 * A domain is one B .. E stretch of an alt path: one pass through the core model.  A multi-hit path holds one per
 * pass (joined through J), a window's edge can cut one short, and two overlapping windows report the same one. */
struct dcp_domain              /* 48 bytes, 12 uint32 words, no padding */
{
    uint32_t path;             /* index into the call's paths */
    uint32_t step_begin;       /* the B step, counted from the path's first step */
    uint32_t step_end;         /* the E step */
    uint32_t seq_begin, seq_end; /* bases of the resident sequence its steps emit, half open */
    uint32_t node_first;       /* node (1-based) of the first core step: an M */
    uint32_t node_last;        /* node of the last core step before E: an M or a D */
    uint32_t n_match, n_insert, n_delete; /* core steps by kind */
    uint32_t n_shift;          /* emitting core steps (M, I) whose seqlen != 3 */
    uint32_t reserved;         /* 0 */
};
/* For npaths (resident sequence, resident profile) pairs and their paths, given as to dcp_gpu_decode_paths -- any
 * valid path of the model graph, not only a Viterbi path -- the domains of every alt path, in path order then step
 * order: path h's are dom_out[dom_off[h] .. dom_off[h + 1]).  A path that starts with R is a null path: no domains.
 * Three sums per call, in the DB's precision and in step order with no reassociation (csrc/dcp_domains.hip), t_i the
 * transition into step i, e_i the emission of its fragment, n_i the resident NULL table's value for the same word:
 *   total_out[h] (may be NULL): s = 0; per step: if (i > 0) s = s + t_i; if (seqlen) s = s + e_i -- bit for bit the
 *     traceback's alt_out and the hit's alt_loglik (null_loglik for a null path) when the path is the Viterbi path;
 *   core_out[d]: from c = 0 at B, for every later step up to and including E: c = c + t_i; if (seqlen) c = c + e_i;
 *   null_out[d]: from n = 0 at B, over the same steps: if (seqlen) n = n + n_i.
 * A domain's sums do not depend on what lies before its B: the same domain seen from two windows gives the same bits.
 * core - null is the domain's log-odds against the null emissions (dcp_domains_merge ranks by it).  Special
 * transitions: the explicit rows while they are in force, else those of the two flags, as dcp_gpu_trace_paths takes
 * them.
 * Everything that integers decide is checked on the host before any launch -- indices, state ids, seqlen ranges, an
 * alt path starts with S, ends with T and holds no R, a null path is all R, the steps emit exactly the sequence's
 * length, every B is followed by an E before the next B and every E follows a B -- and the host counts the B steps:
 * if cap_domains is too small the call returns DCP_ENOMEM with the need in dom_off[npaths] and writes nothing else.
 * An edge that is not in the model graph (M3 -> M5, D1, B -> E ...) is found by the kernel, never scored, and the call
 * returns DCP_EINVAL naming the first such (path, step).  DCP_EINVAL with a message also: no DB or no batch resident,
 * a float call on a double DB or the reverse, a null pointer.  All outputs stay untouched on every error (but
 * dom_off[npaths] of DCP_ENOMEM).  npaths == 0 is DCP_OK.  The call runs on the context's stream and returns
 * synchronised; the last scan's results stay valid. */
int dcp_gpu_path_domains(dcp_gpu_ctx *, uint32_t const *seq_idx, uint32_t const *profile_idx, unsigned npaths,
                         struct dcp_step const *steps, uint32_t const *step_off,
                         int multi_hits, int hmmer3_compat,
                         struct dcp_domain *dom_out, unsigned cap_domains, uint32_t *dom_off /* [npaths + 1] */,
                         float *core_out, float *null_out /* [cap_domains] each */,
                         float *total_out /* [npaths], may be NULL */);
/* The same with double outputs, on a double DB. */
int dcp_gpu_path_domains64(dcp_gpu_ctx *, uint32_t const *seq_idx, uint32_t const *profile_idx, unsigned npaths,
                           struct dcp_step const *steps, uint32_t const *step_off,
                           int multi_hits, int hmmer3_compat,
                           struct dcp_domain *dom_out, unsigned cap_domains, uint32_t *dom_off,
                           double *core_out, double *null_out, double *total_out);
/* Milliseconds the domain kernel of the context's last dcp_gpu_path_domains / ...64 call ran, between two events on
 * the context's stream (copies excluded); 0 before the first call. */
float dcp_gpu_path_domains_kernel_ms(dcp_gpu_ctx *);

/* Where n domains lie on their sources.  Pure host arithmetic.  The resident batch holds `strands` x per_strand
 * sequences of res_len[] bases (strands 1 or 2; resident per_strand + i is the reverse complement of resident i);
 * resident i < per_strand is window win_src[i] + win_off[i] of its source, or source i itself if win_src is NULL (an
 * uncut batch; win_off is then not read).  For domain j on resident r = res_idx[j], i = r % per_strand, minus =
 * r >= per_strand: its interval in the window's plus coordinates is [seq_begin, seq_end), or [len - seq_end, len -
 * seq_begin) on the minus strand; begin_out / end_out add the window's offset (64 bits), src_out is the source,
 * minus_out 0 / 1.  DCP_EINVAL, nothing written: a null pointer with n > 0, strands outside 1..2, r >= strands x
 * per_strand, seq_begin > seq_end or seq_end > len. */
int dcp_domains_locate(uint32_t const *res_idx, struct dcp_domain const *dom, unsigned n, uint32_t const *res_len,
                       unsigned per_strand, unsigned strands, uint32_t const *win_src, uint32_t const *win_off,
                       uint32_t *src_out, uint64_t *begin_out, uint64_t *end_out, uint8_t *minus_out);
/* The same with the context's own lengths, strands and window map.  DCP_EINVAL with a message if no batch is
 * resident. */
int dcp_gpu_domains_locate(dcp_gpu_ctx *, uint32_t const *res_idx, struct dcp_domain const *dom, unsigned n,
                           uint32_t *src_out, uint64_t *begin_out, uint64_t *end_out, uint8_t *minus_out);
/* One representative per duplicated domain.  Within each (src, minus, profile) group the candidates are taken by
 * odds descending -- odds[j] = (double)core - (double)null: the raw core score is a log-likelihood, negative and
 * growing with length, so a stump cut by a window's edge would outrank the whole gene -- then by
 * end - begin descending, then by input index ascending; a candidate is kept unless an already kept one of its group
 * overlaps it by more than half the shorter of the two (2 ov > min(len_a, len_b), in 64 bits).  keep_out[j] = 1 / 0,
 * *nkept_out (may be NULL) the number kept.  One sort, then comparisons inside groups against kept members only.
 * DCP_EINVAL, nothing written: a null pointer with n > 0, a NaN in odds, end <= begin. */
int dcp_domains_merge(uint32_t const *src, uint8_t const *minus, uint32_t const *profile, uint64_t const *begin,
                      uint64_t const *end, double const *odds, unsigned n, uint8_t *keep_out, unsigned *nkept_out);
/* Located domains (as dcp_domains_locate returns them, BEFORE any merge) -> the regions to cut and score again
 * (dcp_gpu_seqs_cut_regions, dcp_gpu_scan_pairs).  Pure host arithmetic.  Within each (src, minus, profile) group the
 * domains go by (begin, end, input index); a domain joins the open cluster if begin <= hi + max_gap (in 64 bits), hi
 * the cluster's largest end so far, else it opens a new one.  There is no collinearity condition: tandem copies that
 * fall into one cluster are separated again by the multi-hit rescan.  A cluster [lo, hi) gives the region
 * [lo - min(lo, flank), min(hi + flank, src_len[src])).  Regions come out ordered by (src, minus, profile, begin):
 * reg_of[j] is domain j's region; per region its source, strand (0 / 1), profile, first base, length and the number
 * of domains in it.  DCP_ENOMEM with *nregions set and nothing else written if cap is too small (the region arrays
 * may be NULL for such a counting call).  DCP_EINVAL, nothing written: end <= begin, end > src_len[src], src >= nsrc,
 * a null pointer.  n == 0 is DCP_OK with 0 regions. */
int dcp_domains_regions(uint32_t const *src, uint8_t const *minus, uint32_t const *profile, uint64_t const *begin,
                        uint64_t const *end, unsigned n, uint32_t const *src_len, unsigned nsrc, uint64_t max_gap,
                        uint32_t flank, uint32_t *reg_of /* [n] */, uint32_t *reg_src, uint8_t *reg_minus,
                        uint32_t *reg_profile, uint32_t *reg_begin, uint32_t *reg_len, uint32_t *reg_nparts /* [cap] each */,
                        unsigned cap, unsigned *nregions);
/* dcp_domains_locate for a batch of regions: resident r < nres is the res_len[r] bases from reg_begin[r] of source
 * reg_src[r], reverse-complemented where reg_minus[r] != 0.  A domain [b, e) on it lies at [reg_begin + b, reg_begin +
 * e) of the source's plus strand, or at [reg_begin + len - e, reg_begin + len - b) where the region is a minus one;
 * src_out is the region's source, minus_out its flag.  DCP_EINVAL, nothing written: a null pointer with n > 0,
 * r >= nres, seq_begin > seq_end or seq_end > len.  dcp_gpu_domains_locate does this with the context's own region map
 * while the resident batch is one of regions. */
int dcp_domains_locate_regions(uint32_t const *res_idx, struct dcp_domain const *dom, unsigned n, uint32_t const *res_len,
                               unsigned nres, uint32_t const *reg_src, uint32_t const *reg_begin, uint8_t const *reg_minus,
                               uint32_t *src_out, uint64_t *begin_out, uint64_t *end_out, uint8_t *minus_out);

/* ------------------------------------------------------------------------ */
/* Calibration: a random batch, one Gumbel fit per profile, E-values */
/* ------------------------------------------------------------------------ */
/* How often does a profile reach a score on sequence that holds no gene?  Score it against random sequences, fit an
 * extreme-value (Gumbel) distribution to the scores x = alt - null, read tail probabilities off the fit.  The
 * answer holds for the sequence length, the scan flags and the base composition it was computed with, and nothing
 * else: calibrate at the window's length what dcp_gpu_seqs_cut_windows will cut.
 *
 * The generator.  Integers only, counter-based, the same on host and device; all arithmetic mod 2^64.
 *   sm(x): z = x + 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
 *          return z ^ (z >> 31)
 *   key(q) = sm(seed ^ sm(q)),  draw(q, i) = sm(key(q) + i)
 *   base b of sequence q: u = (draw(q, b >> 2) >> (16 (b & 3))) & 0xffff, id = (u >= c[0]) + (u >= c[1]) + (u >= c[2])
 * (A C G T = 0 1 2 3).  c_out[k] = floor(65536 (p_0 + .. + p_k) + 0.5) in double, at most 65 536; probs == NULL is
 * uniform: 16 384, 32 768, 49 152.  DCP_EINVAL, nothing written: a non-finite or negative entry, a sum further than
 * 1e-6 from 1, c_out NULL. */
int dcp_seq_random_thresholds(double const probs[4], uint32_t c_out[3]);
/* The len symbol ids of random sequence q under (seed, c) on the host: what dcp_gpu_seqs_random makes resident. */
void dcp_seq_random(uint64_t seed, uint32_t q, unsigned len, uint32_t const c[3], uint8_t *ids_out);
/* The resident batch is REPLACED, as by an upload, with nseqs sequences of len bases, sequence q the bases of
 * dcp_seq_random(seed, q, len, thresholds of probs), written on the device into the resident layout
 * (csrc/dcp_calib.hip, random_words_kernel): no base crosses the host.  The context is back to one strand, uncut,
 * with no regions and no explicit transitions; dcp_gpu_seqs_add_revcomp, _cut_windows and _cut_regions work afterwards
 * as after an upload, and the last scan is void.  DCP_EINVAL, with a message and the batch untouched, all checked
 * before any allocation: nseqs == 0 or len == 0; bad probs (NULL is uniform); nseqs (len / 16 + 3) past 2^32 - 1.  A
 * failed allocation leaves the context without a batch, as a failed upload does.  Works on float and double DBs
 * alike, and with no DB resident. */
int dcp_gpu_seqs_random(dcp_gpu_ctx *, unsigned nseqs, unsigned len, uint64_t seed, double const probs[4]);
/* What a fit can end with.  Distinct from enum dcp_rc, so that dcp_gumbel_fit can return either. */
enum dcp_fit_status
{
    DCP_FIT_OK = 0,
    DCP_FIT_FLAT = 16,      /* every score the same (the tail fit: or every score of the tail): nothing to fit */
    DCP_FIT_NONFINITE = 17, /* a score is +-inf or NaN (an epsilon = 0 profile on a sequence it cannot emit) */
    DCP_FIT_DIVERGED = 18,  /* a step gave a lambda not finite or not positive, or the twelfth still moved it by > 2^-40 of itself */
};
/* The maximum-likelihood Gumbel fit of x[0], x[stride], .. x[(n - 1) stride] on the host: P(X > s) = 1 - exp(-exp(
 * -lambda (s - mu))).  Double arithmetic, every sum sequential in index order (csrc/dcp_calib.h, which the device
 * kernel compiles too).  n < 2, stride == 0 or a null pointer is DCP_EINVAL, nothing written.  Pass 1: a non-finite
 * x is DCP_FIT_NONFINITE; m = min x, mean.  Pass 2: var = sum (x - mean)^2 / (n - 1); 0 is DCP_FIT_FLAT; lambda = pi /
 * sqrt(6 var).  Then exactly 12 Newton steps on the likelihood equation with y = x - m >= 0, w = exp(-lambda y), s0 =
 * sum w, s1 = sum y w, s2 = sum (y y) w, r = s1 / s0: f = 1 / lambda - (mean - m) + r, df = -1 / (lambda lambda) - s2 /
 * s0 + r r, lambda' = lambda - f / df; a lambda' that is not finite or not positive is a sticky DCP_FIT_DIVERGED, and so
 * is a last step with |lambda' - lambda| > 2^-40 lambda'.  mu = m - log(sum exp(-lambda y) / n) / lambda.  Any status
 * but DCP_FIT_OK (which is returned as it is) writes NaN to both outputs. */
int dcp_gumbel_fit(double const *x, unsigned n, size_t stride, double *mu, double *lambda);
/* The same fit, one lane per resident profile p, of x_q = (double) alt[q][p] - (double) null[q][p] over the dense
 * matrices the last scan left on the device (csrc/dcp_calib.hip, gumbel_fit_kernel): mu_out / lambda_out [nprofiles]
 * doubles, status_out [nprofiles] of enum dcp_fit_status.  Float and double DBs alike.  Host and device differ in exp,
 * log and sqrt only (DESIGN.md §17 has the bound).  The call completes the scan first (dcp_gpu_sync) and returns
 * synchronised; the scan's results stay valid.  DCP_EINVAL with a message, outputs untouched: no scan has run; the
 * last scan kept no dense scores (keep_scores == 0, or dcp_gpu_scan_pairs); it was a dcp_gpu_scan_range that did not
 * cover the whole batch; the batch holds fewer than 2 sequences; a null pointer. */
int dcp_gpu_fit_gumbel(dcp_gpu_ctx *, double *mu_out, double *lambda_out, uint8_t *status_out);
/* Exactly these three steps: dcp_gpu_seqs_random(nseqs, len, seed, probs); one dcp_gpu_scan with these flags and
 * kernel, keep_scores = 1 and lrt_threshold = +inf (no hit records; on a double DB the threshold of
 * dcp_gpu_set_lrt_threshold64 is +inf for that scan and restored behind it); dcp_gpu_fit_gumbel.  The first failing
 * step's code is returned.  The call LEAVES the random batch and that scan resident: whatever batch was there before
 * is gone, dcp_gpu_fetch_scores[64] serves the calibration's scores, and the next upload starts afresh.  Nothing is
 * kept with the DB: the caller holds mu / lambda / status and passes them to dcp_hits_evalues. */
int dcp_gpu_db_calibrate(dcp_gpu_ctx *, unsigned nseqs, unsigned len, uint64_t seed, double const probs[4], int multi_hits,
                         int hmmer3_compat, int kernel, double *mu_out, double *lambda_out, uint8_t *status_out);
/* Milliseconds, by HIP events around the kernel alone, of the context's last random_words_kernel (which = 0) or
 * gumbel_fit_kernel (1); negative if none has run. */
float dcp_gpu_calib_kernel_ms(dcp_gpu_ctx *, int which);
/* The tail fit: a censored maximum-likelihood fit, for an E-value is only ever read in the upper tail.
 * tau = the k-th largest of the n values, compared by value (zeros of either sign are one value); the observed set is
 * every x >= tau, k_eff >= k of them (more where values tie at tau), taken in index order wherever it is summed; the
 * other z = n - k_eff enter only as "below tau": log L = k_eff ln lambda - lambda sum_obs (x - mu) - sum_obs exp(-lambda
 * (x - mu)) - z exp(-lambda (tau - mu)).  The steps and statuses are dcp_gumbel_fit's: pass 1 over all n (a non-finite
 * x is DCP_FIT_NONFINITE); the whole sample's variance (0 is DCP_FIT_FLAT) and lambda = pi / sqrt(6 var); gap = (sum_obs
 * x) / k_eff - tau, and gap == 0 -- the whole observed set sits at tau -- is DCP_FIT_FLAT too; then exactly 12 Newton
 * steps with y = x - tau >= 0 over the observed set, w = exp(-lambda y), s0 = sum w + z, s1 = sum y w, s2 = sum (y y) w, r =
 * s1 / s0: f = 1 / lambda - gap + r, df = -1 / (lambda lambda) - s2 / s0 + r r, and DCP_FIT_DIVERGED as there; mu = tau -
 * log(s0 / k_eff) / lambda.  With k = n this is dcp_gumbel_fit in bits: tau the minimum, z = 0, the same sums in the same
 * order.  tau and k_eff are written with every status but DCP_FIT_NONFINITE, which writes NaN and 0; mu and lambda are
 * NaN with every status but DCP_FIT_OK.  DCP_EINVAL, nothing written: n < 2, stride == 0, k < 2, k > n, a null
 * pointer.
 *
 * The fitted law is still Gumbel(mu, lambda): dcp_gumbel_sf and dcp_hits_evalues[64] take the arrays unchanged.  But it is
 * fitted to scores >= tau[p] only.  For a hit that scores below tau[p] the E-value is at least about nsearched
 * k_eff / n -- such a hit is not significant, and its E-value is not calibrated. */
int dcp_gumbel_fit_tail(double const *x, unsigned n, size_t stride, unsigned k, double *mu, double *lambda, double *tau,
                        unsigned *k_eff);
/* The same fit, one lane per resident profile, over the dense matrices the last scan left on the device: two launches
 * (csrc/dcp_calib.hip: tail_select_kernel finds tau and k_eff by comparisons alone -- the host's bits; gumbel_fit_tail_kernel
 * differs from the host in exp, log and sqrt only).  mu_out / lambda_out / tau_out [nprofiles] doubles, status_out
 * [nprofiles] of enum dcp_fit_status, k_eff_out [nprofiles].  The preconditions, the messages and the synchronisation
 * of dcp_gpu_fit_gumbel, and the scan's results stay valid; k < 2 or k > the resident sequences is DCP_EINVAL with a
 * message too.  The outputs are untouched on every error. */
int dcp_gpu_fit_gumbel_tail(dcp_gpu_ctx *, unsigned k, double *mu_out, double *lambda_out, uint8_t *status_out,
                            double *tau_out, uint32_t *k_eff_out);
/* dcp_gpu_db_calibrate's three steps with dcp_gpu_fit_gumbel_tail(k) as the third; what it leaves resident and what it
 * restores are the same.  A null output, or k < 2 or k > nseqs, is refused before the batch is replaced. */
int dcp_gpu_db_calibrate_tail(dcp_gpu_ctx *, unsigned nseqs, unsigned len, uint64_t seed, double const probs[4],
                              int multi_hits, int hmmer3_compat, int kernel, unsigned k, double *mu_out, double *lambda_out,
                              uint8_t *status_out, double *tau_out, uint32_t *k_eff_out);
/* Milliseconds, by HIP events around the kernel alone, of the context's last tail_select_kernel (which = 0) or
 * gumbel_fit_tail_kernel (1); negative if none has run. */
float dcp_gpu_calib_tail_kernel_ms(dcp_gpu_ctx *, int which);
/* P(X > s) under the fit: -expm1(-exp(-lambda (s - mu))) -- expm1 keeps the relative precision far in the tail, where
 * the probability is exp(-lambda (s - mu)) itself. */
double dcp_gumbel_sf(double mu, double lambda, double s);
/* evalue_out[i] = nsearched * dcp_gumbel_sf(mu[p], lambda[p], (double) alt - (double) null) of hit i, p its
 * profile_idx: the number of sequences among nsearched random ones expected to score as high against profile p.  NaN
 * where status[p] != DCP_FIT_OK.  DCP_EINVAL, nothing written: a profile_idx >= nprofiles, a null pointer with n > 0,
 * nsearched not finite or negative.  ...64 takes the hits of a double DB. */
int dcp_hits_evalues(struct dcp_hit const *, unsigned n, double const *mu, double const *lambda, uint8_t const *status,
                     unsigned nprofiles, double nsearched, double *evalue_out);
int dcp_hits_evalues64(struct dcp_hit64 const *, unsigned n, double const *mu, double const *lambda, uint8_t const *status,
                       unsigned nprofiles, double nsearched, double *evalue_out);

/* ------------------------------------------------------------------------ */
/* Forward scores: the summed weight of all paths, for a list of pairs         */
/* ------------------------------------------------------------------------ */
/* Every score above is a Viterbi score, the weight of one best path.  Forward is the same recursion with every max
 * replaced by lse(c_1 .. c_n) = mm + log(sum_i exp(c_i - mm)), mm the largest c_i (0 if that is -inf), the terms added
 * in index order: the log of the summed weight of all paths.  It is computed in double whatever the tables'
 * precision (float tables are promoted, which is exact).
 *
 * The host twin, on tables of the shapes the device holds: trans8 [8][ldk] (DCP_T_* rows), emis_match [1364][ldk],
 * emis_insert [1364], emis_null [1364], xtrans as dcp_xtrans64 writes them, seq of L base ids 0..3.  Sequential in the
 * node index, every lse in the order the recursion is written.  DCP_EINVAL, nothing written: M == 0, M > 4096,
 * ldk < M, L == 0, a base id above 3, a null pointer.  DCP_ENOMEM if its rows cannot be allocated.  No device. */
int dcp_forward_tables(unsigned M, unsigned ldk, double const *trans8, double const *emis_match,
                       double const *emis_insert, double const *emis_null, double const xtrans[13],
                       unsigned char const *seq, unsigned L, double *null_out, double *alt_out);
/* The Forward scores, null and alt, of the npairs pairs (resident sequence seq_idx[i], resident profile
 * profile_idx[i]) on a float or a double DB, in list order: null_out / alt_out [npairs] doubles.  One wavefront per
 * pair (csrc/dcp_forward.hip); the host buckets the list by the kernel's classes.  The special transitions are those a
 * scan would use for the sequence: from its length and the two flags, or the explicit ones of dcp_gpu_seqs_set_xtrans /
 * ...64 while they hold (those of the other precision are refused, as a scan refuses them).  Whatever batch is
 * resident serves: uploaded, random, both strands, windows, regions.  A float DB's row-sweep tables are expanded on
 * first use, as a row-sweep scan expands them.  The call runs on the context's stream behind whatever is outstanding
 * and returns synchronised; the last scan's hits, dense scores, hit buffer and accounting stay what they were.
 * Device and host twin differ in exp and log and in the association of the delete chain and of E(j).  A pair listed
 * twice is scored twice; npairs == 0 is DCP_OK.  DCP_EINVAL with a message, outputs untouched: no DB or no batch
 * resident, a null pointer with npairs > 0, an index out of range (naming the first bad pair), explicit transitions of
 * the other precision. */
int dcp_gpu_forward_pairs(dcp_gpu_ctx *, int multi_hits, int hmmer3_compat, uint32_t const *seq_idx,
                          uint32_t const *profile_idx, unsigned npairs, double *null_out, double *alt_out);
/* Milliseconds, by HIP events around the kernel launches of the context's last dcp_gpu_forward_pairs that launched
 * any; negative before. */
float dcp_gpu_forward_kernel_ms(dcp_gpu_ctx *);

/* ------------------------------------------------------------------------ */
/* Forward E-values: the dense Forward scan and the exponential tail fit */
/* ------------------------------------------------------------------------ */
/* Every resident sequence against every resident profile with the Forward kernels: two nseqs x nprofiles double
 * matrices, null and alt, left on the device in the scan's dense layout, entry [q * nprofiles + p].  Every entry has the
 * bits dcp_gpu_forward_pairs returns for that pair with the same flags, whatever batch is resident and whichever
 * transitions hold.  No list of pairs exists on the host: it orders the profiles (by the kernels' classes, the wide ones by
 * falling width) and the sequences (by falling length), and a small kernel writes each round's pair records -- at most
 * 2^22 of them -- on the device; the order is a matter of speed alone.  nseqs x nprofiles above 2^32 - 1 is DCP_EINVAL.
 * The buffer is the call's own: a later scan or pair-list call (Forward, posterior, decoded alignment) leaves it as it
 * is, and this call leaves the last scan's hits, dense scores, hit buffer and accounting what they were.  The matrices
 * are void from the moment the DB or the batch is replaced (an upload, dcp_gpu_seqs_random, ..._add_revcomp,
 * ..._cut_windows, ..._cut_regions) or explicit transitions are set; a call that fails leaves them void as well.  The
 * call runs on the context's stream behind whatever is outstanding and returns synchronised.  DCP_EINVAL with a
 * message: no DB or no batch resident, explicit transitions of the other precision. */
int dcp_gpu_forward_dense(dcp_gpu_ctx *, int multi_hits, int hmmer3_compat);
/* The two matrices: null_out / alt_out [nseqs * nprofiles] doubles.  DCP_EINVAL with a message, outputs untouched: a
 * null pointer, or matrices that are void or were never computed. */
int dcp_gpu_fetch_forward_scores(dcp_gpu_ctx *, double *null_out, double *alt_out);
/* Milliseconds, by HIP events around all launches (every round's list kernel and sweeps) of the context's last
 * dcp_gpu_forward_dense that ran to its end; negative before. */
float dcp_gpu_forward_dense_kernel_ms(dcp_gpu_ctx *);

/* ------------------------------------------------------------------------ */
/* The scaled probability-space Forward sweep */
/* ------------------------------------------------------------------------ */
/* The Forward recursion with every value held as a probability beside a power-of-two exponent (csrc/
 * dcp_forward_scaled.h): a table value t enters as a factor -- exp(t) in double on a double DB, the float rule
 * dcp_fwd_factor_f32 on a float DB -- every lse becomes a chain of fused multiply-adds, and a score is formed once, at
 * the end.  The scores agree with dcp_forward_tables' to 2^-32 (|x| + 1) with double factors and to n(L, M) delta with
 * float factors (looser than the log-space sweep's).
 *
 * The float rule: exp of a float in -708 .. 708 as a double, by float arithmetic alone (host and device: the same
 * bits); 0 below -708 and for -inf, +inf above 708. */
double dcp_fwd_factor_f32(float t);
/* The host twin.  Arguments and refusals are dcp_forward_tables'; float_factors != 0 applies the float rule to
 * (float)t of every table value, 0 takes exp(t) in double.  *out_of_range = 1, and no score written: a value left the
 * double range (a delete chain that multiplies up, which dcp_forward_tables handles); else 0 and both scores.  A null
 * out_of_range is DCP_EINVAL too.  No device. */
int dcp_forward_scaled_tables(unsigned M, unsigned ldk, double const *trans8, double const *emis_match,
                              double const *emis_insert, double const *emis_null, double const xtrans[13],
                              unsigned char const *seq, unsigned L, int float_factors, double *null_out, double *alt_out,
                              int *out_of_range);
/* The same with the band of the rescaling rule given (1 .. 500; dcp_forward_scaled_tables: 64): the scores do not
 * depend on it. */
int dcp_forward_scaled_tables_band(unsigned M, unsigned ldk, double const *trans8, double const *emis_match,
                                   double const *emis_insert, double const *emis_null, double const xtrans[13],
                                   unsigned char const *seq, unsigned L, int float_factors, int band, double *null_out,
                                   double *alt_out, int *out_of_range);
/* dcp_gpu_forward_pairs by the scaled sweep (csrc/dcp_forward_scaled.hip): the same lists, batches, transitions,
 * refusals and messages; it returns synchronised and leaves a scan's results, and the dense Forward matrices, what they
 * were.  Pairs whose values leave the double range are collected on the device and rerun by dcp_gpu_forward_pairs'
 * kernels in the same call: those come back with dcp_gpu_forward_pairs' bits, and every returned score is valid. */
int dcp_gpu_forward_pairs_scaled(dcp_gpu_ctx *, int multi_hits, int hmmer3_compat, uint32_t const *seq_idx,
                                 uint32_t const *profile_idx, unsigned npairs, double *null_out, double *alt_out);
/* How many pairs the context's last scaled call (pair list or dense) reran in log space. */
unsigned dcp_gpu_forward_scaled_redo_pairs(dcp_gpu_ctx *);
/* Milliseconds, by HIP events around all launches (the rerun's included) of the context's last
 * dcp_gpu_forward_pairs_scaled that launched any; negative before. */
float dcp_gpu_forward_scaled_kernel_ms(dcp_gpu_ctx *);
/* dcp_gpu_forward_dense by the scaled sweep: the same list kernel, rounds, buffer and dense layout, the same lifetime
 * and voiding rules; dcp_gpu_fetch_forward_scores and dcp_gpu_fit_exp_tail(DCP_SCORES_FORWARD, ..) work on its result
 * unchanged, and dcp_gpu_forward_dense_kernel_ms covers it.  Every entry has dcp_gpu_forward_pairs_scaled's bits. */
int dcp_gpu_forward_dense_scaled(dcp_gpu_ctx *, int multi_hits, int hmmer3_compat);
/* 1 if the dense Forward matrices were filled by dcp_gpu_forward_dense_scaled, 0 if by dcp_gpu_forward_dense (or by
 * neither yet). */
int dcp_gpu_forward_dense_is_scaled(dcp_gpu_ctx *);

/* The upper tail of Forward scores is taken as exponential: P(X >= s) = exp(-lambda (s - mu)) for s >= mu.  The censored
 * maximum-likelihood fit is closed-form.  tau, the k-th largest by value, and k_eff = #{x >= tau} are dcp_gumbel_fit_tail's
 * (the same selection).  Pass 1 over all n: a non-finite x is DCP_FIT_NONFINITE.  Pass 2: so = sum (x - tau) over the
 * x >= tau in index order; so == 0 -- the whole observed set sits at tau -- is DCP_FIT_FLAT.  lambda = k_eff / so, and
 * mu = tau + log(k_eff / n) / lambda, so that the law is (k_eff / n) exp(-lambda (s - tau)): the observed fraction at tau.
 * With k = n, mu = tau = the minimum.  There is no iteration and no DCP_FIT_DIVERGED.  tau and k_eff are written with every
 * status but DCP_FIT_NONFINITE, which writes NaN and 0; mu and lambda are NaN with every status but DCP_FIT_OK.
 * DCP_EINVAL, nothing written: n < 2, stride == 0, k < 2, k > n, a null pointer.  No device.
 *
 * The law holds from tau[p] up only: a score below tau[p] has a survival of at least k_eff / n under it and is not
 * calibrated (below mu the survival is 1). */
int dcp_exp_tail_fit(double const *x, unsigned n, size_t stride, unsigned k, double *mu, double *lambda, double *tau,
                     unsigned *k_eff);
/* Which dense matrices a device fit reads: the last scan's (float or double, dcp_gpu_fit_gumbel_tail's preconditions and
 * messages) or the last dcp_gpu_forward_dense's (doubles; DCP_EINVAL with a message while they are void, or with fewer
 * than 2 sequences resident). */
enum { DCP_SCORES_SCAN = 0, DCP_SCORES_FORWARD = 1 };
/* The same fit, one lane per resident profile, of x_q = alt[q][p] - null[q][p]: two launches (csrc/dcp_calib.hip: the
 * selection of dcp_gpu_fit_gumbel_tail, then exp_tail_fit_kernel).  Given the same scores, tau, k_eff, status and lambda
 * are the host twin's bits -- comparisons, ordered sums, one division; mu differs by the side's log.  Outputs as
 * dcp_gpu_fit_gumbel_tail's, untouched on every error; k < 2 or k > the resident sequences and an unknown source are
 * DCP_EINVAL with a message.  Returns synchronised. */
int dcp_gpu_fit_exp_tail(dcp_gpu_ctx *, int source, unsigned k, double *mu_out, double *lambda_out, uint8_t *status_out,
                         double *tau_out, uint32_t *k_eff_out);
/* Milliseconds, by HIP events around the kernel alone, of the last dcp_gpu_fit_exp_tail's tail_select_kernel (which = 0)
 * or exp_tail_fit_kernel (1); negative if none has run.  (dcp_gpu_calib_tail_kernel_ms does not see these launches.) */
float dcp_gpu_exp_tail_kernel_ms(dcp_gpu_ctx *, int which);
/* Exactly three steps: dcp_gpu_seqs_random(nseqs, len, seed, probs), dcp_gpu_forward_dense(multi_hits, hmmer3_compat),
 * dcp_gpu_fit_exp_tail(DCP_SCORES_FORWARD, k); the first failing step's code.  A null output, or k < 2 or k > nseqs, is
 * refused before the batch is replaced.  The random batch and the matrices stay resident. */
int dcp_gpu_db_calibrate_forward(dcp_gpu_ctx *, unsigned nseqs, unsigned len, uint64_t seed, double const probs[4],
                                 int multi_hits, int hmmer3_compat, unsigned k, double *mu_out, double *lambda_out,
                                 uint8_t *status_out, double *tau_out, uint32_t *k_eff_out);
/* P(X >= s) under the exponential law: 1 for s <= mu, else exp(-lambda (s - mu)). */
double dcp_exp_sf(double mu, double lambda, double s);
/* dcp_hits_evalues for scores that are not hit records -- the arrays dcp_gpu_forward_pairs and dcp_gpu_scan_pairs
 * return: evalue_out[i] = nsearched * sf(mu[p], lambda[p], alt[i] - null[i]), p = profile_idx[i], sf = dcp_gumbel_sf
 * (DCP_LAW_GUMBEL) or dcp_exp_sf (DCP_LAW_EXP).  NaN where status[p] != DCP_FIT_OK.  DCP_EINVAL, nothing written: a
 * profile_idx >= nprofiles, a null pointer with n > 0, nsearched not finite or negative, an unknown law. */
enum { DCP_LAW_GUMBEL = 0, DCP_LAW_EXP = 1 };
int dcp_scores_evalues(uint32_t const *profile_idx, double const *null, double const *alt, unsigned n, double const *mu,
                       double const *lambda, uint8_t const *status, unsigned nprofiles, double nsearched, int law,
                       double *evalue_out);

/* ------------------------------------------------------------------------ */
/* Backward sweep and posterior decoding for a list of pairs                   */
/* ------------------------------------------------------------------------ */
/* With the Backward value of a state at row j -- the log of the summed weight of all path suffixes from it to the end
 * (csrc/dcp_posterior.h has the recursion) -- every pair gets three rows of L + 1 doubles, j = 0 .. L:
 *   begin[j]  the posterior that a domain begins at row j:  exp(B(j) + bB(j) - a), a the Forward alt score;
 *   end[j]    the posterior that a domain ends at row j:    exp(E(j) + bE(j) - a); end[0] = 0;
 *   core[j]   the posterior that base j - 1 is emitted by a core state (M or I): 1 minus the posteriors of the at most
 *             15 words of each of N, J, C that cover the base; core[0] = 0.
 * sum(begin) = sum(end) is the expected number of domains.  When a is -inf the three rows are 0, never NaN.  The alt
 * score comes back by both sweeps: alt_fwd (the bits of dcp_forward_tables / dcp_gpu_forward_pairs) and alt_bwd, which
 * agree within the scores' allowance.
 *
 * The host twin takes dcp_forward_tables' tables and refuses as it does (a null output too), nothing written.  It holds
 * the full matrices of the Backward sweep: the tests' yardstick, no hot path.  No device. */
int dcp_posterior_tables(unsigned M, unsigned ldk, double const *trans8, double const *emis_match,
                         double const *emis_insert, double const *emis_null, double const xtrans[13],
                         unsigned char const *seq, unsigned L, double *begin_out, double *end_out, double *core_out,
                         double *alt_fwd_out, double *alt_bwd_out);
/* Envelopes from a core row [L + 1]: the maximal runs of bases with core >= threshold that are at least min_len bases
 * long, as half-open base intervals [begin_out[i], end_out[i]) in order.  *n_out receives the true count, of which the
 * first cap are written.  DCP_EINVAL: n_out null, core null with L > 0, an output null with cap > 0, threshold NaN.
 * No device. */
int dcp_posterior_envelopes(double const *core, unsigned L, double threshold, unsigned min_len, unsigned *begin_out,
                            unsigned *end_out, unsigned cap, unsigned *n_out);
/* The three rows and the two alt scores of the npairs pairs (resident sequence seq_idx[i], resident profile
 * profile_idx[i]), in list order: pair i's rows are [row_off[i], row_off[i + 1]) of begin_out / end_out / core_out
 * [cap_rows], L_i + 1 of them; row_off [npairs + 1] is written by the call; alt_fwd_out / alt_bwd_out [npairs].
 * Device work: the Forward kernels in a variant that also stores five doubles a row, a Backward sweep of the same
 * shape (one wavefront per pair, csrc/dcp_posterior.hip) and a combining kernel, one thread per row.  The two sweeps'
 * row records live in device memory of the call's own, bounded by a budget (1 GiB): a longer list runs in rounds, a
 * single pair that exceeds it in a round of its own.  Checks, messages, special transitions, batches, precisions,
 * stream and what is left untouched: all as dcp_gpu_forward_pairs.  DCP_EINVAL, outputs untouched, also when cap_rows
 * is smaller than the rows the list needs (the message names the need).  After a device failure in a later round the
 * rows of the rounds before are written. */
int dcp_gpu_posterior_pairs(dcp_gpu_ctx *, int multi_hits, int hmmer3_compat, uint32_t const *seq_idx,
                            uint32_t const *profile_idx, unsigned npairs, uint64_t *row_off, double *begin_out,
                            double *end_out, double *core_out, uint64_t cap_rows, double *alt_fwd_out, double *alt_bwd_out);
/* Milliseconds, by HIP events, summed over the rounds' kernel launches of the context's last dcp_gpu_posterior_pairs
 * that launched any; negative before. */
float dcp_gpu_posterior_kernel_ms(dcp_gpu_ctx *);

/* ------------------------------------------------------------------------ */
/* The scaled probability-space Backward sweep and posterior rows */
/* ------------------------------------------------------------------------ */
/* dcp_posterior_tables with both sweeps in the scaled representation of §24 (csrc/dcp_backward_scaled.h): values are
 * probabilities beside a power-of-two exponent, a row's five record values are turned into logs once per row, and the
 * rows are combined by the same rule.  float_factors as dcp_forward_scaled_tables.  Arguments and refusals are
 * dcp_posterior_tables' (a null out_of_range is DCP_EINVAL too).  *out_of_range = 1, nothing else written: a value left
 * the double range in either sweep, or a row's records may have lost a term of 2^-64 or more of a posterior to underflow
 * (F + Bk - a > (958 - band) ln 2 for the largest record values F, Bk of the two sweeps at a row and the Forward alt
 * score a); else 0 and every output.  alt_fwd_out has dcp_forward_scaled_tables' bits.  No device. */
int dcp_posterior_scaled_tables(unsigned M, unsigned ldk, double const *trans8, double const *emis_match,
                                double const *emis_insert, double const *emis_null, double const xtrans[13],
                                unsigned char const *seq, unsigned L, int float_factors, double *begin_out, double *end_out,
                                double *core_out, double *alt_fwd_out, double *alt_bwd_out, int *out_of_range);
/* The same with the band of the rescaling rule given (1 .. 500; dcp_posterior_scaled_tables: 64).  The scores and rows of
 * a pair that is in range under both bands do not depend on it; which pairs the underflow check flags does. */
int dcp_posterior_scaled_tables_band(unsigned M, unsigned ldk, double const *trans8, double const *emis_match,
                                     double const *emis_insert, double const *emis_null, double const xtrans[13],
                                     unsigned char const *seq, unsigned L, int float_factors, int band, double *begin_out,
                                     double *end_out, double *core_out, double *alt_fwd_out, double *alt_bwd_out,
                                     int *out_of_range);
/* dcp_gpu_posterior_pairs by the scaled sweeps (csrc/dcp_forward_scaled.hip's row-storing variant and csrc/
 * dcp_backward_scaled.hip): the same signature, checks, messages, rounds, outputs and synchronisation.  Pairs that either
 * sweep flags are collected on the device and rerun, both sweeps, by dcp_gpu_posterior_pairs' kernels before the round's
 * rows are combined: those come back with dcp_gpu_posterior_pairs' bits, and every returned row is valid.  alt_fwd_out
 * of a pair that was not rerun has dcp_gpu_forward_pairs_scaled's bits. */
int dcp_gpu_posterior_pairs_scaled(dcp_gpu_ctx *, int multi_hits, int hmmer3_compat, uint32_t const *seq_idx,
                                   uint32_t const *profile_idx, unsigned npairs, uint64_t *row_off, double *begin_out,
                                   double *end_out, double *core_out, uint64_t cap_rows, double *alt_fwd_out,
                                   double *alt_bwd_out);
/* How many pairs the context's last dcp_gpu_posterior_pairs_scaled reran in log space, over all its rounds. */
unsigned dcp_gpu_posterior_scaled_redo_pairs(dcp_gpu_ctx *);
/* Milliseconds, by HIP events, summed over the rounds' launches (the reruns included) of the context's last
 * dcp_gpu_posterior_pairs_scaled that launched any; negative before. */
float dcp_gpu_posterior_scaled_kernel_ms(dcp_gpu_ctx *);

/* ------------------------------------------------------------------------ */
/* Posterior-decoded (maximum expected accuracy) alignment for a list of pairs */
/* ------------------------------------------------------------------------ */
/* Every path above is a Viterbi path.  The posterior-decoded path is chosen by what all paths say about each step: with
 * the word posterior w of an emitting step (state, s, l) -- exp(Forward value the word leaves from + its emission +
 * Backward value where it arrives - a), a the Forward alt score; csrc/dcp_mea.h has the rule -- the gain of a path is the
 * sum of l w over its emitting steps, the expected number of bases the true path emits with the same word of the same
 * state, 0 <= gain <= L.  The decoded path is an S .. T path of the alt model graph, over finite transitions and
 * emissions only (its dcp_gpu_path_domains total is finite), that emits exactly L bases and has the largest gain: the
 * scan's recursion with every transition replaced by 0 or -inf, every emission by l w or -inf, every combiner by max,
 * ties to the first candidate in dcp_mea.h's order.  Steps are those dcp_gpu_trace_paths writes for an alt path (S, N
 * words, B, core steps, E, J / C words, T): dcp_gpu_decode_paths and dcp_gpu_path_domains take them as they are.  It is
 * optimal for the gain, not for likelihood: its total is at most the Viterbi score.  When a is -inf there is no such
 * path: zero steps, gain -inf, no error.
 *
 * The host twins take dcp_forward_tables' tables and refuse as dcp_posterior_tables does, nothing written; they hold
 * full matrices of both sweeps: the tests' yardstick, no hot path.  No device.
 * dcp_mea_tables: the decoded path into steps_out [cap_steps], post_out[i] the word posterior of step i (-1.0 for a step
 * that emits nothing), its gain and a (dcp_forward_tables' bits).  *nsteps_out is the true count; if it exceeds
 * cap_steps the call returns DCP_ENOMEM and writes nothing else.  steps_out and post_out may be NULL with cap_steps 0. */
int dcp_mea_tables(unsigned M, unsigned ldk, double const *trans8, double const *emis_match, double const *emis_insert,
                   double const *emis_null, double const xtrans[13], unsigned char const *seq, unsigned L,
                   struct dcp_step *steps_out, unsigned cap_steps, unsigned *nsteps_out, double *post_out,
                   double *gain_out, double *alt_fwd_out);
/* The gain and the per-step word posteriors (post_out [nsteps], may be NULL) of any given alt path under the same
 * sweeps: how good a Viterbi path, or a device path, is by this measure.  Of dcp_mea_tables' own path it returns the
 * reported gain and posteriors bit for bit.  DCP_EINVAL, nothing written: the path is not S .. T, uses an edge that is
 * not in the graph or a transition or emission that is -inf, does not emit exactly L bases, names a node outside
 * 1 .. M, or is NULL. */
int dcp_mea_path_gain(unsigned M, unsigned ldk, double const *trans8, double const *emis_match, double const *emis_insert,
                      double const *emis_null, double const xtrans[13], unsigned char const *seq, unsigned L,
                      struct dcp_step const *steps, unsigned nsteps, double *gain_out, double *post_out);
/* The decoded paths of the npairs pairs (resident sequence seq_idx[i], resident profile profile_idx[i]), in list order:
 * pair i's steps are [step_off[i], step_off[i + 1]) of steps_out / post_out [cap_steps] (post_out may be NULL);
 * step_off [npairs + 1] is written by the call; gain_out / alt_fwd_out [npairs] (alt_fwd: dcp_gpu_forward_pairs' bits).
 * Device work (csrc/dcp_mea.hip): the Forward and Backward kernels in a variant that also stores their core-state
 * matrices (P, Q, bM, bI: 32 bytes a cell of L + 1 rows by M nodes), a max-plus sweep over the word posteriors formed
 * from them, one wavefront per pair, which parks 13 bits of choices a cell (2 bytes) and 8 bytes a row, and a walk, one
 * thread per pair.  Matrices, choices and row records live in device memory of the call's own, bounded by a budget
 * (8 GiB): a longer list runs in rounds of consecutive pairs, a single pair that exceeds it in a round of its own.
 * Device and host twin differ in exp and log and in the association of the two sweeps' sums, so among candidates whose
 * gains are equal within that error they may choose differently: the device's path has, on the host's numbers, the
 * host's optimum within the error of the two gains.  Checks, messages, special transitions, batches, precisions, stream
 * and what is left untouched: all as dcp_gpu_forward_pairs.  DCP_ENOMEM if the paths hold more than cap_steps steps:
 * step_off is written in full (step_off[npairs] is the need) and every other output stays untouched.  A pair listed
 * twice is decoded twice; npairs == 0 is DCP_OK. */
int dcp_gpu_mea_pairs(dcp_gpu_ctx *, int multi_hits, int hmmer3_compat, uint32_t const *seq_idx,
                      uint32_t const *profile_idx, unsigned npairs, struct dcp_step *steps_out, unsigned cap_steps,
                      uint32_t *step_off, double *post_out, double *gain_out, double *alt_fwd_out);
/* Milliseconds, by HIP events, summed over the rounds' kernel launches of the context's last dcp_gpu_mea_pairs that
 * ran all its rounds -- one that then returned DCP_ENOMEM for its cap_steps included; negative before. */
float dcp_gpu_mea_kernel_ms(dcp_gpu_ctx *);

/* ------------------------------------------------------------------------ */
/* Posterior envelopes of a pair list, found on the device       */
/* ------------------------------------------------------------------------ */
/* An envelope of a pair is a maximal run [b, e) of bases with core[i + 1] >= lo (core: dcp_posterior_tables' row) that
 * is at least min_len bases long and whose largest core value is >= hi: a run needs a peak and is extended down to the
 * lower threshold.  With lo == hi the intervals are dcp_posterior_envelopes'.  The rule is csrc/dcp_envelopes.h, which
 * the device kernels (csrc/dcp_envelopes.hip) and the host twin compile alike. */
struct dcp_envelope
{
    uint32_t pair;       /* index into the call's list                                   */
    uint32_t begin, end; /* half-open base interval in the resident sequence             */
    uint32_t peak;       /* first base of the run at which core is largest               */
    double core_max;     /* core[peak + 1]                                               */
    double core_sum;     /* sum of core[i + 1], i in [b, e): expected core-emitted bases */
    double begin_sum;    /* sum of begin[j], j in [b, e - 1]: expected domain starts     */
    double end_sum;      /* sum of end[j],   j in [b + 1, e]: expected domain ends       */
};
/* The host twin, from one pair's three rows [L + 1]: the kept runs in order of begin, pair = 0, the sums in index order.
 * *n_out receives the true count, of which the first cap are written.  DCP_EINVAL, nothing written: n_out null, a row
 * null with L > 0, out null with cap > 0, hi or lo NaN, lo > hi.  No device. */
int dcp_posterior_envelope_records(double const *begin, double const *end, double const *core, unsigned L, double hi,
                                   double lo, unsigned min_len, struct dcp_envelope *out, unsigned cap, unsigned *n_out);
/* The envelopes of the npairs pairs (resident sequence seq_idx[i], resident profile profile_idx[i]): the sweeps, rounds,
 * budget (1 GiB of row records), redo of flagged pairs and combining kernel of dcp_gpu_posterior_pairs_scaled (scaled
 * != 0) or dcp_gpu_posterior_pairs (scaled == 0), but a round's three rows stay in device memory: two kernels, one
 * wavefront per pair, count the round's envelopes and write their records, and only counts and records are copied out.
 * Pair i's records are [env_off[i], env_off[i + 1]) of env_out [cap_env], in order of begin; env_off [npairs + 1] is
 * written by the call; alt_fwd_out / alt_bwd_out [npairs] have the bits of the posterior call of the same sweeps.
 * pair, begin, end, peak and core_max equal the host twin's on the same rows bit for bit; the three sums are a run's
 * own terms added in another order: within (end - begin) 2^-52 sum |term| of the twin's.  A pair listed twice is
 * reported twice; a pair whose alt score is -inf has rows of 0; npairs == 0 is DCP_OK with env_off[0] = 0.
 * Checks, messages, special transitions, batches, precisions, stream and what is left untouched: all as
 * dcp_gpu_forward_pairs.  DCP_EINVAL, nothing written, also: env_off null, env_out null with cap_env > 0, hi or lo NaN,
 * lo > hi.  DCP_ENOMEM if the list has more than cap_env envelopes: env_off is written in full (env_off[npairs] is
 * the need) and every other output stays untouched. */
int dcp_gpu_envelope_pairs(dcp_gpu_ctx *, int multi_hits, int hmmer3_compat, int scaled, uint32_t const *seq_idx,
                           uint32_t const *profile_idx, unsigned npairs, double hi, double lo, unsigned min_len,
                           struct dcp_envelope *env_out, uint64_t cap_env, uint64_t *env_off, double *alt_fwd_out,
                           double *alt_bwd_out);
/* Milliseconds, by HIP events, summed over the rounds' launches (sweeps, reruns, combining and envelope kernels) of
 * the context's last dcp_gpu_envelope_pairs that ran all its rounds -- one that then returned DCP_ENOMEM for its
 * cap_env included; negative before. */
float dcp_gpu_envelope_kernel_ms(dcp_gpu_ctx *);
/* Envelopes as regions for dcp_gpu_seqs_cut_regions: envelope k gives the stretch [max(begin - flank, 0),
 * min(end + flank, L)) of resident sequence seq_idx[env[k].pair], L = seq_len[that sequence]: src_out[k], begin_out[k],
 * len_out[k]; profile_pair_out[k] = env[k].pair, the list entry whose profile the region is to be scored against.
 * DCP_EINVAL, nothing written: a pair >= npairs, a sequence index >= nseqs, end > L, begin >= end, a null pointer with
 * n > 0.  No device. */
int dcp_envelopes_regions(struct dcp_envelope const *env, uint64_t n, uint32_t const *seq_idx, unsigned npairs,
                          uint32_t const *seq_len, unsigned nseqs, unsigned flank, uint32_t *src_out,
                          uint32_t *begin_out, uint32_t *len_out, uint32_t *profile_pair_out);

/* ------------------------------------------------------------------------ */
/* One process per GPU: profile shards + the hit gather over RCCL */
/* ------------------------------------------------------------------------ */
/* Pairs (profile, query) are independent: every rank keeps a contiguous profile shard (balanced by sum
 * of core sizes = DP cells) resident and scans ALL queries against it; the only exchange of the path
 * is the gather of the hit records: 16-byte struct dcp_hit after scans of a float DB, 24-byte struct dcp_hit64 after
 * scans of a double DB (the ...64 calls below; one communicator serves both in turn).  librccl.so is loaded on first
 * use. */
typedef struct dcp_dist dcp_dist;
enum { DCP_DIST_ID_BYTES = 128 }; /* NCCL_UNIQUE_ID_BYTES */
enum { DCP_DIST_META_WORDS = 3 }; /* per rank in the meta all-gather: records held, profile offset, records found */
/* "records found" of a rank whose scan FAILED (it holds 0 records): not a count, a status every rank reads */
#define DCP_DIST_FOUND_FAILED 0xFFFFFFFFu
/* Rank 0 creates the communicator id (ncclGetUniqueId) and hands it to the other ranks through
 * whatever channel the launcher has (bench.py: torch.distributed; a C launcher: the file variant). */
int dcp_dist_unique_id(unsigned char id[DCP_DIST_ID_BYTES]);
dcp_dist *dcp_dist_init(unsigned char const id[DCP_DIST_ID_BYTES], int rank, int nranks, int device);
/* Rendezvous through a file: rank 0 writes the id to `path`, the others wait up to timeout_s for it.
 * Ranks holding different ids would block in ncclCommInitRank, so a peer must tell this run's file from a
 * left-over one.  _run: the launcher gives every rank the same non-zero `run_nonce` (its pid and start time,
 * say); rank 0 writes it into the file and a peer takes ONLY a file carrying it -- safe for back-to-back runs
 * at one path.  Without a nonce (the second form = run_nonce 0) `path` must be FRESH for every run: rank 0
 * removes what lies there before creating its id, and the other ranks refuse a file of another layout or rank
 * count or one written more than 120 s before they arrived. */
dcp_dist *dcp_dist_init_from_file_run(char const *path, uint64_t run_nonce, int rank, int nranks, int device,
                                      double timeout_s);
dcp_dist *dcp_dist_init_from_file(char const *path, int rank, int nranks, int device, double timeout_s);
void dcp_dist_free(dcp_dist *);
int dcp_dist_rank(dcp_dist const *);
int dcp_dist_nranks(dcp_dist const *);
/* Diagnostics for the launcher: the rank count RCCL itself reports for the communicator (ncclCommCount; must
 * equal dcp_dist_nranks; -1 without one), and the wall time of this rank's last gather in ms. */
int dcp_dist_comm_count(dcp_dist const *);
double dcp_dist_last_gather_ms(dcp_dist const *);
char const *dcp_dist_last_error(dcp_dist const *);
/* [begin, end) of rank's shard: dcp_partition_by_cells over nranks. */
void dcp_dist_shard(unsigned const *core_sizes, unsigned nprofiles, int nranks, int rank, unsigned *begin,
                    unsigned *end);
/* Gather the hit records of every rank's last scan -- the form hosts call: completes the scan of `ctx`
 * first (dcp_gpu_sync: a query-lane scan finishes its redo pairs there, and a scan whose redo lists
 * overflowed is repeated with the row sweep, so the list that travels is final), then gathers the buffer
 * that scan wrote.  profile_offset: first global profile index of this rank's shard (records carry
 * shard-local indices).  {held, offset, found} of every rank travel in one 3-word all-gather, the records
 * in one grouped ncclSend/ncclRecv (gather-v).  root >= 0: only that rank receives; root < 0: every rank
 * does.  On a receiving rank *out is a malloc'ed array (dcp_dist_free_hits) of *nout records with GLOBAL
 * profile indices, ordered by (seq_idx, profile_idx); elsewhere *out = NULL and *nout = the global total.
 * If ANY rank's scan found more hits than its buffer holds, every rank still completes both exchanges
 * with the records there are (nobody is left waiting) and then EVERY rank returns DCP_ENOMEM -- on a
 * receiving rank with *out set to the incomplete list.  A rank whose scan FAILED (dcp_gpu_sync /
 * dcp_gpu_hit_buffer returned an error) takes part in both exchanges holding nothing and marks its meta
 * words (found = DCP_DIST_FOUND_FAILED): it returns its scan's error, and EVERY other rank returns DCP_EFAIL
 * -- a root never gets DCP_OK for a list that lacks one shard's hits (*out, if set, is that incomplete list;
 * free it).  More than 2^32 - 1 records in all: DCP_EINVAL everywhere. */
int dcp_dist_gather_scan_hits(dcp_dist *, dcp_gpu_ctx *ctx, unsigned profile_offset, int root,
                              struct dcp_hit **out, unsigned *nout);
/* The same for an explicit device buffer (hits_dev / nhits_dev / cap as given to dcp_gpu_set_hit_buffer).
 * The caller must have completed the scan with dcp_gpu_sync(ctx) -- synchronising the stream alone (what
 * a non-NULL scan_stream does here) does not check the redo lists of a query-lane scan. */
int dcp_dist_gather_hits(dcp_dist *, void const *hits_dev, void const *nhits_dev, unsigned cap,
                         unsigned profile_offset, int root, void *scan_stream, struct dcp_hit **out,
                         unsigned *nout);
/* What every rank derives from the gathered meta words ({held, profile_offset, found} x nranks): counts,
 * offsets, 64-bit displacements displ[nranks + 1], whether any rank overflowed (found > held), whether any
 * rank's scan failed (found = DCP_DIST_FOUND_FAILED, held = 0), the total.  Host only.
 * DCP_EINVAL when the total exceeds 2^32 - 1 or a rank holds more than it found. */
int dcp_dist_gather_plan(uint32_t const *meta, int nranks, unsigned *counts, unsigned *profile_offset,
                         uint64_t *displ, int *any_overflow, int *any_failed, uint64_t *total);
void dcp_dist_free_hits(struct dcp_hit *hits);
/* The bookkeeping of the gather alone (host, no device, no RCCL): counts[r] records of rank r lie back
 * to back in `records`; out receives them with profile_idx += profile_offset[r], ordered by
 * (seq_idx, profile_idx).  Returns the total, -1 if cap is too small. */
long dcp_dist_merge_hits(unsigned const *counts, unsigned const *profile_offset, int nranks,
                         struct dcp_hit const *records, struct dcp_hit *out, unsigned cap);
/* The double twins, for the shards of a double DB (dcp_dist_shard, dcp_gpu_db_upload64 of the shard, the scan): the
 * same contracts word for word -- collective discipline, return codes and messages included -- on struct dcp_hit64.
 * The meta all-gather and dcp_dist_gather_plan are shared; the records travel as 6 uint32 words each and are copied,
 * never converted: a record leaves the gather with the bits the kernel wrote.  dcp_dist_gather_scan_hits64 runs
 * dcp_gpu_sync, then dcp_gpu_hit_buffer64: a context whose last scan ran on a float DB, or that never scanned, holds no
 * such records and counts as a rank whose scan failed (it returns that call's DCP_EINVAL and message, its peers
 * DCP_EFAIL). */
int dcp_dist_gather_scan_hits64(dcp_dist *, dcp_gpu_ctx *ctx, unsigned profile_offset, int root,
                                struct dcp_hit64 **out, unsigned *nout);
int dcp_dist_gather_hits64(dcp_dist *, void const *hits_dev, void const *nhits_dev, unsigned cap,
                           unsigned profile_offset, int root, void *scan_stream, struct dcp_hit64 **out,
                           unsigned *nout);
void dcp_dist_free_hits64(struct dcp_hit64 *hits);
long dcp_dist_merge_hits64(unsigned const *counts, unsigned const *profile_offset, int nranks,
                           struct dcp_hit64 const *records, struct dcp_hit64 *out, unsigned cap);

/* Dynamic batching of the query-lane kernels, host side only (what dcp_gpu_scan does with a batch whose automatic
 * or forced kernel is a query-lane one): the queries in ascending length order are cut into groups of 64 -- one
 * wavefront's lanes -- and the groups are packed into wavefront slots (4 per 256-lane block, 1 for the
 * 64-lane variant) so that the slots of every block carry about the same number of DP rows; a slot sweeps its
 * groups one after the other.  len_sorted: ascending lengths.  Out: the block count, the rows a tile costs summed
 * over the blocks (each block's longest slot: the kernel-choice model's figure), the longest slot's rows; optionally
 * the groups as 4 words each {first query (index into the sorted order), queries, first plane row, longest member}
 * in slot order and slot_first[nblocks * slots + 1].  DCP_EINVAL for unsorted input, DCP_ENOMEM if a capacity
 * (group_cap in groups, slot_cap in words) is too small. */
int dcp_plan_query_slots(unsigned const *len_sorted, unsigned nq, unsigned slots_per_block, unsigned *nblocks,
                         unsigned long long *sum_block_rows, unsigned *plane_rows, unsigned *groups4,
                         unsigned group_cap, unsigned *slot_first, unsigned slot_cap);

/* Work accounting of the last scan (or of a full scan if none ran yet):
 * alt-model DP cells = sum over pairs of core_size * L (the Gcell/s numerator)
 * and the algorithmic bytes of SURVEY.md §8(d): sum over pairs of
 * 20*M*L + 32*(M+1) + L + 8. */
uint64_t dcp_gpu_scan_cells(dcp_gpu_ctx const *);
uint64_t dcp_gpu_scan_algorithmic_bytes(dcp_gpu_ctx const *);

#ifdef __cplusplus
}
#endif
#endif
