/* host_internal.h -- shared by the C files of the host layer (not installed). */
#ifndef DCP_HOST_INTERNAL_H
#define DCP_HOST_INTERNAL_H

#include "deciphon_host.h"

/* positions in protein_profile.xtrans / dcp_xtrans() output (the values protein_profile_setup writes,
 * src/model/protein_profile.c:190-214) */
enum
{
    DCP_HOST_X_RR = 0,
    DCP_HOST_X_SB = 1,
    DCP_HOST_X_SN = 2,
    DCP_HOST_X_NN = 3,
    DCP_HOST_X_NB = 4,
    DCP_HOST_X_ET = 5,
    DCP_HOST_X_EC = 6,
    DCP_HOST_X_CC = 7,
    DCP_HOST_X_CT = 8,
    DCP_HOST_X_EB = 9,
    DCP_HOST_X_EJ = 10,
    DCP_HOST_X_JJ = 11,
    DCP_HOST_X_JB = 12,
};

/* ---- one source, two builds ------------------------------------------------------------------------------
 * imm_float is float or (IMM_DOUBLE_PRECISION) double; the calls below are the C-ABI's float forms or their
 * double twins, so that a value travels from the .dcp file to the product row in the build's own precision
 * and is never converted on the way. */
#ifdef IMM_DOUBLE_PRECISION
typedef struct dcp_hit64 dcph_hit;
#define dcph_profile_new dcp_profile_new64
#define dcph_profile_sample dcp_profile_sample64
#define dcph_profile_from_parts dcp_profile_from_parts64
#define dcph_profile_trans8 dcp_profile_trans8_64
#define dcph_profile_null_dist dcp_profile_null_dist64
#define dcph_profile_insert_dist dcp_profile_insert_dist64
#define dcph_profile_match_dist dcp_profile_match_dist64
#define dcph_xtrans dcp_xtrans64
#define dcph_lprob_normalize dcp_lprob_normalize64
#define dcph_db_upload(ctx, profiles, n) dcp_gpu_db_upload64((ctx), (profiles), (n))
#define dcph_seqs_set_xtrans dcp_gpu_seqs_set_xtrans64
#define dcph_fetch_scores dcp_gpu_fetch_scores64
#define dcph_fetch_hits dcp_gpu_fetch_hits64
#define dcph_trace_paths dcp_gpu_trace_paths64
#define DCPH_1DARRAY_FLOAT LIP_1DARRAY_F64
#define dcph_write_float lip_write_f64
#define dcph_read_float lip_read_f64
#define dcph_write_1darray_float_data lip_write_1darray_f64_data
#define dcph_read_1darray_float_data lip_read_1darray_f64_data
#else
typedef struct dcp_hit dcph_hit;
#define dcph_profile_new dcp_profile_new
#define dcph_profile_sample dcp_profile_sample
#define dcph_profile_from_parts dcp_profile_from_parts
#define dcph_profile_trans8 dcp_profile_trans8
#define dcph_profile_null_dist dcp_profile_null_dist
#define dcph_profile_insert_dist dcp_profile_insert_dist
#define dcph_profile_match_dist dcp_profile_match_dist
#define dcph_xtrans dcp_xtrans
#define dcph_lprob_normalize dcp_lprob_normalize
#define dcph_db_upload(ctx, profiles, n) dcp_gpu_db_upload((ctx), (profiles), (n), 0)
#define dcph_seqs_set_xtrans dcp_gpu_seqs_set_xtrans
#define dcph_fetch_scores dcp_gpu_fetch_scores
#define dcph_fetch_hits dcp_gpu_fetch_hits
#define dcph_trace_paths dcp_gpu_trace_paths
#define DCPH_1DARRAY_FLOAT LIP_1DARRAY_F32
#define dcph_write_float lip_write_f32
#define dcph_read_float lip_read_f32
#define dcph_write_1darray_float_data lip_write_1darray_f32_data
#define dcph_read_1darray_float_data lip_read_1darray_f32_data
#endif

#ifdef IMM_DOUBLE_PRECISION
/* the float64 forms of the lite_pack subset (dcp_lip.c): a MessagePack float64, and the elements of a 1darray
 * of type LIP_1DARRAY_F64, big-endian.  Only the double build has them; they are not part of the installed
 * header, whose function list both libraries export. */
bool lip_write_f64(struct lip_file *file, double val);
bool lip_read_f64(struct lip_file *file, double *val);
bool lip_write_1darray_f64_data(struct lip_file *file, unsigned size, double const *data);
bool lip_read_1darray_f64_data(struct lip_file *file, unsigned size, double *data);
#endif

/* log at the point of detection, return the code (include/deciphon/core/logging.h:32-72) */
enum rc dcp_host_fail(enum rc rc, char const *fmt, ...) __attribute__((format(printf, 2, 3)));
enum rc dcp_host_path_assign(struct imm_path *path, struct dcp_step const *steps, unsigned n);
uint8_t *dcp_host_seq_ids(struct imm_seq const *seq, enum rc *rc);
void dcp_host_forget_profile(dcp_profile *impl);
enum rc dcp_host_adopt(struct protein_profile *p, dcp_profile *impl, int rc);
/* another FILE* on the file behind fp, with a position of its own (NULL on failure) */
FILE *dcp_host_reopen(FILE *fp);

#endif
