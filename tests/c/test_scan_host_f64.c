/*
 * GPU test of the host layer's DOUBLE build (compiled with -DIMM_DOUBLE_PRECISION against
 * libdeciphon_host_f64.so): a database pressed in double, scanned through thread_run (one sequence at a time),
 * thread_run_batch and scan_run_source (1 and 2 partitions, several pass sizes).  Their product rows must be
 * byte-identical to each other and to rows assembled from the C-ABI directly -- dcp_gpu_db_upload64 -> scan ->
 * dcp_gpu_fetch_hits64 -> dcp_gpu_trace_paths64 -> dcp_prod_format_row -- on profiles built by dcp_profile_new64
 * from the same parameters: that direct path is what tests/test_f64_scan.py, test_f64_bits.py and
 * test_f64_trace.py hold to the oracle's double build.  Among the hits: a multi-domain one whose path exceeds the
 * first step estimate (2L + 2M + 16) and a profile of more than 256 nodes.
 * The LRT threshold is applied in double: a hit's own LRT keeps its row, the next double above it drops it.
 *
 *   test_scan_host_f64                    all checks
 *   test_scan_host_f64 viterbi <out>      imm_dp_viterbi after imm_dp_change_trans on sampled profiles: one line
 *                                         per case for tests/test_c_host_f64.py to hold against the oracle --
 *                                         seed M entry_dist sequence, then as hex bits epsilon, the 13 transitions, null and
 *                                         alt loglik
 * Exit status = number of failed checks.
 */
#include "deciphon_host.h"
#include <inttypes.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#ifndef IMM_DOUBLE_PRECISION
#error "this test is the double build's: compile it with -DIMM_DOUBLE_PRECISION"
#endif

static int failed;
#define CHECK(cond)                                                            \
    do                                                                         \
    {                                                                          \
        if (!(cond))                                                           \
        {                                                                      \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            failed++;                                                          \
        }                                                                      \
    } while (0)

/* ---- the database: peaked profiles (node k strongly prefers Met = ATG or Trp = TGG, one codon each); profile 2 has
 * 300 nodes whose middle is crossed by deletes (MM/MI/MD 0.5/0.01/0.49 out of nodes 10 .. M-11, DM/DD 0.5/0.999 -- scores,
 * not a normalised row: leaving the run must be cheaper than leaving the core and entering it again):
 * a domain of it is its first and last ten codons with a 280-state delete run between them ------------------------- */
enum { NPROF = 6, BIG = 2, BIG_M = 300, SCAN_ID = 77 };
static unsigned const kSizes[NPROF] = {20, 33, BIG_M, 57, 60, 41};
static double *g_null[NPROF], *g_match[NPROF], *g_trans[NPROF];
static char g_domain[NPROF][3 * BIG_M + 1];
static char g_acc[NPROF][16];
static char g_db_path[64];

static void make_params(unsigned p)
{
    unsigned const M = kSizes[p];
    static char const amino[] = "ACDEFGHIKLMNPQRSTVWY";
    double *null = g_null[p] = malloc(sizeof(double) * 20), *match = g_match[p] = malloc(sizeof(double) * 20 * M),
           *trans = g_trans[p] = malloc(sizeof(double) * 7 * (M + 1));
    for (int a = 0; a < 20; ++a)
        null[a] = log(1.0 / 20);
    for (unsigned k = 0; k < M; ++k)
    {
        char const fav = ((k + p) % 3 == 0) ? 'W' : 'M';
        for (int a = 0; a < 20; ++a)
            match[20 * k + a] = log(amino[a] == fav ? 0.81 : 0.01);
        memcpy(g_domain[p] + 3 * k, fav == 'W' ? "TGG" : "ATG", 3);
    }
    g_domain[p][3 * M] = '\0';
    for (unsigned i = 0; i <= M; ++i)
    {
        double *t = trans + 7 * i; /* MM MI MD IM II DM DD */
        t[0] = log(0.95), t[1] = log(0.025), t[2] = log(0.025), t[3] = log(0.6), t[4] = log(0.4), t[5] = log(0.6), t[6] = log(0.4);
        if (p == BIG && i >= 10 && i < M - 10) t[0] = log(0.5), t[1] = log(0.01), t[2] = log(0.49);
        if (p == BIG && i >= 11 && i < M - 10) t[5] = log(0.5), t[6] = log(0.999);
        if (i == 0) t[6] = -INFINITY, t[5] = 0.0;
        if (i == M) t[2] = -INFINITY, t[6] = -INFINITY, t[0] = log(0.975), t[5] = 0.0;
    }
    snprintf(g_acc[p], sizeof g_acc[p], "PF%05u", p);
}

static void press_db(void)
{
    struct imm_nuclt const *nuclt = imm_super(&imm_dna_iupac);
    struct imm_nuclt_code code;
    imm_nuclt_code_init(&code, nuclt);
    snprintf(g_db_path, sizeof g_db_path, "/tmp/dcp_test_db64_XXXXXX");
    int fd = mkstemp(g_db_path);
    CHECK(fd >= 0);
    FILE *fp = fdopen(fd, "wb");
    CHECK(fp != NULL);
    struct protein_db_writer db = {0};
    CHECK(protein_db_writer_open(&db, fp, &imm_amino_iupac, nuclt, PROTEIN_CFG_DEFAULT) == RC_OK);
    for (unsigned p = 0; p < NPROF; ++p)
    {
        struct protein_profile prof;
        make_params(p);
        protein_profile_init(&prof, g_acc[p], &imm_amino_iupac, &code, PROTEIN_CFG_DEFAULT);
        CHECK(protein_profile_from_params(&prof, kSizes[p], g_null[p], g_match[p], g_trans[p]) == RC_OK);
        CHECK(dcp_profile_precision(prof.impl) == 64);
        CHECK(protein_db_writer_pack_profile(&db, &prof) == RC_OK);
        profile_del(&prof.super);
    }
    CHECK(db_writer_close((struct db_writer *)&db, true) == RC_OK);
    CHECK(fclose(fp) == 0);
}

/* ---- the queries ------------------------------------------------------------------------------------------------------ */
enum { NSEQ = 9, SEQ_ID0 = 100, GAPPED = 7, GAPPED_COPIES = 8 };
static char g_text[NSEQ][4096];
static struct scan_seq g_seqs[NSEQ];

static void make_queries(void)
{
    char const *flank[NSEQ] = {"ACGTTGCAAGGCTTAACC", "TTGACCA", "GGGCATCATCAGGAC", "A", "CCGTA", "GATTACAGATTACA", "TGCATGCAAT", "", "CAT"};
    char gapped_dom[3 * 20 + 1]; /* the first and the last ten codons of the 300-node profile */
    memcpy(gapped_dom, g_domain[BIG], 30);
    memcpy(gapped_dom + 30, g_domain[BIG] + 3 * (BIG_M - 10), 30);
    gapped_dom[60] = '\0';
    for (unsigned q = 0; q < NSEQ; ++q)
    {
        char *t = g_text[q];
        size_t const cap = sizeof g_text[q];
        if (q == GAPPED)
        {
            /* eight domains across the delete run, six bases between them: about 8 x 306 steps on 534 bases */
            size_t at = 0;
            for (unsigned c = 0; c < GAPPED_COPIES; ++c)
                at += (size_t)snprintf(t + at, cap - at, "%s%s", c % 2 ? "GATTAC" : "CCGTAA", gapped_dom);
            snprintf(t + at, cap - at, "ACGTTG");
        }
        else if (q == 2) snprintf(t, cap, "%s%s%s%s%s", flank[q], g_domain[0], "CCGTAGGCTTAACCGATTACA", g_domain[0], flank[5]); /* two domains */
        else if (q == 4) snprintf(t, cap, "%s%s%s", flank[q], g_domain[BIG], flank[0]); /* the whole 300-node domain */
        else
        {
            char const *dom = q == 0 ? g_domain[3] : q == 5 ? g_domain[1] : q == 6 ? g_domain[4] : q == 8 ? g_domain[5] : "";
            snprintf(t, cap, "%s%s%s", flank[q], dom, flank[(q + 3) % NSEQ]);
        }
        g_seqs[q] = (struct scan_seq){SEQ_ID0 + q, t};
    }
}

static char *slurp(FILE *fp)
{
    fflush(fp);
    fseek(fp, 0, SEEK_END);
    long len = ftell(fp);
    rewind(fp);
    char *text = calloc((size_t)len + 1, 1);
    CHECK(fread(text, 1, (size_t)len, fp) == (size_t)len);
    return text;
}

/* the rows of a products text (header skipped when present), sorted: one canonical text */
static int cmp_str(void const *a, void const *b) { return strcmp(*(char *const *)a, *(char *const *)b); }
static char *canonical(char *text)
{
    size_t const len = strlen(text);
    char *body = text;
    if (!strncmp(text, prod_header(), strlen(prod_header()))) body += strlen(prod_header());
    char **lines = calloc(len / 2 + 2, sizeof *lines);
    unsigned n = 0;
    for (char *l = strtok(body, "\n"); l; l = strtok(NULL, "\n"))
        lines[n++] = l;
    qsort(lines, n, sizeof *lines, cmp_str);
    char *out = calloc(len + 2, 1);
    size_t at = 0;
    for (unsigned i = 0; i < n; ++i)
        at += (size_t)sprintf(out + at, "%s\n", lines[i]);
    free(lines);
    free(text);
    return out;
}

static unsigned count_rows(char const *text)
{
    unsigned n = 0;
    for (; *text; ++text)
        n += *text == '\n';
    return n;
}

/* ---- the direct path: C-ABI only ---------------------------------------------------------------------------------------- */
static char const kAcgt[] = "ACGT";
static dcp_profile *g_direct[NPROF];
static struct dcp_hit64 *g_hits;
static unsigned g_nhits;

static char *rows_direct(double threshold)
{
    dcp_gpu_ctx *ctx = dcp_gpu_ctx_new(0);
    CHECK(ctx != NULL);
    if (!ctx) return calloc(1, 1);
    for (unsigned p = 0; p < NPROF; ++p)
        if (!g_direct[p])
        {
            int rc = 0;
            g_direct[p] = dcp_profile_new64(g_acc[p], kSizes[p], DCP_ENTRY_DIST_OCCUPANCY, (double)DEFAULT_EPSILON, g_null[p],
                                            g_match[p], g_trans[p], NULL, &rc);
            CHECK(g_direct[p] != NULL && rc == 0);
        }
    CHECK(dcp_gpu_db_upload64(ctx, g_direct, NPROF) == 0);
    static uint8_t ids[NSEQ * 4096];
    uint32_t off[NSEQ + 1] = {0};
    for (unsigned q = 0; q < NSEQ; ++q)
    {
        size_t const n = strlen(g_text[q]);
        for (size_t i = 0; i < n; ++i)
            ids[off[q] + i] = (uint8_t)(strchr(kAcgt, g_text[q][i]) - kAcgt);
        off[q + 1] = off[q] + (uint32_t)n;
    }
    CHECK(dcp_gpu_seqs_upload(ctx, ids, off, NSEQ) == 0);
    CHECK(dcp_gpu_set_lrt_threshold64(ctx, threshold) == 0);
    struct dcp_scan_params prm = {1, 0, 10.0f, 0, 0};
    CHECK(dcp_gpu_scan(ctx, &prm) == 0 && dcp_gpu_sync(ctx) == 0);
    unsigned nhits = 0;
    int rc = dcp_gpu_fetch_hits64(ctx, NULL, 0, &nhits);
    CHECK(rc == 0 || rc == DCP_ENOMEM);
    struct dcp_hit64 *hits = calloc(nhits ? nhits : 1, sizeof *hits);
    if (nhits) CHECK(dcp_gpu_fetch_hits64(ctx, hits, nhits, &nhits) == 0);
    uint32_t *soff = calloc((size_t)nhits + 1, sizeof *soff);
    unsigned cap = 0;
    for (unsigned h = 0; h < nhits; ++h)
        cap += 2 * (off[hits[h].seq_idx + 1] - off[hits[h].seq_idx]) + 2 * kSizes[hits[h].profile_idx] + 16;
    struct dcp_step *steps = calloc(cap ? cap : 1, sizeof *steps);
    double *alt = calloc(nhits ? nhits : 1, sizeof *alt);
    rc = dcp_gpu_trace_paths64(ctx, hits, nhits, 1, 0, 0, steps, cap, soff, alt);
    if (rc == DCP_ENOMEM && soff[nhits] > cap)
    {
        cap = soff[nhits];
        steps = realloc(steps, (size_t)cap * sizeof *steps);
        rc = dcp_gpu_trace_paths64(ctx, hits, nhits, 1, 0, 0, steps, cap, soff, alt);
    }
    CHECK(rc == 0);
    size_t text_cap = 1 << 16, at = 0;
    char *text = calloc(text_cap, 1);
    for (unsigned h = 0; h < nhits && !rc; ++h)
    {
        unsigned const q = hits[h].seq_idx, p = hits[h].profile_idx, ns = soff[h + 1] - soff[h];
        CHECK(!memcmp(&alt[h], &hits[h].alt_loglik, 8)); /* the trace recomputes the scan's score bit for bit */
        size_t const need = 512 + 64 * ((size_t)ns + 1) + 2 * (off[q + 1] - off[q]);
        if (at + need > text_cap) text = realloc(text, text_cap = 2 * (at + need));
        long const n = dcp_prod_format_row(text + at, text_cap - at, SCAN_ID, SEQ_ID0 + q, g_acc[p], "dna", hits[h].alt_loglik,
                                           hits[h].null_loglik, "protein", DECIPHON_VERSION, g_direct[p], ids + off[q],
                                           off[q + 1] - off[q], steps + soff[h], ns);
        CHECK(n > 0);
        if (n > 0) at += (size_t)n;
        text[at] = '\0';
        if (q == GAPPED && p == BIG) CHECK(ns > 2 * (off[q + 1] - off[q]) + 2 * BIG_M + 16); /* past the first estimate */
    }
    free(g_hits);
    g_hits = hits, g_nhits = nhits;
    free(soff), free(steps), free(alt);
    dcp_gpu_ctx_del(ctx);
    return canonical(text);
}

/* ---- the host layer's three ways --------------------------------------------------------------------------------------- */
static char *rows_thread_run(unsigned npart, double threshold, bool batched)
{
    FILE *fp = fopen(g_db_path, "rb");
    CHECK(fp != NULL);
    struct protein_db_reader db = {0};
    CHECK(protein_db_reader_open(&db, fp) == RC_OK);
    CHECK(db.super.nprofiles == NPROF && db.cfg.epsilon == DEFAULT_EPSILON && sizeof db.cfg.epsilon == 8);
    static struct profile_reader reader;
    CHECK(profile_reader_setup(&reader, (struct db_reader *)&db, npart) == RC_OK);
    struct scan_thread th[4];
    CHECK(npart <= 4 && prod_fopen(npart) == RC_OK);
    for (unsigned i = 0; i < npart; ++i)
    {
        thread_init(&th[i], i, &reader, true, false, threshold, protein_match_write_func);
        thread_setup_job(&th[i], IMM_DNA, PROFILE_PROTEIN, SCAN_ID);
    }
    struct imm_seq seqs[NSEQ];
    int64_t ids[NSEQ];
    for (unsigned q = 0; q < NSEQ; ++q)
    {
        seqs[q] = imm_seq(imm_str(g_text[q]), imm_super(&db.nuclt));
        ids[q] = g_seqs[q].id;
    }
    if (batched)
        for (unsigned i = 0; i < npart; ++i)
            CHECK(thread_run_batch(&th[i], (int)i, seqs, ids, NSEQ) == RC_OK);
    else
        for (unsigned q = 0; q < NSEQ; ++q)
            for (unsigned i = 0; i < npart; ++i)
            {
                thread_setup_seq(&th[i], &seqs[q], ids[q]);
                CHECK(thread_run(&th[i], (int)i) == RC_OK);
            }
    CHECK(prod_fclose() == RC_OK);
    char *text = slurp(prod_final_fp());
    CHECK(!strncmp(text, prod_header(), strlen(prod_header())));
    prod_final_cleanup();
    for (unsigned i = 0; i < npart; ++i)
        thread_cleanup(&th[i]);
    profile_reader_del(&reader);
    db_reader_close((struct db_reader *)&db);
    fclose(fp);
    return canonical(text);
}

struct list_src
{
    struct scan_seq const *seqs;
    unsigned n, at;
};
static enum rc list_src_next(void *arg, struct scan_seq *seq)
{
    struct list_src *l = arg;
    if (l->at == l->n) return RC_END;
    *seq = l->seqs[l->at++];
    return RC_OK;
}
static char *rows_scan_run_source(unsigned nthreads, unsigned batch, unsigned long symbols, double threshold)
{
    struct list_src src = {g_seqs, NSEQ, 0};
    struct scan_cfg cfg = {.scan_id = SCAN_ID, .multi_hits = true, .hmmer3_compat = false, .lrt_threshold = threshold,
                           .batch = batch, .balance_by_cells = nthreads > 1, .batch_symbols = symbols};
    CHECK(scan_run_source(g_db_path, cfg, nthreads, list_src_next, &src) == RC_OK);
    char *text = slurp(prod_final_fp());
    prod_final_cleanup();
    return canonical(text);
}

static bool has_row(char const *rows, unsigned q, unsigned p)
{
    char key[64];
    snprintf(key, sizeof key, "%d\t%d\t%s\tdna\t", SCAN_ID, SEQ_ID0 + (int)q, g_acc[p]);
    return strstr(rows, key) != NULL;
}

/* `got` (freed here) must be `want`, byte for byte */
static void same_rows_at(char *got, char const *want, int line)
{
    if (strcmp(got, want))
    {
        fprintf(stderr, "%s:%d: product rows differ (%u rows, want %u)\n", __FILE__, line, count_rows(got), count_rows(want));
        failed++;
    }
    free(got);
}
#define SAME_ROWS(got, want) same_rows_at((got), (want), __LINE__)

static void product_rows(void)
{
    char *direct = rows_direct(10.0);
    unsigned const nrows = count_rows(direct);
    CHECK(nrows >= 7 && nrows == g_nhits);
    /* the planted domains are hits of their profiles -- the 300-node one twice, once with eight domains */
    CHECK(has_row(direct, 0, 3) && has_row(direct, 2, 0) && has_row(direct, 4, BIG) && has_row(direct, 5, 1) &&
          has_row(direct, 6, 4) && has_row(direct, GAPPED, BIG) && has_row(direct, 8, 5));
    CHECK(!has_row(direct, 1, 0) && !has_row(direct, 3, 0));
    /* logliks are written as the doubles they are: %.17g of values that are not float values */
    for (unsigned h = 0; h < g_nhits; ++h)
    {
        char want[96];
        snprintf(want, sizeof want, "\t%.17g\t%.17g\tprotein\t", g_hits[h].alt_loglik, g_hits[h].null_loglik);
        CHECK(strstr(direct, want) != NULL);
        CHECK((double)(float)g_hits[h].alt_loglik != g_hits[h].alt_loglik);
    }
    SAME_ROWS(rows_thread_run(2, 10.0, false), direct);
    SAME_ROWS(rows_thread_run(1, 10.0, false), direct);
    SAME_ROWS(rows_thread_run(2, 10.0, true), direct);
    SAME_ROWS(rows_thread_run(1, 10.0, true), direct);
    unsigned const batches[] = {1, 2, 3, 100};
    for (unsigned nthreads = 1; nthreads <= 2; ++nthreads)
        for (unsigned b = 0; b < 4; ++b)
        {
            SAME_ROWS(rows_scan_run_source(nthreads, batches[b], 0, 10.0), direct);
        }
    SAME_ROWS(rows_scan_run_source(2, 100, 200, 10.0), direct); /* passes sized by symbols */
    struct scan_stats st;
    scan_last_stats(&st);
    CHECK(st.passes >= 2 && st.hits == nrows);

    /* the threshold in double: the LRT x of one hit keeps its row, the next double above x drops it -- and only it.
     * x is not a float value, so a threshold rounded to float could not sit between the two. */
    unsigned pick = 0;
    for (unsigned h = 0; h < g_nhits; ++h)
        if (g_hits[h].seq_idx == 2) pick = h;
    unsigned const pq = g_hits[pick].seq_idx, pp = g_hits[pick].profile_idx;
    double const x = xmath_lrt(g_hits[pick].null_loglik, g_hits[pick].alt_loglik);
    CHECK(x > 10.0 && (double)(float)x != x);
    char *at_x = rows_direct(x), *above = rows_direct(nextafter(x, INFINITY));
    CHECK(has_row(at_x, pq, pp) && !has_row(above, pq, pp) && count_rows(at_x) == count_rows(above) + 1);
    for (unsigned nthreads = 1; nthreads <= 2; ++nthreads)
    {
        SAME_ROWS(rows_scan_run_source(nthreads, 3, 0, x), at_x);
        SAME_ROWS(rows_scan_run_source(nthreads, 3, 0, nextafter(x, INFINITY)), above);
    }
    SAME_ROWS(rows_thread_run(2, x, false), at_x);
    SAME_ROWS(rows_thread_run(2, nextafter(x, INFINITY), true), above);
    free(at_x), free(above), free(direct);
}

/* ---- imm_dp_viterbi with the transitions the profile holds NOW ---------------------------------------------------------- */
static void put_bits(FILE *out, double v)
{
    uint64_t b;
    memcpy(&b, &v, 8);
    fprintf(out, " %016" PRIx64, b);
}

static void viterbi_cases(FILE *out)
{
    struct imm_nuclt_code code;
    imm_nuclt_code_init(&code, imm_super(&imm_dna_iupac));
    struct
    {
        unsigned seed, M;
        enum entry_dist entry;
        double epsilon; /* the goldens' profiles are test/protein_profile.c's: protein_cfg(..., 0.1f), a float literal */
        char const *seq;
    } const cases[] = {{1, 2, ENTRY_DIST_UNIFORM, 0.1f, "ATGAAACGCATTAGCACCACCATTACCACCAC"},
                       {1, 2, ENTRY_DIST_OCCUPANCY, 0.1f, "ATGAAACGCATTAGCACCACCATTACCACCAC"},
                       {11, 65, ENTRY_DIST_OCCUPANCY, 0.1, "GATTACAGATTACACCGTAGGCTTAACCGATTACATGCATGCAATACGTTGCAAGGCTTAACC"},
                       {12, 300, ENTRY_DIST_UNIFORM, 0.01, "ACGTTGCAAGGCTTAACCGGTTACGATCGATTAGCATGAAACGCATTAGCACCACCATTACCACCACTTGACCAGG"}};
    for (unsigned c = 0; c < sizeof cases / sizeof cases[0]; ++c)
    {
        struct protein_profile prof;
        protein_profile_init(&prof, "accession", &imm_amino_iupac, &code, protein_cfg(cases[c].entry, cases[c].epsilon));
        CHECK(protein_profile_sample(&prof, cases[c].seed, cases[c].M) == RC_OK);
        struct imm_seq seq = imm_seq(imm_str(cases[c].seq), prof.super.code->abc);
        struct imm_prod prod = imm_prod();
        struct imm_task *tn = imm_task_new(&prof.null.dp), *ta = imm_task_new(&prof.alt.dp);
        CHECK(tn && ta && imm_task_setup(tn, &seq) == IMM_OK && imm_task_setup(ta, &seq) == IMM_OK);
        /* round 0: protein_profile_setup's transitions; round 1: four of them changed by hand, to doubles no flags give
         * (E -> B and E -> J finite and different, N -> N and R -> R off their length-derived values) */
        for (int round = 0; round < 2; ++round)
        {
            CHECK(protein_profile_setup(&prof, imm_seq_size(&seq), round == 0, false) == RC_OK);
            if (round)
            {
                struct imm_dp *dp = &prof.alt.dp;
                imm_dp_change_trans(dp, imm_dp_trans_idx(dp, prof.alt.E, prof.alt.B), -0.3 - 0.01 * c);
                imm_dp_change_trans(dp, imm_dp_trans_idx(dp, prof.alt.E, prof.alt.J), -1.7);
                imm_dp_change_trans(dp, imm_dp_trans_idx(dp, prof.alt.N, prof.alt.N), -0.011);
                imm_dp_change_trans(&prof.null.dp, imm_dp_trans_idx(&prof.null.dp, prof.null.R, prof.null.R), -0.0123);
            }
            CHECK(imm_dp_viterbi(&prof.null.dp, tn, &prod) == IMM_OK); /* IMM_OK: the traced loglik equals the scan's bitwise */
            double const nul = prod.loglik;
            CHECK(imm_path_nsteps(&prod.path) > 0 && imm_path_step(&prod.path, 0)->state_id == PROTEIN_R_STATE);
            CHECK(imm_dp_viterbi(&prof.alt.dp, ta, &prod) == IMM_OK);
            double const alt = prod.loglik;
            CHECK(isfinite(nul) && isfinite(alt) && sizeof prod.loglik == 8);
            unsigned covered = 0;
            for (unsigned i = 0; i < imm_path_nsteps(&prod.path); ++i)
                covered += imm_path_step(&prod.path, i)->seqlen;
            CHECK(covered == imm_seq_size(&seq) && imm_path_step(&prod.path, 0)->state_id == PROTEIN_S_STATE);
            if (c < 2 && round == 0)
            {
                /* the reference's goldens (test/protein_profile.c), to the digits they are written with */
                double const want = cases[c].entry == ENTRY_DIST_UNIFORM ? -55.59428153448 : -54.35543421312;
                CHECK(fabs(nul - -48.9272687711) < 1e-10 && fabs(alt - want) < 1e-10);
            }
            if (out)
            {
                fprintf(out, "%u %u %d %s", cases[c].seed, cases[c].M, (int)cases[c].entry, cases[c].seq);
                put_bits(out, cases[c].epsilon);
                for (int i = 0; i < DCP_NXTRANS; ++i)
                    put_bits(out, prof.xtrans[i]);
                put_bits(out, nul);
                put_bits(out, alt);
                fputc('\n', out);
            }
        }
        imm_del(&prod);
        imm_del(tn);
        imm_del(ta);
        profile_del(&prof.super);
    }
}

int main(int argc, char **argv)
{
    if (argc == 3 && !strcmp(argv[1], "viterbi"))
    {
        FILE *out = fopen(argv[2], "w");
        if (!out) return 2;
        viterbi_cases(out);
        fclose(out);
        if (!failed) puts("test_scan_host_f64 viterbi: all checks passed");
        return failed;
    }
    press_db();
    make_queries();
    product_rows();
    viterbi_cases(NULL);
    for (unsigned p = 0; p < NPROF; ++p)
    {
        dcp_profile_del(g_direct[p]);
        free(g_null[p]), free(g_match[p]), free(g_trans[p]);
    }
    free(g_hits);
    remove(g_db_path);
    if (failed) fprintf(stderr, "%d check(s) failed\n", failed);
    else puts("test_scan_host_f64: all checks passed");
    return failed;
}
