/*
 * GPU test of scan_cfg.minus_strand_id (include/deciphon_host.h): scan_run_source on both strands.  Builds in float
 * against libdeciphon_host.so and with -DIMM_DOUBLE_PRECISION against libdeciphon_host_f64.so.
 *
 * Job A has minus_strand_id set (id -> -id - 1) and a source of n sequences.  Job B has the field NULL and a source
 * that yields each of those sequences followed by its host-made reverse complement under that id -- the only way to
 * get both strands without the switch.  Their product files must be byte-identical, header included, for passes of
 * 1, 3 and 100 sequences, for passes cut at 200 bases, and for 1 and 2 partitions.  Some sequences carry a planted
 * domain forward, some carry its reverse complement: rows under minus-strand ids must be among the products.
 * `progress` of job A sums to profiles x source sequences; with the field NULL job A's source gives exactly the
 * plus-strand rows.
 * Exit status = number of failed checks.
 */
#include "deciphon_host.h"
#include <inttypes.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

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

/* ---- the database: peaked profiles, node k strongly prefers Met = ATG or Trp = TGG (one codon each) ------------ */
enum { NPROF = 4, SCAN_ID = 77, DOM_MAX = 3 * 60 };
static unsigned const kSizes[NPROF] = {20, 33, 57, 41};
static char g_domain[NPROF][DOM_MAX + 1];
static char g_acc[NPROF][16];
static char g_db_path[64];

static void press_db(void)
{
    static char const amino[] = "ACDEFGHIKLMNPQRSTVWY";
    struct imm_nuclt const *nuclt = imm_super(&imm_dna_iupac);
    struct imm_nuclt_code code;
    imm_nuclt_code_init(&code, nuclt);
    snprintf(g_db_path, sizeof g_db_path, "/tmp/dcp_test_strands_XXXXXX");
    int fd = mkstemp(g_db_path);
    CHECK(fd >= 0);
    FILE *fp = fdopen(fd, "wb");
    CHECK(fp != NULL);
    struct protein_db_writer db = {0};
    CHECK(protein_db_writer_open(&db, fp, &imm_amino_iupac, nuclt, PROTEIN_CFG_DEFAULT) == RC_OK);
    for (unsigned p = 0; p < NPROF; ++p)
    {
        unsigned const M = kSizes[p];
        imm_float null[20], *match = malloc(sizeof(imm_float) * 20 * M), *trans = malloc(sizeof(imm_float) * 7 * (M + 1));
        for (int a = 0; a < 20; ++a)
            null[a] = (imm_float)log(1.0 / 20);
        for (unsigned k = 0; k < M; ++k)
        {
            char const fav = ((k + p) % 3 == 0) ? 'W' : 'M';
            for (int a = 0; a < 20; ++a)
                match[20 * k + a] = (imm_float)log(amino[a] == fav ? 0.81 : 0.01);
            memcpy(g_domain[p] + 3 * k, fav == 'W' ? "TGG" : "ATG", 3);
        }
        g_domain[p][3 * M] = '\0';
        for (unsigned i = 0; i <= M; ++i)
        {
            imm_float *t = trans + 7 * i; /* MM MI MD IM II DM DD */
            t[0] = (imm_float)log(0.95), t[1] = (imm_float)log(0.025), t[2] = (imm_float)log(0.025);
            t[3] = (imm_float)log(0.6), t[4] = (imm_float)log(0.4), t[5] = (imm_float)log(0.6), t[6] = (imm_float)log(0.4);
            if (i == 0) t[6] = -INFINITY, t[5] = 0;
            if (i == M) t[2] = -INFINITY, t[6] = -INFINITY, t[0] = (imm_float)log(0.975), t[5] = 0;
        }
        snprintf(g_acc[p], sizeof g_acc[p], "PF%05u", p);
        struct protein_profile prof;
        protein_profile_init(&prof, g_acc[p], &imm_amino_iupac, &code, PROTEIN_CFG_DEFAULT);
        CHECK(protein_profile_from_params(&prof, M, null, match, trans) == RC_OK);
        CHECK(dcp_profile_precision(prof.impl) == 8 * IMM_FLOAT_BYTES);
        CHECK(protein_db_writer_pack_profile(&db, &prof) == RC_OK);
        profile_del(&prof.super);
        free(match), free(trans);
    }
    CHECK(db_writer_close((struct db_writer *)&db, true) == RC_OK);
    CHECK(fclose(fp) == 0);
}

/* ---- the sequences --------------------------------------------------------------------------------------------- */
enum { NSEQ = 9, SEQ_ID0 = 100 };
static char g_text[NSEQ][512], g_rev[NSEQ][512];
static struct scan_seq g_single[NSEQ], g_doubled[2 * NSEQ];

static int64_t minus_id(int64_t id, void *arg)
{
    unsigned *calls = arg; /* the rows of a pass are formatted by several host threads */
#pragma omp atomic
    ++*calls;
    return -id - 1;
}

/* the reverse complement as text, through the library's own host map on symbol ids */
static void revcomp_text(char const *text, char *out)
{
    static char const acgt[] = "ACGT";
    uint8_t ids[512] = {0}, rev[512] = {0};
    unsigned const n = (unsigned)strlen(text);
    for (unsigned i = 0; i < n; ++i)
        ids[i] = (uint8_t)(strchr(acgt, text[i]) - acgt);
    dcp_seq_revcomp(ids, n, rev);
    for (unsigned i = 0; i < n; ++i)
        out[i] = acgt[rev[i]];
    out[n] = '\0';
}

/* sequences 1, 4 and 7 carry the REVERSE COMPLEMENT of a domain (profiles 1, 2, 3): hits of the minus strand only;
 * 0, 2 and 6 carry a domain forward (profiles 3, 0 twice, 2); 3, 5 and 8 carry none (1, 5 and 16 nt) */
static int const kMinusOf[NSEQ] = {-1, 1, -1, -1, 2, -1, -1, 3, -1};
static int const kPlusOf[NSEQ] = {3, -1, 0, -1, -1, -1, 2, -1, -1};

static void make_sequences(void)
{
    char const *flank[NSEQ] = {"ACGTTGCAAGGCTTAACC", "TTGACCA", "GGGCATCATCAGGAC", "A", "CCGTA", "GATTA", "TGCATGCAAT", "C", "CATTACAGGATCCAAG"};
    char rdom[DOM_MAX + 1];
    for (unsigned q = 0; q < NSEQ; ++q)
    {
        char *t = g_text[q];
        size_t const cap = sizeof g_text[q];
        if (kMinusOf[q] >= 0)
        {
            revcomp_text(g_domain[kMinusOf[q]], rdom);
            snprintf(t, cap, "%s%s%s", flank[q], rdom, flank[(q + 2) % NSEQ]);
        }
        else if (q == 2) snprintf(t, cap, "%s%s%s%s%s", flank[q], g_domain[0], "CCGTAGGCTTAACCGATTACA", g_domain[0], flank[5]);
        else if (kPlusOf[q] >= 0) snprintf(t, cap, "%s%s%s", flank[q], g_domain[kPlusOf[q]], flank[(q + 3) % NSEQ]);
        else snprintf(t, cap, "%s", flank[q]);
        revcomp_text(t, g_rev[q]);
        g_single[q] = (struct scan_seq){SEQ_ID0 + q, t};
        g_doubled[2 * q] = g_single[q];
        g_doubled[2 * q + 1] = (struct scan_seq){-(int64_t)(SEQ_ID0 + q) - 1, g_rev[q]};
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

static unsigned long g_pairs;
static void count_pairs(unsigned long pairs, void *arg)
{
    (void)arg;
#pragma omp atomic
    g_pairs += pairs;
}

/* the whole products file of one job; strands: 0 the plain source, 1 the plain source with minus_strand_id set, 2 the
 * hand-doubled source */
static char *job(int strands, unsigned nthreads, unsigned batch, unsigned long symbols, unsigned *id_calls)
{
    struct list_src src = {strands == 2 ? g_doubled : g_single, strands == 2 ? 2 * NSEQ : NSEQ, 0};
    unsigned calls = 0;
    struct scan_cfg cfg = {.scan_id = SCAN_ID, .multi_hits = true, .hmmer3_compat = false, .lrt_threshold = 10.0,
                           .batch = batch, .balance_by_cells = nthreads > 1, .keep_resident = true, .progress = count_pairs,
                           .batch_symbols = symbols};
    if (strands == 1) cfg.minus_strand_id = minus_id, cfg.minus_strand_arg = &calls;
    g_pairs = 0;
    CHECK(scan_run_source(g_db_path, cfg, nthreads, list_src_next, &src) == RC_OK);
    CHECK(src.at == src.n);
    char *text = slurp(prod_final_fp());
    prod_final_cleanup();
    if (id_calls) *id_calls = calls;
    return text;
}

static bool has_row(char const *rows, long long seq_id, unsigned p)
{
    char key[64];
    snprintf(key, sizeof key, "\n%d\t%lld\t%s\tdna\t", SCAN_ID, seq_id, g_acc[p]);
    return strstr(rows, key) != NULL;
}

static unsigned count_rows(char const *text)
{
    unsigned n = 0;
    for (; *text; ++text)
        n += *text == '\n';
    return n;
}

int main(void)
{
    press_db();
    make_sequences();
    static struct
    {
        unsigned nthreads, batch;
        unsigned long symbols;
    } const cases[] = {{1, 1, 0}, {1, 3, 0}, {1, 100, 0}, {1, 100, 200}, {2, 3, 0}, {2, 100, 0}, {2, 100, 200}};
    char *first = NULL;
    for (unsigned c = 0; c < sizeof cases / sizeof cases[0]; ++c)
    {
        unsigned calls = 0;
        char *both = job(1, cases[c].nthreads, cases[c].batch, cases[c].symbols, &calls);
        /* progress counts (profile, SOURCE sequence) pairs, not doubled */
        CHECK(g_pairs == (unsigned long)NPROF * NSEQ);
        struct scan_stats st;
        scan_last_stats(&st);
        char *doubled = job(2, cases[c].nthreads, cases[c].batch, cases[c].symbols, NULL);
        CHECK(g_pairs == 2ul * NPROF * NSEQ);
        if (strcmp(both, doubled))
        {
            fprintf(stderr, "case %u (%u partitions, batch %u, %lu symbols): products differ\n--- minus_strand_id\n%s--- doubled source\n%s",
                    c, cases[c].nthreads, cases[c].batch, cases[c].symbols, both, doubled);
            failed++;
        }
        CHECK(!strncmp(both, prod_header(), strlen(prod_header())));
        /* hits / steps of the stats count both strands: one hit per row */
        CHECK(st.hits == count_rows(both) - 1u && st.steps > st.hits);
        /* the id callback ran once per minus-strand row at least (and once more per partition's last row) */
        CHECK(calls >= 3);
        if (cases[c].nthreads == 1)
        {
            /* one partition: the file is in source order -- the same bytes whatever the pass size */
            if (first) CHECK(!strcmp(first, both));
            else first = strdup(both);
        }
        /* the planted domains: forward ones under the source's id, reversed ones under the minus-strand id only */
        for (unsigned q = 0; q < NSEQ; ++q)
        {
            long long const id = SEQ_ID0 + (long long)q;
            if (kPlusOf[q] >= 0) CHECK(has_row(both, id, (unsigned)kPlusOf[q]) && !has_row(both, -id - 1, (unsigned)kPlusOf[q]));
            if (kMinusOf[q] >= 0) CHECK(has_row(both, -id - 1, (unsigned)kMinusOf[q]) && !has_row(both, id, (unsigned)kMinusOf[q]));
        }
        free(both), free(doubled);
    }
    /* row order within a job: per source sequence the plus-strand rows, then the minus-strand rows (one partition) */
    if (first)
    {
        long long last_src = -1;
        int last_minus = 0;
        for (char const *l = strchr(first, '\n'); l && l[1]; l = strchr(l + 1, '\n'))
        {
            long long scan = 0, id = 0;
            CHECK(sscanf(l + 1, "%lld\t%lld\t", &scan, &id) == 2 && scan == SCAN_ID);
            long long const srcid = id < 0 ? -id - 1 : id;
            CHECK(srcid > last_src || (srcid == last_src && (id < 0) >= last_minus));
            last_src = srcid, last_minus = id < 0;
        }
    }
    /* the field NULL: exactly the plus-strand rows, as before */
    {
        char *plain = job(0, 1, 3, 0, NULL);
        CHECK(g_pairs == (unsigned long)NPROF * NSEQ);
        size_t at = 0;
        char *plus = calloc(first ? strlen(first) + 1 : 1, 1);
        for (char const *l = first; l && *l;)
        {
            char const *e = strchr(l, '\n');
            size_t const n = e ? (size_t)(e - l) + 1 : strlen(l);
            long long scan = 0, id = 0;
            bool const row = l != first; /* the header line stays */
            if (!row || (sscanf(l, "%lld\t%lld\t", &scan, &id) == 2 && id >= 0)) memcpy(plus + at, l, n), at += n;
            l += n;
        }
        CHECK(first && !strcmp(plain, plus));
        CHECK(strstr(plain, "\n77\t-") == NULL); /* no row under a minus-strand id */
        free(plain), free(plus);
    }
    free(first);
    scan_resident_release();
    unlink(g_db_path);
    if (failed) fprintf(stderr, "%d checks failed\n", failed);
    else printf("all checks passed\n");
    return failed;
}
