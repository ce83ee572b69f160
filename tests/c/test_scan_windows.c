/*
 * GPU test of scan_cfg.window / window_step / window_id (include/deciphon_host.h): scan_run_source over windows cut on
 * the device.  Builds in float against libdeciphon_host.so and with -DIMM_DOUBLE_PRECISION against
 * libdeciphon_host_f64.so.
 *
 * Job A has the three members set (window 200, step 100, id -> 4096 id + offset) and a source of n sequences of 1 to
 * 1 531 bases.  Job B has them zero and a source that yields every window of those sequences -- cut on the host by the
 * exported rule -- as a sequence of its own under that id.  Their product files must be byte-identical, header
 * included, for passes of 1, 3 and 100 sequences, for passes cut at 500 bases, for 1 and 2 partitions; then the same
 * with minus_strand_id set in both jobs, and with device_decode set in both.  Planted domains (forward and reverse
 * complement) must come back under the ids of the windows that wholly contain them.  window without window_id, or
 * with a step above it, is RC_EINVAL; window_step 0 is window / 2; a job with the members zero writes what a job with
 * one window per sequence under its own id writes.
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
    snprintf(g_db_path, sizeof g_db_path, "/tmp/dcp_test_windows_XXXXXX");
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
enum { NSEQ = 8, SEQ_ID0 = 100, WINDOW = 200, STEP = 100, LMAX = 1531, WMAX = 128 };
/* lengths around the window (one window at 200 and below, two from 201), a long one whose last window is anchored at
 * an odd offset (1531 - 200), and 1- and 5-base ones */
static unsigned const kLen[NSEQ] = {1531, 1, 200, 201, 5, 700, 199, 1000};
/* plants (sequence, offset, profile, reverse complement?): each lies wholly inside at least one window.  Profiles 0
 * and 3 favour the same residues (a copy of one hits the other): no window holds copies of them on opposite strands */
static struct
{
    unsigned seq, at, prof;
    bool minus;
} const kPlants[] = {{0, 110, 0, false}, {0, 620, 2, true},  {0, 1345, 3, false}, {2, 10, 1, false},
                     {3, 20, 2, false},  {5, 305, 3, true},  {5, 640, 0, false},  {7, 400, 1, true},
                     {7, 805, 2, false}, {6, 30, 0, true}};
enum { NPLANTS = sizeof kPlants / sizeof kPlants[0] };
static char g_text[NSEQ][LMAX + 1];
static char g_win[WMAX][WINDOW + 1];
static struct scan_seq g_whole[NSEQ], g_cut[WMAX];
static unsigned g_ncut;

static int64_t window_id(int64_t id, unsigned off, void *arg)
{
    unsigned *calls = arg; /* may run on several host threads */
    if (calls)
    {
#pragma omp atomic
        ++*calls;
    }
    return id * 4096 + off;
}
static int64_t own_id(int64_t id, unsigned off, void *arg)
{
    (void)arg;
    return off == 0 ? id : -1;
}
static int64_t minus_id(int64_t id, void *arg)
{
    (void)arg;
    return -id - 1;
}

static void revcomp_text(char const *text, char *out)
{
    static char const acgt[] = "ACGT";
    uint8_t ids[DOM_MAX] = {0}, rev[DOM_MAX] = {0};
    unsigned const n = (unsigned)strlen(text);
    for (unsigned i = 0; i < n; ++i)
        ids[i] = (uint8_t)(strchr(acgt, text[i]) - acgt);
    dcp_seq_revcomp(ids, n, rev);
    for (unsigned i = 0; i < n; ++i)
        out[i] = acgt[rev[i]];
    out[n] = '\0';
}

static void make_sequences(void)
{
    uint32_t lcg = 20261019u;
    for (unsigned q = 0; q < NSEQ; ++q)
    {
        for (unsigned i = 0; i < kLen[q]; ++i)
        {
            lcg = lcg * 1664525u + 1013904223u;
            g_text[q][i] = "ACGT"[lcg >> 30];
        }
        g_text[q][kLen[q]] = '\0';
        g_whole[q] = (struct scan_seq){SEQ_ID0 + q, g_text[q]};
    }
    for (unsigned k = 0; k < NPLANTS; ++k)
    {
        char dom[DOM_MAX + 1];
        if (kPlants[k].minus) revcomp_text(g_domain[kPlants[k].prof], dom);
        else strcpy(dom, g_domain[kPlants[k].prof]);
        CHECK(kPlants[k].at + strlen(dom) <= kLen[kPlants[k].seq]);
        memcpy(g_text[kPlants[k].seq] + kPlants[k].at, dom, strlen(dom));
    }
    /* the windows, cut on the host by the exported rule: what job B's source yields */
    uint64_t nwin = 0, nwords = 0;
    CHECK(dcp_seq_window_plan(kLen, NSEQ, WINDOW, STEP, &nwin, &nwords) == 0 && nwin <= WMAX);
    for (unsigned q = 0; q < NSEQ; ++q)
    {
        unsigned const cnt = dcp_seq_window_count(kLen[q], WINDOW, STEP), wl = kLen[q] < WINDOW ? kLen[q] : WINDOW;
        for (unsigned i = 0; i < cnt && g_ncut < WMAX; ++i, ++g_ncut)
        {
            unsigned const off = dcp_seq_window_start(kLen[q], WINDOW, STEP, i);
            memcpy(g_win[g_ncut], g_text[q] + off, wl);
            g_win[g_ncut][wl] = '\0';
            g_cut[g_ncut] = (struct scan_seq){window_id(SEQ_ID0 + q, off, NULL), g_win[g_ncut]};
        }
    }
    CHECK(g_ncut == nwin && g_ncut > NSEQ);
    CHECK(dcp_seq_window_start(1531, WINDOW, STEP, dcp_seq_window_count(1531, WINDOW, STEP) - 1) == 1331);
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

struct job
{
    int cut;              /* 0: whole sequences, members zero; 1: whole sequences, window members set; 2: the hand-cut source */
    unsigned window, step; /* for cut == 1 */
    int64_t (*id)(int64_t, unsigned, void *);
    bool minus, decode;
    unsigned nthreads, batch;
    unsigned long symbols;
};

static char *run_job(struct job j, unsigned *id_calls, enum rc want)
{
    struct list_src src = {j.cut == 2 ? g_cut : g_whole, j.cut == 2 ? g_ncut : NSEQ, 0};
    unsigned calls = 0;
    struct scan_cfg cfg = {.scan_id = SCAN_ID, .multi_hits = true, .hmmer3_compat = false, .lrt_threshold = 10.0,
                           .batch = j.batch, .balance_by_cells = j.nthreads > 1, .keep_resident = true, .progress = count_pairs,
                           .batch_symbols = j.symbols, .device_decode = j.decode};
    if (j.minus) cfg.minus_strand_id = minus_id;
    if (j.cut == 1) cfg.window = j.window, cfg.window_step = j.step, cfg.window_id = j.id, cfg.window_arg = &calls;
    g_pairs = 0;
    enum rc const rc = scan_run_source(g_db_path, cfg, j.nthreads, list_src_next, &src);
    CHECK(rc == want);
    if (rc) return NULL;
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
    } const cases[] = {{1, 1, 0}, {1, 3, 0}, {1, 100, 0}, {1, 100, 500}, {2, 3, 0}, {2, 100, 500}};
    for (int mode = 0; mode < 3; ++mode) /* windows alone; with the minus strand; with the device decode as well */
    {
        bool const minus = mode >= 1, decode = mode >= 2;
        char *first = NULL;
        for (unsigned c = 0; c < sizeof cases / sizeof cases[0]; ++c)
        {
            if (mode == 2 && c != 1 && c != 5) continue; /* the decode does not depend on how passes are cut: two cases */
            unsigned calls = 0;
            struct job a = {1, WINDOW, STEP, window_id, minus, decode, cases[c].nthreads, cases[c].batch, cases[c].symbols};
            struct job b = {2, 0, 0, NULL, minus, decode, cases[c].nthreads, cases[c].batch, cases[c].symbols};
            char *cut = run_job(a, &calls, RC_OK);
            /* progress counts (profile, SOURCE sequence) pairs */
            CHECK(g_pairs == (unsigned long)NPROF * NSEQ);
            struct scan_stats st;
            scan_last_stats(&st);
            char *hand = run_job(b, NULL, RC_OK);
            CHECK(g_pairs == (unsigned long)NPROF * g_ncut);
            if (!cut || !hand || strcmp(cut, hand))
            {
                fprintf(stderr, "mode %d case %u (%u partitions, batch %u, %lu symbols): products differ\n--- windows on the device\n%s--- hand-cut source\n%s",
                        mode, c, cases[c].nthreads, cases[c].batch, cases[c].symbols, cut ? cut : "(none)\n", hand ? hand : "(none)\n");
                failed++;
                free(cut), free(hand);
                continue;
            }
            CHECK(!strncmp(cut, prod_header(), strlen(prod_header())));
            CHECK(st.hits == count_rows(cut) - 1u && st.steps > st.hits);
            /* window_id ran once per window, when its pass was cut from the source (not per partition) */
            CHECK(calls == g_ncut);
            if (cases[c].nthreads == 1)
            {
                /* one partition: the file is in source order -- the same bytes whatever the pass size */
                if (first) CHECK(!strcmp(first, cut));
                else first = strdup(cut);
            }
            /* every plant comes back under the id of every window that wholly contains it -- on its strand only */
            for (unsigned k = 0; k < NPLANTS; ++k)
            {
                unsigned const q = kPlants[k].seq, p = kPlants[k].prof, len = 3 * kSizes[p];
                unsigned const cnt = dcp_seq_window_count(kLen[q], WINDOW, STEP), wl = kLen[q] < WINDOW ? kLen[q] : WINDOW;
                unsigned inside = 0;
                for (unsigned i = 0; i < cnt; ++i)
                {
                    unsigned const off = dcp_seq_window_start(kLen[q], WINDOW, STEP, i);
                    if (off > kPlants[k].at || kPlants[k].at + len > off + wl) continue;
                    ++inside;
                    long long const id = window_id(SEQ_ID0 + q, off, NULL);
                    bool const plus_row = has_row(cut, id, p), minus_row = has_row(cut, -id - 1, p);
                    bool const ok = kPlants[k].minus ? !plus_row && minus_row == minus : plus_row && !minus_row;
                    if (!ok) fprintf(stderr, "plant %u (sequence %u, profile %u) in the window at %u: plus row %d, minus row %d\n", k, q, p, off, plus_row, minus_row);
                    CHECK(ok);
                }
                CHECK(inside >= 1);
            }
            free(cut), free(hand);
        }
        /* row order within a job (one partition): per source sequence its windows by offset, per window its plus rows
         * and then its minus rows */
        long long last_win = -1;
        int last_minus = 0;
        for (char const *l = first ? strchr(first, '\n') : NULL; l && l[1]; l = strchr(l + 1, '\n'))
        {
            long long scan = 0, id = 0;
            CHECK(sscanf(l + 1, "%lld\t%lld\t", &scan, &id) == 2 && scan == SCAN_ID);
            long long const win = id < 0 ? -id - 1 : id;
            CHECK(win > last_win || (win == last_win && (id < 0) >= last_minus));
            last_win = win, last_minus = id < 0;
        }
        CHECK(first && count_rows(first) > NPLANTS);
        free(first);
    }
    /* window_step 0 is window / 2 */
    {
        struct job a = {1, WINDOW, 0, window_id, false, false, 1, 3, 0}, b = {1, WINDOW, STEP, window_id, false, false, 1, 3, 0};
        char *half = run_job(a, NULL, RC_OK), *named = run_job(b, NULL, RC_OK);
        CHECK(half && named && !strcmp(half, named));
        free(half), free(named);
    }
    /* the refusals: window without window_id, a step above the window -- before anything is read or written */
    {
        struct job a = {1, WINDOW, STEP, NULL, false, false, 1, 3, 0}, b = {1, WINDOW, WINDOW + 1, window_id, false, false, 1, 3, 0};
        CHECK(run_job(a, NULL, RC_EINVAL) == NULL);
        CHECK(run_job(b, NULL, RC_EINVAL) == NULL);
    }
    /* the members zero: whole sequences, as before -- the bytes of a job that cuts every sequence into one window (the
     * longest has 1 531 bases) under the sequence's own id; and the whole 1 531-nt sequence carries all its plants */
    {
        struct job plain = {0, 0, 0, NULL, true, false, 1, 3, 0}, one = {1, LMAX, LMAX, own_id, true, false, 1, 3, 0};
        char *was = run_job(plain, NULL, RC_OK), *now = run_job(one, NULL, RC_OK);
        CHECK(g_pairs == (unsigned long)NPROF * NSEQ);
        CHECK(was && now && !strcmp(was, now));
        for (unsigned k = 0; was && k < NPLANTS; ++k)
        {
            long long const id = SEQ_ID0 + (long long)kPlants[k].seq;
            CHECK(has_row(was, kPlants[k].minus ? -id - 1 : id, kPlants[k].prof));
        }
        free(was), free(now);
    }
    scan_resident_release();
    unlink(g_db_path);
    if (failed) fprintf(stderr, "%d checks failed\n", failed);
    else printf("all checks passed\n");
    return failed;
}
