/*
 * GPU test of scan_cfg.device_decode (include/deciphon_host.h): the paths of scan_run_source's hits decoded on the
 * device.  Builds in float against libdeciphon_host.so and with -DIMM_DOUBLE_PRECISION against libdeciphon_host_f64.so.
 *
 * A job of 6 profiles x 8 sequences runs on both strands with device_decode set and again unset, for passes of 3 and
 * 100 sequences and for 1 and 2 partitions.  The products must be identical in every field except codon and amino of
 * M-state steps; there at most 1 step in 1 000 may differ (the device takes exp() of a match distribution itself: a tie
 * of two codons to about 2^-48 may fall the other way), and the amino must be the genetic code's letter for the
 * written codon.  scan_last_stats().decode_s > 0 only with the flag.  Under keep_resident a second job with the same
 * flag picks the resident database up (scan_stats.uploads == 0), a job with the flag flipped uploads again -- and, flipped back, decodes on the
 * device again (a double database left resident without its distributions could not).
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
enum { NPROF = 6, SCAN_ID = 78, DOM_MAX = 3 * 70 };
static unsigned const kSizes[NPROF] = {20, 33, 57, 41, 64, 65};
static char g_domain[NPROF][DOM_MAX + 1];
static char g_acc[NPROF][16];
static char g_db_path[64];

static void press_db(void)
{
    static char const amino[] = "ACDEFGHIKLMNPQRSTVWY";
    struct imm_nuclt const *nuclt = imm_super(&imm_dna_iupac);
    struct imm_nuclt_code code;
    imm_nuclt_code_init(&code, nuclt);
    snprintf(g_db_path, sizeof g_db_path, "/tmp/dcp_test_decode_XXXXXX");
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

/* ---- the sequences: 0, 2, 5 carry a domain forward (2 carries two), 1, 4, 7 the reverse complement of one --------- */
enum { NSEQ = 8, SEQ_ID0 = 200 };
static char g_text[NSEQ][1024];
static struct scan_seq g_seqs[NSEQ];
static int const kMinusOf[NSEQ] = {-1, 1, -1, -1, 4, -1, -1, 5};
static int const kPlusOf[NSEQ] = {3, -1, 0, -1, -1, 2, -1, -1};

static int64_t minus_id(int64_t id, void *arg)
{
    (void)arg;
    return -id - 1;
}

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

static void make_sequences(void)
{
    char const *flank[NSEQ] = {"ACGTTGCAAGGCTTAACC", "TTGACCA", "GGGCATCATCAGGAC", "A", "CCGTA", "GATTA", "TGCATGCAATCATTACAGGATCCAAG", "C"};
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

/* the whole products file of one job and its stats */
static char *job(bool device_decode, unsigned nthreads, unsigned batch, struct scan_stats *st)
{
    struct list_src src = {g_seqs, NSEQ, 0};
    struct scan_cfg cfg = {.scan_id = SCAN_ID, .multi_hits = true, .hmmer3_compat = false, .lrt_threshold = 10.0,
                           .batch = batch, .balance_by_cells = nthreads > 1, .keep_resident = true,
                           .minus_strand_id = minus_id, .device_decode = device_decode};
    CHECK(scan_run_source(g_db_path, cfg, nthreads, list_src_next, &src) == RC_OK);
    CHECK(src.at == src.n);
    char *text = slurp(prod_final_fp());
    prod_final_cleanup();
    scan_last_stats(st);
    return text;
}

/* the next piece of *at up to `sep` or `end` (whichever comes first), NUL-terminated into buf */
static bool piece(char const **at, char const *end, char sep, char *buf, size_t cap)
{
    if (*at > end) return false;
    char const *e = memchr(*at, sep, (size_t)(end - *at));
    if (!e) e = end;
    size_t const n = (size_t)(e - *at);
    if (n >= cap) return false;
    memcpy(buf, *at, n);
    buf[n] = '\0';
    *at = e + 1;
    return true;
}

/* Every field of the two files equal, except codon and amino of M-state steps: those are counted.  The amino of every
 * emitting step of `dev` is the genetic code's letter for its codon. */
static void compare(char const *host, char const *dev, unsigned long *m_steps, unsigned long *m_diff)
{
    struct imm_nuclt const *nuclt = imm_super(&imm_dna_iupac);
    static char mh[1 << 12], md[1 << 12];
    char const *lh = host, *ld = dev;
    unsigned rows = 0;
    while (*lh && *ld)
    {
        char const *eh = strchr(lh, '\n'), *ed = strchr(ld, '\n');
        CHECK(eh && ed);
        if (!eh || !ed) return;
        /* the eight leading fields, tabs included */
        char const *th = lh, *td = ld;
        for (int f = 0; f < 8 && th && td; ++f)
            th = memchr(th, '\t', (size_t)(eh - th)), td = memchr(td, '\t', (size_t)(ed - td)), th = th ? th + 1 : NULL, td = td ? td + 1 : NULL;
        if (lh == host || !th || !td)
        {
            /* the header line */
            CHECK(eh - lh == ed - ld && !memcmp(lh, ld, (size_t)(eh - lh)));
        }
        else
        {
            CHECK(th - lh == td - ld && !memcmp(lh, ld, (size_t)(th - lh)));
            ++rows;
            while (piece(&th, eh, ';', mh, sizeof mh))
            {
                bool const more = piece(&td, ed, ';', md, sizeof md);
                CHECK(more);
                if (!more) break;
                char fh[4][64], fd[4][64];
                char const *ph = mh, *pd = md, *endh = mh + strlen(mh), *endd = md + strlen(md);
                bool ok = true;
                for (int k = 0; k < 4; ++k)
                    ok = ok && piece(&ph, endh, ',', fh[k], sizeof fh[k]) && piece(&pd, endd, ',', fd[k], sizeof fd[k]);
                CHECK(ok);
                if (!ok) break;
                CHECK(!strcmp(fh[0], fd[0]) && !strcmp(fh[1], fd[1])); /* fragment and state */
                bool const is_m = fh[1][0] == 'M';
                bool const same = !strcmp(fh[2], fd[2]) && !strcmp(fh[3], fd[3]);
                if (is_m) ++*m_steps, *m_diff += !same;
                else CHECK(same);
                if (fd[0][0])
                {
                    CHECK(strlen(fd[2]) == 3 && strlen(fd[3]) == 1);
                    if (strlen(fd[2]) == 3) CHECK(fd[3][0] == imm_gc_decode(1, imm_codon_from_symbols(nuclt, fd[2])));
                }
                else CHECK(!fd[2][0] && !fd[3][0]);
            }
            CHECK(!piece(&td, ed, ';', md, sizeof md)); /* no step more */
        }
        lh = eh + 1, ld = ed + 1;
    }
    CHECK(!*lh && !*ld);
    CHECK(rows >= 6); /* the planted domains: three forward, three on the minus strand */
}

int main(void)
{
    press_db();
    make_sequences();
    static struct
    {
        unsigned nthreads, batch;
    } const cases[] = {{1, 3}, {1, 100}, {2, 3}, {2, 100}};
    unsigned long m_steps = 0, m_diff = 0;
    for (unsigned c = 0; c < sizeof cases / sizeof cases[0]; ++c)
    {
        struct scan_stats sh, sd;
        char *host = job(false, cases[c].nthreads, cases[c].batch, &sh);
        char *dev = job(true, cases[c].nthreads, cases[c].batch, &sd);
        CHECK(sh.decode_s == 0.0 && sd.decode_s > 0.0);
        CHECK(sh.hits == sd.hits && sh.steps == sd.steps && sd.hits >= 6);
        compare(host, dev, &m_steps, &m_diff);
        CHECK(strstr(dev, "\n78\t-") != NULL); /* rows of the minus strand are among them */
        free(host), free(dev);
    }
    printf("%lu of %lu M-state steps differ between the host's and the device's decode\n", m_diff, m_steps);
    CHECK(m_steps >= 500 && m_diff * 1000 <= m_steps);
    /* keep_resident: the flag is part of the resident database's key */
    {
        struct scan_stats first, again, flipped, back;
        scan_resident_release();
        char *a = job(true, 1, 100, &first);
        char *b = job(true, 1, 100, &again);     /* picked up: nothing is loaded */
        char *c = job(false, 1, 100, &flipped);  /* uploaded again */
        char *d = job(true, 1, 100, &back);      /* and again, with its distributions */
        CHECK(!strcmp(a, b) && !strcmp(a, d));
        unsigned long ms = 0, md = 0;
        compare(c, d, &ms, &md);
        CHECK(first.uploads == 1 && again.uploads == 0 && flipped.uploads == 1 && back.uploads == 1);
        CHECK(again.decode_s > 0.0 && flipped.decode_s == 0.0 && back.decode_s > 0.0);
        free(a), free(b), free(c), free(d);
    }
    scan_resident_release();
    unlink(g_db_path);
    if (failed) fprintf(stderr, "%d checks failed\n", failed);
    else printf("all checks passed\n");
    return failed;
}
