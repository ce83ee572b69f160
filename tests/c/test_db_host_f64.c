/*
 * CPU-only test of the host layer's DOUBLE build (compiled with -DIMM_DOUBLE_PRECISION against
 * libdeciphon_host_f64.so; no device call): imm_float is a double in every public struct, a pressed .dcp
 * carries float_size 8, epsilon as a MessagePack float64 and its nuclt_dist / dp arrays as float64 1darrays,
 * and every double a profile holds comes back bit for bit through profile_reader_* with 1, 2 and 7 partitions.
 * A float file is refused with the reference's code (src/db/reader.c:51: einval "invalid float size"),
 * truncated and corrupted files fail cleanly.
 *
 *   test_db_host_f64                 all checks
 *   test_db_host_f64 press <out>     press a small double database (for the float build's reader to refuse)
 *   test_db_host_f64 open <in>       protein_db_reader_open on a file; prints "rc=<n>"
 * Exit status = number of failed checks.
 */
#include "deciphon_host.h"
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#ifndef IMM_DOUBLE_PRECISION
#error "this test is the double build's: compile it with -DIMM_DOUBLE_PRECISION"
#endif
_Static_assert(sizeof(imm_float) == 8 && IMM_FLOAT_BYTES == 8, "imm_float is a double in the double build");
_Static_assert(sizeof(((struct imm_prod *)0)->loglik) == 8 && sizeof(((struct protein_cfg *)0)->epsilon) == 8 &&
                   sizeof(((struct protein_trans *)0)->MM) == 8 && sizeof(((struct protein_profile *)0)->xtrans) == 13 * 8 &&
                   sizeof(((struct imm_nuclt_lprob *)0)->lprobs) == 4 * 8 && sizeof(((struct imm_codon_marg *)0)->lprobs) == 125 * 8,
               "every public struct carries doubles");

static int failed;
#define CHECK(cond)                                                                        \
    do                                                                                     \
    {                                                                                      \
        if (!(cond))                                                                       \
        {                                                                                  \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond);       \
            failed++;                                                                      \
        }                                                                                  \
    } while (0)

enum { NPROF = 7 };
static unsigned const kSizes[NPROF] = {2, 63, 4096, 1, 64, 65, 512};

static FILE *tmp(char path[64])
{
    snprintf(path, 64, "/tmp/dcp_test_db64_XXXXXX");
    int fd = mkstemp(path);
    return fd < 0 ? NULL : fdopen(fd, "wb+");
}

static void make_profile(struct protein_profile *prof, struct imm_nuclt_code const *code, struct protein_cfg cfg, unsigned p)
{
    char acc[16];
    snprintf(acc, sizeof acc, "PF%05u.%u", p, p + 1);
    protein_profile_init(prof, acc, &imm_amino_iupac, code, cfg);
    if (kSizes[p] >= 2) CHECK(protein_profile_sample(prof, 100 + p, kSizes[p]) == RC_OK);
    else
    {
        /* protein_profile_sample asserts core_size >= 2: a 1-node profile through the model builder, in double */
        struct imm_rnd rnd = imm_rnd(5);
        imm_float null[IMM_AMINO_SIZE], match[IMM_AMINO_SIZE];
        struct protein_trans t[2];
        imm_lprob_sample(&rnd, IMM_AMINO_SIZE, null);
        imm_lprob_normalize(IMM_AMINO_SIZE, null);
        imm_lprob_sample(&rnd, IMM_AMINO_SIZE, match);
        imm_lprob_normalize(IMM_AMINO_SIZE, match);
        for (int i = 0; i < 2; ++i)
        {
            imm_lprob_sample(&rnd, PROTEIN_TRANS_SIZE, t[i].data);
            imm_lprob_normalize(PROTEIN_TRANS_SIZE, t[i].data);
        }
        /* a normalised vector of doubles: its probabilities sum to 1 within a few ulp, which a float one does not */
        double sum = 0;
        for (int i = 0; i < IMM_AMINO_SIZE; ++i)
            sum += exp(null[i]);
        CHECK(fabs(sum - 1) < 1e-14);
        CHECK((double)(float)null[3] != null[3]); /* not float values */
        struct protein_model model;
        protein_model_init(&model, &imm_amino_iupac, code, cfg, null);
        CHECK(protein_model_setup(&model, 1) == RC_OK);
        CHECK(protein_model_add_node(&model, match, 'K') == RC_OK);
        CHECK(protein_model_add_trans(&model, t[0]) == RC_OK);
        CHECK(protein_model_add_trans(&model, t[1]) == RC_OK);
        CHECK(protein_profile_absorb(prof, &model) == RC_OK);
        CHECK(prof->core_size == 1 && prof->consensus[0] == 'K');
        protein_model_del(&model);
    }
    CHECK(dcp_profile_precision(prof->impl) == 64);
    /* odd profiles carry the special transitions of a setup (doubles that are not float values), even ones LOG1 */
    if (p % 2) CHECK(protein_profile_setup(prof, 100 + p, p % 4 == 1, false) == RC_OK);
}

/* every double part, the struct members mirrored from them, xtrans and epsilon */
static int same_profile(struct protein_profile const *a, struct protein_profile const *b)
{
    unsigned const M = a->core_size;
    if (M != b->core_size || strcmp(a->super.accession, b->super.accession) || strcmp(a->consensus, b->consensus)) return 0;
    if (dcp_profile_precision(a->impl) != 64 || dcp_profile_precision(b->impl) != 64) return 0;
    double const ea = dcp_profile_epsilon64(a->impl), eb = dcp_profile_epsilon64(b->impl);
    if (memcmp(&ea, &eb, 8) || memcmp(&a->cfg.epsilon, &b->cfg.epsilon, 8) || memcmp(&a->cfg.epsilon, &ea, 8)) return 0;
    if (memcmp(&a->eps, &b->eps, sizeof a->eps)) return 0;
    if (memcmp(dcp_profile_trans8_64(a->impl), dcp_profile_trans8_64(b->impl), sizeof(double) * 8 * M)) return 0;
    if (memcmp(dcp_profile_match_dist64(a->impl), dcp_profile_match_dist64(b->impl), sizeof(double) * DCP_NDIST * M)) return 0;
    if (memcmp(dcp_profile_null_dist64(a->impl), dcp_profile_null_dist64(b->impl), sizeof(double) * DCP_NDIST)) return 0;
    if (memcmp(dcp_profile_insert_dist64(a->impl), dcp_profile_insert_dist64(b->impl), sizeof(double) * DCP_NDIST)) return 0;
    /* the float parts are those doubles rounded once, on both sides */
    if (memcmp(dcp_profile_trans8(a->impl), dcp_profile_trans8(b->impl), sizeof(float) * 8 * M)) return 0;
    if (memcmp(dcp_profile_match_dist(a->impl), dcp_profile_match_dist(b->impl), sizeof(float) * DCP_NDIST * M)) return 0;
    for (unsigned k = 0; k < M; ++k)
    {
        if (memcmp(a->alt.match_ndists[k].nucltp.lprobs, b->alt.match_ndists[k].nucltp.lprobs, sizeof(double) * 4)) return 0;
        if (memcmp(a->alt.match_ndists[k].codonm.lprobs, b->alt.match_ndists[k].codonm.lprobs, sizeof(double) * 125)) return 0;
        /* the struct's view is the compact profile's row */
        if (memcmp(a->alt.match_ndists[k].nucltp.lprobs, dcp_profile_match_dist64(a->impl) + (size_t)k * DCP_NDIST, sizeof(double) * 4))
            return 0;
    }
    return !memcmp(a->null.ndist.codonm.lprobs, b->null.ndist.codonm.lprobs, sizeof a->null.ndist.codonm.lprobs) &&
           !memcmp(a->alt.insert_ndist.nucltp.lprobs, b->alt.insert_ndist.nucltp.lprobs, sizeof(double) * 4) &&
           !memcmp(a->xtrans, b->xtrans, sizeof a->xtrans) && a->alt.T == b->alt.T && a->null.R == b->null.R;
}

/* offset just behind the first occurrence of `key` at or after `from` (0 if there is none) */
static long find_key(unsigned char const *buf, long n, long from, char const *key)
{
    long const k = (long)strlen(key);
    for (long i = from; i + k <= n; ++i)
        if (!memcmp(buf + i, key, (size_t)k)) return i + k;
    return 0;
}

static unsigned char *slurp(FILE *fp, long *n)
{
    fflush(fp);
    fseek(fp, 0, SEEK_END);
    *n = ftell(fp);
    rewind(fp);
    unsigned char *buf = malloc((size_t)*n + 1);
    CHECK(buf && fread(buf, 1, (size_t)*n, fp) == (size_t)*n);
    rewind(fp);
    return buf;
}

static void roundtrip(enum entry_dist entry, imm_float epsilon)
{
    struct imm_nuclt const *nuclt = imm_super(&imm_dna_iupac);
    struct imm_nuclt_code code;
    imm_nuclt_code_init(&code, nuclt);
    struct protein_cfg const cfg = protein_cfg(entry, epsilon);
    CHECK((double)(float)epsilon != epsilon); /* 0.1 and 0.01 are not float values */
    char path[64];
    FILE *fp = tmp(path);
    CHECK(fp != NULL);
    struct protein_db_writer w = {0};
    CHECK(protein_db_writer_open(&w, fp, &imm_amino_iupac, nuclt, cfg) == RC_OK);
    static struct protein_profile src[NPROF];
    for (unsigned p = 0; p < NPROF; ++p)
    {
        make_profile(&src[p], &code, cfg, p);
        CHECK(protein_db_writer_pack_profile(&w, &src[p]) == RC_OK);
    }
    CHECK(db_writer_close((struct db_writer *)&w, true) == RC_OK);

    /* the header's bytes: float_size is the fixint 8, epsilon a MessagePack float64 (0xcb) of the cfg's bits; the
     * first profile's dp and nuclt_dist arrays are 1darrays of type LIP_1DARRAY_F64 */
    long file_size = 0;
    unsigned char *bytes = slurp(fp, &file_size);
    long at = find_key(bytes, file_size, 0, "float_size");
    CHECK(at > 0 && bytes[at] == 0x08);
    at = find_key(bytes, file_size, 0, "epsilon");
    CHECK(at > 0 && bytes[at] == 0xcb);
    uint64_t be = 0, want;
    for (int i = 0; i < 8; ++i)
        be = be << 8 | bytes[at + 1 + i];
    memcpy(&want, &epsilon, 8);
    CHECK(be == want);
    at = find_key(bytes, file_size, 0, "xtrans"); /* the null dp of profile 0: ext8, 8 bytes, type 0x22 */
    CHECK(at > 0 && bytes[at] == 0xc7 && bytes[at + 1] == 8 && bytes[at + 2] == LIP_1DARRAY_F64);
    at = find_key(bytes, file_size, 0, "null_ndist"); /* array(2), then the 4 base lprobs: ext8, 32 bytes */
    CHECK(at > 0 && bytes[at] == 0x92 && bytes[at + 1] == 0xc7 && bytes[at + 2] == 32 && bytes[at + 3] == LIP_1DARRAY_F64);
    free(bytes);

    for (unsigned npart = 1; npart <= 7; npart += npart == 1 ? 1 : 5) /* 1, 2, 7 */
    {
        rewind(fp);
        struct protein_db_reader db = {0};
        CHECK(protein_db_reader_open(&db, fp) == RC_OK);
        CHECK(db.super.nprofiles == NPROF && db.super.profile_typeid == PROFILE_PROTEIN);
        CHECK(db.cfg.entry_dist == entry && !memcmp(&db.cfg.epsilon, &epsilon, 8));
        static struct profile_reader reader;
        CHECK(profile_reader_setup(&reader, (struct db_reader *)&db, npart) == RC_OK);
        CHECK(profile_reader_npartitions(&reader) == npart && profile_reader_nprofiles(&reader) == NPROF);
        unsigned j = 0;
        for (unsigned i = 0; i < npart; ++i)
        {
            struct profile *prof = NULL;
            enum rc rc;
            while ((rc = profile_reader_next(&reader, i, &prof)) == RC_OK)
            {
                CHECK(j < NPROF && same_profile((struct protein_profile *)prof, &src[j]));
                ++j;
            }
            CHECK(rc == RC_END);
        }
        CHECK(j == NPROF);
        profile_reader_del(&reader);
        db_reader_close((struct db_reader *)&db);
    }

    /* truncation anywhere in the profiles is an error of the read, never a short profile */
    for (long cut = file_size - 1; cut > file_size - 40000; cut -= 9973)
    {
        CHECK(ftruncate(fileno(fp), cut) == 0);
        rewind(fp);
        struct protein_db_reader t = {0};
        static struct profile_reader reader;
        struct profile *prof = NULL;
        CHECK(protein_db_reader_open(&t, fp) == RC_OK);
        CHECK(profile_reader_setup(&reader, (struct db_reader *)&t, 1) == RC_OK);
        enum rc rc;
        unsigned n = 0;
        while ((rc = profile_reader_next(&reader, 0, &prof)) == RC_OK)
            ++n;
        CHECK(rc != RC_END && n == NPROF - 1);
        profile_reader_del(&reader);
        db_reader_close((struct db_reader *)&t);
    }
    for (unsigned p = 0; p < NPROF; ++p)
        profile_del(&src[p].super);
    fclose(fp);
    remove(path);
}

/* a small database (profiles of 2 and 5 nodes) for the corruption checks and for the float build's reader */
static FILE *press_small(char path[64], char const *at_path)
{
    struct imm_nuclt const *nuclt = imm_super(&imm_dna_iupac);
    struct imm_nuclt_code code;
    imm_nuclt_code_init(&code, nuclt);
    FILE *fp;
    if (at_path) fp = fopen(at_path, "wb+");
    else fp = tmp(path);
    if (!fp) return NULL;
    struct protein_db_writer w = {0};
    CHECK(protein_db_writer_open(&w, fp, &imm_amino_iupac, nuclt, PROTEIN_CFG_DEFAULT) == RC_OK);
    for (unsigned p = 0; p < 2; ++p)
    {
        struct protein_profile prof;
        protein_profile_init(&prof, p ? "PF00002.2" : "PF00001.1", &imm_amino_iupac, &code, PROTEIN_CFG_DEFAULT);
        CHECK(protein_profile_sample(&prof, 7 + p, p ? 5 : 2) == RC_OK);
        CHECK(protein_db_writer_pack_profile(&w, &prof) == RC_OK);
        profile_del(&prof.super);
    }
    CHECK(db_writer_close((struct db_writer *)&w, true) == RC_OK);
    return fp;
}

/* open + read every profile of the bytes; the first failing code (RC_OK if all of it reads) */
static enum rc read_all(unsigned char const *bytes, long n)
{
    char path[64];
    FILE *fp = tmp(path);
    CHECK(fp && fwrite(bytes, 1, (size_t)n, fp) == (size_t)n);
    rewind(fp);
    struct protein_db_reader db = {0};
    enum rc rc = protein_db_reader_open(&db, fp);
    if (!rc)
    {
        static struct profile_reader reader;
        struct profile *prof = NULL;
        rc = profile_reader_setup(&reader, (struct db_reader *)&db, 1);
        if (!rc)
        {
            while ((rc = profile_reader_next(&reader, 0, &prof)) == RC_OK)
                ;
            if (rc == RC_END) rc = RC_OK;
            profile_reader_del(&reader);
        }
        db_reader_close((struct db_reader *)&db);
    }
    fclose(fp);
    remove(path);
    return rc;
}

static void corrupted(void)
{
    char path[64];
    FILE *fp = press_small(path, NULL);
    CHECK(fp != NULL);
    long n = 0;
    unsigned char *good = slurp(fp, &n), *bad = malloc((size_t)n);
    fclose(fp);
    remove(path);
    CHECK(read_all(good, n) == RC_OK);
    /* float_size 4 in a double build's reader: the reference's "invalid float size", and nothing is converted */
    long at = find_key(good, n, 0, "float_size");
    memcpy(bad, good, (size_t)n), bad[at] = 4;
    CHECK(read_all(bad, n) == RC_EINVAL);
    memcpy(bad, good, (size_t)n), bad[at] = 16;
    CHECK(read_all(bad, n) == RC_EINVAL);
    /* epsilon as something that is no float at all; out of range */
    at = find_key(good, n, 0, "epsilon");
    memcpy(bad, good, (size_t)n), bad[at] = 0xc0;
    CHECK(read_all(bad, n) != RC_OK);
    memcpy(bad, good, (size_t)n), bad[at + 1] = 0x40; /* 0x40..: a value above 2 */
    CHECK(read_all(bad, n) == RC_EINVAL);
    /* a float32 array where the double build's float64 one belongs: trans8 of the alt dp, a nuclt_dist block */
    long const prof0 = find_key(good, n, 0, "profiles");
    at = find_key(good, n, prof0, "trans8");       /* the null dp's (empty) */
    at = find_key(good, n, at, "trans8");          /* the alt dp's: ext8, 8 * 2 * 8 = 128 bytes */
    CHECK(good[at] == 0xc7 && good[at + 1] == 128 && good[at + 2] == LIP_1DARRAY_F64);
    memcpy(bad, good, (size_t)n), bad[at + 2] = LIP_1DARRAY_F32;
    CHECK(read_all(bad, n) != RC_OK);
    long const t8 = at + 3;
    /* a NaN among the transitions, among the codon marginals */
    memcpy(bad, good, (size_t)n), bad[t8] = 0x7f, bad[t8 + 1] = 0xf8;
    CHECK(read_all(bad, n) != RC_OK);
    at = find_key(good, n, prof0, "alt_match_ndist");
    CHECK(good[at] == 0x92 && good[at + 1] == 0x92 && good[at + 2] == 0xc7 && good[at + 4] == LIP_1DARRAY_F64);
    memcpy(bad, good, (size_t)n), bad[at + 4] = LIP_1DARRAY_F32;
    CHECK(read_all(bad, n) != RC_OK);
    memcpy(bad, good, (size_t)n), bad[at + 5] = 0xff, bad[at + 6] = 0xf8; /* first base lprob: a NaN */
    CHECK(read_all(bad, n) != RC_OK);
    /* an array one element short (its byte count is no multiple of 8), a length past the end of the file */
    memcpy(bad, good, (size_t)n), bad[at + 3] = 31;
    CHECK(read_all(bad, n) != RC_OK);
    memcpy(bad, good, (size_t)n), bad[at + 3] = 255;
    CHECK(read_all(bad, n) != RC_OK);
    /* every prefix of the file shorter than the whole fails, none crashes */
    for (long cut = 0; cut < n; cut += 37)
        CHECK(read_all(good, cut) != RC_OK);
    free(good), free(bad);
}

static void specials_in_double(void)
{
    struct imm_nuclt_code code;
    imm_nuclt_code_init(&code, imm_super(&imm_dna_iupac));
    struct protein_profile p;
    protein_profile_init(&p, "x", &imm_amino_iupac, &code, protein_cfg(ENTRY_DIST_UNIFORM, 0.1));
    CHECK(protein_profile_sample(&p, 1, 2) == RC_OK);
    CHECK(p.eps.loge == log(0.1) && p.eps.log1e == log(1 - 0.1)); /* imm_log is log */
    CHECK(p.xtrans[0] == 0.0 && p.xtrans[9] == 0.0);
    CHECK(protein_profile_setup(&p, 0, true, false) == RC_EINVAL);
    CHECK(protein_profile_setup(&p, 100, true, false) == RC_OK);
    double xt[DCP_NXTRANS];
    CHECK(dcp_xtrans64(100, 1, 0, xt) == 0 && !memcmp(xt, p.xtrans, sizeof xt));
    CHECK((double)(float)p.xtrans[3] != p.xtrans[3]);
    unsigned const idx = imm_dp_trans_idx(&p.alt.dp, p.alt.E, p.alt.B);
    CHECK(idx == 9);
    imm_dp_change_trans(&p.alt.dp, idx, -0.1234567890123456789);
    CHECK(p.xtrans[9] == -0.1234567890123456789);
    CHECK(imm_dp_trans_idx(&p.null.dp, p.null.R, p.null.R) == 0);
    /* xmath_lrt on imm_float is the double form */
    imm_float const nul = -48.9272687711, alt = -54.35543421312;
    CHECK(xmath_lrt(nul, alt) == -2 * (nul - alt) && sizeof(xmath_lrt(nul, alt)) == 8);
    profile_del(&p.super);
}

int main(int argc, char **argv)
{
    if (argc == 3 && !strcmp(argv[1], "press"))
    {
        char unused[64];
        FILE *fp = press_small(unused, argv[2]);
        if (!fp) return 2;
        fclose(fp);
        return failed;
    }
    if (argc == 3 && !strcmp(argv[1], "open"))
    {
        FILE *fp = fopen(argv[2], "rb");
        if (!fp) return 2;
        struct protein_db_reader db = {0};
        enum rc rc = protein_db_reader_open(&db, fp);
        printf("rc=%d %s\n", (int)rc, rc_string(rc));
        if (!rc) db_reader_close((struct db_reader *)&db);
        fclose(fp);
        return 0;
    }
    specials_in_double();
    roundtrip(ENTRY_DIST_OCCUPANCY, 0.01);
    roundtrip(ENTRY_DIST_UNIFORM, 0.01);
    roundtrip(ENTRY_DIST_OCCUPANCY, 0.1);
    roundtrip(ENTRY_DIST_UNIFORM, 0.1);
    corrupted();
    if (failed) fprintf(stderr, "%d check(s) failed\n", failed);
    else puts("test_db_host_f64: all checks passed");
    return failed;
}
