/* The C half of profiles/decode_probe.py: what the decode of the hits' paths costs a scan_run_source job on the host
 * (protein_profile_decode inside the product rows, up to 32 OpenMP threads) and on the device (scan_cfg.device_decode =
 * dcp_gpu_decode_paths behind the traceback).  The job is profiles/host_scan_probe.c's mixed-length one (same generator,
 * same seeds: 3 000 sequences log-uniform on 100 nt .. 10 kbp against the C3-shaped database, passes of 4 Mi bases).
 *
 *   decode_probe DB_PATH [nprofiles=20000] [nseqs=3000]
 *   DB_PATH is pressed if it does not exist (and left there: the driver runs this program once per CPU count).
 *   The number of host threads is the number of CPUs the process may run on (the driver sets the affinity).
 *
 * Four jobs with keep_resident: host decode (fresh load), host decode (resident), device decode (uploaded again: the
 * flag is part of the resident key), device decode (resident).  One line per job. */
#include "deciphon_host.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>
#include <omp.h>
#include <math.h>

static double now(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64(void)
{
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static double next_unit(void) { return ((double)(next_u64() >> 11) + 0.5) / 9007199254740992.0; }
static double next_normal(void) { return sqrt(-2.0 * log(next_unit())) * cos(6.283185307179586 * next_unit()); }

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

int main(int argc, char **argv)
{
    if (argc < 2) return fprintf(stderr, "usage: decode_probe DB_PATH [nprofiles] [nseqs]\n"), 1;
    char const *path = argv[1];
    unsigned const nprof = argc > 2 ? (unsigned)atoi(argv[2]) : 20000u;
    unsigned const nseqs = argc > 3 ? (unsigned)atoi(argv[3]) : 3000u;
    printf("host layer build: imm_float is %zu bytes; %d CPUs\n", sizeof(imm_float), omp_get_num_procs());
    printf("no build of the parent commit ran here: the \"host decode\" jobs (device_decode = false, the default) run the parent's\n"
           "product-row code unchanged -- prod_fwrite_fp gets a NULL codes argument and calls the match function as before\n");

    /* the database's core sizes come first in the generator's stream, pressed or not: the sequences are the same */
    double sum_core = 0;
    unsigned *sizes = malloc((size_t)nprof * sizeof *sizes);
    for (unsigned p = 0; p < nprof; ++p)
    {
        double m = exp(log(150.0) + 0.6 * next_normal());
        sizes[p] = (unsigned)(m < 30 ? 30 : m > 2000 ? 2000 : m + 0.5);
        sum_core += sizes[p];
    }
    if (access(path, R_OK))
    {
        struct imm_nuclt const *nuclt = imm_super(&imm_dna_iupac);
        struct imm_nuclt_code code;
        imm_nuclt_code_init(&code, nuclt);
        FILE *fp = fopen(path, "wb");
        if (!fp) return perror(path), 2;
        double const t0 = now();
        struct protein_db_writer db = {0};
        if (protein_db_writer_open(&db, fp, &imm_amino_iupac, nuclt, PROTEIN_CFG_DEFAULT) != RC_OK) return 2;
        for (unsigned p = 0; p < nprof; ++p)
        {
            struct protein_profile prof;
            char acc[16];
            snprintf(acc, sizeof acc, "PF%05u", p);
            protein_profile_init(&prof, acc, &imm_amino_iupac, &code, PROTEIN_CFG_DEFAULT);
            if (protein_profile_sample(&prof, 0xDEC1F0u + p, sizes[p]) != RC_OK) return 3;
            if (protein_db_writer_pack_profile(&db, &prof) != RC_OK) return 4;
            profile_del(&prof.super);
        }
        if (db_writer_close((struct db_writer *)&db, true) != RC_OK) return 5;
        fclose(fp);
        printf("press: %u profiles (sum M = %.0f), %.2f s\n", nprof, sum_core, now() - t0);
    }
    free(sizes);
    printf("extra resident bytes of keep-dists: %.1f MB of compact distributions (516 B x %.0f nodes; a default two-layout "
           "float DB holds them anyway) + %.1f MB of exp() tables, rows and epsilons (1 104 B x %u profiles)\n",
           516.0 * sum_core / 1e6, sum_core, 1104.0 * nprof / 1e6, nprof);

    struct scan_seq *seqs = calloc(nseqs, sizeof *seqs);
    unsigned *lens = malloc((size_t)nseqs * sizeof *lens);
    size_t total_len = 0;
    for (unsigned q = 0; q < nseqs; ++q)
    {
        lens[q] = (unsigned)(exp(log(100.0) + next_unit() * log(100.0)) + 0.5); /* 100 .. 10 000, log-uniform */
        total_len += lens[q];
    }
    char *text = malloc(total_len + nseqs);
    size_t at = 0;
    for (unsigned q = 0; q < nseqs; ++q)
    {
        char *s = text + at;
        for (unsigned i = 0; i < lens[q]; i += 32)
        {
            uint64_t r = next_u64();
            for (unsigned k = 0; k < 32 && i + k < lens[q]; ++k, r >>= 2)
                s[i + k] = "ACGT"[r & 3u];
        }
        s[lens[q]] = '\0';
        seqs[q].id = (int64_t)q + 1;
        seqs[q].data = s;
        at += lens[q] + 1u;
    }
    for (int job = 0; job < 4; ++job)
    {
        bool const device = job >= 2;
        struct list_src src = {seqs, nseqs, 0};
        struct scan_cfg cfg = {.scan_id = 1, .multi_hits = true, .hmmer3_compat = false, .lrt_threshold = 10.0, .batch = 1u << 20,
                               .balance_by_cells = true, .keep_resident = true, .batch_symbols = 4ul << 20, .device_decode = device};
        double const t0 = now();
        enum rc rc = scan_run_source(path, cfg, 1, list_src_next, &src);
        double const dt = now() - t0;
        if (rc != RC_OK) return fprintf(stderr, "scan_run_source: rc %d\n", (int)rc), 6;
        prod_final_cleanup();
        struct scan_stats ss;
        scan_last_stats(&ss);
        printf("job %d (%s decode, %s): %zu bases, %.3f s wall; load %.3f, scans %.3f, hit fetch + traceback %.3f, device decode "
               "%.1f ms, product rows %.3f s; %u passes, %lu hits, %lu path steps\n",
               job, device ? "device" : "host", job & 1 ? "database resident" : "database loaded", total_len, dt, ss.load_s,
               ss.scan_wait_s, ss.trace_s, 1e3 * ss.decode_s, ss.rows_s, ss.passes, ss.hits, ss.steps);
    }
    scan_resident_release();
    free(text), free(lens), free(seqs);
    return 0;
}
