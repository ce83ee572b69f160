/*
 * The calibration's host functions (include/dcp_gpu.h: dcp_seq_random_thresholds, dcp_seq_random, dcp_gumbel_fit,
 * dcp_gumbel_sf, dcp_hits_evalues[64]) under ASan + UBSan: a stand-alone CPU program, linked with csrc/dcp_model.cpp
 * alone.  Every array lives on the heap at exactly the size the call is told; the generator is checked against the
 * rule restated here, the fit for its statuses and its strides; the refusals write nothing.
 */
#include "dcp_gpu.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

static uint64_t sm(uint64_t x)
{
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static void generator(void)
{
    static unsigned const lens[] = {1, 3, 4, 5, 16, 17, 1000, 4099};
    static uint64_t const seeds[] = {0, 1, 0xffffffffffffffffull, 0x0123456789abcdefull};
    static uint32_t const qs[] = {0, 1, 0xffffffffu};
    double const skew[4] = {0.1, 0.4, 0.0, 0.5};
    uint32_t c[3] = {9, 9, 9};
    CHECK(dcp_seq_random_thresholds(NULL, c) == DCP_OK && c[0] == 16384 && c[1] == 32768 && c[2] == 49152);
    for (int pass = 0; pass < 2; ++pass)
    {
        if (pass) CHECK(dcp_seq_random_thresholds(skew, c) == DCP_OK && c[0] == 6554 && c[1] == 32768 && c[2] == 32768);
        for (unsigned s = 0; s < sizeof seeds / sizeof *seeds; ++s)
            for (unsigned k = 0; k < sizeof qs / sizeof *qs; ++k)
                for (unsigned l = 0; l < sizeof lens / sizeof *lens; ++l)
                {
                    unsigned const L = lens[l];
                    uint8_t *ids = malloc(L); /* exactly L: a write behind the last base is a finding */
                    dcp_seq_random(seeds[s], qs[k], L, c, ids);
                    uint64_t const key = sm(seeds[s] ^ sm(qs[k]));
                    for (unsigned b = 0; b < L; ++b)
                    {
                        uint32_t const u = (uint32_t)(sm(key + (b >> 2)) >> (16 * (b & 3))) & 0xffffu;
                        CHECK(ids[b] == (u >= c[0]) + (u >= c[1]) + (u >= c[2]));
                        if (pass) CHECK(ids[b] != 2);
                    }
                    free(ids);
                }
    }
    dcp_seq_random(1, 0, 0, c, NULL); /* nothing to write */
    /* the refusals */
    double const bad[][4] = {{0.5, 0.5, 0.5, 0.5}, {1.5, -0.5, 0, 0}, {NAN, 0.5, 0.25, 0.25}, {INFINITY, 0, 0, 0},
                             {0.25, 0.25, 0.25, 0.25 + 2e-6}};
    for (unsigned i = 0; i < sizeof bad / sizeof *bad; ++i)
    {
        uint32_t t[3] = {7, 7, 7};
        CHECK(dcp_seq_random_thresholds(bad[i], t) == DCP_EINVAL && t[0] == 7 && t[1] == 7 && t[2] == 7);
    }
    CHECK(dcp_seq_random_thresholds(skew, NULL) == DCP_EINVAL);
    double const one[4] = {1, 0, 0, 0}, last[4] = {0, 0, 0, 1};
    CHECK(dcp_seq_random_thresholds(one, c) == DCP_OK && c[0] == 65536 && c[2] == 65536);
    CHECK(dcp_seq_random_thresholds(last, c) == DCP_OK && c[0] == 0 && c[2] == 0);
}

/* a Gumbel(mu, 1 / lambda) sample from the generator's own draws */
static void sample(double *x, unsigned n, size_t stride, double mu, double lambda, uint64_t seed)
{
    for (unsigned i = 0; i < n; ++i)
    {
        double const u = ((double)(sm(seed + i) >> 11) + 0.5) / 9007199254740992.0;
        x[i * stride] = mu - log(-log(u)) / lambda;
    }
}

static void fit(void)
{
    static unsigned const ns[] = {2, 3, 64, 300};
    static size_t const strides[] = {1, 2, 7};
    for (unsigned k = 0; k < sizeof ns / sizeof *ns; ++k)
        for (unsigned s = 0; s < sizeof strides / sizeof *strides; ++s)
        {
            unsigned const n = ns[k];
            size_t const stride = strides[s], size = (n - 1) * stride + 1; /* the last value is the last element */
            double *x = malloc(size * sizeof *x), *dense = malloc(n * sizeof *dense);
            for (size_t i = 0; i < size; ++i)
                x[i] = NAN; /* a value read between the strides would show */
            sample(x, n, stride, -4.0, 0.7, 1000 + n);
            sample(dense, n, 1, -4.0, 0.7, 1000 + n);
            double mu = 5, lam = 6, mu1 = 5, lam1 = 6;
            int const st = dcp_gumbel_fit(x, n, stride, &mu, &lam), st1 = dcp_gumbel_fit(dense, n, 1, &mu1, &lam1);
            CHECK(st == st1 && (st == DCP_FIT_OK || st == DCP_FIT_DIVERGED));
            if (st == DCP_FIT_OK) CHECK(mu == mu1 && lam == lam1 && lam > 0);
            else CHECK(isnan(mu) && isnan(lam));
            if (n >= 64) CHECK(st == DCP_FIT_OK && fabs(lam - 0.7) < 0.2 && fabs(mu + 4.0) < 1.0);
            /* statuses */
            for (unsigned i = 0; i < n; ++i)
                dense[i] = 2.5;
            CHECK(dcp_gumbel_fit(dense, 2, 1, &mu, &lam) == DCP_FIT_FLAT && isnan(mu) && isnan(lam));
            sample(dense, n, 1, 0.0, 1.0, 77);
            dense[n - 1] = -INFINITY;
            CHECK(dcp_gumbel_fit(dense, n, 1, &mu, &lam) == DCP_FIT_NONFINITE && isnan(mu) && isnan(lam));
            dense[n - 1] = 0.0, dense[0] = INFINITY;
            CHECK(dcp_gumbel_fit(dense, n, 1, &mu, &lam) == DCP_FIT_NONFINITE);
            dense[0] = NAN;
            CHECK(dcp_gumbel_fit(dense, n, 1, &mu, &lam) == DCP_FIT_NONFINITE);
            /* the refusals */
            mu = 5, lam = 6;
            CHECK(dcp_gumbel_fit(dense, 1, 1, &mu, &lam) == DCP_EINVAL && dcp_gumbel_fit(dense, 0, 1, &mu, &lam) == DCP_EINVAL);
            CHECK(dcp_gumbel_fit(NULL, n, 1, &mu, &lam) == DCP_EINVAL && dcp_gumbel_fit(dense, n, 0, &mu, &lam) == DCP_EINVAL);
            CHECK(dcp_gumbel_fit(dense, n, 1, NULL, &lam) == DCP_EINVAL && dcp_gumbel_fit(dense, n, 1, &mu, NULL) == DCP_EINVAL);
            CHECK(mu == 5 && lam == 6);
            free(x), free(dense);
        }
}

static void evalues(void)
{
    CHECK(fabs(dcp_gumbel_sf(0.0, 1.0, 0.0) - (1.0 - exp(-1.0))) < 1e-15);
    CHECK(fabs(dcp_gumbel_sf(2.0, 0.5, 82.0) / exp(-40.0) - 1.0) < 1e-12);
    unsigned const n = 5, np = 3;
    struct dcp_hit *h = malloc(n * sizeof *h);
    struct dcp_hit64 *h64 = malloc(n * sizeof *h64);
    double *mu = malloc(np * sizeof *mu), *lam = malloc(np * sizeof *lam), *e = malloc(n * sizeof *e), *e64 = malloc(n * sizeof *e64);
    uint8_t *st = malloc(np);
    for (unsigned p = 0; p < np; ++p)
        mu[p] = 1.0 + p, lam[p] = 0.5 + 0.1 * p, st[p] = p == 1 ? DCP_FIT_FLAT : DCP_FIT_OK;
    for (unsigned i = 0; i < n; ++i)
    {
        h[i].seq_idx = h64[i].seq_idx = i, h[i].profile_idx = h64[i].profile_idx = i % np;
        h[i].null_loglik = -100.0f - (float)i, h[i].alt_loglik = -90.0f + 2.0f * (float)i;
        h64[i].null_loglik = h[i].null_loglik, h64[i].alt_loglik = h[i].alt_loglik;
        e[i] = e64[i] = 9.0;
    }
    CHECK(dcp_hits_evalues(h, n, mu, lam, st, np, 1000.0, e) == DCP_OK);
    CHECK(dcp_hits_evalues64(h64, n, mu, lam, st, np, 1000.0, e64) == DCP_OK);
    for (unsigned i = 0; i < n; ++i)
    {
        unsigned const p = i % np;
        double const want = 1000.0 * dcp_gumbel_sf(mu[p], lam[p], (double)h[i].alt_loglik - (double)h[i].null_loglik);
        if (p == 1) CHECK(isnan(e[i]) && isnan(e64[i]));
        else CHECK(e[i] == want && e64[i] == want);
        e[i] = e64[i] = 9.0;
    }
    /* the refusals: nothing written */
    CHECK(dcp_hits_evalues(h, n, mu, lam, st, 2, 1000.0, e) == DCP_EINVAL); /* profile 2 >= 2 */
    CHECK(dcp_hits_evalues64(h64, n, mu, lam, st, 2, 1000.0, e64) == DCP_EINVAL);
    CHECK(dcp_hits_evalues(h, n, mu, lam, st, np, NAN, e) == DCP_EINVAL && dcp_hits_evalues(h, n, mu, lam, st, np, -1.0, e) == DCP_EINVAL);
    CHECK(dcp_hits_evalues(h, n, mu, lam, st, np, INFINITY, e) == DCP_EINVAL);
    CHECK(dcp_hits_evalues(NULL, n, mu, lam, st, np, 1.0, e) == DCP_EINVAL && dcp_hits_evalues(h, n, NULL, lam, st, np, 1.0, e) == DCP_EINVAL);
    CHECK(dcp_hits_evalues(h, n, mu, NULL, st, np, 1.0, e) == DCP_EINVAL && dcp_hits_evalues(h, n, mu, lam, NULL, np, 1.0, e) == DCP_EINVAL);
    CHECK(dcp_hits_evalues64(h64, n, mu, lam, st, np, 1.0, NULL) == DCP_EINVAL);
    for (unsigned i = 0; i < n; ++i)
        CHECK(e[i] == 9.0 && e64[i] == 9.0);
    CHECK(dcp_hits_evalues(NULL, 0, NULL, NULL, NULL, 0, 1.0, NULL) == DCP_OK);
    free(h), free(h64), free(mu), free(lam), free(e), free(e64), free(st);
}

int main(void)
{
    generator();
    fit();
    evalues();
    if (failed) return 1;
    puts("asan_calib ok");
    return 0;
}
