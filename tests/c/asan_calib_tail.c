/*
 * The tail fit's host function (include/dcp_gpu.h: dcp_gumbel_fit_tail) under ASan + UBSan: a stand-alone CPU program,
 * linked with csrc/dcp_model.cpp alone.  Every array lives on the heap at exactly the size the call is told; tau and
 * k_eff are checked against a sort, the fit for its statuses, its strides and k = n against dcp_gumbel_fit; the
 * refusals write nothing.  E-values under a tail fit go through dcp_hits_evalues as they are.
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

/* a Gumbel(mu, 1 / lambda) sample, rounded to eighths so that values tie */
static void sample(double *x, unsigned n, size_t stride, double mu, double lambda, uint64_t seed)
{
    for (unsigned i = 0; i < n; ++i)
    {
        double const u = ((double)(sm(seed + i) >> 11) + 0.5) / 9007199254740992.0;
        x[i * stride] = floor(8.0 * (mu - log(-log(u)) / lambda)) / 8.0;
    }
}

static int descending(void const *a, void const *b)
{
    double const x = *(double const *)a, y = *(double const *)b;
    return (x < y) - (x > y);
}

static void fit(void)
{
    static unsigned const ns[] = {2, 3, 5, 64, 300};
    static size_t const strides[] = {1, 2, 7};
    for (unsigned a = 0; a < sizeof ns / sizeof *ns; ++a)
        for (unsigned s = 0; s < sizeof strides / sizeof *strides; ++s)
        {
            unsigned const n = ns[a];
            size_t const stride = strides[s], size = (n - 1) * stride + 1; /* the last value is the last element */
            double *x = malloc(size * sizeof *x), *dense = malloc(n * sizeof *dense), *sorted = malloc(n * sizeof *sorted);
            for (size_t i = 0; i < size; ++i)
                x[i] = NAN; /* a value read between the strides would show */
            sample(x, n, stride, -4.0, 0.7, 1000 + n);
            sample(dense, n, 1, -4.0, 0.7, 1000 + n);
            memcpy(sorted, dense, n * sizeof *sorted);
            qsort(sorted, n, sizeof *sorted, descending);
            unsigned const ks[] = {2, 3, n / 4, n - 1, n};
            for (unsigned b = 0; b < sizeof ks / sizeof *ks; ++b)
            {
                unsigned const k = ks[b];
                if (k < 2 || k > n) continue;
                double mu = 5, lam = 6, tau = 7, mu1 = 5, lam1 = 6, tau1 = 7;
                unsigned ke = 8, ke1 = 8, want = 0;
                int const st = dcp_gumbel_fit_tail(x, n, stride, k, &mu, &lam, &tau, &ke);
                int const st1 = dcp_gumbel_fit_tail(dense, n, 1, k, &mu1, &lam1, &tau1, &ke1);
                for (unsigned i = 0; i < n; ++i)
                    want += dense[i] >= sorted[k - 1];
                CHECK(st == st1 && (st == DCP_FIT_OK || st == DCP_FIT_DIVERGED || st == DCP_FIT_FLAT));
                CHECK(tau == sorted[k - 1] && tau1 == tau && ke == want && ke1 == want && ke >= k);
                if (st == DCP_FIT_OK) CHECK(mu == mu1 && lam == lam1 && lam > 0);
                else CHECK(isnan(mu) && isnan(lam) && isnan(mu1) && isnan(lam1));
                if (n >= 64 && k >= n / 4) CHECK(st == DCP_FIT_OK && fabs(lam - 0.7) < 0.3 && fabs(mu + 4.0) < 1.5);
                if (k == n)
                {
                    double mu0 = 5, lam0 = 6;
                    CHECK(dcp_gumbel_fit(dense, n, 1, &mu0, &lam0) == st);
                    CHECK(!memcmp(&mu0, &mu, sizeof mu) && !memcmp(&lam0, &lam, sizeof lam));
                }
            }
            /* statuses */
            double mu = 5, lam = 6, tau = 7;
            unsigned ke = 8;
            for (unsigned i = 0; i < n; ++i)
                dense[i] = 2.5;
            CHECK(dcp_gumbel_fit_tail(dense, n, 1, 2, &mu, &lam, &tau, &ke) == DCP_FIT_FLAT && isnan(mu) && isnan(lam));
            CHECK(tau == 2.5 && ke == n);
            if (n >= 3)
            { /* the whole tail at one value, a bulk below it */
                dense[0] = 1.0;
                CHECK(dcp_gumbel_fit_tail(dense, n, 1, 2, &mu, &lam, &tau, &ke) == DCP_FIT_FLAT && isnan(mu) && isnan(lam));
                CHECK(tau == 2.5 && ke == n - 1);
            }
            sample(dense, n, 1, 0.0, 1.0, 77);
            dense[n - 1] = -INFINITY;
            CHECK(dcp_gumbel_fit_tail(dense, n, 1, 2, &mu, &lam, &tau, &ke) == DCP_FIT_NONFINITE);
            CHECK(isnan(mu) && isnan(lam) && isnan(tau) && ke == 0);
            dense[n - 1] = 0.0, dense[0] = INFINITY;
            CHECK(dcp_gumbel_fit_tail(dense, n, 1, n, &mu, &lam, &tau, &ke) == DCP_FIT_NONFINITE && ke == 0);
            dense[0] = NAN;
            CHECK(dcp_gumbel_fit_tail(dense, n, 1, 2, &mu, &lam, &tau, &ke) == DCP_FIT_NONFINITE && isnan(tau));
            /* the refusals */
            dense[0] = 1.0;
            mu = 5, lam = 6, tau = 7, ke = 8;
            CHECK(dcp_gumbel_fit_tail(dense, n, 1, 0, &mu, &lam, &tau, &ke) == DCP_EINVAL);
            CHECK(dcp_gumbel_fit_tail(dense, n, 1, 1, &mu, &lam, &tau, &ke) == DCP_EINVAL);
            CHECK(dcp_gumbel_fit_tail(dense, n, 1, n + 1, &mu, &lam, &tau, &ke) == DCP_EINVAL);
            CHECK(dcp_gumbel_fit_tail(dense, 1, 1, 2, &mu, &lam, &tau, &ke) == DCP_EINVAL);
            CHECK(dcp_gumbel_fit_tail(dense, 0, 1, 2, &mu, &lam, &tau, &ke) == DCP_EINVAL);
            CHECK(dcp_gumbel_fit_tail(NULL, n, 1, 2, &mu, &lam, &tau, &ke) == DCP_EINVAL);
            CHECK(dcp_gumbel_fit_tail(dense, n, 0, 2, &mu, &lam, &tau, &ke) == DCP_EINVAL);
            CHECK(dcp_gumbel_fit_tail(dense, n, 1, 2, NULL, &lam, &tau, &ke) == DCP_EINVAL);
            CHECK(dcp_gumbel_fit_tail(dense, n, 1, 2, &mu, NULL, &tau, &ke) == DCP_EINVAL);
            CHECK(dcp_gumbel_fit_tail(dense, n, 1, 2, &mu, &lam, NULL, &ke) == DCP_EINVAL);
            CHECK(dcp_gumbel_fit_tail(dense, n, 1, 2, &mu, &lam, &tau, NULL) == DCP_EINVAL);
            CHECK(mu == 5 && lam == 6 && tau == 7 && ke == 8);
            free(x), free(dense), free(sorted);
        }
}

/* a tail fit's arrays go through dcp_hits_evalues as a whole-sample fit's do */
static void evalues(void)
{
    unsigned const n = 200, np = 2, nh = 3;
    double *x = malloc(n * sizeof *x), *mu = malloc(np * sizeof *mu), *lam = malloc(np * sizeof *lam), *e = malloc(nh * sizeof *e);
    uint8_t *st = malloc(np);
    struct dcp_hit *h = malloc(nh * sizeof *h);
    for (unsigned p = 0; p < np; ++p)
    {
        double tau;
        unsigned ke;
        sample(x, n, 1, -4.0 + p, 0.7, 5 + p);
        st[p] = (uint8_t)dcp_gumbel_fit_tail(x, n, 1, 50, &mu[p], &lam[p], &tau, &ke);
        CHECK(st[p] == DCP_FIT_OK && ke >= 50);
    }
    for (unsigned i = 0; i < nh; ++i)
        h[i].seq_idx = i, h[i].profile_idx = i % np, h[i].null_loglik = -100.0f, h[i].alt_loglik = -95.0f + 4.0f * (float)i;
    CHECK(dcp_hits_evalues(h, nh, mu, lam, st, np, 1000.0, e) == DCP_OK);
    for (unsigned i = 0; i < nh; ++i)
        CHECK(e[i] == 1000.0 * dcp_gumbel_sf(mu[i % np], lam[i % np], (double)h[i].alt_loglik - (double)h[i].null_loglik));
    CHECK(e[2] < e[0]);
    free(x), free(mu), free(lam), free(e), free(st), free(h);
}

int main(void)
{
    fit();
    evalues();
    if (failed) return 1;
    puts("asan_calib_tail ok");
    return 0;
}
