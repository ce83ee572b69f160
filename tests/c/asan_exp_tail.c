/*
 * The exponential tail fit's host functions (include/dcp_gpu.h: dcp_exp_tail_fit, dcp_exp_sf, dcp_scores_evalues) under
 * ASan + UBSan: a stand-alone CPU program, linked with csrc/dcp_model.cpp alone.  Every array lives on the heap at
 * exactly the size the call is told; tau and k_eff are checked against a sort and against dcp_gumbel_fit_tail's, lambda
 * against the rule's own sum, the statuses, the strides; the refusals write nothing.
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

/* shift + an exponential(lambda) sample, rounded to 64ths so that values tie now and then */
static void sample(double *x, unsigned n, size_t stride, double shift, double lambda, uint64_t seed)
{
    for (unsigned i = 0; i < n; ++i)
    {
        double const u = ((double)(sm(seed + i) >> 11) + 0.5) / 9007199254740992.0;
        x[i * stride] = floor(64.0 * (shift - log(u) / lambda)) / 64.0;
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
                double mu = 5, lam = 6, tau = 7, mu1 = 5, lam1 = 6, tau1 = 7, gmu, glam, gtau, so = 0.0;
                unsigned ke = 8, ke1 = 8, gke, want = 0;
                int const st = dcp_exp_tail_fit(x, n, stride, k, &mu, &lam, &tau, &ke);
                int const st1 = dcp_exp_tail_fit(dense, n, 1, k, &mu1, &lam1, &tau1, &ke1);
                for (unsigned i = 0; i < n; ++i)
                    if (dense[i] >= sorted[k - 1]) ++want, so += dense[i] - sorted[k - 1];
                CHECK(st == st1 && (st == DCP_FIT_OK || st == DCP_FIT_FLAT));
                CHECK((st == DCP_FIT_FLAT) == (so == 0.0));
                CHECK(tau == sorted[k - 1] && tau1 == tau && ke == want && ke1 == want && ke >= k);
                (void)dcp_gumbel_fit_tail(dense, n, 1, k, &gmu, &glam, &gtau, &gke); /* the same selection */
                CHECK(gtau == tau && gke == ke);
                if (st == DCP_FIT_OK)
                {
                    CHECK(mu == mu1 && lam == lam1 && lam == (double)ke / so && mu <= tau);
                    CHECK(fabs(dcp_exp_sf(mu, lam, tau) * n / ke - 1.0) < 1e-12);
                    if (k == n) CHECK(mu == tau && tau == sorted[n - 1]);
                }
                else CHECK(isnan(mu) && isnan(lam) && isnan(mu1) && isnan(lam1));
                /* five standard errors of the estimator, lambda / sqrt(k) */
                if (n >= 64 && k >= n / 4 && k < n) CHECK(st == DCP_FIT_OK && fabs(lam - 0.7) < 5.0 * 0.7 / sqrt((double)k));
            }
            /* statuses */
            double mu = 5, lam = 6, tau = 7;
            unsigned ke = 8;
            for (unsigned i = 0; i < n; ++i)
                dense[i] = 2.5;
            CHECK(dcp_exp_tail_fit(dense, n, 1, 2, &mu, &lam, &tau, &ke) == DCP_FIT_FLAT && isnan(mu) && isnan(lam));
            CHECK(tau == 2.5 && ke == n);
            if (n >= 3)
            { /* the whole tail at one value, a bulk below it */
                dense[0] = 1.0;
                CHECK(dcp_exp_tail_fit(dense, n, 1, 2, &mu, &lam, &tau, &ke) == DCP_FIT_FLAT && isnan(mu) && isnan(lam));
                CHECK(tau == 2.5 && ke == n - 1);
            }
            sample(dense, n, 1, 0.0, 1.0, 77);
            dense[n - 1] = -INFINITY;
            CHECK(dcp_exp_tail_fit(dense, n, 1, 2, &mu, &lam, &tau, &ke) == DCP_FIT_NONFINITE);
            CHECK(isnan(mu) && isnan(lam) && isnan(tau) && ke == 0);
            dense[n - 1] = 0.0, dense[0] = INFINITY;
            CHECK(dcp_exp_tail_fit(dense, n, 1, n, &mu, &lam, &tau, &ke) == DCP_FIT_NONFINITE && ke == 0);
            dense[0] = NAN;
            CHECK(dcp_exp_tail_fit(dense, n, 1, 2, &mu, &lam, &tau, &ke) == DCP_FIT_NONFINITE && isnan(tau));
            /* the refusals */
            dense[0] = 1.0;
            mu = 5, lam = 6, tau = 7, ke = 8;
            CHECK(dcp_exp_tail_fit(dense, n, 1, 0, &mu, &lam, &tau, &ke) == DCP_EINVAL);
            CHECK(dcp_exp_tail_fit(dense, n, 1, 1, &mu, &lam, &tau, &ke) == DCP_EINVAL);
            CHECK(dcp_exp_tail_fit(dense, n, 1, n + 1, &mu, &lam, &tau, &ke) == DCP_EINVAL);
            CHECK(dcp_exp_tail_fit(dense, 1, 1, 2, &mu, &lam, &tau, &ke) == DCP_EINVAL);
            CHECK(dcp_exp_tail_fit(dense, 0, 1, 2, &mu, &lam, &tau, &ke) == DCP_EINVAL);
            CHECK(dcp_exp_tail_fit(NULL, n, 1, 2, &mu, &lam, &tau, &ke) == DCP_EINVAL);
            CHECK(dcp_exp_tail_fit(dense, n, 0, 2, &mu, &lam, &tau, &ke) == DCP_EINVAL);
            CHECK(dcp_exp_tail_fit(dense, n, 1, 2, NULL, &lam, &tau, &ke) == DCP_EINVAL);
            CHECK(dcp_exp_tail_fit(dense, n, 1, 2, &mu, NULL, &tau, &ke) == DCP_EINVAL);
            CHECK(dcp_exp_tail_fit(dense, n, 1, 2, &mu, &lam, NULL, &ke) == DCP_EINVAL);
            CHECK(dcp_exp_tail_fit(dense, n, 1, 2, &mu, &lam, &tau, NULL) == DCP_EINVAL);
            CHECK(mu == 5 && lam == 6 && tau == 7 && ke == 8);
            free(x), free(dense), free(sorted);
        }
}

/* score arrays through dcp_scores_evalues under both laws */
static void evalues(void)
{
    unsigned const n = 200, np = 3, ns = 4;
    double *x = malloc(n * sizeof *x), *mu = malloc(np * sizeof *mu), *lam = malloc(np * sizeof *lam), *e = malloc(ns * sizeof *e);
    double *nl = malloc(ns * sizeof *nl), *al = malloc(ns * sizeof *al);
    uint8_t *st = malloc(np);
    uint32_t *pi = malloc(ns * sizeof *pi);
    for (unsigned p = 0; p < np; ++p)
    {
        double tau;
        unsigned ke;
        sample(x, n, 1, -4.0 + p, 0.7, 5 + p);
        st[p] = (uint8_t)dcp_exp_tail_fit(x, n, 1, 50, &mu[p], &lam[p], &tau, &ke);
        CHECK(st[p] == DCP_FIT_OK && ke >= 50);
    }
    st[2] = DCP_FIT_FLAT;
    for (unsigned i = 0; i < ns; ++i)
        pi[i] = i % np, nl[i] = -100.0, al[i] = -108.0 + 6.0 * (double)i;
    for (int law = DCP_LAW_GUMBEL; law <= DCP_LAW_EXP; ++law)
    {
        CHECK(dcp_scores_evalues(pi, nl, al, ns, mu, lam, st, np, 1000.0, law, e) == DCP_OK);
        for (unsigned i = 0; i < ns; ++i)
        {
            double const s = al[i] - nl[i], m = mu[i % np], l = lam[i % np];
            if (i % np == 2) CHECK(isnan(e[i]));
            else CHECK(e[i] == 1000.0 * (law == DCP_LAW_EXP ? dcp_exp_sf(m, l, s) : dcp_gumbel_sf(m, l, s)));
        }
        CHECK(e[3] < e[0]);
    }
    CHECK(dcp_exp_sf(1.0, 0.5, 1.0) == 1.0 && dcp_exp_sf(1.0, 0.5, -INFINITY) == 1.0 && dcp_exp_sf(1.0, 0.5, 3.0) == exp(-1.0));
    for (unsigned i = 0; i < ns; ++i)
        e[i] = 9.0;
    CHECK(dcp_scores_evalues(pi, nl, al, ns, mu, lam, st, 2, 1000.0, DCP_LAW_EXP, e) == DCP_EINVAL); /* profile 2 >= 2 */
    CHECK(dcp_scores_evalues(pi, nl, al, ns, mu, lam, st, np, -1.0, DCP_LAW_EXP, e) == DCP_EINVAL);
    CHECK(dcp_scores_evalues(pi, nl, al, ns, mu, lam, st, np, NAN, DCP_LAW_EXP, e) == DCP_EINVAL);
    CHECK(dcp_scores_evalues(pi, nl, al, ns, mu, lam, st, np, 1000.0, 2, e) == DCP_EINVAL);
    CHECK(dcp_scores_evalues(NULL, nl, al, ns, mu, lam, st, np, 1000.0, DCP_LAW_EXP, e) == DCP_EINVAL);
    CHECK(dcp_scores_evalues(pi, nl, al, ns, mu, lam, st, np, 1000.0, DCP_LAW_EXP, NULL) == DCP_EINVAL);
    CHECK(dcp_scores_evalues(NULL, NULL, NULL, 0, NULL, NULL, NULL, 0, 1000.0, DCP_LAW_EXP, NULL) == DCP_OK);
    for (unsigned i = 0; i < ns; ++i)
        CHECK(e[i] == 9.0);
    free(x), free(mu), free(lam), free(e), free(nl), free(al), free(st), free(pi);
}

int main(void)
{
    fit();
    evalues();
    if (failed) return 1;
    puts("asan_exp_tail ok");
    return 0;
}
