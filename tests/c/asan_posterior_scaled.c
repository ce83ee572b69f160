/* dcp_posterior_scaled_tables, the host side of the scaled probability-space Backward sweep and posterior rows, as a
 * program of its own for ASan + UBSan (tests/test_posterior_scaled.py builds it with csrc/dcp_model.cpp alone: no device
 * code).  Tables and rows are allocated at their exact sizes, so a read or write one column, code or row too far is a
 * finding.  One ordinary pair per shape, a flagged pair, ET = CT = -705 (row L near the bottom of the range) and the
 * one-node profile. */
#include "dcp_gpu.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static unsigned long long state = 0x9E3779B97F4A7C15ull;
static double draw(void) /* a log-probability-like value in (-6, 0) */
{
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return -6.0 * (double)(state >> 11) / 9007199254740992.0 - 1e-3;
}

struct tables
{
    unsigned M, ldk;
    double *t8, *em, *ei, *en;
};

static struct tables make(unsigned M, unsigned ldk)
{
    struct tables t = {M, ldk, malloc(sizeof(double) * 8 * ldk), malloc(sizeof(double) * DCP_NCODES * ldk),
                       malloc(sizeof(double) * DCP_NCODES), malloc(sizeof(double) * DCP_NCODES)};
    if (!t.t8 || !t.em || !t.ei || !t.en) exit(2);
    for (unsigned r = 0; r < 8; ++r)
        for (unsigned k = 0; k < ldk; ++k)
            t.t8[r * ldk + k] = k < M ? draw() : -INFINITY;
    for (unsigned k = 0; k < ldk; ++k) /* node 0 has no predecessor */
        t.t8[1 * ldk + k] = k ? t.t8[1 * ldk + k] : -INFINITY;
    for (unsigned c = 0; c < DCP_NCODES; ++c)
    {
        for (unsigned k = 0; k < ldk; ++k)
            t.em[c * ldk + k] = k < M ? draw() : -INFINITY;
        t.ei[c] = draw(), t.en[c] = draw();
    }
    return t;
}

static void drop(struct tables *t) { free(t->t8), free(t->em), free(t->ei), free(t->en); }

#define CHECK(x)                                                                                                       \
    do                                                                                                                 \
    {                                                                                                                  \
        if (!(x))                                                                                                      \
        {                                                                                                              \
            fprintf(stderr, "line %d: %s\n", __LINE__, #x);                                                            \
            return 1;                                                                                                  \
        }                                                                                                              \
    } while (0)

struct rows
{
    double *begin, *end, *core;
};

static struct rows rows_of(unsigned L, double fill)
{
    struct rows r = {malloc(sizeof(double) * (L + 1)), malloc(sizeof(double) * (L + 1)), malloc(sizeof(double) * (L + 1))};
    if (!r.begin || !r.end || !r.core) exit(2);
    for (unsigned j = 0; j <= L; ++j)
        r.begin[j] = r.end[j] = r.core[j] = fill;
    return r;
}

static int untouched(struct rows const *r, unsigned L, double fill)
{
    for (unsigned j = 0; j <= L; ++j)
        if (r->begin[j] != fill || r->end[j] != fill || r->core[j] != fill) return 0;
    return 1;
}

static void drop_rows(struct rows *r) { free(r->begin), free(r->end), free(r->core); }

/* the scaled rows against dcp_posterior_tables' within tol */
static int rows_agree(struct tables const *t, double const *xt, unsigned char const *seq, unsigned L, int f32, int band, double tol)
{
    struct rows want = rows_of(L, 0.0), got = rows_of(L, 1.5);
    double wf = 0, wb = 0, gf = 1.5, gb = 2.5;
    int oor = 7, ok = 1;
    ok = ok && dcp_posterior_tables(t->M, t->ldk, t->t8, t->em, t->ei, t->en, xt, seq, L, want.begin, want.end, want.core, &wf, &wb) == DCP_OK;
    ok = ok && dcp_posterior_scaled_tables_band(t->M, t->ldk, t->t8, t->em, t->ei, t->en, xt, seq, L, f32, band, got.begin, got.end,
                                                got.core, &gf, &gb, &oor) == DCP_OK;
    ok = ok && oor == 0 && isfinite(gf) && isfinite(gb) && fabs(gf - wf) <= tol && fabs(gb - wb) <= tol;
    for (unsigned j = 0; ok && j <= L; ++j)
        ok = fabs(got.begin[j] - want.begin[j]) <= 3 * tol && fabs(got.end[j] - want.end[j]) <= 3 * tol &&
             fabs(got.core[j] - want.core[j]) <= 3 * tol;
    ok = ok && got.core[0] == 0.0 && got.end[0] == 0.0;
    drop_rows(&want), drop_rows(&got);
    return ok;
}

int main(void)
{
    static unsigned const shapes[][3] = {{1, 1, 1}, {1, 4, 9}, {2, 2, 7}, {5, 5, 5}, {5, 9, 6}, {67, 67, 41}, {67, 70, 6}, {3, 3, 900}};
    for (unsigned s = 0; s < sizeof shapes / sizeof shapes[0]; ++s)
    {
        unsigned const M = shapes[s][0], ldk = shapes[s][1], L = shapes[s][2];
        struct tables t = make(M, ldk);
        unsigned char *seq = malloc(L);
        if (!seq) return 2;
        for (unsigned i = 0; i < L; ++i)
            seq[i] = (unsigned char)((unsigned)(-draw() * 1000.0) & 3u);
        double xt[DCP_NXTRANS];
        CHECK(dcp_xtrans64(L, (int)(s & 1u), 0, xt) == DCP_OK);
        double ref_nul = 0, ref_alt = 0;
        CHECK(dcp_forward_tables(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, &ref_nul, &ref_alt) == DCP_OK);
        for (int f32 = 0; f32 < 2; ++f32)
            for (int band = 3; band <= 64; band += 61)
            {
                double const tol = f32 ? 2e-7 * ((double)L * (M + 2) + 2) : 2.4e-10 * (fabs(ref_alt) + 1.0);
                CHECK(rows_agree(&t, xt, seq, L, f32, band, tol));
            }
        /* alt_fwd has the scaled Forward twin's bits */
        {
            struct rows r = rows_of(L, 1.5);
            double nul = 0, alt = 0, gf = 0, gb = 0;
            int oor = 7;
            CHECK(dcp_forward_scaled_tables(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, 0, &nul, &alt, &oor) == DCP_OK && oor == 0);
            CHECK(dcp_posterior_scaled_tables(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, 0, r.begin, r.end, r.core, &gf, &gb, &oor) == DCP_OK);
            CHECK(oor == 0 && memcmp(&gf, &alt, sizeof gf) == 0);
            drop_rows(&r);
        }
        /* refusals write nothing */
        struct rows r = rows_of(L, 1.5);
        double a = 1.5, b = 2.5;
        int o = 7;
        CHECK(dcp_posterior_scaled_tables(0, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, 0, r.begin, r.end, r.core, &a, &b, &o) == DCP_EINVAL);
        CHECK(dcp_posterior_scaled_tables(M, M - 1, t.t8, t.em, t.ei, t.en, xt, seq, L, 0, r.begin, r.end, r.core, &a, &b, &o) == DCP_EINVAL);
        CHECK(dcp_posterior_scaled_tables(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, 0, 0, r.begin, r.end, r.core, &a, &b, &o) == DCP_EINVAL);
        CHECK(dcp_posterior_scaled_tables(M, ldk, NULL, t.em, t.ei, t.en, xt, seq, L, 0, r.begin, r.end, r.core, &a, &b, &o) == DCP_EINVAL);
        CHECK(dcp_posterior_scaled_tables(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, 0, NULL, r.end, r.core, &a, &b, &o) == DCP_EINVAL);
        CHECK(dcp_posterior_scaled_tables(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, 0, r.begin, r.end, r.core, &a, &b, NULL) == DCP_EINVAL);
        CHECK(dcp_posterior_scaled_tables_band(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, 0, 501, r.begin, r.end, r.core, &a, &b, &o) == DCP_EINVAL);
        seq[L - 1] = 4;
        CHECK(dcp_posterior_scaled_tables(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, 0, r.begin, r.end, r.core, &a, &b, &o) == DCP_EINVAL);
        CHECK(a == 1.5 && b == 2.5 && o == 7 && untouched(&r, L, 1.5));
        drop_rows(&r);
        free(seq);
        drop(&t);
    }
    /* a delete chain that multiplies up past the double range: flagged, nothing written */
    {
        unsigned const M = 2000, L = 6;
        struct tables t = make(M, M);
        for (unsigned k = 1; k < M; ++k)
            t.t8[4 * M + k] = 0.7, t.t8[5 * M + k] = 0.4; /* MD, DD */
        unsigned char seq[6] = {0, 1, 2, 3, 0, 1};
        double xt[DCP_NXTRANS], a = 1.5, b = 2.5;
        int oor = 0;
        struct rows r = rows_of(L, 1.5);
        CHECK(dcp_xtrans64(L, 1, 0, xt) == DCP_OK);
        CHECK(dcp_posterior_scaled_tables(M, M, t.t8, t.em, t.ei, t.en, xt, seq, L, 0, r.begin, r.end, r.core, &a, &b, &oor) == DCP_OK);
        CHECK(oor == 1 && a == 1.5 && b == 2.5 && untouched(&r, L, 1.5));
        CHECK(dcp_posterior_tables(M, M, t.t8, t.em, t.ei, t.en, xt, seq, L, r.begin, r.end, r.core, &a, &b) == DCP_OK);
        CHECK(isfinite(a) && isfinite(b));
        drop_rows(&r);
        drop(&t);
    }
    /* ET = CT = -705: row L is a row, and its rescaling keeps rows L and L - 1 out of the subnormals */
    {
        enum { X_ET = 5, X_CT = 8 };
        unsigned const M = 5, L = 12;
        struct tables t = make(M, M);
        unsigned char seq[12];
        for (unsigned i = 0; i < L; ++i)
            seq[i] = (unsigned char)((unsigned)(-draw() * 1000.0) & 3u);
        double xt[DCP_NXTRANS], ref_nul = 0, ref_alt = 0;
        CHECK(dcp_xtrans64(L, 1, 0, xt) == DCP_OK);
        xt[X_ET] = xt[X_CT] = -705.0;
        CHECK(dcp_forward_tables(M, M, t.t8, t.em, t.ei, t.en, xt, seq, L, &ref_nul, &ref_alt) == DCP_OK);
        for (int f32 = 0; f32 < 2; ++f32)
            for (int band = 4; band <= 64; band += 60)
                CHECK(rows_agree(&t, xt, seq, L, f32, band, f32 ? 2e-7 * ((double)L * (M + 2) + 2) : 2.4e-10 * (fabs(ref_alt) + 1.0)));
        drop(&t);
    }
    puts("asan_posterior_scaled ok");
    return 0;
}
