/* dcp_posterior_tables and dcp_posterior_envelopes, the host functions of the posterior rows, as a program of its own
 * for ASan + UBSan (tests/test_posterior_pairs.py builds it with csrc/dcp_model.cpp alone: no device code).  Tables and
 * rows are allocated at their exact sizes, so a read or a write one column, one code or one row too far is a finding. */
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

int main(void)
{
    static unsigned const shapes[][3] = {{1, 1, 1}, {1, 4, 9}, {2, 2, 7}, {5, 5, 30}, {5, 9, 30}, {67, 67, 41}, {67, 70, 6}};
    for (unsigned s = 0; s < sizeof shapes / sizeof shapes[0]; ++s)
    {
        unsigned const M = shapes[s][0], ldk = shapes[s][1], L = shapes[s][2];
        struct tables t = make(M, ldk);
        unsigned char *seq = malloc(L);
        double *begin = malloc(sizeof(double) * (L + 1)), *end = malloc(sizeof(double) * (L + 1)),
               *core = malloc(sizeof(double) * (L + 1));
        if (!seq || !begin || !end || !core) return 2;
        for (unsigned i = 0; i < L; ++i)
            seq[i] = (unsigned char)((unsigned)(-draw() * 1000.0) & 3u);
        double xt[DCP_NXTRANS];
        CHECK(dcp_xtrans64(L, (int)(s & 1u), 0, xt) == DCP_OK);
        double fwd = 1.5, bwd = 2.5, nul = 0, alt = 0;
        CHECK(dcp_posterior_tables(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, begin, end, core, &fwd, &bwd) == DCP_OK);
        CHECK(dcp_forward_tables(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, &nul, &alt) == DCP_OK);
        CHECK(isfinite(fwd) && isfinite(bwd) && fwd == alt && fabs(fwd - bwd) <= 1e-9 * (fabs(fwd) + 1.0));
        double nb = 0, ne = 0;
        for (unsigned j = 0; j <= L; ++j)
        {
            CHECK(begin[j] >= 0.0 && end[j] >= 0.0 && core[j] >= -1e-9 && core[j] <= 1.0 + 1e-9);
            nb += begin[j], ne += end[j];
        }
        CHECK(end[0] == 0.0 && core[0] == 0.0 && fabs(nb - ne) <= 1e-9 * (L + 1.0));
        /* envelopes of the row: at exact capacity, at none, one short */
        unsigned n = 0, n2 = 0;
        CHECK(dcp_posterior_envelopes(core, L, 0.5, 1, NULL, NULL, 0, &n) == DCP_OK);
        unsigned *eb = malloc(sizeof(unsigned) * (n ? n : 1)), *ee = malloc(sizeof(unsigned) * (n ? n : 1));
        if (!eb || !ee) return 2;
        CHECK(dcp_posterior_envelopes(core, L, 0.5, 1, eb, ee, n, &n2) == DCP_OK && n2 == n);
        for (unsigned i = 0; i < n; ++i)
            CHECK(eb[i] < ee[i] && ee[i] <= L && (i == 0 || ee[i - 1] < eb[i]));
        if (n) CHECK(dcp_posterior_envelopes(core, L, 0.5, 1, eb, ee, n - 1, &n2) == DCP_OK && n2 == n);
        CHECK(dcp_posterior_envelopes(core, L, -1.0, 1, eb, ee, n ? 1 : 0, &n2) == DCP_OK && n2 == 1); /* all above */
        CHECK(dcp_posterior_envelopes(core, L, 2.0, 1, eb, ee, n, &n2) == DCP_OK && n2 == 0);          /* all below */
        CHECK(dcp_posterior_envelopes(core, L, -1.0, L + 1, eb, ee, n, &n2) == DCP_OK && n2 == 0);     /* min_len */
        CHECK(dcp_posterior_envelopes(core, L, 0.5, 1, eb, ee, n, NULL) == DCP_EINVAL);
        free(eb), free(ee);
        /* refusals write nothing */
        double a = 1.5, b = 2.5;
        begin[0] = end[0] = core[0] = 9.0;
        CHECK(dcp_posterior_tables(0, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, begin, end, core, &a, &b) == DCP_EINVAL);
        CHECK(dcp_posterior_tables(4097, 4097, t.t8, t.em, t.ei, t.en, xt, seq, L, begin, end, core, &a, &b) == DCP_EINVAL);
        CHECK(dcp_posterior_tables(M, M - 1, t.t8, t.em, t.ei, t.en, xt, seq, L, begin, end, core, &a, &b) == DCP_EINVAL);
        CHECK(dcp_posterior_tables(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, 0, begin, end, core, &a, &b) == DCP_EINVAL);
        CHECK(dcp_posterior_tables(M, ldk, NULL, t.em, t.ei, t.en, xt, seq, L, begin, end, core, &a, &b) == DCP_EINVAL);
        CHECK(dcp_posterior_tables(M, ldk, t.t8, t.em, t.ei, t.en, xt, NULL, L, begin, end, core, &a, &b) == DCP_EINVAL);
        CHECK(dcp_posterior_tables(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, NULL, end, core, &a, &b) == DCP_EINVAL);
        CHECK(dcp_posterior_tables(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, begin, end, core, &a, NULL) == DCP_EINVAL);
        seq[L - 1] = 4;
        CHECK(dcp_posterior_tables(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, begin, end, core, &a, &b) == DCP_EINVAL);
        CHECK(a == 1.5 && b == 2.5 && begin[0] == 9.0 && end[0] == 9.0 && core[0] == 9.0);
        free(seq), free(begin), free(end), free(core);
        drop(&t);
    }
    /* all emissions -inf: no path at all, the scores are -inf and the rows 0, never NaN */
    {
        struct tables t = make(3, 3);
        for (unsigned i = 0; i < DCP_NCODES * 3u; ++i)
            t.em[i] = -INFINITY;
        for (unsigned c = 0; c < DCP_NCODES; ++c)
            t.ei[c] = t.en[c] = -INFINITY;
        unsigned char seq[7] = {0, 1, 2, 3, 0, 1, 2};
        double xt[DCP_NXTRANS], fwd = 0, bwd = 0, begin[8], end[8], core[8];
        CHECK(dcp_xtrans64(7, 1, 0, xt) == DCP_OK);
        CHECK(dcp_posterior_tables(3, 3, t.t8, t.em, t.ei, t.en, xt, seq, 7, begin, end, core, &fwd, &bwd) == DCP_OK);
        CHECK(isinf(fwd) && fwd < 0 && isinf(bwd) && bwd < 0);
        for (unsigned j = 0; j < 8; ++j)
            CHECK(begin[j] == 0.0 && end[j] == 0.0 && core[j] == 0.0);
        drop(&t);
    }
    puts("asan_posterior ok");
    return 0;
}
