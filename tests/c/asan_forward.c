/* dcp_forward_tables, the host twin of the Forward kernel, as a program of its own for ASan + UBSan
 * (tests/test_forward_pairs.py builds it with csrc/dcp_model.cpp alone: no device code).  Tables are allocated at
 * their exact sizes, so a read one column or one code too far is a finding. */
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
        if (!seq) return 2;
        for (unsigned i = 0; i < L; ++i)
            seq[i] = (unsigned char)((unsigned)(-draw() * 1000.0) & 3u);
        double xt[DCP_NXTRANS];
        CHECK(dcp_xtrans64(L, (int)(s & 1u), 0, xt) == DCP_OK);
        double nul = 1.5, alt = 2.5;
        CHECK(dcp_forward_tables(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, &nul, &alt) == DCP_OK);
        CHECK(isfinite(nul) && isfinite(alt) && nul < 0.0);
        /* refusals write nothing */
        double a = 1.5, b = 2.5;
        CHECK(dcp_forward_tables(0, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, &a, &b) == DCP_EINVAL);
        CHECK(dcp_forward_tables(4097, 4097, t.t8, t.em, t.ei, t.en, xt, seq, L, &a, &b) == DCP_EINVAL);
        CHECK(dcp_forward_tables(M, M - 1, t.t8, t.em, t.ei, t.en, xt, seq, L, &a, &b) == DCP_EINVAL);
        CHECK(dcp_forward_tables(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, 0, &a, &b) == DCP_EINVAL);
        CHECK(dcp_forward_tables(M, ldk, NULL, t.em, t.ei, t.en, xt, seq, L, &a, &b) == DCP_EINVAL);
        CHECK(dcp_forward_tables(M, ldk, t.t8, t.em, t.ei, t.en, xt, NULL, L, &a, &b) == DCP_EINVAL);
        CHECK(dcp_forward_tables(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, NULL, &b) == DCP_EINVAL);
        seq[L - 1] = 4;
        CHECK(dcp_forward_tables(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, &a, &b) == DCP_EINVAL);
        CHECK(a == 1.5 && b == 2.5);
        free(seq);
        drop(&t);
    }
    /* all emissions -inf: every sum is empty, the scores are -inf, never NaN */
    {
        struct tables t = make(3, 3);
        for (unsigned i = 0; i < DCP_NCODES * 3u; ++i)
            t.em[i] = -INFINITY;
        for (unsigned c = 0; c < DCP_NCODES; ++c)
            t.ei[c] = t.en[c] = -INFINITY;
        unsigned char seq[7] = {0, 1, 2, 3, 0, 1, 2};
        double xt[DCP_NXTRANS], nul = 0, alt = 0;
        CHECK(dcp_xtrans64(7, 1, 0, xt) == DCP_OK);
        CHECK(dcp_forward_tables(3, 3, t.t8, t.em, t.ei, t.en, xt, seq, 7, &nul, &alt) == DCP_OK);
        CHECK(isinf(nul) && nul < 0 && isinf(alt) && alt < 0);
        drop(&t);
    }
    puts("asan_forward ok");
    return 0;
}
