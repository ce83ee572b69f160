/* dcp_mea_tables and dcp_mea_path_gain, the host functions of the posterior-decoded alignment, as a program of its own
 * for ASan + UBSan (tests/test_mea_pairs.py builds it with csrc/dcp_model.cpp alone: no device code).  Tables, steps and
 * posteriors are allocated at their exact sizes, so a read or a write one column, one code, one row or one step too far
 * is a finding. */
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
        /* the count first, with no arrays at all; then at the exact capacity; then one short */
        unsigned n = 0, n2 = 0;
        double gain = 1.5, fwd = 2.5, nul = 0, alt = 0;
        CHECK(dcp_mea_tables(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, NULL, 0, &n, NULL, &gain, &fwd) == DCP_ENOMEM);
        CHECK(n >= 5 && gain == 1.5 && fwd == 2.5);
        struct dcp_step *steps = malloc(sizeof(struct dcp_step) * n);
        double *post = malloc(sizeof(double) * n), *post2 = malloc(sizeof(double) * n);
        if (!steps || !post || !post2) return 2;
        CHECK(dcp_mea_tables(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, steps, n, &n2, post, &gain, &fwd) == DCP_OK && n2 == n);
        CHECK(dcp_forward_tables(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, &nul, &alt) == DCP_OK && fwd == alt);
        CHECK(gain >= 0.0 && gain <= L * (1.0 + 1e-9));
        unsigned emitted = 0;
        for (unsigned i = 0; i < n; ++i)
        {
            emitted += steps[i].seqlen;
            CHECK(steps[i].seqlen ? post[i] >= 0.0 && post[i] <= 1.0 + 1e-9 : post[i] == -1.0);
        }
        CHECK(emitted == L);
        double g2 = 0;
        CHECK(dcp_mea_path_gain(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, steps, n, &g2, post2) == DCP_OK);
        CHECK(g2 == gain && memcmp(post, post2, sizeof(double) * n) == 0);
        CHECK(dcp_mea_path_gain(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, steps, n, &g2, NULL) == DCP_OK && g2 == gain);
        steps[0].state_id = 0xffff, post[0] = 9.0, gain = 1.5;
        CHECK(dcp_mea_tables(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, steps, n - 1, &n2, post, &gain, &fwd) == DCP_ENOMEM);
        CHECK(n2 == n && steps[0].state_id == 0xffff && post[0] == 9.0 && gain == 1.5);
        /* refusals write nothing */
        n2 = 77;
        CHECK(dcp_mea_tables(0, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, steps, n, &n2, post, &gain, &fwd) == DCP_EINVAL);
        CHECK(dcp_mea_tables(M, M - 1, t.t8, t.em, t.ei, t.en, xt, seq, L, steps, n, &n2, post, &gain, &fwd) == DCP_EINVAL);
        CHECK(dcp_mea_tables(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, 0, steps, n, &n2, post, &gain, &fwd) == DCP_EINVAL);
        CHECK(dcp_mea_tables(M, ldk, t.t8, NULL, t.ei, t.en, xt, seq, L, steps, n, &n2, post, &gain, &fwd) == DCP_EINVAL);
        CHECK(dcp_mea_tables(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, NULL, n, &n2, post, &gain, &fwd) == DCP_EINVAL);
        CHECK(dcp_mea_tables(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, steps, n, NULL, post, &gain, &fwd) == DCP_EINVAL);
        CHECK(dcp_mea_tables(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, steps, n, &n2, post, NULL, &fwd) == DCP_EINVAL);
        CHECK(n2 == 77 && steps[0].state_id == 0xffff && post[0] == 9.0 && gain == 1.5);
        g2 = 3.5, post2[0] = 9.0;
        CHECK(dcp_mea_path_gain(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, steps, n, &g2, post2) == DCP_EINVAL); /* not S */
        CHECK(dcp_mea_path_gain(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, NULL, n, &g2, post2) == DCP_EINVAL);
        CHECK(dcp_mea_path_gain(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, steps, 0, &g2, post2) == DCP_EINVAL);
        CHECK(g2 == 3.5 && post2[0] == 9.0);
        free(steps), free(post), free(post2), free(seq);
        drop(&t);
    }
    /* all emissions -inf: no path at all -- zero steps, gain -inf, no error */
    {
        struct tables t = make(3, 3);
        for (unsigned i = 0; i < DCP_NCODES * 3u; ++i)
            t.em[i] = -INFINITY;
        for (unsigned c = 0; c < DCP_NCODES; ++c)
            t.ei[c] = t.en[c] = -INFINITY;
        unsigned char seq[7] = {0, 1, 2, 3, 0, 1, 2};
        double xt[DCP_NXTRANS], fwd = 0, gain = 0;
        unsigned n = 9;
        CHECK(dcp_xtrans64(7, 1, 0, xt) == DCP_OK);
        CHECK(dcp_mea_tables(3, 3, t.t8, t.em, t.ei, t.en, xt, seq, 7, NULL, 0, &n, NULL, &gain, &fwd) == DCP_OK);
        CHECK(n == 0 && isinf(fwd) && fwd < 0 && isinf(gain) && gain < 0);
        drop(&t);
    }
    puts("asan_mea ok");
    return 0;
}
