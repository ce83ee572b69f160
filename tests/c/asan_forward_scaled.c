/* dcp_forward_scaled_tables and dcp_fwd_factor_f32, the host side of the scaled probability-space Forward sweep, as a
 * program of its own for ASan + UBSan (tests/test_forward_scaled.py builds it with csrc/dcp_model.cpp alone: no device
 * code).  Tables are allocated at their exact sizes, so a read one column or one code too far is a finding.  Special
 * transitions at both ends of the range: the exits of row 1, of the finish and of R alone, and rows 0 and 1 near e^-708. */
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
    /* the factor rule at its ends and beyond them */
    CHECK(dcp_fwd_factor_f32(-INFINITY) == 0.0 && dcp_fwd_factor_f32(-709.0f) == 0.0 && dcp_fwd_factor_f32(-3.0e38f) == 0.0);
    CHECK(dcp_fwd_factor_f32(0.0f) == 1.0 && dcp_fwd_factor_f32(-0.0f) == 1.0);
    CHECK(dcp_fwd_factor_f32(-708.0f) > 0.0 && isfinite(dcp_fwd_factor_f32(708.0f)) && isinf(dcp_fwd_factor_f32(3.0e38f)));
    CHECK(dcp_fwd_factor_f32(NAN) == 0.0);
    for (float t = -708.0f; t <= 708.0f; t += 0.37f)
        CHECK(fabs(dcp_fwd_factor_f32(t) / exp((double)t) - 1.0) < 1.2e-7);

    static unsigned const shapes[][3] = {{1, 1, 1}, {1, 4, 9}, {2, 2, 7}, {5, 5, 30}, {5, 9, 30}, {67, 67, 41}, {67, 70, 6}, {3, 3, 900}};
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
        {
            double nul = 1.5, alt = 2.5;
            int oor = 7;
            CHECK(dcp_forward_scaled_tables(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, f32, &nul, &alt, &oor) == DCP_OK);
            CHECK(oor == 0 && isfinite(nul) && isfinite(alt) && nul < 0.0);
            double const tol = f32 ? 1e-7 * ((double)L * (M + 2) + 2) : 2.4e-10 * (fabs(ref_alt) + 1.0);
            CHECK(fabs(nul - ref_nul) <= tol && fabs(alt - ref_alt) <= tol);
            double n4 = 0, a4 = 0;
            CHECK(dcp_forward_scaled_tables_band(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, f32, 3, &n4, &a4, &oor) == DCP_OK);
            CHECK(oor == 0 && n4 == nul && a4 == alt); /* the band changes no bit */
        }
        /* refusals write nothing */
        double a = 1.5, b = 2.5;
        int o = 7;
        CHECK(dcp_forward_scaled_tables(0, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, 0, &a, &b, &o) == DCP_EINVAL);
        CHECK(dcp_forward_scaled_tables(4097, 4097, t.t8, t.em, t.ei, t.en, xt, seq, L, 0, &a, &b, &o) == DCP_EINVAL);
        CHECK(dcp_forward_scaled_tables(M, M - 1, t.t8, t.em, t.ei, t.en, xt, seq, L, 0, &a, &b, &o) == DCP_EINVAL);
        CHECK(dcp_forward_scaled_tables(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, 0, 0, &a, &b, &o) == DCP_EINVAL);
        CHECK(dcp_forward_scaled_tables(M, ldk, NULL, t.em, t.ei, t.en, xt, seq, L, 0, &a, &b, &o) == DCP_EINVAL);
        CHECK(dcp_forward_scaled_tables(M, ldk, t.t8, t.em, t.ei, t.en, xt, NULL, L, 0, &a, &b, &o) == DCP_EINVAL);
        CHECK(dcp_forward_scaled_tables(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, 0, NULL, &b, &o) == DCP_EINVAL);
        CHECK(dcp_forward_scaled_tables(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, 0, &a, &b, NULL) == DCP_EINVAL);
        CHECK(dcp_forward_scaled_tables_band(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, 0, 0, &a, &b, &o) == DCP_EINVAL);
        seq[L - 1] = 4;
        CHECK(dcp_forward_scaled_tables(M, ldk, t.t8, t.em, t.ei, t.en, xt, seq, L, 0, &a, &b, &o) == DCP_EINVAL);
        CHECK(a == 1.5 && b == 2.5 && o == 7);
        free(seq);
        drop(&t);
    }
    /* all emissions -inf: every sum is empty, the scores are -inf, never NaN, and nothing is out of range */
    {
        struct tables t = make(3, 3);
        for (unsigned i = 0; i < DCP_NCODES * 3u; ++i)
            t.em[i] = -INFINITY;
        for (unsigned c = 0; c < DCP_NCODES; ++c)
            t.ei[c] = t.en[c] = -INFINITY;
        unsigned char seq[7] = {0, 1, 2, 3, 0, 1, 2};
        double xt[DCP_NXTRANS], nul = 0, alt = 0;
        int oor = 7;
        CHECK(dcp_xtrans64(7, 1, 0, xt) == DCP_OK);
        CHECK(dcp_forward_scaled_tables(3, 3, t.t8, t.em, t.ei, t.en, xt, seq, 7, 1, &nul, &alt, &oor) == DCP_OK);
        CHECK(oor == 0 && isinf(nul) && nul < 0 && isinf(alt) && alt < 0);
        drop(&t);
    }
    /* a delete chain that multiplies up past the double range: flagged, nothing written */
    {
        unsigned const M = 2000;
        struct tables t = make(M, M);
        for (unsigned k = 1; k < M; ++k)
            t.t8[4 * M + k] = 0.7, t.t8[5 * M + k] = 0.4; /* MD, DD */
        unsigned char seq[6] = {0, 1, 2, 3, 0, 1};
        double xt[DCP_NXTRANS], nul = 1.5, alt = 2.5;
        int oor = 0;
        CHECK(dcp_xtrans64(6, 1, 0, xt) == DCP_OK);
        CHECK(dcp_forward_scaled_tables(M, M, t.t8, t.em, t.ei, t.en, xt, seq, 6, 0, &nul, &alt, &oor) == DCP_OK);
        CHECK(oor == 1 && nul == 1.5 && alt == 2.5);
        CHECK(dcp_forward_tables(M, M, t.t8, t.em, t.ei, t.en, xt, seq, 6, &nul, &alt) == DCP_OK);
        CHECK(isfinite(nul) && isfinite(alt));
        drop(&t);
    }
    /* special transitions at the ends of the range (xtrans order: RR, SB, SN, NN, NB, ET, EC, CC, CT, EB, EJ, JJ, JB): an exit
     * in row 1, one at the finish, rows 0 and 1 near the bottom of the range, and R alone on the one-node profile.  A flagged
     * pair writes nothing, at either band and by either factor rule */
    {
        enum { X_RR = 0, X_SB = 1, X_SN = 2, X_NB = 4, X_ET = 5, X_CT = 8 };
        static struct
        {
            unsigned M, L;
            int which[2];
            double value;
            int oor;
        } const cases[] = {{5, 12, {X_NB, X_NB}, 710.0, 1}, {67, 7, {X_ET, X_CT}, 710.0, 1}, {5, 12, {X_SB, X_SN}, -705.0, 0}, {1, 3, {X_RR, X_RR}, 710.0, 1}};
        for (unsigned s = 0; s < sizeof cases / sizeof cases[0]; ++s)
        {
            unsigned const M = cases[s].M, L = cases[s].L;
            struct tables t = make(M, M);
            unsigned char seq[12];
            for (unsigned i = 0; i < L; ++i)
                seq[i] = (unsigned char)((unsigned)(-draw() * 1000.0) & 3u);
            double xt[DCP_NXTRANS], ref_nul = 0, ref_alt = 0;
            CHECK(dcp_xtrans64(L, 1, 0, xt) == DCP_OK);
            xt[cases[s].which[0]] = xt[cases[s].which[1]] = cases[s].value;
            CHECK(dcp_forward_tables(M, M, t.t8, t.em, t.ei, t.en, xt, seq, L, &ref_nul, &ref_alt) == DCP_OK);
            CHECK(isfinite(ref_nul) && isfinite(ref_alt));
            for (int f32 = 0; f32 < 2; ++f32)
                for (int band = 4; band <= 64; band += 60)
                {
                    double nul = 1.5, alt = 2.5;
                    int oor = 7;
                    CHECK(dcp_forward_scaled_tables_band(M, M, t.t8, t.em, t.ei, t.en, xt, seq, L, f32, band, &nul, &alt, &oor) == DCP_OK);
                    CHECK(oor == cases[s].oor);
                    if (oor)
                    {
                        CHECK(nul == 1.5 && alt == 2.5);
                        continue;
                    }
                    double const tol = f32 ? 1e-7 * ((double)L * (M + 2) + 2) : 2.4e-10 * (fabs(ref_alt) + 1.0);
                    CHECK(fabs(nul - ref_nul) <= tol && fabs(alt - ref_alt) <= tol);
                }
            drop(&t);
        }
    }
    puts("asan_forward_scaled ok");
    return 0;
}
