/* dcp_posterior_envelope_records and dcp_envelopes_regions, the host functions of the posterior envelopes, as a program of
 * its own for ASan + UBSan (tests/test_envelopes.py builds it with csrc/dcp_model.cpp alone: no device code).  Rows,
 * records and region arrays are allocated at their exact sizes, so a read or a write one row or one record too far is a
 * finding. */
#include "dcp_gpu.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static unsigned long long state = 0x9E3779B97F4A7C15ull;
static double draw(void) /* in [0, 1) */
{
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(state >> 11) / 9007199254740992.0;
}

#define CHECK(x)                                                                                                       \
    do                                                                                                                 \
    {                                                                                                                  \
        if (!(x))                                                                                                      \
        {                                                                                                              \
            fprintf(stderr, "line %d: %s\n", __LINE__, #x);                                                            \
            return 1;                                                                                                  \
        }                                                                                                              \
    } while (0)

/* the runs of one thresholds pair, counted without the function under test */
static unsigned count_runs(double const *core, unsigned L, double hi, double lo, unsigned min_len)
{
    unsigned n = 0;
    for (unsigned i = 0; i < L;)
    {
        if (!(core[i + 1] >= lo))
        {
            ++i;
            continue;
        }
        unsigned e = i;
        double mx = core[i + 1];
        for (; e < L && core[e + 1] >= lo; ++e)
            if (core[e + 1] > mx) mx = core[e + 1];
        if (e - i >= min_len && mx >= hi) ++n;
        i = e;
    }
    return n;
}

int main(void)
{
    static unsigned const lens[] = {1, 2, 63, 64, 65, 200};
    static double const thr[][2] = {{0.5, 0.5}, {0.5, 0.1}, {0.9, 0.3}, {0.0, 0.0}, {2.0, -1.0}, {-1.0, -1.0}};
    for (unsigned s = 0; s < sizeof lens / sizeof lens[0]; ++s)
    {
        unsigned const L = lens[s];
        double *begin = malloc(sizeof(double) * (L + 1)), *end = malloc(sizeof(double) * (L + 1)),
               *core = malloc(sizeof(double) * (L + 1));
        if (!begin || !end || !core) return 2;
        for (unsigned j = 0; j <= L; ++j)
            begin[j] = draw() * 0.1, end[j] = j ? draw() * 0.1 : 0.0, core[j] = j ? draw() : 0.0;
        for (unsigned t = 0; t < sizeof thr / sizeof thr[0]; ++t)
            for (unsigned min_len = 0; min_len <= 3; ++min_len)
            {
                double const hi = thr[t][0], lo = thr[t][1];
                unsigned n = 77, n2 = 77;
                CHECK(dcp_posterior_envelope_records(begin, end, core, L, hi, lo, min_len, NULL, 0, &n) == DCP_OK);
                CHECK(n == count_runs(core, L, hi, lo, min_len));
                struct dcp_envelope *out = malloc(sizeof *out * (n ? n : 1));
                if (!out) return 2;
                CHECK(dcp_posterior_envelope_records(begin, end, core, L, hi, lo, min_len, out, n, &n2) == DCP_OK && n2 == n);
                for (unsigned k = 0; k < n; ++k)
                {
                    struct dcp_envelope const *v = out + k;
                    CHECK(v->pair == 0 && v->begin < v->end && v->end <= L && v->begin <= v->peak && v->peak < v->end);
                    CHECK(v->end - v->begin >= min_len && v->core_max >= hi && v->core_max == core[v->peak + 1]);
                    CHECK(k == 0 || out[k - 1].end < v->begin); /* maximal: a base below lo lies between two runs */
                    double cs = 0.0, bs = 0.0, es = 0.0;
                    for (unsigned i = v->begin; i < v->end; ++i)
                    {
                        CHECK(core[i + 1] >= lo && core[i + 1] <= v->core_max);
                        CHECK(i >= v->peak || core[i + 1] < v->core_max); /* the first of equals */
                        cs += core[i + 1], bs += begin[i], es += end[i + 1];
                    }
                    CHECK(v->core_sum == cs && v->begin_sum == bs && v->end_sum == es); /* index order */
                    CHECK(v->begin == 0 || !(core[v->begin] >= lo));
                    CHECK(v->end == L || !(core[v->end + 1] >= lo));
                }
                /* one record short: the count is true, nothing behind the array is written */
                if (n)
                {
                    struct dcp_envelope *few = malloc(sizeof *few * (n - 1 ? n - 1 : 1));
                    if (!few) return 2;
                    CHECK(dcp_posterior_envelope_records(begin, end, core, L, hi, lo, min_len, few, n - 1, &n2) == DCP_OK && n2 == n);
                    CHECK(n == 1 || memcmp(few, out, sizeof *few * (n - 1)) == 0);
                    free(few);
                }
                /* the records as regions, at their exact sizes */
                uint32_t const seq_idx[1] = {0}, seq_len[1] = {L};
                uint32_t *reg = malloc(sizeof(uint32_t) * 4 * (n ? n : 1));
                if (!reg) return 2;
                for (unsigned flank = 0; flank <= 300; flank += 100)
                {
                    CHECK(dcp_envelopes_regions(out, n, seq_idx, 1, seq_len, 1, flank, reg, reg + n, reg + 2 * n, reg + 3 * n) == DCP_OK);
                    for (unsigned k = 0; k < n; ++k)
                    {
                        CHECK(reg[k] == 0 && reg[3 * n + k] == 0 && reg[n + k] <= out[k].begin);
                        CHECK(reg[n + k] + reg[2 * n + k] >= out[k].end && reg[n + k] + reg[2 * n + k] <= L);
                        CHECK(flank || (reg[n + k] == out[k].begin && reg[2 * n + k] == out[k].end - out[k].begin));
                        CHECK(flank < 300 || (reg[n + k] == 0 && reg[2 * n + k] == L));
                    }
                }
                if (n)
                {
                    /* refusals write nothing */
                    memset(reg, 0x5a, sizeof(uint32_t) * 4 * n);
                    uint32_t const past[1] = {1}, shorter[1] = {out[n - 1].end - 1};
                    CHECK(dcp_envelopes_regions(out, n, seq_idx, 0, seq_len, 1, 0, reg, reg + n, reg + 2 * n, reg + 3 * n) == DCP_EINVAL);
                    CHECK(dcp_envelopes_regions(out, n, past, 1, seq_len, 1, 0, reg, reg + n, reg + 2 * n, reg + 3 * n) == DCP_EINVAL);
                    CHECK(dcp_envelopes_regions(out, n, seq_idx, 1, shorter, 1, 0, reg, reg + n, reg + 2 * n, reg + 3 * n) == DCP_EINVAL);
                    CHECK(dcp_envelopes_regions(NULL, n, seq_idx, 1, seq_len, 1, 0, reg, reg + n, reg + 2 * n, reg + 3 * n) == DCP_EINVAL);
                    CHECK(dcp_envelopes_regions(out, n, seq_idx, 1, seq_len, 1, 0, reg, NULL, reg + 2 * n, reg + 3 * n) == DCP_EINVAL);
                    struct dcp_envelope const was = out[n - 1];
                    out[n - 1].begin = out[n - 1].end;
                    CHECK(dcp_envelopes_regions(out, n, seq_idx, 1, seq_len, 1, 0, reg, reg + n, reg + 2 * n, reg + 3 * n) == DCP_EINVAL);
                    out[n - 1] = was;
                    for (unsigned k = 0; k < 4 * n; ++k)
                        CHECK(reg[k] == 0x5a5a5a5au);
                }
                CHECK(dcp_envelopes_regions(NULL, 0, NULL, 0, NULL, 0, 0, NULL, NULL, NULL, NULL) == DCP_OK);
                free(reg);
                free(out);
            }
        /* refusals write nothing */
        struct dcp_envelope one;
        memset(&one, 0x5a, sizeof one);
        unsigned n = 77;
        CHECK(dcp_posterior_envelope_records(begin, end, core, L, NAN, 0.1, 1, &one, 1, &n) == DCP_EINVAL);
        CHECK(dcp_posterior_envelope_records(begin, end, core, L, 0.5, NAN, 1, &one, 1, &n) == DCP_EINVAL);
        CHECK(dcp_posterior_envelope_records(begin, end, core, L, 0.1, 0.5, 1, &one, 1, &n) == DCP_EINVAL);
        CHECK(dcp_posterior_envelope_records(NULL, end, core, L, 0.5, 0.1, 1, &one, 1, &n) == DCP_EINVAL);
        CHECK(dcp_posterior_envelope_records(begin, NULL, core, L, 0.5, 0.1, 1, &one, 1, &n) == DCP_EINVAL);
        CHECK(dcp_posterior_envelope_records(begin, end, NULL, L, 0.5, 0.1, 1, &one, 1, &n) == DCP_EINVAL);
        CHECK(dcp_posterior_envelope_records(begin, end, core, L, 0.5, 0.1, 1, NULL, 1, &n) == DCP_EINVAL);
        CHECK(dcp_posterior_envelope_records(begin, end, core, L, 0.5, 0.1, 1, &one, 1, NULL) == DCP_EINVAL);
        CHECK(n == 77 && one.pair == 0x5a5a5a5au && one.end == 0x5a5a5a5au);
        CHECK(dcp_posterior_envelope_records(NULL, NULL, NULL, 0, 0.5, 0.1, 1, NULL, 0, &n) == DCP_OK && n == 0);
        free(begin), free(end), free(core);
    }
    printf("asan_envelopes ok\n");
    return 0;
}
