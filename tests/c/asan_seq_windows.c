/*
 * The window rule (dcp_seq_window_count / _start / _plan, include/dcp_gpu.h) under ASan + UBSan: a stand-alone CPU
 * program, linked with csrc/dcp_model.cpp alone.  Every edge shape against the rule restated here; the plan over
 * heap arrays of exactly the size it is told; the refusals.
 */
#include "dcp_gpu.h"
#include <stdio.h>
#include <stdlib.h>

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

static uint64_t want_count(uint64_t L, uint64_t window, uint64_t step)
{
    return L <= window ? 1 : 1 + (L - window + step - 1) / step;
}
static uint64_t want_start(uint64_t L, uint64_t window, uint64_t step, uint64_t i)
{
    if (L <= window) return 0;
    return i * step < L - window ? i * step : L - window;
}

int main(void)
{
    static unsigned const lens[] = {1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 100, 1000, 10007, 1u << 20, 0xffffffffu};
    enum { NL = sizeof lens / sizeof lens[0] };
    for (unsigned a = 0; a < NL; ++a)
    {
        unsigned const L = lens[a];
        unsigned const windows[] = {1, 5, 15, 16, 17, 32, 33, 48, 100, L - 1, L, L + 1};
        for (unsigned b = 0; b < sizeof windows / sizeof windows[0]; ++b)
        {
            unsigned const window = windows[b];
            if (window == 0) continue;
            unsigned const steps[] = {1, 15, 16, 17, window - 1, window};
            for (unsigned c = 0; c < sizeof steps / sizeof steps[0]; ++c)
            {
                unsigned const step = steps[c];
                if (step == 0 || step > window) continue;
                uint64_t const cnt = want_count(L, window, step);
                CHECK(dcp_seq_window_count(L, window, step) == cnt);
                uint64_t const probe[] = {0, 1, 2, cnt / 2, cnt - 2, cnt - 1, cnt, 0xffffffffu};
                for (unsigned k = 0; k < sizeof probe / sizeof probe[0]; ++k)
                    if (probe[k] <= 0xffffffffu)
                        CHECK(dcp_seq_window_start(L, window, step, (unsigned)probe[k]) == want_start(L, window, step, probe[k]));
                uint64_t const wl = L < window ? L : window;
                CHECK(dcp_seq_window_start(L, window, step, (unsigned)(cnt - 1)) + wl == L); /* the last window ends at L */
                /* the plan of this sequence three times, in an array of exactly three */
                uint32_t *three = malloc(3 * sizeof *three);
                three[0] = three[1] = three[2] = L;
                uint64_t nwin = 7, nwords = 7;
                int const rc = dcp_seq_window_plan(three, 3, window, step, &nwin, &nwords);
                CHECK(nwin == 3 * cnt && nwords == 3 * cnt * (wl / 16 + 3));
                CHECK((rc != 0) == (nwin > 0xffffffffu || nwords > 0xffffffffu));
                CHECK(dcp_seq_window_plan(three, 3, window, step, NULL, NULL) == rc);
                free(three);
            }
        }
    }
    /* 70 000 sequences of 2^20 bases in windows of one: refused, the totals in 64 bits */
    {
        unsigned const n = 70000;
        uint32_t *len = malloc(n * sizeof *len);
        for (unsigned q = 0; q < n; ++q)
            len[q] = 1u << 20;
        uint64_t nwin = 0, nwords = 0;
        CHECK(dcp_seq_window_plan(len, n, 1, 1, &nwin, &nwords) != 0 && nwin == (uint64_t)n << 20 && nwords == 3 * ((uint64_t)n << 20));
        CHECK(dcp_seq_window_plan(len, 1365, 1, 1, &nwin, &nwords) == 0 && nwin == 1365ull << 20);
        free(len);
    }
    /* bad rules */
    {
        uint32_t one = 100;
        uint64_t nwin = 7, nwords = 7;
        static unsigned const bad[][2] = {{0, 0}, {0, 1}, {5, 0}, {5, 6}, {0xffffffffu, 0}};
        for (unsigned k = 0; k < sizeof bad / sizeof bad[0]; ++k)
        {
            CHECK(dcp_seq_window_count(100, bad[k][0], bad[k][1]) == 0);
            CHECK(dcp_seq_window_start(100, bad[k][0], bad[k][1], 3) == 0);
            CHECK(dcp_seq_window_plan(&one, 1, bad[k][0], bad[k][1], &nwin, &nwords) != 0 && nwin == 0 && nwords == 0);
        }
        CHECK(dcp_seq_window_plan(NULL, 1, 5, 5, &nwin, &nwords) != 0);
        CHECK(dcp_seq_window_plan(NULL, 0, 5, 5, &nwin, &nwords) == 0 && nwin == 0 && nwords == 0);
    }
    if (failed) fprintf(stderr, "%d checks failed\n", failed);
    else printf("asan_seq_windows ok\n");
    return failed;
}
