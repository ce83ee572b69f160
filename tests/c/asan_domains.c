/*
 * dcp_domains_locate and dcp_domains_merge (include/dcp_gpu.h) under ASan + UBSan: a stand-alone CPU program, linked
 * with csrc/dcp_model.cpp alone.  Every array lives on the heap at exactly the size the call is told; the answers are
 * checked against the rules restated here (the merge by the plain quadratic loop); the refusals write nothing.
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

static uint64_t rnd_state = 88172645463325252ull;
static uint64_t rnd(void)
{
    rnd_state ^= rnd_state << 13, rnd_state ^= rnd_state >> 7, rnd_state ^= rnd_state << 17;
    return rnd_state;
}

static void locate_case(unsigned per_strand, unsigned strands, int cut, unsigned n)
{
    unsigned const resident = per_strand * strands;
    uint32_t *len = malloc(resident * sizeof *len), *wsrc = malloc(per_strand * sizeof *wsrc), *woff = malloc(per_strand * sizeof *woff);
    for (unsigned i = 0; i < per_strand; ++i)
    {
        len[i] = 1 + (uint32_t)(rnd() % 5000);
        if (strands == 2) len[per_strand + i] = len[i];
        wsrc[i] = i / 3, woff[i] = i % 3 == 2 ? 0xfffffff0u : (i % 3) * 1023u; /* offsets near 2^32: the sums need 64 bits */
    }
    uint32_t *res = malloc(n * sizeof *res), *src = malloc(n * sizeof *src);
    struct dcp_domain *dom = calloc(n, sizeof *dom);
    uint64_t *b = malloc(n * sizeof *b), *e = malloc(n * sizeof *e);
    uint8_t *minus = malloc(n);
    for (unsigned j = 0; j < n; ++j)
    {
        res[j] = (uint32_t)(rnd() % resident);
        uint32_t const L = len[res[j]];
        dom[j].seq_begin = j % 4 == 0 ? 0 : (uint32_t)(rnd() % L);                   /* touching the first base */
        dom[j].seq_end = j % 4 == 1 ? L : dom[j].seq_begin + (uint32_t)(rnd() % (L - dom[j].seq_begin + 1)); /* the last */
    }
    CHECK(dcp_domains_locate(res, dom, n, len, per_strand, strands, cut ? wsrc : NULL, cut ? woff : NULL, src, b, e, minus) == 0);
    for (unsigned j = 0; j < n; ++j)
    {
        uint32_t const r = res[j], i = r % per_strand, L = len[r];
        int const m = r >= per_strand;
        uint64_t const off = cut ? woff[i] : 0;
        CHECK(src[j] == (cut ? wsrc[i] : i) && minus[j] == m);
        CHECK(b[j] == off + (m ? L - dom[j].seq_end : dom[j].seq_begin));
        CHECK(e[j] == off + (m ? L - dom[j].seq_begin : dom[j].seq_end));
    }
    if (n)
    {
        /* refusals: nothing is written */
        uint32_t const keep_res = res[n - 1], keep_end = dom[n - 1].seq_end;
        memset(src, 0x5a, n * sizeof *src), memset(minus, 0x5a, n);
        res[n - 1] = resident;
        CHECK(dcp_domains_locate(res, dom, n, len, per_strand, strands, NULL, NULL, src, b, e, minus) == DCP_EINVAL);
        res[n - 1] = keep_res;
        dom[n - 1].seq_end = len[keep_res] + 1;
        CHECK(dcp_domains_locate(res, dom, n, len, per_strand, strands, NULL, NULL, src, b, e, minus) == DCP_EINVAL);
        dom[n - 1].seq_end = keep_end;
        CHECK(dcp_domains_locate(res, dom, n, len, per_strand, 3, NULL, NULL, src, b, e, minus) == DCP_EINVAL);
        CHECK(dcp_domains_locate(res, dom, n, len, per_strand, strands, NULL, NULL, NULL, b, e, minus) == DCP_EINVAL);
        for (unsigned j = 0; j < n; ++j)
            CHECK(src[j] == 0x5a5a5a5au && minus[j] == 0x5a);
    }
    free(len), free(wsrc), free(woff), free(res), free(src), free(dom), free(b), free(e), free(minus);
}

/* the rule, quadratic: candidates by (odds desc, length desc, index asc), kept unless a kept one of the group overlaps
 * it by more than half the shorter */
static void merge_case(unsigned n, unsigned nsrc, unsigned nprof, uint64_t span, uint64_t maxlen, uint64_t base)
{
    uint32_t *src = malloc(n * sizeof *src), *prof = malloc(n * sizeof *prof);
    uint8_t *minus = malloc(n), *keep = malloc(n), *want = calloc(n ? n : 1, 1);
    uint64_t *b = malloc(n * sizeof *b), *e = malloc(n * sizeof *e);
    double *odds = malloc(n * sizeof *odds);
    unsigned *order = malloc(n * sizeof *order);
    for (unsigned j = 0; j < n; ++j)
    {
        src[j] = (uint32_t)(rnd() % nsrc), prof[j] = (uint32_t)(rnd() % nprof), minus[j] = (uint8_t)(rnd() % 2 ? 7 : 0); /* any non-zero is minus */
        b[j] = base + rnd() % span, e[j] = b[j] + 1 + rnd() % maxlen;
        odds[j] = (double)(rnd() % 16) - 3.0; /* many ties */
        order[j] = j;
    }
    for (unsigned i = 1; i < n; ++i) /* insertion sort by the rank */
        for (unsigned k = i; k > 0; --k)
        {
            unsigned const x = order[k - 1], y = order[k];
            uint64_t const lx = e[x] - b[x], ly = e[y] - b[y];
            int const before = odds[x] != odds[y] ? odds[x] > odds[y] : lx != ly ? lx > ly : x < y;
            if (before) break;
            order[k - 1] = y, order[k] = x;
        }
    unsigned nwant = 0;
    for (unsigned i = 0; i < n; ++i)
    {
        unsigned const j = order[i];
        int ok = 1;
        for (unsigned k = 0; k < n && ok; ++k)
        {
            if (!want[k] || src[k] != src[j] || !minus[k] != !minus[j] || prof[k] != prof[j]) continue;
            uint64_t const lo = b[j] > b[k] ? b[j] : b[k], hi = e[j] < e[k] ? e[j] : e[k];
            uint64_t const ov = hi > lo ? hi - lo : 0, lj = e[j] - b[j], lk = e[k] - b[k], sh = lj < lk ? lj : lk;
            if (ov > sh - ov) ok = 0;
        }
        want[j] = (uint8_t)ok, nwant += (unsigned)ok;
    }
    unsigned nkept = 12345;
    CHECK(dcp_domains_merge(src, minus, prof, b, e, odds, n, keep, &nkept) == 0);
    CHECK(nkept == nwant);
    for (unsigned j = 0; j < n; ++j)
        CHECK(keep[j] == want[j]);
    CHECK(dcp_domains_merge(src, minus, prof, b, e, odds, n, keep, NULL) == 0);
    if (n)
    {
        memset(keep, 0x5a, n);
        double const o = odds[n / 2];
        odds[n / 2] = NAN;
        CHECK(dcp_domains_merge(src, minus, prof, b, e, odds, n, keep, &nkept) == DCP_EINVAL);
        odds[n / 2] = o;
        uint64_t const en = e[n - 1];
        e[n - 1] = b[n - 1];
        CHECK(dcp_domains_merge(src, minus, prof, b, e, odds, n, keep, &nkept) == DCP_EINVAL);
        e[n - 1] = en;
        CHECK(dcp_domains_merge(src, minus, prof, b, e, NULL, n, keep, &nkept) == DCP_EINVAL);
        for (unsigned j = 0; j < n; ++j)
            CHECK(keep[j] == 0x5a);
        CHECK(nkept == nwant);
    }
    free(src), free(prof), free(minus), free(keep), free(want), free(b), free(e), free(odds), free(order);
}

int main(void)
{
    for (unsigned strands = 1; strands <= 2; ++strands)
        for (int cut = 0; cut <= 1; ++cut)
        {
            locate_case(1, strands, cut, 9);
            locate_case(7, strands, cut, 200);
            locate_case(7, strands, cut, 0);
        }
    CHECK(dcp_domains_locate(NULL, NULL, 0, NULL, 0, 0, NULL, NULL, NULL, NULL, NULL, NULL) == 0); /* n = 0 reads nothing */
    merge_case(0, 1, 1, 1, 1, 0);
    merge_case(1, 1, 1, 1, 1, 0);
    merge_case(300, 1, 1, 2000, 300, 0);          /* one dense group */
    merge_case(300, 1, 1, 50, 40, 0);             /* nearly everything overlaps */
    merge_case(2000, 3, 4, 100000, 900, 0);       /* 24 groups */
    merge_case(400, 2, 2, 5000, 700, 0xffffffffffff0000ull - 6000); /* coordinates near 2^64: ov and 2 ov do not wrap */
    CHECK(dcp_domains_merge(NULL, NULL, NULL, NULL, NULL, NULL, 0, NULL, NULL) == 0);
    if (failed) fprintf(stderr, "%d checks failed\n", failed);
    else printf("asan_domains ok\n");
    return failed;
}
