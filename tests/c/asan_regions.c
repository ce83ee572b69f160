/*
 * dcp_domains_regions and dcp_domains_locate_regions (include/dcp_gpu.h) under ASan + UBSan: a stand-alone CPU program,
 * linked with csrc/dcp_model.cpp alone.  Every array lives on the heap at exactly the size the call is told; the
 * answers are checked against the rules restated here (the clustering by a selection loop over each group); the
 * refusals write nothing.
 */
#include "dcp_gpu.h"
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

/* (src, minus, profile, begin, end, index) of a before that of b */
static int before(uint32_t const *src, uint8_t const *minus, uint32_t const *prof, uint64_t const *b, uint64_t const *e,
                  unsigned x, unsigned y)
{
    if (src[x] != src[y]) return src[x] < src[y];
    if (!minus[x] != !minus[y]) return !minus[x];
    if (prof[x] != prof[y]) return prof[x] < prof[y];
    if (b[x] != b[y]) return b[x] < b[y];
    if (e[x] != e[y]) return e[x] < e[y];
    return x < y;
}

static void regions_case(unsigned n, unsigned nsrc, uint64_t max_gap, uint32_t flank, uint32_t span)
{
    uint32_t *len = malloc(nsrc * sizeof *len);
    for (unsigned s = 0; s < nsrc; ++s)
        len[s] = span + (uint32_t)(rnd() % 1000);
    uint32_t *src = malloc(n * sizeof *src), *prof = malloc(n * sizeof *prof), *reg_of = malloc(n * sizeof *reg_of);
    uint8_t *minus = malloc(n);
    uint64_t *b = malloc(n * sizeof *b), *e = malloc(n * sizeof *e);
    for (unsigned j = 0; j < n; ++j)
    {
        src[j] = (uint32_t)(rnd() % nsrc), prof[j] = (uint32_t)(rnd() % 3), minus[j] = (uint8_t)(rnd() % 2 ? rnd() % 255 + 1 : 0);
        uint32_t const L = len[src[j]];
        b[j] = j % 7 == 0 ? 0 : rnd() % L;                               /* touching the first base */
        e[j] = j % 7 == 1 ? L : b[j] + 1 + rnd() % (L - b[j] < 300 ? L - b[j] : 300); /* the last */
    }
    unsigned nreg = 77;
    /* the counting call: no region arrays at all */
    int rc = dcp_domains_regions(src, minus, prof, b, e, n, len, nsrc, max_gap, flank, reg_of, NULL, NULL, NULL, NULL, NULL, NULL, 0, &nreg);
    CHECK(rc == DCP_ENOMEM && nreg >= 1 && nreg <= n);
    unsigned const cap = nreg;
    uint32_t *rsrc = malloc(cap * sizeof *rsrc), *rprof = malloc(cap * sizeof *rprof), *rb = malloc(cap * sizeof *rb);
    uint32_t *rl = malloc(cap * sizeof *rl), *rn = malloc(cap * sizeof *rn);
    uint8_t *rm = malloc(cap);
    if (cap > 1)
    {
        nreg = 77;
        CHECK(dcp_domains_regions(src, minus, prof, b, e, n, len, nsrc, max_gap, flank, reg_of, rsrc, rm, rprof, rb, rl, rn, cap - 1, &nreg) == DCP_ENOMEM);
        CHECK(nreg == cap);
    }
    CHECK(dcp_domains_regions(src, minus, prof, b, e, n, len, nsrc, max_gap, flank, reg_of, rsrc, rm, rprof, rb, rl, rn, cap, &nreg) == 0);
    CHECK(nreg == cap);
    /* the rule restated: repeatedly take the first domain (in the rule's order) not yet taken */
    unsigned char *taken = calloc(n, 1);
    unsigned r = 0, prev = 0, parts = 0;
    uint64_t lo = 0, hi = 0;
    for (unsigned k = 0; k < n; ++k)
    {
        unsigned best = n;
        for (unsigned j = 0; j < n; ++j)
            if (!taken[j] && (best == n || before(src, minus, prof, b, e, j, best))) best = j;
        taken[best] = 1;
        int const same = k > 0 && src[best] == src[prev] && !minus[best] == !minus[prev] && prof[best] == prof[prev];
        int const joins = same && (b[best] <= hi || b[best] - hi <= max_gap);
        if (k > 0 && !joins)
        {
            uint64_t const rb_ = lo - (lo < flank ? lo : flank), re_ = hi + flank < len[src[prev]] ? hi + flank : len[src[prev]];
            CHECK(r < nreg && rsrc[r] == src[prev] && rm[r] == (minus[prev] ? 1 : 0) && rprof[r] == prof[prev]);
            CHECK(r < nreg && rb[r] == rb_ && rl[r] == re_ - rb_ && rn[r] == parts);
            ++r;
        }
        if (!joins) lo = b[best], hi = e[best], parts = 0;
        else if (e[best] > hi) hi = e[best];
        ++parts;
        CHECK(reg_of[best] == r);
        prev = best;
    }
    {
        uint64_t const rb_ = lo - (lo < flank ? lo : flank), re_ = hi + flank < len[src[prev]] ? hi + flank : len[src[prev]];
        CHECK(r + 1 == nreg && rsrc[r] == src[prev] && rb[r] == rb_ && rl[r] == re_ - rb_ && rn[r] == parts);
    }
    /* the refusals write nothing */
    {
        uint32_t *of2 = malloc(n * sizeof *of2);
        memset(of2, 0x5a, n * sizeof *of2);
        uint32_t const keep_b0 = rb[0];
        uint64_t const old = e[n / 2];
        nreg = 77;
        e[n / 2] = b[n / 2]; /* an empty interval */
        CHECK(dcp_domains_regions(src, minus, prof, b, e, n, len, nsrc, max_gap, flank, of2, rsrc, rm, rprof, rb, rl, rn, cap, &nreg) == DCP_EINVAL);
        e[n / 2] = (uint64_t)len[src[n / 2]] + 1; /* past the source's end */
        CHECK(dcp_domains_regions(src, minus, prof, b, e, n, len, nsrc, max_gap, flank, of2, rsrc, rm, rprof, rb, rl, rn, cap, &nreg) == DCP_EINVAL);
        e[n / 2] = old;
        uint32_t const s_old = src[n - 1];
        src[n - 1] = nsrc; /* no such source */
        CHECK(dcp_domains_regions(src, minus, prof, b, e, n, len, nsrc, max_gap, flank, of2, rsrc, rm, rprof, rb, rl, rn, cap, &nreg) == DCP_EINVAL);
        src[n - 1] = s_old;
        CHECK(dcp_domains_regions(src, minus, prof, b, e, n, NULL, nsrc, max_gap, flank, of2, rsrc, rm, rprof, rb, rl, rn, cap, &nreg) == DCP_EINVAL);
        CHECK(dcp_domains_regions(src, minus, prof, b, e, n, len, nsrc, max_gap, flank, of2, rsrc, rm, rprof, rb, NULL, rn, cap, &nreg) == DCP_EINVAL);
        CHECK(dcp_domains_regions(src, minus, prof, b, e, n, len, nsrc, max_gap, flank, of2, rsrc, rm, rprof, rb, rl, rn, cap, NULL) == DCP_EINVAL);
        CHECK(nreg == 77 && rb[0] == keep_b0);
        for (unsigned j = 0; j < n; ++j)
            CHECK(of2[j] == 0x5a5a5a5au);
        free(of2);
    }
    free(len), free(src), free(prof), free(reg_of), free(minus), free(b), free(e);
    free(rsrc), free(rprof), free(rb), free(rl), free(rn), free(rm), free(taken);
}

static void locate_case(unsigned nres, unsigned n)
{
    uint32_t *len = malloc(nres * sizeof *len), *rsrc = malloc(nres * sizeof *rsrc), *rb = malloc(nres * sizeof *rb);
    uint8_t *rm = malloc(nres);
    for (unsigned r = 0; r < nres; ++r)
    {
        len[r] = 1 + (uint32_t)(rnd() % 5000);
        rsrc[r] = r / 3, rm[r] = (uint8_t)(r % 2 ? 1 + rnd() % 255 : 0);
        rb[r] = r % 3 == 0 ? 0 : r % 3 == 1 ? 0xfffffff0u : (uint32_t)(rnd() % 100000); /* offset 0; sums that need 64 bits */
    }
    uint32_t *res = malloc(n * sizeof *res), *src = malloc(n * sizeof *src);
    struct dcp_domain *dom = calloc(n, sizeof *dom);
    uint64_t *b = malloc(n * sizeof *b), *e = malloc(n * sizeof *e);
    uint8_t *minus = malloc(n);
    for (unsigned j = 0; j < n; ++j)
    {
        res[j] = (uint32_t)(rnd() % nres);
        uint32_t const L = len[res[j]];
        dom[j].seq_begin = j % 4 == 0 ? 0 : (uint32_t)(rnd() % L);
        dom[j].seq_end = j % 4 == 1 ? L : dom[j].seq_begin + (uint32_t)(rnd() % (L - dom[j].seq_begin + 1));
    }
    CHECK(dcp_domains_locate_regions(res, dom, n, len, nres, rsrc, rb, rm, src, b, e, minus) == 0);
    for (unsigned j = 0; j < n; ++j)
    {
        uint32_t const r = res[j], L = len[r];
        CHECK(src[j] == rsrc[r] && minus[j] == (rm[r] ? 1 : 0));
        CHECK(b[j] == (uint64_t)rb[r] + (rm[r] ? L - dom[j].seq_end : dom[j].seq_begin));
        CHECK(e[j] == (uint64_t)rb[r] + (rm[r] ? L - dom[j].seq_begin : dom[j].seq_end));
    }
    memset(src, 0x5a, n * sizeof *src), memset(b, 0x5a, n * sizeof *b), memset(e, 0x5a, n * sizeof *e), memset(minus, 0x5a, n);
    uint32_t const r_old = res[n - 1];
    res[n - 1] = nres;
    CHECK(dcp_domains_locate_regions(res, dom, n, len, nres, rsrc, rb, rm, src, b, e, minus) == DCP_EINVAL);
    res[n - 1] = r_old;
    uint32_t const e_old = dom[n / 2].seq_end;
    dom[n / 2].seq_end = len[res[n / 2]] + 1;
    CHECK(dcp_domains_locate_regions(res, dom, n, len, nres, rsrc, rb, rm, src, b, e, minus) == DCP_EINVAL);
    dom[n / 2].seq_end = e_old;
    CHECK(dcp_domains_locate_regions(res, dom, n, len, nres, rsrc, rb, NULL, src, b, e, minus) == DCP_EINVAL);
    CHECK(dcp_domains_locate_regions(res, dom, n, len, nres, rsrc, rb, rm, src, b, e, NULL) == DCP_EINVAL);
    for (unsigned j = 0; j < n; ++j)
        CHECK(src[j] == 0x5a5a5a5au && b[j] == 0x5a5a5a5a5a5a5a5aull && e[j] == b[j] && minus[j] == 0x5a);
    free(len), free(rsrc), free(rb), free(rm), free(res), free(src), free(dom), free(b), free(e), free(minus);
}

int main(void)
{
    static uint64_t const gaps[] = {0, 1, 50, 100000, ~0ull};
    static uint32_t const flanks[] = {0, 1, 30, 5000, 0xffffffffu};
    for (unsigned g = 0; g < 5; ++g)
        for (unsigned f = 0; f < 5; ++f)
        {
            regions_case(1, 1, gaps[g], flanks[f], 10);
            regions_case(2, 1, gaps[g], flanks[f], 400);
            regions_case(300, 3, gaps[g], flanks[f], 20000);
            regions_case(1500, 2, gaps[g], flanks[f], 3000); /* piled up: long clusters */
        }
    {
        unsigned nreg = 77;
        CHECK(dcp_domains_regions(NULL, NULL, NULL, NULL, NULL, 0, NULL, 0, 0, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, &nreg) == 0 && nreg == 0);
        CHECK(dcp_domains_regions(NULL, NULL, NULL, NULL, NULL, 0, NULL, 0, 0, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, NULL) == DCP_EINVAL);
    }
    locate_case(1, 40);
    locate_case(7, 500);
    locate_case(60, 3000);
    CHECK(dcp_domains_locate_regions(NULL, NULL, 0, NULL, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == 0); /* n = 0 reads nothing */
    if (failed) return 1;
    puts("asan_regions ok");
    return 0;
}
