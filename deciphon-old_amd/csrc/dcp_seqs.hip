// dcp_seqs.hip -- the reverse strand of the resident batch (dcp_gpu_seqs_add_revcomp) with its host restatement, and
// the cut of the resident batch into overlapping windows (dcp_gpu_seqs_cut_windows, further down) and into arbitrary
// regions of either strand (dcp_gpu_seqs_cut_regions, behind the windows).
//
// A resident sequence of L bases is L / 16 + 3 words, base i in bits 2 (i & 15) of word i >> 4 (A = 0, C = 1, G = 2,
// T = 3), every bit behind base L - 1 zero.  Its reverse complement has base i = 3 - base(L - 1 - i): output word j
// holds the input bases [e - 16, e), e = L - 16 j, in falling order -- at most two adjacent input words, aligned by one
// 64-bit shift, their sixteen 2-bit groups reversed, all bits complemented (3 - b = ~b on two bits), the groups behind
// the sequence's end masked off.  One lane per output word of the whole batch, consecutive lanes on consecutive
// words; a lane finds its sequence by a binary search in woff (the lanes of a wavefront mostly share it: the probes
// are broadcast reads of a few cache lines).  Sequences of 1 nt and of 2^20 nt in one batch cost the same per word.
#include "dcp_seqs.h"

#include <hip/hip_runtime.h>

namespace
{

constexpr unsigned kBlock = 256;

__device__ __forceinline__ uint32_t reverse_groups(uint32_t x)
{
    uint32_t const y = __brev(x); // groups in reverse order, the two bits of each swapped
    return ((y >> 1) & 0x55555555u) | ((y & 0x55555555u) << 1);
}

__global__ __launch_bounds__(kBlock) void revcomp_words_kernel(uint32_t const *__restrict__ words_in,
                                                               uint32_t *__restrict__ words_out,
                                                               uint32_t const *__restrict__ woff,
                                                               uint32_t const *__restrict__ len, unsigned nseqs,
                                                               uint32_t nwords)
{
    uint64_t const g64 = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g64 >= nwords) return;
    uint32_t const g = (uint32_t)g64;
    // the sequence whose words [woff[q], woff[q + 1]) hold g: the last q with woff[q] <= g (woff[0] = 0)
    unsigned lo = 0, hi = nseqs;
    while (hi - lo > 1u)
    {
        unsigned const mid = lo + (hi - lo) / 2u;
        if (woff[mid] <= g) lo = mid;
        else hi = mid;
    }
    uint32_t const base = woff[lo], L = len[lo];
    uint32_t const j = g - base; // < L / 16 + 3
    uint32_t out = 0u;           // pad words stay zero
    if ((uint64_t)j * 16u < L)
    {
        uint32_t const e = L - j * 16u;          // the word's bases come from [e - 16, e) of the input, e >= 1
        uint32_t const we = e >> 4, r = e & 15u; // e >> 4 <= L / 16: inside the sequence's words
        uint32_t const *w = words_in + base;
        uint64_t const v = ((uint64_t)w[we] << 32) | (we ? w[we - 1u] : 0u);
        uint32_t const x = (uint32_t)(v >> (2u * r)); // group k = input base e - 16 + k (zero below base 0)
        uint32_t const cnt = e < 16u ? e : 16u;       // bases of this output word
        uint32_t const mask = cnt == 16u ? 0xffffffffu : (1u << (2u * cnt)) - 1u;
        out = ~reverse_groups(x) & mask;
    }
    words_out[g] = out;
}

__global__ __launch_bounds__(kBlock) void revcomp_index_kernel(uint32_t *__restrict__ woff, uint32_t *__restrict__ len,
                                                               unsigned nseqs, uint32_t nwords)
{
    unsigned const q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= nseqs) return;
    woff[nseqs + q] = woff[q] + nwords;
    len[nseqs + q] = len[q];
}

// Windows (dcp_gpu_seqs_cut_windows).  Window i of source s covers the source's bases [off, off + wl), wl =
// min(L, window), off = min(i step, L - window) (0 when L <= window): a sequence of its own in the new batch, wl / 16 + 3
// words.  The index kernel, one lane per window, finds its source in wfirst (the sources' first windows, wfirst[0] = 0,
// rising strictly: no source is empty) and writes the window's entry of the new woff / len and of the map.
__global__ __launch_bounds__(kBlock) void window_index_kernel(uint32_t const *__restrict__ src_len,
                                                              uint32_t const *__restrict__ wfirst,
                                                              uint32_t const *__restrict__ nwfirst, unsigned nsrc,
                                                              unsigned nwin, uint32_t window, uint32_t step,
                                                              uint32_t *__restrict__ woff, uint32_t *__restrict__ len,
                                                              uint32_t *__restrict__ wsrc, uint32_t *__restrict__ wofs)
{
    uint64_t const w64 = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (w64 >= nwin) return;
    uint32_t const w = (uint32_t)w64;
    unsigned lo = 0, hi = nsrc;
    while (hi - lo > 1u)
    {
        unsigned const mid = lo + (hi - lo) / 2u;
        if (wfirst[mid] <= w) lo = mid;
        else hi = mid;
    }
    uint32_t const L = src_len[lo], i = w - wfirst[lo];
    uint32_t const wl = L < window ? L : window;
    uint32_t off = 0u;
    if (L > window)
    {
        uint64_t const at = (uint64_t)i * step;
        off = at < L - window ? (uint32_t)at : L - window; // the last window ends at L
    }
    woff[w] = nwfirst[lo] + i * (wl / 16u + 3u); // the plan checked that the batch's words fit 32 bits
    len[w] = wl;
    wsrc[w] = lo;
    wofs[w] = off;
}

// One lane per word of the new batch, as revcomp_words_kernel: word j of window (src, off, wl) holds the source's
// bases b0 = off + 16 j .. b0 + 15, which lie in the source's words b0 >> 4 and (b0 >> 4) + 1 -- the second exists
// for every b0 < L, a source has L / 16 + 3 words -- aligned by one 64-bit shift.  The source goes on behind the
// window's last base (unlike the reverse strand's input): the groups behind base wl - 1 are masked off, a resident
// sequence is zero there.
__global__ __launch_bounds__(kBlock) void window_words_kernel(uint32_t const *__restrict__ words_in,
                                                              uint32_t const *__restrict__ src_woff,
                                                              uint32_t *__restrict__ words_out,
                                                              uint32_t const *__restrict__ woff,
                                                              uint32_t const *__restrict__ len,
                                                              uint32_t const *__restrict__ wsrc,
                                                              uint32_t const *__restrict__ wofs, unsigned nwin,
                                                              uint32_t nwords)
{
    uint64_t const g64 = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g64 >= nwords) return;
    uint32_t const g = (uint32_t)g64;
    unsigned lo = 0, hi = nwin; // the last window with woff <= g (woff[0] = 0)
    while (hi - lo > 1u)
    {
        unsigned const mid = lo + (hi - lo) / 2u;
        if (woff[mid] <= g) lo = mid;
        else hi = mid;
    }
    uint32_t const wl = len[lo];
    uint32_t const j = g - woff[lo]; // < wl / 16 + 3
    uint32_t out = 0u;               // pad words stay zero
    if ((uint64_t)j * 16u < wl)
    {
        uint32_t const b0 = wofs[lo] + j * 16u; // < off + wl <= L
        uint32_t const *w = words_in + src_woff[wsrc[lo]] + (b0 >> 4);
        uint64_t const v = ((uint64_t)w[1] << 32) | w[0];
        uint32_t const x = (uint32_t)(v >> (2u * (b0 & 15u)));
        uint32_t const cnt = wl - j * 16u < 16u ? wl - j * 16u : 16u; // bases of this output word
        uint32_t const mask = cnt == 16u ? 0xffffffffu : (1u << (2u * cnt)) - 1u;
        out = x & mask;
    }
    words_out[g] = out;
}

// Regions (dcp_gpu_seqs_cut_regions): one lane per word of the new batch, as the two kernels above.  A plus region is a
// window at an arbitrary offset: window_words_kernel's arithmetic.  Word j of a minus region holds the source's bases
// [e - 16, e), e = begin + len - 16 j, in falling order and complemented: revcomp_words_kernel's arithmetic with the
// source's word index -- e >> 4 <= L / 16 stays inside the source's words, the word below is read only if e >= 16 --
// but unlike the whole sequence's reverse complement the bases BELOW `begin` are real bases of the source, not zeros:
// the min(16, len - 16 j) groups of the word are masked after the complement, whatever lies below.
__global__ __launch_bounds__(kBlock) void region_words_kernel(uint32_t const *__restrict__ words_in,
                                                              uint32_t const *__restrict__ src_woff,
                                                              uint32_t *__restrict__ words_out,
                                                              uint32_t const *__restrict__ woff,
                                                              uint32_t const *__restrict__ len,
                                                              uint32_t const *__restrict__ rsrc,
                                                              uint32_t const *__restrict__ rbegin,
                                                              uint32_t const *__restrict__ rminus, unsigned n,
                                                              uint32_t nwords)
{
    uint64_t const g64 = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g64 >= nwords) return;
    uint32_t const g = (uint32_t)g64;
    unsigned lo = 0, hi = n; // the last region with woff <= g (woff[0] = 0)
    while (hi - lo > 1u)
    {
        unsigned const mid = lo + (hi - lo) / 2u;
        if (woff[mid] <= g) lo = mid;
        else hi = mid;
    }
    uint32_t const rl = len[lo];
    uint32_t const j = g - woff[lo]; // < rl / 16 + 3
    uint32_t out = 0u;               // pad words stay zero
    if ((uint64_t)j * 16u < rl)
    {
        uint32_t const *w = words_in + src_woff[rsrc[lo]];
        uint32_t const cnt = rl - j * 16u < 16u ? rl - j * 16u : 16u; // bases of this output word
        uint32_t const mask = cnt == 16u ? 0xffffffffu : (1u << (2u * cnt)) - 1u;
        if (rminus[lo])
        {
            uint32_t const e = rbegin[lo] + rl - j * 16u; // 1 <= e <= L
            uint32_t const we = e >> 4, r = e & 15u;
            uint64_t const v = ((uint64_t)w[we] << 32) | (we ? w[we - 1u] : 0u);
            uint32_t const x = (uint32_t)(v >> (2u * r)); // group k = source base e - 16 + k
            out = ~reverse_groups(x) & mask;
        }
        else
        {
            uint32_t const b0 = rbegin[lo] + j * 16u; // < begin + len <= L: words b0 >> 4 and the next one exist
            uint64_t const v = ((uint64_t)w[(b0 >> 4) + 1u] << 32) | w[b0 >> 4];
            out = (uint32_t)(v >> (2u * (b0 & 15u))) & mask;
        }
    }
    words_out[g] = out;
}

} // namespace

extern "C" int dcp_launch_regions(dcp_region_args const *a, void *stream)
{
    if (!a || a->n == 0 || a->nwords == 0) return (int)hipErrorInvalidValue;
    unsigned const wblocks = (unsigned)(((uint64_t)a->nwords + kBlock - 1u) / kBlock);
    region_words_kernel<<<wblocks, kBlock, 0, (hipStream_t)stream>>>(a->src_words, a->src_woff, a->words, a->woff, a->len,
                                                                     a->rsrc, a->rbegin, a->rminus, a->n, a->nwords);
    return (int)hipGetLastError();
}

extern "C" int dcp_launch_windows(dcp_window_args const *a, void *stream)
{
    if (!a || a->nsrc == 0 || a->nwin == 0 || a->nwords == 0 || a->window == 0 || a->step == 0 || a->step > a->window)
        return (int)hipErrorInvalidValue;
    hipStream_t const s = (hipStream_t)stream;
    unsigned const iblocks = (unsigned)(((uint64_t)a->nwin + kBlock - 1u) / kBlock);
    unsigned const wblocks = (unsigned)(((uint64_t)a->nwords + kBlock - 1u) / kBlock);
    // in this order on one stream: the word kernel reads what the index kernel wrote
    window_index_kernel<<<iblocks, kBlock, 0, s>>>(a->src_len, a->wfirst, a->nwfirst, a->nsrc, a->nwin, a->window, a->step,
                                                   a->woff, a->len, a->wsrc, a->wofs);
    window_words_kernel<<<wblocks, kBlock, 0, s>>>(a->src_words, a->src_woff, a->words, a->woff, a->len, a->wsrc, a->wofs,
                                                   a->nwin, a->nwords);
    return (int)hipGetLastError();
}

extern "C" int dcp_launch_revcomp(uint32_t const *words_in, uint32_t *words_out, uint32_t *woff, uint32_t *len,
                                  unsigned nseqs, uint32_t nwords, void *stream)
{
    if (nseqs == 0 || nwords == 0) return (int)hipErrorInvalidValue;
    hipStream_t const s = (hipStream_t)stream;
    unsigned const wblocks = (unsigned)(((uint64_t)nwords + kBlock - 1u) / kBlock);
    // the word kernel reads the forward half of woff / len only: the index kernel may run behind it
    revcomp_words_kernel<<<wblocks, kBlock, 0, s>>>(words_in, words_out, woff, len, nseqs, nwords);
    revcomp_index_kernel<<<(nseqs + kBlock - 1u) / kBlock, kBlock, 0, s>>>(woff, len, nseqs, nwords);
    return (int)hipGetLastError();
}

// The same map on symbol ids, on the host: what the tests and the host layer restate the kernel with.
extern "C" void dcp_seq_revcomp(uint8_t const *ids, unsigned n, uint8_t *out)
{
    for (unsigned i = 0; i < n; ++i)
        out[i] = (uint8_t)(3u - ids[n - 1u - i]);
}
