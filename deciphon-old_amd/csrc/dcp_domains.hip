// dcp_domains.hip -- hit paths split into domains on the device (dcp_gpu_path_domains / ...64).
//
// One wavefront per path, walking its steps 64 at a time; one template over the DB's real type.
//
// Parallel part of a trip.  Lane l loads step i0 + l and its predecessor (two coalesced 4-byte loads), takes its
// first base from an integer wave prefix sum of the seqlens plus the bases of the trips before, reads its fragment
// out of two adjacent 2-bit words of the resident sequence (as decode_kernel does: a sequence of L bases has L / 16
// + 3 words, so word (start >> 4) + 1 exists), forms the word code -- offsets 0, 4, 20, 84, 340 for 1..5 bases, the
// first base most significant -- and gathers its three values: t, the transition from the predecessor (the edges of
// the model graph, one by one); e, the emission of the fragment from the match table of its node / the insert table
// / the null table; n, the null table's value for the same code.  An edge that is not in the graph is not scored:
// the lane records (path << 32 | step) with a vector atomicMin and scores 0; the host refuses the call.
//
// Serial part.  The three running sums -- the path's total, the open domain's core and null sums -- take the 64
// lanes' values in lane order: an unrolled loop over compile-time lane indices that reads lane l's values with
// v_readlane and branches on bits of __ballot masks ("is B", "is E", "emits", ...), so the sums sit in every lane
// alike, control flow stays wave-uniform, and the additions happen in step order with no reassociation.  There is no
// floating-point reduction across lanes anywhere.  The counts of a domain are population counts of the "is M / I /
// D" and "seqlen != 3" masks between its B and its E, carried across trips.
//
// A domain's record is written at its E step: 12 words by 12 lanes, one vector store; lane 0 stores the two sums.
#include "dcp_domains.h"
#include "dcp_f64.h"
#include "dcp_kernels.h"

#include <hip/hip_runtime.h>

namespace
{

constexpr unsigned kWaves = 4;
constexpr unsigned kBlock = 64u * kWaves;
typedef unsigned long long u64;

// the resident tables of one profile
template <class Real> struct ProfView
{
    Real const *em, *tr, *ei, *en;
    unsigned ldk;
};

template <class Real> __device__ __forceinline__ ProfView<Real> view_of(dcp_domains_args const &a, unsigned slot);
template <> __device__ __forceinline__ ProfView<float> view_of<float>(dcp_domains_args const &a, unsigned slot)
{
    // (code, k) of a profile at emis_off + code ldk + k: also right for the column views of profiles that share rows
    dcp_prof_meta const pm = ((dcp_prof_meta const *)a.profs)[slot];
    return ProfView<float>{(float const *)a.match + pm.emis_off, (float const *)a.trans + pm.trans_off,
                           (float const *)a.insert + (size_t)pm.pidx * DCP_NCODES,
                           (float const *)a.null_tab + (size_t)pm.pidx * DCP_NCODES, pm.ldk};
}
template <> __device__ __forceinline__ ProfView<double> view_of<double>(dcp_domains_args const &a, unsigned slot)
{
    dcp_f64_prof const pm = ((dcp_f64_prof const *)a.profs)[slot];
    double const *xe = (double const *)a.insert + pm.xe_off;
    return ProfView<double>{(double const *)a.match + pm.tab_off, (double const *)a.trans + pm.trans_off, xe,
                            xe + DCP_NCODES, pm.ldk};
}

__device__ __forceinline__ unsigned lane_read(unsigned v, int l) { return (unsigned)__builtin_amdgcn_readlane((int)v, l); }
__device__ __forceinline__ float lane_read(float v, int l)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}
__device__ __forceinline__ double lane_read(double v, int l)
{
    u64 const b = __builtin_bit_cast(u64, v);
    unsigned const lo = lane_read((unsigned)b, l), hi = lane_read((unsigned)(b >> 32), l);
    return __builtin_bit_cast(double, ((u64)hi << 32) | lo);
}

// The transition into step (kind, x) from step (pkind, pk): the edges of the model graph.  false: no such edge.
template <class Real>
__device__ __forceinline__ bool edge(ProfView<Real> const &pv, Real const *xt, unsigned pkind, unsigned pk, unsigned kind,
                                     unsigned x, Real *t)
{
    unsigned const k = x - 1u, ldk = pv.ldk;
    if (kind == 0u) // M_k: from B, or from node k - 1
    {
        if (pkind == 3u && pk == 3u) return *t = pv.tr[(size_t)DCP_T_ENTRY * ldk + k], true;
        if (k > 0u && pk == k && pkind < 3u) return *t = pv.tr[(size_t)(DCP_T_MM + pkind) * ldk + k], true;
        return false;
    }
    if (kind == 1u) // I_k: from M_k or itself
    {
        if (pk == k + 1u && pkind < 2u) return *t = pv.tr[(size_t)(DCP_T_MI + pkind) * ldk + k], true;
        return false;
    }
    if (kind == 2u) // D_k: from M_{k-1} or D_{k-1}
    {
        if (k > 0u && pk == k && (pkind == 0u || pkind == 2u))
            return *t = pv.tr[(size_t)(pkind == 0u ? DCP_T_MD : DCP_T_DD) * ldk + k], true;
        return false;
    }
    unsigned const from = pkind == 3u ? pk : 100u; // a core state only precedes E
    int r = -1;
    switch (x) // 0 R, 1 S, 2 N, 3 B, 4 E, 5 J, 6 C, 7 T
    {
    case 0: r = from == 0u ? DCP_X_RR : -1; break;
    case 2: r = from == 1u ? DCP_X_SN : from == 2u ? DCP_X_NN : -1; break;
    case 3: r = from == 1u ? DCP_X_SB : from == 2u ? DCP_X_NB : from == 4u ? DCP_X_EB : from == 5u ? DCP_X_JB : -1; break;
    case 4: return *t = Real(0), pkind == 0u || (pkind == 2u && pk >= 2u); // every M_k, and D_k for k >= 2, ends the core at 0
    case 5: r = from == 4u ? DCP_X_EJ : from == 5u ? DCP_X_JJ : -1; break;
    case 6: r = from == 4u ? DCP_X_EC : from == 6u ? DCP_X_CC : -1; break;
    case 7: r = from == 4u ? DCP_X_ET : from == 6u ? DCP_X_CT : -1; break;
    default: break;
    }
    if (r < 0) return false;
    return *t = xt[r], true;
}

template <class Real> __global__ __launch_bounds__(kBlock) void domains_kernel(dcp_domains_args a)
{
    unsigned const lane = threadIdx.x & 63u;
    unsigned const path = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (path >= a.npaths) return; // wave-uniform; the kernel has no barrier
    dcp_dom_path const pr = a.paths[path];
    unsigned const nsteps = a.paths[path + 1u].step_off - pr.step_off;
    ProfView<Real> const pv = view_of<Real>(a, pr.slot);
    Real const *xt = (Real const *)a.xtrans + (size_t)(a.xt_per_path ? path : pr.seq) * 16u;
    uint32_t const *sw = a.words + a.woff[pr.seq];
    uint32_t const *st = (uint32_t const *)a.steps + pr.step_off; // a dcp_step is one little-endian word: id | seqlen << 16

    Real s = 0, c = 0, n = 0;  // the path's total; the open domain's core and null sums: the same in every lane
    unsigned pos = 0;          // bases the trips before this one emit
    bool open = false;         // between a B and its E
    unsigned d = 0;            // domains written
    unsigned d_begin = 0, d_seq0 = 0, d_node0 = 0; // the open domain: its B step, first base, first node
    unsigned cm = 0, ci = 0, cd = 0, cs = 0;       // its counts over the trips before this one

    for (unsigned i0 = 0; i0 < nsteps; i0 += 64u)
    {
        unsigned const i = i0 + lane;
        bool const live = i < nsteps;
        uint32_t const w = live ? st[i] : 0u, pw = live && i > 0u ? st[i - 1u] : 0u;
        unsigned const kind = (w >> 14) & 3u, x = w & 0x3fffu, len = (w >> 16) & 0xffu;
        unsigned const pkind = (pw >> 14) & 3u, pk = pw & 0x3fffu;
        unsigned inc = len; // inclusive prefix sum of the seqlens
        for (unsigned o = 1u; o < 64u; o <<= 1)
        {
            unsigned const up = (unsigned)__shfl_up((int)inc, o);
            if (lane >= o) inc += up;
        }
        unsigned const start = pos + inc - len;
        pos += lane_read(inc, 63);

        Real t = 0, e = 0, nl = 0;
        bool ok = true;
        if (live && i > 0u) ok = edge(pv, xt, pkind, pk, kind, x, &t);
        if (!ok)
        {
            t = 0;
            atomicMin(a.bad, ((u64)path << 32) | i);
        }
        if (len)
        {
            uint32_t const *p = sw + (start >> 4);
            u64 const two = ((u64)p[1] << 32) | p[0];
            uint32_t const bits = (uint32_t)(two >> (2u * (start & 15u))); // base j of the fragment in bits 2j
            unsigned v = 0;
            for (unsigned j = 0; j < 5u; ++j)
                if (j < len) v = (v << 2) | ((bits >> (2u * j)) & 3u);
            unsigned const code = (len == 1u ? 0u : len == 2u ? 4u : len == 3u ? 20u : len == 4u ? 84u : 340u) + v;
            nl = pv.en[code];
            e = kind == 0u ? pv.em[(size_t)code * pv.ldk + (x - 1u)] : kind == 1u ? pv.ei[code] : nl;
        }

        u64 const m_live = __ballot(live), m_emit = __ballot(len != 0u);
        u64 const m_b = __ballot(live && kind == 3u && x == 3u), m_e = __ballot(live && kind == 3u && x == 4u);
        u64 const m_after_b = __ballot(live && i > 0u && pkind == 3u && pk == 3u);
        u64 const m_m = __ballot(live && kind == 0u), m_i = __ballot(live && kind == 1u), m_d = __ballot(live && kind == 2u);
        u64 const m_shift = __ballot(live && kind < 2u && len != 3u);
        unsigned from = 0; // first lane of this trip that counts towards the open domain
#pragma unroll
        for (int l = 0; l < 64; ++l)
        {
            if (!((m_live >> l) & 1ull)) continue;
            bool const emits = (m_emit >> l) & 1ull;
            Real const tl = lane_read(t, l);
            Real el = 0, nll = 0;
            if (emits) el = lane_read(e, l), nll = lane_read(nl, l);
            if (l > 0 || i0 > 0u) s = s + tl;
            if (emits) s = s + el;
            if ((m_b >> l) & 1ull)
            {
                open = true;
                c = 0, n = 0;
                cm = ci = cd = cs = 0u;
                from = (unsigned)l;
                d_begin = i0 + (unsigned)l;
                d_seq0 = lane_read(start, l);
            }
            else if (open)
            {
                c = c + tl;
                if (emits) c = c + el, n = n + nll;
                if ((m_after_b >> l) & 1ull) d_node0 = lane_read(x, l);
                if ((m_e >> l) & 1ull)
                {
                    u64 const range = (l == 63 ? ~0ull : (1ull << ((l + 1) & 63)) - 1ull) & ~((1ull << from) - 1ull);
                    unsigned const seq1 = lane_read(start, l), node1 = lane_read(pk, l);
                    unsigned const nm = cm + (unsigned)__popcll(m_m & range), nin = ci + (unsigned)__popcll(m_i & range);
                    unsigned const nd = cd + (unsigned)__popcll(m_d & range), ns = cs + (unsigned)__popcll(m_shift & range);
                    size_t const at = (size_t)pr.dom_off + d;
                    unsigned const word = lane == 0u ? path : lane == 1u ? d_begin : lane == 2u ? i0 + (unsigned)l
                                        : lane == 3u ? d_seq0 : lane == 4u ? seq1 : lane == 5u ? d_node0 : lane == 6u ? node1
                                        : lane == 7u ? nm : lane == 8u ? nin : lane == 9u ? nd : lane == 10u ? ns : 0u;
                    if (lane < 12u) a.dom_out[at * 12u + lane] = word;
                    if (lane == 0u) ((Real *)a.core_out)[at] = c, ((Real *)a.null_out)[at] = n;
                    open = false;
                    ++d;
                }
            }
        }
        if (open) // the domain goes on in the next trip: this trip's share of its counts
        {
            u64 const range = m_live & ~((1ull << from) - 1ull);
            cm += (unsigned)__popcll(m_m & range), ci += (unsigned)__popcll(m_i & range);
            cd += (unsigned)__popcll(m_d & range), cs += (unsigned)__popcll(m_shift & range);
        }
    }
    if (lane == 0u && a.total_out) ((Real *)a.total_out)[path] = s;
}

} // namespace

extern "C" int dcp_launch_domains(dcp_domains_args const *args, int f64, void *stream)
{
    if (!args || args->npaths == 0) return (int)hipErrorInvalidValue;
    unsigned const blocks = (args->npaths + kWaves - 1u) / kWaves;
    hipStream_t const s = (hipStream_t)stream;
    if (f64) domains_kernel<double><<<blocks, kBlock, 0, s>>>(*args);
    else domains_kernel<float><<<blocks, kBlock, 0, s>>>(*args);
    return (int)hipGetLastError();
}
