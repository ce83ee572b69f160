// dcp_f64.hip -- gfx950 kernels of the double build (the reference's IMM_DOUBLE_PRECISION).
//
//  expand64_kernel      frame-state emission tables of an f64 DB, in double: one column (one nuclt_dist) per lane,
//                       four words per block row, code-major / node-contiguous as the float tables.
//  viterbi64_kernel<R>  null + alt Viterbi of one (profile, query) pair per wavefront in double, R = 1, 2 or 4
//                       consecutive nodes per lane.  A profile wider than 256 nodes is swept in column segments of
//                       256 nodes over all rows, one after the other; what row j of the next segment needs from
//                       this one (M, I, D of its last node, E so far) goes through a per-wavefront column in global
//                       memory, as viterbi_segment_kernel's does.
//  viterbi64_kernel<R, true>  the traceback's forward pass: the same sweep over a list of pairs, every row's M, I, D
//                       and N, B, E, J, C written to the pair's work area instead of a score (dcp_f64_trace_args).
//  viterbi64_kernel<R, false, true>  the same sweep over a pair list that was filled on the device: the redo list
//                       of the query-lane kernel (dcp_f64_qlane.hip), scores and hits written as the grid mode's.
//  trace64_kernel       the walk back from T(L) to S(0) on that work area, one wavefront per hit.
//
// Arithmetic contract: the recursion of the CPU oracle's double build, operation by operation --
// every candidate is (predecessor + transition) or (predecessor + emission) formed once in IEEE double, combined
// with max only; no FMA (-ffp-contract=off), no reassociation.  max is exact, so the order of its operands changes
// nothing; the sums are the oracle's sums.  The delete chain D_k = max(M_{k-1} + MD_k, D_{k-1} + DD_k) runs
// sequentially inside a lane and to its fixed point across lanes (the float kernels' construction): the fixed point
// is the sequential recurrence's unique solution, each D_k the same max of the same two sums.
//
// B(j) = max(N(j) + NB, E(j) + EB, J(j) + JB) needs E(j) over the WHOLE profile, which a segment does not have.  The
// segmented sweep takes B as given: the first pass uses N(j) + NB; the last segment, which has the final E(j) and
// J(j), recomputes B(j) from them and keeps it in the column.  If it equals the B the pass used in every row, the pass
// was the exact recursion (row by row: exact rows before j make E(j), J(j) and so B(j) exact); otherwise the pass is
// repeated with the B the last segment found.  The first row whose B was wrong is exact in the next pass, so the
// passes end.  A uni-hit scan never needs a second one: there EJ = -inf, so E(j) + EB and J(j) + JB are -inf.
#include "dcp_f64.h"

#include <hip/hip_runtime.h>

namespace
{

__device__ __forceinline__ double ninf() { return -__builtin_inf(); }

// gfx950's DPP moves 32-bit lanes: a double crosses lanes as its two halves (two v_mov_b32_dpp)
__device__ __forceinline__ double shr1(double v, double first) // value of lane - 1; lane 0 receives `first`
{
    unsigned long long const vb = __builtin_bit_cast(unsigned long long, v);
    unsigned long long const fb = __builtin_bit_cast(unsigned long long, first);
    int const lo = __builtin_amdgcn_update_dpp((int)(unsigned)fb, (int)(unsigned)vb, 0x138 /*wave_shr:1*/, 0xf, 0xf, false);
    int const hi = __builtin_amdgcn_update_dpp((int)(unsigned)(fb >> 32), (int)(unsigned)(vb >> 32), 0x138, 0xf, 0xf, false);
    return __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

__device__ __forceinline__ double readlane(double v, int lane)
{
    unsigned long long const b = __builtin_bit_cast(unsigned long long, v);
    unsigned const lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, lane);
    unsigned const hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), lane);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
        v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// finite, tested on the encoding (the library is built with -fno-honor-nans)
__device__ __forceinline__ bool finite64(double v)
{
    return (__builtin_bit_cast(unsigned long long, v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// ---- frame-state emission in double (imm frame state): the probability-domain formula of
// dcp_frame_table_host, not rounded to float.  b = base probabilities, c3 = codon marginals (index 4 = wildcard).
__device__ double frame64(double const *dist, double e, unsigned code)
{
    unsigned len, v;
    if (code < 4) len = 1, v = code;
    else if (code < 20) len = 2, v = code - 4;
    else if (code < 84) len = 3, v = code - 20;
    else if (code < 340) len = 4, v = code - 84;
    else len = 5, v = code - 340;
    int x[5];
    for (unsigned i = 0; i < len; ++i)
        x[i] = (int)((v >> (2 * (len - 1 - i))) & 3u);
    double const f = 1.0 - e, e2 = e * e, f2 = f * f;
    auto b = [&](int i) { return exp(dist[i]); };
    auto c3 = [&](int p, int q, int r) { return exp(dist[4 + p * 25 + q * 5 + r]); };
    auto s1 = [&](int p) { return c3(p, 4, 4) + c3(4, p, 4) + c3(4, 4, p); };
    auto s2 = [&](int p, int q) { return c3(4, p, q) + c3(p, 4, q) + c3(p, q, 4); };
    double p;
    if (len == 1) p = e2 * f2 / 3.0 * s1(x[0]);
    else if (len == 2)
        p = 2.0 * e * f2 * f / 3.0 * s2(x[0], x[1]) + e2 * e * f / 3.0 * (b(x[1]) * s1(x[0]) + b(x[0]) * s1(x[1]));
    else if (len == 3)
        p = f2 * f2 * c3(x[0], x[1], x[2]) +
            4.0 * e2 * f2 / 9.0 * (b(x[0]) * s2(x[1], x[2]) + b(x[1]) * s2(x[0], x[2]) + b(x[2]) * s2(x[0], x[1])) +
            e2 * e2 / 9.0 * (b(x[0]) * b(x[1]) * s1(x[2]) + b(x[0]) * b(x[2]) * s1(x[1]) + b(x[1]) * b(x[2]) * s1(x[0]));
    else if (len == 4)
    {
        double const one = b(x[0]) * c3(x[1], x[2], x[3]) + b(x[1]) * c3(x[0], x[2], x[3]) +
                           b(x[2]) * c3(x[0], x[1], x[3]) + b(x[3]) * c3(x[0], x[1], x[2]);
        double two = 0;
        for (int i = 0; i < 4; ++i)
            for (int j = i + 1; j < 4; ++j)
            {
                int r[2], n = 0;
                for (int k = 0; k < 4; ++k)
                    if (k != i && k != j) r[n++] = x[k];
                two += b(x[i]) * b(x[j]) * s2(r[0], r[1]);
            }
        p = e * f2 * f / 2.0 * one + e2 * e * f / 9.0 * two;
    }
    else
    {
        double s = 0;
        for (int i = 0; i < 5; ++i)
            for (int j = i + 1; j < 5; ++j)
            {
                int r[3], n = 0;
                for (int k = 0; k < 5; ++k)
                    if (k != i && k != j) r[n++] = x[k];
                s += b(x[i]) * b(x[j]) * c3(r[0], r[1], r[2]);
            }
        p = e2 * f2 / 10.0 * s;
    }
    return log(p);
}

__global__ __launch_bounds__(256) void expand64_kernel(dcp_f64_expand_job const *__restrict__ jobs, unsigned njobs,
                                                       double const *__restrict__ dists, double *__restrict__ out)
{
    unsigned const job = blockIdx.x * 64u + (threadIdx.x & 63u);
    unsigned const code = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (job >= njobs || code >= (unsigned)DCP_NCODES) return;
    dcp_f64_expand_job const jb = jobs[job];
    double const v = jb.dist == ~0u ? ninf() : frame64(dists + (size_t)DCP_NDIST * jb.dist, jb.eps, code);
    out[jb.out_off + (uint64_t)code * jb.stride] = v;
}

// ---- the f64 row sweep -------------------------------------------------------------------------------------------
template <int R> struct Trans64
{
    double ent[R], mm[R], im[R], dm[R], md[R], dd[R], mi[R], ii[R];
};

struct X64 // the pair's special transitions
{
    double RR, SB, SN, NN, NB, ET, EC, CC, CT, EB, EJ, JJ, JB;
};

// history rings: row j's predecessors j - 1 .. j - 5 live in slots (j - l) % 5; PM = max over the edges INTO M_k
// (the transition added, the emission not yet), QI likewise for I_k; the specials as their own rings
template <int R> struct State64
{
    double P[5][R], Q[5][R];
    double PN[5], PJ[5], PC[5], PR[5];
    double E, Cc, Rr;
    unsigned w; // the last five bases, two bits each
};

struct Seg64
{
    double const *tcol; // this lane's first column of the match table (row 0)
    uint64_t ldk;
    double const *ei, *en;
    uint32_t const *words;
    double *col;     // the pair's boundary column (segmented sweep), 5 doubles per row: m, i, d, e, B
    bool first_seg, last_seg, multi, first_pass;
    // TRACE: this lane's first column of the M matrix (row 0), the matrices' and vectors' lengths, N of row 0
    double *wm, *wspec;
    uint64_t wmat, wrows;
};

template <int R> __device__ __forceinline__ void chain_rest(double const (&a)[R], double (&d)[R], double const (&dd)[R])
{
#pragma unroll
    for (int r = 1; r < R; ++r)
        d[r] = fmax(a[r], d[r - 1] + dd[r]);
}

template <int R, int PH, bool TRACE>
__device__ __forceinline__ void row64(State64<R> &s, Trans64<R> const &t, X64 const &x, Seg64 const &g, unsigned j,
                                      unsigned lane, bool &changed)
{
    constexpr int sl[5] = {(PH + 4) % 5, (PH + 3) % 5, (PH + 2) % 5, (PH + 1) % 5, PH}; // slot of row j - l
    constexpr unsigned off[5] = {0u, 4u, 20u, 84u, 340u};
    unsigned const i = j - 1u;
    s.w = ((s.w << 2) | ((g.words[i >> 4] >> ((i & 15u) * 2u)) & 3u)) & 1023u;

    // emitting states: max over the word lengths of predecessor(j - l) + emission (words that would start before
    // row 0 meet -inf predecessors: the rings start as -inf)
    double m[R], ins[R];
#pragma unroll
    for (int r = 0; r < R; ++r)
        m[r] = ins[r] = ninf();
    double N = ninf(), J = ninf(), Cc = ninf(), Rr = ninf();
#pragma unroll
    for (int l = 0; l < 5; ++l)
    {
        unsigned const code = off[l] + (s.w & ((4u << (2 * l)) - 1u));
        double const eI = g.ei[code], eN = g.en[code];
        double const *em = g.tcol + (uint64_t)code * g.ldk;
        double e[R];
        if constexpr (R == 1) e[0] = em[0];
        else
        {
#pragma unroll
            for (int r = 0; r < R; r += 2)
            {
                double2 const v = *(double2 const *)(em + r);
                e[r] = v.x, e[r + 1] = v.y;
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
        {
            m[r] = fmax(m[r], s.P[sl[l]][r] + e[r]);
            ins[r] = fmax(ins[r], s.Q[sl[l]][r] + eI);
        }
        N = fmax(N, s.PN[sl[l]] + eN);
        J = fmax(J, s.PJ[sl[l]] + eN);
        Cc = fmax(Cc, s.PC[sl[l]] + eN);
        Rr = fmax(Rr, s.PR[sl[l]] + eN);
    }

    // the previous segment's last node in this row (lane 63 wrote it there and reads it back: one thread)
    double bm = ninf(), bi = ninf(), bd = ninf(), be = ninf();
    double *const cj = g.col + (uint64_t)j * 5u;
    if (!g.first_seg)
    {
        double v0 = 0, v1 = 0, v2 = 0, v3 = 0;
        if (lane == 63u) v0 = cj[0], v1 = cj[1], v2 = cj[2], v3 = cj[3];
        bm = readlane(v0, 63), bi = readlane(v1, 63), bd = readlane(v2, 63), be = readlane(v3, 63);
    }

    // delete chain: sequential in the lane, to the fixed point across lanes
    double a[R], d[R];
    a[0] = shr1(m[R - 1], bm) + t.md[0];
#pragma unroll
    for (int r = 1; r < R; ++r)
        a[r] = m[r - 1] + t.md[r];
    d[0] = fmax(a[0], shr1(ninf(), bd) + t.dd[0]);
    chain_rest<R>(a, d, t.dd);
    for (;;)
    {
        double const d0 = fmax(a[0], shr1(d[R - 1], bd) + t.dd[0]);
        if (!__any(d0 != d[0])) break;
        d[0] = d0;
        chain_rest<R>(a, d, t.dd);
    }

    // E(j): exit scores are 0 (protein_model.c:441-458); D of the profile's first node is -inf
    double el = fmax(m[0], d[0]);
#pragma unroll
    for (int r = 1; r < R; ++r)
        el = fmax(el, fmax(m[r], d[r]));
    double const E = fmax(wave_max(el), be);

    double const nb = N + x.NB;
    double B;
    if (!g.multi) B = fmax(fmax(nb, E + x.EB), J + x.JB);
    else
    {
        double bu = 0;
        if (!g.first_pass && lane == 63u) bu = cj[4];
        B = g.first_pass ? nb : readlane(bu, 63);
        if (g.last_seg)
        {
            double const bt = fmax(fmax(nb, E + x.EB), J + x.JB);
            if (bt != B) changed = true;
            if (lane == 63u) cj[4] = bt;
        }
    }

    // row j's edges into the next rows
    double const mp = shr1(m[R - 1], bm), ip = shr1(ins[R - 1], bi), dp = shr1(d[R - 1], bd);
    s.P[PH][0] = fmax(fmax(B + t.ent[0], mp + t.mm[0]), fmax(ip + t.im[0], dp + t.dm[0]));
#pragma unroll
    for (int r = 1; r < R; ++r)
        s.P[PH][r] = fmax(fmax(B + t.ent[r], m[r - 1] + t.mm[r]), fmax(ins[r - 1] + t.im[r], d[r - 1] + t.dm[r]));
#pragma unroll
    for (int r = 0; r < R; ++r)
        s.Q[PH][r] = fmax(m[r] + t.mi[r], ins[r] + t.ii[r]);
    s.PN[PH] = N + x.NN;
    s.PJ[PH] = fmax(E + x.EJ, J + x.JJ);
    s.PC[PH] = fmax(E + x.EC, Cc + x.CC);
    s.PR[PH] = Rr + x.RR;
    s.E = E, s.Cc = Cc, s.Rr = Rr;

    if (g.multi && !g.last_seg && lane == 63u)
        cj[0] = m[R - 1], cj[1] = ins[R - 1], cj[2] = d[R - 1], cj[3] = E;

    // the traceback's work area: this segment's columns; the specials only where they are final (the last segment:
    // its E(j) is over the whole profile, its B(j) the one this pass used, and J, C follow from that E)
    if constexpr (TRACE)
    {
        double *const w = g.wm + (uint64_t)j * g.ldk;
#pragma unroll
        for (int r = 0; r < R; ++r)
            w[r] = m[r], w[g.wmat + r] = ins[r], w[2u * g.wmat + r] = d[r];
        if (g.last_seg && lane == 0u)
        {
            double *const sp = g.wspec + j;
            sp[0] = N, sp[g.wrows] = B, sp[2u * g.wrows] = E, sp[3u * g.wrows] = J, sp[4u * g.wrows] = Cc;
        }
    }
}

template <bool TRACE, bool PAIRS = false> struct Args64
{
    using T = dcp_f64_scan_args;
};
template <> struct Args64<true, false>
{
    using T = dcp_f64_trace_args;
};
template <> struct Args64<false, true>
{
    using T = dcp_f64_pairs_args;
};

// TRACE: the traceback's forward pass (dcp_f64_trace_args): pair i of the list writes every row to its work area
// and its alt score to trace_alt[i]; every fixed-point pass rewrites all rows, so the last one leaves the exact
// recursion there.  PAIRS: a scan of a pair list whose length is read on the device (dcp_f64_pairs_args) -- the
// query-lane kernel's redo list: scores, filter and hits as the grid mode's, the special transitions those of the
// pair's QUERY, boundary columns per wavefront as in the other modes.  The grid mode's instantiations (neither)
// are the code they were before the other two existed.
template <int R, bool TRACE = false, bool PAIRS = false>
__global__ __launch_bounds__(256) void viterbi64_kernel(typename Args64<TRACE, PAIRS>::T a)
{
    unsigned const lane = threadIdx.x & 63u;
    uint64_t const gw = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    uint64_t const nw = a.nwaves;
    if (gw >= nw) return; // the grid's last block may hold wavefronts past nwaves: they have no boundary column
    uint64_t npairs;
    if constexpr (TRACE) npairs = a.npairs;
    else if constexpr (PAIRS)
    {
        unsigned const n = *a.npairs_dev; // counts on past the capacity when the list overflowed
        npairs = n < a.pair_cap ? n : a.pair_cap;
    }
    else npairs = (uint64_t)a.nprof * a.nq;
    double *const col = a.col ? a.col + gw * a.col_stride : nullptr;
    for (uint64_t pair = gw; pair < npairs; pair += nw)
    {
        unsigned pi, q;
        if constexpr (TRACE || PAIRS)
        {
            dcp_f64_pair const pp = a.pairs[pair];
            pi = pp.prof, q = pp.q;
        }
        else pi = (unsigned)(pair / a.nq), q = (unsigned)(pair % a.nq);
        dcp_f64_prof const pr = a.profs[pi];
        unsigned const L = a.seq_len[q];
        double const *xt = a.xtrans + (size_t)(TRACE ? pair : q) * DCP_F64_XSTRIDE;
        X64 const x{xt[DCP_X_RR], xt[DCP_X_SB], xt[DCP_X_SN], xt[DCP_X_NN], xt[DCP_X_NB], xt[DCP_X_ET], xt[DCP_X_EC],
                    xt[DCP_X_CC], xt[DCP_X_CT], xt[DCP_X_EB], xt[DCP_X_EJ], xt[DCP_X_JJ], xt[DCP_X_JB]};
        Seg64 g;
        g.ldk = pr.ldk;
        g.ei = a.xe + pr.xe_off;
        g.en = g.ei + DCP_NCODES;
        g.words = a.seq_words + a.seq_woff[q];
        g.col = col;
        g.multi = pr.nseg > 1u;
        double null_ll = 0, alt_ll = 0;
        for (bool first_pass = true;; first_pass = false)
        {
            bool changed = false;
            for (unsigned seg = 0; seg < pr.nseg; ++seg)
            {
                unsigned const c0 = seg * 64u * R + lane * R; // this lane's first column
                g.tcol = a.tab + pr.tab_off + c0;
                g.first_seg = seg == 0u;
                g.last_seg = seg + 1u == pr.nseg;
                g.first_pass = first_pass;
                Trans64<R> t;
                double const *tb = a.trans + pr.trans_off + c0;
#pragma unroll
                for (int r = 0; r < R; ++r)
                {
                    t.ent[r] = tb[DCP_T_ENTRY * g.ldk + r];
                    t.mm[r] = tb[DCP_T_MM * g.ldk + r];
                    t.im[r] = tb[DCP_T_IM * g.ldk + r];
                    t.dm[r] = tb[DCP_T_DM * g.ldk + r];
                    t.md[r] = tb[DCP_T_MD * g.ldk + r];
                    t.dd[r] = tb[DCP_T_DD * g.ldk + r];
                    t.mi[r] = tb[DCP_T_MI * g.ldk + r];
                    t.ii[r] = tb[DCP_T_II * g.ldk + r];
                }
                // row 0: S = 0, B = S + SB; N = S + SN; R starts at 0
                State64<R> s;
#pragma unroll
                for (int h = 0; h < 5; ++h)
                {
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        s.P[h][r] = s.Q[h][r] = ninf();
                    s.PN[h] = s.PJ[h] = s.PC[h] = s.PR[h] = ninf();
                }
                double const B0 = 0.0 + x.SB;
#pragma unroll
                for (int r = 0; r < R; ++r)
                    s.P[0][r] = B0 + t.ent[r];
                if constexpr (TRACE) // row 0: M, I, D, N, E, J, C are -inf, B = S + SB
                {
                    double *const work = a.trace_work + a.trace_woff[pair];
                    g.wrows = (uint64_t)L + 1u;
                    g.wmat = g.wrows * pr.ldk;
                    g.wm = work + c0;
                    g.wspec = work + 3u * g.wmat;
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        g.wm[r] = ninf(), g.wm[g.wmat + r] = ninf(), g.wm[2u * g.wmat + r] = ninf();
                    if (g.last_seg && lane == 0u)
                        g.wspec[0] = ninf(), g.wspec[g.wrows] = B0, g.wspec[2u * g.wrows] = ninf(),
                        g.wspec[3u * g.wrows] = ninf(), g.wspec[4u * g.wrows] = ninf();
                }
                s.PN[0] = 0.0 + x.SN;
                s.PR[0] = 0.0;
                s.E = s.Cc = s.Rr = ninf();
                s.w = 0u;
                unsigned j = 1u;
#define DCP_ROW64(PH)                                                                                                  \
    row64<R, PH, TRACE>(s, t, x, g, j, lane, changed);                                                                        \
    if (j == L) break;                                                                                                 \
    ++j;
                for (;;)
                {
                    DCP_ROW64(1)
                    DCP_ROW64(2)
                    DCP_ROW64(3)
                    DCP_ROW64(4)
                    DCP_ROW64(0)
                }
#undef DCP_ROW64
                null_ll = s.Rr;
                alt_ll = fmax(s.E + x.ET, s.Cc + x.CT);
            }
            if (!changed) break;
        }
        if constexpr (TRACE)
        {
            if (lane == 0u) a.trace_alt[pair] = alt_ll;
            continue;
        }
        if (lane == 0u)
        {
            if (a.out_null)
            {
                a.out_null[(size_t)q * a.nprof_total + pr.pidx] = null_ll;
                a.out_alt[(size_t)q * a.nprof_total + pr.pidx] = alt_ll;
            }
            // xmath_lrt in double; scan_thread.c:121-123 keeps a pair iff the LRT is finite and >= threshold
            double const lrt = -2 * (null_ll - alt_ll);
            if (finite64(lrt) && lrt >= a.lrt_threshold)
            {
                unsigned const k = atomicAdd(a.nhits, 1u);
                if (k < a.hit_cap) a.hits[k] = dcp_hit64{a.q_base + q, pr.pidx, null_ll, alt_ll};
            }
        }
    }
}

// ---- the walk back ----------------------------------------------------------------------------------------------
// viterbi_trace_kernel's walk (dcp_kernels.hip), restated on double values and the f64 DB's layout: lane 0 walks
// from T(L) to S(0) re-deriving each arg-max from the stored rows -- first maximum wins, candidates in the order
// the reference wires the transitions (protein_model.c:460-500, :322-340), which is also the oracle's.  Each
// candidate is the sum the forward pass formed (predecessor + transition, then + emission), so a recomputed maximum
// is the stored value to the bit.
struct View64
{
    double const *Mv, *Iv, *Dv;      // [L + 1][ld]
    double const *N, *B, *E, *J, *C; // [L + 1]
    double const *ent, *mm, *im, *dm, *md, *dd, *mi, *ii;
    double const *eM, *eI, *eN;
    double const *xt;
    uint32_t const *words;
    uint64_t ld; // the DB's columns of the profile: row length of its tables and of the work matrices
    unsigned M, L;
};

__device__ __forceinline__ unsigned code64(unsigned w, unsigned l) // word of the last l bases of window w
{
    constexpr unsigned off[5] = {0u, 4u, 20u, 84u, 340u};
    return off[l - 1u] + (w & ((1u << (2u * l)) - 1u));
}

__device__ __forceinline__ unsigned window64(uint32_t const *words, unsigned j) // the (up to) 5 bases before row j
{
    unsigned w = 0;
    for (unsigned p = j > 5u ? j - 5u : 0u; p < j; ++p)
        w = (w << 2) | ((words[p >> 4] >> ((p & 15u) * 2u)) & 3u);
    return w & 1023u;
}

// P_k(jj): best predecessor of M_k leaving row jj; *arg: 0 = M_{k-1}, 1 = I_{k-1}, 2 = D_{k-1}, 3 = B
__device__ double walk_P(View64 const &v, uint64_t jj, unsigned k, int *arg)
{
    double best = ninf();
    int a = -1;
    if (k > 0)
    {
        uint64_t const o = jj * v.ld + k - 1u;
        double const c0 = v.Mv[o] + v.mm[k], c1 = v.Iv[o] + v.im[k], c2 = v.Dv[o] + v.dm[k];
        if (c0 > best) best = c0, a = 0;
        if (c1 > best) best = c1, a = 1;
        if (c2 > best) best = c2, a = 2;
    }
    double const cb = v.B[jj] + v.ent[k];
    if (cb > best) best = cb, a = 3;
    if (arg) *arg = a;
    return best;
}

// Q_k(jj): best predecessor of I_k; *arg: 0 = M_k, 1 = I_k
__device__ double walk_Q(View64 const &v, uint64_t jj, unsigned k, int *arg)
{
    uint64_t const o = jj * v.ld + k;
    double best = ninf();
    int a = -1;
    double const c0 = v.Mv[o] + v.mi[k], c1 = v.Iv[o] + v.ii[k];
    if (c0 > best) best = c0, a = 0;
    if (c1 > best) best = c1, a = 1;
    if (arg) *arg = a;
    return best;
}

// predecessor maxima of the special emitting states; *arg: 0 = first source, 1 = self loop
__device__ double walk_PN(View64 const &v, uint64_t jj, int *arg)
{
    double best = ninf();
    int a = -1;
    double const c0 = (jj == 0 ? 0.0 : ninf()) + v.xt[DCP_X_SN], c1 = v.N[jj] + v.xt[DCP_X_NN];
    if (c0 > best) best = c0, a = 0;
    if (c1 > best) best = c1, a = 1;
    if (arg) *arg = a;
    return best;
}
__device__ double walk_PJ(View64 const &v, uint64_t jj, int *arg)
{
    double best = ninf();
    int a = -1;
    double const c0 = v.E[jj] + v.xt[DCP_X_EJ], c1 = v.J[jj] + v.xt[DCP_X_JJ];
    if (c0 > best) best = c0, a = 0;
    if (c1 > best) best = c1, a = 1;
    if (arg) *arg = a;
    return best;
}
__device__ double walk_PC(View64 const &v, uint64_t jj, int *arg)
{
    double best = ninf();
    int a = -1;
    double const c0 = v.E[jj] + v.xt[DCP_X_EC], c1 = v.C[jj] + v.xt[DCP_X_CC];
    if (c0 > best) best = c0, a = 0;
    if (c1 > best) best = c1, a = 1;
    if (arg) *arg = a;
    return best;
}

__global__ __launch_bounds__(64) void trace64_kernel(dcp_f64_walk_args a)
{
    unsigned const h = blockIdx.x;
    if (h >= a.nhits || threadIdx.x != 0u) return; // lane 0 walks; the wavefront is one per hit
    dcp_f64_pair const pp = a.pairs[h];
    dcp_f64_prof const pr = a.profs[pp.prof];
    unsigned const q = pp.q;
    View64 v;
    v.ld = pr.ldk;
    v.M = pr.core_size;
    v.L = a.seq_len[q];
    v.words = a.seq_words + a.seq_woff[q];
    v.xt = a.xtrans + (uint64_t)h * DCP_F64_XSTRIDE;
    double const *tb = a.trans + pr.trans_off;
    v.ent = tb + DCP_T_ENTRY * v.ld, v.mm = tb + DCP_T_MM * v.ld, v.im = tb + DCP_T_IM * v.ld;
    v.dm = tb + DCP_T_DM * v.ld, v.md = tb + DCP_T_MD * v.ld, v.dd = tb + DCP_T_DD * v.ld;
    v.mi = tb + DCP_T_MI * v.ld, v.ii = tb + DCP_T_II * v.ld;
    v.eM = a.tab + pr.tab_off;
    v.eI = a.xe + pr.xe_off;
    v.eN = v.eI + DCP_NCODES;
    unsigned const L = v.L;
    uint64_t const rows = (uint64_t)L + 1u, mat = rows * v.ld;
    double *const work = a.work + a.work_off[h];
    v.Mv = work, v.Iv = work + mat, v.Dv = work + 2u * mat;
    v.N = work + 3u * mat, v.B = v.N + rows, v.E = v.B + rows, v.J = v.E + rows, v.C = v.J + rows;
    dcp_step *const out = a.steps + a.step_off[h];
    unsigned const cap = a.step_off[h + 1] - a.step_off[h];
    double const ni = ninf();

    // ---- null model (one state R, protein_model.c:223-225, 316-320): its recursion here, then its walk
    if (a.null_model)
    {
        double *const Rv = work; // [L + 1]
        Rv[0] = ni;
        auto PR = [&](unsigned jj) { return jj == 0 ? 0.0 : Rv[jj] + v.xt[DCP_X_RR]; };
        for (unsigned j = 1; j <= L; ++j)
        {
            unsigned const w = window64(v.words, j);
            double r = ni;
            for (unsigned l = 1; l <= (j < 5u ? j : 5u); ++l)
                r = fmax(r, PR(j - l) + v.eN[code64(w, l)]);
            Rv[j] = r;
        }
        a.alt_out[h] = Rv[L];
        unsigned n = 0, j = L;
        bool ok = Rv[L] > ni;
        while (ok && j > 0)
        {
            unsigned const w = window64(v.words, j);
            double best = ni;
            unsigned bl = 0;
            for (unsigned l = 1; l <= (j < 5u ? j : 5u); ++l)
            {
                double const sc = PR(j - l) + v.eN[code64(w, l)];
                if (sc > best) best = sc, bl = l;
            }
            if (bl == 0) { ok = false; break; }
            if (n < cap) out[n] = dcp_step{(uint16_t)(3u << 14), (uint8_t)bl, 0};
            ++n;
            j -= bl;
        }
        unsigned const m = n < cap ? n : cap;
        for (unsigned i = 0; i < m / 2; ++i)
        {
            dcp_step const t = out[i];
            out[i] = out[m - 1 - i];
            out[m - 1 - i] = t;
        }
        a.nsteps[h] = ok ? n : DCP_F64_TRACE_NO_PATH;
        return;
    }

    double const alt = fmax(v.E[L] + v.xt[DCP_X_ET], v.C[L] + v.xt[DCP_X_CT]);
    a.alt_out[h] = alt;
    unsigned n = 0;
    bool ok = alt > ni, too_long = false;
    enum { ST_S = 1, ST_N, ST_B, ST_E, ST_J, ST_C, ST_T, ST_M, ST_I, ST_D };
    int st = ST_T;
    unsigned k = 0, j = L;
    auto push = [&](unsigned id, unsigned len) {
        if (n < cap) out[n] = dcp_step{(uint16_t)id, (uint8_t)len, 0};
        if (++n == DCP_F64_TRACE_TOO_LONG) too_long = true, ok = false; // an error, never a wrap into the sentinels
    };
    unsigned const EXT = 3u << 14;
    // a path has at most L emitting steps and, per domain (at most L of them), M + 1 silent core steps and B, E, J
    uint64_t guard = 0;
    uint64_t const max_steps = ((uint64_t)L + 1u) * (v.M + 4u) + 64u;
    while (ok && guard++ < max_steps)
    {
        if (st == ST_T)
        {
            push(EXT | 7u, 0);
            double const c0 = v.E[j] + v.xt[DCP_X_ET], c1 = v.C[j] + v.xt[DCP_X_CT];
            st = !(c1 > c0) ? ST_E : ST_C; // E -> T was wired first
        }
        else if (st == ST_E)
        {
            push(EXT | 4u, 0);
            // M_M, M_1 .. M_{M-1}, D_2 .. D_M (1-based): protein_model.c:494, :441-458
            double best = ni;
            int bs = -1;
            unsigned bk = 0;
            double const *Mj = v.Mv + (uint64_t)j * v.ld, *Dj = v.Dv + (uint64_t)j * v.ld;
            double c = Mj[v.M - 1] + 0.0;
            if (c > best) best = c, bs = ST_M, bk = v.M - 1;
            for (unsigned kk = 0; kk + 1 < v.M; ++kk)
            {
                c = Mj[kk] + 0.0;
                if (c > best) best = c, bs = ST_M, bk = kk;
            }
            for (unsigned kk = 1; kk < v.M; ++kk)
            {
                c = Dj[kk] + 0.0;
                if (c > best) best = c, bs = ST_D, bk = kk;
            }
            if (bs < 0) ok = false;
            st = bs, k = bk;
        }
        else if (st == ST_M || st == ST_I || st == ST_N || st == ST_J || st == ST_C)
        {
            unsigned const w = window64(v.words, j);
            unsigned const maxl = j < 5u ? j : 5u;
            double best = ni;
            unsigned bl = 0;
            for (unsigned l = 1; l <= maxl; ++l)
            {
                unsigned const c = code64(w, l);
                double sc;
                if (st == ST_M) sc = walk_P(v, j - l, k, nullptr) + v.eM[(uint64_t)c * v.ld + k];
                else if (st == ST_I) sc = walk_Q(v, j - l, k, nullptr) + v.eI[c];
                else if (st == ST_N) sc = walk_PN(v, j - l, nullptr) + v.eN[c];
                else if (st == ST_J) sc = walk_PJ(v, j - l, nullptr) + v.eN[c];
                else sc = walk_PC(v, j - l, nullptr) + v.eN[c];
                if (sc > best) best = sc, bl = l;
            }
            if (bl == 0) { ok = false; break; }
            int arg = -1;
            if (st == ST_M)
            {
                push(k + 1u, bl);
                walk_P(v, j - bl, k, &arg);
                j -= bl;
                if (arg == 0) st = ST_M, k = k - 1;
                else if (arg == 1) st = ST_I, k = k - 1;
                else if (arg == 2) st = ST_D, k = k - 1;
                else if (arg == 3) st = ST_B;
                else ok = false;
            }
            else if (st == ST_I)
            {
                push((1u << 14) | (k + 1u), bl);
                walk_Q(v, j - bl, k, &arg);
                j -= bl;
                if (arg == 0) st = ST_M;
                else if (arg == 1) st = ST_I;
                else ok = false;
            }
            else if (st == ST_N)
            {
                push(EXT | 2u, bl);
                walk_PN(v, j - bl, &arg);
                j -= bl;
                st = arg == 0 ? ST_S : ST_N;
                if (arg < 0) ok = false;
            }
            else if (st == ST_J)
            {
                push(EXT | 5u, bl);
                walk_PJ(v, j - bl, &arg);
                j -= bl;
                st = arg == 0 ? ST_E : ST_J;
                if (arg < 0) ok = false;
            }
            else
            {
                push(EXT | 6u, bl);
                walk_PC(v, j - bl, &arg);
                j -= bl;
                st = arg == 0 ? ST_E : ST_C;
                if (arg < 0) ok = false;
            }
        }
        else if (st == ST_D)
        {
            push((2u << 14) | (k + 1u), 0);
            if (k == 0) { ok = false; break; }
            uint64_t const o = (uint64_t)j * v.ld + k - 1u;
            double const c0 = v.Mv[o] + v.md[k], c1 = v.Dv[o] + v.dd[k];
            st = !(c1 > c0) ? ST_M : ST_D; // M_{k-1} -> D_k was wired first
            k = k - 1;
        }
        else if (st == ST_B)
        {
            push(EXT | 3u, 0);
            // S -> B, N -> B, E -> B, J -> B (protein_model.c:324-337)
            double best = ni;
            int bs = -1;
            double c = (j == 0 ? 0.0 : ni) + v.xt[DCP_X_SB];
            if (c > best) best = c, bs = ST_S;
            c = v.N[j] + v.xt[DCP_X_NB];
            if (c > best) best = c, bs = ST_N;
            c = v.E[j] + v.xt[DCP_X_EB];
            if (c > best) best = c, bs = ST_E;
            c = v.J[j] + v.xt[DCP_X_JB];
            if (c > best) best = c, bs = ST_J;
            if (bs < 0) ok = false;
            st = bs;
        }
        else // ST_S
        {
            push(EXT | 1u, 0);
            if (j != 0) ok = false;
            break;
        }
    }
    if (st != ST_S) ok = false;
    unsigned const m = n < cap ? n : cap;
    for (unsigned i = 0; i < m / 2; ++i)
    {
        dcp_step const t = out[i];
        out[i] = out[m - 1 - i];
        out[m - 1 - i] = t;
    }
    a.nsteps[h] = ok ? n : too_long ? DCP_F64_TRACE_TOO_LONG : DCP_F64_TRACE_NO_PATH;
}

} // namespace

extern "C" void dcp_f64_launch_expand(dcp_f64_expand_job const *jobs, unsigned njobs, double const *dists, double *out,
                                      void *stream)
{
    if (njobs == 0) return;
    dim3 const grid((njobs + 63u) / 64u, (DCP_NCODES + 3) / 4);
    hipLaunchKernelGGL(expand64_kernel, grid, dim3(256), 0, (hipStream_t)stream, jobs, njobs, dists, out);
}

extern "C" int dcp_f64_launch_scan(int R, dcp_f64_scan_args const *a, unsigned nwaves, void *stream)
{
    unsigned const blocks = (unsigned)(((uint64_t)nwaves + 3u) / 4u);
    if (blocks == 0) return 0;
    hipStream_t const st = (hipStream_t)stream;
    dcp_f64_scan_args b = *a;
    b.nwaves = nwaves;
    switch (R)
    {
    case 1: hipLaunchKernelGGL(viterbi64_kernel<1>, dim3(blocks), dim3(256), 0, st, b); return 0;
    case 2: hipLaunchKernelGGL(viterbi64_kernel<2>, dim3(blocks), dim3(256), 0, st, b); return 0;
    case 4: hipLaunchKernelGGL(viterbi64_kernel<4>, dim3(blocks), dim3(256), 0, st, b); return 0;
    default: return 1;
    }
}

int dcp_f64_launch_scan_pairs(int R, dcp_f64_pairs_args const *a, unsigned nwaves, void *stream)
{
    unsigned const blocks = (unsigned)(((uint64_t)nwaves + 3u) / 4u);
    if (blocks == 0) return 0;
    hipStream_t const st = (hipStream_t)stream;
    dcp_f64_pairs_args b = *a;
    b.nwaves = nwaves;
    switch (R)
    {
    case 1: hipLaunchKernelGGL((viterbi64_kernel<1, false, true>), dim3(blocks), dim3(256), 0, st, b); return 0;
    case 2: hipLaunchKernelGGL((viterbi64_kernel<2, false, true>), dim3(blocks), dim3(256), 0, st, b); return 0;
    case 4: hipLaunchKernelGGL((viterbi64_kernel<4, false, true>), dim3(blocks), dim3(256), 0, st, b); return 0;
    default: return 1;
    }
}

int dcp_f64_launch_trace_forward(int R, dcp_f64_trace_args const *a, unsigned nwaves, void *stream)
{
    unsigned const blocks = (unsigned)(((uint64_t)nwaves + 3u) / 4u);
    if (blocks == 0) return 0;
    hipStream_t const st = (hipStream_t)stream;
    dcp_f64_trace_args b = *a;
    b.nwaves = nwaves;
    switch (R)
    {
    case 1: hipLaunchKernelGGL((viterbi64_kernel<1, true>), dim3(blocks), dim3(256), 0, st, b); return 0;
    case 2: hipLaunchKernelGGL((viterbi64_kernel<2, true>), dim3(blocks), dim3(256), 0, st, b); return 0;
    case 4: hipLaunchKernelGGL((viterbi64_kernel<4, true>), dim3(blocks), dim3(256), 0, st, b); return 0;
    default: return 1;
    }
}

void dcp_f64_launch_walk(dcp_f64_walk_args const *a, void *stream)
{
    if (a->nhits == 0) return;
    hipLaunchKernelGGL(trace64_kernel, dim3(a->nhits), dim3(64), 0, (hipStream_t)stream, *a);
}
