// dcp_posterior.hip -- gfx950 kernels of the Backward sweep and the posterior rows of a pair list
// (dcp_gpu_posterior_pairs; the Forward half is dcp_forward.hip's row-storing variant).
//
//  backward_kernel<Real, R>   the Backward sweep of one (sequence, profile) pair per wavefront, R = 1, 2 or 4
//                             consecutive nodes per lane, the profile's transitions and the rings of bM and bI (rows
//                             j + 1 .. j + 5) in registers, rows j = L .. 0 unrolled by five: forward_kernel's mirror.
//  backward_wide_kernel<Real> the same for wider profiles through the wavefront's work area (12 x ldk doubles; a lane
//                             reads back only what it wrote itself).  Pass one runs over the chunks of 256 columns, forms
//                             bP and bQ from the rings, stores them and accumulates bB; the specials follow; pass two
//                             runs over the chunks in falling order, carrying bD and bP of the next chunk's first node in
//                             registers, and writes bM and bI into the row's slot.
//  posterior_combine_kernel<Real>  one thread per (pair, row): begin, end, core from the two sweeps' row records, by
//                             dcp_posterior_row (dcp_posterior.h), the rule the host twin evaluates too.
//
// The recursion is dcp_posterior.h's.  Within a row: bP, bQ, then bB (a wave-wide sum, as E(j) in the Forward sweep), then
// the specials (one per lane: lane l & 3 keeps the ring of its own one of N, J, C), then D, M, I.  Backward has no E -> B
// problem: bB(j) needs rows j + 1 .. j + 5 only, bE(j) needs bB(j), the core states need bE(j) -- no value of a row
// depends on a sum over that same row's core states.  The delete chain runs downwards in k:
// bD_k = lse(g_k, bD_{k+1} + DD_{k+1}), g_k = lse(bE, DM_{k+1} + bP_{k+1}), the Forward chain's linear recurrence with the
// lanes' order reversed: (s, c) pairs, six __shfl_down steps, and the lane's chain run again from its true input.
// Device and host twin differ in exp and log and in the association of the delete chain and of bB(j).
//
// Both sweeps take a compile-time flag MAT: every lane also stores bM_k(j) and bI_k(j) of its own columns, rows
// j = 0 .. L, the matrices the posterior-decoded alignment reads (dcp_mea.h, dcp_gpu_mea_pairs' second sweep).
// MAT = false is dcp_gpu_posterior_pairs' kernel, with the registers it had before the flag.
//
// A column at or past core_size is never loaded: its entry, emissions and transitions are -inf here, so it adds nothing
// to bB, and the transitions into it (DD, DM, MD, MM, IM of node k + 1 >= core_size) are -inf, so what it holds -- bE at
// most -- reaches no real column.
#include "dcp_mea.h"
#include "dcp_posterior.h"

#include "dcp_forward_dev.h"

namespace
{

struct XB // the pair's special transitions as the Backward rows use them
{
    double EB, EJ, EC, ET, CT;
    double xa, xb; // this lane's own special state X of N, J, C: bX(j) = lse(xa + bB(j) | [j = L] CT, xb + bPX(j))
};

__device__ __forceinline__ XB backward_transitions(double const *xt, unsigned lane)
{
    XB x;
    x.EB = xt[DCP_X_EB], x.EJ = xt[DCP_X_EJ], x.EC = xt[DCP_X_EC], x.ET = xt[DCP_X_ET], x.CT = xt[DCP_X_CT];
    unsigned const sp = lane & 3u;
    x.xa = sp == 0u ? xt[DCP_X_NB] : sp == 1u ? xt[DCP_X_JB] : ninf(); // C has no edge to B; lane 3 keeps no state
    x.xb = sp == 0u ? xt[DCP_X_NN] : sp == 1u ? xt[DCP_X_JJ] : sp == 2u ? xt[DCP_X_CC] : ninf();
    return x;
}

// codes of x[j .. j+l), l = 1 .. 5, first base most significant; w keeps x[j .. j+5).  Past L the bases are 0: such a
// word's successor is a -inf row, whatever its code.
__device__ __forceinline__ void words_from(unsigned &w, uint32_t const *words, unsigned j, unsigned L, unsigned (&code)[5])
{
    unsigned const base = j < L ? (words[j >> 4] >> ((j & 15u) * 2u)) & 3u : 0u;
    w = (w >> 2) | (base << 8);
    constexpr unsigned off[5] = {0u, 4u, 20u, 84u, 340u};
#pragma unroll
    for (int l = 0; l < 5; ++l)
        code[l] = off[l] + (w >> (8 - 2 * l));
}

// the lanes' entry_k + bP_k of one chunk as one term of bB(j) in the running form (exit_terms' shape)
template <int R> __device__ __forceinline__ dcp_lse_acc entry_terms(double const (&e)[R])
{
    double mx = e[0];
#pragma unroll
    for (int r = 1; r < R; ++r)
        mx = dcp_fwd_max(mx, e[r]);
    mx = readlane(wave_max(mx), 0);
    double const mm = dcp_fwd_shift(mx);
    double sum = exp(e[0] - mm);
#pragma unroll
    for (int r = 1; r < R; ++r)
        sum = sum + exp(e[r] - mm);
    return dcp_lse_acc{mx, readlane(wave_sum(sum), 0)};
}

// bD of the lane's R nodes, downwards: c[r] = DM_{k+1} + bP_{k+1}, dd[r] = DD_{k+1}, carry = bD of the node after lane
// 63's last.  dn[r] receives bD_{k+1}, the value bM_k needs as well.  The node's own part g = lse(bE, c) is formed once
// and serves both passes: bD_k = lse(g_k, DD_{k+1} + bD_{k+1}), the rule's three-term lse associated differently.
template <int R>
__device__ __forceinline__ void delete_chain_down(double bE, double const (&c)[R], double const (&dd)[R], double carry,
                                                  double (&d)[R], double (&dn)[R], unsigned lane)
{
    double g[R];
#pragma unroll
    for (int r = 0; r < R; ++r)
        g[r] = dcp_lse2(bE, c[r]);
    double cc = g[R - 1], ss = dd[R - 1]; // the lane's chain from d_in = -inf, and the sum of its DD
#pragma unroll
    for (int r = R - 2; r >= 0; --r)
    {
        cc = dcp_lse2(g[r], dd[r] + cc);
        ss = ss + dd[r];
    }
#pragma unroll
    for (unsigned o = 1; o < 64u; o <<= 1)
    {
        double const sp = __shfl_down(ss, o, 64), cp = __shfl_down(cc, o, 64);
        if (lane + o < 64u)
        {
            cc = dcp_lse2(cc, cp + ss);
            ss = ss + sp;
        }
    }
    // lanes l + 1 .. 63 composed, applied to the carry: lane 63 receives (0, -inf), the identity
    double const cb = shl1(cc, ninf(), lane), sb = shl1(ss, 0.0, lane);
    dn[R - 1] = dcp_lse2(cb, carry + sb);
    d[R - 1] = dcp_lse2(g[R - 1], dd[R - 1] + dn[R - 1]);
#pragma unroll
    for (int r = R - 2; r >= 0; --r)
    {
        dn[r] = d[r + 1];
        d[r] = dcp_lse2(g[r], dd[r] + dn[r]);
    }
}

// the row's specials from bB and the lanes' bPX: bE for all lanes, the lane's own state, the record from lane 0
struct Specials
{
    double bE, own;
};
__device__ __forceinline__ Specials backward_specials(XB const &x, double bB, double bX, bool last, double *rec, unsigned lane)
{
    double const bPJ = readlane(bX, 1), bPC = readlane(bX, 2);
    Specials s;
    s.bE = dcp_lse4(last ? x.ET : ninf(), x.EB + bB, x.EJ + bPJ, x.EC + bPC);
    double const first = (lane & 3u) == 2u ? (last ? x.CT : ninf()) : x.xa + bB;
    s.own = dcp_lse2(first, x.xb + bX);
    double const bN = readlane(s.own, 0), bJ = readlane(s.own, 1), bC = readlane(s.own, 2);
    if (lane == 0u) rec[0] = bN, rec[1] = bJ, rec[2] = bC, rec[3] = bB, rec[4] = s.bE;
    return s;
}

// ---- profiles of at most 64 R nodes: everything in registers -------------------------------------------------------
template <int R> struct BTrans // n..: the transitions into node k + 1
{
    double ent[R], nmm[R], nim[R], ndm[R], nmd[R], ndd[R], mi[R], ii[R];
};

// rings: row j's successors j + 1 .. j + 5 live in slots (L - j - l) % 5
template <int R> struct BState
{
    double bM[5][R], bI[5][R];
    double bX[5]; // the lane's own special state
    double bB, bPN; // the last row's: alt_bwd is formed from row 0's
    unsigned w;
};

// MAT: bM goes to the pair's first matrix (Mats::m0), bI to its second
template <class Real, int R, int PH, bool MAT>
__device__ __forceinline__ void backward_row(BState<R> &s, BTrans<R> const &t, XB const &x, Tabs<Real> const &g, unsigned j,
                                             unsigned L, unsigned lane, double *rec, Mats const &mt)
{
    constexpr int sl[5] = {(PH + 4) % 5, (PH + 3) % 5, (PH + 2) % 5, (PH + 1) % 5, PH}; // slot of row j + l
    unsigned code[5];
    words_from(s.w, g.words, j, L, code);
    unsigned const k0 = lane * R;

    double cm[5][R], ci[5][R], cx[5];
#pragma unroll
    for (int l = 0; l < 5; ++l)
    {
        double const eI = (double)g.ei[code[l]], eN = (double)g.en[code[l]];
        Real const *em = g.tab + (uint64_t)code[l] * g.ld;
#pragma unroll
        for (int r = 0; r < R; ++r)
        {
            cm[l][r] = load_col(em, k0 + r, g.M) + s.bM[sl[l]][r];
            ci[l][r] = eI + s.bI[sl[l]][r];
        }
        cx[l] = eN + s.bX[sl[l]];
    }
    double bP[R], bQ[R], e[R];
#pragma unroll
    for (int r = 0; r < R; ++r)
    {
        bP[r] = dcp_lse5(cm[0][r], cm[1][r], cm[2][r], cm[3][r], cm[4][r]);
        bQ[r] = dcp_lse5(ci[0][r], ci[1][r], ci[2][r], ci[3][r], ci[4][r]);
        e[r] = t.ent[r] + bP[r];
    }
    double const bX = dcp_lse5(cx[0], cx[1], cx[2], cx[3], cx[4]);
    double const bB = dcp_lse_acc_value(entry_terms<R>(e));
    Specials const sp = backward_specials(x, bB, bX, j == L, rec + (uint64_t)DCP_POST_REC * j, lane);

    double bPn[R], c[R], d[R], dn[R]; // node k + 1's bP; lane 63's last node has none
    bPn[R - 1] = shl1(bP[0], ninf(), lane);
#pragma unroll
    for (int r = 0; r < R - 1; ++r)
        bPn[r] = bP[r + 1];
#pragma unroll
    for (int r = 0; r < R; ++r)
        c[r] = t.ndm[r] + bPn[r];
    delete_chain_down<R>(sp.bE, c, t.ndd, ninf(), d, dn, lane);
#pragma unroll
    for (int r = 0; r < R; ++r)
    {
        s.bM[PH][r] = dcp_lse4(sp.bE, t.nmd[r] + dn[r], t.nmm[r] + bPn[r], t.mi[r] + bQ[r]);
        s.bI[PH][r] = dcp_lse2(t.nim[r] + bPn[r], t.ii[r] + bQ[r]);
        if constexpr (MAT)
            if (k0 + r < g.M) mt.m0[(uint64_t)j * g.M + k0 + r] = s.bM[PH][r], mt.m1[(uint64_t)j * g.M + k0 + r] = s.bI[PH][r];
    }
    s.bX[PH] = sp.own;
    s.bB = bB, s.bPN = readlane(bX, 0);
}

template <class Real, int R, bool MAT> __global__ __launch_bounds__(256) void backward_kernel(dcp_fwd_args a)
{
    unsigned const lane = threadIdx.x & 63u;
    uint64_t const gw = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    uint64_t const nw = a.nwaves;
    if (gw >= nw) return; // the grid's last block may hold wavefronts past nwaves
    for (uint64_t pair = gw; pair < a.npairs; pair += nw)
    {
        auto const [pp, pr, L, xt] = pair_head(a, pair);
        XB const x = backward_transitions(xt, lane);
        Tabs<Real> const g = tables_of<Real>(a, pr, pp.q);
        unsigned const k0 = lane * R;
        BTrans<R> t;
#pragma unroll
        for (int r = 0; r < R; ++r)
        {
            t.ent[r] = load_col(g.trans + DCP_T_ENTRY * g.ld, k0 + r, g.M);
            t.mi[r] = load_col(g.trans + DCP_T_MI * g.ld, k0 + r, g.M);
            t.ii[r] = load_col(g.trans + DCP_T_II * g.ld, k0 + r, g.M);
            t.nmm[r] = load_col(g.trans + DCP_T_MM * g.ld, k0 + r + 1u, g.M);
            t.nim[r] = load_col(g.trans + DCP_T_IM * g.ld, k0 + r + 1u, g.M);
            t.ndm[r] = load_col(g.trans + DCP_T_DM * g.ld, k0 + r + 1u, g.M);
            t.nmd[r] = load_col(g.trans + DCP_T_MD * g.ld, k0 + r + 1u, g.M);
            t.ndd[r] = load_col(g.trans + DCP_T_DD * g.ld, k0 + r + 1u, g.M);
        }
        // rows L + 1 .. L + 5, anew for every pair: no word ends there
        BState<R> s;
#pragma unroll
        for (int h = 0; h < 5; ++h)
        {
#pragma unroll
            for (int r = 0; r < R; ++r)
                s.bM[h][r] = s.bI[h][r] = ninf();
            s.bX[h] = ninf();
        }
        s.bB = s.bPN = ninf();
        s.w = 0u;
        double *const rec = record_of(a, pp);
        Mats mt{nullptr, nullptr};
        if constexpr (MAT) mt = mats_of(a, pp);
        unsigned j = L;
#define DCP_BWD_ROW(PH)                                                                                                \
    backward_row<Real, R, PH, MAT>(s, t, x, g, j, L, lane, rec, mt);                                                   \
    if (j == 0u) break;                                                                                                \
    --j;
        for (;;)
        {
            DCP_BWD_ROW(0)
            DCP_BWD_ROW(1)
            DCP_BWD_ROW(2)
            DCP_BWD_ROW(3)
            DCP_BWD_ROW(4)
        }
#undef DCP_BWD_ROW
        if (lane == 0u) a.out_alt[pp.pos] = dcp_lse2(xt[DCP_X_SB] + s.bB, xt[DCP_X_SN] + s.bPN);
    }
}

// ---- wider profiles: chunks of 256 columns, the rings in the wavefront's work area ---------------------------------
// (WideArea: ring0 holds the slots of bM, ring1 those of bI; rows 0, 1 the row's bP, bQ)
struct BWideState
{
    double bX[5];
    double bB, bPN;
    unsigned w;
};

template <class Real, int PH, bool MAT>
__device__ __forceinline__ void backward_wide_row(BWideState &s, XB const &x, Tabs<Real> const &g, WideArea const &wa, unsigned j,
                                                  unsigned L, unsigned lane, double *rec, Mats const &mt)
{
    constexpr int sl[5] = {(PH + 4) % 5, (PH + 3) % 5, (PH + 2) % 5, (PH + 1) % 5, PH};
    unsigned code[5];
    words_from(s.w, g.words, j, L, code);
    double eI[5], cx[5];
#pragma unroll
    for (int l = 0; l < 5; ++l)
    {
        eI[l] = (double)g.ei[code[l]];
        cx[l] = (double)g.en[code[l]] + s.bX[sl[l]];
    }
    double const bX = dcp_lse5(cx[0], cx[1], cx[2], cx[3], cx[4]);

    // pass one: bP, bQ of the row, chunk after chunk, and bB over all of them
    dcp_lse_acc acc = dcp_lse_acc_empty();
    for (unsigned ch = 0; ch < wa.nchunks; ++ch)
    {
        unsigned const k0 = ch * (unsigned)DCP_FWD_CHUNK + lane * WR;
        double cm[5][WR], ci[5][WR];
#pragma unroll
        for (int l = 0; l < 5; ++l)
        {
            Real const *em = g.tab + (uint64_t)code[l] * g.ld;
            double const *m = wa.ring0(sl[l]) + k0, *i = wa.ring1(sl[l]) + k0;
#pragma unroll
            for (int r = 0; r < WR; ++r)
            {
                cm[l][r] = load_col(em, k0 + r, g.M) + m[r];
                ci[l][r] = eI[l] + i[r];
            }
        }
        double e[WR];
        double *const wp = wa.row(0) + k0, *const wq = wa.row(1) + k0;
#pragma unroll
        for (int r = 0; r < WR; ++r)
        {
            double const bP = dcp_lse5(cm[0][r], cm[1][r], cm[2][r], cm[3][r], cm[4][r]);
            wp[r] = bP;
            wq[r] = dcp_lse5(ci[0][r], ci[1][r], ci[2][r], ci[3][r], ci[4][r]);
            e[r] = load_col(g.trans + DCP_T_ENTRY * g.ld, k0 + r, g.M) + bP;
        }
        acc = dcp_lse_acc_merge(acc, entry_terms<WR>(e));
    }
    double const bB = dcp_lse_acc_value(acc);
    Specials const sp = backward_specials(x, bB, bX, j == L, rec + (uint64_t)DCP_POST_REC * j, lane);

    // pass two: D, M, I downwards, into slot PH; bD and bP of the next chunk's first node come along in registers
    double carry_d = ninf(), carry_p = ninf();
    for (unsigned ch = wa.nchunks; ch-- > 0u;)
    {
        unsigned const k0 = ch * (unsigned)DCP_FWD_CHUNK + lane * WR;
        double const *wp = wa.row(0) + k0, *wq = wa.row(1) + k0;
        double bP[WR], bQ[WR], bPn[WR], c[WR], dd[WR], d[WR], dn[WR];
#pragma unroll
        for (int r = 0; r < WR; ++r)
            bP[r] = wp[r], bQ[r] = wq[r];
        bPn[WR - 1] = shl1(bP[0], carry_p, lane);
#pragma unroll
        for (int r = 0; r < WR - 1; ++r)
            bPn[r] = bP[r + 1];
#pragma unroll
        for (int r = 0; r < WR; ++r)
        {
            c[r] = load_col(g.trans + DCP_T_DM * g.ld, k0 + r + 1u, g.M) + bPn[r];
            dd[r] = load_col(g.trans + DCP_T_DD * g.ld, k0 + r + 1u, g.M);
        }
        delete_chain_down<WR>(sp.bE, c, dd, carry_d, d, dn, lane);
        double *const m = wa.ring0(PH) + k0, *const i = wa.ring1(PH) + k0;
#pragma unroll
        for (int r = 0; r < WR; ++r)
        {
            unsigned const k = k0 + r;
            m[r] = dcp_lse4(sp.bE, load_col(g.trans + DCP_T_MD * g.ld, k + 1u, g.M) + dn[r],
                            load_col(g.trans + DCP_T_MM * g.ld, k + 1u, g.M) + bPn[r], load_col(g.trans + DCP_T_MI * g.ld, k, g.M) + bQ[r]);
            i[r] = dcp_lse2(load_col(g.trans + DCP_T_IM * g.ld, k + 1u, g.M) + bPn[r], load_col(g.trans + DCP_T_II * g.ld, k, g.M) + bQ[r]);
            if constexpr (MAT)
                if (k < g.M) mt.m0[(uint64_t)j * g.M + k] = m[r], mt.m1[(uint64_t)j * g.M + k] = i[r];
        }
        carry_p = readlane(bP[0], 0), carry_d = readlane(d[0], 0);
    }
    s.bX[PH] = sp.own;
    s.bB = bB, s.bPN = readlane(bX, 0);
}

template <class Real, bool MAT> __global__ __launch_bounds__(256) void backward_wide_kernel(dcp_fwd_args a)
{
    unsigned const lane = threadIdx.x & 63u;
    uint64_t const gw = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    uint64_t const nw = a.nwaves;
    if (gw >= nw) return; // wavefronts past nwaves have no work area
    for (uint64_t pair = gw; pair < a.npairs; pair += nw)
    {
        auto const [pp, pr, L, xt] = pair_head(a, pair);
        XB const x = backward_transitions(xt, lane);
        Tabs<Real> const g = tables_of<Real>(a, pr, pp.q);
        WideArea const wa = wide_area(a.work, a.work_stride, gw, pr.core_size);
        static_assert((int)DCP_POST_WORK_ROWS <= (int)DCP_FWD_WORK_ROWS, "the Forward sweep's work area serves");
        // rows L + 1 .. L + 5, anew for every pair: the rings' own columns
        for (unsigned ch = 0; ch < wa.nchunks; ++ch)
        {
            unsigned const k0 = ch * (unsigned)DCP_FWD_CHUNK + lane * WR;
#pragma unroll
            for (int r = 0; r < WR; ++r)
#pragma unroll
                for (int h = 0; h < 5; ++h)
                    wa.ring0(h)[k0 + r] = wa.ring1(h)[k0 + r] = ninf();
        }
        BWideState s;
#pragma unroll
        for (int h = 0; h < 5; ++h)
            s.bX[h] = ninf();
        s.bB = s.bPN = ninf();
        s.w = 0u;
        double *const rec = record_of(a, pp);
        Mats mt{nullptr, nullptr};
        if constexpr (MAT) mt = mats_of(a, pp);
        unsigned j = L;
#define DCP_BWD_ROW(PH)                                                                                                \
    backward_wide_row<Real, PH, MAT>(s, x, g, wa, j, L, lane, rec, mt);                                                \
    if (j == 0u) break;                                                                                                \
    --j;
        for (;;)
        {
            DCP_BWD_ROW(0)
            DCP_BWD_ROW(1)
            DCP_BWD_ROW(2)
            DCP_BWD_ROW(3)
            DCP_BWD_ROW(4)
        }
#undef DCP_BWD_ROW
        if (lane == 0u) a.out_alt[pp.pos] = dcp_lse2(xt[DCP_X_SB] + s.bB, xt[DCP_X_SN] + s.bPN);
    }
}

// ---- begin, end, core: one thread per row of the round ----------------------------------------------------------------
template <class Real> __global__ __launch_bounds__(256) void posterior_combine_kernel(dcp_post_args a)
{
    uint64_t const base = a.row_off[0], total = a.row_off[a.nlist] - base;
    uint64_t const t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= total) return;
    unsigned lo = 0, hi = a.nlist; // the pair whose rows hold t: row_off[lo] - base <= t < row_off[lo + 1] - base
    while (hi - lo > 1u)
    {
        unsigned const mid = lo + (hi - lo) / 2u;
        if (a.row_off[mid] - base <= t) lo = mid;
        else hi = mid;
    }
    uint64_t const first = a.row_off[lo] - base;
    dcp_fwd_pair const pp = a.list[lo];
    unsigned const L = a.seq_len[pp.q], j = (unsigned)(t - first);
    uint32_t const *words = a.seq_words + a.seq_woff[pp.q];
    unsigned win = 0; // bases j - 5 .. j + 3, first most significant; outside the sequence 0
#pragma unroll
    for (int i = 0; i < 9; ++i)
    {
        long long const b = (long long)j - 5 + i;
        unsigned v = 0u;
        if (b >= 0 && b < (long long)L) v = (words[(unsigned)b >> 4] >> (((unsigned)b & 15u) * 2u)) & 3u;
        win = (win << 2) | v;
    }
    Real const *en = (Real const *)a.en + a.profs[pp.prof].en_off;
    dcp_posterior_row<Real>(a.rows_f + first * DCP_POST_REC, a.rows_b + first * DCP_POST_REC, en, win, j, L, a.alt_fwd[pp.pos],
                            a.begin + t, a.end + t, a.core + t);
}

template <class Real, bool MAT> int launch_backward(int R, dcp_fwd_args const &a, hipStream_t st)
{
    dim3 const grid((a.nwaves + 3u) / 4u), block(256);
    switch (R)
    {
    case 0: hipLaunchKernelGGL((backward_wide_kernel<Real, MAT>), grid, block, 0, st, a); return 0;
    case 1: hipLaunchKernelGGL((backward_kernel<Real, 1, MAT>), grid, block, 0, st, a); return 0;
    case 2: hipLaunchKernelGGL((backward_kernel<Real, 2, MAT>), grid, block, 0, st, a); return 0;
    case 4: hipLaunchKernelGGL((backward_kernel<Real, 4, MAT>), grid, block, 0, st, a); return 0;
    default: return 1;
    }
}

// (float first, then double, of each variant in turn: the order in which the unit's kernels are emitted)
template <bool MAT> int launch_backward(int precision, int R, dcp_fwd_args const &a, hipStream_t st)
{
    if (precision == 32) return launch_backward<float, MAT>(R, a, st);
    if (precision == 64) return launch_backward<double, MAT>(R, a, st);
    return 1;
}

} // namespace

extern "C" int dcp_backward_launch(int precision, int R, int store, struct dcp_fwd_args const *a, void *stream)
{
    if (store == DCP_FWD_STORE_NONE || dcp_fwd_args_refused(a, R, store)) return 1; // Backward always writes its records
    hipStream_t const st = (hipStream_t)stream;
    if (store == DCP_FWD_STORE_ROWS) return launch_backward<false>(precision, R, *a, st);
    return launch_backward<true>(precision, R, *a, st);
}

extern "C" int dcp_posterior_combine_launch(int precision, struct dcp_post_args const *a, uint64_t total_rows, void *stream)
{
    if (!a || a->nlist == 0 || total_rows == 0 || (total_rows + 255u) / 256u > 0x7fffffffull) return 1;
    dim3 const grid((unsigned)((total_rows + 255u) / 256u)), block(256);
    hipStream_t const st = (hipStream_t)stream;
    if (precision == 32) hipLaunchKernelGGL((posterior_combine_kernel<float>), grid, block, 0, st, *a);
    else if (precision == 64) hipLaunchKernelGGL((posterior_combine_kernel<double>), grid, block, 0, st, *a);
    else return 1;
    return 0;
}
