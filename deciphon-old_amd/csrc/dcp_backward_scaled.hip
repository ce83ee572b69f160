// dcp_backward_scaled.hip -- gfx950 kernels of the scaled probability-space Backward sweep (dcp_gpu_posterior_pairs_scaled;
// the Forward half is dcp_forward_scaled.hip's row-storing variant).  The rule is dcp_backward_scaled.h's; the layout is
// dcp_posterior.hip's:
//
//  backward_scaled_kernel<Real, R>   one (sequence, profile) pair per wavefront, R = 1, 2 or 4 consecutive nodes per
//                                    lane, the profile's transition factors and the rings of bM and bI (rows j + 1 ..
//                                    j + 5) in registers, rows j = L .. 0 unrolled by five.
//  backward_scaled_wide_kernel<Real> wider profiles in two passes over chunks of 256 columns through the wavefront's
//                                    work area: the rings of bM and bI, the row's bP and bQ, and behind them eight rows
//                                    of transition factors (20 x ldk doubles).  The factors of the transitions into node
//                                    k + 1 lie at column k, so a lane reads back only what it wrote itself.
//
// Values are probabilities beside one exponent per pair: bP and bQ are five fused multiply-adds each, the delete chain
// bD_k = g_k + dd_{k+1} bD_{k+1} is closed by the six-step downward lane scan over (product of dd, chain) pairs, bB(j) is
// the wave sum of the lanes' ent_k bP_k.  Transitions are exponentiated once per pair, insert and null emissions once per
// row (one per lane), match emissions on load.  A row's record is five logs, one per lane.  After a row the wave-uniform
// ref decides on a rescaling of every ring value.  A pair that leaves the double range, or whose records could have lost
// a term that matters (dcp_bws_lossy), is appended to the launch's redo list, which the driver hands to the log-space
// kernels.
//
// A column at or past core_size is never loaded: its factors are 0, so it adds nothing to bB, and the factors of the
// transitions into it are 0, so what it holds -- bE at most -- reaches no real column.
#include "dcp_backward_scaled.h"
#include "dcp_host.h"

#include <hip/hip_runtime.h>

#include "dcp_forward_dev.h"

namespace
{

struct Post // what a launch reads beside its arguments, and where it leaves the pairs it could not sweep
{
    double const *rows_f, *alt_fwd;
    dcp_fwd_pair *list;
    uint32_t *count;
    uint32_t cap;
    int band;
};

template <class Real> __device__ __forceinline__ double fac_of(double v) { return dcp_fws_factor((Real)v); }

template <class Real> __device__ __forceinline__ double load_fac(Real const *row, unsigned k, unsigned M)
{
    return k < M ? dcp_fws_factor(row[k]) : 0.0;
}

struct XBS // the pair's special transitions as factors
{
    double EB, EJ, EC, ETL, CTL; // ETL, CTL: row L's, under the exponent that row starts with
    double SB, SN;
    double xa, xb; // this lane's own special state X of N, J, C: bX(j) = fma(xb, bPX(j), xa bB(j) | [j = L] CTL)
};

// the factors, and row L's part of the rescaling rule: ref = max(ET, CT) before anything reads the ring
template <class Real> __device__ __forceinline__ XBS backward_factors(double const *xt, unsigned lane, int band, int &s)
{
    XBS x;
    x.EB = fac_of<Real>(xt[DCP_X_EB]), x.EJ = fac_of<Real>(xt[DCP_X_EJ]), x.EC = fac_of<Real>(xt[DCP_X_EC]);
    x.ETL = fac_of<Real>(xt[DCP_X_ET]), x.CTL = fac_of<Real>(xt[DCP_X_CT]);
    x.SB = fac_of<Real>(xt[DCP_X_SB]), x.SN = fac_of<Real>(xt[DCP_X_SN]);
    unsigned const sp = lane & 3u;
    x.xa = sp == 0u ? fac_of<Real>(xt[DCP_X_NB]) : sp == 1u ? fac_of<Real>(xt[DCP_X_JB]) : 0.0; // C has no edge to B
    x.xb = sp == 3u ? 0.0 : fac_of<Real>(sp == 0u ? xt[DCP_X_NN] : sp == 1u ? xt[DCP_X_JJ] : xt[DCP_X_CC]);
    s = 0;
    if (dcp_fws_finite(x.ETL) && dcp_fws_finite(x.CTL)) // (else row L ends the pair)
        if (int const k = dcp_fws_rescale_by(dcp_fwd_max(x.ETL, x.CTL), band))
        {
            double const c = dcp_fws_pow2(-k);
            x.ETL *= c, x.CTL *= c;
            s = k;
        }
    return x;
}

// x[j .. j+5) in w, first base most significant; past L the bases are 0: such a word's successor row is 0
__device__ __forceinline__ void words_from(unsigned &w, uint32_t const *words, unsigned j, unsigned L, unsigned (&code)[5])
{
    unsigned const base = j < L ? (words[j >> 4] >> ((j & 15u) * 2u)) & 3u : 0u;
    w = (w >> 2) | (base << 8);
    constexpr unsigned off[5] = {0u, 4u, 20u, 84u, 340u};
#pragma unroll
    for (int l = 0; l < 5; ++l)
        code[l] = off[l] + (w >> (8 - 2 * l));
}

// The row's ten wave-uniform factors -- insert and null emissions of the words x[j .. j+l) -- one per lane: lane l < 5
// forms the insert factor of the word of length l + 1, lane 5 + l its null factor (the other lanes repeat lane 0's).
template <class Real>
__device__ __forceinline__ void row_factors(Tabs<Real> const &g, unsigned w, unsigned lane, double (&fI)[5], double (&fN)[5])
{
    unsigned const l = lane < 5u ? lane : lane < 10u ? lane - 5u : 0u;
    unsigned const code = ((0x55555555u & ((1u << (2u * l)) - 1u)) << 2) + (w >> (8u - 2u * l));
    double const f = dcp_fws_factor((lane >= 5u && lane < 10u ? g.en : g.ei)[code]);
#pragma unroll
    for (int i = 0; i < 5; ++i)
        fI[i] = readlane(f, i), fN[i] = readlane(f, 5 + i);
}

// bD of the lane's R nodes, downwards: g[r] = fma(DM_{k+1}, bP_{k+1}, bE), dd[r] = DD_{k+1}, carry = bD of the node after
// lane 63's last.  dn[r] receives bD_{k+1}, the value bM_k needs as well.
template <int R>
__device__ __forceinline__ void delete_chain_down_scaled(double const (&g)[R], double const (&dd)[R], double carry, double (&d)[R],
                                                         double (&dn)[R], unsigned lane)
{
    double cc = g[R - 1], ss = dd[R - 1]; // the lane's chain from d_in = 0, and the product of its dd
#pragma unroll
    for (int r = R - 2; r >= 0; --r)
    {
        cc = dcp_fws_fma(dd[r], cc, g[r]);
        ss = ss * dd[r];
    }
#pragma unroll
    for (unsigned o = 1; o < 64u; o <<= 1)
    {
        double const sp = __shfl_down(ss, o, 64), cp = __shfl_down(cc, o, 64);
        if (lane + o < 64u)
        {
            cc = dcp_fws_fma(cp, ss, cc);
            ss = ss * sp;
        }
    }
    // lanes l + 1 .. 63 composed, applied to the carry: lane 63 receives (1, 0), the identity
    double const cb = shl1(cc, 0.0, lane), sb = shl1(ss, 1.0, lane);
    // (a chain that carries no mass has bD = 0 by the rule, whatever its dd: the product sb may have left the range,
    // and 0 x inf is no value of the rule)
    dn[R - 1] = carry != 0.0 ? dcp_fws_fma(carry, sb, cb) : cb;
    d[R - 1] = dcp_fws_fma(dd[R - 1], dn[R - 1], g[R - 1]);
#pragma unroll
    for (int r = R - 2; r >= 0; --r)
    {
        dn[r] = d[r + 1];
        d[r] = dcp_fws_fma(dd[r], dn[r], g[r]);
    }
}

// what the rows share beside the rings
struct BSpec
{
    double bX[5];   // the lane's own special state's ring
    double bB, bPN; // the last row's: alt_bwd is formed from row 0's
    int s;          // the pair's exponent
    unsigned w;
};

struct RowSpecials
{
    double bE, own;
};

// The row's specials from bB and the lanes' bPX: bE for all lanes, the lane's own state.
__device__ __forceinline__ RowSpecials backward_specials(XBS const &x, double bB, double bX, bool last, unsigned lane)
{
    double const bPJ = readlane(bX, 1), bPC = readlane(bX, 2);
    RowSpecials r;
    double e = last ? x.ETL : 0.0;
    e = dcp_fws_fma(x.EB, bB, e);
    e = dcp_fws_fma(x.EJ, bPJ, e);
    r.bE = dcp_fws_fma(x.EC, bPC, e);
    double const first = (lane & 3u) == 2u ? (last ? x.CTL : 0.0) : x.xa * bB;
    r.own = dcp_fws_fma(x.xb, bX, first);
    return r;
}

// After the row's values are known to be finite: the record as five logs, one per lane (lanes 0 .. 2 hold bN, bJ, bC in
// `own`), and the underflow check against the Forward record of the same row.  Returns true if the pair is lossy.
__device__ __forceinline__ bool record_and_check(double own, double bB, double bE, int s, double *rec, double const *frec, double a,
                                                 int band, unsigned lane)
{
    double const v = lane < 3u ? own : lane == 3u ? bB : bE;
    double const lg = dcp_fws_score(v, s);
    if (lane < 5u) rec[lane] = lg;
    double const b5[5] = {readlane(lg, 0), readlane(lg, 1), readlane(lg, 2), readlane(lg, 3), readlane(lg, 4)};
    return dcp_bws_lossy(dcp_bws_rec_max(frec), dcp_bws_rec_max(b5), a, band) != 0;
}

// the row's rescaling step from its specials (wave-uniform; 0: none)
__device__ __forceinline__ int rescale_step(double own, double bB, double bE, int band)
{
    double const bn = readlane(own, 0), bj = readlane(own, 1), bc = readlane(own, 2);
    double const ref = dcp_fwd_max(dcp_fwd_max(dcp_fwd_max(bn, bj), dcp_fwd_max(bc, bB)), bE);
    return dcp_fws_rescale_by(ref, band);
}

__device__ __forceinline__ void rescale_specials(BSpec &s, int k)
{
    double const c = dcp_fws_pow2(-k);
#pragma unroll
    for (int h = 0; h < 5; ++h)
        s.bX[h] *= c;
    s.bB *= c, s.bPN *= c;
    s.s += k;
}

__device__ __forceinline__ void finish_pair(dcp_fwd_args const &a, Post const &po, dcp_fwd_pair const &pp, BSpec const &s,
                                            XBS const &x, bool bad, unsigned lane)
{
    double alt = 0.0;
    int sA = s.s;
    if (!bad)
    {
        // row 0's bB and bPN with the larger of them in [1, 2): the product with SB, SN near e^-708 stays normal
        int const k = dcp_fws_rescale_by(dcp_fwd_max(s.bB, s.bPN), 0);
        double const c = dcp_fws_pow2(-k);
        alt = dcp_fws_fma(x.SN, s.bPN * c, x.SB * (s.bB * c));
        sA += k;
        bad = !dcp_fws_finite(alt);
    }
    if (lane == 0u)
    {
        if (bad)
        {
            uint32_t const at = atomicAdd(po.count, 1u);
            if (at < po.cap) po.list[at] = pp;
        }
        a.out_alt[pp.pos] = bad ? ninf() : dcp_fws_score(alt, sA);
    }
}

// ---- profiles of at most 64 R nodes: everything in registers -------------------------------------------------------
template <int R> struct BTrans // n..: the factors of the transitions into node k + 1
{
    double ent[R], nmm[R], nim[R], ndm[R], nmd[R], ndd[R], mi[R], ii[R];
};

template <int R> struct BRings // row j's successors j + 1 .. j + 5 live in slots (L - j - l) % 5
{
    double bM[5][R], bI[5][R];
};

// one row; returns true if the pair ends here (wave-uniform)
template <class Real, int R, int PH>
__device__ __forceinline__ bool backward_scaled_row(BRings<R> &g5, BSpec &s, BTrans<R> const &t, XBS const &x, Tabs<Real> const &g,
                                                    unsigned j, unsigned L, unsigned lane, double *rec, double const *frec, double a,
                                                    int band)
{
    constexpr int sl[5] = {(PH + 4) % 5, (PH + 3) % 5, (PH + 2) % 5, (PH + 1) % 5, PH}; // slot of row j + l
    unsigned code[5];
    words_from(s.w, g.words, j, L, code);
    unsigned const k0 = lane * R;

    double fI[5], fN[5];
    row_factors(g, s.w, lane, fI, fN);
    double bP[R], bQ[R], bX = 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r)
        bP[r] = bQ[r] = 0.0;
#pragma unroll
    for (int l = 0; l < 5; ++l)
    {
        Real const *em = g.tab + (uint64_t)code[l] * g.ld;
#pragma unroll
        for (int r = 0; r < R; ++r)
        {
            bP[r] = dcp_fws_fma(g5.bM[sl[l]][r], load_fac(em, k0 + r, g.M), bP[r]);
            bQ[r] = dcp_fws_fma(g5.bI[sl[l]][r], fI[l], bQ[r]);
        }
        bX = dcp_fws_fma(s.bX[sl[l]], fN[l], bX);
    }
    double sum = t.ent[0] * bP[0];
#pragma unroll
    for (int r = 1; r < R; ++r)
        sum = sum + t.ent[r] * bP[r];
    double const bB = readlane(wave_sum(sum), 0);
    RowSpecials const sp = backward_specials(x, bB, bX, j == L, lane);

    double bPn[R], gk[R], d[R], dn[R]; // node k + 1's bP; lane 63's last node has none
    bPn[R - 1] = shl1(bP[0], 0.0, lane);
#pragma unroll
    for (int r = 0; r < R - 1; ++r)
        bPn[r] = bP[r + 1];
#pragma unroll
    for (int r = 0; r < R; ++r)
        gk[r] = dcp_fws_fma(t.ndm[r], bPn[r], sp.bE);
    delete_chain_down_scaled<R>(gk, t.ndd, 0.0, d, dn, lane);
    bool fin = true;
#pragma unroll
    for (int r = 0; r < R; ++r)
    {
        double m = dcp_fws_fma(t.nmd[r], dn[r], sp.bE);
        m = dcp_fws_fma(t.nmm[r], bPn[r], m);
        m = dcp_fws_fma(t.mi[r], bQ[r], m);
        double const i = dcp_fws_fma(t.ii[r], bQ[r], t.nim[r] * bPn[r]);
        g5.bM[PH][r] = m, g5.bI[PH][r] = i;
        fin = fin && dcp_fws_finite(m) && dcp_fws_finite(i);
    }
    s.bX[PH] = sp.own;
    s.bB = bB, s.bPN = readlane(bX, 0);
    fin = fin && dcp_fws_finite(sp.own) && dcp_fws_finite(sp.bE) && dcp_fws_finite(bB);
    if (__any(!fin)) return true;
    if (record_and_check(sp.own, bB, sp.bE, s.s, rec + (uint64_t)DCP_POST_REC * j, frec + (uint64_t)DCP_POST_REC * j, a, band, lane))
        return true;

    if (int const k = rescale_step(sp.own, bB, sp.bE, band))
    {
        double const c = dcp_fws_pow2(-k);
#pragma unroll
        for (int h = 0; h < 5; ++h)
#pragma unroll
            for (int r = 0; r < R; ++r)
                g5.bM[h][r] *= c, g5.bI[h][r] *= c;
        rescale_specials(s, k);
    }
    return false;
}

template <class Real, int R> __global__ __launch_bounds__(256) void backward_scaled_kernel(dcp_fwd_args a, Post po)
{
    unsigned const lane = threadIdx.x & 63u;
    uint64_t const gw = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    uint64_t const nw = a.nwaves;
    if (gw >= nw) return; // the grid's last block may hold wavefronts past nwaves
    for (uint64_t pair = gw; pair < a.npairs; pair += nw)
    {
        auto const [pp, pr, L, xt] = pair_head(a, pair);
        BSpec s;
        XBS const x = backward_factors<Real>(xt, lane, po.band, s.s);
        Tabs<Real> const g = tables_of<Real>(a, pr, pp.q);
        unsigned const k0 = lane * R;
        BTrans<R> t;
#pragma unroll
        for (int r = 0; r < R; ++r)
        {
            t.ent[r] = load_fac(g.trans + DCP_T_ENTRY * g.ld, k0 + r, g.M);
            t.mi[r] = load_fac(g.trans + DCP_T_MI * g.ld, k0 + r, g.M);
            t.ii[r] = load_fac(g.trans + DCP_T_II * g.ld, k0 + r, g.M);
            t.nmm[r] = load_fac(g.trans + DCP_T_MM * g.ld, k0 + r + 1u, g.M);
            t.nim[r] = load_fac(g.trans + DCP_T_IM * g.ld, k0 + r + 1u, g.M);
            t.ndm[r] = load_fac(g.trans + DCP_T_DM * g.ld, k0 + r + 1u, g.M);
            t.nmd[r] = load_fac(g.trans + DCP_T_MD * g.ld, k0 + r + 1u, g.M);
            t.ndd[r] = load_fac(g.trans + DCP_T_DD * g.ld, k0 + r + 1u, g.M);
        }
        // rows L + 1 .. L + 5, anew for every pair: no word ends there
        BRings<R> g5;
#pragma unroll
        for (int h = 0; h < 5; ++h)
        {
#pragma unroll
            for (int r = 0; r < R; ++r)
                g5.bM[h][r] = g5.bI[h][r] = 0.0;
            s.bX[h] = 0.0;
        }
        s.bB = s.bPN = 0.0;
        s.w = 0u;
        uint64_t const at = (a.row_off[pp.pos] - a.row_base) * DCP_POST_REC;
        double *const rec = a.rows + at;
        double const *const frec = po.rows_f + at;
        double const alt_fwd = po.alt_fwd[pp.pos];
        bool bad = false;
        unsigned j = L;
#define DCP_BWS_ROW(PH)                                                                                                \
    bad = backward_scaled_row<Real, R, PH>(g5, s, t, x, g, j, L, lane, rec, frec, alt_fwd, po.band);                   \
    if (bad || j == 0u) break;                                                                                         \
    --j;
        for (;;)
        {
            DCP_BWS_ROW(0)
            DCP_BWS_ROW(1)
            DCP_BWS_ROW(2)
            DCP_BWS_ROW(3)
            DCP_BWS_ROW(4)
        }
#undef DCP_BWS_ROW
        finish_pair(a, po, pp, s, x, bad, lane);
    }
}

// ---- wider profiles: chunks of 256 columns, the rings in the wavefront's work area ---------------------------------
// (WideArea: ring0 holds the slots of bM, ring1 those of bI; rows 0, 1 the row's bP, bQ.)  Behind them the profile's
// eight rows of transition factors, written once per pair, every lane its own columns: row DCP_T_* at column k holds
// ENTRY, MI, II of node k and MM, IM, DM, MD, DD of node k + 1.
__device__ __forceinline__ double *trans_fac(WideArea const &wa, int which)
{
    return wa.base + (uint64_t)(DCP_POST_WORK_ROWS + which) * wa.ldk;
}

template <class Real, int PH>
__device__ __forceinline__ bool backward_scaled_wide_row(BSpec &s, XBS const &x, Tabs<Real> const &g, WideArea const &wa, unsigned j,
                                                         unsigned L, unsigned lane, double *rec, double const *frec, double a, int band)
{
    constexpr int sl[5] = {(PH + 4) % 5, (PH + 3) % 5, (PH + 2) % 5, (PH + 1) % 5, PH};
    unsigned code[5];
    words_from(s.w, g.words, j, L, code);
    double fI[5], fN[5], bX = 0.0;
    row_factors(g, s.w, lane, fI, fN);
#pragma unroll
    for (int l = 0; l < 5; ++l)
        bX = dcp_fws_fma(s.bX[sl[l]], fN[l], bX);

    // pass one: bP, bQ of the row, chunk after chunk, and bB over all of them
    double bB = 0.0;
    for (unsigned ch = 0; ch < wa.nchunks; ++ch)
    {
        unsigned const k0 = ch * (unsigned)DCP_FWD_CHUNK + lane * WR;
        double bP[WR], bQ[WR];
#pragma unroll
        for (int r = 0; r < WR; ++r)
            bP[r] = bQ[r] = 0.0;
#pragma unroll
        for (int l = 0; l < 5; ++l)
        {
            Real const *em = g.tab + (uint64_t)code[l] * g.ld;
            double const *m = wa.ring0(sl[l]) + k0, *i = wa.ring1(sl[l]) + k0;
#pragma unroll
            for (int r = 0; r < WR; ++r)
            {
                bP[r] = dcp_fws_fma(m[r], load_fac(em, k0 + r, g.M), bP[r]);
                bQ[r] = dcp_fws_fma(i[r], fI[l], bQ[r]);
            }
        }
        double *const wp = wa.row(0) + k0, *const wq = wa.row(1) + k0;
        double const *ent = trans_fac(wa, DCP_T_ENTRY) + k0;
        double sum = 0.0;
#pragma unroll
        for (int r = 0; r < WR; ++r)
        {
            wp[r] = bP[r], wq[r] = bQ[r];
            sum = r ? sum + ent[r] * bP[r] : ent[0] * bP[0];
        }
        bB = bB + readlane(wave_sum(sum), 0);
    }
    RowSpecials const sp = backward_specials(x, bB, bX, j == L, lane);

    // pass two: D, M, I downwards, into slot PH; bD and bP of the next chunk's first node come along in registers
    bool fin = true;
    double carry_d = 0.0, carry_p = 0.0;
    for (unsigned ch = wa.nchunks; ch-- > 0u;)
    {
        unsigned const k0 = ch * (unsigned)DCP_FWD_CHUNK + lane * WR;
        double const *wp = wa.row(0) + k0, *wq = wa.row(1) + k0;
        double bP[WR], bQ[WR], bPn[WR], gk[WR], dd[WR], d[WR], dn[WR];
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
            gk[r] = dcp_fws_fma(trans_fac(wa, DCP_T_DM)[k0 + r], bPn[r], sp.bE);
            dd[r] = trans_fac(wa, DCP_T_DD)[k0 + r];
        }
        delete_chain_down_scaled<WR>(gk, dd, carry_d, d, dn, lane);
        double *const m = wa.ring0(PH) + k0, *const i = wa.ring1(PH) + k0;
#pragma unroll
        for (int r = 0; r < WR; ++r)
        {
            unsigned const k = k0 + r;
            double v = dcp_fws_fma(trans_fac(wa, DCP_T_MD)[k], dn[r], sp.bE);
            v = dcp_fws_fma(trans_fac(wa, DCP_T_MM)[k], bPn[r], v);
            v = dcp_fws_fma(trans_fac(wa, DCP_T_MI)[k], bQ[r], v);
            double const u = dcp_fws_fma(trans_fac(wa, DCP_T_II)[k], bQ[r], trans_fac(wa, DCP_T_IM)[k] * bPn[r]);
            m[r] = v, i[r] = u;
            fin = fin && dcp_fws_finite(v) && dcp_fws_finite(u);
        }
        carry_p = readlane(bP[0], 0), carry_d = readlane(d[0], 0);
    }
    s.bX[PH] = sp.own;
    s.bB = bB, s.bPN = readlane(bX, 0);
    fin = fin && dcp_fws_finite(sp.own) && dcp_fws_finite(sp.bE) && dcp_fws_finite(bB);
    if (__any(!fin)) return true;
    if (record_and_check(sp.own, bB, sp.bE, s.s, rec + (uint64_t)DCP_POST_REC * j, frec + (uint64_t)DCP_POST_REC * j, a, band, lane))
        return true;

    if (int const k = rescale_step(sp.own, bB, sp.bE, band))
    {
        // the ten ring rows of the work area, every lane its own columns
        double const c = dcp_fws_pow2(-k);
        for (unsigned ch = 0; ch < wa.nchunks; ++ch)
        {
            unsigned const k0 = ch * (unsigned)DCP_FWD_CHUNK + lane * WR;
#pragma unroll
            for (unsigned h = 0; h < 5u; ++h)
#pragma unroll
                for (int r = 0; r < WR; ++r)
                    wa.ring0(h)[k0 + r] *= c, wa.ring1(h)[k0 + r] *= c;
        }
        rescale_specials(s, k);
    }
    return false;
}

template <class Real> __global__ __launch_bounds__(256) void backward_scaled_wide_kernel(dcp_fwd_args a, Post po)
{
    unsigned const lane = threadIdx.x & 63u;
    uint64_t const gw = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    uint64_t const nw = a.nwaves;
    if (gw >= nw) return; // wavefronts past nwaves have no work area
    for (uint64_t pair = gw; pair < a.npairs; pair += nw)
    {
        auto const [pp, pr, L, xt] = pair_head(a, pair);
        BSpec s;
        XBS const x = backward_factors<Real>(xt, lane, po.band, s.s);
        Tabs<Real> const g = tables_of<Real>(a, pr, pp.q);
        WideArea const wa = wide_area(a.work, a.work_stride, gw, pr.core_size);
        // the transition factors and rows L + 1 .. L + 5, anew for every pair: the lane's own columns
        for (unsigned ch = 0; ch < wa.nchunks; ++ch)
        {
            unsigned const k0 = ch * (unsigned)DCP_FWD_CHUNK + lane * WR;
#pragma unroll
            for (int r = 0; r < WR; ++r)
            {
                unsigned const k = k0 + r;
                trans_fac(wa, DCP_T_ENTRY)[k] = load_fac(g.trans + (uint64_t)DCP_T_ENTRY * g.ld, k, g.M);
                trans_fac(wa, DCP_T_MI)[k] = load_fac(g.trans + (uint64_t)DCP_T_MI * g.ld, k, g.M);
                trans_fac(wa, DCP_T_II)[k] = load_fac(g.trans + (uint64_t)DCP_T_II * g.ld, k, g.M);
                trans_fac(wa, DCP_T_MM)[k] = load_fac(g.trans + (uint64_t)DCP_T_MM * g.ld, k + 1u, g.M);
                trans_fac(wa, DCP_T_IM)[k] = load_fac(g.trans + (uint64_t)DCP_T_IM * g.ld, k + 1u, g.M);
                trans_fac(wa, DCP_T_DM)[k] = load_fac(g.trans + (uint64_t)DCP_T_DM * g.ld, k + 1u, g.M);
                trans_fac(wa, DCP_T_MD)[k] = load_fac(g.trans + (uint64_t)DCP_T_MD * g.ld, k + 1u, g.M);
                trans_fac(wa, DCP_T_DD)[k] = load_fac(g.trans + (uint64_t)DCP_T_DD * g.ld, k + 1u, g.M);
#pragma unroll
                for (int h = 0; h < 5; ++h)
                    wa.ring0(h)[k] = wa.ring1(h)[k] = 0.0;
            }
        }
#pragma unroll
        for (int h = 0; h < 5; ++h)
            s.bX[h] = 0.0;
        s.bB = s.bPN = 0.0;
        s.w = 0u;
        uint64_t const at = (a.row_off[pp.pos] - a.row_base) * DCP_POST_REC;
        double *const rec = a.rows + at;
        double const *const frec = po.rows_f + at;
        double const alt_fwd = po.alt_fwd[pp.pos];
        bool bad = false;
        unsigned j = L;
#define DCP_BWS_ROW(PH)                                                                                                \
    bad = backward_scaled_wide_row<Real, PH>(s, x, g, wa, j, L, lane, rec, frec, alt_fwd, po.band);                    \
    if (bad || j == 0u) break;                                                                                         \
    --j;
        for (;;)
        {
            DCP_BWS_ROW(0)
            DCP_BWS_ROW(1)
            DCP_BWS_ROW(2)
            DCP_BWS_ROW(3)
            DCP_BWS_ROW(4)
        }
#undef DCP_BWS_ROW
        finish_pair(a, po, pp, s, x, bad, lane);
    }
}

template <class Real> int launch(int R, dcp_fwd_args const &a, Post const &po, hipStream_t st)
{
    dim3 const grid((a.nwaves + 3u) / 4u), block(256);
    switch (R)
    {
    case 0: hipLaunchKernelGGL((backward_scaled_wide_kernel<Real>), grid, block, 0, st, a, po); return 0;
    case 1: hipLaunchKernelGGL((backward_scaled_kernel<Real, 1>), grid, block, 0, st, a, po); return 0;
    case 2: hipLaunchKernelGGL((backward_scaled_kernel<Real, 2>), grid, block, 0, st, a, po); return 0;
    case 4: hipLaunchKernelGGL((backward_scaled_kernel<Real, 4>), grid, block, 0, st, a, po); return 0;
    default: return 1;
    }
}

} // namespace

extern "C" int dcp_backward_scaled_launch(int precision, int R, struct dcp_fwd_args const *a, double const *rows_f,
                                          double const *alt_fwd, struct dcp_fwd_pair *redo, uint32_t *nredo, uint32_t redo_cap,
                                          int band, void *stream)
{
    if (dcp_fwd_args_refused(a, R, DCP_FWD_STORE_ROWS)) return 1; // Backward always writes its records
    if (R == 0 && a->work_stride % DCP_BWS_WORK_ROWS) return 1;  // a work area sized for another sweep
    if (!rows_f || !alt_fwd || !redo || !nredo || redo_cap == 0 || band < 1 || band > 500) return 1;
    Post const po{rows_f, alt_fwd, redo, nredo, redo_cap, band};
    hipStream_t const st = (hipStream_t)stream;
    if (precision == 32) return launch<float>(R, *a, po, st);
    if (precision == 64) return launch<double>(R, *a, po, st);
    return 1;
}
