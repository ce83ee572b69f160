// dcp_forward_scaled.hip -- gfx950 kernels of the scaled probability-space Forward sweep (dcp_gpu_forward_pairs_scaled,
// dcp_gpu_forward_dense_scaled).  The rule is dcp_forward_scaled.h's; the layout is dcp_forward.hip's:
//
//  forward_scaled_kernel<Real, R>   one (sequence, profile) pair per wavefront, R = 1, 2 or 4 consecutive nodes per lane,
//                                   the profile's transition factors and the history rings in registers.
//  forward_scaled_wide_kernel<Real> wider profiles, row-major over chunks of 256 columns, the rings of P and Q and the
//                                   row's M, I, D in the wavefront's work area, and behind them the profile's
//                                   eight rows of transition factors (21 x ldk doubles; a lane reads back only what
//                                   it wrote itself).
//
// Values are probabilities beside one exponent per pair (and one for the null state R): M and I are five fused
// multiply-adds each onto the factors of the five word codes, the delete chain D_k = a_k + dd_k D_{k-1} is closed by
// the six-step lane scan with (s1, c1) (+) (s2, c2) = (s1 s2, c2 + c1 s2) and the chunk's carry, E(j) is the wave sum in
// wave_sum's butterfly order.  Transitions are exponentiated once per pair (the wide sweep: into its work area), insert and null
// emissions once per row, match emissions on load.  After a row the wave-uniform ref decides on a rescaling of every
// ring value; a non-finite E, B or ring value (a D or M among them shows in E) ends the pair: it is appended to the
// launch's redo list, which the driver hands to the log-space kernels.
//
// A column at or past core_size is never loaded: its factors are 0, so the padding columns carry 0 and stay 0.
//
// Both sweeps take a compile-time flag ROWS: lanes 0 .. 4 also store the row's record for the posteriors (PN, PJ, PC,
// B, E) as five logs under the exponent in force, what dcp_gpu_posterior_pairs_scaled's Backward sweep and the combining
// kernel read (dcp_backward_scaled.h).  ROWS = false is the scores-only kernel, with the registers it had
// before the flag.
#include "dcp_forward_scaled.h"
#include "dcp_host.h"

#include <hip/hip_runtime.h>

#include "dcp_forward_dev.h"

namespace
{

struct Redo // where a launch leaves the pairs it could not sweep
{
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

// The row's ten wave-uniform factors -- insert and null emissions of the five word codes -- one per lane: lane l < 5
// forms the insert factor of code l, lane 5 + l the null factor of code l (the other lanes repeat lane 0's), and
// every lane reads them from there: fI[l] and fN[l] are scalars, and the rule's bits.
template <class Real>
__device__ __forceinline__ void row_factors(Tabs<Real> const &g, unsigned w, unsigned lane, double (&fI)[5], double (&fN)[5])
{
    unsigned const l = lane < 5u ? lane : lane < 10u ? lane - 5u : 0u;
    // word_codes' code of length l + 1: offset (4^l - 1) / 3 x 4, the word's last l + 1 bases
    unsigned const code = ((0x55555555u & ((1u << (2u * l)) - 1u)) << 2) + (w & ((4u << (2u * l)) - 1u));
    double const f = dcp_fws_factor((lane >= 5u && lane < 10u ? g.en : g.ei)[code]);
#pragma unroll
    for (int i = 0; i < 5; ++i)
        fI[i] = readlane(f, i), fN[i] = readlane(f, 5 + i);
}

struct XS // the pair's special transitions as factors
{
    double NB, EB, JB, ET, CT;
    double xa, xb; // this lane's own special state X of N, J, C, R: PX(j) = E(j) xa + X(j) xb
};

template <class Real> __device__ __forceinline__ XS special_factors(double const *xt, unsigned lane)
{
    XS x;
    x.NB = fac_of<Real>(xt[DCP_X_NB]), x.EB = fac_of<Real>(xt[DCP_X_EB]), x.JB = fac_of<Real>(xt[DCP_X_JB]);
    x.ET = fac_of<Real>(xt[DCP_X_ET]), x.CT = fac_of<Real>(xt[DCP_X_CT]);
    unsigned const sp = lane & 3u;
    x.xa = sp == 1u ? fac_of<Real>(xt[DCP_X_EJ]) : sp == 2u ? fac_of<Real>(xt[DCP_X_EC]) : 0.0; // N and R: no edge from E
    x.xb = fac_of<Real>(sp == 0u ? xt[DCP_X_NN] : sp == 1u ? xt[DCP_X_JJ] : sp == 2u ? xt[DCP_X_CC] : xt[DCP_X_RR]);
    return x;
}

// row 0 of the lane's special state: N = SN, R starts at 1, J and C at 0
template <class Real> __device__ __forceinline__ double special_row0_fac(double const *xt, unsigned lane)
{
    unsigned const sp = lane & 3u;
    return sp == 0u ? fac_of<Real>(xt[DCP_X_SN]) : sp == 3u ? 1.0 : 0.0;
}

// D of the lane's R nodes: a[r] = M_{k-1} md_k, dd[r] = dd_k, carry = D of the node before lane 0's first
template <int R>
__device__ __forceinline__ void delete_chain_scaled(double const (&a)[R], double const (&dd)[R], double carry, double (&d)[R],
                                                    unsigned lane)
{
    double c = a[0], s = dd[0]; // the lane's chain from d_in = 0, and the product of its dd
#pragma unroll
    for (int r = 1; r < R; ++r)
    {
        c = dcp_fws_fma(dd[r], c, a[r]);
        s = s * dd[r];
    }
#pragma unroll
    for (unsigned o = 1; o < 64u; o <<= 1)
    {
        double const sp = __shfl_up(s, o, 64), cp = __shfl_up(c, o, 64);
        if (lane >= o)
        {
            c = dcp_fws_fma(cp, s, c);
            s = sp * s;
        }
    }
    // lanes 0 .. l - 1 composed, applied to the carry: lane 0 receives (1, 0), the identity
    double const cb = shr1(c, 0.0), sb = shr1(s, 1.0);
    // (a chain that carries no mass has D = 0 by the rule, whatever its dd: the product sb may have left the range,
    // and 0 x inf is no value of the rule)
    double const d_in = carry != 0.0 ? dcp_fws_fma(carry, sb, cb) : cb;
    d[0] = dcp_fws_fma(dd[0], d_in, a[0]);
#pragma unroll
    for (int r = 1; r < R; ++r)
        d[r] = dcp_fws_fma(dd[r], d[r - 1], a[r]);
}

// what the rows share beside the rings: the special states' ring of the lane, the row's E, C, R, the two exponents
struct Specials
{
    double PX[5];
    double E, Cc, Rr;
    int sA, sR;
    unsigned w;
};

// After a row: the rescaling steps of the alt group (kA) and of R (kR), from the row's PN, PJ, PC (lanes 0 .. 2 of px),
// E and B, and PR (lane 3).  Both wave-uniform; 0: none.
__device__ __forceinline__ void rescale_steps(double px, double E, double B, int band, int &kA, int &kR)
{
    double const pn = readlane(px, 0), pj = readlane(px, 1), pc = readlane(px, 2), pr = readlane(px, 3);
    double const ref = dcp_fwd_max(dcp_fwd_max(dcp_fwd_max(pn, pj), dcp_fwd_max(pc, E)), B);
    kA = dcp_fws_rescale_by(ref, band);
    kR = dcp_fws_rescale_by(pr, band);
}

__device__ __forceinline__ void rescale_specials(Specials &s, int kA, int kR, unsigned lane)
{
    double const cA = dcp_fws_pow2(-kA), cR = dcp_fws_pow2(-kR);
    double const cX = (lane & 3u) == 3u ? cR : cA;
#pragma unroll
    for (int h = 0; h < 5; ++h)
        s.PX[h] *= cX;
    s.E *= cA, s.Cc *= cA, s.Rr *= cR;
    s.sA += kA, s.sR += kR;
}

// Row 0 under the rescaling rule, before its P is formed: ref = max(PN, B) = max(SN, SB).  Returns B for row 0's P.
__device__ __forceinline__ double rescale_row0(double B0, Specials &s, int band, unsigned lane)
{
    double const sn = readlane(s.PX[0], 0);
    if (!dcp_fws_finite(sn) || !dcp_fws_finite(B0)) return B0; // row 1 ends the pair
    int const k = dcp_fws_rescale_by(dcp_fwd_max(sn, B0), band);
    if (k == 0) return B0;
    double const c = dcp_fws_pow2(-k);
    if ((lane & 3u) != 3u) s.PX[0] *= c;
    s.sA = k;
    return B0 * c;
}

__device__ __forceinline__ void finish_pair(dcp_fwd_args const &a, Redo const &rd, dcp_fwd_pair const &pp, Specials const &s,
                                            XS const &x, bool bad, unsigned lane)
{
    double alt = 0.0;
    int sA = s.sA;
    if (!bad)
    {
        // the last row's E and C with the larger of them in [1, 2): the product with ET, CT near e^-708 stays normal
        int const k = dcp_fws_rescale_by(dcp_fwd_max(s.E, s.Cc), 0);
        double const c = dcp_fws_pow2(-k);
        alt = dcp_fws_fma(s.Cc * c, x.CT, (s.E * c) * x.ET);
        sA += k;
        bad = !dcp_fws_finite(alt);
    }
    if (lane == 0u)
    {
        if (bad)
        {
            uint32_t const at = atomicAdd(rd.count, 1u);
            if (at < rd.cap) rd.list[at] = pp;
        }
        a.out_null[pp.pos] = bad ? ninf() : dcp_fws_score(s.Rr, s.sR);
        a.out_alt[pp.pos] = bad ? ninf() : dcp_fws_score(alt, sA);
    }
}

// ROWS: the row's record for the posteriors (dcp_posterior.h) -- PN(j), PJ(j), PC(j), B(j), E(j) -- as logs under the
// exponent in force, one per lane: lanes 0 .. 2 hold their own state's value in px, lane 3 takes B, lane 4 E
__device__ __forceinline__ void store_record(double px, double B, double E, int sA, double *rec, unsigned lane)
{
    double const v = lane < 3u ? px : lane == 3u ? B : E;
    double const lg = dcp_fws_score(v, sA);
    if (lane < 5u) rec[lane] = lg;
}

// ---- profiles of at most 64 R nodes: everything in registers -------------------------------------------------------
template <int R> struct Trans
{
    double ent[R], mm[R], im[R], dm[R], md[R], dd[R], mi[R], ii[R];
};

template <int R> struct Rings
{
    double P[5][R], Q[5][R];
};

// one row; returns true if a value left the double range (wave-uniform)
template <class Real, int R, int PH, bool ROWS>
__device__ __forceinline__ bool scaled_row(Rings<R> &g5, Specials &s, Trans<R> const &t, XS const &x, Tabs<Real> const &g,
                                           unsigned j, unsigned lane, int band, double *rec)
{
    constexpr int sl[5] = {(PH + 4) % 5, (PH + 3) % 5, (PH + 2) % 5, (PH + 1) % 5, PH}; // slot of row j - l
    unsigned const i = j - 1u;
    s.w = ((s.w << 2) | ((g.words[i >> 4] >> ((i & 15u) * 2u)) & 3u)) & 1023u;
    unsigned code[5];
    word_codes(s.w, code);
    unsigned const k0 = lane * R;

    double fI[5], fN[5];
    row_factors(g, s.w, lane, fI, fN);
    double m[R], ins[R], X = 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r)
        m[r] = ins[r] = 0.0;
#pragma unroll
    for (int l = 0; l < 5; ++l)
    {
        Real const *em = g.tab + (uint64_t)code[l] * g.ld;
#pragma unroll
        for (int r = 0; r < R; ++r)
        {
            m[r] = dcp_fws_fma(g5.P[sl[l]][r], load_fac(em, k0 + r, g.M), m[r]);
            ins[r] = dcp_fws_fma(g5.Q[sl[l]][r], fI[l], ins[r]);
        }
        X = dcp_fws_fma(s.PX[sl[l]], fN[l], X);
    }

    double a[R], d[R];
    a[0] = shr1(m[R - 1], 0.0) * t.md[0];
#pragma unroll
    for (int r = 1; r < R; ++r)
        a[r] = m[r - 1] * t.md[r];
    delete_chain_scaled<R>(a, t.dd, 0.0, d, lane);

    double sum = m[0] + d[0];
#pragma unroll
    for (int r = 1; r < R; ++r)
        sum = sum + m[r] + d[r];
    double const E = readlane(wave_sum(sum), 0);
    double const N = readlane(X, 0), J = readlane(X, 1), Cc = readlane(X, 2), Rr = readlane(X, 3);
    double B = N * x.NB;
    B = dcp_fws_fma(E, x.EB, B);
    B = dcp_fws_fma(J, x.JB, B);

    double const mp = shr1(m[R - 1], 0.0), ip = shr1(ins[R - 1], 0.0), dp = shr1(d[R - 1], 0.0);
    bool fin = true;
#pragma unroll
    for (int r = 0; r < R; ++r)
    {
        double p = B * t.ent[r];
        p = dcp_fws_fma(r ? m[r - 1] : mp, t.mm[r], p);
        p = dcp_fws_fma(r ? ins[r - 1] : ip, t.im[r], p);
        p = dcp_fws_fma(r ? d[r - 1] : dp, t.dm[r], p);
        double const q = dcp_fws_fma(ins[r], t.ii[r], m[r] * t.mi[r]);
        g5.P[PH][r] = p, g5.Q[PH][r] = q;
        fin = fin && dcp_fws_finite(p) && dcp_fws_finite(q);
    }
    double const px = dcp_fws_fma(X, x.xb, E * x.xa);
    s.PX[PH] = px;
    s.E = E, s.Cc = Cc, s.Rr = Rr;
    fin = fin && dcp_fws_finite(px) && dcp_fws_finite(E) && dcp_fws_finite(B);
    if (__any(!fin)) return true;
    if constexpr (ROWS) store_record(px, B, E, s.sA, rec + (uint64_t)DCP_POST_REC * j, lane);

    int kA, kR;
    rescale_steps(px, E, B, band, kA, kR);
    if (kA | kR)
    {
        if (kA)
        {
            double const cA = dcp_fws_pow2(-kA);
#pragma unroll
            for (int h = 0; h < 5; ++h)
#pragma unroll
                for (int r = 0; r < R; ++r)
                    g5.P[h][r] *= cA, g5.Q[h][r] *= cA;
        }
        rescale_specials(s, kA, kR, lane);
    }
    return false;
}

template <class Real, int R, bool ROWS> __global__ __launch_bounds__(256) void forward_scaled_kernel(dcp_fwd_args a, Redo rd)
{
    unsigned const lane = threadIdx.x & 63u;
    uint64_t const gw = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    uint64_t const nw = a.nwaves;
    if (gw >= nw) return; // the grid's last block may hold wavefronts past nwaves
    for (uint64_t pair = gw; pair < a.npairs; pair += nw)
    {
        auto const [pp, pr, L, xt] = pair_head(a, pair);
        XS const x = special_factors<Real>(xt, lane);
        Tabs<Real> const g = tables_of<Real>(a, pr, pp.q);
        unsigned const k0 = lane * R;
        // row 0 of the special states and its rescaling, anew for every pair: S = 1, B = SB
        Specials s;
#pragma unroll
        for (int h = 1; h < 5; ++h)
            s.PX[h] = 0.0;
        s.PX[0] = special_row0_fac<Real>(xt, lane);
        s.E = s.Cc = s.Rr = 0.0;
        s.sA = s.sR = 0;
        s.w = 0u;
        double const B0 = rescale_row0(fac_of<Real>(xt[DCP_X_SB]), s, rd.band, lane);
        Trans<R> t;
#pragma unroll
        for (int r = 0; r < R; ++r)
        {
            t.ent[r] = load_fac(g.trans + DCP_T_ENTRY * g.ld, k0 + r, g.M);
            t.mm[r] = load_fac(g.trans + DCP_T_MM * g.ld, k0 + r, g.M);
            t.im[r] = load_fac(g.trans + DCP_T_IM * g.ld, k0 + r, g.M);
            t.dm[r] = load_fac(g.trans + DCP_T_DM * g.ld, k0 + r, g.M);
            t.md[r] = load_fac(g.trans + DCP_T_MD * g.ld, k0 + r, g.M);
            t.dd[r] = load_fac(g.trans + DCP_T_DD * g.ld, k0 + r, g.M);
            t.mi[r] = load_fac(g.trans + DCP_T_MI * g.ld, k0 + r, g.M);
            t.ii[r] = load_fac(g.trans + DCP_T_II * g.ld, k0 + r, g.M);
        }
        // row 0 of the rings: 0 but for row 0's slot
        Rings<R> g5;
#pragma unroll
        for (int h = 0; h < 5; ++h)
#pragma unroll
            for (int r = 0; r < R; ++r)
                g5.P[h][r] = g5.Q[h][r] = 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r)
            g5.P[0][r] = B0 * t.ent[r];
        double *rec = nullptr;
        if constexpr (ROWS)
        {
            rec = record_of(a, pp);
            store_record(s.PX[0], B0, 0.0, s.sA, rec, lane); // row 0: PN = SN, B = SB, no J, C, E yet
        }
        bool bad = false;
        unsigned j = 1u;
#define DCP_FWS_ROW(PH)                                                                                                \
    bad = scaled_row<Real, R, PH, ROWS>(g5, s, t, x, g, j, lane, rd.band, rec);                                        \
    if (bad || j == L) break;                                                                                          \
    ++j;
        for (;;)
        {
            DCP_FWS_ROW(1)
            DCP_FWS_ROW(2)
            DCP_FWS_ROW(3)
            DCP_FWS_ROW(4)
            DCP_FWS_ROW(0)
        }
#undef DCP_FWS_ROW
        finish_pair(a, rd, pp, s, x, bad, lane);
    }
}

// ---- wider profiles: row-major over chunks of 256 columns, the rings in the wavefront's work area ------------------
// The scaled sweep's work area has eight rows more than the log-space sweep's thirteen (DCP_FWS_WORK_ROWS): the
// profile's transition factors, row DCP_T_* of them behind the row's M, I, D, written once per pair, every lane its own
// columns.
__device__ __forceinline__ double *trans_fac(WideArea const &wa, int which)
{
    return wa.base + (uint64_t)(DCP_FWD_WORK_ROWS + which) * wa.ldk;
}

template <class Real, int PH, bool ROWS>
__device__ __forceinline__ bool scaled_wide_row(Specials &s, XS const &x, Tabs<Real> const &g, WideArea const &wa, unsigned j,
                                                unsigned lane, int band, double *rec)
{
    constexpr int sl[5] = {(PH + 4) % 5, (PH + 3) % 5, (PH + 2) % 5, (PH + 1) % 5, PH};
    unsigned const i = j - 1u;
    s.w = ((s.w << 2) | ((g.words[i >> 4] >> ((i & 15u) * 2u)) & 3u)) & 1023u;
    unsigned code[5];
    word_codes(s.w, code);
    double fI[5], fN[5], X = 0.0;
    row_factors(g, s.w, lane, fI, fN);
#pragma unroll
    for (int l = 0; l < 5; ++l)
        X = dcp_fws_fma(s.PX[sl[l]], fN[l], X);

    // first pass: M, I, D of the row, chunk after chunk, and E over all of them
    double E = 0.0;
    double em_ = 0.0, ed_ = 0.0; // M, D of the chunk's last node
    for (unsigned ch = 0; ch < wa.nchunks; ++ch)
    {
        unsigned const k0 = ch * (unsigned)DCP_FWD_CHUNK + lane * WR;
        double m[WR], ins[WR], a[WR], dd[WR], d[WR];
#pragma unroll
        for (int r = 0; r < WR; ++r)
            m[r] = ins[r] = 0.0;
#pragma unroll
        for (int l = 0; l < 5; ++l)
        {
            Real const *em = g.tab + (uint64_t)code[l] * g.ld;
            double const *p = wa.ring0(sl[l]) + k0, *q = wa.ring1(sl[l]) + k0;
#pragma unroll
            for (int r = 0; r < WR; ++r)
            {
                m[r] = dcp_fws_fma(p[r], load_fac(em, k0 + r, g.M), m[r]);
                ins[r] = dcp_fws_fma(q[r], fI[l], ins[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < WR; ++r)
            dd[r] = trans_fac(wa, DCP_T_DD)[k0 + r];
        a[0] = shr1(m[WR - 1], em_) * trans_fac(wa, DCP_T_MD)[k0];
#pragma unroll
        for (int r = 1; r < WR; ++r)
            a[r] = m[r - 1] * trans_fac(wa, DCP_T_MD)[k0 + r];
        delete_chain_scaled<WR>(a, dd, ed_, d, lane);
        double *const wm = wa.row(0) + k0, *const wi = wa.row(1) + k0, *const wd = wa.row(2) + k0;
        double sum = 0.0;
#pragma unroll
        for (int r = 0; r < WR; ++r)
        {
            wm[r] = m[r], wi[r] = ins[r], wd[r] = d[r];
            sum = r ? sum + m[r] + d[r] : m[0] + d[0];
        }
        E = E + readlane(wave_sum(sum), 0);
        em_ = readlane(m[WR - 1], 63), ed_ = readlane(d[WR - 1], 63);
    }
    double const N = readlane(X, 0), J = readlane(X, 1), Cc = readlane(X, 2), Rr = readlane(X, 3);
    double B = N * x.NB;
    B = dcp_fws_fma(E, x.EB, B);
    B = dcp_fws_fma(J, x.JB, B);

    // second pass: row j's edges into the next rows, into slot j mod 5
    bool fin = true;
    double bm = 0.0, bi = 0.0, bd = 0.0;
    for (unsigned ch = 0; ch < wa.nchunks; ++ch)
    {
        unsigned const k0 = ch * (unsigned)DCP_FWD_CHUNK + lane * WR;
        double const *wm = wa.row(0) + k0, *wi = wa.row(1) + k0, *wd = wa.row(2) + k0;
        double m[WR], ins[WR], d[WR];
#pragma unroll
        for (int r = 0; r < WR; ++r)
            m[r] = wm[r], ins[r] = wi[r], d[r] = wd[r];
        double pm[WR], pi[WR], pd[WR]; // node k - 1's values
        pm[0] = shr1(m[WR - 1], bm), pi[0] = shr1(ins[WR - 1], bi), pd[0] = shr1(d[WR - 1], bd);
#pragma unroll
        for (int r = 1; r < WR; ++r)
            pm[r] = m[r - 1], pi[r] = ins[r - 1], pd[r] = d[r - 1];
        double *const p = wa.ring0(PH) + k0, *const q = wa.ring1(PH) + k0;
#pragma unroll
        for (int r = 0; r < WR; ++r)
        {
            unsigned const k = k0 + r;
            double v = B * trans_fac(wa, DCP_T_ENTRY)[k];
            v = dcp_fws_fma(pm[r], trans_fac(wa, DCP_T_MM)[k], v);
            v = dcp_fws_fma(pi[r], trans_fac(wa, DCP_T_IM)[k], v);
            v = dcp_fws_fma(pd[r], trans_fac(wa, DCP_T_DM)[k], v);
            double const u = dcp_fws_fma(ins[r], trans_fac(wa, DCP_T_II)[k], m[r] * trans_fac(wa, DCP_T_MI)[k]);
            p[r] = v, q[r] = u;
            fin = fin && dcp_fws_finite(v) && dcp_fws_finite(u);
        }
        bm = readlane(m[WR - 1], 63), bi = readlane(ins[WR - 1], 63), bd = readlane(d[WR - 1], 63);
    }
    double const px = dcp_fws_fma(X, x.xb, E * x.xa);
    s.PX[PH] = px;
    s.E = E, s.Cc = Cc, s.Rr = Rr;
    fin = fin && dcp_fws_finite(px) && dcp_fws_finite(E) && dcp_fws_finite(B);
    if (__any(!fin)) return true;
    if constexpr (ROWS) store_record(px, B, E, s.sA, rec + (uint64_t)DCP_POST_REC * j, lane);

    int kA, kR;
    rescale_steps(px, E, B, band, kA, kR);
    if (kA | kR)
    {
        if (kA)
        {
            // the ten ring rows of the work area, every lane its own columns
            double const cA = dcp_fws_pow2(-kA);
            for (unsigned ch = 0; ch < wa.nchunks; ++ch)
            {
                unsigned const k0 = ch * (unsigned)DCP_FWD_CHUNK + lane * WR;
#pragma unroll
                for (unsigned h = 0; h < 5u; ++h)
#pragma unroll
                    for (int r = 0; r < WR; ++r)
                        wa.ring0(h)[k0 + r] *= cA, wa.ring1(h)[k0 + r] *= cA;
            }
        }
        rescale_specials(s, kA, kR, lane);
    }
    return false;
}

template <class Real, bool ROWS> __global__ __launch_bounds__(256) void forward_scaled_wide_kernel(dcp_fwd_args a, Redo rd)
{
    unsigned const lane = threadIdx.x & 63u;
    uint64_t const gw = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    uint64_t const nw = a.nwaves;
    if (gw >= nw) return; // wavefronts past nwaves have no work area
    for (uint64_t pair = gw; pair < a.npairs; pair += nw)
    {
        auto const [pp, pr, L, xt] = pair_head(a, pair);
        XS const x = special_factors<Real>(xt, lane);
        Tabs<Real> const g = tables_of<Real>(a, pr, pp.q);
        WideArea const wa = wide_area(a.work, a.work_stride, gw, pr.core_size);
        // row 0, anew for every pair (the pair before may have been of another width): the rings' own columns
        Specials s;
#pragma unroll
        for (int h = 0; h < 5; ++h)
            s.PX[h] = 0.0;
        s.PX[0] = special_row0_fac<Real>(xt, lane);
        s.E = s.Cc = s.Rr = 0.0;
        s.sA = s.sR = 0;
        s.w = 0u;
        double const B0 = rescale_row0(fac_of<Real>(xt[DCP_X_SB]), s, rd.band, lane);
        for (unsigned ch = 0; ch < wa.nchunks; ++ch)
        {
            unsigned const k0 = ch * (unsigned)DCP_FWD_CHUNK + lane * WR;
#pragma unroll
            for (int r = 0; r < WR; ++r)
            {
#pragma unroll
                for (int t = 0; t < 8; ++t)
                    trans_fac(wa, t)[k0 + r] = load_fac(g.trans + (uint64_t)t * g.ld, k0 + r, g.M);
                wa.ring0(0)[k0 + r] = B0 * trans_fac(wa, DCP_T_ENTRY)[k0 + r];
                wa.ring1(0)[k0 + r] = 0.0;
#pragma unroll
                for (int h = 1; h < 5; ++h)
                    wa.ring0(h)[k0 + r] = wa.ring1(h)[k0 + r] = 0.0;
            }
        }
        double *rec = nullptr;
        if constexpr (ROWS)
        {
            rec = record_of(a, pp);
            store_record(s.PX[0], B0, 0.0, s.sA, rec, lane);
        }
        bool bad = false;
        unsigned j = 1u;
#define DCP_FWS_ROW(PH)                                                                                                \
    bad = scaled_wide_row<Real, PH, ROWS>(s, x, g, wa, j, lane, rd.band, rec);                                         \
    if (bad || j == L) break;                                                                                          \
    ++j;
        for (;;)
        {
            DCP_FWS_ROW(1)
            DCP_FWS_ROW(2)
            DCP_FWS_ROW(3)
            DCP_FWS_ROW(4)
            DCP_FWS_ROW(0)
        }
#undef DCP_FWS_ROW
        finish_pair(a, rd, pp, s, x, bad, lane);
    }
}

template <class Real, bool ROWS> int launch(int R, dcp_fwd_args const &a, Redo const &rd, hipStream_t st)
{
    dim3 const grid((a.nwaves + 3u) / 4u), block(256);
    switch (R)
    {
    case 0: hipLaunchKernelGGL((forward_scaled_wide_kernel<Real, ROWS>), grid, block, 0, st, a, rd); return 0;
    case 1: hipLaunchKernelGGL((forward_scaled_kernel<Real, 1, ROWS>), grid, block, 0, st, a, rd); return 0;
    case 2: hipLaunchKernelGGL((forward_scaled_kernel<Real, 2, ROWS>), grid, block, 0, st, a, rd); return 0;
    case 4: hipLaunchKernelGGL((forward_scaled_kernel<Real, 4, ROWS>), grid, block, 0, st, a, rd); return 0;
    default: return 1;
    }
}

template <bool ROWS> int launch(int precision, int R, dcp_fwd_args const &a, Redo const &rd, hipStream_t st)
{
    if (precision == 32) return launch<float, ROWS>(R, a, rd, st);
    if (precision == 64) return launch<double, ROWS>(R, a, rd, st);
    return 1;
}

} // namespace

extern "C" int dcp_forward_scaled_launch(int precision, int R, int store, struct dcp_fwd_args const *a, struct dcp_fwd_pair *redo,
                                         uint32_t *nredo, uint32_t redo_cap, int band, void *stream)
{
    if (store > DCP_FWD_STORE_ROWS || dcp_fwd_args_refused(a, R, store)) return 1; // there is no matrix-storing variant
    if (R == 0 && a->work_stride % DCP_FWS_WORK_ROWS) return 1; // a work area sized for the log-space sweep
    if (!redo || !nredo || redo_cap == 0 || band < 1 || band > 500) return 1;
    Redo const rd{redo, nredo, redo_cap, band};
    hipStream_t const st = (hipStream_t)stream;
    if (store == DCP_FWD_STORE_ROWS) return launch<true>(precision, R, *a, rd, st);
    return launch<false>(precision, R, *a, rd, st);
}
