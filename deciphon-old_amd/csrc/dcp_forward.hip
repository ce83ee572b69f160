// dcp_forward.hip -- gfx950 kernels of the Forward scores of a pair list (dcp_gpu_forward_pairs).
//
//  forward_kernel<Real, R>   null + alt Forward score of one (sequence, profile) pair per wavefront, R = 1, 2 or 4
//                            consecutive nodes per lane, the whole profile (at most 64 R nodes) and its history rings
//                            in registers.
//  forward_wide_kernel<Real> the same for wider profiles, row-major: for each row the wavefront sweeps all chunks of
//                            256 columns in order, with the rings of P and Q and the row's M, I, D in a per-wavefront
//                            work area in global memory (13 x ldk doubles; a lane reads back only what it wrote
//                            itself), the edge values (M, I, D of the chunk's last node, the running E) carried from
//                            chunk to chunk in registers.  B(j) follows after the row's last chunk; a second pass over
//                            the chunks forms P(j) and Q(j) into slot j mod 5.
//
// Both take a compile-time flag ROWS: the same sweep that also stores, per row j = 0 .. L, the five values the posterior
// rows are built from -- PN(j), PJ(j), PC(j), B(j), E(j), dcp_posterior.h -- from lane 0 (dcp_gpu_posterior_pairs' first
// half).  ROWS = false is dcp_gpu_forward_pairs' kernel, with the registers it had before the flag.
// And a flag MAT, with ROWS: every lane also stores P_k(j) and Q_k(j) of its own columns, rows j = 0 .. L, the matrices
// the posterior-decoded alignment reads (dcp_mea.h, dcp_gpu_mea_pairs' first sweep).
//
//  dense_pairs_kernel        the pair records of one round of the dense scan (dcp_gpu_forward_dense): every resident
//                            sequence against every resident profile, one thread per record, so that no list of
//                            pairs is built on the host or copied up (dcp_forward.h: dcp_fwd_dense_args has the order).
//
// Real is the tables' scalar (a float DB's values are promoted to double, which is exact); the arithmetic is double.
// The recursion is the Viterbi one of dcp_f64.hip with every max replaced by lse (dcp_forward.h), every candidate
// (predecessor + transition) or (predecessor + emission) formed once.  Two things max allowed there do not carry over:
//  * the delete chain D_k = lse(M_{k-1} + MD_k, D_{k-1} + DD_k) is a linear recurrence, not a fixed point: a lane's R
//    nodes compose to d_out = lse(c, d_in + s), pairs combine as (s1, c1) (+) (s2, c2) = (s1 + s2, lse(c2, c1 + s2)),
//    an inclusive scan over the 64 lanes (six steps) and the carry of the chunk before give every lane its true d_in,
//    and the lane's chain is run again from it;
//  * E(j) over the lanes is a sum: the wave's maximum, every lane's terms scaled by it and added, the lanes' sums added
//    by a butterfly (the same tree in every lane), chunks merged in the running form.
// The four special states that emit (N, J, C, R) are one state per lane: lane l & 3 keeps the ring of its own one,
// and the row's values are read from lanes 0 .. 3.
//
// A column at or past core_size is never loaded: its transitions and emissions are -inf by construction here, so the
// padding columns carry -inf and stay -inf, whatever the DB's own padding is (a float DB's small profiles share rows).
#include "dcp_forward.h"
#include "dcp_host.h"
#include "dcp_mea.h"
#include "dcp_posterior.h"

#include <hip/hip_runtime.h>

#include "dcp_forward_dev.h"

namespace
{

// ---- profiles of at most 64 R nodes: everything in registers -------------------------------------------------------
template <int R> struct Trans
{
    double ent[R], mm[R], im[R], dm[R], md[R], dd[R], mi[R], ii[R];
};

// history rings (State64's shape, dcp_f64.hip): row j's predecessors j - 1 .. j - 5 live in slots (j - l) % 5
template <int R> struct State
{
    double P[5][R], Q[5][R];
    double PX[5]; // the lane's own special state
    double E, Cc, Rr;
    unsigned w;
};

// ROWS: the row's record for the posteriors (dcp_posterior.h) -- PN(j), PJ(j), PC(j), B(j), E(j) -- goes to rec from lane 0
template <int PH> __device__ __forceinline__ void store_record(double const (&PX)[5], double B, double E, double *rec, unsigned lane)
{
    double const pn = readlane(PX[PH], 0), pj = readlane(PX[PH], 1), pc = readlane(PX[PH], 2);
    if (lane == 0u) rec[0] = pn, rec[1] = pj, rec[2] = pc, rec[3] = B, rec[4] = E;
}

// MAT: row j of the pair's P (m0) and Q (m1) matrices, the lane's own columns below core_size
template <int R>
__device__ __forceinline__ void store_cells(Mats const &mt, double const (&p)[R], double const (&q)[R], unsigned j, unsigned k0, unsigned M)
{
    uint64_t const at = (uint64_t)j * M;
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (k0 + r < M) mt.m0[at + k0 + r] = p[r], mt.m1[at + k0 + r] = q[r];
}

template <class Real, int R, int PH, bool ROWS, bool MAT>
__device__ __forceinline__ void forward_row(State<R> &s, Trans<R> const &t, XF const &x, Tabs<Real> const &g, unsigned j,
                                            unsigned lane, double *rec, Mats const &mt)
{
    constexpr int sl[5] = {(PH + 4) % 5, (PH + 3) % 5, (PH + 2) % 5, (PH + 1) % 5, PH}; // slot of row j - l
    unsigned const i = j - 1u;
    s.w = ((s.w << 2) | ((g.words[i >> 4] >> ((i & 15u) * 2u)) & 3u)) & 1023u;
    unsigned code[5];
    word_codes(s.w, code);
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
            cm[l][r] = s.P[sl[l]][r] + load_col(em, k0 + r, g.M);
            ci[l][r] = s.Q[sl[l]][r] + eI;
        }
        cx[l] = s.PX[sl[l]] + eN;
    }
    double m[R], ins[R];
#pragma unroll
    for (int r = 0; r < R; ++r)
    {
        m[r] = dcp_lse5(cm[0][r], cm[1][r], cm[2][r], cm[3][r], cm[4][r]);
        ins[r] = dcp_lse5(ci[0][r], ci[1][r], ci[2][r], ci[3][r], ci[4][r]);
    }
    double const X = dcp_lse5(cx[0], cx[1], cx[2], cx[3], cx[4]);

    double a[R], d[R];
    a[0] = shr1(m[R - 1], ninf()) + t.md[0];
#pragma unroll
    for (int r = 1; r < R; ++r)
        a[r] = m[r - 1] + t.md[r];
    delete_chain<R>(a, t.dd, ninf(), d, lane);

    double const E = dcp_lse_acc_value(exit_terms<R>(m, d));
    double const N = readlane(X, 0), J = readlane(X, 1), Cc = readlane(X, 2), Rr = readlane(X, 3);
    double const B = dcp_lse3(N + x.NB, E + x.EB, J + x.JB);

    double const mp = shr1(m[R - 1], ninf()), ip = shr1(ins[R - 1], ninf()), dp = shr1(d[R - 1], ninf());
    s.P[PH][0] = dcp_lse4(B + t.ent[0], mp + t.mm[0], ip + t.im[0], dp + t.dm[0]);
#pragma unroll
    for (int r = 1; r < R; ++r)
        s.P[PH][r] = dcp_lse4(B + t.ent[r], m[r - 1] + t.mm[r], ins[r - 1] + t.im[r], d[r - 1] + t.dm[r]);
#pragma unroll
    for (int r = 0; r < R; ++r)
        s.Q[PH][r] = dcp_lse2(m[r] + t.mi[r], ins[r] + t.ii[r]);
    s.PX[PH] = dcp_lse2(E + x.xa, X + x.xb);
    s.E = E, s.Cc = Cc, s.Rr = Rr;
    if constexpr (ROWS) store_record<PH>(s.PX, B, E, rec + (uint64_t)DCP_POST_REC * j, lane);
    if constexpr (MAT) store_cells<R>(mt, s.P[PH], s.Q[PH], j, k0, g.M);
}

template <class Real, int R, bool ROWS, bool MAT> __global__ __launch_bounds__(256) void forward_kernel(dcp_fwd_args a)
{
    unsigned const lane = threadIdx.x & 63u;
    uint64_t const gw = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    uint64_t const nw = a.nwaves;
    if (gw >= nw) return; // the grid's last block may hold wavefronts past nwaves
    for (uint64_t pair = gw; pair < a.npairs; pair += nw)
    {
        auto const [pp, pr, L, xt] = pair_head(a, pair);
        XF const x = special_transitions(xt, lane);
        Tabs<Real> const g = tables_of<Real>(a, pr, pp.q);
        unsigned const k0 = lane * R;
        Trans<R> t;
#pragma unroll
        for (int r = 0; r < R; ++r)
        {
            t.ent[r] = load_col(g.trans + DCP_T_ENTRY * g.ld, k0 + r, g.M);
            t.mm[r] = load_col(g.trans + DCP_T_MM * g.ld, k0 + r, g.M);
            t.im[r] = load_col(g.trans + DCP_T_IM * g.ld, k0 + r, g.M);
            t.dm[r] = load_col(g.trans + DCP_T_DM * g.ld, k0 + r, g.M);
            t.md[r] = load_col(g.trans + DCP_T_MD * g.ld, k0 + r, g.M);
            t.dd[r] = load_col(g.trans + DCP_T_DD * g.ld, k0 + r, g.M);
            t.mi[r] = load_col(g.trans + DCP_T_MI * g.ld, k0 + r, g.M);
            t.ii[r] = load_col(g.trans + DCP_T_II * g.ld, k0 + r, g.M);
        }
        // row 0, anew for every pair: S = 0, B = S + SB; the rings are -inf but for row 0's slot
        State<R> s;
#pragma unroll
        for (int h = 0; h < 5; ++h)
        {
#pragma unroll
            for (int r = 0; r < R; ++r)
                s.P[h][r] = s.Q[h][r] = ninf();
            s.PX[h] = ninf();
        }
        double const B0 = 0.0 + xt[DCP_X_SB];
#pragma unroll
        for (int r = 0; r < R; ++r)
            s.P[0][r] = B0 + t.ent[r];
        s.PX[0] = special_row0(xt, lane);
        s.E = s.Cc = s.Rr = ninf();
        s.w = 0u;
        double *rec = nullptr;
        if constexpr (ROWS)
        {
            rec = record_of(a, pp);
            store_record<0>(s.PX, B0, ninf(), rec, lane); // row 0: PN = SN, B = SB, no J, C, E yet
        }
        Mats mt{nullptr, nullptr};
        if constexpr (MAT)
        {
            mt = mats_of(a, pp);
            store_cells<R>(mt, s.P[0], s.Q[0], 0u, k0, g.M);
        }
        unsigned j = 1u;
#define DCP_FWD_ROW(PH)                                                                                                \
    forward_row<Real, R, PH, ROWS, MAT>(s, t, x, g, j, lane, rec, mt);                                                 \
    if (j == L) break;                                                                                                 \
    ++j;
        for (;;)
        {
            DCP_FWD_ROW(1)
            DCP_FWD_ROW(2)
            DCP_FWD_ROW(3)
            DCP_FWD_ROW(4)
            DCP_FWD_ROW(0)
        }
#undef DCP_FWD_ROW
        if (lane == 0u)
        {
            a.out_null[pp.pos] = s.Rr;
            a.out_alt[pp.pos] = dcp_lse2(s.E + x.ET, s.Cc + x.CT);
        }
    }
}

// ---- wider profiles: row-major over chunks of 256 columns, the rings in the wavefront's work area ------------------
// (WideArea: ring0 holds the slots of P, ring1 those of Q; rows 0 .. 2 the row's M, I, D)
struct WideState
{
    double PX[5];
    double E, Cc, Rr;
    unsigned w;
};

template <class Real, int PH, bool ROWS, bool MAT>
__device__ __forceinline__ void forward_wide_row(WideState &s, XF const &x, Tabs<Real> const &g, WideArea const &wa, unsigned j,
                                                 unsigned lane, double *rec, Mats const &mt)
{
    constexpr int sl[5] = {(PH + 4) % 5, (PH + 3) % 5, (PH + 2) % 5, (PH + 1) % 5, PH};
    unsigned const i = j - 1u;
    s.w = ((s.w << 2) | ((g.words[i >> 4] >> ((i & 15u) * 2u)) & 3u)) & 1023u;
    unsigned code[5];
    word_codes(s.w, code);
    double eI[5], cx[5];
#pragma unroll
    for (int l = 0; l < 5; ++l)
    {
        eI[l] = (double)g.ei[code[l]];
        cx[l] = s.PX[sl[l]] + (double)g.en[code[l]];
    }
    double const X = dcp_lse5(cx[0], cx[1], cx[2], cx[3], cx[4]);

    // first pass: M, I, D of the row, chunk after chunk, and E over all of them
    dcp_lse_acc acc = dcp_lse_acc_empty();
    double em_ = ninf(), ed_ = ninf(); // M, D of the chunk's last node
    for (unsigned ch = 0; ch < wa.nchunks; ++ch)
    {
        unsigned const k0 = ch * (unsigned)DCP_FWD_CHUNK + lane * WR;
        double cm[5][WR], ci[5][WR];
#pragma unroll
        for (int l = 0; l < 5; ++l)
        {
            Real const *em = g.tab + (uint64_t)code[l] * g.ld;
            double const *p = wa.ring0(sl[l]) + k0, *q = wa.ring1(sl[l]) + k0;
#pragma unroll
            for (int r = 0; r < WR; ++r)
            {
                cm[l][r] = p[r] + load_col(em, k0 + r, g.M);
                ci[l][r] = q[r] + eI[l];
            }
        }
        double m[WR], ins[WR], a[WR], dd[WR], d[WR];
#pragma unroll
        for (int r = 0; r < WR; ++r)
        {
            m[r] = dcp_lse5(cm[0][r], cm[1][r], cm[2][r], cm[3][r], cm[4][r]);
            ins[r] = dcp_lse5(ci[0][r], ci[1][r], ci[2][r], ci[3][r], ci[4][r]);
            dd[r] = load_col(g.trans + DCP_T_DD * g.ld, k0 + r, g.M);
        }
        a[0] = shr1(m[WR - 1], em_) + load_col(g.trans + DCP_T_MD * g.ld, k0, g.M);
#pragma unroll
        for (int r = 1; r < WR; ++r)
            a[r] = m[r - 1] + load_col(g.trans + DCP_T_MD * g.ld, k0 + r, g.M);
        delete_chain<WR>(a, dd, ed_, d, lane);
        double *const wm = wa.row(0) + k0, *const wi = wa.row(1) + k0, *const wd = wa.row(2) + k0;
#pragma unroll
        for (int r = 0; r < WR; ++r)
            wm[r] = m[r], wi[r] = ins[r], wd[r] = d[r];
        acc = dcp_lse_acc_merge(acc, exit_terms<WR>(m, d));
        em_ = readlane(m[WR - 1], 63), ed_ = readlane(d[WR - 1], 63);
    }
    double const E = dcp_lse_acc_value(acc);
    double const N = readlane(X, 0), J = readlane(X, 1), Cc = readlane(X, 2), Rr = readlane(X, 3);
    double const B = dcp_lse3(N + x.NB, E + x.EB, J + x.JB);

    // second pass: row j's edges into the next rows, into slot j mod 5
    double bm = ninf(), bi = ninf(), bd = ninf();
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
            p[r] = dcp_lse4(B + load_col(g.trans + DCP_T_ENTRY * g.ld, k, g.M), pm[r] + load_col(g.trans + DCP_T_MM * g.ld, k, g.M),
                            pi[r] + load_col(g.trans + DCP_T_IM * g.ld, k, g.M), pd[r] + load_col(g.trans + DCP_T_DM * g.ld, k, g.M));
            q[r] = dcp_lse2(m[r] + load_col(g.trans + DCP_T_MI * g.ld, k, g.M), ins[r] + load_col(g.trans + DCP_T_II * g.ld, k, g.M));
            if constexpr (MAT)
                if (k < g.M) mt.m0[(uint64_t)j * g.M + k] = p[r], mt.m1[(uint64_t)j * g.M + k] = q[r];
        }
        bm = readlane(m[WR - 1], 63), bi = readlane(ins[WR - 1], 63), bd = readlane(d[WR - 1], 63);
    }
    s.PX[PH] = dcp_lse2(E + x.xa, X + x.xb);
    s.E = E, s.Cc = Cc, s.Rr = Rr;
    if constexpr (ROWS) store_record<PH>(s.PX, B, E, rec + (uint64_t)DCP_POST_REC * j, lane);
}

template <class Real, bool ROWS, bool MAT> __global__ __launch_bounds__(256) void forward_wide_kernel(dcp_fwd_args a)
{
    unsigned const lane = threadIdx.x & 63u;
    uint64_t const gw = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    uint64_t const nw = a.nwaves;
    if (gw >= nw) return; // wavefronts past nwaves have no work area
    for (uint64_t pair = gw; pair < a.npairs; pair += nw)
    {
        auto const [pp, pr, L, xt] = pair_head(a, pair);
        XF const x = special_transitions(xt, lane);
        Tabs<Real> const g = tables_of<Real>(a, pr, pp.q);
        WideArea const wa = wide_area(a.work, a.work_stride, gw, pr.core_size);
        Mats mt{nullptr, nullptr};
        if constexpr (MAT) mt = mats_of(a, pp);
        // row 0, anew for every pair (the pair before may have been of another width): the rings' own columns
        double const B0 = 0.0 + xt[DCP_X_SB];
        for (unsigned ch = 0; ch < wa.nchunks; ++ch)
        {
            unsigned const k0 = ch * (unsigned)DCP_FWD_CHUNK + lane * WR;
#pragma unroll
            for (int r = 0; r < WR; ++r)
            {
                wa.ring0(0)[k0 + r] = B0 + load_col(g.trans + DCP_T_ENTRY * g.ld, k0 + r, g.M);
                wa.ring1(0)[k0 + r] = ninf();
                if constexpr (MAT)
                    if (k0 + r < g.M) mt.m0[k0 + r] = wa.ring0(0)[k0 + r], mt.m1[k0 + r] = ninf();
#pragma unroll
                for (int h = 1; h < 5; ++h)
                    wa.ring0(h)[k0 + r] = wa.ring1(h)[k0 + r] = ninf();
            }
        }
        WideState s;
#pragma unroll
        for (int h = 0; h < 5; ++h)
            s.PX[h] = ninf();
        s.PX[0] = special_row0(xt, lane);
        s.E = s.Cc = s.Rr = ninf();
        s.w = 0u;
        double *rec = nullptr;
        if constexpr (ROWS)
        {
            rec = record_of(a, pp);
            store_record<0>(s.PX, B0, ninf(), rec, lane);
        }
        unsigned j = 1u;
#define DCP_FWD_ROW(PH)                                                                                                \
    forward_wide_row<Real, PH, ROWS, MAT>(s, x, g, wa, j, lane, rec, mt);                                              \
    if (j == L) break;                                                                                                 \
    ++j;
        for (;;)
        {
            DCP_FWD_ROW(1)
            DCP_FWD_ROW(2)
            DCP_FWD_ROW(3)
            DCP_FWD_ROW(4)
            DCP_FWD_ROW(0)
        }
#undef DCP_FWD_ROW
        if (lane == 0u)
        {
            a.out_null[pp.pos] = s.Rr;
            a.out_alt[pp.pos] = dcp_lse2(s.E + x.ET, s.Cc + x.CT);
        }
    }
}

template <class Real, bool ROWS, bool MAT> int launch(int R, dcp_fwd_args const &a, hipStream_t st)
{
    dim3 const grid((a.nwaves + 3u) / 4u), block(256);
    switch (R)
    {
    case 0: hipLaunchKernelGGL((forward_wide_kernel<Real, ROWS, MAT>), grid, block, 0, st, a); return 0;
    case 1: hipLaunchKernelGGL((forward_kernel<Real, 1, ROWS, MAT>), grid, block, 0, st, a); return 0;
    case 2: hipLaunchKernelGGL((forward_kernel<Real, 2, ROWS, MAT>), grid, block, 0, st, a); return 0;
    case 4: hipLaunchKernelGGL((forward_kernel<Real, 4, ROWS, MAT>), grid, block, 0, st, a); return 0;
    default: return 1;
    }
}

// (float first, then double, of each variant in turn: the order in which the unit's kernels are emitted)
template <bool ROWS, bool MAT> int launch(int precision, int R, dcp_fwd_args const &a, hipStream_t st)
{
    if (precision == 32) return launch<float, ROWS, MAT>(R, a, st);
    if (precision == 64) return launch<double, ROWS, MAT>(R, a, st);
    return 1;
}

// ---- the dense scan's lists: one thread per record of a round (dcp_fwd_dense_args has the order) --------------------
__global__ __launch_bounds__(256) void dense_pairs_kernel(dcp_fwd_dense_args a)
{
    uint32_t const i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n) return;
    uint32_t const t = a.t0 + i;
    int k = 0;
    while (k < 3 && t >= a.nseqs * a.class_first[k + 1])
        ++k;
    uint32_t const local = t - a.nseqs * a.class_first[k], np = a.class_first[k + 1] - a.class_first[k];
    uint32_t const s = local / np;
    uint32_t const q = a.seq_order[s], prof = a.prof_order[a.class_first[k] + (local - s * np)];
    a.pairs[i] = dcp_fwd_pair{q, prof, q * a.nprof + prof};
}

} // namespace

extern "C" int dcp_forward_dense_pairs_launch(struct dcp_fwd_dense_args const *a, void *stream)
{
    if (!a || !a->seq_order || !a->prof_order || !a->pairs || a->n == 0 || a->nseqs == 0 || a->nprof == 0) return 1;
    if (a->class_first[0] != 0 || a->class_first[4] != a->nprof) return 1;
    for (int k = 0; k < 4; ++k)
        if (a->class_first[k] > a->class_first[k + 1]) return 1;
    uint64_t const total = (uint64_t)a->nseqs * a->nprof;
    if (total > 0xffffffffull || a->n > (1u << 30) || (uint64_t)a->t0 + a->n > total) return 1;
    hipLaunchKernelGGL(dense_pairs_kernel, dim3((a->n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, *a);
    return 0;
}

extern "C" int dcp_forward_launch(int precision, int R, int store, struct dcp_fwd_args const *a, void *stream)
{
    if (dcp_fwd_args_refused(a, R, store)) return 1;
    hipStream_t const st = (hipStream_t)stream;
    if (store == DCP_FWD_STORE_NONE) return launch<false, false>(precision, R, *a, st);
    if (store == DCP_FWD_STORE_ROWS) return launch<true, false>(precision, R, *a, st);
    return launch<true, true>(precision, R, *a, st);
}
