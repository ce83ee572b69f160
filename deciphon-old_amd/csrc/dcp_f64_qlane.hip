// dcp_f64_qlane.hip -- the query-lane kernel of the double build ("query-lane kernel").
//
//  viterbi64_qlane_kernel   null + alt Viterbi in double, one LANE per query: a block is 256 threads = four
//                           wavefront slots against ONE profile, each slot sweeping a list of 64-query groups of the
//                           length-sorted batch one after the other (the batch plan, dcp_f64.h).  The profile is cut
//                           into tiles of KT = 4 consecutive nodes; a tile is swept over all rows of a group with the
//                           five-row P_k / Q_k history of its nodes in registers, the delete chain sequential in k
//                           inside the lane, E(j) a running maximum, N / J / C and the null model's R per lane.  No
//                           cross-lane operation, no polling: the only synchronisation is the block barrier around
//                           the LDS images.
//
// Arithmetic contract: dcp_f64.hip's -- every candidate is one double add of the oracle's operands, combined with
// max only, -ffp-contract=off.  What differs from the row sweep is the ORDER in which exact maxima are taken
// (max is exact, so the order changes nothing) and where B(j) comes from:
//
// B(j) = max(N(j) + NB, E(j) + EB, J(j) + JB) needs E(j) over the whole profile.  The sweep runs with
// B0(j) = N(j) + NB; the last tile, which has the final E(j) and J(j), checks max(E(j) + EB, J(j) + JB) > B0(j) per
// row.  Where that never holds, B0 was B in every row and the lane's scores are the exact recursion's; such a lane
// publishes them.  A lane where it holds publishes nothing and appends {query, profile} to the redo list of the
// profile's launch group, which viterbi64_kernel<R, false, true> (dcp_f64.hip) scores right behind on the same stream.
// A uni-hit scan has EB = EJ = -inf: the check is never true.
//
// E(j) is taken over M_k AND D_k of every node always (as the row sweep does), so profiles with positive MD / DD
// need no flag.  Padding columns (core_size .. ldk) have -inf emissions and transitions: their M, I, D are -inf.
//
// Tile t hands row j to tile t + 1 through three per-block planes in global memory, [row][plane][lane] doubles (a
// group's rows in its own region of the slot's columns, from the group's rowbase on):
//   Xd = D of tile t + 1's first node (the end of tile t's delete chain),
//   Xm = max over the M / I / D edges into that node's M (the entry edge B + ENTRY is added by tile t + 1),
//   E  = the running maximum.
// A lane reads back only what it wrote itself (same address, same thread, program order), rows are prefetched PF = 5
// ahead into a register ring that turns with the history ring, and a tile overwrites row j in place after it has
// read it.  The last tile hands nothing over and does not touch the transition column behind it (which does not
// exist when core_size == ldk).
#include "dcp_f64.h"
#include "dcp_kernels.h" // dcp_ql_group

#include <hip/hip_runtime.h>

namespace
{

constexpr int KT = DCP_F64_QL_KT;
static_assert(KT == 4, "the image row is two 16-byte LDS reads");
constexpr unsigned NT = DCP_F64_QL_LANES;
constexpr unsigned PLANE_ROW = 3u * NT; // doubles per row of a block's planes

// comment marks in the ISA: one at the top of every row loop's body, one behind the loop
// (tests/test_f64_qlane_build.py finds the loops by them)
#define DCP_ISA_MARK(name) asm volatile("; " name)

__device__ __forceinline__ double ninf() { return -__builtin_inf(); }

__device__ __forceinline__ bool finite64(double v)
{
    return (__builtin_bit_cast(unsigned long long, v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// a uniform double the compiler cannot prove uniform (the planes are written by this kernel, so it will not use
// scalar loads for anything else): into scalar registers by hand
__device__ __forceinline__ double uni(double v)
{
    unsigned long long const b = __builtin_bit_cast(unsigned long long, v);
    unsigned const lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b);
    unsigned const hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(b >> 32));
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

struct QTrans // the tile's transitions and the edges into the next tile's first node: uniform, so scalar registers
{
    double ent[KT], mm[KT], im[KT], dm[KT], md[KT], dd[KT], mi[KT], ii[KT];
    double nmm, nim, ndm, nmd, ndd;
};

struct QX
{
    double RR, SB, SN, NN, NB, ET, EC, CC, CT, EB, EJ, JJ, JB;
};

struct QState // a tile's sweep
{
    double P[5][KT], Q[5][KT];
    double PN[5];
    double fxd[5], fxm[5], fe[5]; // rows j .. j + 4 of the planes, slot = row % 5
    unsigned w;                   // the last five bases, two bits each
    unsigned long long win;       // the words the next turn takes its bases from
};

struct SState // the special states' sweep behind the last tile
{
    double PN[5], PJ[5], PC[5], PR[5];
    double fe[5];
    double Cc, Rr; // of row L
    unsigned w;
    unsigned long long win;
    bool fb;
};

// Every lane of a group runs the rows of the group's LONGEST query (Lb, wave-uniform: the wavefront waits for that
// one anyway) in whole turns of the five-row ring, so the row loops' control flow is scalar and has one exit; a lane
// past its own L computes on values nobody reads, with its reads clamped to its own words and plane rows.
//
// The bases of a turn: ten bits cut from a 64-bit window of the query's words that was loaded one turn ahead --
// unconditionally, so that no loaded value crosses a branch (a copy of one at a join is a full wait).
template <class S> __device__ __forceinline__ unsigned turn_bases(S &s, uint32_t const *words, unsigned i0, unsigned L)
{
    unsigned const ten = (unsigned)(s.win >> ((i0 & 15u) * 2u)) & 1023u; // bases i0 .. i0 + 4
    unsigned const wi = (i0 + 5u) >> 4, wmax = (L >> 4) + 2u;            // a query's words are padded to L / 16 + 3
    unsigned const lo = words[wi < wmax ? wi : wmax], hi = words[wi + 1u < wmax ? wi + 1u : wmax];
    s.win = ((unsigned long long)hi << 32) | lo;
    return ten;
}
__device__ __forceinline__ unsigned long long first_window(uint32_t const *words)
{
    return ((unsigned long long)words[1] << 32) | words[0];
}

// HAND: the tile is not the profile's last one and hands Xd, Xm, E to the next; the last tile leaves E(j) only.
template <int PH, bool FIRST, bool HAND>
__device__ __forceinline__ void qrow(QState &s, QTrans const &t, double xNB, double xNN, double2 const *img,
                                     double2 const *lxe, unsigned base, double *plane, unsigned j, unsigned L)
{
    constexpr int sl[5] = {(PH + 4) % 5, (PH + 3) % 5, (PH + 2) % 5, (PH + 1) % 5, PH}; // slot of row j - l
    constexpr unsigned off[5] = {0u, 4u, 20u, 84u, 340u};
    s.w = ((s.w << 2) | base) & 1023u;

    double m[KT], ins[KT];
#pragma unroll
    for (int r = 0; r < KT; ++r)
        m[r] = ins[r] = ninf();
    double N = ninf();
#pragma unroll
    for (int l = 0; l < 5; ++l)
    {
        unsigned const code = off[l] + (s.w & ((4u << (2 * l)) - 1u));
        double2 const en = lxe[code]; // {eI, eN}
        double2 const e01 = img[2u * code], e23 = img[2u * code + 1u];
        double const e[KT] = {e01.x, e01.y, e23.x, e23.y};
#pragma unroll
        for (int r = 0; r < KT; ++r)
        {
            m[r] = fmax(m[r], s.P[sl[l]][r] + e[r]);
            ins[r] = fmax(ins[r], s.Q[sl[l]][r] + en.x);
        }
        N = fmax(N, s.PN[sl[l]] + en.y);
    }

    // what the tile before this one left for row j; then the slot is refilled with row j + 5
    double xd = ninf(), xm = ninf(), ein = ninf();
    if constexpr (!FIRST)
    {
        xd = s.fxd[PH], xm = s.fxm[PH], ein = s.fe[PH];
        unsigned const jn = j + 5u < L ? j + 5u : L;
        double const *const p = plane + jn * PLANE_ROW;
        s.fxd[PH] = p[0], s.fxm[PH] = p[NT], s.fe[PH] = p[2u * NT];
    }

    // delete chain, sequential in k; D of the profile's first node is -inf
    double d[KT];
    d[0] = xd;
#pragma unroll
    for (int r = 1; r < KT; ++r)
        d[r] = fmax(m[r - 1] + t.md[r], d[r - 1] + t.dd[r]);

    // E(j): exit scores are 0; over M and D of every node
    double E = ein;
#pragma unroll
    for (int r = 0; r < KT; ++r)
        E = fmax(E, fmax(m[r], d[r]));

    double *const o = plane + j * PLANE_ROW;
    if constexpr (HAND)
    {
        o[0] = fmax(m[KT - 1] + t.nmd, d[KT - 1] + t.ndd);
        o[NT] = fmax(fmax(m[KT - 1] + t.nmm, ins[KT - 1] + t.nim), d[KT - 1] + t.ndm);
    }
    o[2u * NT] = E;

    // row j's edges into the next rows, with B0(j) = N(j) + NB
    double const B = N + xNB;
    s.P[PH][0] = fmax(B + t.ent[0], xm);
#pragma unroll
    for (int r = 1; r < KT; ++r)
        s.P[PH][r] = fmax(fmax(B + t.ent[r], m[r - 1] + t.mm[r]), fmax(ins[r - 1] + t.im[r], d[r - 1] + t.dm[r]));
#pragma unroll
    for (int r = 0; r < KT; ++r)
        s.Q[PH][r] = fmax(m[r] + t.mi[r], ins[r] + t.ii[r]);
    s.PN[PH] = N + xNN;
}

// One tile over rows 1 .. L of this lane's query.
template <bool FIRST, bool HAND>
__device__ __forceinline__ void qtile(QTrans const &t, double const *xt, double2 const *img, double2 const *lxe,
                                      uint32_t const *words, double *plane, unsigned L, unsigned Lb)
{
    QState s;
    double const xNB = xt[DCP_X_NB], xNN = xt[DCP_X_NN];
#pragma unroll
    for (int h = 0; h < 5; ++h)
    {
#pragma unroll
        for (int r = 0; r < KT; ++r)
            s.P[h][r] = s.Q[h][r] = ninf();
        s.PN[h] = ninf();
        s.fxd[h] = s.fxm[h] = s.fe[h] = ninf();
    }
    // row 0: S = 0, B = S + SB, N = S + SN; M, I, D, E are -inf (so is the Xm of row 0)
    double const B0 = 0.0 + xt[DCP_X_SB];
#pragma unroll
    for (int r = 0; r < KT; ++r)
        s.P[0][r] = B0 + t.ent[r];
    s.PN[0] = 0.0 + xt[DCP_X_SN];
    s.w = 0u;
    s.win = first_window(words);
    if constexpr (!FIRST)
    {
#pragma unroll
        for (unsigned jj = 1; jj <= 5u; ++jj) // rows 1 .. 5 (clamped to L) into slots 1, 2, 3, 4, 0
        {
            double const *const p = plane + (jj < L ? jj : L) * PLANE_ROW;
            s.fxd[jj % 5u] = p[0], s.fxm[jj % 5u] = p[NT], s.fe[jj % 5u] = p[2u * NT];
        }
    }
    // whole turns of the ring: up to four rows past Lb, which the planes have room for and nobody reads.  The first
    // turn stands in front of the loop so that the loop is entered with the loads and stores of a turn in flight, as
    // it is re-entered: the waits inside it are then counted ones on both edges.
#define DCP_QTURN64(j)                                                                                                 \
    {                                                                                                                  \
        unsigned const ten = turn_bases(s, words, (j)-1u, L);                                                          \
        qrow<1, FIRST, HAND>(s, t, xNB, xNN, img, lxe, ten & 3u, plane, (j), L);                                       \
        qrow<2, FIRST, HAND>(s, t, xNB, xNN, img, lxe, (ten >> 2) & 3u, plane, (j) + 1u, L);                           \
        qrow<3, FIRST, HAND>(s, t, xNB, xNN, img, lxe, (ten >> 4) & 3u, plane, (j) + 2u, L);                           \
        qrow<4, FIRST, HAND>(s, t, xNB, xNN, img, lxe, (ten >> 6) & 3u, plane, (j) + 3u, L);                           \
        qrow<0, FIRST, HAND>(s, t, xNB, xNN, img, lxe, (ten >> 8) & 3u, plane, (j) + 4u, L);                           \
    }
    DCP_QTURN64(1u)
    for (unsigned j = 6u; j <= Lb; j += 5u)
    {
        DCP_ISA_MARK("DCP_QL64_ROWS_BEGIN");
        DCP_QTURN64(j)
    }
    DCP_ISA_MARK("DCP_QL64_ROWS_END");
#undef DCP_QTURN64
}

// The special states over the final E(j) the last tile left in the planes: N, J, C, the null model's R, and the
// feedback check of every row.
template <int PH>
__device__ __forceinline__ void srow(SState &s, QX const &x, double2 const *lxe, unsigned base, double const *plane,
                                     unsigned j, unsigned L)
{
    constexpr int sl[5] = {(PH + 4) % 5, (PH + 3) % 5, (PH + 2) % 5, (PH + 1) % 5, PH};
    constexpr unsigned off[5] = {0u, 4u, 20u, 84u, 340u};
    s.w = ((s.w << 2) | base) & 1023u;
    double N = ninf(), J = ninf(), Cc = ninf(), Rr = ninf();
#pragma unroll
    for (int l = 0; l < 5; ++l)
    {
        double const eN = lxe[off[l] + (s.w & ((4u << (2 * l)) - 1u))].y;
        N = fmax(N, s.PN[sl[l]] + eN);
        J = fmax(J, s.PJ[sl[l]] + eN);
        Cc = fmax(Cc, s.PC[sl[l]] + eN);
        Rr = fmax(Rr, s.PR[sl[l]] + eN);
    }
    double const E = s.fe[PH];
    bool const mine = j <= L;
    if (mine && fmax(E + x.EB, J + x.JB) > N + x.NB) s.fb = true; // B(j) is not the B0(j) the tiles used
    s.PN[PH] = N + x.NN;
    s.PJ[PH] = fmax(E + x.EJ, J + x.JJ);
    s.PC[PH] = fmax(E + x.EC, Cc + x.CC);
    s.PR[PH] = Rr + x.RR;
    if (j == L) s.Cc = Cc, s.Rr = Rr;
    // the slot is refilled behind the last use of E(j), and the load kept where it stands (in the tile loops the
    // stores do that): with both values alive at once the ring's slots are copied at the loop's back edge, and a
    // copy of a loaded value is a full wait per turn
    asm volatile("" ::: "memory");
    s.fe[PH] = plane[(j + 5u < L ? j + 5u : L) * PLANE_ROW + 2u * NT];
    asm volatile("" ::: "memory");
}

__device__ __forceinline__ void qspecials(SState &s, QX const &x, double2 const *lxe, uint32_t const *words,
                                          double const *plane, unsigned L, unsigned Lb)
{
#pragma unroll
    for (int h = 0; h < 5; ++h)
        s.PN[h] = s.PJ[h] = s.PC[h] = s.PR[h] = ninf();
    s.PN[0] = 0.0 + x.SN;
    s.PR[0] = 0.0;
    s.Cc = s.Rr = ninf();
    s.w = 0u;
    s.win = first_window(words);
    s.fb = false;
#pragma unroll
    for (unsigned jj = 1; jj <= 5u; ++jj)
        s.fe[jj % 5u] = plane[(jj < L ? jj : L) * PLANE_ROW + 2u * NT];
#define DCP_STURN64(j)                                                                                                 \
    {                                                                                                                  \
        unsigned const ten = turn_bases(s, words, (j)-1u, L);                                                          \
        srow<1>(s, x, lxe, ten & 3u, plane, (j), L);                                                                   \
        srow<2>(s, x, lxe, (ten >> 2) & 3u, plane, (j) + 1u, L);                                                       \
        srow<3>(s, x, lxe, (ten >> 4) & 3u, plane, (j) + 2u, L);                                                       \
        srow<4>(s, x, lxe, (ten >> 6) & 3u, plane, (j) + 3u, L);                                                       \
        srow<0>(s, x, lxe, (ten >> 8) & 3u, plane, (j) + 4u, L);                                                       \
    }
    DCP_STURN64(1u)
    for (unsigned j = 6u; j <= Lb; j += 5u)
    {
        DCP_ISA_MARK("DCP_QL64_ROWS_BEGIN");
        DCP_STURN64(j)
    }
    DCP_ISA_MARK("DCP_QL64_ROWS_END");
#undef DCP_STURN64
}

__device__ __forceinline__ int group_of(unsigned M) // the launch group of dcp_gpu_db_upload64 (f64_group)
{
    return M <= 64u ? 0 : M <= 128u ? 1 : M <= (unsigned)DCP_F64_SEG ? 2 : 3;
}

// One group of a wavefront slot as its lanes see it.  The record is read through wave-uniform values only (the
// bound of the row loops must be scalar); lane l of the slot has the group's l-th query, a lane past group.nq is idle:
// L = 0, and nothing of it is read.
struct QLaneGroup
{
    unsigned q, L, Lb;
    bool active;
    uint32_t const *words;
    double const *xt;
    double *plane;
};
__device__ __forceinline__ QLaneGroup lane_group(dcp_f64_qlane_args const &a, unsigned gi, double *slot_plane)
{
    dcp_ql_group const g = a.groups[gi];
    unsigned const wl = threadIdx.x & 63u;
    unsigned const gq = (unsigned)__builtin_amdgcn_readfirstlane((int)g.nq);
    unsigned const gfirst = (unsigned)__builtin_amdgcn_readfirstlane((int)g.qfirst);
    unsigned const rowbase = (unsigned)__builtin_amdgcn_readfirstlane((int)g.rowbase);
    QLaneGroup r;
    r.Lb = (unsigned)__builtin_amdgcn_readfirstlane((int)g.lmax);
    r.active = wl < gq;
    r.q = r.active ? a.qorder[gfirst + wl] : 0u;
    r.L = r.active ? a.seq_len[r.q] : 0u;
    r.words = a.seq_words + a.seq_woff[r.q];
    r.xt = a.xtrans + (size_t)r.q * DCP_F64_XSTRIDE;
    // The group's region is dcp_qlane_group_rows(Lb) = (Lb + 11) & ~1 rows from rowbase on.  The sweeps touch its
    // rows 0 .. ceil(Lb / 5) * 5 <= Lb + 4 and prefetch clamped to L <= Lb: inside the region.
    r.plane = slot_plane + (uint64_t)rowbase * PLANE_ROW;
    return r;
}

__global__ __launch_bounds__(NT, 2) void viterbi64_qlane_kernel(dcp_f64_qlane_args a)
{
    __shared__ double2 img[2 * DCP_NCODES]; // [code][KT] match emissions of the tile
    __shared__ double2 lxe[DCP_NCODES];     // [code]{insert, null} emissions of the profile
    __shared__ unsigned s_task;
    unsigned const lane = threadIdx.x;
    double *const plane = a.planes + (uint64_t)blockIdx.x * a.plane_stride + lane;
    for (;;)
    {
        __syncthreads(); // the task before: its LDS images and s_task have been read by everyone
        if (lane == 0u) s_task = atomicAdd(a.task_counter, 1u);
        __syncthreads();
        unsigned const task = (unsigned)__builtin_amdgcn_readfirstlane((int)s_task);
        if (task >= a.ntasks) break;
        unsigned const pi = a.order[task / a.nqb], qb = task % a.nqb; // largest profiles first
        dcp_f64_prof const pr = a.profs[pi];
        double const *const ei = a.xe + pr.xe_off;
        for (unsigned c = lane; c < (unsigned)DCP_NCODES; c += NT)
            lxe[c] = double2{ei[c], ei[DCP_NCODES + c]};
        // this wavefront slot's groups; a slot with none only takes part in the barriers
        unsigned const sidx = qb * (NT / 64u) + (lane >> 6);
        unsigned const g0 = (unsigned)__builtin_amdgcn_readfirstlane((int)a.slot_first[sidx]);
        unsigned const g1 = (unsigned)__builtin_amdgcn_readfirstlane((int)a.slot_first[sidx + 1u]);
        unsigned const ntiles = (pr.core_size + (unsigned)KT - 1u) / (unsigned)KT;
        double const *const tab = a.tab + pr.tab_off;
        double const *const tr = a.trans + pr.trans_off;
        for (unsigned t = 0; t < ntiles; ++t)
        {
            bool const first = t == 0u, last = t + 1u == ntiles;
            if (!first) __syncthreads(); // every lane is through the tile before
            // the tile's image from the resident [1364][ldk] table: 32 contiguous bytes per code
            for (unsigned c = lane; c < (unsigned)DCP_NCODES; c += NT)
            {
                double2 const *const src = (double2 const *)(tab + (uint64_t)c * pr.ldk + (uint64_t)t * KT);
                img[2u * c] = src[0], img[2u * c + 1u] = src[1];
            }
            QTrans tt;
            double const *const tb = tr + (uint64_t)t * KT;
#pragma unroll
            for (int r = 0; r < KT; ++r)
            {
                tt.ent[r] = uni(tb[DCP_T_ENTRY * (uint64_t)pr.ldk + r]);
                tt.mm[r] = uni(tb[DCP_T_MM * (uint64_t)pr.ldk + r]);
                tt.im[r] = uni(tb[DCP_T_IM * (uint64_t)pr.ldk + r]);
                tt.dm[r] = uni(tb[DCP_T_DM * (uint64_t)pr.ldk + r]);
                tt.md[r] = uni(tb[DCP_T_MD * (uint64_t)pr.ldk + r]);
                tt.dd[r] = uni(tb[DCP_T_DD * (uint64_t)pr.ldk + r]);
                tt.mi[r] = uni(tb[DCP_T_MI * (uint64_t)pr.ldk + r]);
                tt.ii[r] = uni(tb[DCP_T_II * (uint64_t)pr.ldk + r]);
            }
            tt.nmm = tt.nim = tt.ndm = tt.nmd = tt.ndd = ninf();
            if (!last) // column KT (t + 1) < core_size <= ldk
            {
                tt.nmm = uni(tb[DCP_T_MM * (uint64_t)pr.ldk + KT]);
                tt.nim = uni(tb[DCP_T_IM * (uint64_t)pr.ldk + KT]);
                tt.ndm = uni(tb[DCP_T_DM * (uint64_t)pr.ldk + KT]);
                tt.nmd = uni(tb[DCP_T_MD * (uint64_t)pr.ldk + KT]);
                tt.ndd = uni(tb[DCP_T_DD * (uint64_t)pr.ldk + KT]);
            }
            __syncthreads();
            // the slot's groups one after the other; the group loop goes around the four sweeps, each of which
            // stands here once
            for (unsigned gi = g0; gi < g1; ++gi)
            {
                QLaneGroup const g = lane_group(a, gi, plane);
                if (first && last) qtile<true, false>(tt, g.xt, img, lxe, g.words, g.plane, g.L, g.Lb);
                else if (first) qtile<true, true>(tt, g.xt, img, lxe, g.words, g.plane, g.L, g.Lb);
                else if (!last) qtile<false, true>(tt, g.xt, img, lxe, g.words, g.plane, g.L, g.Lb);
                else qtile<false, false>(tt, g.xt, img, lxe, g.words, g.plane, g.L, g.Lb);
            }
        }
        // The special states of every group over its own region, and its lanes' results: nothing was parked between
        // the tiles, every per-lane result comes out of this sweep.  (Reads lxe only: no barrier between the last
        // tile and this.)
        for (unsigned gi = g0; gi < g1; ++gi)
        {
            QLaneGroup const g = lane_group(a, gi, plane);
            double const *const xt = g.xt;
            unsigned const q = g.q, L = g.L;
            QX const x{xt[DCP_X_RR], xt[DCP_X_SB], xt[DCP_X_SN], xt[DCP_X_NN], xt[DCP_X_NB], xt[DCP_X_ET],
                       xt[DCP_X_EC], xt[DCP_X_CC], xt[DCP_X_CT], xt[DCP_X_EB], xt[DCP_X_EJ], xt[DCP_X_JJ],
                       xt[DCP_X_JB]};
            SState s;
            qspecials(s, x, lxe, g.words, g.plane, L, g.Lb);
            if (!g.active) continue;
            if (s.fb) // the E -> B / J -> B feedback won in some row: the exact kernel scores this pair
            {
                int const lg = group_of(pr.core_size);
                unsigned const k = atomicAdd(a.redo_n + lg, 1u);
                if (k < a.redo_cap[lg]) a.redo[a.redo_first[lg] + k] = dcp_f64_pair{q, pi};
                else atomicOr(a.redo_n + 4, 1u); // the list is full: dcp_gpu_sync repeats the scan with the row sweep
                continue;
            }
            // E(L) from the plane again: a loaded value that lives out of the row loop costs the loop a full wait
            double const EL = g.plane[L * PLANE_ROW + 2u * NT];
            double const null_ll = s.Rr, alt_ll = fmax(EL + x.ET, s.Cc + x.CT);
            if (a.out_null)
            {
                a.out_null[(size_t)q * a.nprof_total + pr.pidx] = null_ll;
                a.out_alt[(size_t)q * a.nprof_total + pr.pidx] = alt_ll;
            }
            double const lrt = -2 * (null_ll - alt_ll);
            if (finite64(lrt) && lrt >= a.lrt_threshold)
            {
                unsigned const k = atomicAdd(a.nhits, 1u);
                if (k < a.hit_cap) a.hits[k] = dcp_hit64{a.q_base + q, pr.pidx, null_ll, alt_ll};
            }
        }
    }
}

} // namespace

void dcp_f64_launch_qlane(dcp_f64_qlane_args const *a, unsigned nblocks, void *stream)
{
    if (nblocks == 0 || a->ntasks == 0) return;
    hipLaunchKernelGGL(viterbi64_qlane_kernel, dim3(nblocks), dim3(NT), 0, (hipStream_t)stream, *a);
}
