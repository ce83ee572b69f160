// dcp_forward_dev.h -- device helpers the Forward kernels (dcp_forward.hip), the Backward kernels (dcp_posterior.hip) and
// the max-plus sweep (dcp_mea.hip) share: lane moves of doubles, the wave-wide maximum and sum, the head of the loop
// over a launch's pairs (the pair, its profile, length, special transitions and tables), where a pair's row records and
// matrices lie, the wide sweeps' work area, the word codes, the Forward delete chain and E(j), the special states'
// per-lane layout.  Local to each unit.
#ifndef DCP_FORWARD_DEV_H
#define DCP_FORWARD_DEV_H

#include "dcp_forward.h"
#include "dcp_host.h"
#include "dcp_posterior.h"

#include <hip/hip_runtime.h>

namespace
{

__device__ __forceinline__ double ninf() { return -__builtin_inf(); }

// gfx950's DPP moves 32-bit lanes: a double crosses lanes as its two halves (dcp_f64.hip)
__device__ __forceinline__ double shr1(double v, double first) // value of lane - 1; lane 0 receives `first`
{
    unsigned long long const vb = __builtin_bit_cast(unsigned long long, v);
    unsigned long long const fb = __builtin_bit_cast(unsigned long long, first);
    int const lo = __builtin_amdgcn_update_dpp((int)(unsigned)fb, (int)(unsigned)vb, 0x138 /*wave_shr:1*/, 0xf, 0xf, false);
    int const hi = __builtin_amdgcn_update_dpp((int)(unsigned)(fb >> 32), (int)(unsigned)(vb >> 32), 0x138, 0xf, 0xf, false);
    return __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

__device__ __forceinline__ double shl1(double v, double last, unsigned lane) // value of lane + 1; lane 63 receives `last`
{
    double const n = __shfl_down(v, 1, 64);
    return lane == 63u ? last : n;
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
        v = dcp_fwd_max(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ double wave_sum(double v) // lane i and lane i ^ o add the same two values: one tree for all
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
        v = v + __shfl_xor(v, o, 64);
    return v;
}

struct XF // the pair's special transitions as the rows use them
{
    double NB, EB, JB, ET, CT;
    double xa, xb; // this lane's own special state X of N, J, C, R: PX(j) = lse(E(j) + xa, X(j) + xb)
};

template <class Real> struct Tabs
{
    Real const *tab, *trans, *ei, *en;
    uint64_t ld;
    unsigned M;
    uint32_t const *words;
};

template <class Real> __device__ __forceinline__ double load_col(Real const *row, unsigned k, unsigned M)
{
    return k < M ? (double)row[k] : ninf();
}

// the last five bases' word codes, the shortest word first
__device__ __forceinline__ void word_codes(unsigned w, unsigned (&code)[5])
{
    constexpr unsigned off[5] = {0u, 4u, 20u, 84u, 340u};
#pragma unroll
    for (int l = 0; l < 5; ++l)
        code[l] = off[l] + (w & ((4u << (2 * l)) - 1u));
}

// D of the lane's R nodes: a[r] = M_{k-1} + MD_k, dd[r] = DD_k, carry = D of the node before lane 0's first
template <int R>
__device__ __forceinline__ void delete_chain(double const (&a)[R], double const (&dd)[R], double carry, double (&d)[R],
                                             unsigned lane)
{
    double c = a[0], s = dd[0]; // the lane's chain from d_in = -inf, and the sum of its DD
#pragma unroll
    for (int r = 1; r < R; ++r)
    {
        c = dcp_lse2(a[r], c + dd[r]);
        s = s + dd[r];
    }
#pragma unroll
    for (unsigned o = 1; o < 64u; o <<= 1)
    {
        double const sp = __shfl_up(s, o, 64), cp = __shfl_up(c, o, 64);
        if (lane >= o)
        {
            c = dcp_lse2(c, cp + s);
            s = sp + s;
        }
    }
    // lanes 0 .. l - 1 composed, applied to the carry: lane 0 receives (0, -inf), the identity
    double const cb = shr1(c, ninf()), sb = shr1(s, 0.0);
    double const d_in = dcp_lse2(cb, carry + sb);
    d[0] = dcp_lse2(a[0], d_in + dd[0]);
#pragma unroll
    for (int r = 1; r < R; ++r)
        d[r] = dcp_lse2(a[r], d[r - 1] + dd[r]);
}

// the lanes' M and D of one chunk as one term of E(j) in the running form
template <int R> __device__ __forceinline__ dcp_lse_acc exit_terms(double const (&m)[R], double const (&d)[R])
{
    double mx = dcp_fwd_max(m[0], d[0]);
#pragma unroll
    for (int r = 1; r < R; ++r)
        mx = dcp_fwd_max(mx, dcp_fwd_max(m[r], d[r]));
    mx = readlane(wave_max(mx), 0);
    double const mm = dcp_fwd_shift(mx);
    double sum = exp(m[0] - mm) + exp(d[0] - mm);
#pragma unroll
    for (int r = 1; r < R; ++r)
        sum = sum + exp(m[r] - mm) + exp(d[r] - mm);
    return dcp_lse_acc{mx, readlane(wave_sum(sum), 0)};
}

__device__ __forceinline__ XF special_transitions(double const *xt, unsigned lane)
{
    XF x;
    x.NB = xt[DCP_X_NB], x.EB = xt[DCP_X_EB], x.JB = xt[DCP_X_JB], x.ET = xt[DCP_X_ET], x.CT = xt[DCP_X_CT];
    unsigned const sp = lane & 3u;
    x.xa = sp == 1u ? xt[DCP_X_EJ] : sp == 2u ? xt[DCP_X_EC] : ninf(); // N and R have no edge from E
    x.xb = sp == 0u ? xt[DCP_X_NN] : sp == 1u ? xt[DCP_X_JJ] : sp == 2u ? xt[DCP_X_CC] : xt[DCP_X_RR];
    return x;
}

// row 0 of the lane's special state: N = S + SN, R starts at 0, J and C are -inf
__device__ __forceinline__ double special_row0(double const *xt, unsigned lane)
{
    unsigned const sp = lane & 3u;
    return sp == 0u ? 0.0 + xt[DCP_X_SN] : sp == 3u ? 0.0 : ninf();
}

template <class Real> __device__ __forceinline__ Tabs<Real> tables_of(dcp_fwd_args const &a, dcp_fwd_prof const &pr, unsigned q)
{
    Tabs<Real> g;
    g.tab = (Real const *)a.tab + pr.tab_off;
    g.trans = (Real const *)a.trans + pr.trans_off;
    g.ei = (Real const *)a.ei + pr.ei_off;
    g.en = (Real const *)a.en + pr.en_off;
    g.ld = pr.ld;
    g.M = pr.core_size;
    g.words = a.seq_words + a.seq_woff[q];
    return g;
}

// the head of the loop over a launch's pairs.  (The pair's tables, tables_of, follow the sweep's own special transitions
// at each use: formed in here, their loads move ahead of those and the kernels' schedules change.)
struct PairHead
{
    dcp_fwd_pair pp;
    dcp_fwd_prof pr;
    unsigned L;
    double const *xt; // the sequence's special transitions
};
__device__ __forceinline__ PairHead pair_head(dcp_fwd_args const &a, uint64_t pair)
{
    dcp_fwd_pair const pp = a.pairs[pair];
    dcp_fwd_prof const pr = a.profs[pp.prof];
    return PairHead{pp, pr, a.seq_len[pp.q], a.xtrans + (size_t)pp.q * DCP_FWD_XSTRIDE};
}

// the pair's row records (dcp_posterior.h), row 0 first
__device__ __forceinline__ double *record_of(dcp_fwd_args const &a, dcp_fwd_pair const &pp)
{
    return a.rows + (a.row_off[pp.pos] - a.row_base) * DCP_POST_REC;
}

// the pair's two matrices (dcp_mea.h), rows j = 0 .. L of core_size columns: a lane stores its own columns below core_size
struct Mats
{
    double *m0, *m1;
};
__device__ __forceinline__ Mats mats_of(dcp_fwd_args const &a, dcp_fwd_pair const &pp)
{
    uint64_t const at = a.cell_off[pp.pos] - a.cell_base;
    return Mats{a.mat0 + at, a.mat1 + at};
}

// ---- the wide sweeps: chunks of DCP_FWD_CHUNK columns through the wavefront's work area ------------------------------
constexpr int WR = 4; // nodes per lane of a chunk

// wavefront gw's work area for a profile of M nodes: rows of ldk doubles, two rings of five slots, then the row's own
// values.  ldk x the sweep's rows <= work_stride: the host sized the stride by the widest listed profile.
struct WideArea
{
    double *base;
    uint64_t ldk;
    unsigned nchunks;
    __device__ __forceinline__ double *ring0(unsigned slot) const { return base + (uint64_t)slot * ldk; }
    __device__ __forceinline__ double *ring1(unsigned slot) const { return base + (uint64_t)(5u + slot) * ldk; }
    __device__ __forceinline__ double *row(unsigned which) const { return base + (uint64_t)(10u + which) * ldk; }
};
__device__ __forceinline__ WideArea wide_area(double *work, uint64_t work_stride, uint64_t gw, unsigned M)
{
    WideArea wa;
    wa.nchunks = (M + (unsigned)DCP_FWD_CHUNK - 1u) / (unsigned)DCP_FWD_CHUNK;
    wa.ldk = (uint64_t)wa.nchunks * DCP_FWD_CHUNK;
    wa.base = work + gw * work_stride;
    return wa;
}

} // namespace

#endif
