// dcp_mea.hip -- gfx950 kernels of the posterior-decoded alignment of a pair list (dcp_gpu_mea_pairs; the two sweeps
// that come first are the matrix-storing variants of dcp_forward.hip and dcp_posterior.hip).
//
//  mea_sweep_kernel<Real>  the max-plus sweep of dcp_mea.h over one (sequence, profile) pair per wavefront, rows
//                          j = L .. 0, chunks of 256 columns (four per lane) for every width.  The rings of gM and gI
//                          (rows j + 1 .. j + 5) and the row's gP, gQ live in the wavefront's work area (12 x ldk doubles; a
//                          lane reads back only what it wrote itself).  Pass one runs over the chunks in rising order: the
//                          five words' posteriors of every cell from P, Q, bM, bI and the emission tables, gP and gQ and their
//                          word choices, and gB as the wave's maximum with the lowest node that reaches it.  The specials
//                          follow (one per lane for the words of N, J, C: lane l & 3 keeps the ring of its own one; their
//                          few maxima in every lane alike).  Pass two runs over the chunks in falling order, carrying gD and
//                          gP of the next chunk's first node in registers, and writes gM, gI into the row's slot and the
//                          cell's 13 bits of choices.
//  mea_walk_kernel<Real>   one thread per pair: dcp_mea_walk (dcp_mea.h, the host twin's too) from S along the parked
//                          choices, steps and word posteriors into the round's step buffer, counting past its capacity.
//
// The delete chain under max with links of 0 / -inf is the Backward chain's linear recurrence with lse replaced by max:
// gD_k = max(h_k, s_{k+1} + gD_{k+1}), h_k = max(gE, [DM_{k+1}] gP_{k+1}), s = 0 or -inf -- a segmented maximum.  The lanes'
// (s, c) pairs compose by (s1, c1) (+) (s2, c2) = (s1 + s2, max(c1, c2 + s1)) in six __shfl_down steps; max is exact, so
// the scan's value is the serial chain's in bits, and the lane's chain is run again from its true input for the choices.
// No +inf and no NaN arises: gains are finite and >= 0 or -inf, links are 0 or -inf.
//
// A column at or past core_size is never loaded: its emissions are -inf, so its gP and gQ are -inf and it adds nothing to
// gB; the links into it are -inf, so what its ring holds -- gE at most -- reaches no real column.  Nothing of it is stored
// in the choices, whose rows are core_size wide.
#include "dcp_mea.h"

#include "dcp_forward_dev.h"

namespace
{

struct DevSeq // base i of a resident sequence: 2 bits each, 16 a word
{
    uint32_t const *w;
    __device__ __forceinline__ unsigned operator()(unsigned i) const { return (w[i >> 4] >> ((i & 15u) * 2u)) & 3u; }
};

// (WideArea: ring0 holds the slots of gM, ring1 those of gI; rows 0, 1 the row's gP, gQ)
// gD of the lane's WR nodes, downwards: h[r] the node's own part, s[r] = 0 or -inf the link DD_{k+1}, carry = gD of the
// node after lane 63's last.  dn[r] receives gD_{k+1}.
__device__ __forceinline__ void chain_down(double const (&h)[WR], double const (&s)[WR], double carry, double (&dn)[WR], unsigned lane)
{
    double cc = h[WR - 1], ss = s[WR - 1]; // the lane's chain from d_in = -inf, and the sum of its links
#pragma unroll
    for (int r = WR - 2; r >= 0; --r)
    {
        cc = dcp_fwd_max(h[r], s[r] + cc);
        ss = ss + s[r];
    }
#pragma unroll
    for (unsigned o = 1; o < 64u; o <<= 1)
    {
        double const sp = __shfl_down(ss, o, 64), cp = __shfl_down(cc, o, 64);
        if (lane + o < 64u)
        {
            cc = dcp_fwd_max(cc, cp + ss);
            ss = ss + sp;
        }
    }
    // lanes l + 1 .. 63 composed, applied to the carry: lane 63 receives (0, -inf), the identity
    double const cb = shl1(cc, ninf(), lane), sb = shl1(ss, 0.0, lane);
    dn[WR - 1] = dcp_fwd_max(cb, carry + sb);
#pragma unroll
    for (int r = WR - 2; r >= 0; --r)
        dn[r] = dcp_fwd_max(h[r + 1], s[r + 1] + dn[r + 1]);
}

__device__ __forceinline__ unsigned wave_min(unsigned v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
    {
        unsigned const t = (unsigned)__shfl_xor((int)v, o, 64);
        v = t < v ? t : v;
    }
    return v;
}

template <class Real> __global__ __launch_bounds__(256) void mea_sweep_kernel(dcp_mea_args a)
{
    unsigned const lane = threadIdx.x & 63u;
    uint64_t const gw = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    uint64_t const nw = a.nwaves;
    if (gw >= nw) return; // wavefronts past nwaves have no work area
    for (uint64_t pair = gw; pair < a.nlist; pair += nw)
    {
        dcp_fwd_pair const pp = a.list[pair];
        dcp_fwd_prof const pr = a.profs[pp.prof];
        unsigned const L = a.seq_len[pp.q], M = pr.core_size;
        double const *xt = a.xtrans + (size_t)pp.q * DCP_FWD_XSTRIDE;
        Real const *tab = (Real const *)a.tab + pr.tab_off, *trans = (Real const *)a.trans + pr.trans_off;
        Real const *ei = (Real const *)a.ei + pr.ei_off, *en = (Real const *)a.en + pr.en_off;
        uint64_t const ld = pr.ld;
        uint32_t const *words = a.seq_words + a.seq_woff[pp.q];
        uint64_t const row0 = a.row_off[pair] - a.row_off[0], cell0 = a.cell_off[pair] - a.cell_off[0];
        double const *P = a.P + cell0, *Q = a.Q + cell0, *bM = a.bM + cell0, *bI = a.bI + cell0;
        double const *fr = a.rows_f + row0 * DCP_POST_REC, *br = a.rows_b + row0 * DCP_POST_REC;
        uint16_t *const cell = a.cell + cell0;
        uint32_t *const rowc = a.rowc + row0 * DCP_MEA_ROWC;
        double const alt = a.alt_fwd[pp.pos];
        WideArea const wa = wide_area(a.work, a.work_stride, gw, M);
        unsigned const nchunks = wa.nchunks;
        // rows L + 1 .. L + 5, anew for every pair: the rings' own columns
        for (unsigned ch = 0; ch < nchunks; ++ch)
        {
            unsigned const k0 = ch * (unsigned)DCP_FWD_CHUNK + lane * WR;
#pragma unroll
            for (int r = 0; r < WR; ++r)
#pragma unroll
                for (unsigned h = 0; h < 5u; ++h)
                    wa.ring0(h)[k0 + r] = wa.ring1(h)[k0 + r] = ninf();
        }
        unsigned const X = (lane & 3u) < 2u ? (lane & 3u) : 2u; // the lane's own one of N, J, C
        double gx[5]; // its suffix gains at rows j + 1 .. j + 5
#pragma unroll
        for (int l = 0; l < 5; ++l)
            gx[l] = ninf();
        unsigned w = 0u; // x[j .. j + 5), first base most significant; past L the bases are 0
        for (unsigned j = L;; --j)
        {
            bool const last = j == L;
            unsigned const nl = L - j < 5u ? L - j : 5u; // words that end at or before L
            unsigned const base = j < L ? (words[j >> 4] >> ((j & 15u) * 2u)) & 3u : 0u;
            w = (w >> 2) | (base << 8);
            constexpr unsigned off[5] = {0u, 4u, 20u, 84u, 340u};
            unsigned code[5];
            double eI[5];
#pragma unroll
            for (int l = 0; l < 5; ++l)
            {
                code[l] = off[l] + (w >> (8 - 2 * l));
                eI[l] = (double)ei[code[l]];
            }
            dcp_mea_best px = dcp_mea_none();
            {
                double const f = fr[(uint64_t)DCP_POST_REC * j + X];
#pragma unroll
                for (unsigned l = 1; l <= 5u; ++l)
                    if (l <= nl)
                        dcp_mea_take(px, dcp_mea_word(f, (double)en[code[l - 1u]], br[(uint64_t)DCP_POST_REC * (j + l) + X], alt, l, gx[l - 1u]), l);
            }

            // pass one: gP, gQ of the row and their words, chunk after chunk, and gB over all of them
            dcp_mea_best bb = dcp_mea_none();
            for (unsigned ch = 0; ch < nchunks; ++ch)
            {
                unsigned const k0 = ch * (unsigned)DCP_FWD_CHUNK + lane * WR;
                double *const wp = wa.row(0) + k0, *const wq = wa.row(1) + k0;
#pragma unroll
                for (int r = 0; r < WR; ++r)
                {
                    unsigned const k = k0 + r;
                    dcp_mea_best p = dcp_mea_none(), q = dcp_mea_none();
                    if (k < M)
                    {
                        double const fp = P[(uint64_t)j * M + k], fq = Q[(uint64_t)j * M + k];
#pragma unroll
                        for (unsigned l = 1; l <= 5u; ++l)
                            if (l <= nl)
                            {
                                uint64_t const to = (uint64_t)(j + l) * M + k;
                                unsigned const slot = (j + l) % 5u;
                                dcp_mea_take(p, dcp_mea_word(fp, (double)tab[(uint64_t)code[l - 1u] * ld + k], bM[to], alt, l, wa.ring0(slot)[k]), l);
                                dcp_mea_take(q, dcp_mea_word(fq, eI[l - 1u], bI[to], alt, l, wa.ring1(slot)[k]), l);
                            }
                        cell[(uint64_t)j * M + k] = (uint16_t)((p.c << DCP_MEA_SH_P) | (q.c << DCP_MEA_SH_Q));
                        dcp_mea_take(bb, dcp_mea_link((double)trans[(uint64_t)DCP_T_ENTRY * ld + k], p.g), k + 1u);
                    }
                    wp[r] = p.g, wq[r] = q.g;
                }
            }
            // the wave's maximum and the lowest node that reaches it
            double const gB = readlane(wave_max(bb.g), 0);
            unsigned const cB = gB == ninf() ? 0u : wave_min(bb.g == gB ? bb.c : 0xffffffffu);

            // the specials, in every lane alike
            double const gPN = readlane(px.g, 0), gPJ = readlane(px.g, 1), gPC = readlane(px.g, 2);
            unsigned const cPN = (unsigned)__builtin_amdgcn_readlane((int)px.c, 0), cPJ = (unsigned)__builtin_amdgcn_readlane((int)px.c, 1),
                           cPC = (unsigned)__builtin_amdgcn_readlane((int)px.c, 2);
            dcp_mea_best const sc = dcp_mea_c(last, xt[DCP_X_CT], xt[DCP_X_CC], gPC);
            dcp_mea_best const sj = dcp_mea_nj(xt[DCP_X_JB], xt[DCP_X_JJ], gB, gPJ);
            dcp_mea_best const sn = dcp_mea_nj(xt[DCP_X_NB], xt[DCP_X_NN], gB, gPN);
            dcp_mea_best const se = dcp_mea_e(last, xt[DCP_X_ET], xt[DCP_X_EB], xt[DCP_X_EJ], xt[DCP_X_EC], gB, gPJ, gPC);
            gx[4] = gx[3], gx[3] = gx[2], gx[2] = gx[1], gx[1] = gx[0];
            gx[0] = X == 0u ? sn.g : X == 1u ? sj.g : sc.g;
            if (lane == 0u)
            {
                rowc[(uint64_t)DCP_MEA_ROWC * j] = (cPN << DCP_MEA_SH_PN) | (cPJ << DCP_MEA_SH_PJ) | (cPC << DCP_MEA_SH_PC) |
                                                   (sn.c << DCP_MEA_SH_N) | (sj.c << DCP_MEA_SH_J) | (sc.c << DCP_MEA_SH_C) |
                                                   (se.c << DCP_MEA_SH_E);
                rowc[(uint64_t)DCP_MEA_ROWC * j + 1u] = cB;
            }
            double const gE = se.g;

            // pass two: D, M, I downwards, into slot j mod 5; gD and gP of the next chunk's first node come along
            double carry_d = ninf(), carry_p = ninf();
            unsigned const slot = j % 5u;
            for (unsigned ch = nchunks; ch-- > 0u;)
            {
                unsigned const k0 = ch * (unsigned)DCP_FWD_CHUNK + lane * WR;
                double const *wp = wa.row(0) + k0, *wq = wa.row(1) + k0;
                double gP[WR], gQ[WR], gPn[WR], DMn[WR], DDn[WR], h[WR], s[WR], dn[WR];
#pragma unroll
                for (int r = 0; r < WR; ++r)
                    gP[r] = wp[r], gQ[r] = wq[r];
                gPn[WR - 1] = shl1(gP[0], carry_p, lane);
#pragma unroll
                for (int r = 0; r < WR - 1; ++r)
                    gPn[r] = gP[r + 1];
#pragma unroll
                for (int r = 0; r < WR; ++r)
                {
                    DMn[r] = load_col(trans + DCP_T_DM * ld, k0 + r + 1u, M);
                    DDn[r] = load_col(trans + DCP_T_DD * ld, k0 + r + 1u, M);
                    h[r] = dcp_fwd_max(gE, dcp_mea_link(DMn[r], gPn[r]));
                    s[r] = dcp_mea_link(DDn[r], 0.0);
                }
                chain_down(h, s, carry_d, dn, lane);
                double *const gm = wa.ring0(slot) + k0, *const gi = wa.ring1(slot) + k0;
                double d0 = ninf();
#pragma unroll
                for (int r = 0; r < WR; ++r)
                {
                    unsigned const k = k0 + r;
                    dcp_mea_best const bd = dcp_mea_d(gE, DDn[r], DMn[r], dn[r], gPn[r]);
                    dcp_mea_best const bm = dcp_mea_m(gE, load_col(trans + DCP_T_MD * ld, k + 1u, M), load_col(trans + DCP_T_MM * ld, k + 1u, M),
                                                      load_col(trans + DCP_T_MI * ld, k, M), dn[r], gPn[r], gQ[r]);
                    dcp_mea_best const bi = dcp_mea_i(load_col(trans + DCP_T_IM * ld, k + 1u, M), load_col(trans + DCP_T_II * ld, k, M), gPn[r], gQ[r]);
                    gm[r] = bm.g, gi[r] = bi.g;
                    if (r == 0) d0 = bd.g;
                    if (k < M)
                    {
                        uint16_t *const c = cell + (uint64_t)j * M + k;
                        *c = (uint16_t)(*c | (bm.c << DCP_MEA_SH_M) | (bi.c << DCP_MEA_SH_I) | (bd.c << DCP_MEA_SH_D));
                    }
                }
                carry_p = readlane(gP[0], 0), carry_d = readlane(d0, 0);
            }
            if (j == 0u)
            {
                dcp_mea_best const ss = dcp_mea_nj(xt[DCP_X_SB], xt[DCP_X_SN], gB, gPN);
                if (lane == 0u)
                {
                    a.gain[pp.pos] = ss.g;
                    a.start[pair] = ss.c;
                }
                break;
            }
        }
    }
}

template <class Real> __global__ __launch_bounds__(64) void mea_walk_kernel(dcp_mea_args a)
{
    uint64_t const pair = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (pair >= a.nlist) return;
    dcp_fwd_pair const pp = a.list[pair];
    dcp_fwd_prof const pr = a.profs[pp.prof];
    uint64_t const row0 = a.row_off[pair] - a.row_off[0], cell0 = a.cell_off[pair] - a.cell_off[0];
    dcp_mea_view<Real> v;
    v.M = pr.core_size, v.L = a.seq_len[pp.q], v.ldm = pr.core_size;
    v.P = a.P + cell0, v.Q = a.Q + cell0, v.bM = a.bM + cell0, v.bI = a.bI + cell0;
    v.cell = a.cell + cell0, v.rowc = a.rowc + row0 * DCP_MEA_ROWC;
    v.fr = a.rows_f + row0 * DCP_POST_REC, v.br = a.rows_b + row0 * DCP_POST_REC;
    v.em = (Real const *)a.tab + pr.tab_off, v.ei = (Real const *)a.ei + pr.ei_off, v.en = (Real const *)a.en + pr.en_off;
    v.ld = pr.ld;
    DevSeq const x{a.seq_words + a.seq_woff[pp.q]};
    uint64_t const at = a.step_at[pair];
    a.nsteps[pair] = dcp_mea_walk(v, x, a.alt_fwd[pp.pos], a.start[pair], a.steps + at, a.post + at, a.step_cap[pair]);
}

} // namespace

extern "C" int dcp_mea_sweep_launch(int precision, struct dcp_mea_args const *a, void *stream)
{
    if (!a || a->nlist == 0 || a->nwaves == 0 || !a->work || !a->cell || !a->rowc || !a->gain || !a->start) return 1;
    dim3 const grid((a->nwaves + 3u) / 4u), block(256);
    hipStream_t const st = (hipStream_t)stream;
    if (precision == 32) hipLaunchKernelGGL((mea_sweep_kernel<float>), grid, block, 0, st, *a);
    else if (precision == 64) hipLaunchKernelGGL((mea_sweep_kernel<double>), grid, block, 0, st, *a);
    else return 1;
    return 0;
}

extern "C" int dcp_mea_walk_launch(int precision, struct dcp_mea_args const *a, void *stream)
{
    if (!a || a->nlist == 0 || !a->steps || !a->post || !a->step_at || !a->step_cap || !a->nsteps) return 1;
    dim3 const grid((a->nlist + 63u) / 64u), block(64);
    hipStream_t const st = (hipStream_t)stream;
    if (precision == 32) hipLaunchKernelGGL((mea_walk_kernel<float>), grid, block, 0, st, *a);
    else if (precision == 64) hipLaunchKernelGGL((mea_walk_kernel<double>), grid, block, 0, st, *a);
    else return 1;
    return 0;
}
