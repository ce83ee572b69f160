// dcp_calib.hip -- calibration on the device: a batch of random sequences written straight into the resident layout
// (dcp_gpu_seqs_random), and one Gumbel fit per profile over the dense scores a scan of that batch left behind
// (dcp_gpu_fit_gumbel).  The rules are dcp_calib.h, which dcp_model.cpp compiles as the host twins.
//
// random_words_kernel: one lane per word of the batch, consecutive lanes on consecutive words (one coalesced store per
// wavefront).  Every sequence has the same length, so a lane finds its sequence and its word by one division -- no
// search in woff as dcp_seqs.hip needs -- and the index is arithmetic too: woff[q] = q (len / 16 + 3).  A word of 16
// bases is four draws; draws are keyed by (seed, q, index), so no lane depends on another.
//
// gumbel_fit_kernel<Real>: one lane per profile.  The score matrices are [seq][profile], so the 64 lanes of a wavefront
// read 64 consecutive values of row q: one coalesced load per matrix and row.  Each of the fit's 15 passes walks the
// rows in order q = 0 .. n - 1 and fetches four rows ahead of their use (dcp_fit_pass), so that the loads of four rows are
// in flight while the sums -- which stay in index order -- take the rows before them.  The trip counts depend on n
// alone: the wavefront's loops are uniform, a lane whose fit ended early (a non-finite score, no variance) just sits
// masked off.
//
// tail_select_kernel<Real> and gumbel_fit_tail_kernel<Real> (dcp_gpu_fit_gumbel_tail): the same lane and row layout.
// The selection finds each lane's k-th largest score by descending the 64 bits of an order-preserving key, one counting
// pass over the rows per bit: comparisons only, so tau and k_eff are the host's bits; no LDS, no atomics, nothing
// crosses lanes.  The fit is the 16 passes of the censored rule over the rows with x >= tau, a lane's own tau.
//
// exp_tail_fit_kernel<Real> (dcp_gpu_fit_exp_tail): the same lane and row layout behind the same selection; the two
// passes of dcp_exp_tail_fit_rule, no exp in them.
#include "dcp_calib.h"

#include <hip/hip_runtime.h>

namespace
{

constexpr unsigned kBlock = 256;
constexpr unsigned kFitBlock = 64; // one wavefront: a DB of a few hundred profiles still spreads over as many CUs

__global__ __launch_bounds__(kBlock) void random_words_kernel(uint32_t *__restrict__ words, uint32_t *__restrict__ woff,
                                                              uint32_t *__restrict__ len_out, unsigned nseqs, uint32_t len,
                                                              uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2)
{
    uint32_t const wps = len / 16u + 3u; // words per sequence
    uint64_t const g = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= (uint64_t)nseqs * wps) return;
    uint32_t const q = (uint32_t)(g / wps), j = (uint32_t)(g - (uint64_t)q * wps);
    uint32_t out = 0u; // pad words stay zero
    if ((uint64_t)j * 16u < len)
    {
        uint64_t const key = dcp_rand_key(seed, q);
        for (unsigned k = 0; k < 4u; ++k) // bases 16 j + 4 k .. + 3 are draw 4 j + k
            out |= dcp_rand_groups(dcp_rand_draw(key, 4ull * j + k), c0, c1, c2) << (8u * k);
        uint32_t const cnt = len - j * 16u < 16u ? len - j * 16u : 16u; // bases of this word
        if (cnt < 16u) out &= (1u << (2u * cnt)) - 1u;                  // every bit behind the last base is zero
    }
    words[g] = out;
    if (j == 0u)
    {
        woff[q] = (uint32_t)g; // q wps: the caller checked that it fits
        len_out[q] = len;
    }
}

template <class Real>
__global__ __launch_bounds__(kFitBlock) void gumbel_fit_kernel(Real const *__restrict__ null_scores,
                                                               Real const *__restrict__ alt_scores, unsigned nseqs,
                                                               unsigned nprof, double *__restrict__ mu,
                                                               double *__restrict__ lambda, uint8_t *__restrict__ status)
{
    unsigned const p = blockIdx.x * kFitBlock + threadIdx.x;
    if (p >= nprof) return;
    Real const *nl = null_scores + p, *al = alt_scores + p;
    auto x = [=](unsigned q) {
        size_t const at = (size_t)q * nprof;
        return (double)al[at] - (double)nl[at];
    };
    double m = 0.0, l = 0.0;
    int const st = dcp_gumbel_fit_rule(x, nseqs, &m, &l);
    mu[p] = m;
    lambda[p] = l;
    status[p] = (uint8_t)st;
}

template <class Real>
__global__ __launch_bounds__(kFitBlock) void tail_select_kernel(Real const *__restrict__ null_scores,
                                                                Real const *__restrict__ alt_scores, unsigned nseqs,
                                                                unsigned nprof, unsigned k, double *__restrict__ tau,
                                                                uint32_t *__restrict__ k_eff)
{
    unsigned const p = blockIdx.x * kFitBlock + threadIdx.x;
    if (p >= nprof) return;
    Real const *nl = null_scores + p, *al = alt_scores + p;
    auto x = [=](unsigned q) {
        size_t const at = (size_t)q * nprof;
        return (double)al[at] - (double)nl[at];
    };
    double t = 0.0;
    unsigned ke = 0u;
    (void)dcp_tail_select_rule(x, nseqs, k, &t, &ke);
    tau[p] = t;
    k_eff[p] = ke;
}

template <class Real>
__global__ __launch_bounds__(kFitBlock) void gumbel_fit_tail_kernel(Real const *__restrict__ null_scores,
                                                                    Real const *__restrict__ alt_scores, unsigned nseqs,
                                                                    unsigned nprof, double const *__restrict__ tau,
                                                                    uint32_t const *__restrict__ k_eff,
                                                                    double *__restrict__ mu, double *__restrict__ lambda,
                                                                    uint8_t *__restrict__ status)
{
    unsigned const p = blockIdx.x * kFitBlock + threadIdx.x;
    if (p >= nprof) return;
    Real const *nl = null_scores + p, *al = alt_scores + p;
    auto x = [=](unsigned q) {
        size_t const at = (size_t)q * nprof;
        return (double)al[at] - (double)nl[at];
    };
    double m = 0.0, l = 0.0;
    int const st = dcp_gumbel_fit_tail_rule(x, nseqs, tau[p], k_eff[p], &m, &l);
    mu[p] = m;
    lambda[p] = l;
    status[p] = (uint8_t)st;
}

template <class Real>
__global__ __launch_bounds__(kFitBlock) void exp_tail_fit_kernel(Real const *__restrict__ null_scores,
                                                                 Real const *__restrict__ alt_scores, unsigned nseqs,
                                                                 unsigned nprof, double const *__restrict__ tau,
                                                                 uint32_t const *__restrict__ k_eff, double *__restrict__ mu,
                                                                 double *__restrict__ lambda, uint8_t *__restrict__ status)
{
    unsigned const p = blockIdx.x * kFitBlock + threadIdx.x;
    if (p >= nprof) return;
    Real const *nl = null_scores + p, *al = alt_scores + p;
    auto x = [=](unsigned q) {
        size_t const at = (size_t)q * nprof;
        return (double)al[at] - (double)nl[at];
    };
    double m = 0.0, l = 0.0;
    int const st = dcp_exp_tail_fit_rule(x, nseqs, tau[p], k_eff[p], &m, &l);
    mu[p] = m;
    lambda[p] = l;
    status[p] = (uint8_t)st;
}

} // namespace

extern "C" int dcp_launch_random(uint32_t *words, uint32_t *woff, uint32_t *len_out, unsigned nseqs, uint32_t len,
                                 uint64_t seed, uint32_t const c[3], void *stream)
{
    if (!words || !woff || !len_out || !c || nseqs == 0 || len == 0) return (int)hipErrorInvalidValue;
    uint64_t const nwords = (uint64_t)nseqs * (len / 16u + 3u);
    if (nwords > 0xffffffffull) return (int)hipErrorInvalidValue;
    unsigned const blocks = (unsigned)((nwords + kBlock - 1u) / kBlock);
    random_words_kernel<<<blocks, kBlock, 0, (hipStream_t)stream>>>(words, woff, len_out, nseqs, len, seed, c[0], c[1], c[2]);
    return (int)hipGetLastError();
}

extern "C" int dcp_launch_gumbel_fit(void const *null_scores, void const *alt_scores, unsigned nseqs, unsigned nprof,
                                     int real_bytes, double *mu, double *lambda, uint8_t *status, void *stream)
{
    if (!null_scores || !alt_scores || !mu || !lambda || !status || nseqs < 2u || nprof == 0) return (int)hipErrorInvalidValue;
    unsigned const blocks = (nprof + kFitBlock - 1u) / kFitBlock;
    hipStream_t const s = (hipStream_t)stream;
    if (real_bytes == 4)
        gumbel_fit_kernel<float><<<blocks, kFitBlock, 0, s>>>((float const *)null_scores, (float const *)alt_scores, nseqs,
                                                              nprof, mu, lambda, status);
    else if (real_bytes == 8)
        gumbel_fit_kernel<double><<<blocks, kFitBlock, 0, s>>>((double const *)null_scores, (double const *)alt_scores,
                                                               nseqs, nprof, mu, lambda, status);
    else return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}

extern "C" int dcp_launch_tail_select(void const *null_scores, void const *alt_scores, unsigned nseqs, unsigned nprof,
                                      int real_bytes, unsigned k, double *tau, uint32_t *k_eff, void *stream)
{
    if (!null_scores || !alt_scores || !tau || !k_eff || nseqs < 2u || nprof == 0 || k < 2u || k > nseqs)
        return (int)hipErrorInvalidValue;
    unsigned const blocks = (nprof + kFitBlock - 1u) / kFitBlock;
    hipStream_t const s = (hipStream_t)stream;
    if (real_bytes == 4)
        tail_select_kernel<float><<<blocks, kFitBlock, 0, s>>>((float const *)null_scores, (float const *)alt_scores, nseqs,
                                                               nprof, k, tau, k_eff);
    else if (real_bytes == 8)
        tail_select_kernel<double><<<blocks, kFitBlock, 0, s>>>((double const *)null_scores, (double const *)alt_scores,
                                                                nseqs, nprof, k, tau, k_eff);
    else return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}

extern "C" int dcp_launch_gumbel_fit_tail(void const *null_scores, void const *alt_scores, unsigned nseqs, unsigned nprof,
                                          int real_bytes, double const *tau, uint32_t const *k_eff, double *mu,
                                          double *lambda, uint8_t *status, void *stream)
{
    if (!null_scores || !alt_scores || !tau || !k_eff || !mu || !lambda || !status || nseqs < 2u || nprof == 0)
        return (int)hipErrorInvalidValue;
    unsigned const blocks = (nprof + kFitBlock - 1u) / kFitBlock;
    hipStream_t const s = (hipStream_t)stream;
    if (real_bytes == 4)
        gumbel_fit_tail_kernel<float><<<blocks, kFitBlock, 0, s>>>((float const *)null_scores, (float const *)alt_scores,
                                                                   nseqs, nprof, tau, k_eff, mu, lambda, status);
    else if (real_bytes == 8)
        gumbel_fit_tail_kernel<double><<<blocks, kFitBlock, 0, s>>>((double const *)null_scores, (double const *)alt_scores,
                                                                    nseqs, nprof, tau, k_eff, mu, lambda, status);
    else return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}

extern "C" int dcp_launch_exp_tail_fit(void const *null_scores, void const *alt_scores, unsigned nseqs, unsigned nprof,
                                       int real_bytes, double const *tau, uint32_t const *k_eff, double *mu, double *lambda,
                                       uint8_t *status, void *stream)
{
    if (!null_scores || !alt_scores || !tau || !k_eff || !mu || !lambda || !status || nseqs < 2u || nprof == 0)
        return (int)hipErrorInvalidValue;
    unsigned const blocks = (nprof + kFitBlock - 1u) / kFitBlock;
    hipStream_t const s = (hipStream_t)stream;
    if (real_bytes == 4)
        exp_tail_fit_kernel<float><<<blocks, kFitBlock, 0, s>>>((float const *)null_scores, (float const *)alt_scores, nseqs,
                                                                nprof, tau, k_eff, mu, lambda, status);
    else if (real_bytes == 8)
        exp_tail_fit_kernel<double><<<blocks, kFitBlock, 0, s>>>((double const *)null_scores, (double const *)alt_scores,
                                                                 nseqs, nprof, tau, k_eff, mu, lambda, status);
    else return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}
