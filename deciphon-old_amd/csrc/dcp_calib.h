// dcp_calib.h -- calibration: the random batch and the per-profile Gumbel fit (dcp_calib.hip), and the two rules that
// the kernels there and their host twins in dcp_model.cpp both evaluate.  One source for both sides, as
// dcp_frame_word.h: the generator is integer arithmetic mod 2^64, equal in bits wherever it runs; the fit is double
// arithmetic with every sum taken in index order and a fixed number of steps, so that with no contraction
// (-ffp-contract=off in both units) host and device differ only in exp, log and sqrt.
#ifndef DCP_CALIB_H
#define DCP_CALIB_H

#include <math.h>
#include <stdint.h>

#ifdef __HIP__
#define DCP_HD __host__ __device__
#else
#define DCP_HD
#endif

// ---- the generator ------------------------------------------------------------------------------------------------
// splitmix64's output function; key(q) = sm(seed ^ sm(q)), draw(q, i) = sm(key(q) + i): counter-based, any base of any
// sequence is computed on its own.  One draw gives four bases, 16 bits each: base b of sequence q is
//   u = (draw(q, b >> 2) >> (16 (b & 3))) & 0xffff,  id = (u >= c[0]) + (u >= c[1]) + (u >= c[2])   (A C G T = 0 1 2 3)
// with thresholds c in 0 .. 65 536 (dcp_seq_random_thresholds).
DCP_HD inline uint64_t dcp_rand_sm(uint64_t x)
{
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
DCP_HD inline uint64_t dcp_rand_key(uint64_t seed, uint32_t q) { return dcp_rand_sm(seed ^ dcp_rand_sm((uint64_t)q)); }
DCP_HD inline uint64_t dcp_rand_draw(uint64_t key, uint64_t i) { return dcp_rand_sm(key + i); }
// the four bases of one draw as four 2-bit groups, the first base lowest
DCP_HD inline uint32_t dcp_rand_groups(uint64_t d, uint32_t c0, uint32_t c1, uint32_t c2)
{
    uint32_t out = 0;
    for (unsigned t = 0; t < 4u; ++t)
    {
        uint32_t const u = (uint32_t)(d >> (16u * t)) & 0xffffu;
        out |= ((uint32_t)(u >= c0) + (uint32_t)(u >= c1) + (uint32_t)(u >= c2)) << (2u * t);
    }
    return out;
}

// ---- the fit ------------------------------------------------------------------------------------------------------
// Status of one fit (include/dcp_gpu.h: enum dcp_fit_status has the same values).
enum
{
    DCP_FITR_OK = 0,
    DCP_FITR_FLAT = 16,
    DCP_FITR_NONFINITE = 17,
    DCP_FITR_DIVERGED = 18,
    DCP_FIT_STEPS = 12,
};

// by the encoding: right whatever the unit's NaN flags are
DCP_HD inline bool dcp_fit_finite(double v)
{
    uint64_t b;
    __builtin_memcpy(&b, &v, sizeof b);
    return ((b >> 52) & 0x7ffu) != 0x7ffu;
}
DCP_HD inline double dcp_fit_nan()
{
    uint64_t const b = 0x7ff8000000000000ull;
    double v;
    __builtin_memcpy(&v, &b, sizeof v);
    return v;
}

// One pass: f(x(0)), f(x(1)), .. f(x(n - 1)) in this order, the values fetched four at a time ahead of their use -- on the
// device four rows' loads are in flight while f, whose sums stay in index order, takes the four before them.
template <class X, class F> DCP_HD inline void dcp_fit_pass(X const &x, unsigned n, F const &f)
{
    unsigned i = 0;
    for (; i + 4u <= n; i += 4u)
    {
        double const v0 = x(i), v1 = x(i + 1u), v2 = x(i + 2u), v3 = x(i + 3u);
        f(v0), f(v1), f(v2), f(v3);
    }
    for (; i < n; ++i)
        f(x(i));
}

// Maximum-likelihood Gumbel fit of x(0) .. x(n - 1), n >= 2 (the caller checks): 15 passes over the sample, each in
// index order.  Pass 1: non-finite -> NONFINITE; the minimum m and the mean.  Pass 2: the variance; 0 -> FLAT, else
// the moment estimate lambda = pi / sqrt(6 var).  Then exactly DCP_FIT_STEPS Newton steps on
//   f(lambda) = 1 / lambda - (mean - m) + s1 / s0,  s_k = sum y^k exp(-lambda y),  y = x - m >= 0
// (every term of every sum is non-negative).  A step to a lambda that is not finite or not positive sets a sticky
// DIVERGED and keeps the lambda it came from, so every caller runs the same number of passes; so does a last step that
// moved lambda by more than 2^-40 of itself.  Last pass: mu = m - log(s0 / n) / lambda.  Any status but OK gives
// NaN in both outputs.  exp, log and sqrt are the side's own.
template <class X> DCP_HD inline int dcp_gumbel_fit_rule(X const &x, unsigned n, double *mu, double *lambda)
{
    *mu = *lambda = dcp_fit_nan();
    bool bad = false;
    double m = 1.7976931348623157e308, sum = 0.0;
    dcp_fit_pass(x, n, [&](double v) {
        bad |= !dcp_fit_finite(v);
        m = v < m ? v : m;
        sum += v;
    });
    if (bad) return DCP_FITR_NONFINITE;
    double const mean = sum / (double)n;
    double ss = 0.0;
    dcp_fit_pass(x, n, [&](double v) {
        double const d = v - mean;
        ss += d * d;
    });
    double const var = ss / (double)(n - 1u);
    if (var == 0.0) return DCP_FITR_FLAT;
    double lam = 3.14159265358979323846 / sqrt(6.0 * var);
    double const gap = mean - m;
    bool diverged = false, settled = false;
    for (int step = 0; step < DCP_FIT_STEPS; ++step)
    {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        dcp_fit_pass(x, n, [&](double v) {
            double const y = v - m;
            double const w = exp(-(lam * y));
            s0 += w;
            s1 += y * w;
            s2 += (y * y) * w;
        });
        double const r = s1 / s0;
        double const f = 1.0 / lam - gap + r;
        double const df = -1.0 / (lam * lam) - s2 / s0 + r * r;
        double next = lam - f / df;
        if (!dcp_fit_finite(next) || !(next > 0.0)) diverged = true, next = lam;
        double const moved = next > lam ? next - lam : lam - next;
        settled = moved <= 0x1p-40 * next;
        lam = next;
    }
    double s0 = 0.0;
    dcp_fit_pass(x, n, [&](double v) { s0 += exp(-(lam * (v - m))); });
    if (diverged || !settled) return DCP_FITR_DIVERGED;
    *lambda = lam;
    *mu = m - log(s0 / (double)n) / lam;
    return DCP_FITR_OK;
}

// ---- the tail fit -------------------------------------------------------------------------------------------------
// A censored fit: only the scores >= tau, the k-th largest, enter with their values; the z others enter as "below
// tau".  Two rules, each one launch on the device: the selection, which only compares and is exact, and the fit.

// An order-preserving key: a < b <=> key(a) < key(b) for finite a, b, and zeros of either sign share one key (v + 0.0
// is +0.0 for both), so that key order is value order.
DCP_HD inline uint64_t dcp_fit_key(double v)
{
    v += 0.0;
    uint64_t b;
    __builtin_memcpy(&b, &v, sizeof b);
    return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}

// tau = the k-th largest of x(0) .. x(n - 1) by value, 2 <= k <= n (the caller checks), and k_eff = #{x >= tau} >= k:
// 66 passes.  Pass 1: non-finite -> NONFINITE, tau = NaN, k_eff = 0.  Then the key of the k-th largest, bit by bit from
// the top: the largest K with #{key >= K} >= k, one counting pass per bit.  Last pass: k_eff, and tau as the minimum of
// the values that have key >= K, taken as pass 1 of dcp_gumbel_fit_rule takes its minimum (with k = n: its bits).
template <class X> DCP_HD inline int dcp_tail_select_rule(X const &x, unsigned n, unsigned k, double *tau, unsigned *k_eff)
{
    *tau = dcp_fit_nan();
    *k_eff = 0u;
    bool bad = false;
    dcp_fit_pass(x, n, [&](double v) { bad |= !dcp_fit_finite(v); });
    if (bad) return DCP_FITR_NONFINITE;
    uint64_t key = 0u;
    for (int bit = 63; bit >= 0; --bit)
    {
        uint64_t const cand = key | (1ull << bit);
        unsigned cnt = 0u;
        dcp_fit_pass(x, n, [&](double v) { cnt += dcp_fit_key(v) >= cand ? 1u : 0u; });
        key = cnt >= k ? cand : key;
    }
    double m = 1.7976931348623157e308;
    unsigned ke = 0u;
    dcp_fit_pass(x, n, [&](double v) {
        bool const in = dcp_fit_key(v) >= key;
        m = in && v < m ? v : m;
        ke += in ? 1u : 0u;
    });
    *tau = m;
    *k_eff = ke;
    return DCP_FITR_OK;
}

// The censored maximum-likelihood fit, given tau and k_eff = #{x >= tau} of dcp_tail_select_rule: 16 passes, the
// steps and statuses of dcp_gumbel_fit_rule.  log L = k_eff ln lambda - lambda sum_obs (x - mu) - sum_obs exp(-lambda
// (x - mu)) - z exp(-lambda (tau - mu)), z = n - k_eff, the observed set {x >= tau} summed in index order.  Pass 1 and 2
// over all n: NONFINITE; the whole sample's variance, 0 -> FLAT, else lambda = pi / sqrt(6 var).  Pass 3: gap = (sum_obs
// x) / k_eff - tau; 0 -> FLAT (the whole observed set sits at tau).  Newton on
//   f(lambda) = 1 / lambda - gap + s1 / s0,  s0 = sum_obs exp(-lambda y) + z,  s_k = sum_obs y^k exp(-lambda y),  y = x - tau >= 0
// and mu = tau - log(s0 / k_eff) / lambda.  With k_eff = n (tau the minimum, z = 0) these are the sums of
// dcp_gumbel_fit_rule in its order: the same bits.
template <class X>
DCP_HD inline int dcp_gumbel_fit_tail_rule(X const &x, unsigned n, double tau, unsigned k_eff, double *mu, double *lambda)
{
    *mu = *lambda = dcp_fit_nan();
    bool bad = false;
    double sum = 0.0;
    dcp_fit_pass(x, n, [&](double v) {
        bad |= !dcp_fit_finite(v);
        sum += v;
    });
    if (bad) return DCP_FITR_NONFINITE;
    double const mean = sum / (double)n;
    double ss = 0.0;
    dcp_fit_pass(x, n, [&](double v) {
        double const d = v - mean;
        ss += d * d;
    });
    double const var = ss / (double)(n - 1u);
    if (var == 0.0) return DCP_FITR_FLAT;
    double lam = 3.14159265358979323846 / sqrt(6.0 * var);
    double so = 0.0;
    dcp_fit_pass(x, n, [&](double v) {
        if (v >= tau) so += v;
    });
    double const ke = (double)k_eff, z = (double)(n - k_eff);
    double const gap = so / ke - tau;
    if (gap == 0.0) return DCP_FITR_FLAT;
    bool diverged = false, settled = false;
    for (int step = 0; step < DCP_FIT_STEPS; ++step)
    {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        dcp_fit_pass(x, n, [&](double v) {
            if (v >= tau)
            {
                double const y = v - tau;
                double const w = exp(-(lam * y));
                s0 += w;
                s1 += y * w;
                s2 += (y * y) * w;
            }
        });
        s0 += z;
        double const r = s1 / s0;
        double const f = 1.0 / lam - gap + r;
        double const df = -1.0 / (lam * lam) - s2 / s0 + r * r;
        double next = lam - f / df;
        if (!dcp_fit_finite(next) || !(next > 0.0)) diverged = true, next = lam;
        double const moved = next > lam ? next - lam : lam - next;
        settled = moved <= 0x1p-40 * next;
        lam = next;
    }
    double s0 = 0.0;
    dcp_fit_pass(x, n, [&](double v) {
        if (v >= tau) s0 += exp(-(lam * (v - tau)));
    });
    s0 += z;
    if (diverged || !settled) return DCP_FITR_DIVERGED;
    *lambda = lam;
    *mu = tau - log(s0 / ke) / lam;
    return DCP_FITR_OK;
}

// ---- the exponential tail fit ------------------------------------------------------------------------------------------
// The upper tail of Forward scores: P(X >= s) = exp(-lambda (s - mu)) for s >= mu, fitted to the scores
// >= tau by censored maximum likelihood, which is closed-form.  Given tau and k_eff = #{x >= tau} of
// dcp_tail_select_rule: two passes.  Pass 1: non-finite -> NONFINITE.  Pass 2: so = sum_obs (x - tau), the observed set
// {x >= tau} in index order, every term >= 0; so == 0 -> FLAT (the whole observed set sits at tau).  lambda = k_eff / so
// and mu = tau + log(k_eff / n) / lambda, so that P(X >= tau) = k_eff / n: the fitted law is (k_eff / n) exp(-lambda
// (s - tau)).  No Newton step, no exp: comparisons, one ordered sum and one division give lambda, equal in bits wherever
// it runs; only mu passes through the side's own log.  With k_eff = n the log is of 1: mu = tau, the minimum.  Any
// status but OK gives NaN in both outputs.
template <class X>
DCP_HD inline int dcp_exp_tail_fit_rule(X const &x, unsigned n, double tau, unsigned k_eff, double *mu, double *lambda)
{
    *mu = *lambda = dcp_fit_nan();
    bool bad = false;
    dcp_fit_pass(x, n, [&](double v) { bad |= !dcp_fit_finite(v); });
    if (bad) return DCP_FITR_NONFINITE;
    double so = 0.0;
    dcp_fit_pass(x, n, [&](double v) {
        if (v >= tau) so += v - tau;
    });
    if (so == 0.0) return DCP_FITR_FLAT;
    double const ke = (double)k_eff;
    double const lam = ke / so;
    *lambda = lam;
    *mu = tau + log(ke / (double)n) / lam;
    return DCP_FITR_OK;
}

// ---- the launches (dcp_calib.hip) -----------------------------------------------------------------------------------
extern "C" {
// A batch of nseqs sequences of len bases in the resident layout (dcp_seqs.hip: len / 16 + 3 words each, every bit
// behind the last base and every pad word zero): words [nseqs (len / 16 + 3)], woff / len_out [nseqs].  Device
// pointers; the caller has checked that the words and nseqs fit 32 bits.  One launch on `stream`; HIP's error code.
int dcp_launch_random(uint32_t *words, uint32_t *woff, uint32_t *len_out, unsigned nseqs, uint32_t len, uint64_t seed,
                      uint32_t const c[3], void *stream);
// One fit per profile p < nprof of x_q = (double) alt[q nprof + p] - (double) null[q nprof + p], q < nseqs (>= 2):
// mu / lambda [nprof] doubles, status [nprof] bytes.  real_bytes: 4 (float matrices) or 8.  One launch on `stream`.
int dcp_launch_gumbel_fit(void const *null_scores, void const *alt_scores, unsigned nseqs, unsigned nprof, int real_bytes,
                          double *mu, double *lambda, uint8_t *status, void *stream);
// The tail fit of the same x, 2 <= k <= nseqs (the caller checks), as two launches on `stream`.  The selection writes
// tau / k_eff [nprof] (NaN and 0 in a lane with a non-finite score); the fit reads them and writes mu / lambda / status.
int dcp_launch_tail_select(void const *null_scores, void const *alt_scores, unsigned nseqs, unsigned nprof, int real_bytes,
                           unsigned k, double *tau, uint32_t *k_eff, void *stream);
int dcp_launch_gumbel_fit_tail(void const *null_scores, void const *alt_scores, unsigned nseqs, unsigned nprof,
                               int real_bytes, double const *tau, uint32_t const *k_eff, double *mu, double *lambda,
                               uint8_t *status, void *stream);
// The exponential tail fit behind the same selection: one launch on `stream`, the same arrays.
int dcp_launch_exp_tail_fit(void const *null_scores, void const *alt_scores, unsigned nseqs, unsigned nprof, int real_bytes,
                            double const *tau, uint32_t const *k_eff, double *mu, double *lambda, uint8_t *status,
                            void *stream);
}

#endif
