/* fwd_factor_exhaustive.c -- the largest relative error of dcp_fwd_factor_f32 (csrc/dcp_forward_scaled.h) against exp
 * in double over EVERY float of its supported range -708 .. 708, both signs of zero and the subnormals included; and
 * that the rule never decreases from one float to the next by more than that error allows (a count of the steps on
 * which it decreases at all is printed).  A program of its own: at most 16 threads, a few seconds.
 *
 *   gcc -O2 -std=gnu11 -I include -c tests/c/fwd_factor_exhaustive.c -o fwd_factor_exhaustive.o
 *   g++ -O2 -std=c++17 -I include -I deciphon-old_amd/csrc fwd_factor_exhaustive.o deciphon-old_amd/csrc/dcp_model.cpp \
 *       -lpthread -o fwd_factor_exhaustive
 *
 * Its output is recorded in profiles/forward_scaled/factor_delta.txt; tests/test_forward_scaled.py holds its sampled
 * maximum against the delta recorded there. */
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "dcp_gpu.h"

enum { NTHREADS = 16 };

static float from_bits(uint32_t b)
{
    float f;
    memcpy(&f, &b, sizeof f);
    return f;
}
static uint32_t to_bits(float f)
{
    uint32_t b;
    memcpy(&b, &f, sizeof b);
    return b;
}

struct part
{
    uint32_t lo, hi, sign; /* magnitudes' bit patterns [lo, hi), the sign bit */
    double worst;
    float at;
    uint64_t count, decreasing;
};

static void *run(void *arg)
{
    struct part *p = (struct part *)arg;
    p->worst = 0.0, p->at = 0.0f, p->count = 0, p->decreasing = 0;
    double prev = -1.0;
    for (uint32_t b = p->lo; b < p->hi; ++b)
    {
        float const t = from_bits(b | p->sign);
        double const got = dcp_fwd_factor_f32(t), want = exp((double)t);
        double const rel = fabs(got - want) / want;
        if (rel > p->worst) p->worst = rel, p->at = t;
        /* magnitudes rise: the factor rises with them for t > 0 and falls for t < 0 */
        if (prev >= 0.0 && (p->sign ? got > prev : got < prev)) ++p->decreasing;
        prev = got;
        ++p->count;
    }
    return NULL;
}

int main(void)
{
    uint32_t const top = to_bits(708.0f) + 1u; /* magnitudes 0 .. 708, as bit patterns */
    struct part parts[NTHREADS];
    pthread_t th[NTHREADS];
    /* eight slices of the magnitudes per sign */
    for (int i = 0; i < NTHREADS; ++i)
    {
        int const s = i % 8;
        parts[i].lo = (uint32_t)((uint64_t)top * (uint64_t)s / 8u);
        parts[i].hi = (uint32_t)((uint64_t)top * (uint64_t)(s + 1) / 8u);
        parts[i].sign = i < 8 ? 0u : 0x80000000u;
        if (pthread_create(&th[i], NULL, run, &parts[i])) return 2;
    }
    double worst = 0.0;
    float at = 0.0f;
    uint64_t count = 0, decreasing = 0;
    for (int i = 0; i < NTHREADS; ++i)
    {
        pthread_join(th[i], NULL);
        if (parts[i].worst > worst) worst = parts[i].worst, at = parts[i].at;
        count += parts[i].count, decreasing += parts[i].decreasing;
    }
    printf("floats %llu\n", (unsigned long long)count);
    printf("delta %.17g\n", worst);
    printf("at %.9g (bits 0x%08x)\n", (double)at, to_bits(at));
    printf("steps against the direction of exp %llu\n", (unsigned long long)decreasing);
    /* the ends of the range and what lies outside it */
    int const ends_ok = dcp_fwd_factor_f32(-INFINITY) == 0.0 && dcp_fwd_factor_f32(nextafterf(-708.0f, -INFINITY)) == 0.0 &&
                        dcp_fwd_factor_f32(-708.0f) > 0.0 && dcp_fwd_factor_f32(-708.0f) >= 2.2250738585072014e-308 &&
                        isfinite(dcp_fwd_factor_f32(708.0f)) && isinf(dcp_fwd_factor_f32(nextafterf(708.0f, INFINITY))) &&
                        dcp_fwd_factor_f32(0.0f) == 1.0 && dcp_fwd_factor_f32(-0.0f) == 1.0;
    printf("ends %s\n", ends_ok ? "ok" : "WRONG");
    return ends_ok ? 0 : 1;
}
