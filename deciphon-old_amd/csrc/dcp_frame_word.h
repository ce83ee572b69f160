// dcp_frame_word.h -- the frame state's emission probability of ONE word, in the probability domain: the formula
// dcp_profile_decode (dcp_model.cpp, host) and decode_kernel (dcp_decode.hip, device) both evaluate.  One source for
// both, so that the operands and the order of the operations are the same on either side: with IEEE double arithmetic
// and no contraction (-ffp-contract=off in both units) equal operands give equal bits.
#ifndef DCP_FRAME_WORD_H
#define DCP_FRAME_WORD_H

#include <stdint.h>

#ifdef __HIP__
#define DCP_HD __host__ __device__
#else
#define DCP_HD
#endif

// imm frame state: probability of emitting word x (1..5 bases) given base probs b and
// codon marginals C (5x5x5, index 4 = wildcard) -- the formula of dcp_frame_table_host,
// evaluated for one word.
// C3(p, q, r): codon marginal with wildcard index 4 -- a table or computed on the fly (decode)
// A length outside 1..5 gives -1 (no probability).
template <class C3> DCP_HD double frame_prob_word_of(double const *b, C3 const &c3, double e, double f, uint8_t const *x, unsigned len)
{
    auto s1 = [&](int p) { return c3(p, 4, 4) + c3(4, p, 4) + c3(4, 4, p); };
    auto s2 = [&](int p, int q) { return c3(4, p, q) + c3(p, 4, q) + c3(p, q, 4); };
    double const e2 = e * e, f2 = f * f;
    switch (len)
    {
    case 1: return e2 * f2 / 3.0 * s1(x[0]);
    case 2:
        return 2.0 * e * f2 * f / 3.0 * s2(x[0], x[1]) +
               e2 * e * f / 3.0 * (b[x[1]] * s1(x[0]) + b[x[0]] * s1(x[1]));
    case 3:
        return f2 * f2 * c3(x[0], x[1], x[2]) +
               4.0 * e2 * f2 / 9.0 * (b[x[0]] * s2(x[1], x[2]) + b[x[1]] * s2(x[0], x[2]) + b[x[2]] * s2(x[0], x[1])) +
               e2 * e2 / 9.0 * (b[x[0]] * b[x[1]] * s1(x[2]) + b[x[0]] * b[x[2]] * s1(x[1]) + b[x[1]] * b[x[2]] * s1(x[0]));
    case 4:
    {
        double one = b[x[0]] * c3(x[1], x[2], x[3]) + b[x[1]] * c3(x[0], x[2], x[3]) +
                     b[x[2]] * c3(x[0], x[1], x[3]) + b[x[3]] * c3(x[0], x[1], x[2]);
        double two = 0;
        for (int i = 0; i < 4; ++i)
            for (int j = i + 1; j < 4; ++j)
            {
                int r[2], n = 0;
                for (int k = 0; k < 4; ++k)
                    if (k != i && k != j) r[n++] = x[k];
                two += b[x[i]] * b[x[j]] * s2(r[0], r[1]);
            }
        return e * f2 * f / 2.0 * one + e2 * e * f / 9.0 * two;
    }
    case 5:
    {
        double s = 0;
        for (int i = 0; i < 5; ++i)
            for (int j = i + 1; j < 5; ++j)
            {
                int r[3], n = 0;
                for (int k = 0; k < 5; ++k)
                    if (k != i && k != j) r[n++] = x[k];
                s += b[x[i]] * b[x[j]] * c3(r[0], r[1], r[2]);
            }
        return e2 * f2 / 10.0 * s;
    }
    default: return -1.0;
    }
}

// The marginal table of "the codon IS (a, bb, cc)" with probability pc: pc where every index is that base or the
// wildcard, 0 elsewhere -- read entry by entry instead of being built.
struct dcp_one_codon
{
    int a, bb, cc;
    double pc;
    DCP_HD double operator()(int i, int j, int k) const
    {
        return ((i == 4 || i == a) && (j == 4 || j == bb) && (k == 4 || k == cc)) ? pc : 0.0;
    }
};

#endif
