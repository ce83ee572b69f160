// dcp_model.cpp -- host side of the scan engine: builds the compact profile
// ("dcpx") the device consumes. Product code; never calls the oracle.
//
// Restates, MI355X-first, what the reference's model layer computes:
//   protein_model_init / add_node / add_trans / setup_transitions
//       src/model/protein_model.c:49-137, 460-500
//   setup_nuclt_dist / codon_lprob / nuclt_lprob      :342-408
//   calculate_occupancy, setup_entry_trans            :258-283, :410-439
//   protein_profile_sample / setup                    src/model/protein_profile.c:155-304
// Differences by design: the reference keeps per-state imm_dp emission tables
// on the host and re-reads them per pair; here only the 129-float nuclt_dist
// per node and an 8-row transition matrix are kept, and all arithmetic is done
// in double in the probability domain and rounded once to float32 (imm_float).
#include "dcp_host.h"

#include <algorithm>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <string>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <mutex>
#include <vector>

namespace
{
constexpr double kNegInf = -std::numeric_limits<double>::infinity();
constexpr float kNegInfF = -std::numeric_limits<float>::infinity();

// --- imm_rnd: xoshiro256+ seeded with splitmix64 (pinned by the reference's
// golden test/protein_profile.c:41 through the oracle's search) -------------
struct Rnd
{
    uint64_t s[4];
    explicit Rnd(uint64_t seed)
    {
        for (auto &v : s)
        {
            uint64_t z = (seed += 0x9e3779b97f4a7c15ULL);
            z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
            z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
            v = z ^ (z >> 31);
        }
    }
    static uint64_t rotl(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
    double next()
    {
        uint64_t const r = s[0] + s[3];
        uint64_t const t = s[1] << 17;
        s[2] ^= s[0];
        s[3] ^= s[1];
        s[1] ^= s[2];
        s[0] ^= s[3];
        s[2] ^= t;
        s[3] = rotl(s[3], 45);
        return (double)(r >> 11) * 0x1.0p-53;
    }
};

double logsumexp(double const *v, int n)
{
    double m = kNegInf;
    for (int i = 0; i < n; ++i)
        m = std::fmax(m, v[i]);
    if (!(m > kNegInf)) return kNegInf;
    double s = 0;
    for (int i = 0; i < n; ++i)
        s += std::exp(v[i] - m);
    return m + std::log(s);
}

double logadd(double a, double b)
{
    double v[2] = {a, b};
    return logsumexp(v, 2);
}

// imm_lprob_sample + imm_lprob_normalize on imm_float values
void sample_normalized(Rnd &rnd, int n, float *out, int const *force_zero,
                       int nforce)
{
    std::vector<double> lp((size_t)n);
    for (int i = 0; i < n; ++i)
        lp[(size_t)i] = (double)(float)std::log(rnd.next());
    for (int i = 0; i < nforce; ++i)
        lp[(size_t)force_zero[i]] = kNegInf;
    double z = logsumexp(lp.data(), n);
    for (int i = 0; i < n; ++i)
        out[i] = (float)(lp[(size_t)i] - z);
}

// NCBI genetic code 1 (imm_gc table 1), codon index = 16*b1 + 4*b2 + b3 in the
// TCAG order of the published table; converted to ACGT ids below.
constexpr char kGcAmino[] =
    "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";
constexpr int kTcagToAcgt[4] = {3, 1, 0, 2};
constexpr char kAminoSymbols[] = "ACDEFGHIKLMNPQRSTVWY";

struct CodonTable
{
    char aa[64];        // amino acid (or '*') of codon a*16+b*4+c in ACGT ids
    int synonyms[128];  // number of codons per amino acid letter
    CodonTable()
    {
        std::memset(synonyms, 0, sizeof synonyms);
        for (int i = 0; i < 64; ++i)
        {
            int a = kTcagToAcgt[i >> 4], b = kTcagToAcgt[(i >> 2) & 3],
                c = kTcagToAcgt[i & 3];
            aa[a * 16 + b * 4 + c] = kGcAmino[i];
            synonyms[(int)kGcAmino[i]]++;
        }
    }
};
CodonTable const g_codons;

// setup_nuclt_dist: amino log-(odds|probs) -> 4 base lprobs + 125 codon marginals
void make_nuclt_dist(float const aa_lprobs[20], float out[DCP_NDIST])
{
    double by_letter[128];
    for (double &v : by_letter)
        v = kNegInf;
    for (int i = 0; i < 20; ++i)
    {
        int letter = kAminoSymbols[i];
        by_letter[letter] =
            (double)aa_lprobs[i] - std::log((double)g_codons.synonyms[letter]);
    }
    double codon_lp[64];
    for (int i = 0; i < 64; ++i)
        codon_lp[i] = by_letter[(int)g_codons.aa[i]]; // stops ('*') stay -inf
    double z = logsumexp(codon_lp, 64);
    double p[64]; // probability domain from here on
    for (int i = 0; i < 64; ++i)
        p[i] = std::exp(codon_lp[i] - z);

    double base[4] = {0, 0, 0, 0};
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b)
            for (int c = 0; c < 4; ++c)
            {
                double third = p[a * 16 + b * 4 + c] / 3.0;
                base[a] += third;
                base[b] += third;
                base[c] += third;
            }
    for (int i = 0; i < 4; ++i)
        out[i] = (float)std::log(base[i]);

    for (int a = 0; a < 5; ++a)
        for (int b = 0; b < 5; ++b)
            for (int c = 0; c < 5; ++c)
            {
                double s = 0;
                for (int i = (a == 4 ? 0 : a); i < (a == 4 ? 4 : a + 1); ++i)
                    for (int j = (b == 4 ? 0 : b); j < (b == 4 ? 4 : b + 1); ++j)
                        for (int k = (c == 4 ? 0 : c); k < (c == 4 ? 4 : c + 1); ++k)
                            s += p[i * 16 + j * 4 + k];
                out[4 + a * 25 + b * 5 + c] = (float)std::log(s);
            }
}

// ---- the double build (IMM_DOUBLE_PRECISION): imm's own log-domain arithmetic, no rounding to float -------------
// imm_lprob_add: logaddexp with log1p, as imm computes it (the order of every sum below is imm's, so that the parts
// are those of the reference's double build to the last bit where the C library's log / exp / log1p agree)
double lp_add(double x, double y)
{
    if (x == y) return x + 0.69314718055994530942;
    double const t = x - y;
    if (t > 0) return x + std::log1p(std::exp(-t));
    if (t <= 0) return y + std::log1p(std::exp(t));
    return t; // NaN
}

// imm_lprob_normalize: subtract the chained sum
void lp_normalize64(unsigned n, double *v)
{
    double s = kNegInf;
    for (unsigned i = 0; i < n; ++i)
        s = lp_add(s, v[i]);
    for (unsigned i = 0; i < n; ++i)
        v[i] -= s;
}

// setup_nuclt_dist in double (protein_model.c:342-408): codon lprobs from the amino lprobs split over synonyms,
// normalised; base lprobs as imm's chained sums over the codon table in its published (TCAG) order; codon marginals
// as chained sums over the matching codons.
void make_nuclt_dist64(double const aa_lprobs[20], double out[DCP_NDIST])
{
    double by_letter[128];
    for (double &v : by_letter)
        v = kNegInf;
    for (int i = 0; i < 20; ++i)
    {
        int const letter = kAminoSymbols[i];
        by_letter[letter] = aa_lprobs[i] - std::log((double)g_codons.synonyms[letter]);
    }
    double codon_lp[64]; // a*16+b*4+c in ACGT ids
    for (int i = 0; i < 64; ++i)
        codon_lp[i] = by_letter[(int)g_codons.aa[i]];
    lp_normalize64(64, codon_lp);
    double base[4] = {kNegInf, kNegInf, kNegInf, kNegInf};
    double const norm = std::log(3.0);
    for (int i = 0; i < 64; ++i) // the genetic code's own codon order
    {
        int const a = kTcagToAcgt[i >> 4], b = kTcagToAcgt[(i >> 2) & 3], c = kTcagToAcgt[i & 3];
        double const lp = codon_lp[a * 16 + b * 4 + c];
        base[a] = lp_add(base[a], lp - norm);
        base[b] = lp_add(base[b], lp - norm);
        base[c] = lp_add(base[c], lp - norm);
    }
    for (int i = 0; i < 4; ++i)
        out[i] = base[i];
    for (int a = 0; a < 5; ++a)
        for (int b = 0; b < 5; ++b)
            for (int c = 0; c < 5; ++c)
            {
                double acc = kNegInf;
                for (int i = (a == 4 ? 0 : a); i < (a == 4 ? 4 : a + 1); ++i)
                    for (int j = (b == 4 ? 0 : b); j < (b == 4 ? 4 : b + 1); ++j)
                        for (int k = (c == 4 ? 0 : c); k < (c == 4 ? 4 : c + 1); ++k)
                            acc = lp_add(acc, codon_lp[i * 16 + j * 4 + k]);
                out[4 + a * 25 + b * 5 + c] = acc;
            }
}

// calculate_occupancy + setup_entry_trans in double (protein_model.c:258-283, 410-439)
void entry_scores64(unsigned M, int entry_dist, double const *trans, double *entry)
{
    if (entry_dist == DCP_ENTRY_DIST_UNIFORM)
    {
        double const Mf = (double)M;
        double const cost = std::log(2.0 / (Mf * (Mf + 1))) * Mf;
        for (unsigned i = 0; i < M; ++i)
            entry[i] = cost;
        return;
    }
    enum { MM, MI, MD, IM, II, DM, DD };
    std::vector<double> locc(M);
    locc[0] = lp_add(trans[MI], trans[MM]);
    for (unsigned i = 1; i < M; ++i)
    {
        double const *t = trans + 7 * (size_t)i;
        double const v0 = locc[i - 1] + lp_add(t[MM], t[MI]);
        double const v1 = std::log1p(-std::exp(locc[i - 1])) + t[DM];
        locc[i] = lp_add(v0, v1);
    }
    double logZ = kNegInf;
    for (unsigned i = 0; i < M; ++i)
        logZ = lp_add(logZ, locc[i] + std::log((double)(M - i)));
    for (unsigned i = 0; i < M; ++i)
        entry[i] = locc[i] - logZ;
}

} // namespace

struct dcp_profile
{
    char accession[DCP_PROFILE_ACC_SIZE];
    unsigned core_size;
    int entry_dist;
    float epsilon;
    std::vector<char> consensus;
    std::vector<float> trans8;     // [8][M]
    std::vector<float> match_dist; // [M][129]
    float null_dist[DCP_NDIST];
    float insert_dist[DCP_NDIST];
    // exp() of the base and codon probabilities of the null and insert distributions, for dcp_profile_decode:
    // most steps of a path are flank steps in N / C / J, all decoded against the null distribution, and the 68
    // exp() calls were two thirds of a decode.  Filled on first use (profiles are read-only once built).
    struct DecodeExp
    {
        double b[4], pc[64];
    };
    mutable std::once_flag decode_once;
    mutable DecodeExp decode_exp[2]; // 0 null, 1 insert
    // A profile of the double build (dcp_profile_new64 / dcp_profile_sample64) keeps its scan-time parts in double
    // as well; the float parts above are then those values rounded once (what the float-only consumers read).
    bool f64 = false;
    double epsilon64 = 0;
    std::vector<double> trans8_64;     // [8][M]
    std::vector<double> match_dist64;  // [M][129]
    std::vector<double> null_dist64;   // [129]
    std::vector<double> insert_dist64; // [129]
    // dcp_profile_decode's exp() cache of null_dist64 / insert_dist64 (the double build decodes with those)
    mutable std::once_flag decode_once64;
    mutable DecodeExp decode_exp64[2]; // 0 null, 1 insert
};

// calculate_occupancy + setup_entry_trans (protein_model.c:258-283,410-439)
static void entry_scores(unsigned M, int entry_dist, float const *trans,
                         float *entry)
{
    if (entry_dist == DCP_ENTRY_DIST_UNIFORM)
    {
        // imm_log(2.0 / (M * (M + 1))) * M  -- reproduced as written (:415)
        float Mf = (float)M;
        float cost = (float)(std::log(2.0 / ((double)Mf * ((double)Mf + 1.0))) * (double)Mf);
        for (unsigned i = 0; i < M; ++i)
            entry[i] = cost;
        return;
    }
    std::vector<double> locc(M);
    auto T = [&](unsigned i, int f) { return (double)trans[7 * i + f]; };
    enum { MM, MI, MD, IM, II, DM, DD };
    locc[0] = logadd(T(0, MI), T(0, MM));
    for (unsigned i = 1; i < M; ++i)
    {
        double v0 = locc[i - 1] + logadd(T(i, MM), T(i, MI));
        double v1 = std::log1p(-std::exp(locc[i - 1])) + T(i, DM);
        locc[i] = logadd(v0, v1);
    }
    double logZ = kNegInf;
    for (unsigned i = 0; i < M; ++i)
        logZ = logadd(logZ, locc[i] + std::log((double)(M - i)));
    for (unsigned i = 0; i < M; ++i)
        entry[i] = (float)(locc[i] - logZ);
}

extern "C" {

dcp_profile *dcp_profile_new(char const *accession, unsigned core_size,
                             int entry_dist, float epsilon,
                             float const *null_lprobs,
                             float const *match_lprobs, float const *trans,
                             char const *consensus, int *rc)
{
    auto fail = [&](int code) -> dcp_profile * {
        if (rc) *rc = code;
        return nullptr;
    };
    if (core_size == 0 || core_size > DCP_CORE_SIZE_MAX) return fail(DCP_EINVAL);
    if (!null_lprobs || !match_lprobs || !trans) return fail(DCP_EINVAL);
    if (entry_dist != DCP_ENTRY_DIST_UNIFORM && entry_dist != DCP_ENTRY_DIST_OCCUPANCY)
        return fail(DCP_EINVAL);
    if (!(epsilon >= 0.0f && epsilon <= 1.0f)) return fail(DCP_EINVAL); // protein_cfg.h:18

    dcp_profile *p = new (std::nothrow) dcp_profile();
    if (!p) return fail(DCP_ENOMEM);
    unsigned const M = core_size;
    std::memset(p->accession, 0, sizeof p->accession);
    if (accession) std::strncpy(p->accession, accession, sizeof p->accession - 1);
    p->core_size = M;
    p->entry_dist = entry_dist;
    p->epsilon = epsilon;
    p->consensus.assign(M + 1, '\0');
    bool ended = !consensus; // a consensus shorter than the core is padded, never read past its NUL
    for (unsigned i = 0; i < M; ++i)
    {
        if (!ended && consensus[i] == '\0') ended = true;
        p->consensus[i] = ended ? '-' : consensus[i];
    }

    // protein_model_init: null dist from the null amino lprobs, insert dist from
    // all-zero log-odds (protein_model.c:122-127)
    make_nuclt_dist(null_lprobs, p->null_dist);
    float const zeros[20] = {0};
    make_nuclt_dist(zeros, p->insert_dist);
    // protein_model_add_node: match dist from lodds = lprob - null (:60-66)
    p->match_dist.resize((size_t)M * DCP_NDIST);
    for (unsigned k = 0; k < M; ++k)
    {
        float lodds[20];
        for (int i = 0; i < 20; ++i)
            lodds[i] = match_lprobs[k * 20 + i] - null_lprobs[i];
        make_nuclt_dist(lodds, &p->match_dist[(size_t)k * DCP_NDIST]);
    }

    // setup_transitions (:460-500) folded into per-destination-node rows.
    // trans[j] (j = i+1) carries the edges between node i and node i+1 and the
    // MI/II edges of node i (:469-489).  B->M1 = trans[0].MM and M_M->E =
    // trans[M].MM are overwritten by entry / exit scores (:421,:433,:448).
    enum { MM, MI, MD, IM, II, DM, DD };
    p->trans8.assign((size_t)8 * M, kNegInfF);
    float *t8 = p->trans8.data();
    entry_scores(M, entry_dist, trans, t8 + DCP_T_ENTRY * M);
    for (unsigned i = 0; i + 1 < M; ++i)
    {
        float const *t = trans + 7 * (i + 1);
        t8[DCP_T_MI * M + i] = t[MI];
        t8[DCP_T_II * M + i] = t[II];
        t8[DCP_T_MM * M + i + 1] = t[MM];
        t8[DCP_T_IM * M + i + 1] = t[IM];
        t8[DCP_T_MD * M + i + 1] = t[MD];
        t8[DCP_T_DD * M + i + 1] = t[DD];
        t8[DCP_T_DM * M + i + 1] = t[DM];
    }
    if (rc) *rc = DCP_OK;
    return p;
}

dcp_profile *dcp_profile_sample(char const *accession, unsigned seed,
                                unsigned core_size, int entry_dist,
                                float epsilon, int *rc)
{
    if (core_size < 2 || core_size > DCP_CORE_SIZE_MAX) // assert(core_size >= 2) :262
    {
        if (rc) *rc = DCP_EINVAL;
        return nullptr;
    }
    Rnd rnd(seed);
    unsigned const M = core_size;
    float null_lp[20];
    sample_normalized(rnd, 20, null_lp, nullptr, 0);
    std::vector<float> match((size_t)20 * M), trans((size_t)7 * (M + 1));
    for (unsigned k = 0; k < M; ++k)
        sample_normalized(rnd, 20, &match[(size_t)20 * k], nullptr, 0);
    for (unsigned i = 0; i <= M; ++i)
    {
        int zero[2] = {6 /*DD*/, 2 /*MD*/};
        int nz = i == 0 ? 1 : (i == M ? 2 : 0);
        sample_normalized(rnd, 7, &trans[(size_t)7 * i], zero, nz);
    }
    return dcp_profile_new(accession, M, entry_dist, epsilon, null_lp,
                           match.data(), trans.data(), nullptr, rc);
}

dcp_profile *dcp_profile_from_parts(char const *accession, unsigned core_size, int entry_dist, float epsilon,
                                    char const *consensus, float const *trans8, float const *null_dist,
                                    float const *insert_dist, float const *match_dist, int *rc)
{
    auto fail = [&](int code) -> dcp_profile * {
        if (rc) *rc = code;
        return nullptr;
    };
    if (core_size == 0 || core_size > DCP_CORE_SIZE_MAX) return fail(DCP_EINVAL);
    if (!trans8 || !null_dist || !insert_dist || !match_dist) return fail(DCP_EINVAL);
    if (!(epsilon >= 0.0f && epsilon <= 1.0f)) return fail(DCP_EINVAL);
    dcp_profile *p = new (std::nothrow) dcp_profile();
    if (!p) return fail(DCP_ENOMEM);
    unsigned const M = core_size;
    std::memset(p->accession, 0, sizeof p->accession);
    if (accession) std::strncpy(p->accession, accession, sizeof p->accession - 1);
    p->core_size = M;
    p->entry_dist = entry_dist;
    p->epsilon = epsilon;
    p->consensus.assign(M + 1, '\0');
    bool ended = !consensus;
    for (unsigned i = 0; i < M; ++i)
    {
        if (!ended && consensus[i] == '\0') ended = true;
        p->consensus[i] = ended ? '-' : consensus[i];
    }
    p->trans8.assign(trans8, trans8 + (size_t)8 * M);
    p->match_dist.assign(match_dist, match_dist + (size_t)M * DCP_NDIST);
    std::memcpy(p->null_dist, null_dist, sizeof p->null_dist);
    std::memcpy(p->insert_dist, insert_dist, sizeof p->insert_dist);
    // a NaN anywhere would poison every max: reject it here rather than on the device
    for (float v : p->trans8)
        if (v != v) { delete p; return fail(DCP_EINVAL); }
    for (float v : p->match_dist)
        if (v != v) { delete p; return fail(DCP_EINVAL); }
    for (int i = 0; i < DCP_NDIST; ++i)
        if (p->null_dist[i] != p->null_dist[i] || p->insert_dist[i] != p->insert_dist[i]) { delete p; return fail(DCP_EINVAL); }
    if (rc) *rc = DCP_OK;
    return p;
}

dcp_profile *dcp_profile_new64(char const *accession, unsigned core_size, int entry_dist, double epsilon,
                               double const *null_lprobs, double const *match_lprobs, double const *trans,
                               char const *consensus, int *rc)
{
    auto fail = [&](int code) -> dcp_profile * {
        if (rc) *rc = code;
        return nullptr;
    };
    if (core_size == 0 || core_size > DCP_CORE_SIZE_MAX) return fail(DCP_EINVAL);
    if (!null_lprobs || !match_lprobs || !trans) return fail(DCP_EINVAL);
    if (entry_dist != DCP_ENTRY_DIST_UNIFORM && entry_dist != DCP_ENTRY_DIST_OCCUPANCY)
        return fail(DCP_EINVAL);
    if (!(epsilon >= 0.0 && epsilon <= 1.0)) return fail(DCP_EINVAL);

    dcp_profile *p = new (std::nothrow) dcp_profile();
    if (!p) return fail(DCP_ENOMEM);
    unsigned const M = core_size;
    std::memset(p->accession, 0, sizeof p->accession);
    if (accession) std::strncpy(p->accession, accession, sizeof p->accession - 1);
    p->core_size = M;
    p->entry_dist = entry_dist;
    p->f64 = true;
    p->epsilon64 = epsilon;
    p->epsilon = (float)epsilon;
    p->consensus.assign(M + 1, '\0');
    bool ended = !consensus;
    for (unsigned i = 0; i < M; ++i)
    {
        if (!ended && consensus[i] == '\0') ended = true;
        p->consensus[i] = ended ? '-' : consensus[i];
    }

    // the same wiring as dcp_profile_new, every value in double
    p->null_dist64.resize(DCP_NDIST);
    p->insert_dist64.resize(DCP_NDIST);
    make_nuclt_dist64(null_lprobs, p->null_dist64.data());
    double const zeros[20] = {0};
    make_nuclt_dist64(zeros, p->insert_dist64.data());
    p->match_dist64.resize((size_t)M * DCP_NDIST);
    for (unsigned k = 0; k < M; ++k)
    {
        double lodds[20];
        for (int i = 0; i < 20; ++i)
            lodds[i] = match_lprobs[k * 20 + i] - null_lprobs[i];
        make_nuclt_dist64(lodds, &p->match_dist64[(size_t)k * DCP_NDIST]);
    }
    enum { MM, MI, MD, IM, II, DM, DD };
    p->trans8_64.assign((size_t)8 * M, kNegInf);
    double *t8 = p->trans8_64.data();
    entry_scores64(M, entry_dist, trans, t8 + DCP_T_ENTRY * M);
    for (unsigned i = 0; i + 1 < M; ++i)
    {
        double const *t = trans + 7 * (i + 1);
        t8[DCP_T_MI * M + i] = t[MI];
        t8[DCP_T_II * M + i] = t[II];
        t8[DCP_T_MM * M + i + 1] = t[MM];
        t8[DCP_T_IM * M + i + 1] = t[IM];
        t8[DCP_T_MD * M + i + 1] = t[MD];
        t8[DCP_T_DD * M + i + 1] = t[DD];
        t8[DCP_T_DM * M + i + 1] = t[DM];
    }
    // the float parts: the double values rounded once
    p->trans8.assign(p->trans8_64.begin(), p->trans8_64.end());
    p->match_dist.assign(p->match_dist64.begin(), p->match_dist64.end());
    for (int i = 0; i < DCP_NDIST; ++i)
    {
        p->null_dist[i] = (float)p->null_dist64[i];
        p->insert_dist[i] = (float)p->insert_dist64[i];
    }
    if (rc) *rc = DCP_OK;
    return p;
}

dcp_profile *dcp_profile_sample64(char const *accession, unsigned seed, unsigned core_size, int entry_dist,
                                  double epsilon, int *rc)
{
    if (core_size < 2 || core_size > DCP_CORE_SIZE_MAX)
    {
        if (rc) *rc = DCP_EINVAL;
        return nullptr;
    }
    // imm_lprob_sample + imm_lprob_normalize on doubles: the same random stream as dcp_profile_sample
    Rnd rnd(seed);
    unsigned const M = core_size;
    auto sample = [&](unsigned n, double *out) {
        for (unsigned i = 0; i < n; ++i)
            out[i] = std::log(rnd.next());
    };
    double null_lp[20];
    sample(20, null_lp);
    lp_normalize64(20, null_lp);
    std::vector<double> match((size_t)20 * M), trans((size_t)7 * (M + 1));
    for (unsigned k = 0; k < M; ++k)
    {
        sample(20, &match[(size_t)20 * k]);
        lp_normalize64(20, &match[(size_t)20 * k]);
    }
    for (unsigned i = 0; i <= M; ++i)
    {
        double *t = &trans[(size_t)7 * i];
        sample(7, t);
        if (i == 0) t[6] = kNegInf; // DD
        if (i == M) t[2] = t[6] = kNegInf; // MD, DD
        lp_normalize64(7, t);
    }
    return dcp_profile_new64(accession, M, entry_dist, epsilon, null_lp, match.data(), trans.data(), nullptr, rc);
}

dcp_profile *dcp_profile_from_parts64(char const *accession, unsigned core_size, int entry_dist, double epsilon,
                                      char const *consensus, double const *trans8, double const *null_dist,
                                      double const *insert_dist, double const *match_dist, int *rc)
{
    auto fail = [&](int code) -> dcp_profile * {
        if (rc) *rc = code;
        return nullptr;
    };
    if (core_size == 0 || core_size > DCP_CORE_SIZE_MAX) return fail(DCP_EINVAL);
    if (!trans8 || !null_dist || !insert_dist || !match_dist) return fail(DCP_EINVAL);
    if (!(epsilon >= 0.0 && epsilon <= 1.0)) return fail(DCP_EINVAL);
    dcp_profile *p = new (std::nothrow) dcp_profile();
    if (!p) return fail(DCP_ENOMEM);
    unsigned const M = core_size;
    std::memset(p->accession, 0, sizeof p->accession);
    if (accession) std::strncpy(p->accession, accession, sizeof p->accession - 1);
    p->core_size = M;
    p->entry_dist = entry_dist;
    p->f64 = true;
    p->epsilon64 = epsilon;
    p->epsilon = (float)epsilon;
    p->consensus.assign(M + 1, '\0');
    bool ended = !consensus;
    for (unsigned i = 0; i < M; ++i)
    {
        if (!ended && consensus[i] == '\0') ended = true;
        p->consensus[i] = ended ? '-' : consensus[i];
    }
    p->trans8_64.assign(trans8, trans8 + (size_t)8 * M);
    p->match_dist64.assign(match_dist, match_dist + (size_t)M * DCP_NDIST);
    p->null_dist64.assign(null_dist, null_dist + DCP_NDIST);
    p->insert_dist64.assign(insert_dist, insert_dist + DCP_NDIST);
    // a NaN anywhere would poison every max: reject it here rather than on the device
    auto has_nan = [](std::vector<double> const &v) {
        for (double x : v)
            if (x != x) return true;
        return false;
    };
    if (has_nan(p->trans8_64) || has_nan(p->match_dist64) || has_nan(p->null_dist64) || has_nan(p->insert_dist64))
    {
        delete p;
        return fail(DCP_EINVAL);
    }
    // the float parts: the double values rounded once, as dcp_profile_new64 leaves them
    p->trans8.assign(p->trans8_64.begin(), p->trans8_64.end());
    p->match_dist.assign(p->match_dist64.begin(), p->match_dist64.end());
    for (int i = 0; i < DCP_NDIST; ++i)
    {
        p->null_dist[i] = (float)p->null_dist64[i];
        p->insert_dist[i] = (float)p->insert_dist64[i];
    }
    if (rc) *rc = DCP_OK;
    return p;
}

void dcp_lprob_normalize64(unsigned n, double *lprobs) { lp_normalize64(n, lprobs); }

int dcp_profile_precision(dcp_profile const *p) { return p && p->f64 ? 64 : 32; }
double dcp_profile_epsilon64(dcp_profile const *p) { return p->f64 ? p->epsilon64 : (double)p->epsilon; }
double const *dcp_profile_trans8_64(dcp_profile const *p) { return p->f64 ? p->trans8_64.data() : nullptr; }
double const *dcp_profile_null_dist64(dcp_profile const *p) { return p->f64 ? p->null_dist64.data() : nullptr; }
double const *dcp_profile_insert_dist64(dcp_profile const *p) { return p->f64 ? p->insert_dist64.data() : nullptr; }
double const *dcp_profile_match_dist64(dcp_profile const *p) { return p->f64 ? p->match_dist64.data() : nullptr; }

// protein_profile_setup in double (protein_profile.c:155-216)
int dcp_xtrans64(unsigned seq_size, int multi_hits, int hmmer3_compat, double out[DCP_NXTRANS])
{
    if (seq_size == 0) return DCP_EINVAL;
    double const L = (double)seq_size;
    double q = 0.0, log_q = kNegInf;
    if (multi_hits)
    {
        q = 0.5;
        log_q = std::log(0.5);
    }
    double const lp = std::log(L) - std::log(L + 2 + q / (1 - q));
    double const l1p = std::log(2 + q / (1 - q)) - std::log(L + 2 + q / (1 - q));
    double const lr = std::log(L) - std::log(L + 1);
    double NN = lp, CC = lp, JJ = lp;
    double const NB = l1p, CT = l1p, JB = l1p, RR = lr, EJ = log_q, EC = std::log(1 - q);
    if (hmmer3_compat) NN = CC = JJ = 0.0;
    out[DCP_X_RR] = RR;
    out[DCP_X_SB] = NB;
    out[DCP_X_SN] = NN;
    out[DCP_X_NN] = NN;
    out[DCP_X_NB] = NB;
    out[DCP_X_ET] = EC + CT;
    out[DCP_X_EC] = EC + CC;
    out[DCP_X_CC] = CC;
    out[DCP_X_CT] = CT;
    out[DCP_X_EB] = EJ + JB;
    out[DCP_X_EJ] = EJ + JJ;
    out[DCP_X_JJ] = JJ;
    out[DCP_X_JB] = JB;
    return DCP_OK;
}

void dcp_rnd_seed(uint64_t state[4], uint64_t seed)
{
    Rnd r(seed);
    std::memcpy(state, r.s, sizeof r.s);
}

double dcp_rnd_next(uint64_t state[4])
{
    Rnd r(0);
    std::memcpy(r.s, state, sizeof r.s);
    double const v = r.next();
    std::memcpy(state, r.s, sizeof r.s);
    return v;
}

void dcp_lprob_normalize(unsigned n, float *lprobs)
{
    std::vector<double> lp(lprobs, lprobs + n);
    double const z = logsumexp(lp.data(), (int)n);
    for (unsigned i = 0; i < n; ++i)
        lprobs[i] = (float)(lp[i] - z);
}

int dcp_profile_entry_dist(dcp_profile const *p) { return p->entry_dist; }

void dcp_profile_del(dcp_profile *p) { delete p; }
unsigned dcp_profile_core_size(dcp_profile const *p) { return p->core_size; }
char const *dcp_profile_accession(dcp_profile const *p) { return p->accession; }
char const *dcp_profile_consensus(dcp_profile const *p) { return p->consensus.data(); }
float const *dcp_profile_trans8(dcp_profile const *p) { return p->trans8.data(); }
float const *dcp_profile_null_dist(dcp_profile const *p) { return p->null_dist; }
float const *dcp_profile_insert_dist(dcp_profile const *p) { return p->insert_dist; }
float const *dcp_profile_match_dist(dcp_profile const *p) { return p->match_dist.data(); }
float dcp_profile_epsilon(dcp_profile const *p) { return p->epsilon; }

// Frame-state emission in the probability domain (imm frame state; the 4-event
// indel model of SURVEY Appendix A).  b = base probs, C = codon marginals.
void dcp_frame_table_host(float const dist[DCP_NDIST], float epsilon,
                          float out[DCP_NCODES])
{
    double b[4], C[125];
    for (int i = 0; i < 4; ++i)
        b[i] = std::exp((double)dist[i]);
    for (int i = 0; i < 125; ++i)
        C[i] = std::exp((double)dist[4 + i]);
    double const e = (double)epsilon, f = 1.0 - (double)epsilon;
    double const e2 = e * e, f2 = f * f;
    auto c3 = [&](int x, int y, int z) { return C[x * 25 + y * 5 + z]; };
    auto s1 = [&](int x) { return c3(x, 4, 4) + c3(4, x, 4) + c3(4, 4, x); };
    auto s2 = [&](int x, int y) { return c3(4, x, y) + c3(x, 4, y) + c3(x, y, 4); };

    for (int x = 0; x < 4; ++x)
        out[x] = (float)std::log(e2 * f2 / 3.0 * s1(x));
    for (int v = 0; v < 16; ++v)
    {
        int x1 = v >> 2, x2 = v & 3;
        double p = 2.0 * e * f2 * f / 3.0 * s2(x1, x2) +
                   e2 * e * f / 3.0 * (b[x2] * s1(x1) + b[x1] * s1(x2));
        out[4 + v] = (float)std::log(p);
    }
    for (int v = 0; v < 64; ++v)
    {
        int x1 = v >> 4, x2 = (v >> 2) & 3, x3 = v & 3;
        double p = f2 * f2 * c3(x1, x2, x3) +
                   4.0 * e2 * f2 / 9.0 *
                       (b[x1] * s2(x2, x3) + b[x2] * s2(x1, x3) + b[x3] * s2(x1, x2)) +
                   e2 * e2 / 9.0 *
                       (b[x1] * b[x2] * s1(x3) + b[x1] * b[x3] * s1(x2) +
                        b[x2] * b[x3] * s1(x1));
        out[20 + v] = (float)std::log(p);
    }
    for (int v = 0; v < 256; ++v)
    {
        int x[4] = {v >> 6, (v >> 4) & 3, (v >> 2) & 3, v & 3};
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
        out[84 + v] = (float)std::log(e * f2 * f / 2.0 * one + e2 * e * f / 9.0 * two);
    }
    for (int v = 0; v < 1024; ++v)
    {
        int x[5] = {v >> 8, (v >> 6) & 3, (v >> 4) & 3, (v >> 2) & 3, v & 3};
        double s = 0;
        for (int i = 0; i < 5; ++i)
            for (int j = i + 1; j < 5; ++j)
            {
                int r[3], n = 0;
                for (int k = 0; k < 5; ++k)
                    if (k != i && k != j) r[n++] = x[k];
                s += b[x[i]] * b[x[j]] * c3(r[0], r[1], r[2]);
            }
        out[340 + v] = (float)std::log(e2 * f2 / 10.0 * s);
    }
}

// protein_profile_setup (protein_profile.c:155-216)
int dcp_xtrans(unsigned seq_size, int multi_hits, int hmmer3_compat,
               float out[DCP_NXTRANS])
{
    if (seq_size == 0) return DCP_EINVAL;
    float const L = (float)seq_size;
    float q = 0.0f, log_q = kNegInfF;
    if (multi_hits)
    {
        q = 0.5f;
        log_q = (float)std::log(0.5);
    }
    float lp = (float)std::log((double)L) - (float)std::log((double)(L + 2 + q / (1 - q)));
    float l1p = (float)std::log((double)(2 + q / (1 - q))) -
                (float)std::log((double)(L + 2 + q / (1 - q)));
    float lr = (float)std::log((double)L) - (float)std::log((double)(L + 1));
    float NN = lp, CC = lp, JJ = lp, NB = l1p, CT = l1p, JB = l1p, RR = lr;
    float EJ = log_q, EC = (float)std::log((double)(1 - q));
    if (hmmer3_compat) NN = CC = JJ = 0.0f;
    out[DCP_X_RR] = RR;
    out[DCP_X_SB] = NB;
    out[DCP_X_SN] = NN;
    out[DCP_X_NN] = NN;
    out[DCP_X_NB] = NB;
    out[DCP_X_ET] = EC + CT;
    out[DCP_X_EC] = EC + CC;
    out[DCP_X_CC] = CC;
    out[DCP_X_CT] = CT;
    out[DCP_X_EB] = EJ + JB;
    out[DCP_X_EJ] = EJ + JJ;
    out[DCP_X_JJ] = JJ;
    out[DCP_X_JB] = JB;
    return DCP_OK;
}

float dcp_lrt(float null_loglik, float alt_loglik)
{
    return -2 * (null_loglik - alt_loglik);
}

// xmath_partition_size (xmath.h:24-30) + partition_it (profile_reader.c:54-72)
unsigned dcp_partition_by_count(unsigned nprofiles, unsigned npartitions,
                                unsigned part_size[DCP_NUM_THREADS])
{
    if (npartitions == 0 || npartitions > DCP_NUM_THREADS) return 0;
    unsigned nparts = npartitions < nprofiles ? npartitions : nprofiles;
    for (unsigned i = 0; i < DCP_NUM_THREADS; ++i)
        part_size[i] = 0;
    if (nparts == 0) return 0;
    unsigned i = 0, size = 0;
    unsigned const chunk = (nprofiles + nparts - 1) / nparts;
    for (unsigned j = 0; j < nprofiles; ++j)
    {
        unsigned want = chunk * i <= nprofiles
                            ? (chunk < nprofiles - chunk * i ? chunk : nprofiles - chunk * i)
                            : 0;
        if (++size >= want)
        {
            part_size[i] = size;
            ++i;
            size = 0;
            if (i >= nparts) break;
        }
    }
    return nparts;
}

void dcp_partition_by_cells(unsigned const *core_sizes, unsigned nprofiles,
                            unsigned npartitions, unsigned *part_begin)
{
    uint64_t total = 0;
    for (unsigned i = 0; i < nprofiles; ++i)
        total += core_sizes[i];
    part_begin[0] = 0;
    uint64_t acc = 0;
    unsigned p = 0;
    for (unsigned g = 1; g < npartitions; ++g)
    {
        // boundary g: first profile whose prefix sum reaches g/npartitions of the work
        uint64_t target = (total * g + npartitions / 2) / npartitions;
        while (p < nprofiles && acc + core_sizes[p] / 2 < target)
            acc += core_sizes[p++];
        part_begin[g] = p;
    }
    part_begin[npartitions] = nprofiles;
}

} // extern "C"

// ---------------------------------------------------------------------------
// Hit post-processing: state names, codon decode, product rows
// ---------------------------------------------------------------------------
// the frame state's probability of one word (frame_prob_word_of): shared with the device decode
#include "dcp_frame_word.h"

extern "C" {

// protein_state_name: src/model/protein_state.c:5-39
unsigned dcp_state_name(unsigned id, char name[8])
{
    unsigned const msb = id & (3u << 14);
    if (msb == (3u << 14))
    {
        static char const ext[] = "RSNBEJCT";
        unsigned i = id & 0x3FFFu;
        name[0] = i < 8 ? ext[i] : '?';
        name[1] = '\0';
        return 1;
    }
    name[0] = msb == 0 ? 'M' : msb == (1u << 14) ? 'I' : 'D';
    return (unsigned)snprintf(name + 1, 7, "%u", id & 0x3FFFu) + 1;
}

char dcp_gc_decode(uint8_t const codon[3])
{
    if (codon[0] > 3 || codon[1] > 3 || codon[2] > 3) return 'X';
    return g_codons.aa[codon[0] * 16 + codon[1] * 4 + codon[2]];
}

} // extern "C"

namespace
{
// What a decode of (profile, state) reads: exp() of the 4 base and 64 codon entries of the state's distribution (the
// insert dist for I states, the node's match dist for M states, the null dist otherwise) and epsilon.  Null and insert
// come from the profile's cache, a match dist is exponentiated into `own`.  A profile of the double build decodes
// with its double parts and epsilon, as the reference's IMM_DOUBLE_PRECISION build does: its float parts are those
// rounded once, and a near-tie of two codons can fall either way after that rounding.
void fill_decode_exp(float const *d, dcp_profile::DecodeExp &x)
{
    for (int i = 0; i < 4; ++i)
        x.b[i] = std::exp((double)d[i]);
    for (int a = 0; a < 4; ++a)
        for (int bb = 0; bb < 4; ++bb)
            for (int cc = 0; cc < 4; ++cc)
                x.pc[a * 16 + bb * 4 + cc] = std::exp((double)d[4 + a * 25 + bb * 5 + cc]);
}
void fill_decode_exp(double const *d, dcp_profile::DecodeExp &x)
{
    for (int i = 0; i < 4; ++i)
        x.b[i] = std::exp(d[i]);
    for (int a = 0; a < 4; ++a)
        for (int bb = 0; bb < 4; ++bb)
            for (int cc = 0; cc < 4; ++cc)
                x.pc[a * 16 + bb * 4 + cc] = std::exp(d[4 + a * 25 + bb * 5 + cc]);
}
// the cached exp() of the null (0) and insert (1) dists, in the profile's precision
dcp_profile::DecodeExp const *cached_decode_exp(dcp_profile const *p)
{
    if (p->f64)
    {
        std::call_once(p->decode_once64, [&]() {
            fill_decode_exp(p->null_dist64.data(), p->decode_exp64[0]), fill_decode_exp(p->insert_dist64.data(), p->decode_exp64[1]);
        });
        return p->decode_exp64;
    }
    std::call_once(p->decode_once, [&]() { fill_decode_exp(p->null_dist, p->decode_exp[0]), fill_decode_exp(p->insert_dist, p->decode_exp[1]); });
    return p->decode_exp;
}
// DCP_EINVAL for a bad fragment, an M index outside the core or a mute state (assert(!protein_state_is_mute) :310)
int decode_operands(dcp_profile const *p, uint8_t const *frag, unsigned len, unsigned state_id, dcp_profile::DecodeExp &own,
                    dcp_profile::DecodeExp const **x, double *e)
{
    if (!p || !frag || len < 1 || len > 5) return DCP_EINVAL;
    for (unsigned i = 0; i < len; ++i)
        if (frag[i] > 3) return DCP_EINVAL;
    unsigned const msb = state_id & (3u << 14);
    unsigned const k = (state_id & 0x3FFFu) - 1u; // protein_state_idx of an M state
    if (msb == 0 && k >= p->core_size) return DCP_EINVAL;
    if (state_id == ((3u << 14) | 1u) || state_id == ((3u << 14) | 3u) || state_id == ((3u << 14) | 4u) ||
        state_id == ((3u << 14) | 7u) || msb == (2u << 14))
        return DCP_EINVAL;
    int const which = msb == (1u << 14) ? 1 : msb == 0 ? 2 : 0; // the null, the insert or the node's match dist
    if (which == 2)
    {
        if (p->f64) fill_decode_exp(&p->match_dist64[(size_t)k * DCP_NDIST], own);
        else fill_decode_exp(&p->match_dist[(size_t)k * DCP_NDIST], own);
        *x = &own;
    }
    else
        *x = &cached_decode_exp(p)[which];
    *e = p->f64 ? p->epsilon64 : (double)p->epsilon;
    return DCP_OK;
}
} // namespace

// csrc-internal (dcp_host.h): the exp() cache of the null and insert dists as dcp_profile_decode reads it --
// out[0..67] null {b[4], pc[64]}, out[68..135] insert -- and the epsilon it decodes with.  The device decode takes its
// operands for I, N, J, C, R steps from here, so both sides multiply the same doubles.
extern "C" void dcp_profile_decode_exp(dcp_profile const *p, double out[136], double *epsilon)
{
    dcp_profile::DecodeExp const *x = cached_decode_exp(p);
    for (int w = 0; w < 2; ++w)
    {
        std::memcpy(out + 68 * w, x[w].b, sizeof x[w].b);
        std::memcpy(out + 68 * w + 4, x[w].pc, sizeof x[w].pc);
    }
    *epsilon = p->f64 ? p->epsilon64 : (double)p->epsilon;
}

extern "C" {

// protein_profile_decode (src/model/protein_profile.c:306-331): the distribution is the
// insert dist for I states, the node's match dist for M states, the null dist otherwise;
// imm_frame_cond_decode = arg-max over the 64 codons of p(fragment, codon).  A profile of the double build decodes
// with its double parts and epsilon, as the reference's IMM_DOUBLE_PRECISION build does: its float parts are those
// rounded once, and a near-tie of two codons can fall either way after that rounding.
int dcp_profile_decode(dcp_profile const *p, uint8_t const *frag, unsigned len, unsigned state_id,
                       uint8_t codon[3])
{
    if (!codon) return DCP_EINVAL;
    dcp_profile::DecodeExp own;
    dcp_profile::DecodeExp const *x = nullptr;
    double e;
    if (int rc = decode_operands(p, frag, len, state_id, own, &x, &e)) return rc;
    double const *b = x->b;
    double const f = 1.0 - e;
    double best = -1.0;
    codon[0] = codon[1] = codon[2] = 4;
    for (int a = 0; a < 4; ++a)
        for (int bb = 0; bb < 4; ++bb)
            for (int cc = 0; cc < 4; ++cc)
            {
                // the marginal table of "the codon IS (a, bb, cc)" (dcp_one_codon), read entry by entry instead of
                // being built (125 stores per codon, 64 codons per decoded step); the sums see the same operands in
                // the same order, so the arg-max is the one the table gave
                dcp_one_codon const c3{a, bb, cc, x->pc[a * 16 + bb * 4 + cc]};
                double const v = frame_prob_word_of(b, c3, e, f, frag, len);
                if (v >= best)
                {
                    best = v;
                    codon[0] = (uint8_t)a, codon[1] = (uint8_t)bb, codon[2] = (uint8_t)cc;
                }
            }
    return best >= 0.0 ? DCP_OK : DCP_EINVAL;
}

// p(fragment, codon) of ONE codon: the quantity dcp_profile_decode maximises, from the same operands
int dcp_profile_codon_joint(dcp_profile const *p, uint8_t const *frag, unsigned len, unsigned state_id,
                            uint8_t const codon[3], double *out)
{
    if (!codon || !out || codon[0] > 3 || codon[1] > 3 || codon[2] > 3) return DCP_EINVAL;
    dcp_profile::DecodeExp own;
    dcp_profile::DecodeExp const *x = nullptr;
    double e;
    if (int rc = decode_operands(p, frag, len, state_id, own, &x, &e)) return rc;
    dcp_one_codon const c3{codon[0], codon[1], codon[2], x->pc[codon[0] * 16 + codon[1] * 4 + codon[2]]};
    *out = frame_prob_word_of(x->b, c3, e, 1.0 - e, frag, len);
    return DCP_OK;
}

char const *dcp_prod_header(void)
{
    return "scan_id\tseq_id\tprofile_name\tabc_name\talt_loglik\tnull_loglik\tprofile_typeid\tversion\tmatch\n";
}

// prod_fwrite + protein_match_write_func (src/server/prod.c:13-41,153-181; protein_match.c:21-56).  codes: NULL (every
// emitting step is decoded here) or one code per step as dcp_gpu_decode_paths writes them.
static long format_row(char *buf, size_t cap, int64_t scan_id, int64_t seq_id,
                       char const *profile_name, char const *abc_name, double alt_loglik,
                       double null_loglik, char const *profile_typeid, char const *version,
                       dcp_profile const *prof, uint8_t const *seq, unsigned seq_len,
                       struct dcp_step const *steps, unsigned nsteps, uint8_t const *codes)
{
    if (!buf || !prof || !seq || (nsteps && !steps)) return -1;
    std::string out;
    char head[512];
    int n = snprintf(head, sizeof head, "%" PRId64 "\t%" PRId64 "\t%s\t%s\t%.17g\t%.17g\t%s\t%s\t", scan_id,
                     seq_id, profile_name ? profile_name : "", abc_name ? abc_name : "", alt_loglik,
                     null_loglik, profile_typeid ? profile_typeid : "", version ? version : "");
    if (n < 0 || (size_t)n >= sizeof head) return -1;
    out.assign(head, (size_t)n);
    unsigned start = 0;
    for (unsigned i = 0; i < nsteps; ++i)
    {
        unsigned const len = steps[i].seqlen, id = steps[i].state_id;
        if (start + len > seq_len) return -1;
        if (i > 0) out.push_back(';');
        for (unsigned k = 0; k < len; ++k)
            out.push_back("ACGT"[seq[start + k] & 3]);
        out.push_back(',');
        char name[8];
        dcp_state_name(id, name);
        out += name;
        out.push_back(',');
        bool const mute = len == 0; // S, B, E, T and D states (protein_state_is_mute)
        if (codes && (mute ? codes[i] != DCP_CODE_MUTE : codes[i] > 63u)) return -1;
        if (!mute)
        {
            uint8_t codon[3];
            if (codes) codon[0] = (uint8_t)(codes[i] >> 4), codon[1] = (uint8_t)((codes[i] >> 2) & 3u), codon[2] = (uint8_t)(codes[i] & 3u);
            else if (dcp_profile_decode(prof, seq + start, len, id, codon)) return -1;
            for (int k = 0; k < 3; ++k)
                out.push_back("ACGT"[codon[k] & 3]);
            out.push_back(',');
            out.push_back(dcp_gc_decode(codon));
        }
        else
            out.push_back(',');
        start += len;
    }
    out.push_back('\n');
    if (out.size() + 1 > cap) return -1;
    std::memcpy(buf, out.data(), out.size());
    buf[out.size()] = '\0';
    return (long)out.size();
}

long dcp_prod_format_row(char *buf, size_t cap, int64_t scan_id, int64_t seq_id,
                         char const *profile_name, char const *abc_name, double alt_loglik,
                         double null_loglik, char const *profile_typeid, char const *version,
                         dcp_profile const *prof, uint8_t const *seq, unsigned seq_len,
                         struct dcp_step const *steps, unsigned nsteps)
{
    return format_row(buf, cap, scan_id, seq_id, profile_name, abc_name, alt_loglik, null_loglik, profile_typeid, version,
                      prof, seq, seq_len, steps, nsteps, nullptr);
}

long dcp_prod_format_row_codes(char *buf, size_t cap, int64_t scan_id, int64_t seq_id,
                               char const *profile_name, char const *abc_name, double alt_loglik,
                               double null_loglik, char const *profile_typeid, char const *version,
                               dcp_profile const *prof, uint8_t const *seq, unsigned seq_len,
                               struct dcp_step const *steps, unsigned nsteps, uint8_t const *codes)
{
    if (nsteps && !codes) return -1;
    return format_row(buf, cap, scan_id, seq_id, profile_name, abc_name, alt_loglik, null_loglik, profile_typeid, version,
                      prof, seq, seq_len, steps, nsteps, codes ? codes : (uint8_t const *)"");
}

} // extern "C"

// ---------------------------------------------------------------------------
// HMMER3 ASCII reader
// ---------------------------------------------------------------------------
#include <sstream>

struct dcp_h3reader
{
    FILE *fp = nullptr;
    bool owns_fp = false;
    int entry_dist;
    float epsilon;
    std::string err;
    unsigned line_no = 0;
    // parameters of the profile the last next() parsed (dcp_h3reader_next_params)
    std::vector<float> trans, match;
    std::string cons, name, acc;
    ~dcp_h3reader()
    {
        if (fp && owns_fp) std::fclose(fp);
    }
};

namespace
{
// one numeric field of a HMMER3 model line: -ln(p), or '*' for p = 0  ->  ln(p)
bool h3_lprob(std::string const &tok, float *out)
{
    if (tok == "*")
    {
        *out = kNegInfF;
        return true;
    }
    char *end = nullptr;
    double v = std::strtod(tok.c_str(), &end);
    if (end == tok.c_str() || *end != '\0' || !(v >= 0.0)) return false;
    *out = (float)(-v);
    if (*out == 0.0f) *out = 0.0f; // no negative zero
    return true;
}

std::vector<std::string> h3_split(std::string const &line)
{
    std::vector<std::string> out;
    std::istringstream ss(line);
    std::string tok;
    while (ss >> tok)
        out.push_back(tok);
    return out;
}
} // namespace

extern "C" {

void dcp_swissprot_null_lprobs(float out[DCP_AMINO_SIZE])
{
    // HMMER3's Swiss-Prot 50.8 amino-acid frequencies, alphabet order ACDEFGHIKLMNPQRSTVWY
    static double const freq[20] = {0.0787945, 0.0151600, 0.0535222, 0.0668298, 0.0397062, 0.0695071, 0.0229198,
                                    0.0590092, 0.0594422, 0.0963728, 0.0237718, 0.0414386, 0.0482904, 0.0395639,
                                    0.0540978, 0.0683364, 0.0540687, 0.0673417, 0.0114135, 0.0304133};
    for (int i = 0; i < 20; ++i)
        out[i] = (float)std::log(freq[i]);
}

dcp_h3reader *dcp_h3reader_open_fp(FILE *fp, int entry_dist, float epsilon)
{
    if (!fp) return nullptr;
    dcp_h3reader *r = new (std::nothrow) dcp_h3reader();
    if (!r) return nullptr;
    r->fp = fp;
    r->entry_dist = entry_dist;
    r->epsilon = epsilon;
    return r;
}

dcp_h3reader *dcp_h3reader_open(char const *path, int entry_dist, float epsilon)
{
    if (!path) return nullptr;
    FILE *fp = std::fopen(path, "r");
    if (!fp) return nullptr;
    dcp_h3reader *r = dcp_h3reader_open_fp(fp, entry_dist, epsilon);
    if (!r) std::fclose(fp);
    else r->owns_fp = true;
    return r;
}

char const *dcp_h3reader_error(dcp_h3reader const *r) { return r ? r->err.c_str() : "no reader"; }
void dcp_h3reader_close(dcp_h3reader *r) { delete r; }

int dcp_h3reader_next_params(dcp_h3reader *r, struct dcp_h3params *out)
{
    if (!r || !out) return DCP_EINVAL;
    std::memset(out, 0, sizeof *out);
    auto parse_error = [&](std::string const &what) {
        r->err = "line " + std::to_string(r->line_no) + ": " + what;
        return (int)DCP_EPARSE;
    };
    std::string line;
    auto next_line = [&]() -> bool {
        char buf[4096];
        for (;;)
        {
            line.clear();
            bool got = false;
            while (std::fgets(buf, sizeof buf, r->fp)) // a line may be longer than the buffer
            {
                got = true;
                line += buf;
                if (!line.empty() && line.back() == '\n') break;
            }
            if (!got) return false;
            ++r->line_no;
            while (!line.empty() && (line.back() == '\n' || line.back() == '\r'))
                line.pop_back();
            if (line.find_first_not_of(" \t") != std::string::npos) return true;
        }
    };

    // ---- header -----------------------------------------------------------
    if (!next_line()) return DCP_END;
    if (line.compare(0, 6, "HMMER3") != 0) return parse_error("expected a HMMER3 header");
    std::string name, acc, alph;
    unsigned leng = 0;
    bool have_leng = false;
    for (;;)
    {
        if (!next_line()) return parse_error("unexpected end of file in the header");
        std::vector<std::string> f = h3_split(line);
        if (f[0] == "HMM") break;
        if (f.size() >= 2)
        {
            if (f[0] == "NAME") name = f[1];
            else if (f[0] == "ACC") acc = f[1];
            else if (f[0] == "ALPH") alph = f[1];
            else if (f[0] == "LENG")
            {
                char *end = nullptr;
                long v = std::strtol(f[1].c_str(), &end, 10);
                if (*end != '\0' || v < 0) return parse_error("bad LENG");
                leng = (unsigned)v;
                have_leng = true;
            }
        }
    }
    if (!have_leng) return parse_error("missing LENG");
    if (alph != "amino") return parse_error("ALPH must be amino");
    {
        std::vector<std::string> f = h3_split(line); // "HMM A C D ... Y"
        if (f.size() != 21) return parse_error("expected 20 amino-acid columns");
        for (int i = 0; i < 20; ++i)
            if (f[(size_t)i + 1].size() != 1 || f[(size_t)i + 1][0] != kAminoSymbols[i])
                return parse_error("amino-acid columns are not in ACDEFGHIKLMNPQRSTVWY order");
    }
    if (!next_line()) return parse_error("missing the transition header line"); // m->m m->i ...
    if (leng == 0 || leng > DCP_CORE_SIZE_MAX)
    {
        r->err = "core size out of range";
        return DCP_EINVAL; // protein_model_setup: protein_model.c:157-160
    }

    std::vector<float> &trans = r->trans, &match = r->match;
    std::string &cons = r->cons;
    trans.assign((size_t)7 * (leng + 1), 0.0f);
    match.assign((size_t)20 * leng, 0.0f);
    cons.assign(leng, '-');
    auto read_trans = [&](unsigned i) -> bool {
        std::vector<std::string> f = h3_split(line);
        if (f.size() != 7) return false;
        for (int k = 0; k < 7; ++k) // m->m m->i m->d i->m i->i d->m d->d = MM MI MD IM II DM DD
            if (!h3_lprob(f[(size_t)k], &trans[(size_t)7 * i + k])) return false;
        return true;
    };

    // ---- node 0: optional COMPO line, insert emissions, transitions ---------------------------
    if (!next_line()) return parse_error("unexpected end of file");
    if (h3_split(line)[0] == "COMPO" && !next_line()) return parse_error("unexpected end of file");
    if (h3_split(line).size() != 20) return parse_error("expected the insert emissions of node 0");
    if (!next_line() || !read_trans(0)) return parse_error("bad transitions of node 0");

    // ---- nodes 1..LENG -------------------------------------------------------------------------
    for (unsigned k = 1; k <= leng; ++k)
    {
        if (!next_line()) return parse_error("unexpected end of file in the model");
        std::vector<std::string> f = h3_split(line);
        if (f.size() < 21) return parse_error("bad match line");
        char *end = nullptr;
        long idx = std::strtol(f[0].c_str(), &end, 10);
        if (*end != '\0' || idx != (long)k) return parse_error("node index out of sequence");
        for (int a = 0; a < 20; ++a)
            if (!h3_lprob(f[(size_t)a + 1], &match[(size_t)20 * (k - 1) + a])) return parse_error("bad match emission");
        if (f.size() >= 23 && f[22].size() == 1) cons[k - 1] = f[22][0]; // MAP CONS RF MM CS
        if (!next_line() || h3_split(line).size() != 20) return parse_error("bad insert line");
        if (!next_line() || !read_trans(k)) return parse_error("bad transition line");
    }
    if (!next_line() || h3_split(line)[0] != "//") return parse_error("expected the // terminator");

    r->name = name;
    r->acc = acc;
    out->core_size = leng;
    out->match_lprobs = match.data();
    out->trans = trans.data();
    out->consensus = cons.c_str();
    out->name = r->name.c_str();
    out->acc = r->acc.c_str();
    return DCP_OK;
}

int dcp_h3reader_next(dcp_h3reader *r, dcp_profile **out)
{
    if (!r || !out) return DCP_EINVAL;
    *out = nullptr;
    struct dcp_h3params prm;
    int rc = dcp_h3reader_next_params(r, &prm);
    if (rc) return rc;
    float null_lp[20];
    dcp_swissprot_null_lprobs(null_lp);
    char const *label = prm.acc[0] ? prm.acc : prm.name; // hmm.c:113-117
    *out = dcp_profile_new(label, prm.core_size, r->entry_dist, r->epsilon, null_lp, prm.match_lprobs, prm.trans,
                           prm.consensus, &rc);
    if (!*out) r->err = "profile rejected";
    return rc;
}

} // extern "C"

// ---------------------------------------------------------------------------
// dcpx container
// ---------------------------------------------------------------------------
struct dcp_db
{
    FILE *fp = nullptr;
    int entry_dist = 0;
    float epsilon = 0;
    std::vector<uint32_t> sizes;
    int64_t profiles_offset = 0; // where the first profile starts
    std::vector<int64_t> offsets; // per profile
};

namespace
{
constexpr uint16_t kDbMagic = 0xC6F0; // MAGIC_NUMBER, include/deciphon/db/types.h:11
constexpr uint32_t kProfileProtein = 2; // PROFILE_PROTEIN, profile_typeid.h

uint32_t profile_bytes(unsigned M)
{
    unsigned cons = (M + 3u) & ~3u;
    return (uint32_t)(DCP_PROFILE_ACC_SIZE + 4 + cons + 4 * (8 * M + 2 * DCP_NDIST + (size_t)M * DCP_NDIST));
}

template <class T> bool wr(FILE *fp, T const *p, size_t n) { return std::fwrite(p, sizeof(T), n, fp) == n; }
template <class T> bool rd(FILE *fp, T *p, size_t n) { return std::fread(p, sizeof(T), n, fp) == n; }
} // namespace

extern "C" {

int dcp_db_write(char const *path, dcp_profile *const *profiles, unsigned n)
{
    if (!path || !profiles || n == 0 || n > (1u << 20)) return DCP_EINVAL;
    for (unsigned i = 0; i < n; ++i)
        if (!profiles[i] || profiles[i]->entry_dist != profiles[0]->entry_dist ||
            profiles[i]->epsilon != profiles[0]->epsilon)
            return DCP_EINVAL; // one protein_cfg per DB
    FILE *fp = std::fopen(path, "wb");
    if (!fp) return DCP_EIO;
    bool ok = true;
    char const magic[4] = {'D', 'C', 'P', 'X'};
    uint16_t const num = kDbMagic, version = 1;
    uint32_t const typeid_ = kProfileProtein, float_size = 4, entry = (uint32_t)profiles[0]->entry_dist, count = n;
    float const eps = profiles[0]->epsilon;
    char abc[8] = "ACGT", amino[24] = "ACDEFGHIKLMNPQRSTVWY";
    ok = ok && wr(fp, magic, 4) && wr(fp, &num, 1) && wr(fp, &version, 1) && wr(fp, &typeid_, 1) &&
         wr(fp, &float_size, 1) && wr(fp, &entry, 1) && wr(fp, &eps, 1) && wr(fp, abc, 8) && wr(fp, amino, 24) &&
         wr(fp, &count, 1);
    std::vector<uint32_t> sizes(n);
    for (unsigned i = 0; i < n; ++i)
        sizes[i] = profile_bytes(profiles[i]->core_size);
    ok = ok && wr(fp, sizes.data(), n);
    for (unsigned i = 0; ok && i < n; ++i)
    {
        dcp_profile const *p = profiles[i];
        uint32_t const M = p->core_size;
        std::vector<char> cons((M + 3u) & ~3u, '\0');
        std::memcpy(cons.data(), p->consensus.data(), M);
        ok = wr(fp, p->accession, DCP_PROFILE_ACC_SIZE) && wr(fp, &M, 1) && wr(fp, cons.data(), cons.size()) &&
             wr(fp, p->trans8.data(), (size_t)8 * M) && wr(fp, p->null_dist, DCP_NDIST) &&
             wr(fp, p->insert_dist, DCP_NDIST) && wr(fp, p->match_dist.data(), (size_t)M * DCP_NDIST);
    }
    ok = std::fclose(fp) == 0 && ok;
    return ok ? DCP_OK : DCP_EIO;
}

dcp_db *dcp_db_open(char const *path, int *rc)
{
    auto fail = [&](dcp_db *db, int code) -> dcp_db * {
        if (rc) *rc = code;
        if (db)
        {
            if (db->fp) std::fclose(db->fp);
            delete db;
        }
        return nullptr;
    };
    if (!path) return fail(nullptr, DCP_EINVAL);
    dcp_db *db = new (std::nothrow) dcp_db();
    if (!db) return fail(nullptr, DCP_ENOMEM);
    db->fp = std::fopen(path, "rb");
    if (!db->fp) return fail(db, DCP_EIO);
    char magic[4], abc[8], amino[24];
    uint16_t num = 0, version = 0;
    uint32_t typeid_ = 0, float_size = 0, entry = 0, count = 0;
    float eps = 0;
    if (!(rd(db->fp, magic, 4) && rd(db->fp, &num, 1) && rd(db->fp, &version, 1) && rd(db->fp, &typeid_, 1) &&
          rd(db->fp, &float_size, 1) && rd(db->fp, &entry, 1) && rd(db->fp, &eps, 1) && rd(db->fp, abc, 8) &&
          rd(db->fp, amino, 24) && rd(db->fp, &count, 1)))
        return fail(db, DCP_EIO);
    if (std::memcmp(magic, "DCPX", 4) != 0 || num != kDbMagic || version != 1) return fail(db, DCP_EINVAL); // invalid magic number
    if (typeid_ != kProfileProtein) return fail(db, DCP_EINVAL);                                          // invalid typeid
    if (float_size != 4) return fail(db, DCP_EINVAL);                                                     // invalid float size
    if (entry <= DCP_ENTRY_DIST_NULL || entry > DCP_ENTRY_DIST_OCCUPANCY) return fail(db, DCP_EINVAL);   // invalid entry dist
    if (!(eps >= 0.0f && eps <= 1.0f)) return fail(db, DCP_EINVAL);                                       // invalid epsilon
    if (std::memcmp(abc, "ACGT", 5) != 0 || std::memcmp(amino, "ACDEFGHIKLMNPQRSTVWY", 21) != 0) return fail(db, DCP_EINVAL);
    if (count == 0 || count > (1u << 20)) return fail(db, DCP_EINVAL); // MAX_NPROFILES
    db->entry_dist = (int)entry;
    db->epsilon = eps;
    db->sizes.resize(count);
    if (!rd(db->fp, db->sizes.data(), count)) return fail(db, DCP_EIO);
    db->profiles_offset = (int64_t)std::ftell(db->fp);
    db->offsets.resize((size_t)count + 1);
    db->offsets[0] = db->profiles_offset;
    for (uint32_t i = 0; i < count; ++i)
        db->offsets[i + 1] = db->offsets[i] + db->sizes[i];
    if (std::fseek(db->fp, 0, SEEK_END) != 0 || (int64_t)std::ftell(db->fp) != db->offsets[count])
        return fail(db, DCP_EIO); // truncated or trailing bytes
    if (rc) *rc = DCP_OK;
    return db;
}

void dcp_db_close(dcp_db *db)
{
    if (!db) return;
    if (db->fp) std::fclose(db->fp);
    delete db;
}

unsigned dcp_db_nprofiles(dcp_db const *db) { return (unsigned)db->sizes.size(); }
int dcp_db_entry_dist(dcp_db const *db) { return db->entry_dist; }
float dcp_db_epsilon(dcp_db const *db) { return db->epsilon; }
uint32_t const *dcp_db_profile_sizes(dcp_db const *db) { return db->sizes.data(); }

unsigned dcp_db_partitions(dcp_db const *db, unsigned npartitions, unsigned part_size[DCP_NUM_THREADS],
                           int64_t part_offset[DCP_NUM_THREADS + 1])
{
    // partition_init + partition_it, src/db/profile_reader.c:45-72
    unsigned const nprofs = dcp_db_nprofiles(db);
    unsigned const nparts = dcp_partition_by_count(nprofs, npartitions, part_size);
    if (nparts == 0) return 0;
    for (unsigned i = 0; i <= DCP_NUM_THREADS; ++i)
        part_offset[i] = 0;
    part_offset[0] = db->profiles_offset;
    unsigned i = 0, size = 0;
    for (unsigned j = 0; j < nprofs; ++j)
    {
        part_offset[i + 1] += db->sizes[j];
        if (++size >= part_size[i])
        {
            part_offset[i + 1] += part_offset[i];
            ++i;
            size = 0;
        }
    }
    return nparts;
}

int dcp_db_read(dcp_db *db, unsigned begin, unsigned end, dcp_profile **out)
{
    if (!db || !out || begin > end || end > dcp_db_nprofiles(db)) return DCP_EINVAL;
    if (std::fseek(db->fp, (long)db->offsets[begin], SEEK_SET) != 0) return DCP_EIO;
    for (unsigned i = begin; i < end; ++i)
        out[i - begin] = nullptr;
    for (unsigned i = begin; i < end; ++i)
    {
        dcp_profile *p = new (std::nothrow) dcp_profile();
        if (!p) return DCP_ENOMEM;
        out[i - begin] = p;
        uint32_t M = 0;
        if (!(rd(db->fp, p->accession, DCP_PROFILE_ACC_SIZE) && rd(db->fp, &M, 1))) return DCP_EIO;
        p->accession[DCP_PROFILE_ACC_SIZE - 1] = '\0';
        if (M == 0 || M > DCP_CORE_SIZE_MAX || profile_bytes(M) != db->sizes[i]) return DCP_EPARSE; // profile is too long
        std::vector<char> cons((M + 3u) & ~3u);
        p->core_size = M;
        p->entry_dist = db->entry_dist;
        p->epsilon = db->epsilon;
        p->trans8.resize((size_t)8 * M);
        p->match_dist.resize((size_t)M * DCP_NDIST);
        if (!(rd(db->fp, cons.data(), cons.size()) && rd(db->fp, p->trans8.data(), (size_t)8 * M) &&
              rd(db->fp, p->null_dist, DCP_NDIST) && rd(db->fp, p->insert_dist, DCP_NDIST) &&
              rd(db->fp, p->match_dist.data(), (size_t)M * DCP_NDIST)))
            return DCP_EIO;
        p->consensus.assign(cons.begin(), cons.begin() + M);
        p->consensus.push_back('\0');
    }
    return DCP_OK;
}

// ---------------------------------------------------------------------------
// The window rule (dcp_gpu_seqs_cut_windows): a sequence of L bases is cut into windows of `window` bases every
// `step` bases, the last one anchored at the sequence's end.  Pure integer arithmetic, no device.
// ---------------------------------------------------------------------------
static bool window_rule_ok(unsigned window, unsigned step) { return window >= 1u && step >= 1u && step <= window; }

unsigned dcp_seq_window_count(unsigned L, unsigned window, unsigned step)
{
    if (!window_rule_ok(window, step)) return 0;
    if (L <= window) return 1;
    uint64_t const rest = (uint64_t)L - window; // >= 1
    return (unsigned)(1u + (rest + step - 1u) / step); // <= L - window + 1: fits
}

unsigned dcp_seq_window_start(unsigned L, unsigned window, unsigned step, unsigned i)
{
    if (!window_rule_ok(window, step) || L <= window) return 0;
    uint64_t const at = (uint64_t)i * step, last = (uint64_t)L - window;
    return (unsigned)(at < last ? at : last);
}

int dcp_seq_window_plan(uint32_t const *len, unsigned nseqs, unsigned window, unsigned step, uint64_t *nwindows,
                        uint64_t *nwords)
{
    if (nwindows) *nwindows = 0;
    if (nwords) *nwords = 0;
    if (!window_rule_ok(window, step) || (!len && nseqs)) return DCP_EINVAL;
    uint64_t W = 0, words = 0;
    for (unsigned q = 0; q < nseqs; ++q)
    {
        uint64_t const cnt = dcp_seq_window_count(len[q], window, step);
        uint64_t const wl = len[q] < window ? len[q] : window;
        W += cnt; // cnt < 2^32, nseqs < 2^32: no wrap
        // one term is below 2^32 * 2^29; 2^32 of them could pass 2^64: the total saturates there
        if (__builtin_add_overflow(words, cnt * (wl / 16u + 3u), &words)) words = ~0ull;
    }
    if (nwindows) *nwindows = W;
    if (nwords) *nwords = words;
    return W > 0xffffffffull || words > 0xffffffffull ? DCP_EINVAL : DCP_OK;
}

// ---------------------------------------------------------------------------
// Domains (dcp_gpu_path_domains) on their sources, and one representative per duplicate.  Pure arithmetic, no device.
// ---------------------------------------------------------------------------
int dcp_domains_locate(uint32_t const *res_idx, struct dcp_domain const *dom, unsigned n, uint32_t const *res_len,
                       unsigned per_strand, unsigned strands, uint32_t const *win_src, uint32_t const *win_off,
                       uint32_t *src_out, uint64_t *begin_out, uint64_t *end_out, uint8_t *minus_out)
{
    if (n == 0) return DCP_OK;
    if (!res_idx || !dom || !res_len || !src_out || !begin_out || !end_out || !minus_out) return DCP_EINVAL;
    if (win_src && !win_off) return DCP_EINVAL;
    if (strands < 1u || strands > 2u || per_strand == 0u) return DCP_EINVAL;
    uint64_t const resident = (uint64_t)per_strand * strands;
    // everything is checked before anything is written
    for (unsigned j = 0; j < n; ++j)
    {
        if (res_idx[j] >= resident) return DCP_EINVAL;
        if (dom[j].seq_begin > dom[j].seq_end || dom[j].seq_end > res_len[res_idx[j]]) return DCP_EINVAL;
    }
    for (unsigned j = 0; j < n; ++j)
    {
        uint32_t const r = res_idx[j], i = r % per_strand, len = res_len[r];
        bool const minus = r >= per_strand;
        uint64_t const b = minus ? len - dom[j].seq_end : dom[j].seq_begin;
        uint64_t const e = minus ? len - dom[j].seq_begin : dom[j].seq_end;
        uint64_t const off = win_src ? win_off[i] : 0u;
        src_out[j] = win_src ? win_src[i] : i;
        begin_out[j] = off + b;
        end_out[j] = off + e;
        minus_out[j] = minus ? 1u : 0u;
    }
    return DCP_OK;
}

int dcp_domains_merge(uint32_t const *src, uint8_t const *minus, uint32_t const *profile, uint64_t const *begin,
                      uint64_t const *end, double const *odds, unsigned n, uint8_t *keep_out, unsigned *nkept_out)
{
    if (n == 0)
    {
        if (nkept_out) *nkept_out = 0;
        return DCP_OK;
    }
    if (!src || !minus || !profile || !begin || !end || !odds || !keep_out) return DCP_EINVAL;
    for (unsigned j = 0; j < n; ++j)
        if (odds[j] != odds[j] || end[j] <= begin[j]) return DCP_EINVAL; // (this unit is built with -fhonor-nans)
    auto same_group = [&](unsigned a, unsigned b) {
        return src[a] == src[b] && (minus[a] != 0) == (minus[b] != 0) && profile[a] == profile[b];
    };
    // one sort: by group, then by the rank inside it
    std::vector<unsigned> order(n);
    for (unsigned j = 0; j < n; ++j)
        order[j] = j;
    std::sort(order.begin(), order.end(), [&](unsigned a, unsigned b) {
        if (src[a] != src[b]) return src[a] < src[b];
        if ((minus[a] != 0) != (minus[b] != 0)) return minus[a] == 0;
        if (profile[a] != profile[b]) return profile[a] < profile[b];
        if (odds[a] != odds[b]) return odds[a] > odds[b];
        uint64_t const la = end[a] - begin[a], lb = end[b] - begin[b];
        if (la != lb) return la > lb;
        return a < b;
    });
    unsigned nkept = 0;
    // the kept members of the group at hand by their first base, and the longest of them: a kept member that overlaps
    // [b, e) begins after b - longest and before e, so only that stretch of the map is compared
    std::multimap<uint64_t, unsigned> kept;
    uint64_t longest = 0;
    for (unsigned o = 0; o < n; ++o)
    {
        unsigned const j = order[o];
        if (o > 0 && !same_group(order[o - 1], j)) kept.clear(), longest = 0;
        uint64_t const b = begin[j], e = end[j], len = e - b;
        bool keep = true;
        for (auto it = b > longest ? kept.upper_bound(b - longest) : kept.begin(); keep && it != kept.end() && it->first < e; ++it)
        {
            unsigned const k = it->second;
            uint64_t const lo = std::max(b, begin[k]), hi = std::min(e, end[k]);
            if (hi <= lo) continue;
            uint64_t const ov = hi - lo, shorter = std::min(len, end[k] - begin[k]);
            if (ov > shorter - ov) keep = false; // 2 ov > shorter, with no doubling to overflow
        }
        keep_out[j] = keep ? 1u : 0u;
        if (keep)
        {
            kept.emplace(b, j);
            longest = std::max(longest, len);
            ++nkept;
        }
    }
    if (nkept_out) *nkept_out = nkept;
    return DCP_OK;
}

// Located domains -> the regions to score again (dcp_gpu_seqs_cut_regions): inside each (src, minus, profile) group
// the domains by (begin, end, index); one joins the open cluster while it begins at most max_gap behind the cluster's
// largest end; a cluster [lo, hi) becomes the region [lo - flank, hi + flank) clipped to its source.
int dcp_domains_regions(uint32_t const *src, uint8_t const *minus, uint32_t const *profile, uint64_t const *begin,
                        uint64_t const *end, unsigned n, uint32_t const *src_len, unsigned nsrc, uint64_t max_gap,
                        uint32_t flank, uint32_t *reg_of, uint32_t *reg_src, uint8_t *reg_minus, uint32_t *reg_profile,
                        uint32_t *reg_begin, uint32_t *reg_len, uint32_t *reg_nparts, unsigned cap, unsigned *nregions)
{
    if (!nregions) return DCP_EINVAL;
    if (n == 0)
    {
        *nregions = 0;
        return DCP_OK;
    }
    if (!src || !minus || !profile || !begin || !end || !src_len || !reg_of) return DCP_EINVAL;
    for (unsigned j = 0; j < n; ++j)
        if (src[j] >= nsrc || end[j] <= begin[j] || end[j] > src_len[src[j]]) return DCP_EINVAL;
    std::vector<unsigned> order(n);
    for (unsigned j = 0; j < n; ++j)
        order[j] = j;
    std::sort(order.begin(), order.end(), [&](unsigned a, unsigned b) {
        if (src[a] != src[b]) return src[a] < src[b];
        if ((minus[a] != 0) != (minus[b] != 0)) return minus[a] == 0;
        if (profile[a] != profile[b]) return profile[a] < profile[b];
        if (begin[a] != begin[b]) return begin[a] < begin[b];
        if (end[a] != end[b]) return end[a] < end[b];
        return a < b;
    });
    // a domain opens a cluster if it is the first of its group or begins more than max_gap behind the cluster's end
    // (begin - hi > max_gap: hi + max_gap itself could pass 64 bits)
    auto opens = [&](unsigned o, uint64_t hi) {
        unsigned const j = order[o], p = order[o - 1];
        bool const same = src[j] == src[p] && (minus[j] != 0) == (minus[p] != 0) && profile[j] == profile[p];
        return !same || (begin[j] > hi && begin[j] - hi > max_gap);
    };
    uint64_t count = 1, hi = end[order[0]];
    for (unsigned o = 1; o < n; ++o)
    {
        if (opens(o, hi)) ++count, hi = end[order[o]];
        else hi = std::max(hi, end[order[o]]);
    }
    if (count > cap)
    {
        *nregions = (unsigned)count; // <= n
        return DCP_ENOMEM;
    }
    if (!reg_src || !reg_minus || !reg_profile || !reg_begin || !reg_len || !reg_nparts) return DCP_EINVAL;
    *nregions = (unsigned)count;
    unsigned r = 0;
    uint64_t lo = 0;
    auto close = [&](unsigned j) { // the open cluster [lo, hi) of j's group: every end is within the source's 32 bits
        uint64_t const b = lo - std::min<uint64_t>(lo, flank), e = std::min<uint64_t>(hi + flank, src_len[src[j]]);
        reg_src[r] = src[j], reg_minus[r] = minus[j] ? 1u : 0u, reg_profile[r] = profile[j];
        reg_begin[r] = (uint32_t)b, reg_len[r] = (uint32_t)(e - b);
    };
    for (unsigned o = 0; o < n; ++o)
    {
        unsigned const j = order[o];
        if (o == 0 || opens(o, hi))
        {
            if (o > 0) close(order[o - 1]), ++r;
            lo = begin[j], hi = end[j];
            reg_nparts[r] = 0;
        }
        else hi = std::max(hi, end[j]);
        reg_of[j] = r;
        ++reg_nparts[r];
    }
    close(order[n - 1]);
    return DCP_OK;
}

// dcp_domains_locate for a batch of regions (dcp_gpu_seqs_cut_regions): resident r is the bases [reg_begin[r],
// reg_begin[r] + res_len[r]) of source reg_src[r], reverse-complemented where reg_minus[r].
int dcp_domains_locate_regions(uint32_t const *res_idx, struct dcp_domain const *dom, unsigned n, uint32_t const *res_len,
                               unsigned nres, uint32_t const *reg_src, uint32_t const *reg_begin, uint8_t const *reg_minus,
                               uint32_t *src_out, uint64_t *begin_out, uint64_t *end_out, uint8_t *minus_out)
{
    if (n == 0) return DCP_OK;
    if (!res_idx || !dom || !res_len || !reg_src || !reg_begin || !reg_minus || !src_out || !begin_out || !end_out || !minus_out)
        return DCP_EINVAL;
    for (unsigned j = 0; j < n; ++j)
    {
        if (res_idx[j] >= nres) return DCP_EINVAL;
        if (dom[j].seq_begin > dom[j].seq_end || dom[j].seq_end > res_len[res_idx[j]]) return DCP_EINVAL;
    }
    for (unsigned j = 0; j < n; ++j)
    {
        uint32_t const r = res_idx[j], len = res_len[r];
        bool const minus = reg_minus[r] != 0;
        uint64_t const b = minus ? len - dom[j].seq_end : dom[j].seq_begin;
        uint64_t const e = minus ? len - dom[j].seq_begin : dom[j].seq_end;
        src_out[j] = reg_src[r];
        begin_out[j] = (uint64_t)reg_begin[r] + b;
        end_out[j] = (uint64_t)reg_begin[r] + e;
        minus_out[j] = minus ? 1u : 0u;
    }
    return DCP_OK;
}

} // extern "C"

// ---------------------------------------------------------------------------
// Calibration on the host: the generator's and the fit's twins (the rules are dcp_calib.h, which dcp_calib.hip compiles
// for the device), the Gumbel tail and E-values.  No device.
// ---------------------------------------------------------------------------
#include "dcp_calib.h"

static_assert(DCP_FIT_OK == DCP_FITR_OK && DCP_FIT_FLAT == DCP_FITR_FLAT && DCP_FIT_NONFINITE == DCP_FITR_NONFINITE &&
                  DCP_FIT_DIVERGED == DCP_FITR_DIVERGED,
              "dcp_calib.h restates enum dcp_fit_status");

extern "C" {

int dcp_seq_random_thresholds(double const probs[4], uint32_t c_out[3])
{
    if (!c_out) return DCP_EINVAL;
    uint32_t c[3] = {16384u, 32768u, 49152u};
    if (probs)
    {
        double sum = 0.0, cum[4];
        for (int k = 0; k < 4; ++k)
        {
            if (!std::isfinite(probs[k]) || probs[k] < 0.0) return DCP_EINVAL;
            cum[k] = sum += probs[k];
        }
        if (!(std::fabs(sum - 1.0) <= 1e-6)) return DCP_EINVAL;
        for (int k = 0; k < 3; ++k)
        {
            double const t = std::floor(65536.0 * cum[k] + 0.5);
            c[k] = t >= 65536.0 ? 65536u : (uint32_t)t;
        }
    }
    std::memcpy(c_out, c, sizeof c);
    return DCP_OK;
}

void dcp_seq_random(uint64_t seed, uint32_t q, unsigned len, uint32_t const c[3], uint8_t *ids_out)
{
    if (!c || !ids_out) return;
    uint64_t const key = dcp_rand_key(seed, q);
    for (unsigned b = 0; b < len; b += 4u)
    {
        uint32_t g = dcp_rand_groups(dcp_rand_draw(key, b >> 2), c[0], c[1], c[2]);
        for (unsigned t = 0; t < 4u && b + t < len; ++t, g >>= 2)
            ids_out[b + t] = (uint8_t)(g & 3u);
    }
}

int dcp_gumbel_fit(double const *x, unsigned n, size_t stride, double *mu, double *lambda)
{
    if (!x || !mu || !lambda || n < 2u || stride == 0) return DCP_EINVAL;
    return dcp_gumbel_fit_rule([=](unsigned i) { return x[(size_t)i * stride]; }, n, mu, lambda);
}

int dcp_gumbel_fit_tail(double const *x, unsigned n, size_t stride, unsigned k, double *mu, double *lambda, double *tau,
                        unsigned *k_eff)
{
    if (!x || !mu || !lambda || !tau || !k_eff || n < 2u || stride == 0 || k < 2u || k > n) return DCP_EINVAL;
    auto const at = [=](unsigned i) { return x[(size_t)i * stride]; };
    *mu = *lambda = dcp_fit_nan();
    if (int st = dcp_tail_select_rule(at, n, k, tau, k_eff)) return st;
    return dcp_gumbel_fit_tail_rule(at, n, *tau, *k_eff, mu, lambda);
}

double dcp_gumbel_sf(double mu, double lambda, double s) { return -std::expm1(-std::exp(-lambda * (s - mu))); }

int dcp_exp_tail_fit(double const *x, unsigned n, size_t stride, unsigned k, double *mu, double *lambda, double *tau,
                     unsigned *k_eff)
{
    if (!x || !mu || !lambda || !tau || !k_eff || n < 2u || stride == 0 || k < 2u || k > n) return DCP_EINVAL;
    auto const at = [=](unsigned i) { return x[(size_t)i * stride]; };
    *mu = *lambda = dcp_fit_nan();
    if (int st = dcp_tail_select_rule(at, n, k, tau, k_eff)) return st;
    return dcp_exp_tail_fit_rule(at, n, *tau, *k_eff, mu, lambda);
}

double dcp_exp_sf(double mu, double lambda, double s) { return s <= mu ? 1.0 : std::exp(-lambda * (s - mu)); }

int dcp_scores_evalues(uint32_t const *profile_idx, double const *null, double const *alt, unsigned n, double const *mu,
                       double const *lambda, uint8_t const *status, unsigned nprofiles, double nsearched, int law,
                       double *evalue_out)
{
    if (!std::isfinite(nsearched) || nsearched < 0.0) return DCP_EINVAL;
    if (law != DCP_LAW_GUMBEL && law != DCP_LAW_EXP) return DCP_EINVAL;
    if (n == 0) return DCP_OK;
    if (!profile_idx || !null || !alt || !mu || !lambda || !status || !evalue_out) return DCP_EINVAL;
    for (unsigned i = 0; i < n; ++i) // everything is checked before anything is written
        if (profile_idx[i] >= nprofiles) return DCP_EINVAL;
    for (unsigned i = 0; i < n; ++i)
    {
        uint32_t const p = profile_idx[i];
        double const s = alt[i] - null[i];
        double const sf = law == DCP_LAW_EXP ? dcp_exp_sf(mu[p], lambda[p], s) : dcp_gumbel_sf(mu[p], lambda[p], s);
        evalue_out[i] = status[p] == DCP_FIT_OK ? nsearched * sf : dcp_fit_nan();
    }
    return DCP_OK;
}

} // extern "C"

namespace
{
template <class Hit>
int hits_evalues(Hit const *hits, unsigned n, double const *mu, double const *lambda, uint8_t const *status, unsigned nprofiles,
                 double nsearched, double *evalue_out)
{
    if (!std::isfinite(nsearched) || nsearched < 0.0) return DCP_EINVAL;
    if (n == 0) return DCP_OK;
    if (!hits || !mu || !lambda || !status || !evalue_out) return DCP_EINVAL;
    for (unsigned i = 0; i < n; ++i) // everything is checked before anything is written
        if (hits[i].profile_idx >= nprofiles) return DCP_EINVAL;
    for (unsigned i = 0; i < n; ++i)
    {
        uint32_t const p = hits[i].profile_idx;
        double const s = (double)hits[i].alt_loglik - (double)hits[i].null_loglik;
        evalue_out[i] = status[p] == DCP_FIT_OK ? nsearched * dcp_gumbel_sf(mu[p], lambda[p], s) : dcp_fit_nan();
    }
    return DCP_OK;
}
} // namespace

extern "C" {

int dcp_hits_evalues(struct dcp_hit const *hits, unsigned n, double const *mu, double const *lambda, uint8_t const *status,
                     unsigned nprofiles, double nsearched, double *evalue_out)
{
    return hits_evalues(hits, n, mu, lambda, status, nprofiles, nsearched, evalue_out);
}

int dcp_hits_evalues64(struct dcp_hit64 const *hits, unsigned n, double const *mu, double const *lambda, uint8_t const *status,
                       unsigned nprofiles, double nsearched, double *evalue_out)
{
    return hits_evalues(hits, n, mu, lambda, status, nprofiles, nsearched, evalue_out);
}

} // extern "C"


// ---------------------------------------------------------------------------
// Forward on the host: the twin of dcp_forward.hip.  The end-indexed recursion of the scan with
// every max replaced by lse (dcp_forward.h), sequential in k, every lse in the order written; tables as the device
// holds them ([8][ldk], [1364][ldk], [1364], [1364]) in double.  No device.
// ---------------------------------------------------------------------------
#include "dcp_forward.h"
#include "dcp_posterior.h"

// The sweep itself, arguments checked.  rec, if given, receives per row j = 0 .. L the five values a word starting
// after row j, or a domain beginning or ending there, leaves from: PN(j), PJ(j), PC(j), B(j), E(j) (dcp_posterior.h).
// Pm and Qm, if given, receive P_k(j) and Q_k(j), rows j = 0 .. L of M (dcp_mea.h).
static int forward_sweep(unsigned M, unsigned ldk, double const *trans8, double const *emis_match, double const *emis_insert,
                         double const *emis_null, double const *xtrans, unsigned char const *seq, unsigned L, double *rec,
                         double *null_out, double *alt_out, double *Pm = nullptr, double *Qm = nullptr)
{
    double const *ENT = trans8 + (size_t)DCP_T_ENTRY * ldk, *MM = trans8 + (size_t)DCP_T_MM * ldk,
                 *IM = trans8 + (size_t)DCP_T_IM * ldk, *DM = trans8 + (size_t)DCP_T_DM * ldk,
                 *MD = trans8 + (size_t)DCP_T_MD * ldk, *DD = trans8 + (size_t)DCP_T_DD * ldk,
                 *MI = trans8 + (size_t)DCP_T_MI * ldk, *II = trans8 + (size_t)DCP_T_II * ldk;
    double const *x = xtrans;
    double const ninf = dcp_fwd_ninf();
    // rows j - 1 .. j - 5 of P and Q in slots (j - l) % 5, then the row's M, I, D: DCP_FWD_WORK_ROWS rows of M
    double *const rows = (double *)std::malloc(sizeof(double) * DCP_FWD_WORK_ROWS * (size_t)M);
    if (!rows) return DCP_ENOMEM;
    double *const P = rows, *const Q = rows + 5 * (size_t)M, *const Mr = rows + 10 * (size_t)M, *const Ir = Mr + M,
                 *const Dr = Ir + M;
    double PN[5], PJ[5], PC[5], PR[5];
    for (size_t i = 0; i < 10 * (size_t)M; ++i)
        rows[i] = ninf;
    for (int h = 0; h < 5; ++h)
        PN[h] = PJ[h] = PC[h] = PR[h] = ninf;
    // row 0: S = 0, B = S + SB; N = S + SN; R starts at 0
    double const B0 = 0.0 + x[DCP_X_SB];
    for (unsigned k = 0; k < M; ++k)
        P[k] = B0 + ENT[k];
    PN[0] = 0.0 + x[DCP_X_SN];
    PR[0] = 0.0;
    if (rec) rec[0] = PN[0], rec[1] = ninf, rec[2] = ninf, rec[3] = B0, rec[4] = ninf;
    if (Pm)
        for (unsigned k = 0; k < M; ++k)
            Pm[k] = P[k], Qm[k] = Q[k];

    static unsigned const code_off[5] = {0u, 4u, 20u, 84u, 340u};
    double E = ninf, Cc = ninf, Rr = ninf;
    unsigned w = 0;
    for (unsigned j = 1; j <= L; ++j)
    {
        w = ((w << 2) | seq[j - 1]) & 1023u;
        // words that would start before row 0 meet -inf predecessors: they add exp(-inf) = 0
        unsigned code[5], slot[5];
        for (unsigned l = 1; l <= 5u; ++l)
        {
            code[l - 1] = code_off[l - 1] + (w & ((1u << (2 * l)) - 1u));
            slot[l - 1] = (j + 5u - l) % 5u;
        }
        double cn[5], cj[5], cc[5], cr[5];
        for (int l = 0; l < 5; ++l)
        {
            double const eN = emis_null[code[l]];
            cn[l] = PN[slot[l]] + eN, cj[l] = PJ[slot[l]] + eN, cc[l] = PC[slot[l]] + eN, cr[l] = PR[slot[l]] + eN;
        }
        double const N = dcp_lse5(cn[0], cn[1], cn[2], cn[3], cn[4]), J = dcp_lse5(cj[0], cj[1], cj[2], cj[3], cj[4]);
        Cc = dcp_lse5(cc[0], cc[1], cc[2], cc[3], cc[4]);
        Rr = dcp_lse5(cr[0], cr[1], cr[2], cr[3], cr[4]);
        for (unsigned k = 0; k < M; ++k)
        {
            double cm[5], ci[5];
            for (int l = 0; l < 5; ++l)
            {
                cm[l] = P[(size_t)slot[l] * M + k] + emis_match[(size_t)code[l] * ldk + k];
                ci[l] = Q[(size_t)slot[l] * M + k] + emis_insert[code[l]];
            }
            Mr[k] = dcp_lse5(cm[0], cm[1], cm[2], cm[3], cm[4]);
            Ir[k] = dcp_lse5(ci[0], ci[1], ci[2], ci[3], ci[4]);
        }
        Dr[0] = ninf;
        for (unsigned k = 1; k < M; ++k)
            Dr[k] = dcp_lse2(Mr[k - 1] + MD[k], Dr[k - 1] + DD[k]);
        // E = lse(M_0, M_1, D_1, M_2, D_2, ..): the maximum, then the terms in this order
        double mx = ninf;
        for (unsigned k = 0; k < M; ++k)
            mx = dcp_fwd_max(mx, dcp_fwd_max(Mr[k], Dr[k]));
        double const mm = dcp_fwd_shift(mx);
        double sum = 0.0;
        for (unsigned k = 0; k < M; ++k)
        {
            sum += std::exp(Mr[k] - mm);
            if (k) sum += std::exp(Dr[k] - mm);
        }
        E = mm + std::log(sum);
        double const B = dcp_lse3(N + x[DCP_X_NB], E + x[DCP_X_EB], J + x[DCP_X_JB]);
        unsigned const r = j % 5u; // row j - 5's slot: M(j) and I(j) are formed, nothing reads it any more
        double *const pm = P + (size_t)r * M, *const qi = Q + (size_t)r * M;
        for (unsigned k = 0; k < M; ++k)
        {
            pm[k] = k ? dcp_lse4(B + ENT[k], Mr[k - 1] + MM[k], Ir[k - 1] + IM[k], Dr[k - 1] + DM[k]) : B + ENT[0];
            qi[k] = dcp_lse2(Mr[k] + MI[k], Ir[k] + II[k]);
        }
        if (Pm)
            for (unsigned k = 0; k < M; ++k)
                Pm[(size_t)j * M + k] = pm[k], Qm[(size_t)j * M + k] = qi[k];
        PN[r] = N + x[DCP_X_NN];
        PJ[r] = dcp_lse2(E + x[DCP_X_EJ], J + x[DCP_X_JJ]);
        PC[r] = dcp_lse2(E + x[DCP_X_EC], Cc + x[DCP_X_CC]);
        PR[r] = Rr + x[DCP_X_RR];
        if (rec)
        {
            double *const o = rec + (size_t)DCP_POST_REC * j;
            o[0] = PN[r], o[1] = PJ[r], o[2] = PC[r], o[3] = B, o[4] = E;
        }
    }
    *null_out = Rr;
    *alt_out = dcp_lse2(E + x[DCP_X_ET], Cc + x[DCP_X_CT]);
    std::free(rows);
    return DCP_OK;
}

extern "C" int dcp_forward_tables(unsigned M, unsigned ldk, double const *trans8, double const *emis_match,
                                  double const *emis_insert, double const *emis_null, double const xtrans[13],
                                  unsigned char const *seq, unsigned L, double *null_out, double *alt_out)
{
    if (M == 0 || M > 4096u || ldk < M || L == 0) return DCP_EINVAL;
    if (!trans8 || !emis_match || !emis_insert || !emis_null || !xtrans || !seq || !null_out || !alt_out) return DCP_EINVAL;
    for (unsigned i = 0; i < L; ++i)
        if (seq[i] > 3) return DCP_EINVAL;
    return forward_sweep(M, ldk, trans8, emis_match, emis_insert, emis_null, xtrans, seq, L, nullptr, null_out, alt_out);
}

// ---------------------------------------------------------------------------
// The scaled probability-space Forward on the host: the twin of dcp_forward_scaled.hip.  forward_sweep's recursion by
// dcp_forward_scaled.h's rule, sequential in k, every sum in index order.  No device.
// ---------------------------------------------------------------------------
#include "dcp_forward_scaled.h"

extern "C" double dcp_fwd_factor_f32(float t) { return dcp_fws_factor_f32(t); }

namespace
{
struct ScaledFactor
{
    bool f32;
    double operator()(double t) const { return f32 ? dcp_fws_factor((float)t) : dcp_fws_factor(t); }
};
} // namespace

// The sweep itself.  rec, if given, receives the row records PN(j), PJ(j), PC(j), B(j), E(j) as logs under the exponent
// in force (dcp_backward_scaled.h), rows 0 .. L of an unflagged pair (a flagged one: the rows before its last).
static int forward_scaled_sweep(unsigned M, unsigned ldk, double const *trans8, double const *emis_match,
                                double const *emis_insert, double const *emis_null, double const xtrans[13],
                                unsigned char const *seq, unsigned L, int float_factors, int band, double *null_out,
                                double *alt_out, int *out_of_range, double *rec)
{
    if (M == 0 || M > 4096u || ldk < M || L == 0 || band < 1 || band > 500) return DCP_EINVAL;
    if (!trans8 || !emis_match || !emis_insert || !emis_null || !xtrans || !seq || !null_out || !alt_out || !out_of_range)
        return DCP_EINVAL;
    for (unsigned i = 0; i < L; ++i)
        if (seq[i] > 3) return DCP_EINVAL;
    ScaledFactor const f{float_factors != 0};
    // the transitions' factors once ([8][M]), the rings of P and Q, the row's M, I, D
    double *const rows = (double *)std::malloc(sizeof(double) * (DCP_FWD_WORK_ROWS + 8) * (size_t)M);
    if (!rows) return DCP_ENOMEM;
    double *const P = rows, *const Q = rows + 5 * (size_t)M, *const Mr = rows + 10 * (size_t)M, *const Ir = Mr + M,
                 *const Dr = Ir + M, *const T = Dr + M;
    for (int t = 0; t < 8; ++t)
        for (unsigned k = 0; k < M; ++k)
            T[(size_t)t * M + k] = f(trans8[(size_t)t * ldk + k]);
    double const *ENT = T + (size_t)DCP_T_ENTRY * M, *MM = T + (size_t)DCP_T_MM * M, *IM = T + (size_t)DCP_T_IM * M,
                 *DM = T + (size_t)DCP_T_DM * M, *MD = T + (size_t)DCP_T_MD * M, *DD = T + (size_t)DCP_T_DD * M,
                 *MI = T + (size_t)DCP_T_MI * M, *II = T + (size_t)DCP_T_II * M;
    double x[13];
    for (int i = 0; i < 13; ++i)
        x[i] = f(xtrans[i]);
    double PN[5], PJ[5], PC[5], PR[5];
    for (size_t i = 0; i < 10 * (size_t)M; ++i)
        rows[i] = 0.0;
    for (int h = 0; h < 5; ++h)
        PN[h] = PJ[h] = PC[h] = PR[h] = 0.0;
    // row 0: S = 1, B = SB; N = SN; R starts at 1.  The row's ref is max(PN, B), and the rule applies before P is formed
    int s = 0, sR = 0;
    double B0 = x[DCP_X_SB];
    PN[0] = x[DCP_X_SN];
    if (dcp_fws_finite(B0) && dcp_fws_finite(PN[0]))
        if (int const k = dcp_fws_rescale_by(dcp_fwd_max(PN[0], B0), band))
        {
            double const c = dcp_fws_pow2(-k);
            B0 *= c, PN[0] *= c;
            s = k;
        }
    for (unsigned k = 0; k < M; ++k)
        P[k] = B0 * ENT[k];
    PR[0] = 1.0;
    bool bad = false;
    for (unsigned k = 0; k < M; ++k)
        bad |= !dcp_fws_finite(P[k]);
    bad |= !dcp_fws_finite(PN[0]);
    if (rec && !bad)
    {
        double const ninf = dcp_fwd_ninf();
        rec[0] = dcp_fws_score(PN[0], s), rec[1] = ninf, rec[2] = ninf, rec[3] = dcp_fws_score(B0, s), rec[4] = ninf;
    }

    static unsigned const code_off[5] = {0u, 4u, 20u, 84u, 340u};
    double E = 0.0, Cc = 0.0, Rr = 0.0;
    unsigned w = 0;
    for (unsigned j = 1; j <= L && !bad; ++j)
    {
        w = ((w << 2) | seq[j - 1]) & 1023u;
        unsigned code[5], slot[5];
        double fN[5], fI[5];
        for (unsigned l = 1; l <= 5u; ++l)
        {
            code[l - 1] = code_off[l - 1] + (w & ((1u << (2 * l)) - 1u));
            slot[l - 1] = (j + 5u - l) % 5u;
            fN[l - 1] = f(emis_null[code[l - 1]]);
            fI[l - 1] = f(emis_insert[code[l - 1]]);
        }
        double N = 0.0, J = 0.0;
        Cc = 0.0, Rr = 0.0;
        for (int l = 0; l < 5; ++l)
        {
            N = dcp_fws_fma(PN[slot[l]], fN[l], N), J = dcp_fws_fma(PJ[slot[l]], fN[l], J);
            Cc = dcp_fws_fma(PC[slot[l]], fN[l], Cc), Rr = dcp_fws_fma(PR[slot[l]], fN[l], Rr);
        }
        for (unsigned k = 0; k < M; ++k)
        {
            double m = 0.0, ins = 0.0;
            for (int l = 0; l < 5; ++l)
            {
                m = dcp_fws_fma(P[(size_t)slot[l] * M + k], f(emis_match[(size_t)code[l] * ldk + k]), m);
                ins = dcp_fws_fma(Q[(size_t)slot[l] * M + k], fI[l], ins);
            }
            Mr[k] = m, Ir[k] = ins;
        }
        Dr[0] = 0.0;
        for (unsigned k = 1; k < M; ++k)
            Dr[k] = dcp_fws_fma(DD[k], Dr[k - 1], Mr[k - 1] * MD[k]);
        E = 0.0; // M_0, M_1, D_1, M_2, D_2, .. in this order
        for (unsigned k = 0; k < M; ++k)
        {
            E += Mr[k];
            if (k) E += Dr[k];
        }
        double B = N * x[DCP_X_NB];
        B = dcp_fws_fma(E, x[DCP_X_EB], B);
        B = dcp_fws_fma(J, x[DCP_X_JB], B);
        unsigned const r = j % 5u;
        double *const pm = P + (size_t)r * M, *const qi = Q + (size_t)r * M;
        for (unsigned k = 0; k < M; ++k)
        {
            double p = B * ENT[k];
            if (k)
            {
                p = dcp_fws_fma(Mr[k - 1], MM[k], p);
                p = dcp_fws_fma(Ir[k - 1], IM[k], p);
                p = dcp_fws_fma(Dr[k - 1], DM[k], p);
            }
            pm[k] = p;
            qi[k] = dcp_fws_fma(Ir[k], II[k], Mr[k] * MI[k]);
            bad |= !dcp_fws_finite(p) || !dcp_fws_finite(qi[k]);
        }
        PN[r] = N * x[DCP_X_NN];
        PJ[r] = dcp_fws_fma(J, x[DCP_X_JJ], E * x[DCP_X_EJ]);
        PC[r] = dcp_fws_fma(Cc, x[DCP_X_CC], E * x[DCP_X_EC]);
        PR[r] = Rr * x[DCP_X_RR];
        bad |= !dcp_fws_finite(E) || !dcp_fws_finite(B) || !dcp_fws_finite(PN[r]) || !dcp_fws_finite(PJ[r]) ||
               !dcp_fws_finite(PC[r]) || !dcp_fws_finite(PR[r]);
        if (bad) break;
        if (rec)
        {
            double *const o = rec + (size_t)DCP_POST_REC * j;
            o[0] = dcp_fws_score(PN[r], s), o[1] = dcp_fws_score(PJ[r], s), o[2] = dcp_fws_score(PC[r], s);
            o[3] = dcp_fws_score(B, s), o[4] = dcp_fws_score(E, s);
        }
        double const ref = dcp_fwd_max(dcp_fwd_max(dcp_fwd_max(PN[r], PJ[r]), dcp_fwd_max(PC[r], E)), B);
        if (int const k = dcp_fws_rescale_by(ref, band))
        {
            double const c = dcp_fws_pow2(-k);
            for (size_t i = 0; i < 10 * (size_t)M; ++i)
                rows[i] *= c;
            for (int h = 0; h < 5; ++h)
                PN[h] *= c, PJ[h] *= c, PC[h] *= c;
            E *= c, Cc *= c;
            s += k;
        }
        if (int const k = dcp_fws_rescale_by(PR[r], band))
        {
            double const c = dcp_fws_pow2(-k);
            for (int h = 0; h < 5; ++h)
                PR[h] *= c;
            Rr *= c;
            sR += k;
        }
    }
    double alt = 0.0;
    if (!bad)
    {
        // the last row's E and C with the larger of them in [1, 2): the product with ET, CT near e^-708 stays normal
        int const k = dcp_fws_rescale_by(dcp_fwd_max(E, Cc), 0);
        double const c = dcp_fws_pow2(-k);
        alt = dcp_fws_fma(Cc * c, x[DCP_X_CT], (E * c) * x[DCP_X_ET]);
        s += k;
        bad = !dcp_fws_finite(alt);
    }
    std::free(rows);
    *out_of_range = bad ? 1 : 0;
    if (bad) return DCP_OK; // the scores stay unwritten: the values left the double range
    *null_out = dcp_fws_score(Rr, sR);
    *alt_out = dcp_fws_score(alt, s);
    return DCP_OK;
}

extern "C" int dcp_forward_scaled_tables_band(unsigned M, unsigned ldk, double const *trans8, double const *emis_match,
                                              double const *emis_insert, double const *emis_null, double const xtrans[13],
                                              unsigned char const *seq, unsigned L, int float_factors, int band,
                                              double *null_out, double *alt_out, int *out_of_range)
{
    return forward_scaled_sweep(M, ldk, trans8, emis_match, emis_insert, emis_null, xtrans, seq, L, float_factors, band,
                                null_out, alt_out, out_of_range, nullptr);
}

extern "C" int dcp_forward_scaled_tables(unsigned M, unsigned ldk, double const *trans8, double const *emis_match,
                                         double const *emis_insert, double const *emis_null, double const xtrans[13],
                                         unsigned char const *seq, unsigned L, int float_factors, double *null_out,
                                         double *alt_out, int *out_of_range)
{
    return dcp_forward_scaled_tables_band(M, ldk, trans8, emis_match, emis_insert, emis_null, xtrans, seq, L, float_factors,
                                          DCP_FWS_BAND, null_out, alt_out, out_of_range);
}

// ---------------------------------------------------------------------------
// Backward and the posterior rows on the host: the twin of dcp_posterior.hip and the tests' yardstick.  The rule is
// dcp_posterior.h's; sequential in k, every lse in the order written, bB and E summed in k order from the maximum.  It
// holds the full matrices of bM and bI: it is no hot path.  No device.
// ---------------------------------------------------------------------------
// The Backward sweep itself, arguments checked: br the row records, bM and bI the full matrices, rows 0 .. L + 5 of M
// (rows past L are -inf already), row3 three rows of M for bP, bQ, bD.  Returns bPN(0).
static double backward_sweep(unsigned M, unsigned ldk, double const *trans8, double const *emis_match, double const *emis_insert,
                             double const *emis_null, double const *xtrans, unsigned char const *seq, unsigned L, double *br,
                             double *bM, double *bI, double *row3)
{
    double const *ENT = trans8 + (size_t)DCP_T_ENTRY * ldk, *MM = trans8 + (size_t)DCP_T_MM * ldk,
                 *IM = trans8 + (size_t)DCP_T_IM * ldk, *DM = trans8 + (size_t)DCP_T_DM * ldk,
                 *MD = trans8 + (size_t)DCP_T_MD * ldk, *DD = trans8 + (size_t)DCP_T_DD * ldk,
                 *MI = trans8 + (size_t)DCP_T_MI * ldk, *II = trans8 + (size_t)DCP_T_II * ldk;
    double const *x = xtrans;
    double const ninf = dcp_fwd_ninf();
    double *const bP = row3, *const bQ = bP + M, *const bD = bQ + M;
    static unsigned const code_off[5] = {0u, 4u, 20u, 84u, 340u};
    double bPN0 = ninf;
    for (unsigned j = L;; --j)
    {
        // x[j .. j+l), first base most significant; a word past L meets the -inf rows, whatever its code
        unsigned code[5], v = 0;
        for (unsigned l = 1; l <= 5u; ++l)
        {
            v = (v << 2) | (j + l - 1u < L ? seq[j + l - 1u] : 0u);
            code[l - 1] = code_off[l - 1] + v;
        }
        double cn[5], cj[5], cc[5];
        for (unsigned l = 1; l <= 5u; ++l)
        {
            double const eN = emis_null[code[l - 1]];
            double const *b = br + (size_t)DCP_POST_REC * (j + l);
            cn[l - 1] = eN + b[0], cj[l - 1] = eN + b[1], cc[l - 1] = eN + b[2];
        }
        double const bPN = dcp_lse5(cn[0], cn[1], cn[2], cn[3], cn[4]), bPJ = dcp_lse5(cj[0], cj[1], cj[2], cj[3], cj[4]),
                     bPC = dcp_lse5(cc[0], cc[1], cc[2], cc[3], cc[4]);
        for (unsigned k = 0; k < M; ++k)
        {
            double cm[5], ci[5];
            for (unsigned l = 1; l <= 5u; ++l)
            {
                cm[l - 1] = emis_match[(size_t)code[l - 1] * ldk + k] + bM[(size_t)(j + l) * M + k];
                ci[l - 1] = emis_insert[code[l - 1]] + bI[(size_t)(j + l) * M + k];
            }
            bP[k] = dcp_lse5(cm[0], cm[1], cm[2], cm[3], cm[4]);
            bQ[k] = dcp_lse5(ci[0], ci[1], ci[2], ci[3], ci[4]);
        }
        // bB = lse_k entry_k + bP_k: the maximum, then the terms in k order
        double mx = ninf;
        for (unsigned k = 0; k < M; ++k)
            mx = dcp_fwd_max(mx, ENT[k] + bP[k]);
        double const mm = dcp_fwd_shift(mx);
        double sum = 0.0;
        for (unsigned k = 0; k < M; ++k)
            sum += std::exp((ENT[k] + bP[k]) - mm);
        double const bB = mm + std::log(sum);
        bool const last = j == L;
        double *const o = br + (size_t)DCP_POST_REC * j;
        double const bE = dcp_lse4(last ? x[DCP_X_ET] : ninf, x[DCP_X_EB] + bB, x[DCP_X_EJ] + bPJ, x[DCP_X_EC] + bPC);
        o[0] = dcp_lse2(x[DCP_X_NB] + bB, x[DCP_X_NN] + bPN);
        o[1] = dcp_lse2(x[DCP_X_JB] + bB, x[DCP_X_JJ] + bPJ);
        o[2] = dcp_lse2(last ? x[DCP_X_CT] : ninf, x[DCP_X_CC] + bPC);
        o[3] = bB, o[4] = bE;
        double *const m = bM + (size_t)j * M, *const ins = bI + (size_t)j * M;
        for (unsigned k = M; k-- > 0;)
        {
            bool const nx = k + 1u < M; // node k + 1 exists
            double const dn = nx ? bD[k + 1] : ninf, pn = nx ? bP[k + 1] : ninf;
            bD[k] = dcp_lse3(bE, nx ? DD[k + 1] + dn : ninf, nx ? DM[k + 1] + pn : ninf);
            m[k] = dcp_lse4(bE, nx ? MD[k + 1] + dn : ninf, nx ? MM[k + 1] + pn : ninf, MI[k] + bQ[k]);
            ins[k] = dcp_lse2(nx ? IM[k + 1] + pn : ninf, II[k] + bQ[k]);
        }
        if (j == 0)
        {
            bPN0 = bPN;
            break;
        }
    }
    return bPN0;
}

extern "C" int dcp_posterior_tables(unsigned M, unsigned ldk, double const *trans8, double const *emis_match,
                                    double const *emis_insert, double const *emis_null, double const xtrans[13],
                                    unsigned char const *seq, unsigned L, double *begin_out, double *end_out,
                                    double *core_out, double *alt_fwd_out, double *alt_bwd_out)
{
    if (M == 0 || M > 4096u || ldk < M || L == 0) return DCP_EINVAL;
    if (!trans8 || !emis_match || !emis_insert || !emis_null || !xtrans || !seq) return DCP_EINVAL;
    if (!begin_out || !end_out || !core_out || !alt_fwd_out || !alt_bwd_out) return DCP_EINVAL;
    for (unsigned i = 0; i < L; ++i)
        if (seq[i] > 3) return DCP_EINVAL;
    double const *x = xtrans;
    double const ninf = dcp_fwd_ninf();
    size_t const rows = (size_t)L + 6u; // rows L + 1 .. L + 5 stay -inf: words that would end past L
    size_t const nrec = 2u * (size_t)DCP_POST_REC * rows, nmat = 2u * rows * M, nrow = 3u * (size_t)M;
    double *const mem = (double *)std::malloc(sizeof(double) * (nrec + nmat + nrow));
    if (!mem) return DCP_ENOMEM;
    double *const fr = mem, *const br = fr + DCP_POST_REC * rows, *const bM = mem + nrec, *const bI = bM + rows * M,
                 *const bP = mem + nrec + nmat;
    for (size_t i = 0; i < nrec + nmat; ++i)
        mem[i] = ninf;
    double null_fwd, alt_fwd;
    if (int rc = forward_sweep(M, ldk, trans8, emis_match, emis_insert, emis_null, xtrans, seq, L, fr, &null_fwd, &alt_fwd))
    {
        std::free(mem);
        return rc;
    }
    double const bPN0 = backward_sweep(M, ldk, trans8, emis_match, emis_insert, emis_null, xtrans, seq, L, br, bM, bI, bP);
    double const alt_bwd = dcp_lse2(x[DCP_X_SB] + br[3], x[DCP_X_SN] + bPN0);
    for (unsigned j = 0; j <= L; ++j)
    {
        unsigned win = 0; // bases j - 5 .. j + 3, first most significant; outside the sequence 0
        for (unsigned i = 0; i < 9u; ++i)
        {
            long const t = (long)j - 5 + (long)i;
            win = (win << 2) | (t >= 0 && t < (long)L ? seq[t] : 0u);
        }
        dcp_posterior_row<double>(fr, br, emis_null, win, j, L, alt_fwd, begin_out + j, end_out + j, core_out + j);
    }
    *alt_fwd_out = alt_fwd;
    *alt_bwd_out = alt_bwd;
    std::free(mem);
    return DCP_OK;
}

// ---------------------------------------------------------------------------
// The scaled Backward and the posterior rows on the host: the twin of dcp_backward_scaled.hip.  backward_sweep's
// recursion by dcp_backward_scaled.h's rule, sequential in k, every sum in index order; the rings of bM and bI are five
// rows each, as on the device.  The Forward half is forward_scaled_sweep with its records.  No device.
// ---------------------------------------------------------------------------
#include "dcp_backward_scaled.h"

extern "C" int dcp_posterior_scaled_tables_band(unsigned M, unsigned ldk, double const *trans8, double const *emis_match,
                                                double const *emis_insert, double const *emis_null, double const xtrans[13],
                                                unsigned char const *seq, unsigned L, int float_factors, int band,
                                                double *begin_out, double *end_out, double *core_out, double *alt_fwd_out,
                                                double *alt_bwd_out, int *out_of_range)
{
    if (M == 0 || M > 4096u || ldk < M || L == 0 || band < 1 || band > 500) return DCP_EINVAL;
    if (!trans8 || !emis_match || !emis_insert || !emis_null || !xtrans || !seq) return DCP_EINVAL;
    if (!begin_out || !end_out || !core_out || !alt_fwd_out || !alt_bwd_out || !out_of_range) return DCP_EINVAL;
    for (unsigned i = 0; i < L; ++i)
        if (seq[i] > 3) return DCP_EINVAL;
    ScaledFactor const f{float_factors != 0};
    size_t const rows = (size_t)L + 1u;
    // the two sweeps' records, the transitions' factors ([8][M]), the rings of bM and bI, the row's bP, bQ, bD
    size_t const nrec = 2u * (size_t)DCP_POST_REC * rows, nwork = (size_t)(8 + 10 + 3) * M;
    double *const mem = (double *)std::malloc(sizeof(double) * (nrec + nwork));
    if (!mem) return DCP_ENOMEM;
    double *const fr = mem, *const br = fr + DCP_POST_REC * rows, *const T = mem + nrec, *const bM = T + 8 * (size_t)M,
                 *const bI = bM + 5 * (size_t)M, *const bP = bI + 5 * (size_t)M, *const bQ = bP + M, *const bD = bQ + M;
    for (size_t i = 0; i < nrec; ++i)
        mem[i] = dcp_fwd_ninf();
    double null_fwd = 0.0, alt_fwd = 0.0;
    int oor = 0;
    if (int rc = forward_scaled_sweep(M, ldk, trans8, emis_match, emis_insert, emis_null, xtrans, seq, L, float_factors, band,
                                      &null_fwd, &alt_fwd, &oor, fr))
    {
        std::free(mem);
        return rc;
    }
    if (oor)
    {
        std::free(mem);
        *out_of_range = 1;
        return DCP_OK;
    }
    for (int t = 0; t < 8; ++t)
        for (unsigned k = 0; k < M; ++k)
            T[(size_t)t * M + k] = f(trans8[(size_t)t * ldk + k]);
    double const *ENT = T + (size_t)DCP_T_ENTRY * M, *MM = T + (size_t)DCP_T_MM * M, *IM = T + (size_t)DCP_T_IM * M,
                 *DM = T + (size_t)DCP_T_DM * M, *MD = T + (size_t)DCP_T_MD * M, *DD = T + (size_t)DCP_T_DD * M,
                 *MI = T + (size_t)DCP_T_MI * M, *II = T + (size_t)DCP_T_II * M;
    double x[13];
    for (int i = 0; i < 13; ++i)
        x[i] = f(xtrans[i]);
    for (size_t i = 0; i < 10 * (size_t)M; ++i)
        bM[i] = 0.0; // (bI follows bM)
    double bN[5], bJ[5], bC[5];
    for (int h = 0; h < 5; ++h)
        bN[h] = bJ[h] = bC[h] = 0.0;
    // row L's part of the rule: ref = max(ET, CT), before anything reads the ring
    int s = 0;
    double ETL = x[DCP_X_ET], CTL = x[DCP_X_CT];
    if (dcp_fws_finite(ETL) && dcp_fws_finite(CTL))
        if (int const k = dcp_fws_rescale_by(dcp_fwd_max(ETL, CTL), band))
        {
            double const c = dcp_fws_pow2(-k);
            ETL *= c, CTL *= c;
            s = k;
        }
    static unsigned const code_off[5] = {0u, 4u, 20u, 84u, 340u};
    bool bad = false;
    double bB = 0.0, bPN = 0.0;
    for (unsigned j = L;; --j)
    {
        unsigned code[5], slot[5], v = 0;
        double fN[5], fI[5];
        for (unsigned l = 1; l <= 5u; ++l)
        {
            v = (v << 2) | (j + l - 1u < L ? seq[j + l - 1u] : 0u);
            code[l - 1] = code_off[l - 1] + v;
            slot[l - 1] = (j + l) % 5u; // row j + l's slot; row j itself goes to j % 5, row j + 5's
            fN[l - 1] = f(emis_null[code[l - 1]]);
            fI[l - 1] = f(emis_insert[code[l - 1]]);
        }
        bPN = 0.0;
        double bPJ = 0.0, bPC = 0.0;
        for (int l = 0; l < 5; ++l)
        {
            bPN = dcp_fws_fma(bN[slot[l]], fN[l], bPN), bPJ = dcp_fws_fma(bJ[slot[l]], fN[l], bPJ);
            bPC = dcp_fws_fma(bC[slot[l]], fN[l], bPC);
        }
        for (unsigned k = 0; k < M; ++k)
        {
            double p = 0.0, q = 0.0;
            for (int l = 0; l < 5; ++l)
            {
                p = dcp_fws_fma(bM[(size_t)slot[l] * M + k], f(emis_match[(size_t)code[l] * ldk + k]), p);
                q = dcp_fws_fma(bI[(size_t)slot[l] * M + k], fI[l], q);
            }
            bP[k] = p, bQ[k] = q;
        }
        bB = 0.0;
        for (unsigned k = 0; k < M; ++k)
            bB += ENT[k] * bP[k];
        bool const last = j == L;
        double bE = last ? ETL : 0.0;
        bE = dcp_fws_fma(x[DCP_X_EB], bB, bE);
        bE = dcp_fws_fma(x[DCP_X_EJ], bPJ, bE);
        bE = dcp_fws_fma(x[DCP_X_EC], bPC, bE);
        unsigned const r = j % 5u;
        bN[r] = dcp_fws_fma(x[DCP_X_NN], bPN, x[DCP_X_NB] * bB);
        bJ[r] = dcp_fws_fma(x[DCP_X_JJ], bPJ, x[DCP_X_JB] * bB);
        bC[r] = dcp_fws_fma(x[DCP_X_CC], bPC, last ? CTL : 0.0);
        double *const m = bM + (size_t)r * M, *const ins = bI + (size_t)r * M;
        for (unsigned k = M; k-- > 0;)
        {
            bool const nx = k + 1u < M; // node k + 1 exists; else its factors are 0
            double const dn = nx ? bD[k + 1] : 0.0, pn = nx ? bP[k + 1] : 0.0;
            double const dd = nx ? DD[k + 1] : 0.0, dm = nx ? DM[k + 1] : 0.0, md = nx ? MD[k + 1] : 0.0,
                         mm = nx ? MM[k + 1] : 0.0, im = nx ? IM[k + 1] : 0.0;
            bD[k] = dcp_fws_fma(dd, dn, dcp_fws_fma(dm, pn, bE));
            double mv = dcp_fws_fma(md, dn, bE);
            mv = dcp_fws_fma(mm, pn, mv);
            m[k] = dcp_fws_fma(MI[k], bQ[k], mv);
            ins[k] = dcp_fws_fma(II[k], bQ[k], im * pn);
            bad |= !dcp_fws_finite(m[k]) || !dcp_fws_finite(ins[k]);
        }
        bad |= !dcp_fws_finite(bB) || !dcp_fws_finite(bE) || !dcp_fws_finite(bN[r]) || !dcp_fws_finite(bJ[r]) ||
               !dcp_fws_finite(bC[r]);
        if (bad) break;
        double *const o = br + (size_t)DCP_POST_REC * j;
        o[0] = dcp_fws_score(bN[r], s), o[1] = dcp_fws_score(bJ[r], s), o[2] = dcp_fws_score(bC[r], s);
        o[3] = dcp_fws_score(bB, s), o[4] = dcp_fws_score(bE, s);
        if (dcp_bws_lossy(dcp_bws_rec_max(fr + (size_t)DCP_POST_REC * j), dcp_bws_rec_max(o), alt_fwd, band))
        {
            bad = true;
            break;
        }
        double const ref = dcp_fwd_max(dcp_fwd_max(dcp_fwd_max(bN[r], bJ[r]), dcp_fwd_max(bC[r], bB)), bE);
        if (int const k = dcp_fws_rescale_by(ref, band))
        {
            double const c = dcp_fws_pow2(-k);
            for (size_t i = 0; i < 10 * (size_t)M; ++i)
                bM[i] *= c;
            for (int h = 0; h < 5; ++h)
                bN[h] *= c, bJ[h] *= c, bC[h] *= c;
            bB *= c, bPN *= c;
            s += k;
        }
        if (j == 0) break;
    }
    double alt = 0.0;
    if (!bad)
    {
        // row 0's bB and bPN with the larger of them in [1, 2): the product with SB, SN near e^-708 stays normal
        int const k = dcp_fws_rescale_by(dcp_fwd_max(bB, bPN), 0);
        double const c = dcp_fws_pow2(-k);
        alt = dcp_fws_fma(x[DCP_X_SN], bPN * c, x[DCP_X_SB] * (bB * c));
        s += k;
        bad = !dcp_fws_finite(alt);
    }
    *out_of_range = bad ? 1 : 0;
    if (!bad)
    {
        for (unsigned j = 0; j <= L; ++j)
        {
            unsigned win = 0; // bases j - 5 .. j + 3, first most significant; outside the sequence 0
            for (unsigned i = 0; i < 9u; ++i)
            {
                long const t = (long)j - 5 + (long)i;
                win = (win << 2) | (t >= 0 && t < (long)L ? seq[t] : 0u);
            }
            dcp_posterior_row<double>(fr, br, emis_null, win, j, L, alt_fwd, begin_out + j, end_out + j, core_out + j);
        }
        *alt_fwd_out = alt_fwd;
        *alt_bwd_out = dcp_fws_score(alt, s);
    }
    std::free(mem);
    return DCP_OK;
}

extern "C" int dcp_posterior_scaled_tables(unsigned M, unsigned ldk, double const *trans8, double const *emis_match,
                                           double const *emis_insert, double const *emis_null, double const xtrans[13],
                                           unsigned char const *seq, unsigned L, int float_factors, double *begin_out,
                                           double *end_out, double *core_out, double *alt_fwd_out, double *alt_bwd_out,
                                           int *out_of_range)
{
    return dcp_posterior_scaled_tables_band(M, ldk, trans8, emis_match, emis_insert, emis_null, xtrans, seq, L, float_factors,
                                            DCP_FWS_BAND, begin_out, end_out, core_out, alt_fwd_out, alt_bwd_out, out_of_range);
}

// Envelopes: the maximal runs of bases with core >= threshold that are at least min_len bases long, as half-open base
// intervals in order.  core is dcp_posterior_tables' row [L + 1]: base i is core[i + 1].  *n_out is the true count, of
// which the first cap are written.  Plain C++, no device.
extern "C" int dcp_posterior_envelopes(double const *core, unsigned L, double threshold, unsigned min_len,
                                       unsigned *begin_out, unsigned *end_out, unsigned cap, unsigned *n_out)
{
    if (!n_out || (L && !core) || (cap && (!begin_out || !end_out)) || !(threshold == threshold)) return DCP_EINVAL;
    unsigned n = 0;
    for (unsigned i = 0; i < L;)
    {
        if (!(core[i + 1u] >= threshold))
        {
            ++i;
            continue;
        }
        unsigned e = i + 1u;
        while (e < L && core[e + 1u] >= threshold)
            ++e;
        if (e - i >= min_len)
        {
            if (n < cap) begin_out[n] = i, end_out[n] = e;
            ++n;
        }
        i = e;
    }
    *n_out = n;
    return DCP_OK;
}

// ---------------------------------------------------------------------------
// Envelope records on the host: the twin of dcp_envelopes.hip.  The rule is dcp_envelopes.h's; the bases of a run are
// taken one by one, so the sums run in index order.  No device.
// ---------------------------------------------------------------------------
#include "dcp_envelopes.h"

extern "C" int dcp_posterior_envelope_records(double const *begin, double const *end, double const *core, unsigned L,
                                              double hi, double lo, unsigned min_len, struct dcp_envelope *out,
                                              unsigned cap, unsigned *n_out)
{
    if (!n_out || (L && (!begin || !end || !core)) || (cap && !out) || dcp_env_thresholds_refused(hi, lo)) return DCP_EINVAL;
    unsigned n = 0;
    for (unsigned i = 0; i < L;)
    {
        if (!dcp_env_in(core[i + 1u], lo))
        {
            ++i;
            continue;
        }
        dcp_env_run run{i, i, core[i + 1u], core[i + 1u], begin[i], end[i + 1u]};
        unsigned e = i + 1u;
        for (; e < L && dcp_env_in(core[e + 1u], lo); ++e)
            dcp_env_run_add(run, e, core[e + 1u], core[e + 1u], begin[e], end[e + 1u]);
        if (dcp_env_kept(run.begin, e, run.core_max, hi, min_len))
        {
            if (n < cap) out[n] = dcp_env_record(run, 0u, e);
            ++n;
        }
        i = e;
    }
    *n_out = n;
    return DCP_OK;
}

// Envelopes as dcp_gpu_seqs_cut_regions' (src, begin, length), widened by flank and clipped to their sequences.
extern "C" int dcp_envelopes_regions(struct dcp_envelope const *env, uint64_t n, uint32_t const *seq_idx, unsigned npairs,
                                     uint32_t const *seq_len, unsigned nseqs, unsigned flank, uint32_t *src_out,
                                     uint32_t *begin_out, uint32_t *len_out, uint32_t *profile_pair_out)
{
    if (n && (!env || !seq_idx || !seq_len || !src_out || !begin_out || !len_out || !profile_pair_out)) return DCP_EINVAL;
    for (uint64_t k = 0; k < n; ++k)
    {
        dcp_envelope const &v = env[k];
        if (v.pair >= npairs || seq_idx[v.pair] >= nseqs) return DCP_EINVAL;
        if (v.begin >= v.end || v.end > seq_len[seq_idx[v.pair]]) return DCP_EINVAL;
    }
    for (uint64_t k = 0; k < n; ++k)
    {
        dcp_envelope const &v = env[k];
        uint32_t const src = seq_idx[v.pair], len = seq_len[src];
        uint32_t const b = v.begin > flank ? v.begin - flank : 0u;
        uint32_t const e = len - v.end > flank ? v.end + flank : len;
        src_out[k] = src, begin_out[k] = b, len_out[k] = e - b, profile_pair_out[k] = v.pair;
    }
    return DCP_OK;
}

// ---------------------------------------------------------------------------
// The posterior-decoded alignment on the host: the twin of dcp_mea.hip and the tests' yardstick.  The rule, the choice
// codes and the walk are dcp_mea.h's; the two sweeps are the ones above, with their full matrices.  No device.
// ---------------------------------------------------------------------------
#include "dcp_mea.h"

namespace
{

struct MeaSeq
{
    unsigned char const *s;
    unsigned operator()(unsigned i) const { return s[i]; }
};

// the two sweeps' matrices of one pair, and the max-plus sweep's choices over them
struct MeaHost
{
    void *mem = nullptr;
    double *fr, *br, *bM, *bI, *P, *Q; // records and bM, bI: rows 0 .. L + 5; P, Q: rows 0 .. L
    double *gM, *gI, *gX;              // suffix gains: rows 0 .. L + 5 of M, M and 3
    uint16_t *cell;
    uint32_t *rowc;
    double alt, gain;
    unsigned start;
    ~MeaHost() { std::free(mem); }
};

int mea_sweeps(unsigned M, unsigned ldk, double const *trans8, double const *emis_match, double const *emis_insert,
               double const *emis_null, double const *xtrans, unsigned char const *seq, unsigned L, MeaHost &h)
{
    double const ninf = dcp_fwd_ninf();
    size_t const rows = (size_t)L + 6u, cells = ((size_t)L + 1u) * M;
    size_t const nrec = 2u * (size_t)DCP_POST_REC * rows, nmat = 4u * rows * M + 3u * rows, npq = 2u * cells, nrow = 3u * (size_t)M;
    size_t const ndbl = nrec + nmat + npq + nrow;
    h.mem = std::malloc(sizeof(double) * ndbl + sizeof(uint32_t) * DCP_MEA_ROWC * rows + sizeof(uint16_t) * cells);
    if (!h.mem) return DCP_ENOMEM;
    double *const d = (double *)h.mem;
    h.fr = d, h.br = h.fr + DCP_POST_REC * rows;
    h.bM = d + nrec, h.bI = h.bM + rows * M, h.gM = h.bI + rows * M, h.gI = h.gM + rows * M, h.gX = h.gI + rows * M;
    h.P = d + nrec + nmat, h.Q = h.P + cells;
    double *const row3 = h.Q + cells;
    h.rowc = (uint32_t *)(d + ndbl);
    h.cell = (uint16_t *)(h.rowc + DCP_MEA_ROWC * rows);
    for (size_t i = 0; i < nrec + nmat; ++i)
        d[i] = ninf;
    double null_fwd;
    if (int rc = forward_sweep(M, ldk, trans8, emis_match, emis_insert, emis_null, xtrans, seq, L, h.fr, &null_fwd, &h.alt, h.P, h.Q))
        return rc;
    backward_sweep(M, ldk, trans8, emis_match, emis_insert, emis_null, xtrans, seq, L, h.br, h.bM, h.bI, row3);

    double const *ENT = trans8 + (size_t)DCP_T_ENTRY * ldk, *MM = trans8 + (size_t)DCP_T_MM * ldk,
                 *IM = trans8 + (size_t)DCP_T_IM * ldk, *DM = trans8 + (size_t)DCP_T_DM * ldk,
                 *MD = trans8 + (size_t)DCP_T_MD * ldk, *DD = trans8 + (size_t)DCP_T_DD * ldk,
                 *MI = trans8 + (size_t)DCP_T_MI * ldk, *II = trans8 + (size_t)DCP_T_II * ldk;
    double const *x = xtrans;
    double const a = h.alt;
    double *const gP = row3, *const gQ = gP + M, *const gD = gQ + M;
    MeaSeq const sq{seq};
    double gPN0 = ninf;
    for (unsigned j = L;; --j)
    {
        bool const last = j == L;
        unsigned code[5] = {0, 0, 0, 0, 0};
        unsigned const nl = L - j < 5u ? L - j : 5u; // words that end at or before L
        for (unsigned l = 1; l <= nl; ++l)
            code[l - 1] = dcp_mea_code(sq, j, l);
        dcp_mea_best px[3];
        for (unsigned X = 0; X < 3u; ++X)
        {
            px[X] = dcp_mea_none();
            for (unsigned l = 1; l <= nl; ++l)
                dcp_mea_take(px[X], dcp_mea_word(h.fr[(size_t)DCP_POST_REC * j + X], emis_null[code[l - 1]],
                                                 h.br[(size_t)DCP_POST_REC * (j + l) + X], a, l, h.gX[3u * (size_t)(j + l) + X]), l);
        }
        dcp_mea_best bb = dcp_mea_none();
        uint16_t *const cj = h.cell + (size_t)j * M;
        for (unsigned k = 0; k < M; ++k)
        {
            dcp_mea_best p = dcp_mea_none(), q = dcp_mea_none();
            for (unsigned l = 1; l <= nl; ++l)
            {
                size_t const to = (size_t)(j + l) * M + k;
                dcp_mea_take(p, dcp_mea_word(h.P[(size_t)j * M + k], emis_match[(size_t)code[l - 1] * ldk + k], h.bM[to], a, l, h.gM[to]), l);
                dcp_mea_take(q, dcp_mea_word(h.Q[(size_t)j * M + k], emis_insert[code[l - 1]], h.bI[to], a, l, h.gI[to]), l);
            }
            gP[k] = p.g, gQ[k] = q.g;
            cj[k] = (uint16_t)((p.c << DCP_MEA_SH_P) | (q.c << DCP_MEA_SH_Q));
            dcp_mea_take(bb, dcp_mea_link(ENT[k], p.g), k + 1u);
        }
        dcp_mea_best const c = dcp_mea_c(last, x[DCP_X_CT], x[DCP_X_CC], px[2].g);
        dcp_mea_best const jj = dcp_mea_nj(x[DCP_X_JB], x[DCP_X_JJ], bb.g, px[1].g);
        dcp_mea_best const n = dcp_mea_nj(x[DCP_X_NB], x[DCP_X_NN], bb.g, px[0].g);
        dcp_mea_best const e = dcp_mea_e(last, x[DCP_X_ET], x[DCP_X_EB], x[DCP_X_EJ], x[DCP_X_EC], bb.g, px[1].g, px[2].g);
        double *const gx = h.gX + 3u * (size_t)j;
        gx[0] = n.g, gx[1] = jj.g, gx[2] = c.g;
        h.rowc[(size_t)DCP_MEA_ROWC * j] = (px[0].c << DCP_MEA_SH_PN) | (px[1].c << DCP_MEA_SH_PJ) | (px[2].c << DCP_MEA_SH_PC) |
                                           (n.c << DCP_MEA_SH_N) | (jj.c << DCP_MEA_SH_J) | (c.c << DCP_MEA_SH_C) | (e.c << DCP_MEA_SH_E);
        h.rowc[(size_t)DCP_MEA_ROWC * j + 1u] = bb.c;
        double *const gm = h.gM + (size_t)j * M, *const gi = h.gI + (size_t)j * M;
        for (unsigned k = M; k-- > 0;)
        {
            bool const nx = k + 1u < M; // node k + 1 exists
            double const dn = nx ? gD[k + 1] : ninf, pn = nx ? gP[k + 1] : ninf;
            dcp_mea_best const dd = dcp_mea_d(e.g, nx ? DD[k + 1] : ninf, nx ? DM[k + 1] : ninf, dn, pn);
            dcp_mea_best const mm = dcp_mea_m(e.g, nx ? MD[k + 1] : ninf, nx ? MM[k + 1] : ninf, MI[k], dn, pn, gQ[k]);
            dcp_mea_best const ii = dcp_mea_i(nx ? IM[k + 1] : ninf, II[k], pn, gQ[k]);
            gD[k] = dd.g, gm[k] = mm.g, gi[k] = ii.g;
            cj[k] = (uint16_t)(cj[k] | (mm.c << DCP_MEA_SH_M) | (ii.c << DCP_MEA_SH_I) | (dd.c << DCP_MEA_SH_D));
        }
        if (j == 0)
        {
            gPN0 = px[0].g;
            dcp_mea_best const s = dcp_mea_nj(x[DCP_X_SB], x[DCP_X_SN], bb.g, gPN0);
            h.gain = s.g, h.start = s.c;
            break;
        }
    }
    return DCP_OK;
}

dcp_mea_view<double> mea_view(MeaHost const &h, unsigned M, unsigned ldk, unsigned L, double const *emis_match,
                              double const *emis_insert, double const *emis_null)
{
    dcp_mea_view<double> v;
    v.M = M, v.L = L, v.ldm = M;
    v.P = h.P, v.Q = h.Q, v.bM = h.bM, v.bI = h.bI;
    v.cell = h.cell, v.rowc = h.rowc, v.fr = h.fr, v.br = h.br;
    v.em = emis_match, v.ei = emis_insert, v.en = emis_null, v.ld = ldk;
    return v;
}

bool mea_inputs_ok(unsigned M, unsigned ldk, double const *trans8, double const *emis_match, double const *emis_insert,
                   double const *emis_null, double const *xtrans, unsigned char const *seq, unsigned L)
{
    if (M == 0 || M > 4096u || ldk < M || L == 0) return false;
    if (!trans8 || !emis_match || !emis_insert || !emis_null || !xtrans || !seq) return false;
    for (unsigned i = 0; i < L; ++i)
        if (seq[i] > 3) return false;
    return true;
}

} // namespace

extern "C" int dcp_mea_tables(unsigned M, unsigned ldk, double const *trans8, double const *emis_match,
                              double const *emis_insert, double const *emis_null, double const xtrans[13],
                              unsigned char const *seq, unsigned L, struct dcp_step *steps_out, unsigned cap_steps,
                              unsigned *nsteps_out, double *post_out, double *gain_out, double *alt_fwd_out)
{
    static_assert(sizeof(dcp_step) == sizeof(uint32_t), "a step is one word: state_id | seqlen << 16");
    if (!mea_inputs_ok(M, ldk, trans8, emis_match, emis_insert, emis_null, xtrans, seq, L)) return DCP_EINVAL;
    if (!nsteps_out || !gain_out || !alt_fwd_out || (cap_steps && (!steps_out || !post_out))) return DCP_EINVAL;
    MeaHost h;
    if (int rc = mea_sweeps(M, ldk, trans8, emis_match, emis_insert, emis_null, xtrans, seq, L, h)) return rc;
    dcp_mea_view<double> const v = mea_view(h, M, ldk, L, emis_match, emis_insert, emis_null);
    MeaSeq const sq{seq};
    uint64_t const n = dcp_mea_walk(v, sq, h.alt, h.start, (uint32_t *)nullptr, (double *)nullptr, 0u);
    if (n > 0xffffffffull) return DCP_EFAIL;
    *nsteps_out = (unsigned)n;
    if (n > cap_steps) return DCP_ENOMEM;
    dcp_mea_walk(v, sq, h.alt, h.start, (uint32_t *)steps_out, post_out, n);
    *gain_out = n ? h.gain : dcp_fwd_ninf();
    *alt_fwd_out = h.alt;
    return DCP_OK;
}

extern "C" int dcp_mea_path_gain(unsigned M, unsigned ldk, double const *trans8, double const *emis_match,
                                 double const *emis_insert, double const *emis_null, double const xtrans[13],
                                 unsigned char const *seq, unsigned L, struct dcp_step const *steps, unsigned nsteps,
                                 double *gain_out, double *post_out)
{
    if (!mea_inputs_ok(M, ldk, trans8, emis_match, emis_insert, emis_null, xtrans, seq, L)) return DCP_EINVAL;
    if (!steps || nsteps < 2u || !gain_out) return DCP_EINVAL;
    double const ninf = dcp_fwd_ninf();
    unsigned const EXT = 3u << 14;
    if (steps[0].state_id != (EXT | 1u) || steps[nsteps - 1u].state_id != (EXT | 7u)) return DCP_EINVAL;
    // first the integers and the edges: the graph of dcp_domains.hip's edge(), every transition and emission finite
    MeaSeq const sq{seq};
    uint64_t pos = 0;
    for (unsigned i = 0; i < nsteps; ++i)
    {
        unsigned const id = steps[i].state_id, kind = id >> 14, xx = id & 0x3fffu, len = steps[i].seqlen;
        bool const emits = kind < 2u || (kind == 3u && (xx == 2u || xx == 5u || xx == 6u));
        if (kind < 3u && (xx < 1u || xx > M)) return DCP_EINVAL;
        if (kind == 3u && (xx == 0u || xx > 7u)) return DCP_EINVAL;
        if (emits ? (len < 1u || len > 5u) : len != 0u) return DCP_EINVAL;
        if (pos + len > L) return DCP_EINVAL;
        if (i > 0u)
        {
            unsigned const pid = steps[i - 1u].state_id, pkind = pid >> 14, pk = pid & 0x3fffu, k = xx - 1u;
            unsigned const from = pkind == 3u ? pk : 100u;
            double t = ninf;
            if (kind == 0u)
            {
                if (from == 3u) t = trans8[(size_t)DCP_T_ENTRY * ldk + k];
                else if (k > 0u && pk == k && pkind < 3u) t = trans8[(size_t)(DCP_T_MM + pkind) * ldk + k];
            }
            else if (kind == 1u)
            {
                if (pk == k + 1u && pkind < 2u) t = trans8[(size_t)(DCP_T_MI + pkind) * ldk + k];
            }
            else if (kind == 2u)
            {
                if (k > 0u && pk == k && (pkind == 0u || pkind == 2u)) t = trans8[(size_t)(pkind == 0u ? DCP_T_MD : DCP_T_DD) * ldk + k];
            }
            else
            {
                int r = -1;
                switch (xx)
                {
                case 2: r = from == 1u ? DCP_X_SN : from == 2u ? DCP_X_NN : -1; break;
                case 3: r = from == 1u ? DCP_X_SB : from == 2u ? DCP_X_NB : from == 4u ? DCP_X_EB : from == 5u ? DCP_X_JB : -1; break;
                case 4: t = pkind == 0u || (pkind == 2u && pk >= 2u) ? 0.0 : ninf; break;
                case 5: r = from == 4u ? DCP_X_EJ : from == 5u ? DCP_X_JJ : -1; break;
                case 6: r = from == 4u ? DCP_X_EC : from == 6u ? DCP_X_CC : -1; break;
                case 7: r = from == 4u ? DCP_X_ET : from == 6u ? DCP_X_CT : -1; break;
                default: break;
                }
                if (r >= 0) t = xtrans[r];
            }
            if (t == ninf) return DCP_EINVAL;
        }
        if (emits)
        {
            unsigned const code = dcp_mea_code(sq, (unsigned)pos, len);
            double const e = kind == 0u ? emis_match[(size_t)code * ldk + (xx - 1u)] : kind == 1u ? emis_insert[code] : emis_null[code];
            if (e == ninf) return DCP_EINVAL;
        }
        pos += len;
    }
    if (pos != L) return DCP_EINVAL;
    MeaHost h;
    if (int rc = mea_sweeps(M, ldk, trans8, emis_match, emis_insert, emis_null, xtrans, seq, L, h)) return rc;
    // the gain from the path's end, as the sweep forms it: suffix + l w
    double g = 0.0;
    unsigned j = L;
    for (unsigned i = nsteps; i-- > 0u;)
    {
        unsigned const id = steps[i].state_id, kind = id >> 14, xx = id & 0x3fffu, l = steps[i].seqlen;
        double w = -1.0;
        if (l)
        {
            unsigned const s = j - l, code = dcp_mea_code(sq, s, l);
            if (kind == 3u)
            {
                unsigned const X = xx == 2u ? 0u : xx == 5u ? 1u : 2u;
                w = dcp_post_prob(h.fr[(size_t)DCP_POST_REC * s + X] + emis_null[code], h.br[(size_t)DCP_POST_REC * j + X], h.alt);
            }
            else
            {
                unsigned const k = xx - 1u;
                size_t const from = (size_t)s * M + k, to = (size_t)j * M + k;
                w = kind == 0u ? dcp_post_prob(h.P[from] + emis_match[(size_t)code * ldk + k], h.bM[to], h.alt)
                               : dcp_post_prob(h.Q[from] + emis_insert[code], h.bI[to], h.alt);
            }
            double const lw = (double)l * w;
            g = g + lw;
            j = s;
        }
        if (post_out) post_out[i] = w;
    }
    *gain_out = g;
    return DCP_OK;
}
