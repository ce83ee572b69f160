// dcp_decode.hip -- protein_profile_decode / imm_frame_cond_decode on the device (dcp_gpu_decode_paths).
//
// One wavefront per emitting step, lane l = codon l = 16a + 4b + c.  The wavefront reads its work item (all lanes the
// same 16 bytes), takes the fragment's up to five bases out of two adjacent 2-bit words of the resident sequence
// (a fragment may straddle a 16-base word; a sequence of L bases has L / 16 + 3 words, so word (start >> 4) + 1
// exists), and picks the distribution as the host does: the insert dist for I, the node's match dist for M, the null
// dist for N, J, C, R.  Of that distribution it needs 68 values in the probability domain: the 4 base probabilities,
// which every lane reads (LDS, one row per wavefront), and the 64 codon probabilities, of which lane l reads only
// its own (a register).  For the null and insert dists they are the host's own exp() values stored at upload --
// those dists are flat or shared, exact ties are structural there, and only equal operands give the host's winner; a
// match step takes exp() of the resident dist here.  Each lane then evaluates frame_prob_word_of (dcp_frame_word.h:
// the source the host compiles too, this unit also with -ffp-contract=off) for "the codon is l", and the wavefront
// reduces (value, lane) to the maximum, the HIGHEST lane among equal values: what the host's `v >= best` loop over
// ascending (a, b, c) returns.  Lane 0 writes the code.
//
// Four wavefronts per block, each block walking the work list with a block-uniform stride: every wavefront of a
// block makes the same number of trips, so the two block barriers per trip (the base row is written, then read) are
// reached by all of them.
#include "dcp_decode.h"
#include "dcp_frame_word.h"

#include <hip/hip_runtime.h>

namespace
{

constexpr unsigned kWaves = 4;
constexpr unsigned kBlock = 64u * kWaves;

template <class Real> __global__ __launch_bounds__(kBlock) void decode_kernel(dcp_decode_args a)
{
    __shared__ double base_p[kWaves][4];
    unsigned const lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    unsigned const stride = gridDim.x * kWaves;
    for (unsigned i0 = blockIdx.x * kWaves; i0 < a.nitems; i0 += stride) // block-uniform bounds
    {
        unsigned const i = i0 + w;
        bool const live = i < a.nitems;
        dcp_decode_item it{0u, 0u, 0u, 1u};
        if (live) it = a.items[i];
        unsigned const len = it.sel & 7u, kind = (it.sel >> 3) & 3u, k = (it.sel >> 8) & 0xfffu;
        double pc = 0.0;
        if (live)
        {
            if (kind == DCP_DECODE_MATCH)
            {
                Real const *d = (Real const *)a.dists + ((size_t)a.match_row[it.prof] + k) * DCP_NDIST;
                unsigned const ca = lane >> 4, cb = (lane >> 2) & 3u, cc = lane & 3u;
                pc = exp((double)d[4u + ca * 25u + cb * 5u + cc]);
                if (lane < 4u) base_p[w][lane] = exp((double)d[lane]);
            }
            else
            {
                double const *x = a.exp_ni + ((size_t)it.prof * 2u + kind) * DCP_DECODE_EXP;
                pc = x[4u + lane];
                if (lane < 4u) base_p[w][lane] = x[lane];
            }
        }
        __syncthreads();
        if (live)
        {
            uint32_t const *sw = a.words + a.woff[it.seq] + (it.start >> 4);
            uint64_t const two = ((uint64_t)sw[1] << 32) | sw[0];
            uint32_t const bits = (uint32_t)(two >> (2u * (it.start & 15u))); // base j of the fragment in bits 2j
            uint8_t x[5];
            for (unsigned j = 0; j < 5u; ++j)
                x[j] = (uint8_t)((bits >> (2u * j)) & 3u);
            double const e = a.eps[it.prof], f = 1.0 - e;
            dcp_one_codon const c3{(int)(lane >> 4), (int)((lane >> 2) & 3u), (int)(lane & 3u), pc};
            double v = frame_prob_word_of(&base_p[w][0], c3, e, f, x, len);
            unsigned best = lane;
            for (unsigned m = 32u; m > 0u; m >>= 1)
            {
                double const ov = __shfl_xor(v, (int)m);
                unsigned const ol = (unsigned)__shfl_xor((int)best, (int)m);
                if (ov > v || (ov == v && ol > best)) v = ov, best = ol;
            }
            if (lane == 0u) a.codes[i] = (uint8_t)best;
        }
        __syncthreads(); // the next trip rewrites the base row
    }
}

} // namespace

extern "C" int dcp_launch_decode(dcp_decode_args const *args, int f64, void *stream)
{
    if (!args || args->nitems == 0 || args->nitems > (unsigned)DCP_DECODE_MAX_ITEMS) return (int)hipErrorInvalidValue;
    unsigned const need = (args->nitems + kWaves - 1u) / kWaves;
    // at 72 VGPRs a SIMD holds 7 wavefronts, a CU 7 blocks of 4: 8 192 blocks are more than the 256 CUs hold at once, the
    // rest of the list is the blocks' loop
    unsigned const blocks = need < 8192u ? need : 8192u;
    hipStream_t const s = (hipStream_t)stream;
    if (f64) decode_kernel<double><<<blocks, kBlock, 0, s>>>(*args);
    else decode_kernel<float><<<blocks, kBlock, 0, s>>>(*args);
    return (int)hipGetLastError();
}
