// dcp_envelopes.hip -- gfx950 kernels that turn a round's posterior rows, still in device memory, into envelope records
// (dcp_gpu_envelope_pairs; the rule is dcp_envelopes.h, which dcp_model.cpp compiles as the host twin).
//
//  envelope_kernel<WRITE>  one wavefront per pair, striding over the round's list.  The pair's bases go by in chunks of
//                          64: lane t of chunk c holds base 64 c + t.  A ballot of core >= lo is the chunk's mask, whose
//                          maximal stretches of ones are the chunk's runs; the loop over them is scalar (the mask is
//                          wave-uniform).  A run that reaches lane 63 stays open in wave-uniform state (dcp_env_run) and
//                          is continued by a run that starts at lane 0 of the next chunk, or closed there; whatever is
//                          open after the last chunk ends at L.  The state is void at every pair's start.
//    WRITE = false         the count pass: reads the core plane alone.  Whether a run has a peak is the mask of
//                          core >= hi met with the run's own bits -- no reduction at all.  count[i] = pair i's kept runs.
//    WRITE = true          the write pass: a pair without a kept run is skipped; of the others a chunk with an empty mask
//                          and no open run costs its core loads only.  Per run and chunk four masked butterfly
//                          reductions (the three sums, the maximum) over the run's own lanes, the other lanes holding
//                          0 and -inf, and one ballot for the first lane that holds the maximum.  Lane 0 stores a kept
//                          run's record at env[env_at[i] + k], k counting the pair's kept runs: list order, then begin,
//                          whichever wavefront ends first.
//
// Both passes decide "kept" by comparisons on the same values: a run of values >= lo holds no NaN, so its maximum is
// >= hi exactly when one of its values is.  The write pass still never stores past the pair's own records.
// The loads are coalesced: consecutive lanes read consecutive doubles of a plane.  Vector stores and plain C++ only.
#include "dcp_envelopes.h"

#include <hip/hip_runtime.h>

namespace
{

__device__ __forceinline__ double env_ninf() { return -__builtin_inf(); }

__device__ __forceinline__ double env_readlane(double v, int lane)
{
    unsigned long long const b = __builtin_bit_cast(unsigned long long, v);
    unsigned const lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, lane);
    unsigned const hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), lane);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// lane i and lane i ^ o combine the same two values: every lane ends with the one result
__device__ __forceinline__ double env_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
        v = v + __shfl_xor(v, o, 64);
    return env_readlane(v, 0);
}

__device__ __forceinline__ double env_wave_max(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
    {
        double const w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return env_readlane(v, 0);
}

// the bits [s, s + len) of a chunk's mask, 1 <= len <= 64
__device__ __forceinline__ unsigned long long env_bits(unsigned s, unsigned len)
{
    return (len >= 64u ? ~0ull : (1ull << len) - 1ull) << s;
}

template <bool WRITE> __global__ __launch_bounds__(256) void envelope_kernel(dcp_env_args a)
{
    unsigned const lane = threadIdx.x & 63u;
    uint64_t const gw = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    uint64_t const nw = a.nwaves;
    if (gw >= nw) return; // the grid's last block may hold wavefronts past nwaves
    uint64_t const base = a.row_off[0];
    for (uint64_t pair = gw; pair < a.nlist; pair += nw)
    {
        uint64_t at = 0, room = 0; // the pair's records: where they start, how many there are
        if constexpr (WRITE)
        {
            at = a.env_at[pair], room = a.env_at[pair + 1u] - at;
            if (room == 0u) continue;
        }
        uint64_t const first = a.row_off[pair] - base;
        unsigned const L = (unsigned)(a.row_off[pair + 1u] - a.row_off[pair] - 1u);
        double const *const core = a.core + first + 1u, *const begin = a.begin + first, *const end = a.end + first + 1u;

        // the state of the pair's open run, void at every pair's start
        bool open = false, open_peak = false; // (open_peak: the count pass's "a value >= hi so far")
        unsigned open_begin = 0;
        dcp_env_run run{};
        unsigned kept = 0;

        // the run [b, e) is complete
        auto const close = [&](unsigned e) {
            if constexpr (WRITE)
            {
                if (dcp_env_kept(run.begin, e, run.core_max, a.hi, a.min_len))
                {
                    if (lane == 0u && kept < room) a.env[at + kept] = dcp_env_record(run, a.pair_base + (unsigned)pair, e);
                    ++kept;
                }
            }
            else if (e - open_begin >= a.min_len && open_peak) ++kept;
            open = false;
        };

        for (unsigned c0 = 0; c0 < L; c0 += 64u)
        {
            unsigned const i = c0 + lane;
            bool const valid = i < L;
            double const v = valid ? core[i] : 0.0;
            unsigned long long mask = __ballot(valid && dcp_env_in(v, a.lo));
            if (open && !(mask & 1ull)) close(c0);
            if (mask == 0ull) continue;
            unsigned long long peaks = 0ull;
            double vb = 0.0, ve = 0.0;
            if constexpr (WRITE)
            {
                vb = valid ? begin[i] : 0.0;
                ve = valid ? end[i] : 0.0;
            }
            else peaks = __ballot(valid && v >= a.hi);
            while (mask)
            {
                unsigned const s = (unsigned)__builtin_ctzll(mask);
                unsigned long long const rest = ~(mask >> s); // (zeros shifted in from above end the run at lane 63)
                unsigned const len = rest ? (unsigned)__builtin_ctzll(rest) : 64u;
                unsigned long long const bits = env_bits(s, len);
                mask &= ~bits;
                if constexpr (WRITE)
                {
                    bool const mine = (bits >> lane) & 1ull;
                    double const mx = env_wave_max(mine ? v : env_ninf());
                    unsigned const pk = c0 + (unsigned)__builtin_ctzll(__ballot(mine && v == mx));
                    double const cmax = env_readlane(v, (int)(pk - c0));
                    double const cs = env_wave_sum(mine ? v : 0.0), bs = env_wave_sum(mine ? vb : 0.0),
                                 es = env_wave_sum(mine ? ve : 0.0);
                    if (open) dcp_env_run_add(run, pk, cmax, cs, bs, es); // (s == 0: a run at any other lane found it closed)
                    else run = dcp_env_run{c0 + s, pk, cmax, cs, bs, es};
                }
                else
                {
                    bool const pk = (peaks & bits) != 0ull;
                    if (open) open_peak = open_peak || pk;
                    else open_begin = c0 + s, open_peak = pk;
                }
                open = true;
                if (s + len < 64u) close(c0 + s + len);
            }
        }
        if (open) close(L); // it reached lane 63 of the last chunk: L is that chunk's end
        if constexpr (!WRITE)
            if (lane == 0u) a.count[pair] = kept;
    }
}

bool refused(dcp_env_args const *a, bool write)
{
    if (!a || a->nlist == 0u || a->nwaves == 0u || !a->row_off || !a->core) return true;
    if (write) return !a->begin || !a->end || !a->env_at || !a->env;
    return !a->count;
}

} // namespace

extern "C" int dcp_envelopes_count_launch(struct dcp_env_args const *a, void *stream)
{
    if (refused(a, false)) return 1;
    dim3 const grid((a->nwaves + 3u) / 4u), block(256);
    hipLaunchKernelGGL((envelope_kernel<false>), grid, block, 0, (hipStream_t)stream, *a);
    return 0;
}

extern "C" int dcp_envelopes_write_launch(struct dcp_env_args const *a, void *stream)
{
    if (refused(a, true)) return 1;
    dim3 const grid((a->nwaves + 3u) / 4u), block(256);
    hipLaunchKernelGGL((envelope_kernel<true>), grid, block, 0, (hipStream_t)stream, *a);
    return 0;
}
