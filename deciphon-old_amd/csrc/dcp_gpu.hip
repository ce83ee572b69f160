// dcp_gpu.hip -- C-ABI of the device path (include/dcp_gpu.h): context, resident
// profile DB, resident sequence batch, scan launch, result fetch.
//
// Replaces, for the hot path only: profile_reader_* + protein_profile.unpack
// (src/db/profile_reader.c:74-168, src/model/protein_profile.c:38-117),
// imm_task_setup (src/server/scan_thread.c:51-55) and the per-pair body of
// thread_run (src/server/scan_thread.c:99-123).  No CPU fallback exists.
#include "dcp_kernels.h"
#include "dcp_f64.h"
#include "dcp_seqs.h"
#include "dcp_decode.h"
#include "dcp_domains.h"
#include "dcp_calib.h"
#include "dcp_forward.h"
#include "dcp_forward_scaled.h"
#include "dcp_backward_scaled.h"
#include "dcp_mea.h"
#include "dcp_posterior.h"
#include "dcp_envelopes.h"
#include "dcp_test_hooks.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <new>
#include <numeric>
#include <string>
#include <queue>
#include <type_traits>
#include <vector>

namespace
{

// Size classes: a profile with core_size M runs in the smallest class whose
// capacity 64*R*W holds it (R nodes per lane, W wavefronts per pair).
struct SizeClass
{
    int R, W;
    unsigned cap() const { return 64u * (unsigned)R * (unsigned)W; }
};
// One wavefront with up to 8 nodes per lane covers core sizes up to 512 (97 % of a Pfam-like DB) without
// any cross-wavefront exchange; measured on the C3 DB, R = 5..8 in one wavefront take 0.52 / 0.66 of the
// time of the two-wavefront classes R = 3, 4 they replace, while two wavefronts of 6 or 8 nodes per lane
// (two per SIMD: too few to hide the block barriers) are slower than four of 3 or 4
// (profiles/r02/rowsweep_tuning.txt).
constexpr SizeClass kClasses[] = {{1, 1}, {2, 1}, {3, 1}, {4, 1}, {5, 1}, {6, 1}, {7, 1}, {8, 1},
                                  {3, 4}, {4, 4}, {3, 8}, {4, 8}, {3, 16}, {4, 16}};
// cells/s of each class on a full grid, measured on the C3 DB (profiles/r03/rowsweep_variants.txt; round 2:
// profiles/r02/rowsweep_tuning.txt): the kernel choice prices a row-sweep scan with them
constexpr double kClassRate[] = {880e9, 930e9, 1120e9, 1250e9, 1240e9, 1320e9, 1220e9, 1230e9,
                                 830e9, 960e9, 820e9, 600e9, 600e9, 600e9}; // multi-wavefront classes: the segmented sweep (round 4: profiles/r04/rowsweep_multiwave.txt)
constexpr int kNumClasses = (int)(sizeof kClasses / sizeof kClasses[0]);
static_assert(sizeof kClassRate / sizeof kClassRate[0] == sizeof kClasses / sizeof kClasses[0], "one rate per class");
static_assert(kNumClasses <= DCP_MAX_CLASSES, "redo lists are sized for DCP_MAX_CLASSES size classes");

// profiles per wavefront of the two smallest classes in grid mode (viterbi_mp_kernel<K>: 64 / K lanes x 4 nodes each)
constexpr unsigned kMpParts[2] = {4u, 2u};
constexpr unsigned kMpClass1MaxQueries = 96u; // the 65 .. 128-node class runs two profiles per wavefront below this many queries

int class_of(unsigned M)
{
    for (int c = 0; c < kNumClasses; ++c)
        if (M <= kClasses[c].cap()) return c;
    return -1;
}

// Nodes per lane of the segments a profile of more than 512 nodes is cut into by the segmented row sweep
// (viterbi_segment_kernel): the fewest segments of at most 512 nodes, and the narrowest lanes that cover the profile
// with them -- R = ceil(M / (64 x ceil(M / 512))), 5..8 -- so that a segment's lanes are at least 80 % full (with a
// fixed 384 / 512 nodes per class they were 67 .. 100 %).  0: a one-wavefront profile.
unsigned seg_r_of(unsigned M)
{
    if (M <= 512u) return 0u;
    unsigned const nseg = (M + 511u) / 512u;
    return (M + 64u * nseg - 1u) / (64u * nseg);
}

template <class T> struct DevBuf
{
    T *p = nullptr;
    size_t n = 0;
    hipError_t alloc(size_t count)
    {
        release();
        if (count == 0) return hipSuccess;
        hipError_t e = hipMalloc((void **)&p, count * sizeof(T));
        if (e == hipSuccess) n = count;
        else p = nullptr;
        return e;
    }
    // room for at least `count`: a buffer kept between calls grows, and never shrinks
    hipError_t reserve(size_t count) { return n < count ? alloc(count) : hipSuccess; }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    ~DevBuf() { release(); }
};

// What a scan leaves on the device, in the DB's precision: the dense scores (keep_scores) and the hit list with its
// counter -- the context's own, or a caller-owned buffer (e.g. a torch tensor that RCCL gathers).
template <class Real, class Hit> struct ScanResults
{
    DevBuf<Real> d_null, d_alt;
    DevBuf<Hit> d_hits;
    DevBuf<unsigned> d_nhits;
    unsigned hit_cap = 0;
    bool have_scores = false;
    Hit *ext_hits = nullptr;
    unsigned *ext_nhits = nullptr;
    unsigned ext_cap = 0;
    Hit *hits() const { return ext_hits ? ext_hits : d_hits.p; }
    unsigned *nhits() const { return ext_hits ? ext_nhits : d_nhits.p; }
    unsigned cap() const { return ext_hits ? ext_cap : hit_cap; }
    hipError_t ensure(size_t npairs, bool keep_scores)
    {
        hipError_t e = hipSuccess;
        if (keep_scores && d_null.n != npairs)
        {
            if ((e = d_null.alloc(npairs)) != hipSuccess) return e;
            if ((e = d_alt.alloc(npairs)) != hipSuccess) return e;
        }
        have_scores = keep_scores;
        unsigned const want_cap = (unsigned)std::min<size_t>(npairs, (size_t)1 << 22);
        if (!ext_hits && hit_cap < want_cap)
        {
            if ((e = d_hits.alloc(want_cap)) != hipSuccess) return e;
            hit_cap = want_cap;
        }
        return d_nhits.p ? hipSuccess : d_nhits.alloc(1);
    }
    void release()
    {
        d_null.release(), d_alt.release(), d_hits.release(), d_nhits.release();
        hit_cap = 0;
        have_scores = false;
    }
};

// This file is built with -fno-honor-nans: a NaN is found by its encoding, not by v != v.
bool is_nan(float v)
{
    uint32_t bits;
    std::memcpy(&bits, &v, sizeof bits);
    return (bits & 0x7fffffffu) > 0x7f800000u;
}
bool is_nan(double v)
{
    uint64_t bits;
    std::memcpy(&bits, &v, sizeof bits);
    return (bits & 0x7fffffffffffffffull) > 0x7ff0000000000000ull;
}

constexpr int kMaxLaunches = 2 * kNumClasses + 1; // a segmented class is two launches

// What the last scan was, and what of it has not been looked at yet: every default means "no scan".  The four scan
// drivers (dcp_gpu_scan_range with its launch functions, scan64, dcp_gpu_scan_pairs, scan_pairs64) each begin with a
// fresh record -- once the call's refusals are past and the scan before it is complete -- and fill in what they know,
// `scanned` last: a scan that fails on the way leaves "no scan".  finish_scan settles the pending flags; a new DB or a
// new batch puts the empty record back (void_last_scan).  Nothing else writes a member: Forward, posterior, traceback,
// decode and domains do not mention it.
struct LastScan
{
    bool scanned = false;
    bool f64 = false;       // it ran on a double DB: its results are the context's f64 ones
    bool pair_scan = false; // dcp_gpu_scan_pairs: the accounting is that of the list, not of a range x the whole DB
    unsigned q0 = 0, q1 = 0;
    int kernel = 0;         // 1 row sweep, 2 query lane
    int kernel_variant = 0; // as dcp_scan_params.kernel names it: 1, 2, 3 (two-stage query lane) or 4 (f64 query lane)
    struct dcp_scan_params prm = {};
    unsigned launches = 0;
    // the float kernels' launches, one HIP event (ev_class) behind each; the f64 kernels keep no such records
    unsigned n_launched = 0;
    int launched_class[kMaxLaunches] = {0};      // -1: the query-lane launch
    bool launched_redo[kMaxLaunches] = {false}; // the exact kernel behind a segmented sweep: its cells are counted there
    bool overlapped = false; // the row sweep's class launches ran side by side on their own streams
    unsigned redo_pairs = 0;
    // a pair list's cells and bytes, and (a float DB's) their parts per size class
    uint64_t pair_cells = 0, pair_bytes = 0;
    uint64_t pair_class_cells[DCP_MAX_CLASSES] = {0}, pair_class_bytes[DCP_MAX_CLASSES] = {0};
    // not looked at yet: the redo counters of a float / an f64 query-lane scan, a two-stage scan's error word
    bool redo_pending = false, redo_pending64 = false, ring_check_pending = false;
#ifdef DCP_TEST_HOOKS
    // test hook (dcp_gpu_test_last_rowsweep_plan): what launch_rowsweep_scan did with each size class
    struct RowsweepClassPlan
    {
        unsigned path = 0;         // DCP_RS_PATH_*: 0 = the class is empty
        unsigned stage = 0, waves = 0, prefetch = 0; // plain grid: rowsweep_variant's answer
        unsigned chunk = 0;        // segmented: queries per pass
        unsigned flagged_rest = 0; // K profiles per wavefront: the flagged profiles got a launch of their own
    } rs_plan[kNumClasses];
    // test hook (dcp_gpu_test_last_pair_launches): the pair-mode launches, in launch order
    struct PairLaunch
    {
        unsigned kind, precision, a, b, units, tpb, cap;
    };
    std::vector<PairLaunch> pair_launches;
#endif
};

} // namespace

struct dcp_gpu_ctx
{
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    std::string err;

    // resident DB
    unsigned nprof = 0;
    std::vector<dcp_prof_meta> metas;   // sorted by class
    std::vector<unsigned> core_sizes;   // by pidx
    unsigned class_first[kNumClasses + 1] = {0};
    DevBuf<dcp_prof_meta> d_metas;
    DevBuf<uint32_t> d_slot_of_pidx;
    std::vector<uint32_t> slot_of_pidx;
    DevBuf<float> d_emis_match, d_emis_insert, d_emis_null, d_trans8;
    // the row-sweep layout of the match tables (d_emis_match) is expanded on first use: the
    // throughput path only needs the tile images, and both together double the DB's footprint
    DevBuf<float> d_dists, d_eps;
    std::vector<dcp_expand_tile> rs_tiles;
    uint64_t rs_floats = 0;
    bool rs_ready = false;
    // DCP_DB_ONE_LAYOUT: no tile images; the query-lane kernels gather a tile's LDS image from d_emis_match (always resident)
    bool one_layout = false;
    uint64_t table_bytes = 0; // expanded match tables resident after the upload (either or both layouts)
    // query-lane kernel layout (dcp_qlane.hip)
    int ql_G = 2; // nodes per tile = 4 * G (KT = 8: the tile transitions fit in SGPRs)
    std::vector<dcp_ql_prof> ql_metas; // same order as metas
    uint64_t sum_core = 0, sum_tiles = 0; // over the resident DB (kernel choice)
    uint64_t class_core[DCP_MAX_CLASSES] = {0}; // sum of core sizes per row-sweep size class
    unsigned max_tiles = 0;
    DevBuf<dcp_ql_prof> d_ql_metas;
    DevBuf<float> d_emis_tiles, d_ttrans, d_scratch;
    DevBuf<uint32_t> d_qorder;
    DevBuf<uint32_t> d_words_t, d_wt_off; // query-lane kernel: per-block window planes
    // profiles of at most 128 nodes: groups of K sharing table rows (dcp_mp_group), per row-sweep class 0 / 1
    std::vector<dcp_mp_group> mp_groups;
    unsigned mp_first[3] = {0, 0, 0};        // groups of class 0: [mp_first[0], mp_first[1]), class 1: [mp_first[1], mp_first[2])
    unsigned mp_flagged_first[2] = {0, 0};   // first flagged (ungrouped) profile of class 0 / 1 in metas order
    DevBuf<dcp_mp_group> d_mp_groups;
    DevBuf<float> d_mp_in;                   // [group][1364][K] {eI, eN}
    bool mp_in_ready = false;
    DevBuf<dcp_ql_group> d_ql_groups;     // groups of up to 64 queries and the wavefront slots they are packed into
    DevBuf<uint32_t> d_slot_first;
    unsigned ql_nqb = 0, ql_plane_rows = 0; // the cached plan: blocks of slots, rows of a block's scratch planes
    unsigned ring_stall = 0;                // test hook: dcp_qlane_args::ring_stall
    // the length-sorted query order and the plane offsets travel through pinned host memory: the copies are
    // truly asynchronous and dcp_gpu_scan_range returns without waiting for the stream
    uint32_t *h_qstage = nullptr;
    size_t h_qstage_n = 0;
    hipEvent_t ev_qstage = nullptr;       // recorded behind the copies: the buffer may be rewritten after it
    int rs_force_stg = -1;                // test hook: row-sweep variant (rows staged, wavefronts per block)
    unsigned rs_force_bw = 0;
    unsigned rs_pad_lds = 0;
    int rs_force_pf = 0;
    int rs_force_R = 0; // 0: every class
    bool any_exact_e = false;             // some profile has a positive MD / DD (dcp_ql_prof::needs_exact_e)
    DevBuf<unsigned> d_task_counter;
    // redo lists of the query-lane kernel (pairs handed to the row sweep), one per size class;
    // d_redo_n = [DCP_MAX_CLASSES counters][overflow flag][ring hand-shake error word]
    DevBuf<dcp_pair> d_redo;
    DevBuf<unsigned> d_redo_n;
    unsigned qorder_q0 = ~0u, qorder_q1 = ~0u, qorder_lmax = 0;
    unsigned num_cus = 0;
    unsigned qorder_nt = 0;         // block size the cached query order / transposed words were built for
    unsigned redo_cap_limit = 1u << 26; // only the -DDCP_TEST_HOOKS build can change it
    float last_ql_ms = 0;

    // resident sequences
    unsigned nseqs = 0;
    unsigned strands = 0; // 0 no batch, 1 as uploaded, 2 after dcp_gpu_seqs_add_revcomp: [nseqs / 2, nseqs) is the reverse strand
    uint64_t total_len = 0;
    std::vector<uint32_t> seq_len;
    // dcp_gpu_seqs_cut_windows: the rule in force (0 / 0: the batch is as uploaded) and the map of its windows, window ->
    // (source index in the uploaded batch, offset); after dcp_gpu_seqs_add_revcomp still the forward half's entries
    unsigned win_window = 0, win_step = 0;
    std::vector<uint32_t> win_src, win_off;
    // dcp_gpu_seqs_cut_regions: the map of the resident regions, region -> (source index in the uploaded batch, first
    // base there, strand); empty unless the batch is one of regions
    std::vector<uint32_t> reg_src, reg_begin;
    std::vector<uint8_t> reg_minus;
    void drop_windows() // a batch as uploaded: neither windows nor regions
    {
        win_window = win_step = 0;
        win_src.clear(), win_off.clear();
        reg_src.clear(), reg_begin.clear(), reg_minus.clear();
    }
    DevBuf<uint32_t> d_seq_words, d_seq_woff, d_seq_len;
    DevBuf<float> d_xtrans;
    int xt_multi = -1, xt_h3 = -1;
    bool xt_explicit = false; // dcp_gpu_seqs_set_xtrans: the caller's transitions, not the length-derived ones
    // dcp_gpu_seqs_set_xtrans64: the caller's transitions in double, [nseqs][13] on the host (the scans and traces of a
    // double DB copy the rows of their queries / hits from here); empty while the derived ones hold
    std::vector<double> xt64;

    // results
    ScanResults<float, dcp_hit> res;
    LastScan last;
    // dcp_gpu_scan_pairs: the float DB's lists, one per size class back to back, and their lengths
    DevBuf<dcp_pair> d_pair_list;
    DevBuf<unsigned> d_pair_n; // [DCP_MAX_CLASSES]
    // one HIP event after each size-class launch of the last scan
    hipEvent_t ev_class[kMaxLaunches] = {nullptr};
    // small row-sweep scans (the reference's one-sequence-at-a-time mode) are bound by the latency
    // of one pair's row chain, not by throughput: their size-class launches run side by side
    hipStream_t class_stream[kNumClasses] = {nullptr};
    hipEvent_t ev_trace[kNumClasses + 1] = {nullptr}; // traceback: the fork point and one event per class's forward launch
    // segmented sweep of the multi-wavefront classes (grid mode): per-class scratch columns and redo lists
    DevBuf<float> d_trace_work;   // the traceback's work areas (kept between calls, grows to the largest round): floats, or
                                  // the double traceback's values in the same bytes (one work area per context)
    int trace_mode = 0;            // test hook: 1 = the trace kernel's own forward loop instead of the row sweep's
    uint64_t trace_budget = 0;     // test hook: 4-byte units of work area per round of launches (0 = 2^31: 8 GiB)
    DevBuf<float> d_seg_scratch;
    DevBuf<dcp_pair> d_seg_redo;
    DevBuf<unsigned> d_seg_redo_n; // [DCP_MAX_CLASSES]
    int seg_mode = -1;             // test hook: 0 never, 1 always where a kernel exists, -1 automatic
    int mp_mode = -1;              // test hook: 0 never K profiles per wavefront, 1 always, -1 automatic
    uint64_t seg_col_bytes = (uint64_t)6 << 30; // cap on one class's boundary columns (test hook: shrink it to reach the chunked path)

    // The resident DB is float (dcp_gpu_db_upload) or double (dcp_gpu_db_upload64): 32 / 64, 0 while none is.
    int precision = 0;
    double lrt_threshold64 = std::numeric_limits<double>::quiet_NaN(); // NaN: the scan's float threshold
    struct F64Db
    {
        std::vector<dcp_f64_prof> profs;   // by launch group (kF64Groups), then by caller index
        std::vector<uint32_t> slot_of_pidx; // the entry of profs of each caller's profile index
        unsigned group_first[5] = {0, 0, 0, 0, 0};
        DevBuf<dcp_f64_prof> d_profs;
        DevBuf<double> d_tab, d_trans, d_xe; // match tables, trans8 rows, insert + null tables
        DevBuf<double> d_xt, d_col;
        ScanResults<double, dcp_hit64> res;
        // the query-lane kernel (dcp_f64_qlane.hip): profiles by falling core size, the scan's queries by rising
        // length and their batch plan (group records, slot table), the resident blocks' boundary planes, the task
        // counter, the redo lists of the four launch groups and their counters ([4] pairs, [1] overflow flag); kept
        // between scans
        DevBuf<uint32_t> d_order, d_qorder, d_slot_first;
        DevBuf<dcp_ql_group> d_groups;
        // the plan of the last kernel-4 scan (dcp_gpu_last_scan_query_plan)
        unsigned plan_blocks = 0, plan_rows = 0, plan_max_groups = 0;
        uint64_t plan_sum_rows = 0;
        DevBuf<double> d_planes;
        DevBuf<unsigned> d_task, d_redo_n;
        DevBuf<dcp_f64_pair> d_redo;
        DevBuf<dcp_f64_pair> d_pair_list; // dcp_gpu_scan_pairs: one list per launch group back to back, their lengths
        DevBuf<unsigned> d_pair_n;        // [4]
        void release()
        {
            d_pair_list.release(), d_pair_n.release();
            profs.clear();
            d_profs.release(), d_tab.release(), d_trans.release(), d_xe.release();
            d_xt.release(), d_col.release(), res.release();
            d_order.release(), d_qorder.release(), d_planes.release(), d_task.release(), d_redo_n.release();
            d_redo.release(), d_slot_first.release(), d_groups.release();
            slot_of_pidx.clear();
        }
    } f64;

    // The decode of paths (dcp_gpu_decode_paths, dcp_decode.hip).  keep_dists: dcp_gpu_db_keep_dists -- uploads keep the
    // compact dists also where they would release them.  What the resident DB holds for it: the dists themselves
    // (a float DB's are d_dists above, a double DB's d_dists64 here), each profile's first match row in them, the
    // host's exp() of its null and insert dists ([2][68] doubles) and its epsilon in double, all by caller index.
    bool keep_dists = false;
    struct DecodeDb
    {
        bool ready = false;
        DevBuf<double> d_dists64;
        DevBuf<uint32_t> d_match_row;
        DevBuf<double> d_exp, d_eps;
        void release()
        {
            ready = false;
            d_dists64.release(), d_match_row.release(), d_exp.release(), d_eps.release();
        }
    } dec;
    DevBuf<dcp_decode_item> d_dec_items; // one round's work list and codes (kept between calls)
    DevBuf<uint8_t> d_dec_codes;
    // dcp_gpu_path_domains (dcp_domains.hip): the call's steps, its path records, its special transitions (a double
    // DB: one row per path), the domain records, and core / null / total sums with the error word in one buffer of
    // 8-byte units; kept between calls, grown when a call needs more.  ev_dom: around the kernel of the last call.
    DevBuf<dcp_step> d_dom_steps;
    DevBuf<dcp_dom_path> d_dom_paths;
    DevBuf<double> d_dom_xt, d_dom_sums;
    DevBuf<uint32_t> d_dom_recs;
    hipEvent_t ev_dom[2] = {nullptr, nullptr};
    bool dom_timed = false;
    // calibration (dcp_calib.hip): the last fit's mu [nprof], lambda [nprof] and status bytes on the device (kept between
    // calls), and events around the last random_words_kernel ([0], [1]) and the last gumbel_fit_kernel ([2], [3])
    DevBuf<double> d_fit;
    DevBuf<uint8_t> d_fit_status;
    hipEvent_t ev_calib[4] = {nullptr, nullptr, nullptr, nullptr};
    bool calib_timed[2] = {false, false};
    // the tail fit: tau [nprof] and k_eff [nprof] of the last selection (mu, lambda and status go through d_fit and
    // d_fit_status), and events around the last tail_select_kernel ([0], [1]) and gumbel_fit_tail_kernel ([2], [3])
    DevBuf<double> d_tail_tau;
    DevBuf<uint32_t> d_tail_keff;
    hipEvent_t ev_tail[4] = {nullptr, nullptr, nullptr, nullptr};
    bool tail_timed = false;
    // the exponential tail fit (dcp_gpu_fit_exp_tail) goes through the same four buffers; its own events around its
    // tail_select_kernel ([0], [1]) and its exp_tail_fit_kernel ([2], [3])
    hipEvent_t ev_exp[4] = {nullptr, nullptr, nullptr, nullptr};
    bool exp_timed = false;
    // The pair-list sweeps (dcp_gpu_forward_pairs, dcp_gpu_posterior_pairs, dcp_gpu_mea_pairs; dcp_forward.hip,
    // dcp_posterior.hip, dcp_mea.hip).  The three calls are synchronous and share one workspace, kept between calls and
    // grown when a call needs more; nothing of a scan's is written, and a call reads nothing an earlier call left but
    // the profile table:
    //  d_profs   the resident DB's profiles as the kernels address them, by caller index (built on first use, void
    //            with the DB)
    //  d_xt      the call's special transitions (xt: on the host, until the call's first synchronise)
    //  d_pairs   a round's pairs bucketed by class, then the same in list order
    //  d_off     the list's row offsets, then (mea) its cell offsets
    //  d_score   [the list] null, alt by Forward, alt by Backward, gain: as far as the call goes
    //  d_rec     a round's row records of the two sweeps;  d_work: the wide sweeps' work areas
    //  d_rows    posterior's three output rows of a round
    //  mea's own: a round's matrices (P, Q, bM, bI), cell and row choices, S's choices, where each pair's steps go, how
    //            many fit and how many there are, the steps and their posteriors, the max-plus sweep's work areas
    // ev: around the launches of the round in flight.  waves_cap, post_budget, mea_budget: the hooks build's cap on a
    // launch's wavefronts (0: none) and bounds on a round's bytes (0: 1 GiB of row records; 8 GiB of matrices, choices and
    // records).  fwd_ms, post_ms, mea_ms: the kernel time of the last call of each kind, summed over its rounds.
    // The dense Forward scan (dcp_gpu_forward_dense) runs the same sweeps over every sequence x every profile, its lists
    // written on the device into d_pairs, and keeps what no pair-list call touches:
    //  d_dense   [2][nseqs x nprof] null, alt in the scan's dense layout, valid (dense_valid) until the DB, the batch or
    //            the explicit transitions change (void_forward_dense)
    //  d_order   the sequences by falling length, then the profiles by class
    // dense_round: the hooks build's bound on a round's pairs (0: kDenseRound); dense_ms: the last call's launches.
    // The scaled sweeps (dcp_gpu_forward_pairs_scaled, dcp_gpu_forward_dense_scaled; dcp_forward_scaled.hip) add:
    //  d_redo    the pairs a round's scaled launches could not sweep, appended on the device;  d_nredo: how many
    //  d_redo_pairs  the same bucketed by class for the log-space kernels
    // band: the hooks build's band of the rescaling rule (0: DCP_FWS_BAND); scaled_ms, scaled_redo: the last scaled
    // pair-list call's launches, the last scaled call's rerun pairs; dense_scaled: which sweep filled d_dense.
    // post_scaled_ms, post_scaled_redo: the same of the last dcp_gpu_posterior_pairs_scaled, summed over its rounds.
    // The envelope call (dcp_gpu_envelope_pairs; dcp_envelopes.hip) reads a round's d_rows on the device and adds:
    //  d_env_count  a round's envelopes per pair, as its count pass leaves them
    //  d_env_at     their exclusive scan, formed on the host;  d_env: the round's records
    // ev_env: around each of the two envelope passes.  env_ms: the last call's launches, summed over its rounds;
    // env_own_ms: the envelope kernels' own part of it.
    struct PairSweeps
    {
        DevBuf<uint32_t> d_env_count;
        DevBuf<uint64_t> d_env_at;
        DevBuf<dcp_envelope> d_env;
        hipEvent_t ev_env[2] = {nullptr, nullptr};
        float env_ms = -1.0f, env_own_ms = -1.0f;
        DevBuf<dcp_fwd_pair> d_redo, d_redo_pairs;
        DevBuf<uint32_t> d_nredo;
        int band = 0;
        float scaled_ms = -1.0f;
        unsigned scaled_redo = 0;
        float post_scaled_ms = -1.0f;
        unsigned post_scaled_redo = 0;
        bool dense_scaled = false;
        DevBuf<double> d_dense;
        DevBuf<uint32_t> d_order;
        bool dense_valid = false;
        unsigned dense_round = 0;
        float dense_ms = -1.0f;
        bool profs_ready = false;
        DevBuf<dcp_fwd_prof> d_profs;
        DevBuf<dcp_fwd_pair> d_pairs;
        DevBuf<uint64_t> d_off, d_step_idx;
        DevBuf<double> d_xt, d_score, d_rec, d_work, d_rows, d_mat, d_mea_work, d_post;
        std::vector<double> xt;
        DevBuf<uint16_t> d_cell;
        DevBuf<uint32_t> d_rowc, d_start, d_steps;
        hipEvent_t ev[2] = {nullptr, nullptr};
        unsigned waves_cap = 0;
        uint64_t post_budget = 0, mea_budget = 0;
        float fwd_ms = -1.0f, post_ms = -1.0f, mea_ms = -1.0f;
        void release() // a new DB
        {
            profs_ready = false;
            d_profs.release();
        }
    } sweeps;

    int fail(int rc, char const *fmt, ...)
    {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
        fprintf(stderr, "dcp_gpu: %s\n", buf);
        return rc;
    }
};

#define HIP_TRY(ctx, call)                                                     \
    do                                                                         \
    {                                                                          \
        hipError_t e_ = (call);                                                \
        if (e_ != hipSuccess)                                                  \
            return (ctx)->fail(e_ == hipErrorOutOfMemory ? DCP_ENOMEM : DCP_EFAIL, \
                               "%s: %s", #call, hipGetErrorString(e_));        \
    } while (0)

// The dense Forward matrices are void: whatever they were computed from has changed (the buffer stays for the next call).
static void void_forward_dense(dcp_gpu_ctx *c) { c->sweeps.dense_valid = false; }

// A new DB or a new batch: the last scan is void, and so is whatever of it has not been looked at yet; and so are the
// dense Forward matrices.
static void void_last_scan(dcp_gpu_ctx *c)
{
    c->last = LastScan{};
    void_forward_dense(c);
}

// What the float and the double path share (templates: outside the extern "C" block)
extern "C" { static int finish_scan(dcp_gpu_ctx *c); } // defined behind dcp_gpu_scan_range

namespace
{

// the size class / launch group k whose DB slots [first[k], first[k + 1]) hold `slot`
int range_of(unsigned const *first, int n, unsigned slot)
{
    int k = 0;
    while (k + 1 < n && slot >= first[k + 1])
        ++k;
    return k;
}

// A stable counting sort of n items into nclasses classes.  first[k] .. first[k + 1] are then the places of the items of
// class k = class_of(item), in the order they came in (first: [nclasses + 1]); returns the item at each place.
template <class ClassOf> std::vector<unsigned> sort_into_classes(unsigned n, int nclasses, unsigned *first, ClassOf class_of)
{
    std::fill(first, first + nclasses + 1, 0u);
    for (unsigned i = 0; i < n; ++i)
        ++first[class_of(i) + 1];
    for (int k = 0; k < nclasses; ++k)
        first[k + 1] += first[k];
    std::vector<unsigned> at(first, first + nclasses), order(n);
    for (unsigned i = 0; i < n; ++i)
        order[at[class_of(i)]++] = i;
    return order;
}

// A list that runs in rounds of consecutive pairs: the end of the round that begins at pair i0, the furthest i1 with
// bytes_of(i0, i1) within the budget.  A single pair that exceeds it gets a round of its own.
template <class BytesOf> unsigned round_end(unsigned i0, unsigned npairs, uint64_t budget, BytesOf bytes_of)
{
    unsigned i1 = i0 + 1u;
    while (i1 < npairs && bytes_of(i0, i1 + 1u) <= budget)
        ++i1;
    return i1;
}

template <class Real> int fetch_table_rows(dcp_gpu_ctx *c, Real const *src, unsigned ldk, unsigned core_size, Real *out)
{
    // rows of (possibly shared) length ldk from the profile's first column to its last row's last node
    std::vector<Real> tab((size_t)(DCP_NCODES - 1) * ldk + core_size);
    HIP_TRY(c, hipMemcpy(tab.data(), src, tab.size() * sizeof(Real), hipMemcpyDeviceToHost));
    for (unsigned code = 0; code < DCP_NCODES; ++code)
        std::memcpy(out + (size_t)code * core_size, &tab[(size_t)code * ldk], sizeof(Real) * core_size);
    return DCP_OK;
}

int xtrans_of_length(unsigned L, int multi_hits, int hmmer3_compat, float *out) { return dcp_xtrans(L, multi_hits, hmmer3_compat, out); }
int xtrans_of_length(unsigned L, int multi_hits, int hmmer3_compat, double *out) { return dcp_xtrans64(L, multi_hits, hmmer3_compat, out); }

// protein_profile_setup once per sequence length instead of once per pair: row i of xt ([seqs.size()][stride], the tail
// of a row zero) gets the special transitions of the resident sequence seqs[i].  In double the caller's own rows
// (dcp_gpu_seqs_set_xtrans64) are copied instead while they hold: the flags are then ignored.
template <class Real>
int fill_xtrans(dcp_gpu_ctx *c, std::vector<uint32_t> const &seqs, int multi_hits, int hmmer3_compat, unsigned stride,
                std::vector<Real> &xt)
{
    bool const given = std::is_same<Real, double>::value && !c->xt64.empty();
    xt.assign(seqs.size() * stride, Real(0));
    std::map<uint32_t, size_t> row_of_len;
    for (size_t i = 0; i < seqs.size(); ++i)
    {
        Real *const row = &xt[i * stride];
        if (given)
        {
            std::memcpy(row, &c->xt64[(size_t)seqs[i] * DCP_NXTRANS], sizeof(double) * DCP_NXTRANS);
            continue;
        }
        uint32_t const L = c->seq_len[seqs[i]];
        auto const it = row_of_len.find(L);
        if (it != row_of_len.end())
        {
            std::memcpy(row, &xt[it->second * stride], sizeof(Real) * DCP_NXTRANS);
            continue;
        }
        if (int rc = xtrans_of_length(L, multi_hits, hmmer3_compat, row)) return c->fail(rc, "sequence cannot be empty");
        row_of_len.emplace(L, i);
    }
    return DCP_OK;
}

// dcp_gpu_fetch_scores[64] / dcp_gpu_fetch_hits[64] once the last scan is known to be of the precision asked for
template <class Real, class Hit> int fetch_scores(dcp_gpu_ctx *c, ScanResults<Real, Hit> const &r, Real *null_out, Real *alt_out)
{
    if (!c->last.scanned || !r.have_scores) return c->fail(DCP_EINVAL, "no dense scores kept by the last scan");
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = finish_scan(c)) return rc;
    size_t const bytes = (size_t)c->nseqs * c->nprof * sizeof(Real);
    if (null_out) HIP_TRY(c, hipMemcpy(null_out, r.d_null.p, bytes, hipMemcpyDeviceToHost));
    if (alt_out) HIP_TRY(c, hipMemcpy(alt_out, r.d_alt.p, bytes, hipMemcpyDeviceToHost));
    return DCP_OK;
}

template <class Real, class Hit> int fetch_hits(dcp_gpu_ctx *c, ScanResults<Real, Hit> const &r, Hit *hits, unsigned cap, unsigned *nhits)
{
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = finish_scan(c)) return rc;
    unsigned n = 0;
    HIP_TRY(c, hipMemcpy(&n, r.nhits(), sizeof n, hipMemcpyDeviceToHost));
    *nhits = n;
    if (n > r.cap()) return c->fail(DCP_ENOMEM, "device hit buffer overflow: %u > %u", n, r.cap());
    if (n > cap || (n && !hits)) return DCP_ENOMEM;
    if (n == 0) return DCP_OK;
    HIP_TRY(c, hipMemcpy(hits, r.hits(), (size_t)n * sizeof(Hit), hipMemcpyDeviceToHost));
    std::sort(hits, hits + n, [](Hit const &x, Hit const &y) {
        return x.seq_idx != y.seq_idx ? x.seq_idx < y.seq_idx : x.profile_idx < y.profile_idx;
    });
    return DCP_OK;
}

// dcp_gpu_set_hit_buffer[64]: the registration of one precision's results; the scans of a DB of that precision use it
template <class Real, class Hit>
int set_hit_buffer(dcp_gpu_ctx *c, ScanResults<Real, Hit> &r, void *hits_dev, unsigned cap, void *nhits_dev)
{
    if ((hits_dev == nullptr) != (nhits_dev == nullptr) || (hits_dev && cap == 0))
        return c->fail(DCP_EINVAL, "hit buffer and counter must be given together");
    r.ext_hits = (Hit *)hits_dev;
    r.ext_nhits = (unsigned *)nhits_dev;
    r.ext_cap = hits_dev ? cap : 0;
    return DCP_OK;
}

template <class Real, class Hit>
int hit_buffer(ScanResults<Real, Hit> const &r, void **hits_dev, void **nhits_dev, unsigned *cap)
{
    *hits_dev = r.hits();
    *nhits_dev = r.nhits();
    *cap = r.cap();
    return DCP_OK;
}

static_assert((uint32_t)DCP_F64_TRACE_NO_PATH == (uint32_t)DCP_TRACE_NO_PATH && (uint32_t)DCP_F64_TRACE_TOO_LONG == (uint32_t)DCP_TRACE_TOO_LONG,
              "the walks of both precisions report a missing and an overlong path alike");

// One round of a traceback: n hits in launch order and the device buffers that the kernels of either precision share.
template <class Real> struct TraceRound
{
    unsigned n = 0;
    std::vector<unsigned> ord, first; // [n] the caller's index of each hit; [classes + 1] where each launch class starts
    Real *work = nullptr;             // the context's work area
    DevBuf<uint64_t> woff;            // [n] each hit's part of it, in values
    DevBuf<Real> alt;                 // [n]
    DevBuf<uint32_t> soff, nsteps;    // [n + 1] each hit's part of steps; [n] its steps, or DCP_TRACE_NO_PATH / _TOO_LONG
    DevBuf<dcp_step> steps;
};

// The traceback of both precisions around its launches.  Per hit h: need[h] values of work area, cap[h] steps of
// capacity (an estimate -- the walk counts past it, and a hit whose path is longer is traced once more at its exact
// count) and its launch class cls[h].  The hits are cut into rounds of at most `budget` values of work area and 2^32 - 1
// steps; round(TraceRound) uploads what only its precision needs and enqueues forward pass and walk on the context
// stream.  `model` names the path in the "no finite path" error.
template <class Hit, class Real, class Round>
int trace_rounds(dcp_gpu_ctx *c, Hit const *hits, unsigned nhits, std::vector<uint64_t> const &need, std::vector<uint32_t> &cap,
                 std::vector<int> const &cls, int nclasses, bool sort_by_class, uint64_t budget, char const *model,
                 struct dcp_step *steps_out, unsigned cap_steps, uint32_t *step_off, Real *alt_out, Round round)
{
    int rc = DCP_OK;
    std::vector<std::vector<dcp_step>> got(nhits);
    std::vector<unsigned> todo(nhits);
    std::iota(todo.begin(), todo.end(), 0u);
    for (int pass = 0; !todo.empty(); ++pass)
    {
        std::vector<unsigned> again; // hits whose paths exceeded their capacity
        for (size_t t0 = 0; t0 < todo.size();)
        {
            size_t t1 = t0;
            uint64_t work = 0, scap = 0;
            while (t1 < todo.size() &&
                   (t1 == t0 || (work + need[todo[t1]] <= budget && scap + cap[todo[t1]] <= UINT32_MAX)))
                work += need[todo[t1]], scap += cap[todo[t1]], ++t1;
            unsigned const n = (unsigned)(t1 - t0);
            TraceRound<Real> r;
            r.n = n;
            // this round's hits in launch-class order (the forward launches take contiguous pair lists); results go back
            // to the caller's order on the host
            std::vector<unsigned> &ord = r.ord, &first = r.first;
            ord.assign(todo.begin() + t0, todo.begin() + t1);
            if (sort_by_class) std::stable_sort(ord.begin(), ord.end(), [&](unsigned x, unsigned y) { return cls[x] < cls[y]; });
            std::vector<uint64_t> woff(n);
            std::vector<uint32_t> soff(n + 1, 0);
            first.assign(nclasses + 1, 0u);
            uint64_t acc = 0;
            for (unsigned i = 0; i < n; ++i)
            {
                unsigned const h = ord[i];
                woff[i] = acc;
                acc += need[h];
                soff[i + 1] = soff[i] + cap[h];
                first[cls[h] + 1] = i + 1u;
            }
            for (int k = 1; k <= nclasses; ++k)
                if (first[k] < first[k - 1]) first[k] = first[k - 1];
            // one work area per context, kept between calls: floats, or the double traceback's values in the same bytes
            size_t const work_floats = (size_t)(work * (sizeof(Real) / sizeof(float)));
            HIP_TRY(c, c->d_trace_work.reserve(work_floats));
            r.work = reinterpret_cast<Real *>(c->d_trace_work.p);
            HIP_TRY(c, r.alt.alloc(n));
            HIP_TRY(c, r.woff.alloc(n));
            HIP_TRY(c, r.soff.alloc(n + 1));
            HIP_TRY(c, r.nsteps.alloc(n));
            HIP_TRY(c, r.steps.alloc(scap));
            HIP_TRY(c, hipMemcpy(r.woff.p, woff.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice));
            HIP_TRY(c, hipMemcpy(r.soff.p, soff.data(), (n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice));
            if (int e = round(r)) return e;
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            std::vector<uint32_t> ns(n);
            std::vector<dcp_step> st(scap);
            std::vector<Real> alts(n);
            HIP_TRY(c, hipMemcpy(ns.data(), r.nsteps.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
            HIP_TRY(c, hipMemcpy(st.data(), r.steps.p, scap * sizeof(dcp_step), hipMemcpyDeviceToHost));
            HIP_TRY(c, hipMemcpy(alts.data(), r.alt.p, n * sizeof(Real), hipMemcpyDeviceToHost));
            for (unsigned i = 0; i < n; ++i)
            {
                unsigned const h = ord[i];
                if (alt_out) alt_out[h] = alts[i];
                if (ns[i] == DCP_TRACE_NO_PATH)
                    rc = c->fail(DCP_EFAIL, "pair (seq %u, profile %u) has no finite %s path", hits[h].seq_idx, hits[h].profile_idx, model);
                else if (ns[i] == DCP_TRACE_TOO_LONG)
                    rc = c->fail(DCP_EFAIL, "path of pair (seq %u, profile %u) has more than 2^32 - 3 steps", hits[h].seq_idx,
                                 hits[h].profile_idx);
                else if (ns[i] > cap[h] && pass == 0)
                    cap[h] = ns[i], again.push_back(h);
                else if (ns[i] > cap[h])
                    rc = c->fail(DCP_EFAIL, "path of hit %u exceeds its step capacity", h);
                else
                    got[h].assign(st.begin() + soff[i], st.begin() + soff[i] + ns[i]);
            }
            t0 = t1;
        }
        if (rc) return rc;
        todo.swap(again);
    }
    uint64_t total_steps = 0;
    for (unsigned h = 0; h < nhits; ++h)
    {
        total_steps += got[h].size();
        if (total_steps > UINT32_MAX) return c->fail(DCP_EFAIL, "the paths of %u hits exceed 2^32 - 1 steps", nhits);
        step_off[h + 1] = (uint32_t)total_steps;
    }
    if (total_steps > cap_steps || (total_steps && !steps_out)) return DCP_ENOMEM;
    for (unsigned h = 0; h < nhits; ++h)
        if (!got[h].empty()) std::memcpy(steps_out + step_off[h], got[h].data(), got[h].size() * sizeof(dcp_step));
    return DCP_OK;
}

} // namespace

extern "C" {

int dcp_gpu_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

dcp_gpu_ctx *dcp_gpu_ctx_new(int device)
{
    int n = dcp_gpu_device_count();
    if (n <= 0 || device < 0 || device >= n)
    {
        fprintf(stderr,
                "dcp_gpu: no HIP device %d (found %d); this engine has no CPU "
                "fallback\n",
                device, n);
        return nullptr;
    }
    dcp_gpu_ctx *c = new (std::nothrow) dcp_gpu_ctx();
    if (!c) return nullptr;
    c->device = device;
    if (hipSetDevice(device) != hipSuccess ||
        hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&c->ev_start) != hipSuccess ||
        hipEventCreate(&c->ev_stop) != hipSuccess)
    {
        fprintf(stderr, "dcp_gpu: failed to create stream/events on device %d\n", device);
        delete c;
        return nullptr;
    }
    if (dcp_qlane_diag_build())
        fprintf(stderr, "dcp_gpu: WARNING: this library is a -DDCP_QLANE_DIAG=%u timing build; its scores are WRONG\n",
                dcp_qlane_diag_build());
    {
        hipDeviceProp_t prop;
        c->num_cus = hipGetDeviceProperties(&prop, device) == hipSuccess ? (unsigned)prop.multiProcessorCount : 256u;
        c->ql_G = (int)dcp_qlane_tile_nodes() / 4;
    }
    bool ok = true;
    for (int k = 0; k < kMaxLaunches; ++k)
        ok = ok && hipEventCreate(&c->ev_class[k]) == hipSuccess;
    for (int k = 0; k < kNumClasses; ++k)
        ok = ok && hipStreamCreateWithFlags(&c->class_stream[k], hipStreamNonBlocking) == hipSuccess;
    if (!ok)
    {
        fprintf(stderr, "dcp_gpu: failed to create stream/events on device %d\n", device);
        delete c;
        return nullptr;
    }
    return c;
}

void dcp_gpu_ctx_del(dcp_gpu_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->ev_qstage) (void)hipEventDestroy(c->ev_qstage);
    if (c->h_qstage) (void)hipHostFree(c->h_qstage);
    if (c->ev_start) (void)hipEventDestroy(c->ev_start);
    if (c->ev_stop) (void)hipEventDestroy(c->ev_stop);
    for (hipEvent_t e : c->ev_dom)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->ev_calib)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->ev_tail)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->ev_exp)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->sweeps.ev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->sweeps.ev_env)
        if (e) (void)hipEventDestroy(e);
    for (int k = 0; k < kMaxLaunches; ++k)
        if (c->ev_class[k]) (void)hipEventDestroy(c->ev_class[k]);
    for (int k = 0; k <= kNumClasses; ++k)
        if (c->ev_trace[k]) (void)hipEventDestroy(c->ev_trace[k]);
    for (int k = 0; k < kNumClasses; ++k)
        if (c->class_stream[k]) (void)hipStreamDestroy(c->class_stream[k]);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

char const *dcp_gpu_last_error(dcp_gpu_ctx const *c) { return c ? c->err.c_str() : "no context"; }
void *dcp_gpu_stream(dcp_gpu_ctx *c) { return (void *)c->stream; }
unsigned dcp_gpu_db_nprofiles(dcp_gpu_ctx const *c) { return c->nprof; }
unsigned dcp_gpu_nseqs(dcp_gpu_ctx const *c) { return c->nseqs; }

// Host -> device stream of floats in device order through two pinned buffers (dcp_gpu_db_upload).
struct StagedUpload
{
    static constexpr size_t kCap = (size_t)16 << 20; // floats per buffer (64 MB)
    dcp_gpu_ctx *c = nullptr;
    float *dst = nullptr, *buf[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool busy[2] = {false, false};
    size_t off = 0, fill = 0;
    int cur = 0;
    int begin(dcp_gpu_ctx *ctx, float *device_dst)
    {
        c = ctx, dst = device_dst;
        for (int i = 0; i < 2; ++i)
        {
            HIP_TRY(c, hipHostMalloc((void **)&buf[i], kCap * sizeof(float), hipHostMallocDefault));
            HIP_TRY(c, hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
        }
        return DCP_OK;
    }
    int flush()
    {
        if (fill == 0) return DCP_OK;
        HIP_TRY(c, hipMemcpyAsync(dst + off, buf[cur], fill * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipEventRecord(ev[cur], c->stream));
        busy[cur] = true;
        off += fill, fill = 0, cur ^= 1;
        if (busy[cur]) // the buffer about to be refilled: its copy must have left it
        {
            HIP_TRY(c, hipEventSynchronize(ev[cur]));
            busy[cur] = false;
        }
        return DCP_OK;
    }
    int append(float const *src, size_t n)
    {
        while (n)
        {
            size_t const k = std::min(n, kCap - fill);
            std::memcpy(buf[cur] + fill, src, k * sizeof(float));
            fill += k, src += k, n -= k;
            if (fill == kCap)
                if (int rc = flush()) return rc;
        }
        return DCP_OK;
    }
    int finish()
    {
        if (int rc = flush()) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        busy[0] = busy[1] = false;
        return DCP_OK;
    }
    ~StagedUpload()
    {
        if (c && (busy[0] || busy[1])) (void)hipStreamSynchronize(c->stream);
        for (int i = 0; i < 2; ++i)
        {
            if (buf[i]) (void)hipHostFree(buf[i]);
            if (ev[i]) (void)hipEventDestroy(ev[i]);
        }
    }
};

// What dcp_gpu_decode_paths needs besides the dists themselves: match_row[p], the row of profile p's first match dist in
// the resident dists; the host's exp() of the null and insert dists; the epsilon of the decode.
static int decode_db_setup(dcp_gpu_ctx *c, dcp_profile *const *profiles, unsigned nprofiles, std::vector<uint32_t> const &match_row)
{
    std::vector<double> ex((size_t)nprofiles * 2u * DCP_DECODE_EXP), eps(nprofiles);
    for (unsigned p = 0; p < nprofiles; ++p)
        dcp_profile_decode_exp(profiles[p], &ex[(size_t)p * 2u * DCP_DECODE_EXP], &eps[p]);
    HIP_TRY(c, c->dec.d_match_row.alloc(nprofiles));
    HIP_TRY(c, c->dec.d_exp.alloc(ex.size()));
    HIP_TRY(c, c->dec.d_eps.alloc(nprofiles));
    HIP_TRY(c, hipMemcpy(c->dec.d_match_row.p, match_row.data(), nprofiles * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->dec.d_exp.p, ex.data(), ex.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->dec.d_eps.p, eps.data(), nprofiles * sizeof(double), hipMemcpyHostToDevice));
    c->dec.ready = true;
    return DCP_OK;
}

// ---------------------------------------------------------------------------
// DB upload
// ---------------------------------------------------------------------------
int dcp_gpu_db_upload(dcp_gpu_ctx *c, dcp_profile *const *profiles,
                      unsigned nprofiles, int flags)
{
    if (!c) return DCP_EINVAL;
    if (flags & ~(DCP_DB_EXPAND_ON_HOST | DCP_DB_ONE_LAYOUT)) return c->fail(DCP_EINVAL, "unknown upload flags %d", flags);
    int const expand_on_host = flags & DCP_DB_EXPAND_ON_HOST;
    if (!profiles || nprofiles == 0) return c->fail(DCP_EINVAL, "empty profile list");
    if (nprofiles > (1u << 20)) return c->fail(DCP_EINVAL, "too many profiles"); // MAX_NPROFILES limits.h:7
    for (unsigned p = 0; p < nprofiles; ++p)
        if (profiles[p] && dcp_profile_precision(profiles[p]) == 64)
            return c->fail(DCP_EINVAL, "profile %u was built in double: upload it with dcp_gpu_db_upload64", p);
    HIP_TRY(c, hipSetDevice(c->device));
    void_last_scan(c);
    c->dec.release();
    c->sweeps.release();
    if (c->precision == 64) // one resident DB per context: the double one goes
    {
        c->f64.release();
        c->nprof = 0;
    }
    c->precision = 0;

    // classify and order: by size class, then by caller index
    std::vector<int> cls(nprofiles);
    c->core_sizes.assign(nprofiles, 0);
    for (unsigned p = 0; p < nprofiles; ++p)
    {
        if (!profiles[p]) return c->fail(DCP_EINVAL, "null profile %u", p);
        unsigned M = dcp_profile_core_size(profiles[p]);
        int k = class_of(M);
        if (k < 0) return c->fail(DCP_EINVAL, "profile %u: core_size %u too big", p, M);
        cls[p] = k;
        c->core_sizes[p] = M;
    }
    // E(j) as the match states' maximum (both kernels) needs MD, DD <= 0: true of every profile whose
    // transitions are log-probabilities.  Any other profile is flagged: the row sweep then takes the
    // delete states into E(j), the query-lane kernels hand its pairs to the row sweep (redo lists).
    std::vector<uint8_t> flagged(nprofiles, 0);
    for (unsigned p = 0; p < nprofiles; ++p)
    {
        float const *t8 = dcp_profile_trans8(profiles[p]);
        unsigned const M = c->core_sizes[p];
        bool pos = false;
        for (unsigned k = 1; k < M && !pos; ++k) // edges into node 0 do not exist (-inf below)
            pos = t8[(size_t)DCP_T_MD * M + k] > 0.0f || t8[(size_t)DCP_T_DD * M + k] > 0.0f;
        flagged[p] = pos ? 1 : 0;
    }
    std::vector<unsigned> order(nprofiles);
    for (unsigned p = 0; p < nprofiles; ++p)
        order[p] = p;
    // by size class; inside a class of several wavefronts by the segmented sweep's lane width (seg_r_of), so that the
    // profiles of one segment kernel are a contiguous range; inside the two smallest classes the flagged profiles last
    // (the others are grouped K to a wavefront: kMpParts); then by the caller's index
    std::stable_sort(order.begin(), order.end(), [&](unsigned a, unsigned b) {
        if (cls[a] != cls[b]) return cls[a] < cls[b];
        if (cls[a] < 2) return flagged[a] < flagged[b];
        return seg_r_of(c->core_sizes[a]) < seg_r_of(c->core_sizes[b]);
    });

    c->metas.assign(nprofiles, dcp_prof_meta{});
    std::vector<uint32_t> dist_row(nprofiles);
    uint64_t emis_floats = 0, trans_floats = 0, match_rows = 0;
    for (int k = 0; k <= kNumClasses; ++k)
        c->class_first[k] = 0;
    c->mp_groups.clear();
    c->mp_first[0] = c->mp_first[1] = c->mp_first[2] = 0;
    c->mp_flagged_first[0] = c->mp_flagged_first[1] = 0;
    c->mp_in_ready = false;
    uint64_t mp_in_pairs = 0;
    for (unsigned i = 0; i < nprofiles;)
    {
        unsigned const p0 = order[i];
        int const k0 = cls[p0];
        SizeClass const sc = kClasses[k0];
        // The two smallest classes (at most 128 nodes), unflagged: kMpParts[class] consecutive profiles share one
        // table -- their columns side by side, each followed by >= 8 columns of -inf -- and one wavefront scores
        // them against a query together (viterbi_mp_kernel).  Each member's meta is a column view of that table.
        unsigned members = 1;
        if (k0 < 2 && !flagged[p0])
            while (members < kMpParts[k0] && i + members < nprofiles && cls[order[i + members]] == k0 && !flagged[order[i + members]])
                ++members;
        bool const grouped = k0 < 2 && !flagged[p0];
        unsigned widths[4] = {0, 0, 0, 0}, ldk = 0;
        for (unsigned j = 0; j < members; ++j)
        {
            unsigned const M = c->core_sizes[order[i + j]];
            if (grouped) widths[j] = (M + 8u + 3u) & ~3u;
            else
            {
                // Row length of a stand-alone profile's tables.  Several wavefronts per pair: the class capacity
                // (every lane has columns, the padding ones -inf), or core_size + 8 if that is shorter.  One
                // wavefront: core_size + R columns rounded up to 4 -- every row ends in at least R columns of -inf,
                // which all lanes past the last node read instead of owning padding columns: 15 % fewer bytes per
                // row on a Pfam-like size distribution, fewer HBM and L2 lines per DP row.
                unsigned w = sc.cap();
                if (sc.W == 1 && M <= 63u * (unsigned)sc.R) w = (M + (unsigned)sc.R + 3u) & ~3u;
                if (sc.W > 1) w = std::min(w, (M + 8u + 3u) & ~3u);
                widths[j] = w;
            }
            ldk += widths[j];
        }
        dcp_mp_group g{};
        if (grouped)
        {
            g.emis_off = emis_floats, g.trans_off = (uint32_t)trans_floats, g.ldk = ldk;
            g.in_off = (uint32_t)mp_in_pairs, g.nparts = members;
            mp_in_pairs += (uint64_t)DCP_NCODES * kMpParts[k0];
        }
        unsigned col0 = 0;
        for (unsigned j = 0; j < members; ++j)
        {
            unsigned const p = order[i + j];
            dcp_prof_meta &m = c->metas[i + j];
            m.emis_off = emis_floats + col0;
            m.trans_off = (uint32_t)(trans_floats + col0);
            m.core_size = c->core_sizes[p];
            m.ldk = ldk;
            m.width = widths[j];
            m.pidx = p;
            m.flags = flagged[p] ? DCP_PROF_EXACT_E : 0u;
            dist_row[i + j] = (uint32_t)match_rows;
            match_rows += m.core_size;
            if (grouped) g.col0[j] = col0, g.core_size[j] = m.core_size, g.pidx[j] = p, g.slot[j] = i + j;
            col0 += widths[j];
        }
        if (grouped)
        {
            // an absent member's lanes read -inf: the padding behind the last member
            for (unsigned j = members; j < 4; ++j)
                g.col0[j] = g.col0[members - 1] + ((g.core_size[members - 1] + 3u) & ~3u), g.core_size[j] = 0;
            c->mp_groups.push_back(g);
            c->mp_first[k0 + 1] = (unsigned)c->mp_groups.size();
        }
        else if (k0 < 2 && c->mp_flagged_first[k0] == 0 && flagged[p0])
            c->mp_flagged_first[k0] = i + 1u; // (+1: 0 means none)
        emis_floats += (uint64_t)DCP_NCODES * ldk;
        trans_floats += 8ull * ldk;
        for (unsigned j = 0; j < members; ++j)
            c->class_first[cls[order[i + j]] + 1] = i + j + 1;
        i += members;
    }
    if (c->mp_first[1] < c->mp_first[0]) c->mp_first[1] = c->mp_first[0];
    if (c->mp_first[2] < c->mp_first[1]) c->mp_first[2] = c->mp_first[1];
    if (mp_in_pairs > 0xffffffffull) return c->fail(DCP_EINVAL, "DB too large for 32-bit table offsets");
    for (int k = 1; k <= kNumClasses; ++k) // empty classes inherit the boundary
        if (c->class_first[k] < c->class_first[k - 1]) c->class_first[k] = c->class_first[k - 1];
    if (trans_floats > 0xffffffffull || match_rows > 0xffffffffull)
        return c->fail(DCP_EINVAL, "DB too large for 32-bit row offsets");

    HIP_TRY(c, c->d_metas.alloc(nprofiles));
    c->slot_of_pidx.assign(nprofiles, 0);
    for (unsigned i = 0; i < nprofiles; ++i)
        c->slot_of_pidx[c->metas[i].pidx] = i;
    HIP_TRY(c, c->d_slot_of_pidx.alloc(nprofiles));
    HIP_TRY(c, hipMemcpy(c->d_slot_of_pidx.p, c->slot_of_pidx.data(), nprofiles * sizeof(uint32_t), hipMemcpyHostToDevice));
    c->rs_floats = emis_floats;
    c->rs_ready = false;
    c->rs_tiles.clear();
    c->d_emis_match.release();
    c->d_emis_tiles.release();
    c->d_dists.release();
    c->d_eps.release();
    // One table layout or two.  The tile images of the query-lane kernels (19.6 GB for 20 000 Pfam-like profiles) repeat
    // the numbers of the row-sweep tables (20.6 GB), which a scan with hits needs anyway (redo lists, traceback).  With
    // DCP_DB_ONE_LAYOUT -- or by itself when both would not leave 16 GiB of this device's free memory for planes,
    // sequences and the traceback's work areas -- only the row-sweep tables are built, at once, and the query-lane
    // kernels gather each tile's image from them (stage_tile_image<G, true>, dcp_qlane.hip).
    uint64_t tile_floats_needed = 0;
    for (unsigned i = 0; i < nprofiles; ++i)
        tile_floats_needed += (uint64_t)((c->metas[i].core_size + 4u * (unsigned)c->ql_G - 1u) / (4u * (unsigned)c->ql_G)) *
                              (4u * (unsigned)c->ql_G) * DCP_NCODES;
    c->one_layout = (flags & DCP_DB_ONE_LAYOUT) != 0;
    if (!c->one_layout)
    {
        size_t free_b = 0, total_b = 0;
        HIP_TRY(c, hipMemGetInfo(&free_b, &total_b));
        uint64_t const both = (tile_floats_needed + emis_floats + (match_rows + 2ull * nprofiles) * (DCP_NDIST + 1)) * sizeof(float);
        if (both + (16ull << 30) > (uint64_t)free_b) c->one_layout = true;
    }
    c->table_bytes = (c->one_layout ? emis_floats : tile_floats_needed + (expand_on_host ? emis_floats : 0)) * sizeof(float);
    if (expand_on_host || c->one_layout) HIP_TRY(c, c->d_emis_match.alloc(emis_floats));
    HIP_TRY(c, c->d_trans8.alloc(trans_floats));
    HIP_TRY(c, c->d_emis_insert.alloc((size_t)nprofiles * DCP_NCODES));
    HIP_TRY(c, c->d_emis_null.alloc((size_t)nprofiles * DCP_NCODES));
    HIP_TRY(c, hipMemcpyAsync(c->d_metas.p, c->metas.data(), nprofiles * sizeof(dcp_prof_meta),
                              hipMemcpyHostToDevice, c->stream));

    // transitions, padded with -inf (unreachable padding nodes)
    {
        float const ninf = -std::numeric_limits<float>::infinity();
        std::vector<float> t8(trans_floats, ninf);
        for (unsigned i = 0; i < nprofiles; ++i)
        {
            dcp_prof_meta const &m = c->metas[i];
            float const *src = dcp_profile_trans8(profiles[m.pidx]);
            for (int row = 0; row < 8; ++row)
                std::memcpy(&t8[m.trans_off + (size_t)row * m.ldk], src + (size_t)row * m.core_size,
                            sizeof(float) * m.core_size); // (a view: row stride = the group's ldk)
            // The first node has no predecessor node: whatever a caller-built profile (dcp_profile_from_parts)
            // holds there, the edges into it are -inf.  The row sweep relies on it (lane 0 adds them to 0).
            for (int row : {DCP_T_MM, DCP_T_IM, DCP_T_DM, DCP_T_MD, DCP_T_DD})
                t8[m.trans_off + (size_t)row * m.ldk] = ninf;
        }
        HIP_TRY(c, hipMemcpyAsync(c->d_trans8.p, t8.data(), t8.size() * sizeof(float),
                                  hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }

    // query-lane layout: per profile T = ceil(M / KT) tile images and per-tile transitions
    unsigned const KT = 4u * (unsigned)c->ql_G;
    uint64_t tile_floats = 0, ttrans_floats = 0;
    c->ql_metas.assign(nprofiles, dcp_ql_prof{});
    c->any_exact_e = false;
    c->sum_core = c->sum_tiles = 0;
    c->max_tiles = 0;
    for (uint64_t &v : c->class_core)
        v = 0;
    for (unsigned i = 0; i < nprofiles; ++i)
    {
        dcp_prof_meta const &m = c->metas[i];
        dcp_ql_prof &qm = c->ql_metas[i];
        qm.core_size = m.core_size;
        qm.pidx = m.pidx;
        qm.rs_slot = i; // ql_metas and metas share one order
        qm.cls = (uint32_t)class_of(m.core_size);
        qm.ntiles = (m.core_size + KT - 1) / KT;
        c->sum_core += m.core_size;
        c->class_core[qm.cls] += m.core_size;
        c->sum_tiles += qm.ntiles;
        c->max_tiles = std::max(c->max_tiles, qm.ntiles);
        qm.needs_exact_e = (m.flags & DCP_PROF_EXACT_E) ? 1u : 0u;
        c->any_exact_e = c->any_exact_e || qm.needs_exact_e != 0u;
        qm.tile_off = c->one_layout ? m.emis_off : tile_floats; // one layout: its first column in emis_match
        qm.ldk = c->one_layout ? m.ldk : 0u;
        qm.ttrans_off = (uint32_t)ttrans_floats;
        tile_floats += (uint64_t)qm.ntiles * KT * DCP_NCODES;
        ttrans_floats += (uint64_t)qm.ntiles * (KT + 1) * 8;
    }
    if (ttrans_floats > 0xffffffffull) return c->fail(DCP_EINVAL, "DB too large for 32-bit transition offsets");
    HIP_TRY(c, c->d_ql_metas.alloc(nprofiles));
    if (!c->one_layout) HIP_TRY(c, c->d_emis_tiles.alloc(tile_floats));
    HIP_TRY(c, c->d_ttrans.alloc(ttrans_floats));
    HIP_TRY(c, hipMemcpy(c->d_ql_metas.p, c->ql_metas.data(), nprofiles * sizeof(dcp_ql_prof), hipMemcpyHostToDevice));
    {
        float const ninf = -std::numeric_limits<float>::infinity();
        std::vector<float> tt(ttrans_floats, ninf);
        for (unsigned i = 0; i < nprofiles; ++i)
        {
            dcp_ql_prof const &qm = c->ql_metas[i];
            float const *src = dcp_profile_trans8(profiles[qm.pidx]);
            unsigned const M = qm.core_size;
            for (unsigned t = 0; t < qm.ntiles; ++t)
                for (unsigned kk = 0; kk <= KT; ++kk)
                {
                    unsigned node = t * KT + kk;
                    if (node >= M) break;
                    float *dst = &tt[qm.ttrans_off + ((size_t)t * (KT + 1) + kk) * 8];
                    for (int row = 0; row < 8; ++row)
                        dst[row] = src[(size_t)row * M + node];
                }
        }
        HIP_TRY(c, hipMemcpy(c->d_ttrans.p, tt.data(), tt.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    c->qorder_q0 = c->qorder_q1 = ~0u;

    if (expand_on_host)
    {
        // parity path: tables from dcp_frame_table_host, profile by profile
        std::vector<float> col(DCP_NCODES), tab;
        std::vector<float> ins((size_t)nprofiles * DCP_NCODES), nul((size_t)nprofiles * DCP_NCODES);
        float const ninf = -std::numeric_limits<float>::infinity();
        std::vector<float> emis_host((size_t)emis_floats, ninf);
        for (unsigned i = 0; i < nprofiles; ++i)
        {
            dcp_prof_meta const &m = c->metas[i];
            dcp_profile const *pr = profiles[m.pidx];
            float eps = dcp_profile_epsilon(pr);
            tab.assign((size_t)DCP_NCODES * m.width, ninf);
            dcp_ql_prof const &qm = c->ql_metas[i];
            std::vector<float> img((size_t)qm.ntiles * KT * DCP_NCODES, ninf);
            float const *md = dcp_profile_match_dist(pr);
            for (unsigned k = 0; k < m.core_size; ++k)
            {
                dcp_frame_table_host(md + (size_t)k * DCP_NDIST, eps, col.data());
                size_t const grp = (size_t)(k / KT) * (KT / 4) + (k % KT) / 4;
                for (unsigned code = 0; code < DCP_NCODES; ++code)
                {
                    tab[(size_t)code * m.width + k] = col[code];
                    img[(grp * DCP_NCODES + code) * 4 + (k & 3u)] = col[code];
                }
            }
            // its own columns of rows it may share with other profiles: into the host image of all tables, which goes
            // to the device in one piece below (this path is the tests': small databases)
            for (unsigned code = 0; code < DCP_NCODES; ++code)
                std::memcpy(&emis_host[m.emis_off + (size_t)code * m.ldk], &tab[(size_t)code * m.width], sizeof(float) * m.width);
            if (!c->one_layout)
                HIP_TRY(c, hipMemcpy(c->d_emis_tiles.p + qm.tile_off, img.data(), img.size() * sizeof(float),
                                     hipMemcpyHostToDevice));
            dcp_frame_table_host(dcp_profile_insert_dist(pr), eps, &ins[(size_t)m.pidx * DCP_NCODES]);
            dcp_frame_table_host(dcp_profile_null_dist(pr), eps, &nul[(size_t)m.pidx * DCP_NCODES]);
        }
        HIP_TRY(c, hipMemcpy(c->d_emis_match.p, emis_host.data(), emis_host.size() * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(c->d_emis_insert.p, ins.data(), ins.size() * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(c->d_emis_null.p, nul.data(), nul.size() * sizeof(float), hipMemcpyHostToDevice));
        if (c->keep_dists)
        {
            // the match dists in the rows they have after a device expansion (this path is the tests': small databases)
            HIP_TRY(c, c->d_dists.alloc((size_t)match_rows * DCP_NDIST));
            for (unsigned i = 0; i < nprofiles; ++i)
                HIP_TRY(c, hipMemcpy(c->d_dists.p + (size_t)dist_row[i] * DCP_NDIST, dcp_profile_match_dist(profiles[c->metas[i].pidx]),
                                     (size_t)c->metas[i].core_size * DCP_NDIST * sizeof(float), hipMemcpyHostToDevice));
        }
    }
    else
    {
        // dists rows: all match nodes (sorted profile order), then insert dists
        // by pidx, then null dists by pidx
        // The compact DB (129 floats per node: 1.9 GB for 20k profiles) goes to the device in the order
        // the rows have there, through two pinned 64 MB buffers: the copy of one overlaps the filling of
        // the other, and no host-side image of the whole array is built.
        size_t const rows = (size_t)match_rows + 2 * (size_t)nprofiles;
        std::vector<float> eps(rows);
        HIP_TRY(c, c->d_dists.alloc(rows * DCP_NDIST));
        StagedUpload up;
        if (int rc = up.begin(c, c->d_dists.p)) return rc;
        for (unsigned i = 0; i < nprofiles; ++i)
        {
            dcp_prof_meta const &m = c->metas[i];
            dcp_profile const *pr = profiles[m.pidx];
            if (int rc = up.append(dcp_profile_match_dist(pr), (size_t)DCP_NDIST * m.core_size)) return rc;
            std::fill(eps.begin() + dist_row[i], eps.begin() + dist_row[i] + m.core_size,
                      dcp_profile_epsilon(pr));
        }
        for (unsigned p = 0; p < nprofiles; ++p)
        {
            if (int rc = up.append(dcp_profile_insert_dist(profiles[p]), DCP_NDIST)) return rc;
            eps[(size_t)match_rows + p] = eps[(size_t)match_rows + nprofiles + p] =
                dcp_profile_epsilon(profiles[p]);
        }
        for (unsigned p = 0; p < nprofiles; ++p)
            if (int rc = up.append(dcp_profile_null_dist(profiles[p]), DCP_NDIST)) return rc;
        if (int rc = up.finish()) return rc;
        std::vector<dcp_expand_tile> tiles;
        for (unsigned i = 0; i < nprofiles; ++i)
        {
            dcp_prof_meta const &m = c->metas[i];
            for (unsigned k0 = 0; k0 < m.width; k0 += 64) // its own columns of the (possibly shared) rows
            {
                dcp_expand_tile t{};
                t.out_off = m.emis_off + k0;
                t.ncols = k0 < m.core_size ? std::min(64u, m.core_size - k0) : 0u;
                t.dist_row = t.ncols ? dist_row[i] + k0 : 0u;
                t.nstore = std::min(64u, m.width - k0);
                t.ld_code = m.ldk;
                t.ld_col = 1;
                tiles.push_back(t);
            }
        }
        size_t const n_match_tiles = tiles.size();
        for (unsigned i = 0; i < nprofiles && !c->one_layout; ++i)
        {
            dcp_prof_meta const &m = c->metas[i];
            dcp_ql_prof const &qm = c->ql_metas[i];
            unsigned const ncol = qm.ntiles * KT; // incl. -inf padding nodes
            for (unsigned k0 = 0; k0 < ncol; k0 += 64)
            {
                dcp_expand_tile t{};
                t.out_off = qm.tile_off;
                t.ncols = k0 < m.core_size ? std::min(64u, m.core_size - k0) : 0u;
                t.dist_row = t.ncols ? dist_row[i] + k0 : 0u;
                t.nstore = std::min(64u, ncol - k0);
                t.kt = KT;
                t.col0 = k0;
                tiles.push_back(t);
            }
        }
        size_t const n_image_tiles = tiles.size() - n_match_tiles;
        for (int which = 0; which < 2; ++which)
            for (unsigned p0 = 0; p0 < nprofiles; p0 += 64)
            {
                dcp_expand_tile t{};
                t.out_off = (uint64_t)p0 * DCP_NCODES;
                t.ncols = t.nstore = std::min(64u, nprofiles - p0);
                t.dist_row = (uint32_t)(match_rows + (which ? nprofiles : 0) + p0);
                t.ld_code = 1;
                t.ld_col = DCP_NCODES;
                tiles.push_back(t);
            }
        size_t const n_special_tiles = (tiles.size() - n_match_tiles - n_image_tiles) / 2;

        DevBuf<float> &d_dists = c->d_dists, &d_eps = c->d_eps; // kept for the lazy row-sweep layout
        DevBuf<dcp_expand_tile> d_tiles;
        HIP_TRY(c, d_eps.alloc(eps.size()));
        HIP_TRY(c, d_tiles.alloc(tiles.size()));
        HIP_TRY(c, hipMemcpy(d_eps.p, eps.data(), eps.size() * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(d_tiles.p, tiles.data(), tiles.size() * sizeof(dcp_expand_tile), hipMemcpyHostToDevice));
        c->rs_tiles.assign(tiles.begin(), tiles.begin() + (long)n_match_tiles);
        dcp_expand_args ea{d_tiles.p, d_dists.p, d_eps.p, nullptr};
        if (c->one_layout)
        {
            // the row-sweep tables now, not on first use
            ea.tiles = d_tiles.p;
            ea.out = c->d_emis_match.p;
            dcp_launch_expand(&ea, (unsigned)n_match_tiles, c->stream);
        }
        else
        {
            ea.tiles = d_tiles.p + n_match_tiles;
            ea.out = c->d_emis_tiles.p;
            dcp_launch_expand(&ea, (unsigned)n_image_tiles, c->stream);
        }
        ea.tiles = d_tiles.p + n_match_tiles + n_image_tiles;
        ea.out = c->d_emis_insert.p;
        dcp_launch_expand(&ea, (unsigned)n_special_tiles, c->stream);
        ea.tiles = d_tiles.p + n_match_tiles + n_image_tiles + n_special_tiles;
        ea.out = c->d_emis_null.p;
        dcp_launch_expand(&ea, (unsigned)n_special_tiles, c->stream);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (c->one_layout)
        {
            // nothing is rebuilt later: the compact dists go, unless the decode was promised them
            c->rs_tiles.clear();
            if (!c->keep_dists) c->d_dists.release();
            c->d_eps.release();
        }
    }
    // the grouped profiles' descriptors and their merged {insert, background} tables
    if (!c->mp_groups.empty())
    {
        HIP_TRY(c, c->d_mp_groups.alloc(c->mp_groups.size()));
        HIP_TRY(c, hipMemcpy(c->d_mp_groups.p, c->mp_groups.data(), c->mp_groups.size() * sizeof(dcp_mp_group), hipMemcpyHostToDevice));
        HIP_TRY(c, c->d_mp_in.alloc((size_t)mp_in_pairs * 2u));
        dcp_launch_mp_in(c->d_mp_groups.p, (unsigned)c->mp_groups.size(), c->mp_first[1], kMpParts[0], kMpParts[1],
                         c->d_emis_insert.p, c->d_emis_null.p, c->d_mp_in.p, c->stream);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    c->rs_ready = expand_on_host != 0 || c->one_layout;
    if (c->d_dists.p) // kept for the decode, or for the lazy row-sweep layout (a default two-layout DB): either way it can decode
    {
        std::vector<uint32_t> match_row(nprofiles);
        for (unsigned i = 0; i < nprofiles; ++i)
            match_row[c->metas[i].pidx] = dist_row[i];
        if (int rc = decode_db_setup(c, profiles, nprofiles, match_row)) return rc;
    }
    c->nprof = nprofiles;
    c->precision = 32;
    return DCP_OK;
}

// Expand the row-sweep layout of the match tables ([1364][ldk] per profile) if it is not resident yet.
static int ensure_rowsweep_layout(dcp_gpu_ctx *c)
{
    if (c->rs_ready) return DCP_OK;
    if (c->rs_tiles.empty() || !c->d_dists.p) return c->fail(DCP_EFAIL, "row-sweep layout cannot be rebuilt");
    HIP_TRY(c, c->d_emis_match.alloc(c->rs_floats));
    DevBuf<dcp_expand_tile> d_tiles;
    HIP_TRY(c, d_tiles.alloc(c->rs_tiles.size()));
    HIP_TRY(c, hipMemcpy(d_tiles.p, c->rs_tiles.data(), c->rs_tiles.size() * sizeof(dcp_expand_tile), hipMemcpyHostToDevice));
    dcp_expand_args ea{d_tiles.p, c->d_dists.p, c->d_eps.p, c->d_emis_match.p};
    dcp_launch_expand(&ea, (unsigned)c->rs_tiles.size(), c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->rs_ready = true;
    return DCP_OK;
}

int dcp_gpu_db_one_layout(dcp_gpu_ctx const *c) { return c && c->one_layout ? 1 : 0; }
int dcp_gpu_db_precision(dcp_gpu_ctx const *c) { return c ? c->precision : 0; }
uint64_t dcp_gpu_db_table_bytes(dcp_gpu_ctx const *c)
{
    if (!c || c->nprof == 0) return 0;
    if (c->precision == 64) return c->f64.d_tab.n * sizeof(double);
    // the lazily expanded row-sweep tables count once they are there
    bool const lazy_there = !c->one_layout && c->rs_ready && c->d_dists.p && !c->rs_tiles.empty();
    return c->table_bytes + (lazy_there ? c->rs_floats * sizeof(float) : 0);
}

int dcp_gpu_db_fetch_match_table(dcp_gpu_ctx *c, unsigned p, float *out)
{
    if (!c || !out || p >= c->nprof) return DCP_EINVAL;
    if (c->precision == 64) return c->fail(DCP_EINVAL, "the resident DB is double: it has no float match tables");
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = ensure_rowsweep_layout(c)) return rc;
    for (dcp_prof_meta const &m : c->metas)
        if (m.pidx == p) return fetch_table_rows(c, c->d_emis_match.p + m.emis_off, m.ldk, m.core_size, out);
    return DCP_EINVAL;
}

int dcp_gpu_db_fetch_match_table64(dcp_gpu_ctx *c, unsigned p, double *out)
{
    if (!c || !out || p >= c->nprof) return DCP_EINVAL;
    if (c->precision != 64) return c->fail(DCP_EINVAL, "the resident DB is float: it has no double match tables");
    HIP_TRY(c, hipSetDevice(c->device));
    for (dcp_f64_prof const &m : c->f64.profs)
        if (m.pidx == p) return fetch_table_rows(c, c->f64.d_tab.p + m.tab_off, m.ldk, m.core_size, out);
    return DCP_EINVAL;
}

int dcp_gpu_db_fetch_insert_null64(dcp_gpu_ctx *c, unsigned p, double *insert, double *null_tab)
{
    if (!c || p >= c->nprof) return DCP_EINVAL;
    if (c->precision != 64) return c->fail(DCP_EINVAL, "the resident DB is float: it has no double tables");
    HIP_TRY(c, hipSetDevice(c->device));
    for (dcp_f64_prof const &m : c->f64.profs)
        if (m.pidx == p)
        {
            // [2][1364]: the insert table, then the null table
            if (insert) HIP_TRY(c, hipMemcpy(insert, c->f64.d_xe.p + m.xe_off, DCP_NCODES * sizeof(double), hipMemcpyDeviceToHost));
            if (null_tab)
                HIP_TRY(c, hipMemcpy(null_tab, c->f64.d_xe.p + m.xe_off + DCP_NCODES, DCP_NCODES * sizeof(double),
                                     hipMemcpyDeviceToHost));
            return DCP_OK;
        }
    return DCP_EINVAL;
}

// ---------------------------------------------------------------------------
// The double DB (dcp_gpu_db_upload64) and its scan: dcp_f64.hip
// ---------------------------------------------------------------------------
// Launch groups of an f64 DB: nodes per lane R of viterbi64_kernel<R>, and whether the profiles are swept in
// column segments (more than 64 x 4 nodes: DCP_F64_SEG)
static constexpr int kF64R[4] = {1, 2, 4, 4};
static int f64_group(unsigned M) { return M <= 64u ? 0 : M <= 128u ? 1 : M <= (unsigned)DCP_F64_SEG ? 2 : 3; }

int dcp_gpu_db_upload64(dcp_gpu_ctx *c, dcp_profile *const *profiles, unsigned nprofiles)
{
    if (!c) return DCP_EINVAL;
    if (!profiles || nprofiles == 0) return c->fail(DCP_EINVAL, "empty profile list");
    if (nprofiles > (1u << 20)) return c->fail(DCP_EINVAL, "too many profiles");
    for (unsigned p = 0; p < nprofiles; ++p)
    {
        if (!profiles[p]) return c->fail(DCP_EINVAL, "null profile %u", p);
        if (dcp_profile_precision(profiles[p]) != 64)
            return c->fail(DCP_EINVAL, "profile %u was built in float: dcp_gpu_db_upload64 takes double profiles only", p);
    }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    // one resident DB per context: whatever was there goes, also if this upload fails half way
    void_last_scan(c);
    c->dec.release();
    c->sweeps.release();
    c->precision = 0;
    c->nprof = 0;
    c->f64.release();
    c->d_emis_match.release(), c->d_emis_tiles.release(), c->d_mp_in.release(), c->d_dists.release();
    c->rs_tiles.clear();
    c->rs_ready = false;
    c->mp_in_ready = false;
    c->one_layout = false;
    c->table_bytes = 0;

    std::vector<unsigned> order(nprofiles);
    for (unsigned p = 0; p < nprofiles; ++p)
        order[p] = p;
    std::stable_sort(order.begin(), order.end(), [&](unsigned a, unsigned b) {
        return f64_group(dcp_profile_core_size(profiles[a])) < f64_group(dcp_profile_core_size(profiles[b]));
    });
    auto &F = c->f64;
    F.profs.assign(nprofiles, dcp_f64_prof{});
    for (int g = 0; g < 5; ++g)
        F.group_first[g] = 0;
    uint64_t tab = 0, trans = 0, xe = 0;
    for (unsigned i = 0; i < nprofiles; ++i)
    {
        unsigned const p = order[i], M = dcp_profile_core_size(profiles[p]);
        int const g = f64_group(M);
        unsigned const span = 64u * (unsigned)kF64R[g];
        unsigned const nseg = (M + span - 1u) / span;
        dcp_f64_prof &m = F.profs[i];
        m.core_size = M;
        m.nseg = nseg;
        m.ldk = nseg * span;
        m.pidx = p;
        m.tab_off = tab;
        m.trans_off = trans;
        m.xe_off = xe;
        tab += (uint64_t)DCP_NCODES * m.ldk; // ldk is a multiple of 64: every table starts 512-byte aligned
        trans += 8ull * m.ldk;
        xe += 2ull * DCP_NCODES;
        F.group_first[g + 1] = i + 1;
    }
    for (int g = 1; g < 5; ++g) // empty groups start where the one before ends
        F.group_first[g] = std::max(F.group_first[g], F.group_first[g - 1]);
    F.slot_of_pidx.assign(nprofiles, 0);
    for (unsigned i = 0; i < nprofiles; ++i)
        F.slot_of_pidx[F.profs[i].pidx] = i;

    // transitions padded with -inf; one expansion job per table column
    std::vector<double> h_trans(trans, -std::numeric_limits<double>::infinity());
    std::vector<double> h_dists;
    std::vector<dcp_f64_expand_job> jobs, xe_jobs; // columns of the match tables; the insert / null tables
    std::vector<uint32_t> match_row(nprofiles);    // by caller index: the decode's map
    jobs.reserve(tab / DCP_NCODES);
    xe_jobs.reserve(2ull * nprofiles);
    for (dcp_f64_prof const &m : F.profs)
    {
        dcp_profile const *pf = profiles[m.pidx];
        unsigned const M = m.core_size;
        double const *t8 = dcp_profile_trans8_64(pf);
        for (unsigned r = 0; r < 8; ++r)
            std::memcpy(&h_trans[m.trans_off + (uint64_t)r * m.ldk], t8 + (size_t)r * M, sizeof(double) * M);
        double const eps = dcp_profile_epsilon64(pf);
        uint32_t const d0 = (uint32_t)(h_dists.size() / DCP_NDIST);
        double const *md = dcp_profile_match_dist64(pf);
        match_row[m.pidx] = d0;
        h_dists.insert(h_dists.end(), md, md + (size_t)M * DCP_NDIST);
        h_dists.insert(h_dists.end(), dcp_profile_insert_dist64(pf), dcp_profile_insert_dist64(pf) + DCP_NDIST);
        h_dists.insert(h_dists.end(), dcp_profile_null_dist64(pf), dcp_profile_null_dist64(pf) + DCP_NDIST);
        for (unsigned k = 0; k < m.ldk; ++k)
            jobs.push_back(dcp_f64_expand_job{m.tab_off + k, k < M ? d0 + k : ~0u, m.ldk, eps});
        xe_jobs.push_back(dcp_f64_expand_job{m.xe_off, d0 + M, 1u, eps});
        xe_jobs.push_back(dcp_f64_expand_job{m.xe_off + DCP_NCODES, d0 + M + 1u, 1u, eps});
    }
    if (jobs.size() >= (1ull << 30) || h_dists.size() / DCP_NDIST >= 0xffffffffull)
        return c->fail(DCP_EINVAL, "profile DB too large");
    HIP_TRY(c, F.d_profs.alloc(nprofiles));
    HIP_TRY(c, F.d_tab.alloc(tab));
    HIP_TRY(c, F.d_trans.alloc(trans));
    HIP_TRY(c, F.d_xe.alloc(xe));
    DevBuf<double> d_dists;
    DevBuf<dcp_f64_expand_job> d_jobs, d_xe_jobs;
    HIP_TRY(c, d_dists.alloc(h_dists.size()));
    HIP_TRY(c, d_jobs.alloc(jobs.size()));
    HIP_TRY(c, d_xe_jobs.alloc(xe_jobs.size()));
    HIP_TRY(c, hipMemcpy(F.d_profs.p, F.profs.data(), nprofiles * sizeof(dcp_f64_prof), hipMemcpyHostToDevice));
    {
        // the query-lane kernel's task order: largest profiles first
        std::vector<uint32_t> by_size(nprofiles);
        for (unsigned i = 0; i < nprofiles; ++i)
            by_size[i] = i;
        std::stable_sort(by_size.begin(), by_size.end(),
                         [&](uint32_t x, uint32_t y) { return F.profs[x].core_size > F.profs[y].core_size; });
        HIP_TRY(c, F.d_order.alloc(nprofiles));
        HIP_TRY(c, hipMemcpy(F.d_order.p, by_size.data(), nprofiles * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    HIP_TRY(c, hipMemcpy(F.d_trans.p, h_trans.data(), trans * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(d_dists.p, h_dists.data(), h_dists.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(d_jobs.p, jobs.data(), jobs.size() * sizeof(dcp_f64_expand_job), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(d_xe_jobs.p, xe_jobs.data(), xe_jobs.size() * sizeof(dcp_f64_expand_job), hipMemcpyHostToDevice));
    // every column of the match tables (padding ones -inf), then the insert / null tables
    dcp_f64_launch_expand(d_jobs.p, (unsigned)jobs.size(), d_dists.p, F.d_tab.p, c->stream);
    dcp_f64_launch_expand(d_xe_jobs.p, (unsigned)xe_jobs.size(), d_dists.p, F.d_xe.p, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->keep_dists)
    {
        if (int rc = decode_db_setup(c, profiles, nprofiles, match_row)) return rc;
        std::swap(c->dec.d_dists64.p, d_dists.p), std::swap(c->dec.d_dists64.n, d_dists.n);
    }
    c->core_sizes.assign(nprofiles, 0);
    for (unsigned p = 0; p < nprofiles; ++p)
        c->core_sizes[p] = dcp_profile_core_size(profiles[p]);
    c->nprof = nprofiles;
    c->precision = 64;
    return DCP_OK;
}

// ---------------------------------------------------------------------------
// The decode of paths on the device: dcp_decode.hip
// ---------------------------------------------------------------------------
int dcp_gpu_db_keep_dists(dcp_gpu_ctx *c, int on)
{
    if (!c) return DCP_EINVAL;
    c->keep_dists = on != 0;
    return DCP_OK;
}

int dcp_gpu_db_has_dists(dcp_gpu_ctx const *c) { return c && c->nprof && c->dec.ready ? 1 : 0; }

// One step of a path as the decode sees it: 0 mute, else DCP_DECODE_NULL / _INSERT / _MATCH + 1; *k the node of an M
// state.  -1: not a state of a profile of core_size nodes.
static int decode_step_kind(unsigned id, unsigned core_size, unsigned *k)
{
    unsigned const msb = id & (3u << 14), idx = id & 0x3FFFu;
    if (msb == (3u << 14))
    {
        // R S N B E J C T: R, N, J, C emit (the null dist)
        if (idx > 7u) return -1;
        return idx == 0u || idx == 2u || idx == 5u || idx == 6u ? DCP_DECODE_NULL + 1 : 0;
    }
    if (idx < 1u || idx > core_size) return -1;
    *k = idx - 1u;
    return msb == 0 ? DCP_DECODE_MATCH + 1 : msb == (1u << 14) ? DCP_DECODE_INSERT + 1 : 0;
}

// What dcp_gpu_decode_paths and dcp_gpu_path_domains check of the caller's paths before anything is launched or
// written, from integers alone: the indices, the step offsets, every state id and seqlen, and the bases the steps emit
// -- at most the sequence's length, or (whole) exactly that.  *nemit: the emitting steps of all paths.
static int check_path_steps(dcp_gpu_ctx *c, uint32_t const *seq_idx, uint32_t const *profile_idx, unsigned npaths,
                            struct dcp_step const *steps, uint32_t const *step_off, bool whole, uint64_t *nemit)
{
    *nemit = 0;
    for (unsigned h = 0; h < npaths; ++h)
    {
        if (step_off[h + 1] < step_off[h]) return c->fail(DCP_EINVAL, "path %u: step offsets decrease", h);
        if (seq_idx[h] >= c->nseqs) return c->fail(DCP_EINVAL, "path %u: sequence %u is not resident (%u are)", h, seq_idx[h], c->nseqs);
        if (profile_idx[h] >= c->nprof) return c->fail(DCP_EINVAL, "path %u: profile %u is not resident (%u are)", h, profile_idx[h], c->nprof);
        if (step_off[h + 1] > step_off[h] && !steps) return c->fail(DCP_EINVAL, "null steps");
        unsigned const M = c->core_sizes[profile_idx[h]];
        uint64_t pos = 0;
        for (uint32_t i = step_off[h]; i < step_off[h + 1]; ++i)
        {
            unsigned k = 0;
            unsigned const len = steps[i].seqlen;
            int const kind = decode_step_kind(steps[i].state_id, M, &k);
            if (kind < 0)
                return c->fail(DCP_EINVAL, "path %u, step %u: state id 0x%04x is no state of a profile of %u nodes", h,
                               i - step_off[h], (unsigned)steps[i].state_id, M);
            if (kind == 0 && len != 0)
                return c->fail(DCP_EINVAL, "path %u, step %u: a mute state with seqlen %u", h, i - step_off[h], len);
            if (kind > 0 && (len < 1u || len > 5u))
                return c->fail(DCP_EINVAL, "path %u, step %u: an emitting state with seqlen %u (1..5)", h, i - step_off[h], len);
            pos += len;
            *nemit += kind > 0;
        }
        uint32_t const L = c->seq_len[seq_idx[h]];
        if (pos > L || (whole && pos != L))
            return c->fail(DCP_EINVAL, "path %u: its steps emit %llu bases, sequence %u has %u", h, (unsigned long long)pos,
                           seq_idx[h], L);
    }
    return DCP_OK;
}

int dcp_gpu_decode_paths(dcp_gpu_ctx *c, uint32_t const *seq_idx, uint32_t const *profile_idx, unsigned npaths,
                         struct dcp_step const *steps, uint32_t const *step_off, uint8_t *codes_out)
{
    if (!c) return DCP_EINVAL;
    if (c->nprof == 0) return c->fail(DCP_EINVAL, "no profile DB resident: nothing to decode with");
    if (c->nseqs == 0) return c->fail(DCP_EINVAL, "no sequences resident: nothing to decode");
    if (!c->dec.ready)
        return c->fail(DCP_EINVAL, "the resident DB's compact distributions are not resident: switch them on with "
                                   "dcp_gpu_db_keep_dists before the upload");
    if (npaths == 0) return DCP_OK;
    if (!seq_idx || !profile_idx || !step_off) return c->fail(DCP_EINVAL, "null index array");
    // everything is checked before anything is launched or written
    uint64_t nemit = 0;
    if (int rc = check_path_steps(c, seq_idx, profile_idx, npaths, steps, step_off, false, &nemit)) return rc;
    uint32_t const first = step_off[0], total = step_off[npaths] - step_off[0];
    if (total == 0) return DCP_OK;
    if (!codes_out) return c->fail(DCP_EINVAL, "null output");
    std::vector<uint8_t> codes(total, (uint8_t)DCP_CODE_MUTE);
    if (nemit)
    {
        HIP_TRY(c, hipSetDevice(c->device));
        size_t const cap = (size_t)std::min<uint64_t>(nemit, (uint64_t)DCP_DECODE_MAX_ITEMS);
        HIP_TRY(c, c->d_dec_items.reserve(cap)); // (the two grow together: a failed second allocation is tried again)
        HIP_TRY(c, c->d_dec_codes.reserve(cap));
        // rounds of at most DCP_DECODE_MAX_ITEMS emitting steps, cut wherever the list is full: the work list (path,
        // fragment start, length, state) holds integers only
        std::vector<dcp_decode_item> items;
        std::vector<uint32_t> dst; // the step each item decodes, relative to `first`
        std::vector<uint8_t> out(cap);
        items.reserve(cap), dst.reserve(cap);
        dcp_decode_args a{};
        a.items = c->d_dec_items.p, a.codes = c->d_dec_codes.p;
        a.words = c->d_seq_words.p, a.woff = c->d_seq_woff.p;
        a.dists = c->precision == 64 ? (void const *)c->dec.d_dists64.p : (void const *)c->d_dists.p;
        a.match_row = c->dec.d_match_row.p, a.exp_ni = c->dec.d_exp.p, a.eps = c->dec.d_eps.p;
        auto flush = [&]() -> int {
            if (items.empty()) return DCP_OK;
            a.nitems = (unsigned)items.size();
            HIP_TRY(c, hipMemcpyAsync(c->d_dec_items.p, items.data(), items.size() * sizeof(dcp_decode_item), hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, (hipError_t)dcp_launch_decode(&a, c->precision == 64, c->stream));
            HIP_TRY(c, hipMemcpyAsync(out.data(), c->d_dec_codes.p, items.size(), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            for (size_t j = 0; j < items.size(); ++j)
                codes[dst[j]] = out[j];
            items.clear(), dst.clear();
            return DCP_OK;
        };
        for (unsigned h = 0; h < npaths; ++h)
        {
            unsigned const M = c->core_sizes[profile_idx[h]];
            uint32_t pos = 0;
            for (uint32_t i = step_off[h]; i < step_off[h + 1]; ++i)
            {
                unsigned k = 0;
                unsigned const len = steps[i].seqlen;
                int const kind = decode_step_kind(steps[i].state_id, M, &k);
                if (kind > 0)
                {
                    items.push_back(dcp_decode_item{seq_idx[h], pos, profile_idx[h], len | ((unsigned)(kind - 1) << 3) | (k << 8)});
                    dst.push_back(i - first);
                    if (items.size() == cap)
                        if (int rc = flush()) return rc;
                }
                pos += len;
            }
        }
        if (int rc = flush()) return rc;
    }
    std::memcpy(codes_out + first, codes.data(), total);
    return DCP_OK;
}

// ---------------------------------------------------------------------------
// Sequences
// ---------------------------------------------------------------------------
static int upload_seqs(dcp_gpu_ctx *c, uint8_t const *seqs, uint32_t const *seq_off,
                       unsigned nseqs, bool text)
{
    if (!c) return DCP_EINVAL;
    if (!seqs || !seq_off || nseqs == 0) return c->fail(DCP_EINVAL, "empty sequence batch");
    HIP_TRY(c, hipSetDevice(c->device));
    void_last_scan(c); // the previous batch's scan
    // the length order and the transposed word planes belong to the batch that was resident
    c->qorder_q0 = c->qorder_q1 = ~0u; // also when this upload fails half way
    std::vector<uint32_t> woff(nseqs), len(nseqs);
    uint64_t nwords = 0, total = 0;
    for (unsigned q = 0; q < nseqs; ++q)
    {
        if (seq_off[q + 1] <= seq_off[q])
            return c->fail(DCP_EINVAL, "sequence cannot be empty"); // protein_profile.c:158
        uint32_t L = seq_off[q + 1] - seq_off[q];
        woff[q] = (uint32_t)nwords;
        len[q] = L;
        nwords += L / 16 + 3; // pad: the kernels look ahead by up to one word + two bases
        total += L;
        if (nwords > 0xffffffffull) return c->fail(DCP_EINVAL, "sequence batch too large");
    }
    std::vector<uint32_t> words(nwords, 0u);
    for (unsigned q = 0; q < nseqs; ++q)
    {
        uint8_t const *s = seqs + seq_off[q];
        uint32_t *w = &words[woff[q]];
        for (uint32_t i = 0; i < len[q]; ++i)
        {
            unsigned b = s[i];
            if (text)
            {
                switch (s[i])
                {
                case 'A': b = 0; break;
                case 'C': b = 1; break;
                case 'G': b = 2; break;
                case 'T': b = 3; break;
                default: b = 255; break;
                }
            }
            if (b > 3)
                return c->fail(DCP_EINVAL, "sequence %u: symbol at %u is outside ACGT", q, i);
            w[i >> 4] |= b << ((i & 15u) * 2u);
        }
    }
    // a failed (re)allocation below must not leave the old batch's size paired with new buffers
    c->nseqs = 0;
    c->strands = 0;
    c->total_len = 0;
    c->seq_len.clear();
    c->drop_windows(); // a new batch is uncut
    HIP_TRY(c, c->d_seq_words.alloc(nwords));
    HIP_TRY(c, c->d_seq_woff.alloc(nseqs));
    HIP_TRY(c, c->d_seq_len.alloc(nseqs));
    HIP_TRY(c, c->d_xtrans.alloc((size_t)nseqs * DCP_XSTRIDE));
    HIP_TRY(c, hipMemcpy(c->d_seq_words.p, words.data(), nwords * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->d_seq_woff.p, woff.data(), nseqs * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->d_seq_len.p, len.data(), nseqs * sizeof(uint32_t), hipMemcpyHostToDevice));
    c->seq_len = len;
    c->nseqs = nseqs;
    c->strands = 1;
    c->total_len = total;
    c->xt_multi = c->xt_h3 = -1;
    c->xt_explicit = false;
    c->xt64.clear();
    return DCP_OK;
}

int dcp_gpu_seqs_upload(dcp_gpu_ctx *c, uint8_t const *seqs, uint32_t const *seq_off, unsigned nseqs)
{
    return upload_seqs(c, seqs, seq_off, nseqs, false);
}

int dcp_gpu_seqs_upload_text(dcp_gpu_ctx *c, char const *text, uint32_t const *seq_off, unsigned nseqs)
{
    return upload_seqs(c, (uint8_t const *)text, seq_off, nseqs, true);
}

unsigned dcp_gpu_seqs_strands(dcp_gpu_ctx const *c) { return c && c->nseqs ? c->strands : 0u; }

// Both strands: the resident batch of n sequences becomes 2n, sequence n + q the reverse complement of q.  The forward
// half of every array is copied on the device, the reverse half written by dcp_seqs.hip's kernels: no base goes
// through the host again.  Dependent state is treated as by an upload.
int dcp_gpu_seqs_add_revcomp(dcp_gpu_ctx *c)
{
    if (!c) return DCP_EINVAL;
    if (c->nseqs == 0) return c->fail(DCP_EINVAL, "no sequences resident: upload a batch before adding its reverse strand");
    if (c->strands != 1) return c->fail(DCP_EINVAL, "the resident batch already holds both strands");
    if (!c->reg_src.empty())
        return c->fail(DCP_EINVAL, "the resident batch is one of regions: a region carries its own strand (dcp_gpu_seqs_cut_regions)");
    if (c->xt_explicit || !c->xt64.empty())
        return c->fail(DCP_EINVAL, "explicit special transitions are in force: they are per sequence -- set them after "
                                   "dcp_gpu_seqs_add_revcomp, for %llu rows", 2ull * c->nseqs);
    unsigned const n = c->nseqs;
    uint64_t const nwords = c->d_seq_words.n;
    if (2ull * n > 0xffffffffull || 2ull * nwords > 0xffffffffull)
        return c->fail(DCP_EINVAL, "sequence batch too large for both strands (%llu sequences, %llu words)", 2ull * n,
                       2ull * (unsigned long long)nwords);
    HIP_TRY(c, hipSetDevice(c->device));
    // a scan of the forward batch may still be running on the stream (and on the size classes' streams, which join
    // it): it reads the arrays that are replaced below
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    void_last_scan(c);
    c->qorder_q0 = c->qorder_q1 = ~0u; // the length order and the word planes belong to the batch that was resident
    std::vector<uint32_t> len(c->seq_len);
    len.insert(len.end(), c->seq_len.begin(), c->seq_len.end());
    uint64_t const total = c->total_len;
    DevBuf<uint32_t> words, woff, dlen;
    DevBuf<float> xt;
    // as in an upload: a failed allocation must not leave the old batch's size paired with new buffers
    auto drop = [&]() {
        c->nseqs = 0, c->strands = 0, c->total_len = 0;
        c->seq_len.clear();
        c->drop_windows();
        c->xt_multi = c->xt_h3 = -1;
    };
#define SEQS_TRY(call)                                                                                                  \
    do                                                                                                                  \
    {                                                                                                                   \
        hipError_t e_ = (call);                                                                                         \
        if (e_ != hipSuccess)                                                                                           \
        {                                                                                                               \
            drop();                                                                                                     \
            return c->fail(e_ == hipErrorOutOfMemory ? DCP_ENOMEM : DCP_EFAIL, "%s: %s", #call, hipGetErrorString(e_)); \
        }                                                                                                               \
    } while (0)
    SEQS_TRY(words.alloc(2u * (size_t)nwords));
    SEQS_TRY(woff.alloc(2u * (size_t)n));
    SEQS_TRY(dlen.alloc(2u * (size_t)n));
    SEQS_TRY(xt.alloc(2u * (size_t)n * DCP_XSTRIDE));
    SEQS_TRY(hipMemcpyAsync(words.p, c->d_seq_words.p, nwords * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    SEQS_TRY(hipMemcpyAsync(woff.p, c->d_seq_woff.p, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    SEQS_TRY(hipMemcpyAsync(dlen.p, c->d_seq_len.p, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    SEQS_TRY(hipMemcpyAsync(xt.p, c->d_xtrans.p, (size_t)n * DCP_XSTRIDE * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    SEQS_TRY((hipError_t)dcp_launch_revcomp(words.p, words.p + nwords, woff.p, dlen.p, n, (uint32_t)nwords, c->stream));
    SEQS_TRY(hipStreamSynchronize(c->stream)); // the old arrays are freed below
#undef SEQS_TRY
    std::swap(c->d_seq_words.p, words.p), std::swap(c->d_seq_words.n, words.n);
    std::swap(c->d_seq_woff.p, woff.p), std::swap(c->d_seq_woff.n, woff.n);
    std::swap(c->d_seq_len.p, dlen.p), std::swap(c->d_seq_len.n, dlen.n);
    std::swap(c->d_xtrans.p, xt.p), std::swap(c->d_xtrans.n, xt.n);
    c->seq_len.swap(len);
    c->nseqs = 2u * n;
    c->strands = 2;
    c->total_len = 2u * total;
    c->xt_multi = c->xt_h3 = -1; // the rows of the reverse half are derived with the next scan's flags
    c->xt64.clear();
    return DCP_OK;
}

// Windows: the resident batch of n sequences is replaced by its W windows (dcp_seq_window_count / _start), in source
// order, then offset order, written on the device from the resident words (dcp_seqs.hip).  Dependent state is
// treated as dcp_gpu_seqs_add_revcomp treats it.
int dcp_gpu_seqs_cut_windows(dcp_gpu_ctx *c, unsigned window, unsigned step)
{
    if (!c) return DCP_EINVAL;
    if (c->nseqs == 0) return c->fail(DCP_EINVAL, "no sequences resident: upload a batch before cutting it into windows");
    if (window < 1u || step < 1u || step > window)
        return c->fail(DCP_EINVAL, "bad window rule (window %u, step %u): window >= 1 and 1 <= step <= window", window, step);
    if (c->strands != 1)
        return c->fail(DCP_EINVAL, "the resident batch already holds both strands: cut the windows first, then add the reverse strand");
    if (c->win_window) return c->fail(DCP_EINVAL, "the resident batch is already cut into windows (window %u, step %u)", c->win_window, c->win_step);
    if (!c->reg_src.empty())
        return c->fail(DCP_EINVAL, "the resident batch is one of regions (dcp_gpu_seqs_cut_regions): windows are cut from an uploaded batch");
    if (c->xt_explicit || !c->xt64.empty())
        return c->fail(DCP_EINVAL, "explicit special transitions are in force: they are per sequence -- set them after "
                                   "dcp_gpu_seqs_cut_windows, one row per window");
    unsigned const n = c->nseqs;
    uint64_t W64 = 0, nwords64 = 0;
    if (dcp_seq_window_plan(c->seq_len.data(), n, window, step, &W64, &nwords64))
        return c->fail(DCP_EINVAL, "sequence batch too large for these windows (%llu windows, %llu words)",
                       (unsigned long long)W64, (unsigned long long)nwords64);
    unsigned const W = (unsigned)W64;
    uint32_t const nwords = (uint32_t)nwords64;
    HIP_TRY(c, hipSetDevice(c->device));
    // a scan of the uncut batch may still be running on the stream: it reads the arrays that are replaced below
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    void_last_scan(c);
    c->qorder_q0 = c->qorder_q1 = ~0u; // the length order and the word planes belong to the batch that was resident
    // the plan: each source's first window and that window's first word (what the index kernel searches), the
    // windows' lengths and the map
    std::vector<uint32_t> first(2u * (size_t)n), len(W), src(W), off(W);
    uint64_t total = 0;
    {
        uint32_t w = 0, words = 0;
        for (unsigned q = 0; q < n; ++q)
        {
            uint32_t const L = c->seq_len[q], wl = L < window ? L : window;
            unsigned const cnt = dcp_seq_window_count(L, window, step);
            first[q] = w, first[(size_t)n + q] = words;
            for (unsigned i = 0; i < cnt; ++i, ++w)
                len[w] = wl, src[w] = q, off[w] = dcp_seq_window_start(L, window, step, i);
            words += cnt * (wl / 16u + 3u);
            total += (uint64_t)cnt * wl;
        }
    }
    DevBuf<uint32_t> words, woff, dlen, dfirst, dsrc, dofs;
    DevBuf<float> xt;
    // as in an upload: a failed allocation must not leave the old batch's size paired with new buffers
    auto drop = [&]() {
        c->nseqs = 0, c->strands = 0, c->total_len = 0;
        c->seq_len.clear();
        c->drop_windows();
        c->xt_multi = c->xt_h3 = -1;
    };
#define SEQS_TRY(call)                                                                                                  \
    do                                                                                                                  \
    {                                                                                                                   \
        hipError_t e_ = (call);                                                                                         \
        if (e_ != hipSuccess)                                                                                           \
        {                                                                                                               \
            drop();                                                                                                     \
            return c->fail(e_ == hipErrorOutOfMemory ? DCP_ENOMEM : DCP_EFAIL, "%s: %s", #call, hipGetErrorString(e_)); \
        }                                                                                                               \
    } while (0)
    SEQS_TRY(words.alloc(nwords));
    SEQS_TRY(woff.alloc(W));
    SEQS_TRY(dlen.alloc(W));
    SEQS_TRY(dsrc.alloc(W));
    SEQS_TRY(dofs.alloc(W));
    SEQS_TRY(dfirst.alloc(2u * (size_t)n));
    SEQS_TRY(xt.alloc((size_t)W * DCP_XSTRIDE));
    SEQS_TRY(hipMemcpyAsync(dfirst.p, first.data(), first.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    dcp_window_args a{};
    a.src_words = c->d_seq_words.p, a.src_woff = c->d_seq_woff.p, a.src_len = c->d_seq_len.p;
    a.wfirst = dfirst.p, a.nwfirst = dfirst.p + n;
    a.words = words.p, a.woff = woff.p, a.len = dlen.p, a.wsrc = dsrc.p, a.wofs = dofs.p;
    a.nsrc = n, a.nwin = W, a.nwords = nwords, a.window = window, a.step = step;
    SEQS_TRY((hipError_t)dcp_launch_windows(&a, c->stream));
    SEQS_TRY(hipStreamSynchronize(c->stream)); // `first` and the old arrays are freed below
#undef SEQS_TRY
    std::swap(c->d_seq_words.p, words.p), std::swap(c->d_seq_words.n, words.n);
    std::swap(c->d_seq_woff.p, woff.p), std::swap(c->d_seq_woff.n, woff.n);
    std::swap(c->d_seq_len.p, dlen.p), std::swap(c->d_seq_len.n, dlen.n);
    std::swap(c->d_xtrans.p, xt.p), std::swap(c->d_xtrans.n, xt.n);
    c->seq_len.swap(len);
    c->win_src.swap(src), c->win_off.swap(off);
    c->win_window = window, c->win_step = step;
    c->nseqs = W;
    c->total_len = total;
    c->xt_multi = c->xt_h3 = -1; // the windows' rows are derived with the next scan's flags
    c->xt64.clear();
    return DCP_OK;
}

// A random batch (dcp_calib.hip): nseqs sequences of len bases written on the device into new arrays, which then replace
// the resident ones as in dcp_gpu_seqs_add_revcomp.  Every refusal comes before anything is touched.
int dcp_gpu_seqs_random(dcp_gpu_ctx *c, unsigned nseqs, unsigned len, uint64_t seed, double const probs[4])
{
    if (!c) return DCP_EINVAL;
    if (nseqs == 0 || len == 0) return c->fail(DCP_EINVAL, "a random batch needs sequences and bases (%u sequences of %u)", nseqs, len);
    uint32_t thr[3];
    if (dcp_seq_random_thresholds(probs, thr))
        return c->fail(DCP_EINVAL, "bad base probabilities: four finite values >= 0 that sum to 1");
    uint64_t const nwords = (uint64_t)nseqs * (len / 16u + 3u);
    if (nwords > 0xffffffffull)
        return c->fail(DCP_EINVAL, "random batch too large (%u sequences, %llu words)", nseqs, (unsigned long long)nwords);
    HIP_TRY(c, hipSetDevice(c->device));
    // a scan of the batch that is replaced may still be running on the stream: it reads the arrays freed below
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::vector<uint32_t> lens;
    try
    {
        lens.assign(nseqs, len);
    }
    catch (std::bad_alloc const &)
    {
        return c->fail(DCP_ENOMEM, "out of host memory for %u sequence lengths", nseqs);
    }
    for (hipEvent_t &e : c->ev_calib)
        if (!e) HIP_TRY(c, hipEventCreate(&e));
    void_last_scan(c);
    c->qorder_q0 = c->qorder_q1 = ~0u; // the length order and the word planes belong to the batch that was resident
    DevBuf<uint32_t> words, woff, dlen;
    DevBuf<float> xt;
    // as in an upload: a failed allocation must not leave the old batch's size paired with new buffers
    auto drop = [&]() {
        c->nseqs = 0, c->strands = 0, c->total_len = 0;
        c->seq_len.clear();
        c->drop_windows();
        c->xt_multi = c->xt_h3 = -1;
        c->xt_explicit = false;
        c->xt64.clear();
    };
#define SEQS_TRY(call)                                                                                                  \
    do                                                                                                                  \
    {                                                                                                                   \
        hipError_t e_ = (call);                                                                                         \
        if (e_ != hipSuccess)                                                                                           \
        {                                                                                                               \
            drop();                                                                                                     \
            return c->fail(e_ == hipErrorOutOfMemory ? DCP_ENOMEM : DCP_EFAIL, "%s: %s", #call, hipGetErrorString(e_)); \
        }                                                                                                               \
    } while (0)
    SEQS_TRY(words.alloc((size_t)nwords));
    SEQS_TRY(woff.alloc(nseqs));
    SEQS_TRY(dlen.alloc(nseqs));
    SEQS_TRY(xt.alloc((size_t)nseqs * DCP_XSTRIDE));
    SEQS_TRY(hipEventRecord(c->ev_calib[0], c->stream));
    SEQS_TRY((hipError_t)dcp_launch_random(words.p, woff.p, dlen.p, nseqs, len, seed, thr, c->stream));
    SEQS_TRY(hipEventRecord(c->ev_calib[1], c->stream));
    SEQS_TRY(hipStreamSynchronize(c->stream)); // the old arrays are freed below
#undef SEQS_TRY
    c->calib_timed[0] = true;
    std::swap(c->d_seq_words.p, words.p), std::swap(c->d_seq_words.n, words.n);
    std::swap(c->d_seq_woff.p, woff.p), std::swap(c->d_seq_woff.n, woff.n);
    std::swap(c->d_seq_len.p, dlen.p), std::swap(c->d_seq_len.n, dlen.n);
    std::swap(c->d_xtrans.p, xt.p), std::swap(c->d_xtrans.n, xt.n);
    c->seq_len.swap(lens);
    c->drop_windows(); // a new batch is uncut
    c->nseqs = nseqs;
    c->strands = 1;
    c->total_len = (uint64_t)nseqs * len;
    c->xt_multi = c->xt_h3 = -1;
    c->xt_explicit = false;
    c->xt64.clear();
    return DCP_OK;
}

int dcp_gpu_seqs_windows(dcp_gpu_ctx const *c, unsigned *window, unsigned *step)
{
    bool const cut = c && c->nseqs && c->win_window;
    if (window) *window = cut ? c->win_window : 0u;
    if (step) *step = cut ? c->win_step : 0u;
    return cut ? 1 : 0;
}

int dcp_gpu_seqs_window_map(dcp_gpu_ctx *c, uint32_t *src, uint32_t *off, unsigned cap)
{
    if (!c) return DCP_EINVAL;
    if (!c->nseqs || !c->win_window) return c->fail(DCP_EINVAL, "the resident batch is not cut into windows");
    size_t const W = c->win_src.size();
    if (cap < W || !src || !off) return c->fail(DCP_ENOMEM, "the batch has %zu windows: the buffers hold %u", W, cap);
    std::memcpy(src, c->win_src.data(), W * sizeof(uint32_t));
    std::memcpy(off, c->win_off.data(), W * sizeof(uint32_t));
    return DCP_OK;
}

// Regions: the resident batch is replaced by n stretches of its sequences, each on the strand the list names, written
// on the device from the resident words (dcp_seqs.hip).  The host holds the list, so the new index is computed here
// and uploaded with the map.  Dependent state is treated as dcp_gpu_seqs_cut_windows treats it.
int dcp_gpu_seqs_cut_regions(dcp_gpu_ctx *c, uint32_t const *src, uint32_t const *begin, uint32_t const *len,
                             uint8_t const *minus, unsigned n)
{
    if (!c) return DCP_EINVAL;
    if (c->nseqs == 0) return c->fail(DCP_EINVAL, "no sequences resident: upload a batch before cutting regions out of it");
    if (c->win_window) return c->fail(DCP_EINVAL, "the resident batch is cut into windows (window %u, step %u): regions are cut from an uploaded batch", c->win_window, c->win_step);
    if (c->strands != 1) return c->fail(DCP_EINVAL, "the resident batch holds both strands: regions are cut from an uploaded batch, each on the strand its list names");
    if (!c->reg_src.empty()) return c->fail(DCP_EINVAL, "the resident batch is already one of regions (%zu of them)", c->reg_src.size());
    if (c->xt_explicit || !c->xt64.empty())
        return c->fail(DCP_EINVAL, "explicit special transitions are in force: they are per sequence -- set them after "
                                   "dcp_gpu_seqs_cut_regions, one row per region");
    if (n == 0 || !src || !begin || !len || !minus) return c->fail(DCP_EINVAL, "an empty list of regions, or a null pointer");
    uint64_t nwords64 = 0, total = 0;
    for (unsigned i = 0; i < n; ++i)
    {
        if (src[i] >= c->nseqs || len[i] == 0 || (uint64_t)begin[i] + len[i] > c->seq_len[src[i]])
            return c->fail(DCP_EINVAL, "region %u (source %u, bases %u + %u) is empty or lies outside its source (%u sequences resident, %u bases)",
                           i, src[i], begin[i], len[i], c->nseqs, src[i] < c->nseqs ? c->seq_len[src[i]] : 0u);
        nwords64 += len[i] / 16u + 3u; // n < 2^32 terms below 2^28 + 3: no wrap
        total += len[i];
    }
    if (nwords64 > 0xffffffffull)
        return c->fail(DCP_EINVAL, "sequence batch too large for these regions (%u regions, %llu words)", n, (unsigned long long)nwords64);
    uint32_t const nwords = (uint32_t)nwords64;
    HIP_TRY(c, hipSetDevice(c->device));
    // a scan of the uncut batch may still be running on the stream: it reads the arrays that are replaced below
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    void_last_scan(c);
    c->qorder_q0 = c->qorder_q1 = ~0u; // the length order and the word planes belong to the batch that was resident
    // the new index and the map, in one array: woff, len, source, first base, strand
    std::vector<uint32_t> plan(5u * (size_t)n);
    {
        uint32_t at = 0;
        for (unsigned i = 0; i < n; ++i)
        {
            plan[i] = at, plan[(size_t)n + i] = len[i], plan[2u * (size_t)n + i] = src[i];
            plan[3u * (size_t)n + i] = begin[i], plan[4u * (size_t)n + i] = minus[i] ? 1u : 0u;
            at += len[i] / 16u + 3u;
        }
    }
    DevBuf<uint32_t> words, woff, dlen, dmap;
    DevBuf<float> xt;
    // as in an upload: a failed allocation must not leave the old batch's size paired with new buffers
    auto drop = [&]() {
        c->nseqs = 0, c->strands = 0, c->total_len = 0;
        c->seq_len.clear();
        c->drop_windows();
        c->xt_multi = c->xt_h3 = -1;
    };
#define SEQS_TRY(call)                                                                                                  \
    do                                                                                                                  \
    {                                                                                                                   \
        hipError_t e_ = (call);                                                                                         \
        if (e_ != hipSuccess)                                                                                           \
        {                                                                                                               \
            drop();                                                                                                     \
            return c->fail(e_ == hipErrorOutOfMemory ? DCP_ENOMEM : DCP_EFAIL, "%s: %s", #call, hipGetErrorString(e_)); \
        }                                                                                                               \
    } while (0)
    SEQS_TRY(words.alloc(nwords));
    SEQS_TRY(woff.alloc(n));
    SEQS_TRY(dlen.alloc(n));
    SEQS_TRY(dmap.alloc(3u * (size_t)n));
    SEQS_TRY(xt.alloc((size_t)n * DCP_XSTRIDE));
    SEQS_TRY(hipMemcpyAsync(woff.p, plan.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    SEQS_TRY(hipMemcpyAsync(dlen.p, plan.data() + n, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    SEQS_TRY(hipMemcpyAsync(dmap.p, plan.data() + 2u * (size_t)n, 3u * (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    dcp_region_args a{};
    a.src_words = c->d_seq_words.p, a.src_woff = c->d_seq_woff.p;
    a.words = words.p, a.woff = woff.p, a.len = dlen.p;
    a.rsrc = dmap.p, a.rbegin = dmap.p + n, a.rminus = dmap.p + 2u * (size_t)n;
    a.n = n, a.nwords = nwords;
    SEQS_TRY((hipError_t)dcp_launch_regions(&a, c->stream));
    SEQS_TRY(hipStreamSynchronize(c->stream)); // `plan`, the map and the old arrays are freed below
#undef SEQS_TRY
    std::swap(c->d_seq_words.p, words.p), std::swap(c->d_seq_words.n, words.n);
    std::swap(c->d_seq_woff.p, woff.p), std::swap(c->d_seq_woff.n, woff.n);
    std::swap(c->d_seq_len.p, dlen.p), std::swap(c->d_seq_len.n, dlen.n);
    std::swap(c->d_xtrans.p, xt.p), std::swap(c->d_xtrans.n, xt.n);
    c->seq_len.assign(len, len + n);
    c->reg_src.assign(src, src + n), c->reg_begin.assign(begin, begin + n);
    c->reg_minus.resize(n);
    for (unsigned i = 0; i < n; ++i)
        c->reg_minus[i] = minus[i] ? 1u : 0u;
    c->nseqs = n;
    c->total_len = total;
    c->xt_multi = c->xt_h3 = -1; // the regions' rows are derived with the next scan's flags
    c->xt64.clear();
    return DCP_OK;
}

unsigned dcp_gpu_seqs_regions(dcp_gpu_ctx const *c) { return c && c->nseqs ? (unsigned)c->reg_src.size() : 0u; }

int dcp_gpu_seqs_region_map(dcp_gpu_ctx *c, uint32_t *src, uint32_t *begin, uint8_t *minus, unsigned cap)
{
    if (!c) return DCP_EINVAL;
    if (!c->nseqs || c->reg_src.empty()) return c->fail(DCP_EINVAL, "the resident batch is not one of regions");
    size_t const n = c->reg_src.size();
    if (cap < n || !src || !begin || !minus) return c->fail(DCP_ENOMEM, "the batch has %zu regions: the buffers hold %u", n, cap);
    std::memcpy(src, c->reg_src.data(), n * sizeof(uint32_t));
    std::memcpy(begin, c->reg_begin.data(), n * sizeof(uint32_t));
    std::memcpy(minus, c->reg_minus.data(), n);
    return DCP_OK;
}

// the words of resident sequence q, as the device holds them
static int fetch_seq_words(dcp_gpu_ctx *c, unsigned q, std::vector<uint32_t> &w)
{
    HIP_TRY(c, hipSetDevice(c->device));
    uint32_t woff = 0;
    HIP_TRY(c, hipMemcpy(&woff, c->d_seq_woff.p + q, sizeof woff, hipMemcpyDeviceToHost));
    w.resize((size_t)c->seq_len[q] / 16u + 3u);
    if ((uint64_t)woff + w.size() > c->d_seq_words.n) return c->fail(DCP_EFAIL, "sequence %u lies outside the resident words", q);
    HIP_TRY(c, hipMemcpy(w.data(), c->d_seq_words.p + woff, w.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return DCP_OK;
}

int dcp_gpu_seqs_fetch(dcp_gpu_ctx *c, unsigned q, uint8_t *ids, unsigned cap, unsigned *len)
{
    if (!c) return DCP_EINVAL;
    if (q >= c->nseqs) return c->fail(DCP_EINVAL, "sequence %u is not resident (%u are)", q, c->nseqs);
    uint32_t const L = c->seq_len[q];
    if (len) *len = L;
    if (cap < L || !ids) return c->fail(DCP_ENOMEM, "sequence %u has %u symbols: the buffer holds %u", q, L, cap);
    std::vector<uint32_t> w;
    if (int rc = fetch_seq_words(c, q, w)) return rc;
    for (uint32_t i = 0; i < L; ++i)
        ids[i] = (uint8_t)((w[i >> 4] >> ((i & 15u) * 2u)) & 3u);
    return DCP_OK;
}

#ifdef DCP_TEST_HOOKS
int dcp_gpu_test_fetch_seq_words(dcp_gpu_ctx *c, unsigned q, uint32_t *out, unsigned cap, unsigned *nwords)
{
    if (!c) return DCP_EINVAL;
    if (q >= c->nseqs) return c->fail(DCP_EINVAL, "sequence %u is not resident (%u are)", q, c->nseqs);
    unsigned const nw = c->seq_len[q] / 16u + 3u;
    if (nwords) *nwords = nw;
    if (cap < nw || !out) return DCP_ENOMEM;
    std::vector<uint32_t> w;
    if (int rc = fetch_seq_words(c, q, w)) return rc;
    std::memcpy(out, w.data(), nw * sizeof(uint32_t));
    return DCP_OK;
}
#endif

// ---------------------------------------------------------------------------
// Scan
// ---------------------------------------------------------------------------
// the float DB's special transitions: resident for the whole batch, rebuilt when the flags change
static int ensure_xtrans(dcp_gpu_ctx *c, int multi_hits, int hmmer3_compat)
{
    if (c->xt_explicit) return DCP_OK;
    if (c->xt_multi == !!multi_hits && c->xt_h3 == !!hmmer3_compat) return DCP_OK;
    std::vector<uint32_t> seqs(c->nseqs);
    std::iota(seqs.begin(), seqs.end(), 0u);
    std::vector<float> xt;
    if (int rc = fill_xtrans(c, seqs, multi_hits, hmmer3_compat, DCP_XSTRIDE, xt)) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->d_xtrans.p, xt.data(), xt.size() * sizeof(float),
                              hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->xt_multi = !!multi_hits;
    c->xt_h3 = !!hmmer3_compat;
    return DCP_OK;
}

int dcp_gpu_seqs_set_xtrans(dcp_gpu_ctx *c, float const *xt, unsigned nseqs)
{
    if (!c) return DCP_EINVAL;
    if (!xt || nseqs == 0 || nseqs != c->nseqs) return c->fail(DCP_EINVAL, "xtrans must cover the resident sequences");
    HIP_TRY(c, hipSetDevice(c->device));
    std::vector<float> buf((size_t)nseqs * DCP_XSTRIDE, 0.0f);
    for (unsigned q = 0; q < nseqs; ++q)
        for (int i = 0; i < DCP_NXTRANS; ++i)
        {
            float const v = xt[(size_t)q * DCP_NXTRANS + i];
            if (is_nan(v)) return c->fail(DCP_EINVAL, "NaN special transition");
            buf[(size_t)q * DCP_XSTRIDE + i] = v;
        }
    HIP_TRY(c, hipMemcpy(c->d_xtrans.p, buf.data(), buf.size() * sizeof(float), hipMemcpyHostToDevice));
    c->xt_explicit = true;
    c->xt64.clear(); // one explicit set holds: the last one given
    c->xt_multi = c->xt_h3 = -1;
    void_forward_dense(c);
    return DCP_OK;
}

int dcp_gpu_seqs_set_xtrans64(dcp_gpu_ctx *c, double const *xt, unsigned nseqs)
{
    if (!c) return DCP_EINVAL;
    if (!xt || nseqs == 0 || nseqs != c->nseqs) return c->fail(DCP_EINVAL, "xtrans must cover the resident sequences");
    for (size_t i = 0; i < (size_t)nseqs * DCP_NXTRANS; ++i)
        if (is_nan(xt[i])) return c->fail(DCP_EINVAL, "NaN special transition");
    c->xt64.assign(xt, xt + (size_t)nseqs * DCP_NXTRANS);
    c->xt_explicit = false; // one explicit set holds: the last one given
    c->xt_multi = c->xt_h3 = -1;
    void_forward_dense(c);
    return DCP_OK;
}

int dcp_gpu_scan(dcp_gpu_ctx *c, struct dcp_scan_params const *prm)
{
    if (!c) return DCP_EINVAL;
    return dcp_gpu_scan_range(c, prm, 0, c->nseqs);
}

int dcp_gpu_set_lrt_threshold64(dcp_gpu_ctx *c, double lrt_threshold64)
{
    if (!c) return DCP_EINVAL;
    c->lrt_threshold64 = lrt_threshold64;
    return DCP_OK;
}

int dcp_gpu_set_hit_buffer(dcp_gpu_ctx *c, void *hits_dev, unsigned cap, void *nhits_dev)
{
    if (!c) return DCP_EINVAL;
    return set_hit_buffer(c, c->res, hits_dev, cap, nhits_dev);
}

int dcp_gpu_hit_buffer(dcp_gpu_ctx *c, void **hits_dev, void **nhits_dev, unsigned *cap)
{
    if (!c || !hits_dev || !nhits_dev || !cap) return DCP_EINVAL;
    if (!c->last.scanned) return c->fail(DCP_EINVAL, "no scan yet");
    if (c->last.f64) return c->fail(DCP_EINVAL, "the last scan ran on a double DB: its hits are struct dcp_hit64 (dcp_gpu_fetch_hits64)");
    return hit_buffer(c->res, hits_dev, nhits_dev, cap);
}

int dcp_gpu_set_hit_buffer64(dcp_gpu_ctx *c, void *hits_dev, unsigned cap, void *nhits_dev)
{
    if (!c) return DCP_EINVAL;
    return set_hit_buffer(c, c->f64.res, hits_dev, cap, nhits_dev);
}

int dcp_gpu_hit_buffer64(dcp_gpu_ctx *c, void **hits_dev, void **nhits_dev, unsigned *cap)
{
    if (!c || !hits_dev || !nhits_dev || !cap) return DCP_EINVAL;
    if (!c->last.scanned) return c->fail(DCP_EINVAL, "no scan yet");
    if (!c->last.f64) return c->fail(DCP_EINVAL, "the last scan ran on a float DB: its hits are struct dcp_hit (dcp_gpu_hit_buffer)");
    return hit_buffer(c->f64.res, hits_dev, nhits_dev, cap);
}

// ---- dynamic batching of the query-lane kernels (BASELINE configs[4]) ----------------------------
// The queries of a scan, sorted by length, are cut into GROUPS of 64 consecutive ones -- what one wavefront sweeps
// together, one lane each, for as many rows as its longest member has.  A block has `slots` wavefront slots (4: the
// 256 lanes of a stage; 1 for the three-independent-wavefronts variant) and sits through a tile until its slowest
// slot is done, so a block of four CONSECUTIVE groups (rounds 1-3) wastes (longest - mean) of its slots' time:
// a 1 000-query batch of 100 nt .. 10 kbp ran at 0.6 of the rate of a uniform one.  Here each slot holds a LIST of
// groups, swept one after the other per tile, and the groups are packed into slots so that all slots of all blocks
// carry about the same number of rows (longest-processing-time-first; the block count is the one that wastes least).
// Uniform batches come out as before: one group per slot.
struct QlPlan
{
    std::vector<dcp_ql_group> groups;  // in slot order
    std::vector<uint32_t> slot_first;  // [nqb * slots + 1]
    std::vector<uint32_t> block_rows;  // [nqb] rows of the block's planes: its longest slot
    unsigned nqb = 0;
    unsigned plane_rows = 0;           // max over blocks
    uint64_t sum_block_rows = 0;       // what a tile costs, summed over the blocks: the cost model's figure
    unsigned busy_slots = 0;           // slots of the first block that hold a group (cost model)
};
// len_sorted: the lengths in ascending order (entry i belongs to qorder[i]).
static QlPlan plan_query_groups(unsigned const *len_sorted, unsigned nq, unsigned slots)
{
    QlPlan pl;
    unsigned const ng = (nq + 63u) / 64u;
    struct G
    {
        unsigned first, n, lmax, rows;
    };
    std::vector<G> gs(ng);
    uint64_t sum_rows = 0;
    unsigned max_rows = 0;
    // full groups from the LONG end: if nq is not a multiple of 64 the partial group is the one of the shortest
    // queries -- idle lanes then cost the fewest rows (the other way round, a 965-query pass of 100 nt .. 10 kbp spent
    // a slot's 10 000 rows on the five longest queries: profiles/r04/host_scan_probe.txt)
    unsigned const rem = nq % 64u;
    for (unsigned g = 0; g < ng; ++g)
    {
        unsigned const first = rem == 0u ? g * 64u : (g == 0u ? 0u : rem + (g - 1u) * 64u);
        unsigned const n = rem != 0u && g == 0u ? rem : 64u;
        unsigned const lmax = len_sorted[first + n - 1u];
        gs[g] = G{first, n, lmax, dcp_qlane_group_rows(lmax)};
        sum_rows += gs[g].rows;
        max_rows = std::max(max_rows, gs[g].rows);
    }
    // longest first into the least loaded slot; slots sorted by load, `slots` consecutive ones make a block
    auto pack = [&](unsigned nqb, std::vector<std::vector<unsigned>> &slot_groups, std::vector<uint64_t> &load) {
        unsigned const S = nqb * slots;
        slot_groups.assign(S, {});
        load.assign(S, 0);
        typedef std::pair<uint64_t, unsigned> LS; // (load, slot): least loaded on top, lowest slot first on ties
        std::priority_queue<LS, std::vector<LS>, std::greater<LS>> heap;
        for (unsigned i = 0; i < S; ++i)
            heap.push(LS(0, i));
        for (unsigned g = ng; g-- > 0;) // ascending lengths: the last group is the longest
        {
            LS top = heap.top();
            heap.pop();
            slot_groups[top.second].push_back(g);
            load[top.second] += gs[g].rows;
            heap.push(LS(load[top.second], top.second));
        }
        std::vector<unsigned> order(S);
        for (unsigned i = 0; i < S; ++i)
            order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](unsigned x, unsigned y) { return load[x] > load[y]; });
        std::vector<std::vector<unsigned>> sg(S);
        std::vector<uint64_t> ld(S);
        for (unsigned i = 0; i < S; ++i)
            sg[i] = std::move(slot_groups[order[i]]), ld[i] = load[order[i]];
        slot_groups.swap(sg), load.swap(ld);
        uint64_t cost = 0;
        for (unsigned b = 0; b < nqb; ++b)
            cost += load[(size_t)b * slots]; // the block's longest slot
        return cost;
    };
    // candidate block counts around (all rows) / (slots x the longest group): fewer blocks balance better, more blocks
    // keep more tasks in flight; take the cheapest, the larger count on ties
    unsigned const cap = (ng + slots - 1u) / slots; // one group per slot: more blocks than that only adds empty slots
    uint64_t const denom = (uint64_t)slots * max_rows;
    unsigned const lo = (unsigned)std::min<uint64_t>(std::max<uint64_t>(sum_rows / denom, 1), cap);
    unsigned const hi = (unsigned)std::min<uint64_t>(std::max<uint64_t>((sum_rows + denom - 1u) / denom, 1), cap);
    std::vector<std::vector<unsigned>> best_sg, sg;
    std::vector<uint64_t> best_ld, ld;
    uint64_t best_cost = ~0ull;
    unsigned best_nqb = 0;
    for (unsigned nqb = lo; nqb <= hi; ++nqb)
    {
        uint64_t const cost = pack(nqb, sg, ld);
        if (cost <= best_cost) best_cost = cost, best_nqb = nqb, best_sg.swap(sg), best_ld.swap(ld);
    }
    pl.nqb = best_nqb;
    pl.sum_block_rows = best_cost;
    pl.slot_first.assign((size_t)best_nqb * slots + 1u, 0);
    pl.block_rows.assign(best_nqb, 0);
    for (unsigned sidx = 0; sidx < best_nqb * slots; ++sidx)
    {
        pl.slot_first[sidx] = (uint32_t)pl.groups.size();
        uint32_t rowbase = 0;
        for (unsigned g : best_sg[sidx])
        {
            pl.groups.push_back(dcp_ql_group{gs[g].first, gs[g].n, rowbase, gs[g].lmax});
            rowbase += gs[g].rows;
        }
        pl.block_rows[sidx / slots] = std::max<uint32_t>(pl.block_rows[sidx / slots], rowbase);
        if (sidx < slots && rowbase) ++pl.busy_slots;
    }
    pl.slot_first.back() = (uint32_t)pl.groups.size();
    for (unsigned b = 0; b < best_nqb; ++b)
        pl.plane_rows = std::max(pl.plane_rows, pl.block_rows[b]);
    return pl;
}

// The queries [q_begin, q_end) by rising length (stable; entries relative to q_begin), their lengths in that order and
// the plan that packs them into blocks of `slots` wavefront slots.
namespace
{
struct SortedQueries
{
    std::vector<uint32_t> order;
    std::vector<unsigned> len;
    QlPlan plan;
};
} // namespace
static SortedQueries sorted_query_plan(dcp_gpu_ctx const *c, unsigned q_begin, unsigned q_end, unsigned slots)
{
    unsigned const nq = q_end - q_begin;
    SortedQueries s;
    s.order.resize(nq);
    std::iota(s.order.begin(), s.order.end(), 0u);
    std::stable_sort(s.order.begin(), s.order.end(),
                     [&](uint32_t x, uint32_t y) { return c->seq_len[q_begin + x] < c->seq_len[q_begin + y]; });
    s.len.resize(nq);
    for (unsigned i = 0; i < nq; ++i)
        s.len[i] = c->seq_len[q_begin + s.order[i]];
    s.plan = plan_query_groups(s.len.data(), nq, slots);
    return s;
}

// The plan as plain arrays (host only; tests/test_query_slots.py checks its invariants on the CPU).
extern "C" int dcp_plan_query_slots(unsigned const *len_sorted, unsigned nq, unsigned slots_per_block, unsigned *nblocks,
                                    unsigned long long *sum_block_rows, unsigned *plane_rows, unsigned *groups4,
                                    unsigned group_cap, unsigned *slot_first, unsigned slot_cap)
{
    if (!len_sorted || nq == 0 || (slots_per_block != 1u && slots_per_block != 4u) || !nblocks) return DCP_EINVAL;
    for (unsigned i = 1; i < nq; ++i)
        if (len_sorted[i] < len_sorted[i - 1]) return DCP_EINVAL;
    QlPlan const pl = plan_query_groups(len_sorted, nq, slots_per_block);
    *nblocks = pl.nqb;
    if (sum_block_rows) *sum_block_rows = pl.sum_block_rows;
    if (plane_rows) *plane_rows = pl.plane_rows;
    if (groups4)
    {
        if (group_cap < pl.groups.size()) return DCP_ENOMEM;
        std::memcpy(groups4, pl.groups.data(), pl.groups.size() * sizeof(dcp_ql_group));
    }
    if (slot_first)
    {
        if (slot_cap < pl.slot_first.size()) return DCP_ENOMEM;
        std::memcpy(slot_first, pl.slot_first.data(), pl.slot_first.size() * sizeof(uint32_t));
    }
    return DCP_OK;
}

// Which grid-mode row-sweep kernel scores one size class against `nchunks` queries: rows of the emission table
// each block stages in LDS and wavefronts per block (dcp_kernels.hip).  Measured on the 20 000-profile DB
// (profiles/r03/rowsweep_variants.txt, ms per scan for 1 .. 1 000 queries):
//   * small batches stream the tables from HBM (an XCD's 512 wavefront slots work on far more profiles than its
//     4 MB L2 holds tables of), so what a block keeps in LDS is traffic saved: with the three-base rows staged
//     as well, 8 queries take 49 ms instead of 57, 16: 80 instead of 99, 32: 142 instead of 160 -- provided the
//     block is wide enough that the 21.5 KB x R image does not cost wavefront slots (one profile per block);
//   * from about 40 queries on the L2 serves the rows and the 20-row image with narrower blocks wins (64 queries:
//     259 vs 270 ms); wide blocks start and drain together, which a long launch pays for (1 000 queries: 3.65 s
//     with 4 wavefronts per block, 3.83 with 8, 4.14 with 16).
static void rowsweep_variant(dcp_gpu_ctx const *c, int R, int W, unsigned nchunks, int *stg, unsigned *bw, int *pf)
{
    *pf = 0;
    if (W != 1)
    {
        *stg = 0, *bw = 1;
        return;
    }
    // blocks of equal width: 24 queries are two blocks of 12 wavefronts, not 16 + 8
    auto balanced = [&](unsigned maxw) {
        unsigned const nb = (nchunks + maxw - 1u) / maxw;
        return (nchunks + nb - 1u) / nb;
    };
    int g = 20;
    unsigned w = balanced(nchunks <= 56u ? 8u : 4u); // 48 queries: 198 ms with 8 wavefronts per block, 205 with 4; 64: 256 / 252
    unsigned const max84 = dcp_rowsweep_max_block_waves(R, W, 84);
    if (nchunks >= 6u && nchunks <= 36u && max84 != 0u)
    {
        unsigned const w84 = balanced(max84);
        unsigned const slots = dcp_rowsweep_max_block_waves(R, W, 84); // wavefronts of this class a CU runs at the kernel's register count
        unsigned const blocks = (160u * 1024u) / dcp_rowsweep_stage_bytes(R, 84);
        // the image may cost up to half of them: such a batch waits for HBM, not for issue slots (8 queries with
        // the R = 4 class at 8 of 16 wavefronts per CU: 49 ms; with that class on the 20-row image: 51)
        if (std::min(blocks * w84, slots) * 2u >= slots) g = 84, w = w84;
    }
    bool const forced = c->rs_force_stg >= 0 && (c->rs_force_R == 0 || c->rs_force_R == R) &&
                        dcp_rowsweep_max_block_waves(R, W, c->rs_force_stg) != 0u;
    if (forced)
    {
        g = c->rs_force_stg;
        w = g == 0 ? 4u : std::min(std::min(c->rs_force_bw ? c->rs_force_bw : 4u, dcp_rowsweep_max_block_waves(R, W, g)), nchunks);
    }
    *stg = g, *bw = std::max(1u, w);
    // two rows of prefetch: the batches that wait for HBM (the 84-row variants' range, and below it)
    *pf = g > 0 && nchunks <= 36u;
    if (forced && g > 0) *pf = c->rs_force_pf;
}

// Boundary columns of the f64 DB's segmented launch group, for the npairs pairs of it that a scan or a traceback round
// sweeps: 5 doubles per row and wavefront, at most 1 GiB of them; the wavefronts stride over the pairs.
struct F64Seg
{
    uint64_t col_stride = 0, waves = 0;
};
static int f64_seg_columns(dcp_gpu_ctx *c, uint32_t lmax, uint64_t npairs, F64Seg *seg)
{
    seg->col_stride = 5ull * ((uint64_t)lmax + 1u);
    seg->waves = npairs ? std::min<uint64_t>(npairs, std::max<uint64_t>(1u, ((uint64_t)1 << 27) / seg->col_stride)) : 0;
    HIP_TRY(c, c->f64.d_col.reserve(seg->waves * seg->col_stride));
    return DCP_OK;
}

// The geometry of launch group g of an f64 DB over `count` pairs: one wavefront per pair, at most `cap` (2^24: 2^22
// blocks of 256); the segmented group strides over its pairs with one boundary column per wavefront (seg:
// f64_seg_columns' answer for those pairs, never more wavefronts than pairs or than 2^24).  Returns the wavefronts.
static unsigned f64_group_geometry(dcp_gpu_ctx const *c, int g, uint64_t count, F64Seg const &seg, dcp_f64_scan_args &a,
                                   uint64_t cap = 1ull << 24)
{
    a.col = g == 3 ? c->f64.d_col.p : nullptr;
    a.col_stride = g == 3 ? seg.col_stride : 0;
    uint64_t const waves = std::min(count, cap);
    return (unsigned)(g == 3 ? std::min(waves, seg.waves) : waves);
}

// What every driver that takes explicit special transitions refuses: the set of the other precision.
static int check_xtrans_precision(dcp_gpu_ctx *c)
{
    if (c->precision == 64 && c->xt_explicit)
        return c->fail(DCP_EINVAL, "the explicit special transitions are float: a double DB takes them from dcp_gpu_seqs_set_xtrans64");
    if (c->precision != 64 && !c->xt64.empty())
        return c->fail(DCP_EINVAL, "the explicit special transitions are double: a float DB takes them from dcp_gpu_seqs_set_xtrans");
    return DCP_OK;
}

// The bounds of a list of n (sequence, profile) pairs, `stride` words from one pair's indices to the next's (1: two
// arrays; a traceback's hit records: the record's words).  `hit`: the tracebacks' short message.
static_assert(sizeof(dcp_hit) % sizeof(uint32_t) == 0 && sizeof(dcp_hit64) % sizeof(uint32_t) == 0, "hit records are whole words");
static int check_pairs(dcp_gpu_ctx *c, uint32_t const *seq_idx, uint32_t const *profile_idx, size_t stride, unsigned n, bool hit)
{
    for (unsigned i = 0; i < n; ++i)
    {
        uint32_t const s = seq_idx[i * stride], p = profile_idx[i * stride];
        if (s < c->nseqs && p < c->nprof) continue;
        char who[64] = "", batch[32] = "", db[32] = "";
        if (!hit)
        {
            snprintf(who, sizeof who, " (sequence %u, profile %u)", s, p);
            snprintf(batch, sizeof batch, " (%u sequences)", c->nseqs);
            snprintf(db, sizeof db, " (%u profiles)", c->nprof);
        }
        return c->fail(DCP_EINVAL, "%s %u%s is outside the resident batch%s / DB%s", hit ? "hit" : "pair", i, who, batch, db);
    }
    return DCP_OK;
}

// One scan is outstanding per context: results (hits, scores, redo lists) are those of the LAST scan.  A scan enqueued
// while the one before it still has unchecked redo lists or ring word first completes that one (its overflow re-run
// included), so nothing of it is silently half done.
static int complete_pending_scan(dcp_gpu_ctx *c)
{
    bool const pending = c->last.redo_pending || c->last.redo_pending64 || c->last.ring_check_pending;
    return pending ? finish_scan(c) : DCP_OK;
}

// The hooks build's records of what launch_rowsweep_scan did with size class k (dcp_gpu_test_last_rowsweep_plan) and of
// a pair-mode launch (dcp_gpu_test_last_pair_launches); nothing in the shipped library.
static inline void note_rowsweep_plan(dcp_gpu_ctx *c, int k, unsigned path, int stage, unsigned waves, int prefetch, unsigned chunk,
                                      bool flagged_rest)
{
#ifdef DCP_TEST_HOOKS
    c->last.rs_plan[k] = {path, (unsigned)stage, waves, (unsigned)prefetch, chunk, flagged_rest ? 1u : 0u};
#else
    (void)c, (void)k, (void)path, (void)stage, (void)waves, (void)prefetch, (void)chunk, (void)flagged_rest;
#endif
}
static inline void note_pair_launch(dcp_gpu_ctx *c, unsigned kind, unsigned precision, unsigned a, unsigned b, unsigned units,
                                    unsigned tpb, unsigned cap)
{
#ifdef DCP_TEST_HOOKS
    c->last.pair_launches.push_back({kind, precision, a, b, units, tpb, cap});
#else
    (void)c, (void)kind, (void)precision, (void)a, (void)b, (void)units, (void)tpb, (void)cap;
#endif
}

// A scan of the resident double DB: viterbi64_kernel<R> per launch group (dcp_f64.hip), or -- kernel 4 -- the
// query-lane kernel (dcp_f64_qlane.hip) with the row sweep behind it on the pairs it could not finish; the LRT
// filter in their epilogues, results in the f64 buffers.
static int scan64(dcp_gpu_ctx *c, struct dcp_scan_params const *prm, unsigned q_begin, unsigned q_end)
{
    if (prm->kernel != 0 && prm->kernel != 1 && prm->kernel != 4)
        return c->fail(DCP_EINVAL, "a double DB is scanned by the f64 row sweep (kernel 0 or 1) or the f64 query-lane kernel (4), not %d", prm->kernel);
    if (int rc = check_xtrans_precision(c)) return rc;
    auto &F = c->f64;
    // one scan is outstanding per context: a query-lane scan whose redo counters have not been looked at is
    // completed first (its overflow re-run included)
    if (int rc = complete_pending_scan(c)) return rc;
    bool const qlane = prm->kernel == 4;
    c->last = LastScan{};
    c->last.f64 = true;
    c->last.prm = *prm;
    c->last.q0 = q_begin, c->last.q1 = q_end;
    c->last.kernel = qlane ? 2 : 1, c->last.kernel_variant = qlane ? 4 : 1;
    unsigned const nq = q_end - q_begin;
    bool const xt_given = !c->xt64.empty(); // dcp_gpu_seqs_set_xtrans64: the flags are ignored
    std::vector<uint32_t> seqs(nq);
    std::iota(seqs.begin(), seqs.end(), q_begin);
    std::vector<double> xt;
    if (int rc = fill_xtrans(c, seqs, prm->multi_hits, prm->hmmer3_compat, DCP_F64_XSTRIDE, xt)) return rc;
    uint32_t const lmax = *std::max_element(c->seq_len.begin() + q_begin, c->seq_len.begin() + q_end);
    HIP_TRY(c, F.d_xt.reserve(xt.size()));
    HIP_TRY(c, hipMemcpyAsync(F.d_xt.p, xt.data(), xt.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));

    HIP_TRY(c, F.res.ensure((size_t)c->nseqs * c->nprof, prm->keep_scores != 0));
    F64Seg seg;
    if (int rc = f64_seg_columns(c, lmax, (uint64_t)(F.group_first[4] - F.group_first[3]) * nq, &seg)) return rc;

    dcp_f64_scan_args a{};
    a.nprof_total = c->nprof;
    a.tab = F.d_tab.p;
    a.trans = F.d_trans.p;
    a.xe = F.d_xe.p;
    a.seq_words = c->d_seq_words.p;
    a.seq_woff = c->d_seq_woff.p + q_begin;
    a.seq_len = c->d_seq_len.p + q_begin;
    a.xtrans = F.d_xt.p;
    a.nq = nq;
    a.q_base = q_begin;
    a.out_null = F.res.have_scores ? F.res.d_null.p + (size_t)q_begin * c->nprof : nullptr;
    a.out_alt = F.res.have_scores ? F.res.d_alt.p + (size_t)q_begin * c->nprof : nullptr;
    a.hits = F.res.hits();
    a.nhits = F.res.nhits();
    a.hit_cap = F.res.cap();
    a.lrt_threshold = is_nan(c->lrt_threshold64) ? (double)prm->lrt_threshold : c->lrt_threshold64; // NaN: not set
    bool const redo = prm->multi_hits != 0 || xt_given;
    dcp_f64_qlane_args qa{};
    unsigned ql_blocks = 0;
    if (qlane)
    {
        // the range's queries by rising length, packed into blocks of four wavefront slots as the float query-lane
        // kernels' batches are (plan_query_groups); a persistent grid of at most two blocks per CU, fewer where their
        // boundary planes ([the plan's plane rows][3][256] doubles each) would take too much memory
        SortedQueries const sorted = sorted_query_plan(c, q_begin, q_end, DCP_F64_QL_LANES / 64u);
        std::vector<uint32_t> const &qorder = sorted.order;
        QlPlan const &plan = sorted.plan;
        unsigned const nqb = plan.nqb;
        uint64_t const ntasks = (uint64_t)c->nprof * nqb;
        uint64_t const plane_stride = (uint64_t)plan.plane_rows * 3u * DCP_F64_QL_LANES;
        if (plane_stride > (1ull << 31) || ntasks > 0xf0000000ull)
            return c->fail(DCP_ENOMEM, "batch too large for the f64 query-lane kernel (%u rows, %llu tasks): use kernel = 1", lmax,
                           (unsigned long long)ntasks);
        size_t free_b = 0, total_b = 0;
        HIP_TRY(c, hipMemGetInfo(&free_b, &total_b));
        // (two blocks on each of 256 CUs at 10 kbp are 31 GB of planes; at 1 kbp 3 GB)
        uint64_t const budget = std::min<uint64_t>(((uint64_t)free_b + F.d_planes.n * sizeof(double)) / 2u, 40ull << 30);
        ql_blocks = (unsigned)std::min<uint64_t>(std::min<uint64_t>(2ull * c->num_cus, ntasks), budget / (plane_stride * sizeof(double)));
        if (ql_blocks == 0)
            return c->fail(DCP_ENOMEM, "sequences too long for the f64 query-lane kernel (%u rows of boundary planes do not fit the device): use kernel = 1", lmax);
        HIP_TRY(c, F.d_planes.reserve(ql_blocks * plane_stride));
        HIP_TRY(c, F.d_qorder.reserve(nq));
        HIP_TRY(c, F.d_slot_first.reserve(plan.slot_first.size()));
        HIP_TRY(c, F.d_groups.reserve(plan.groups.size()));
        HIP_TRY(c, hipMemcpyAsync(F.d_qorder.p, qorder.data(), nq * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(F.d_slot_first.p, plan.slot_first.data(), plan.slot_first.size() * sizeof(uint32_t),
                                  hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(F.d_groups.p, plan.groups.data(), plan.groups.size() * sizeof(dcp_ql_group),
                                  hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream)); // qorder, the plan and xt leave scope
        F.plan_blocks = nqb, F.plan_rows = plan.plane_rows, F.plan_sum_rows = plan.sum_block_rows;
        F.plan_max_groups = 0;
        for (size_t i = 0; i + 1u < plan.slot_first.size(); ++i)
            F.plan_max_groups = std::max<unsigned>(F.plan_max_groups, plan.slot_first[i + 1u] - plan.slot_first[i]);
        HIP_TRY(c, F.d_task.reserve(1));
        HIP_TRY(c, F.d_redo_n.reserve(5));
        // a redo list per launch group; uni-hit scans have no feedback and no lists (explicit transitions may carry
        // E -> B / J -> B feedback whatever the flag says)
        uint64_t redo_total = 0;
        for (int g = 0; g < 4; ++g)
        {
            uint64_t const pairs = (uint64_t)(F.group_first[g + 1] - F.group_first[g]) * nq;
            qa.redo_first[g] = (unsigned)redo_total;
            qa.redo_cap[g] = redo ? (unsigned)std::min<uint64_t>(pairs, c->redo_cap_limit) : 0u;
            redo_total += qa.redo_cap[g];
        }
        if (redo_total > 0xffffffffull)
            return c->fail(DCP_ENOMEM, "batch too large for the f64 query-lane kernel's redo lists: use kernel = 1");
        HIP_TRY(c, F.d_redo.reserve(redo_total));
        qa.profs = F.d_profs.p;
        qa.order = F.d_order.p;
        qa.nprof_total = c->nprof;
        qa.tab = a.tab, qa.trans = a.trans, qa.xe = a.xe;
        qa.seq_words = a.seq_words, qa.seq_woff = a.seq_woff, qa.seq_len = a.seq_len;
        qa.xtrans = a.xtrans;
        qa.qorder = F.d_qorder.p;
        qa.groups = F.d_groups.p, qa.slot_first = F.d_slot_first.p;
        qa.nq = nq, qa.q_base = q_begin, qa.nqb = nqb, qa.ntasks = (unsigned)ntasks;
        qa.out_null = a.out_null, qa.out_alt = a.out_alt;
        qa.hits = a.hits, qa.nhits = a.nhits, qa.hit_cap = a.hit_cap;
        qa.lrt_threshold = a.lrt_threshold;
        qa.planes = F.d_planes.p;
        qa.plane_stride = plane_stride;
        qa.task_counter = F.d_task.p;
        qa.redo = F.d_redo.p;
        qa.redo_n = F.d_redo_n.p;
        HIP_TRY(c, hipMemsetAsync(F.d_task.p, 0, sizeof(unsigned), c->stream));
        HIP_TRY(c, hipMemsetAsync(F.d_redo_n.p, 0, 5 * sizeof(unsigned), c->stream));
    }
    HIP_TRY(c, hipMemsetAsync(a.nhits, 0, sizeof(unsigned), c->stream));
    HIP_TRY(c, hipEventRecord(c->ev_start, c->stream));
    if (qlane)
    {
        dcp_f64_launch_qlane(&qa, ql_blocks, c->stream);
        HIP_TRY(c, hipGetLastError());
        ++c->last.launches;
        // the pairs whose B(j) was not B0(j): the row sweep over each group's list, right behind
        for (int g = 0; g < 4 && redo; ++g)
        {
            if (qa.redo_cap[g] == 0) continue;
            dcp_f64_pairs_args pa{};
            static_cast<dcp_f64_scan_args &>(pa) = a;
            pa.profs = F.d_profs.p;
            pa.nprof = c->nprof;
            pa.pairs = F.d_redo.p + qa.redo_first[g];
            pa.npairs_dev = F.d_redo_n.p + g;
            pa.pair_cap = qa.redo_cap[g];
            unsigned const waves = f64_group_geometry(c, g, qa.redo_cap[g], seg, pa, 4096u); // (these launches' own cap)
            if (dcp_f64_launch_scan_pairs(kF64R[g], &pa, waves, c->stream))
                return c->fail(DCP_EFAIL, "no f64 kernel for %d nodes per lane", kF64R[g]);
            HIP_TRY(c, hipGetLastError());
            ++c->last.launches;
            note_pair_launch(c, DCP_PL_QLANE_REDO, 64u, (unsigned)g, (unsigned)kF64R[g], waves, 1u, pa.pair_cap);
        }
    }
    for (int g = 0; g < 4 && !qlane; ++g)
    {
        unsigned const n = F.group_first[g + 1] - F.group_first[g];
        if (n == 0) continue;
        a.profs = F.d_profs.p + F.group_first[g];
        a.nprof = n;
        if (dcp_f64_launch_scan(kF64R[g], &a, f64_group_geometry(c, g, (uint64_t)n * nq, seg, a), c->stream))
            return c->fail(DCP_EFAIL, "no f64 kernel for %d nodes per lane", kF64R[g]);
        HIP_TRY(c, hipGetLastError());
        ++c->last.launches;
    }
    HIP_TRY(c, hipEventRecord(c->ev_stop, c->stream));
    c->last.redo_pending64 = qlane && redo;
    c->last.scanned = true;
    return DCP_OK;
}

// What a row-sweep kernel reads of the resident DB and of the queries [q_begin, q_end) of the resident batch, and the
// geometry of the range; no outputs (the traceback's forward pass has none of a scan's).
static dcp_scan_args scan_inputs(dcp_gpu_ctx const *c, unsigned q_begin, unsigned q_end)
{
    dcp_scan_args a{};
    a.profs = c->d_metas.p;
    a.emis_match = c->d_emis_match.p;
    a.emis_insert = c->d_emis_insert.p;
    a.emis_null = c->d_emis_null.p;
    a.trans8 = c->d_trans8.p;
    a.seq_words = c->d_seq_words.p;
    // the kernels index sequences relative to q_begin
    unsigned const nq = q_end - q_begin;
    a.seq_woff = c->d_seq_woff.p + q_begin;
    a.seq_len = c->d_seq_len.p + q_begin;
    a.xtrans = c->d_xtrans.p + (size_t)q_begin * DCP_XSTRIDE;
    a.nprof_total = c->nprof;
    a.nseqs = nq;
    a.q_base = q_begin;
    // Queries a row-sweep wavefront scores one after the other with the profile's transitions in registers:
    // ONE.  More (8 per task in round 1) saves the reload of 8 transitions per node and nothing else, but
    // leaves fewer concurrent tasks per profile, so that an XCD works on more profiles at a time than its
    // 4 MB L2 holds tables of (C3 step: 848 -> 879 Gcell/s from 8 to 1; 25 profiles x 256 queries: 8.8 -> 1.8 ms).
    a.qchunk = 1u;
    a.nchunks = (nq + a.qchunk - 1) / a.qchunk;
    return a;
}

// The row-sweep kernels' argument block for a scan of those queries: the inputs, and the float results as its outputs.
static dcp_scan_args scan_args(dcp_gpu_ctx const *c, struct dcp_scan_params const *prm, unsigned q_begin, unsigned q_end)
{
    dcp_scan_args a = scan_inputs(c, q_begin, q_end);
    a.out_null = c->res.have_scores ? c->res.d_null.p + (size_t)q_begin * c->nprof : nullptr;
    a.out_alt = c->res.have_scores ? c->res.d_alt.p + (size_t)q_begin * c->nprof : nullptr;
    a.hits = c->res.hits();
    a.nhits = c->res.nhits();
    a.hit_cap = c->res.cap();
    a.lrt_threshold = prm->lrt_threshold;
    return a;
}

// Kernel 0: 1 (row sweep), 2 (query lane) or 3 (its two-stage variant) for the queries [q_begin, q_end), by a
// cost model fitted to profiles/latency_probe.py and profiles/smalldb_probe.py:
//   row sweep    cells of each size class / that class's rate (kClassRate: 0.5-1.05 Tcell/s with one
//                wavefront per pair, 0.4-0.6 with 4-16) + one pass over the emission tables at
//                3 TB/s (a small batch streams them from HBM: 20k profiles, 16 queries: 103 ms =
//                67 + 36) + the last task's row chain
//   query lane   max(longest task, all tile rows / resident blocks); a tile row of a block
//                takes 0.52 us with one busy wavefront, 0.73 us with four.
// On the 20k-profile DB the switch comes at about 150 queries since round 3 (128 queries: 484 ms in
// the row sweep, 480 in the single-stage query-lane kernel; round 2: at about 115); a DB of a few
// hundred profiles stays with the row sweep up to several hundred queries (its tasks cannot fill the grid).
// ql_nt, ql_blocks_per_cu, w3: how the single-stage query-lane kernel would take the batch.
static int choose_kernel(dcp_gpu_ctx const *c, unsigned q_begin, unsigned q_end, unsigned qchunk, unsigned ql_nt,
                         unsigned ql_blocks_per_cu, bool w3)
{
    unsigned const nq = q_end - q_begin;
    // rows a tile costs, summed over the blocks of wavefront slots the batch is packed into (plan_query_groups)
    SortedQueries const sorted = sorted_query_plan(c, q_begin, q_end, ql_nt / 64u);
    QlPlan const &plan = sorted.plan;
    double sum_len = 0;
    for (unsigned L : sorted.len)
        sum_len += L;
    unsigned const nqb = plan.nqb;
    double const sum_block_lmax = (double)plan.sum_block_rows;
    unsigned const lmax = sorted.len.back();
    double t_rs = (double)c->sum_core * (DCP_NCODES * 4.0) / 3e12 + qchunk * lmax * 1.2e-6; // 1.2 us per row
    // (the class rates are those of a 1 000-query step; between 64 and 256 queries the row sweep runs 5 %
    // below them -- 128 queries 450 ms, 160: 558 -- profiles/r03/switch_probe.txt)
    for (int k = 0; k < kNumClasses; ++k)
        t_rs += 1.05 * (double)c->class_core[k] * sum_len / kClassRate[k];
    unsigned const waves = std::max(1u, std::min(4u, plan.busy_slots));
    // (round 3, 20k-profile DB: 96 and 128 queries 477 / 480 ms, 256 queries 659 ms in the single-stage kernel)
    static double const kTrow[4] = {0.52, 0.54, 0.62, 0.73}; // 144..191 queries: 544-555 ms
    double const trow = (w3 ? 0.56 : kTrow[waves - 1u]) * 1e-6; // w3: + one add per gather
    double const resident = (double)std::min<uint64_t>((uint64_t)c->nprof * nqb, (uint64_t)ql_blocks_per_cu * c->num_cus);
    double const t_ql = std::max((double)c->max_tiles * lmax * 0.52e-6,
                                 (double)c->sum_tiles * sum_block_lmax * trow / resident) +
                        1e-4; // its redo launches
    // The two-stage variant (512-thread blocks, two tiles of a profile in flight) wins once the
    // query blocks are mostly full -- measured on the C3 DB (profiles/r02/latency_probe.txt):
    // 256 queries 641 vs 678 ms, 1024 queries 2508 vs 2657 ms (0.94); below that its idle
    // wavefronts still sit through every barrier (128 queries 583 vs 514 ms).  With fewer tasks
    // than blocks fit on the chip it takes 0.66 of the single-stage time (profiles/smalldb_probe.py).
    bool const stage2 = nq > 192u; // 192 queries (three full wavefronts per block): 555 ms single-stage, 569 two-stage; 224: 654 / 628
    double const fill = std::min(1.0, (double)c->nprof * nqb / (4.0 * c->num_cus));
    double const t_q = stage2 ? t_ql * (0.66 + 0.28 * fill) : t_ql;
    // a batch with very long sequences cannot keep enough blocks resident: row sweep instead
    if (lmax > 200000u) return 1;
    return t_q < t_rs ? (stage2 ? 3 : 2) : 1;
}

// What a query-lane launch with ql_nt queries per block needs of the range's queries: their length order, the plan that
// packs 64-query groups into wavefront slots (plan_query_groups) and the blocks' transposed window planes.  Kept
// between scans of the same range and block size.
static int ensure_qlane_layout(dcp_gpu_ctx *c, dcp_scan_args const &a, unsigned q_begin, unsigned q_end, unsigned ql_nt)
{
    HIP_TRY(c, c->d_task_counter.reserve(1));
    if (c->qorder_q0 == q_begin && c->qorder_q1 == q_end && c->qorder_nt == ql_nt) return DCP_OK;
    unsigned const nq = q_end - q_begin, NTq = ql_nt, slots = NTq / 64u;
    SortedQueries const sorted = sorted_query_plan(c, q_begin, q_end, slots);
    QlPlan const &plan = sorted.plan;
    unsigned const nqb = plan.nqb;
    if ((uint64_t)plan.plane_rows * NTq * 4u > 0xffffffffull) // 32-bit byte offsets into a block's planes
        return c->fail(DCP_ENOMEM, "sequences too long for the query-lane kernel (%u plane rows): use kernel = 1", plan.plane_rows);
    // The length-sorted query order and the plane offsets travel through pinned host memory -- [nq] order, [nqb + 1]
    // plane offsets, [nslots + 1] slot table, 4 words per group
    size_t const nslot_words = (size_t)nqb * slots + 1u, ngroup_words = plan.groups.size() * 4u;
    size_t const need_stage = (size_t)nq + nqb + 1u + nslot_words + ngroup_words;
    if (!c->ev_qstage) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_qstage, hipEventDisableTiming));
    else HIP_TRY(c, hipEventSynchronize(c->ev_qstage)); // the previous layout's copies have left the buffer
    if (c->h_qstage_n < need_stage)
    {
        if (c->h_qstage) (void)hipHostFree(c->h_qstage);
        c->h_qstage = nullptr, c->h_qstage_n = 0;
        HIP_TRY(c, hipHostMalloc((void **)&c->h_qstage, need_stage * sizeof(uint32_t), hipHostMallocDefault));
        c->h_qstage_n = need_stage;
    }
    uint32_t *const h_ord = c->h_qstage, *const wt_off = h_ord + nq, *const h_slots = wt_off + nqb + 1u,
                   *const h_groups = h_slots + nslot_words;
    static_assert(sizeof(dcp_ql_group) == 4 * sizeof(uint32_t), "group records travel as four words");
    std::memcpy(h_ord, sorted.order.data(), nq * sizeof(uint32_t));
    std::memcpy(h_slots, plan.slot_first.data(), nslot_words * sizeof(uint32_t));
    std::memcpy(h_groups, plan.groups.data(), ngroup_words * sizeof(uint32_t));
    // per block: its window plane, uint16 [block rows + 8][NTq] (the prefetch runs a few rows past the end)
    uint64_t tot = 0;
    wt_off[0] = 0u;
    for (unsigned b = 0; b < nqb; ++b)
    {
        tot += ((uint64_t)plan.block_rows[b] + 8u) * NTq / 2u;
        if (tot > 0xffffffffull) return c->fail(DCP_EINVAL, "sequence batch too large");
        wt_off[b + 1u] = (uint32_t)tot;
    }
    HIP_TRY(c, c->d_qorder.reserve(nq));
    HIP_TRY(c, c->d_wt_off.reserve(nqb + 1u));
    HIP_TRY(c, c->d_slot_first.reserve(nslot_words));
    HIP_TRY(c, c->d_ql_groups.reserve(plan.groups.size()));
    HIP_TRY(c, c->d_words_t.reserve((size_t)tot));
    HIP_TRY(c, hipMemcpyAsync(c->d_qorder.p, h_ord, nq * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_wt_off.p, wt_off, (nqb + 1u) * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_slot_first.p, h_slots, nslot_words * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_ql_groups.p, h_groups, ngroup_words * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipEventRecord(c->ev_qstage, c->stream));
    dcp_qlane_args ta{};
    ta.seq_words = a.seq_words, ta.seq_woff = a.seq_woff, ta.seq_len = a.seq_len;
    ta.qorder = c->d_qorder.p, ta.words_t = c->d_words_t.p, ta.wt_off = c->d_wt_off.p;
    ta.groups = c->d_ql_groups.p, ta.slot_first = c->d_slot_first.p;
    ta.nseqs = nq, ta.nqblocks = nqb;
    if (dcp_launch_qlane_transpose(&ta, NTq, c->stream)) return c->fail(DCP_EFAIL, "no kernel for %u-query blocks", NTq);
    HIP_TRY(c, hipGetLastError());
    c->qorder_q0 = q_begin, c->qorder_q1 = q_end, c->qorder_nt = NTq;
    c->ql_nqb = nqb, c->ql_plane_rows = plan.plane_rows + 8u;
    return DCP_OK;
}

// A launch of the scan has been enqueued on `stream`: the event behind it (dcp_gpu_last_scan_launch_info times the
// launches by them), the context stream's join on it when the launch ran on a forked stream, and the launch's record.
static int record_launch(dcp_gpu_ctx *c, int k, bool is_redo, hipStream_t stream, bool join)
{
    HIP_TRY(c, hipEventRecord(c->ev_class[c->last.n_launched], stream));
    if (join) HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_class[c->last.n_launched], 0));
    c->last.launched_redo[c->last.n_launched] = is_redo; // the exact kernel behind a segmented sweep
    c->last.launched_class[c->last.n_launched++] = k;    // -1: the query-lane launch
    c->last.launches++;
    return DCP_OK;
}

// The query-lane kernel (single-stage, its three-independent-wavefronts variant or two-stage) on the layout of
// ensure_qlane_layout, and behind it the row sweep of each size class over the pairs the kernel handed on.
static int launch_qlane_scan(dcp_gpu_ctx *c, struct dcp_scan_params const *prm, dcp_scan_args &a, unsigned NT,
                             unsigned ql_blocks_per_cu, bool two_stage, bool use_w3)
{
    dcp_qlane_args qa{};
    qa.profs = c->d_ql_metas.p;
    qa.emis_tiles = c->one_layout ? c->d_emis_match.p : c->d_emis_tiles.p;
    qa.tiles_from_rows = c->one_layout ? 1u : 0u;
    qa.emis_insert = c->d_emis_insert.p;
    qa.emis_null = c->d_emis_null.p;
    qa.ttrans = c->d_ttrans.p;
    qa.seq_words = a.seq_words;
    qa.seq_woff = a.seq_woff;
    qa.seq_len = a.seq_len;
    qa.xtrans = a.xtrans;
    qa.qorder = c->d_qorder.p;
    qa.words_t = c->d_words_t.p;
    qa.wt_off = c->d_wt_off.p;
    qa.groups = c->d_ql_groups.p;
    qa.slot_first = c->d_slot_first.p;
    qa.ring_stall = c->ring_stall;
    qa.task_counter = c->d_task_counter.p;
    qa.out_null = a.out_null;
    qa.out_alt = a.out_alt;
    qa.hits = a.hits;
    qa.nhits = a.nhits;
    qa.hit_cap = a.hit_cap;
    qa.lrt_threshold = prm->lrt_threshold;
    qa.nprof = c->nprof;
    qa.nprof_total = c->nprof;
    qa.nseqs = a.nseqs;
    qa.q_base = a.q_base;
    qa.plane_rows = c->ql_plane_rows;
    qa.nqblocks = c->ql_nqb;
    uint64_t const ntasks = (uint64_t)c->nprof * qa.nqblocks;
    if (ntasks > 0xffffffffull) return c->fail(DCP_EINVAL, "scan too large for one launch");
    qa.ntasks = (unsigned)ntasks;
    // redo lists: pairs whose multi-hit feedback beat B0 go to the row-sweep kernel, which
    // runs right behind the query-lane kernel on this stream (uni-hit scans have no feedback)
    // (explicit transitions may carry E->B feedback; flagged profiles leave the kernel through the lists too)
    bool const redo = prm->multi_hits != 0 || c->xt_explicit || (dcp_qlane_exact_e_by_redo() && c->any_exact_e);
    unsigned redo_grid[kNumClasses] = {0};
    if (redo)
    {
        if (int rc = ensure_rowsweep_layout(c)) return rc;
        a.emis_match = c->d_emis_match.p;
        uint64_t tot = 0;
        uint64_t const cap_limit = c->redo_cap_limit; // per size class (2^26: 512 MB of pairs at most)
        for (int k = 0; k < kNumClasses; ++k)
        {
            uint64_t const pairs = (uint64_t)a.nseqs * (c->class_first[k + 1] - c->class_first[k]);
            unsigned const cap = (unsigned)std::min<uint64_t>(pairs, cap_limit);
            qa.redo_base[k] = (unsigned)tot;
            qa.redo_cap[k] = cap;
            tot += cap;
            uint64_t const tpb = dcp_rowsweep_tasks_per_block(kClasses[k].W);
            uint64_t g = std::min<uint64_t>((cap + tpb - 1) / tpb, 8ull * c->num_cus);
            redo_grid[k] = (unsigned)((g + 7) / 8 * 8);
        }
        HIP_TRY(c, c->d_redo.reserve((size_t)tot));
    }
    // counters, overflow flag and the ring's error word start every query-lane scan at zero (without redo the
    // lists' capacities are 0: the counters are never written)
    HIP_TRY(c, c->d_redo_n.reserve(DCP_MAX_CLASSES + 2));
    HIP_TRY(c, hipMemsetAsync(c->d_redo_n.p, 0, (DCP_MAX_CLASSES + 2) * sizeof(unsigned), c->stream));
    qa.redo = c->d_redo.p;
    qa.redo_n = c->d_redo_n.p;
    qa.redo_overflow = c->d_redo_n.p + DCP_MAX_CLASSES;
    qa.ring_error = c->d_redo_n.p + DCP_MAX_CLASSES + 1;
    // scratch = 3 planes x plane rows x NT floats per resident block; long sequences
    // (SCHED_SEQ_SIZE allows 1 MiB) get fewer resident blocks so the planes stay within budget
    uint64_t const per_block = (uint64_t)dcp_qlane_scratch_planes() * (uint64_t)qa.plane_rows * NT; // floats
    uint64_t const budget = (uint64_t)64 << 28;                      // 64 GiB of floats / 4
    uint64_t fit = per_block ? budget / per_block : 0;
    // one 512-thread block per CU (two-stage) or two 256-thread blocks (single-stage)
    uint64_t const resident_blocks = (uint64_t)ql_blocks_per_cu * c->num_cus; // w3: wavefront slots, 3 per block
    unsigned nblocks = (unsigned)std::min<uint64_t>(std::min<uint64_t>(ntasks, resident_blocks), fit);
    if (use_w3) nblocks = (nblocks + 2u) / 3u * 3u; // whole 3-slot blocks (scratch is sized for every slot)
    if (nblocks == 0)
        return c->fail(DCP_ENOMEM, "sequences too long for the query-lane kernel (%u plane rows): use kernel = 1", qa.plane_rows);
    size_t const need = (size_t)nblocks * per_block;
    HIP_TRY(c, c->d_scratch.reserve(need));
    qa.scratch = c->d_scratch.p;
    HIP_TRY(c, hipMemsetAsync(c->d_task_counter.p, 0, sizeof(unsigned), c->stream));
    HIP_TRY(c, hipEventRecord(c->ev_start, c->stream));
    if (two_stage ? dcp_launch_qlane2(&qa, nblocks, c->stream)
                  : use_w3 ? dcp_launch_qlane_w3(&qa, nblocks / 3u, c->stream)
                           : dcp_launch_qlane(&qa, nblocks, NT, c->stream))
        return c->fail(DCP_EFAIL, "query-lane launch failed");
    HIP_TRY(c, hipGetLastError());
    if (int rc = record_launch(c, -1, false, c->stream, false)) return rc;
    for (int k = 0; redo && k < kNumClasses; ++k)
    {
        if (redo_grid[k] == 0) continue;
        a.pairs = c->d_redo.p + qa.redo_base[k];
        a.npairs = c->d_redo_n.p + k;
        a.pair_cap = qa.redo_cap[k];
        a.first_prof = 0;
        a.nprof = c->nprof;
        SizeClass const sc = kClasses[k];
        if (dcp_launch_rowsweep(sc.R, sc.W, &a, redo_grid[k], c->stream))
            return c->fail(DCP_EFAIL, "no kernel for class R=%d W=%d", sc.R, sc.W);
        if (int rc = record_launch(c, k, true, c->stream, false)) return rc;
        note_pair_launch(c, DCP_PL_QLANE_REDO, 32u, (unsigned)sc.R, (unsigned)sc.W, redo_grid[k], dcp_rowsweep_tasks_per_block(sc.W), a.pair_cap);
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->ev_stop, c->stream));
    c->last.redo_pending = redo;
    c->last.ring_check_pending = two_stage;
    c->last.scanned = true;
    return DCP_OK;
}

// Multi-wavefront classes with a segmented-sweep kernel (dcp_kernels.hip): one wavefront per pair, one SEGMENT of
// the profile per launch, B(j) = N(j) + NB, the pairs with feedback finished by the exact kernel behind it.
// Per class: two boundary columns of lmax + 2 rows of 16 bytes per pair, and a redo list of all its pairs.  The
// columns of a class are capped at seg_col_bytes: beyond, its queries are swept chunk by chunk.
struct SegSweepPlan
{
    unsigned stride = 0;                                     // rows of 16 bytes per column
    unsigned chunk[kNumClasses] = {0};                       // queries per pass; 0: the class is not swept in segments
    uint64_t redo_off[kNumClasses] = {0}, col_rows = 0, redo_tot = 0;
};
static SegSweepPlan plan_segsweep(dcp_gpu_ctx const *c, unsigned q_begin, unsigned q_end)
{
    SegSweepPlan sp;
    unsigned const nq = q_end - q_begin;
    sp.stride = *std::max_element(c->seq_len.begin() + q_begin, c->seq_len.begin() + q_end) + 2u;
    for (int k = 0; k < kNumClasses; ++k)
    {
        unsigned const np = c->class_first[k + 1] - c->class_first[k];
        SizeClass const sc = kClasses[k];
        uint64_t const pairs = (uint64_t)np * nq;
        // (once the class has pairs enough to fill the chip's wavefront slots twice over: below, a pair's segments one
        // after the other are a longer serial chain than the exact kernel's wavefronts side by side -- C3 DB, 1 query
        // 11.8 -> 14.4 ms with round 3's kernel; C5 DB, where 37 % of the profiles are in these classes: 16 queries
        // 291 ms with the exact kernel, profiles/r04/latency_probe_c5_db.txt)
        bool const want = c->seg_mode == 1 || (c->seg_mode < 0 && pairs >= 16ull * c->num_cus);
        bool const have = sc.W > 1 && want && np > 0 && pairs <= ((uint64_t)1 << 26);
        if (!have) continue;
        // queries per chunk: np x chunk pairs x 2 columns x stride x 16 bytes within the cap
        uint64_t const per_query = (uint64_t)np * 2u * sp.stride * 16u;
        uint64_t const chunk = std::min<uint64_t>(nq, c->seg_col_bytes / per_query);
        if (chunk == 0) continue; // very long sequences: the exact kernel
        if ((uint64_t)np * ((chunk + 3u) / 4u) > 0x7ffffff0ull) continue;
        sp.chunk[k] = (unsigned)chunk;
        // (classes run one after the other on a stream, or side by side on their own streams when the scan is small:
        // every class gets columns of its own)
        sp.col_rows += (uint64_t)np * chunk * 2u * sp.stride;
        sp.redo_off[k] = sp.redo_tot, sp.redo_tot += pairs;
    }
    return sp;
}

// Class k of a row-sweep scan in segments (a.first_prof / a.nprof: the class; col_base: its boundary columns), on ls.
static int launch_segsweep_class(dcp_gpu_ctx *c, dcp_scan_args &a, int k, SegSweepPlan const &sp, float *col_base,
                                 hipStream_t ls, bool overlap)
{
    unsigned const first = a.first_prof, last = first + a.nprof, np = a.nprof, chunk = sp.chunk[k], nq = a.nseqs;
    uint64_t const ntasks = (uint64_t)a.nprof * a.nchunks;
    SizeClass const sc = kClasses[k];
    a.seg_stride = sp.stride;
    a.seg_redo = c->d_seg_redo.p + sp.redo_off[k];
    a.seg_redo_n = c->d_seg_redo_n.p + k;
    a.seg_redo_cap = (unsigned)ntasks;
    // Segment-major: launch s sweeps segment s of every pair of the chunk; the kernel boundary is the hand-off.
    // The class's profiles are ordered by their segments' lane width: one run of launches per width.
    for (unsigned sub = first; sub < last;)
    {
        unsigned const segR = seg_r_of(c->metas[sub].core_size);
        unsigned sub_end = sub, max_m = 0;
        while (sub_end < last && seg_r_of(c->metas[sub_end].core_size) == segR)
            max_m = std::max(max_m, c->metas[sub_end].core_size), ++sub_end;
        unsigned const nsub = sub_end - sub, nseg_max = (max_m + 64u * segR - 1u) / (64u * segR);
        a.first_prof = sub, a.nprof = nsub;
        a.seg_col0 = col_base + (size_t)(sub - first) * chunk * 2u * sp.stride * 4u;
        a.seg_col1 = a.seg_col0 + (size_t)nsub * chunk * sp.stride * 4u;
        for (unsigned qc = 0; qc < nq; qc += chunk)
        {
            a.seg_q0 = qc, a.seg_nq = std::min(chunk, nq - qc);
            for (unsigned sg = 0; sg < nseg_max; ++sg)
            {
                a.seg_index = sg;
                if (dcp_launch_segsweep((int)segR, &a, dcp_segsweep_blocks(nsub, a.seg_nq), ls))
                    return c->fail(DCP_EFAIL, "no segmented kernel for %u nodes per lane", segR);
            }
        }
        sub = sub_end;
    }
    a.first_prof = first, a.nprof = np;
    if (int rc = record_launch(c, k, false, ls, false)) return rc;
    // the pairs it could not finish: the exact kernel in pair mode, right behind
    a.pairs = a.seg_redo, a.npairs = a.seg_redo_n, a.pair_cap = a.seg_redo_cap;
    a.first_prof = 0, a.nprof = c->nprof;
    uint64_t g = std::min<uint64_t>(ntasks, 8ull * c->num_cus);
    g = (g + 7u) / 8u * 8u;
    if (dcp_launch_rowsweep(sc.R, sc.W, &a, (unsigned)g, ls))
        return c->fail(DCP_EFAIL, "no kernel for class R=%d W=%d", sc.R, sc.W);
    note_pair_launch(c, DCP_PL_SEG_REDO, 32u, (unsigned)sc.R, (unsigned)sc.W, (unsigned)g, dcp_rowsweep_tasks_per_block(sc.W), a.pair_cap);
    return record_launch(c, k, true, ls, overlap);
}

// The row sweep over every pair of the range: one launch per non-empty size class (segmented, K profiles per
// wavefront, or plain), one after the other or -- small scans -- side by side on the classes' own streams.
static int launch_rowsweep_scan(dcp_gpu_ctx *c, dcp_scan_args &a, unsigned q_begin, unsigned q_end)
{
    unsigned const nq = q_end - q_begin;
    if (int rc = ensure_rowsweep_layout(c)) return rc;
    a.emis_match = c->d_emis_match.p;
    HIP_TRY(c, hipEventRecord(c->ev_start, c->stream));
    // fork / join around the class launches when no single one fills the chip for long (2^22 pairs: 20 000 profiles x 209
    // queries, i.e. every batch the automatic choice gives the row sweep; 112 .. 160 queries: 1 % faster than one launch
    // after the other, profiles/r04/class_launch_order.txt)
    bool const overlap = (uint64_t)nq * c->nprof < ((uint64_t)1 << 22);
    c->last.overlapped = overlap;
    SegSweepPlan const sp = plan_segsweep(c, q_begin, q_end);
    if (sp.col_rows)
    {
        HIP_TRY(c, c->d_seg_scratch.reserve((size_t)sp.col_rows * 4u));
        HIP_TRY(c, c->d_seg_redo.reserve((size_t)sp.redo_tot));
        HIP_TRY(c, c->d_seg_redo_n.reserve(DCP_MAX_CLASSES));
        HIP_TRY(c, hipMemsetAsync(c->d_seg_redo_n.p, 0, DCP_MAX_CLASSES * sizeof(unsigned), c->stream));
        HIP_TRY(c, hipEventRecord(c->ev_start, c->stream)); // the forked streams wait for the counters' reset too
    }
    uint64_t seg_col_at = 0; // floats
    for (int kk = 0; kk < kNumClasses; ++kk)
    {
        // Forked launches (small batches): the classes of the largest profiles first.  A pair takes rows x the row's
        // latency, which grows with the wavefronts the pair spans, and the few pairs of the largest classes, started
        // last, ran on alone at the end: C3 DB, 1 / 2 / 4 / 16 queries 10.3 / 16.8 / 26.5 / 74.2 -> 9.4 / 15.4 / 25.2 /
        // 70.8 ms; C5 DB 4 .. 32 queries 1-5 % less, 1 and 64 queries 1-2 % more (profiles/r04/class_launch_order.txt;
        // the chip-filling classes first and only then the sparse ones, or the sparse ones first: in between)
        int const k = overlap ? kNumClasses - 1 - kk : kk;
        unsigned first = c->class_first[k], last = c->class_first[k + 1];
        if (last <= first) continue;
        hipStream_t const ls = overlap ? c->class_stream[k] : c->stream;
        if (overlap) HIP_TRY(c, hipStreamWaitEvent(ls, c->ev_start, 0));
        a.first_prof = first;
        a.nprof = last - first;
        a.pairs = nullptr, a.npairs = nullptr, a.pair_cap = 0;
        SizeClass const sc = kClasses[k];
        uint64_t const ntasks = (uint64_t)a.nprof * a.nchunks;
        if (ntasks > 0xffffffffull) return c->fail(DCP_EINVAL, "scan too large for one launch");
        if (sp.chunk[k])
        {
            float *const col_base = c->d_seg_scratch.p + seg_col_at;
            seg_col_at += (uint64_t)a.nprof * sp.chunk[k] * 2u * sp.stride * 4u;
            note_rowsweep_plan(c, k, DCP_RS_PATH_SEGMENTED, 0, 0u, 0, sp.chunk[k], false);
            if (int rc = launch_segsweep_class(c, a, k, sp, col_base, ls, overlap)) return rc;
            continue;
        }
        // K profiles per wavefront: the class of at most 64 nodes always (855-890 Gcell/s against 600 with one node
        // per lane); the class of 65 .. 128 nodes while the batch is small -- its one-profile kernels at six or seven
        // wavefronts per SIMD are faster on a full grid (936 against 860 Gcell/s at 1 000 queries), slower below
        // (profiles/r04/rowsweep_small_classes.txt)
        bool const use_mp = k < 2 && c->mp_first[k + 1] > c->mp_first[k] &&
                            (c->mp_mode == 1 || (c->mp_mode < 0 && (k == 0 || nq < kMpClass1MaxQueries)));
        if (use_mp)
        {
            // The two smallest classes: K profiles per wavefront (viterbi_mp_kernel) for the grouped ones, the
            // unstaged one-profile kernel on the column views of the flagged rest.
            unsigned const g0 = c->mp_first[k], g1 = c->mp_first[k + 1];
            if (g1 > g0)
            {
                a.mp_groups = c->d_mp_groups.p, a.mp_in = c->d_mp_in.p;
                a.first_prof = g0, a.nprof = g1 - g0;
                if (int lrc = dcp_launch_mp((int)kMpParts[k], &a, ls))
                    return lrc == -2 ? c->fail(DCP_EINVAL, "scan too large for one launch") : c->fail(DCP_EFAIL, "no %u-profile kernel", kMpParts[k]);
            }
            if (c->mp_flagged_first[k])
            {
                a.first_prof = c->mp_flagged_first[k] - 1u, a.nprof = last - a.first_prof;
                if (int lrc = dcp_launch_rowsweep_grid(sc.R, sc.W, &a, 0, 1u, ls, 0u, 0))
                    return lrc == -2 ? c->fail(DCP_EINVAL, "scan too large for one launch") : c->fail(DCP_EFAIL, "no kernel for class R=%d W=%d", sc.R, sc.W);
            }
            a.first_prof = first, a.nprof = last - first;
            note_rowsweep_plan(c, k, DCP_RS_PATH_MP, 0, 0u, 0, 0u, c->mp_flagged_first[k] != 0u);
        }
        else
        {
            int stg, pf;
            unsigned bw;
            rowsweep_variant(c, sc.R, sc.W, a.nchunks, &stg, &bw, &pf);
            note_rowsweep_plan(c, k, DCP_RS_PATH_PLAIN, stg, bw, pf, 0u, false);
            if (int lrc = dcp_launch_rowsweep_grid(sc.R, sc.W, &a, stg, bw, ls, c->rs_pad_lds, pf))
                return lrc == -2 ? c->fail(DCP_EINVAL, "scan too large for one launch")
                                 : c->fail(DCP_EFAIL, "no kernel for class R=%d W=%d (stage %d, %u wavefronts)", sc.R, sc.W, stg, bw);
        }
        if (int rc = record_launch(c, k, false, ls, overlap)) return rc;
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->ev_stop, c->stream));
    c->last.scanned = true;
    return DCP_OK;
}

int dcp_gpu_scan_range(dcp_gpu_ctx *c, struct dcp_scan_params const *prm, unsigned q_begin,
                       unsigned q_end)
{
    if (!c || !prm) return DCP_EINVAL;
    if (c->nprof == 0) return c->fail(DCP_EINVAL, "no profile DB resident");
    if (c->nseqs == 0) return c->fail(DCP_EINVAL, "no sequences resident");
    if (q_begin >= q_end || q_end > c->nseqs) return c->fail(DCP_EINVAL, "bad sequence range");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->precision == 64) return scan64(c, prm, q_begin, q_end);
    if (int rc = complete_pending_scan(c)) return rc;
    if (int rc = check_xtrans_precision(c)) return rc;
    if (prm->kernel < 0 || prm->kernel > 3) return c->fail(DCP_EINVAL, "unknown kernel %d", prm->kernel);
    c->last = LastScan{};
    c->last.prm = *prm;
    c->last.q0 = q_begin, c->last.q1 = q_end;

    if (int rc = ensure_xtrans(c, prm->multi_hits, prm->hmmer3_compat)) return rc;
    HIP_TRY(c, c->res.ensure((size_t)c->nseqs * c->nprof, prm->keep_scores != 0));
    dcp_scan_args a = scan_args(c, prm, q_begin, q_end);
    unsigned const nq = q_end - q_begin;

    // Queries per block of the single-stage query-lane kernel.  (Narrow 64- / 128-query blocks were tried for
    // small batches: hipOccupancyMaxActiveBlocksPerMultiprocessor reports three 54.5 KB blocks per CU, the
    // measured rate is that of two -- profiles/r02/latency_probe_narrow_blocks_attempt.txt -- so they are gone.)
    unsigned ql_nt = dcp_qlane_block_size(), ql_blocks_per_cu = 2; // 2 x 54.5 KB of LDS, 2 x 4 wavefronts of 256 VGPRs
    // up to 64 queries: the three-independent-wavefronts variant (64 queries per task, 3 busy wavefronts per CU)
    // (since the row sweep went from 370 to 850 Gcell/s the automatic choice no longer reaches it:
    // 64 queries 283 ms there against 330 ms here; it is what kernel = 2 runs for such batches)
    bool const w3 = nq <= 64u;
    if (w3) ql_nt = 64u, ql_blocks_per_cu = 3; // counted in wavefront slots
    // kernel choice: the query-lane kernel needs enough queries to fill its lanes
    int kernel = prm->kernel;
    if (kernel == 0) kernel = choose_kernel(c, q_begin, q_end, a.qchunk, ql_nt, ql_blocks_per_cu, w3);
    bool const two_stage = kernel == 3; // the query-lane kernel's two-stage variant (dcp_qlane.hip)
    c->last.kernel_variant = kernel;
    if (two_stage) kernel = 2;
    c->last.kernel = kernel;
    if (two_stage) ql_nt = dcp_qlane_block_size(), ql_blocks_per_cu = 1; // 2 x 256 queries' wavefronts, one block per CU
    if (kernel == 2)
        if (int rc = ensure_qlane_layout(c, a, q_begin, q_end, ql_nt)) return rc;

    HIP_TRY(c, hipMemsetAsync(a.nhits, 0, sizeof(unsigned), c->stream));
    if (kernel == 2) return launch_qlane_scan(c, prm, a, ql_nt, ql_blocks_per_cu, two_stage, w3 && !two_stage);
    return launch_rowsweep_scan(c, a, q_begin, q_end);
}

// dcp_gpu_scan_pairs on a double DB: the lists by launch group, viterbi64_kernel<R, false, PAIRS> over each -- what
// scan64 launches behind the query-lane kernel over its redo lists.
static int scan_pairs64(dcp_gpu_ctx *c, struct dcp_scan_params const *prm, uint32_t const *seq_idx, uint32_t const *profile_idx,
                        unsigned npairs)
{
    if (int rc = check_xtrans_precision(c)) return rc;
    auto &F = c->f64;
    if (int rc = complete_pending_scan(c)) return rc;
    c->last = LastScan{};
    c->last.f64 = c->last.pair_scan = true;
    c->last.prm = *prm;
    c->last.q0 = 0, c->last.q1 = c->nseqs;
    c->last.kernel = c->last.kernel_variant = 1;
    unsigned first[5], count[4];
    std::vector<unsigned> const order = sort_into_classes(
        npairs, 4, first, [&](unsigned i) { return range_of(F.group_first, 4, F.slot_of_pidx[profile_idx[i]]); });
    for (int g = 0; g < 4; ++g)
        count[g] = first[g + 1] - first[g];
    std::vector<dcp_f64_pair> pairs(npairs);
    uint32_t seg_lmax = 0;
    for (unsigned j = 0; j < npairs; ++j)
    {
        unsigned const i = order[j];
        uint32_t const slot = F.slot_of_pidx[profile_idx[i]];
        pairs[j] = dcp_f64_pair{seq_idx[i], slot};
        uint64_t const M = F.profs[slot].core_size, L = c->seq_len[seq_idx[i]];
        if (j >= first[3]) seg_lmax = std::max(seg_lmax, (uint32_t)L); // the segmented group's pairs
        c->last.pair_cells += M * L, c->last.pair_bytes += 20ull * M * L + 32ull * (M + 1u) + L + 8u;
    }
    // the kernel takes a pair's special transitions from its query's row: one row per resident sequence, as a scan's
    std::vector<uint32_t> seqs(c->nseqs);
    std::iota(seqs.begin(), seqs.end(), 0u);
    std::vector<double> xt;
    if (int rc = fill_xtrans(c, seqs, prm->multi_hits, prm->hmmer3_compat, DCP_F64_XSTRIDE, xt)) return rc;
    HIP_TRY(c, F.d_xt.reserve(xt.size()));
    HIP_TRY(c, F.res.ensure(npairs, false));
    F64Seg seg;
    if (int rc = f64_seg_columns(c, seg_lmax, count[3], &seg)) return rc;
    HIP_TRY(c, F.d_pair_list.reserve(npairs));
    HIP_TRY(c, F.d_pair_n.reserve(4));
    HIP_TRY(c, hipMemcpyAsync(F.d_xt.p, xt.data(), xt.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (npairs) HIP_TRY(c, hipMemcpyAsync(F.d_pair_list.p, pairs.data(), (size_t)npairs * sizeof(dcp_f64_pair), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(F.d_pair_n.p, count, sizeof count, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // the lists and xt leave scope (and an earlier scan has read its own)

    dcp_f64_pairs_args pa{};
    pa.profs = F.d_profs.p;
    pa.nprof = c->nprof;
    pa.nprof_total = c->nprof;
    pa.tab = F.d_tab.p, pa.trans = F.d_trans.p, pa.xe = F.d_xe.p;
    pa.seq_words = c->d_seq_words.p, pa.seq_woff = c->d_seq_woff.p, pa.seq_len = c->d_seq_len.p;
    pa.xtrans = F.d_xt.p;
    pa.nq = c->nseqs, pa.q_base = 0;
    pa.out_null = pa.out_alt = nullptr;
    pa.hits = F.res.hits(), pa.nhits = F.res.nhits(), pa.hit_cap = F.res.cap();
    pa.lrt_threshold = is_nan(c->lrt_threshold64) ? (double)prm->lrt_threshold : c->lrt_threshold64; // NaN: not set
    HIP_TRY(c, hipMemsetAsync(pa.nhits, 0, sizeof(unsigned), c->stream));
    HIP_TRY(c, hipEventRecord(c->ev_start, c->stream));
    for (int g = 0; g < 4; ++g)
    {
        if (count[g] == 0) continue;
        pa.pairs = F.d_pair_list.p + first[g];
        pa.npairs_dev = F.d_pair_n.p + g;
        pa.pair_cap = count[g];
        unsigned const waves = f64_group_geometry(c, g, count[g], seg, pa);
        if (dcp_f64_launch_scan_pairs(kF64R[g], &pa, waves, c->stream))
            return c->fail(DCP_EFAIL, "no f64 kernel for %d nodes per lane", kF64R[g]);
        HIP_TRY(c, hipGetLastError());
        ++c->last.launches;
        note_pair_launch(c, DCP_PL_SCAN_PAIRS, 64u, (unsigned)g, (unsigned)kF64R[g], waves, 1u, pa.pair_cap);
    }
    HIP_TRY(c, hipEventRecord(c->ev_stop, c->stream));
    c->last.scanned = true;
    return DCP_OK;
}

// Score a list of pairs: bucketed by size class on the host, then the row-sweep kernels in pair mode over each
// non-empty class's list -- what the query-lane scans launch over their redo lists, with lists the host wrote.
int dcp_gpu_scan_pairs(dcp_gpu_ctx *c, struct dcp_scan_params const *prm, uint32_t const *seq_idx, uint32_t const *profile_idx,
                       unsigned npairs)
{
    if (!c || !prm) return DCP_EINVAL;
    if (c->nprof == 0) return c->fail(DCP_EINVAL, "no profile DB resident");
    if (c->nseqs == 0) return c->fail(DCP_EINVAL, "no sequences resident");
    if (prm->keep_scores) return c->fail(DCP_EINVAL, "a scan of a pair list keeps no dense score matrix: keep_scores must be 0");
    if (prm->kernel != 0 && prm->kernel != 1)
        return c->fail(DCP_EINVAL, "a pair list is scored by the row sweep (kernel 0 or 1), not %d", prm->kernel);
    if (npairs && (!seq_idx || !profile_idx)) return c->fail(DCP_EINVAL, "a pair list without its indices");
    if (int rc = check_pairs(c, seq_idx, profile_idx, 1u, npairs, false)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->precision == 64) return scan_pairs64(c, prm, seq_idx, profile_idx, npairs);
    // one scan is outstanding per context: an earlier query-lane scan is completed first
    if (int rc = complete_pending_scan(c)) return rc;
    if (int rc = check_xtrans_precision(c)) return rc;
    c->last = LastScan{};
    c->last.pair_scan = true;
    c->last.prm = *prm;
    c->last.q0 = 0, c->last.q1 = c->nseqs;
    c->last.kernel = c->last.kernel_variant = 1;
    if (int rc = ensure_xtrans(c, prm->multi_hits, prm->hmmer3_compat)) return rc;
    if (int rc = ensure_rowsweep_layout(c)) return rc;
    HIP_TRY(c, c->res.ensure(npairs, false));
    unsigned first[kNumClasses + 1], count[DCP_MAX_CLASSES] = {0};
    std::vector<unsigned> const order = sort_into_classes(
        npairs, kNumClasses, first, [&](unsigned i) { return range_of(c->class_first, kNumClasses, c->slot_of_pidx[profile_idx[i]]); });
    for (int k = 0; k < kNumClasses; ++k)
        count[k] = first[k + 1] - first[k];
    std::vector<dcp_pair> pairs(npairs);
    for (int k = 0; k < kNumClasses; ++k)
        for (unsigned j = first[k]; j < first[k + 1]; ++j)
        {
            unsigned const i = order[j];
            uint32_t const slot = c->slot_of_pidx[profile_idx[i]];
            pairs[j] = dcp_pair{seq_idx[i], slot}; // {q, slot}: the scan's first sequence is resident 0
            uint64_t const M = c->metas[slot].core_size, L = c->seq_len[seq_idx[i]];
            c->last.pair_class_cells[k] += M * L;
            c->last.pair_class_bytes[k] += 20ull * M * L + 32ull * (M + 1u) + L + 8u;
        }
    for (int k = 0; k < kNumClasses; ++k)
        c->last.pair_cells += c->last.pair_class_cells[k], c->last.pair_bytes += c->last.pair_class_bytes[k];
    HIP_TRY(c, c->d_pair_list.reserve(npairs));
    HIP_TRY(c, c->d_pair_n.reserve(DCP_MAX_CLASSES));
    if (npairs) HIP_TRY(c, hipMemcpyAsync(c->d_pair_list.p, pairs.data(), (size_t)npairs * sizeof(dcp_pair), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_pair_n.p, count, sizeof count, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // the lists leave scope (and an earlier scan has read its own)

    dcp_scan_args a = scan_args(c, prm, 0, c->nseqs); // no score matrix: res.have_scores is false
    a.emis_match = c->d_emis_match.p;
    a.first_prof = 0;
    a.nprof = c->nprof;
    HIP_TRY(c, hipMemsetAsync(a.nhits, 0, sizeof(unsigned), c->stream));
    HIP_TRY(c, hipEventRecord(c->ev_start, c->stream));
    for (int k = 0; k < kNumClasses; ++k)
    {
        if (count[k] == 0) continue;
        a.pairs = c->d_pair_list.p + first[k];
        a.npairs = c->d_pair_n.p + k;
        a.pair_cap = count[k];
        SizeClass const sc = kClasses[k];
        uint64_t const tpb = dcp_rowsweep_tasks_per_block(sc.W);
        unsigned const grid = (unsigned)((std::min<uint64_t>((count[k] + tpb - 1u) / tpb, 8ull * c->num_cus) + 7u) / 8u * 8u);
        if (dcp_launch_rowsweep(sc.R, sc.W, &a, grid, c->stream))
            return c->fail(DCP_EFAIL, "no kernel for class R=%d W=%d", sc.R, sc.W);
        if (int rc = record_launch(c, k, false, c->stream, false)) return rc;
        note_pair_launch(c, DCP_PL_SCAN_PAIRS, 32u, (unsigned)sc.R, (unsigned)sc.W, grid, (unsigned)tpb, a.pair_cap);
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->ev_stop, c->stream));
    c->last.scanned = true;
    return DCP_OK;
}

// ---- The pair-list sweeps: what the three calls share (dcp_forward.hip, dcp_posterior.hip) ---------------------------
// The kernels' classes: nodes per lane with the whole profile in registers (core sizes up to 64 R), or 0: the wide
// sweep through a work area per wavefront.
static constexpr int kFwdR[4] = {1, 2, 4, 0};
static int fwd_class(unsigned M) { return M <= 64u ? 0 : M <= 128u ? 1 : M <= (unsigned)DCP_FWD_CHUNK ? 2 : 3; }
static unsigned chunks_of(unsigned M) { return (M + (unsigned)DCP_FWD_CHUNK - 1u) / (unsigned)DCP_FWD_CHUNK; }

// The resident DB's profiles as the Forward kernel addresses them, by caller index: base, row stride and core size.  A
// float DB's small profiles share their rows (dcp_mp_group): a member's meta is already a column view of them.
static int forward_profiles(dcp_gpu_ctx *c)
{
    auto &W = c->sweeps;
    if (W.profs_ready) return DCP_OK;
    std::vector<dcp_fwd_prof> profs(c->nprof);
    if (c->precision == 64)
        for (dcp_f64_prof const &m : c->f64.profs)
            profs[m.pidx] = dcp_fwd_prof{m.tab_off, m.trans_off, m.xe_off, m.xe_off + DCP_NCODES, m.core_size, m.ldk};
    else
        for (dcp_prof_meta const &m : c->metas)
            profs[m.pidx] = dcp_fwd_prof{m.emis_off, m.trans_off, (uint64_t)m.pidx * DCP_NCODES, (uint64_t)m.pidx * DCP_NCODES,
                                         m.core_size, m.ldk};
    HIP_TRY(c, W.d_profs.alloc(profs.size()));
    HIP_TRY(c, hipMemcpy(W.d_profs.p, profs.data(), profs.size() * sizeof(dcp_fwd_prof), hipMemcpyHostToDevice));
    W.profs_ready = true;
    return DCP_OK;
}

// What the three pair-list calls refuse alike, on the host, before anything runs.
static int forward_check_list(dcp_gpu_ctx *c, uint32_t const *seq_idx, uint32_t const *profile_idx, unsigned npairs, bool outputs)
{
    if (c->nprof == 0) return c->fail(DCP_EINVAL, "no profile DB resident");
    if (c->nseqs == 0) return c->fail(DCP_EINVAL, "no sequences resident");
    if (npairs && (!seq_idx || !profile_idx)) return c->fail(DCP_EINVAL, "a pair list without its indices");
    if (npairs && !outputs) return c->fail(DCP_EINVAL, "a pair list without its score arrays");
    if (int rc = check_pairs(c, seq_idx, profile_idx, 1u, npairs, false)) return rc;
    return check_xtrans_precision(c);
}

// The special transitions a scan would use, one row per resident sequence, in double: a float DB's are the float ones
// (derived, or the caller's resident rows) promoted.
static int forward_special_transitions(dcp_gpu_ctx *c, int multi_hits, int hmmer3_compat, std::vector<double> &xt)
{
    bool const f64 = c->precision == 64;
    {
        std::vector<uint32_t> seqs(c->nseqs);
        std::iota(seqs.begin(), seqs.end(), 0u);
        if (f64)
        {
            if (int rc = fill_xtrans(c, seqs, multi_hits, hmmer3_compat, DCP_FWD_XSTRIDE, xt)) return rc;
        }
        else
        {
            static_assert((int)DCP_XSTRIDE == (int)DCP_FWD_XSTRIDE, "one row layout in both precisions");
            std::vector<float> xf;
            if (c->xt_explicit)
            {
                xf.resize((size_t)c->nseqs * DCP_XSTRIDE);
                HIP_TRY(c, hipMemcpy(xf.data(), c->d_xtrans.p, xf.size() * sizeof(float), hipMemcpyDeviceToHost));
            }
            else if (int rc = fill_xtrans(c, seqs, multi_hits, hmmer3_compat, DCP_XSTRIDE, xf)) return rc;
            xt.assign(xf.begin(), xf.end());
        }
    }
    return DCP_OK;
}

// What the Forward and Backward launches read of the resident DB (forward_profiles, and the tables of its precision) and
// batch; xt: the call's special transitions on the device.
static dcp_fwd_args forward_args(dcp_gpu_ctx const *c, double const *xt)
{
    dcp_fwd_args a{};
    a.profs = c->sweeps.d_profs.p;
    if (c->precision == 64) a.tab = c->f64.d_tab.p, a.trans = c->f64.d_trans.p, a.ei = a.en = c->f64.d_xe.p;
    else a.tab = c->d_emis_match.p, a.trans = c->d_trans8.p, a.ei = c->d_emis_insert.p, a.en = c->d_emis_null.p;
    a.seq_words = c->d_seq_words.p, a.seq_woff = c->d_seq_woff.p, a.seq_len = c->d_seq_len.p;
    a.xtrans = xt;
    return a;
}

// Everything between a call's refusals and its first launch: the DB's layout and profile table, the special transitions
// and the list's offsets (none: Forward) uploaded anew, room for nscores scores in d_score, the events.  a: forward_args,
// with work, row_off and out_null in place.  Returns synchronised if there are offsets, which are the caller's to drop;
// Forward's transitions go up under the synchronise of its one round's lists (if upload_round fails before that, the
// copy from W.xt is still queued: the vector is the workspace's and stays).
// wide: the wide class's pairs and the widest profile's chunks -- of a list (wide_of_list), or of the dense scan's outer
// product.
struct WidePairs
{
    uint64_t pairs = 0;
    unsigned chunks = 0;
};

static WidePairs wide_of_list(dcp_gpu_ctx const *c, uint32_t const *profile_idx, unsigned npairs)
{
    WidePairs w;
    for (unsigned i = 0; i < npairs; ++i)
    {
        unsigned const M = c->core_sizes[profile_idx[i]];
        if (fwd_class(M) == 3) ++w.pairs, w.chunks = std::max(w.chunks, chunks_of(M));
    }
    return w;
}

static int sweeps_setup(dcp_gpu_ctx *c, int multi_hits, int hmmer3_compat, WidePairs wide, size_t nscores,
                        std::vector<uint64_t> const &off, dcp_fwd_args *a, unsigned work_rows = DCP_FWD_WORK_ROWS)
{
    HIP_TRY(c, hipSetDevice(c->device));
    auto &W = c->sweeps;
    if (c->precision != 64)
        if (int rc = ensure_rowsweep_layout(c)) return rc;
    if (int rc = forward_profiles(c)) return rc;
    std::vector<double> &xt = W.xt;
    if (int rc = forward_special_transitions(c, multi_hits, hmmer3_compat, xt)) return rc;
    // The wide sweep's work areas, by far the largest of the buffers, come first, as much as any round of this list
    // can ask for (forward_bucket: a round's widest profile and its wavefronts are at most the list's).  Reserved
    // behind the small buffers on a context's first call, a float DB's Forward sweeps measured 1 % slower.
    uint64_t wide_waves = std::min<uint64_t>(wide.pairs, 4ull * c->num_cus);
    if (W.waves_cap) wide_waves = std::min<uint64_t>(wide_waves, W.waves_cap);
    HIP_TRY(c, W.d_work.reserve((uint64_t)work_rows * wide.chunks * DCP_FWD_CHUNK * wide_waves));
    HIP_TRY(c, W.d_off.reserve(off.size()));
    HIP_TRY(c, W.d_xt.reserve(xt.size()));
    HIP_TRY(c, W.d_score.reserve(nscores));
    for (hipEvent_t &e : W.ev)
        if (!e) HIP_TRY(c, hipEventCreate(&e));
    HIP_TRY(c, hipMemcpyAsync(W.d_xt.p, xt.data(), xt.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (!off.empty())
    {
        HIP_TRY(c, hipMemcpyAsync(W.d_off.p, off.data(), off.size() * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream)); // (and whatever was outstanding is done)
    }
    *a = forward_args(c, W.d_xt.p);
    a->work = W.d_work.p;
    if (!off.empty()) a->row_off = W.d_off.p;
    a->out_null = W.d_score.p;
    return DCP_OK;
}

// The list by class, each class in list order, the dearest pairs of a class first; a pair remembers its position pos0 + i
// in the caller's list.  waves: the wavefronts of each class's launch.  list: the same pairs in list order, for the
// kernels that follow the sweeps (upload_round fills it where there are any).
struct ForwardBuckets
{
    unsigned first[5] = {0, 0, 0, 0, 0}, count[4] = {0, 0, 0, 0}, waves[4] = {0, 0, 0, 0};
    unsigned wide_chunks = 0;
    std::vector<dcp_fwd_pair> pairs, list;
};

static void forward_bucket(dcp_gpu_ctx *c, uint32_t const *seq_idx, uint32_t const *profile_idx, unsigned npairs, unsigned pos0,
                           ForwardBuckets &b)
{
    std::vector<unsigned> const order =
        sort_into_classes(npairs, 4, b.first, [&](unsigned i) { return fwd_class(c->core_sizes[profile_idx[i]]); });
    b.pairs.resize(npairs);
    for (int k = 0; k < 4; ++k)
        b.count[k] = b.first[k + 1] - b.first[k];
    for (unsigned j = 0; j < npairs; ++j)
    {
        unsigned const i = order[j];
        b.pairs[j] = dcp_fwd_pair{seq_idx[i], profile_idx[i], pos0 + i};
        if (j >= b.first[3]) b.wide_chunks = std::max(b.wide_chunks, chunks_of(c->core_sizes[profile_idx[i]]));
    }
    // a pair costs its rows times its chunks: the dearest first, so that the wavefronts striding over a class's
    // list end together (pairs of one cost keep their list order)
    auto const cost = [&](dcp_fwd_pair const &p) { return (uint64_t)c->seq_len[p.q] * chunks_of(c->core_sizes[p.prof]); };
    for (int k = 0; k < 4; ++k)
        std::stable_sort(b.pairs.begin() + b.first[k], b.pairs.begin() + b.first[k + 1],
                         [&](dcp_fwd_pair const &x, dcp_fwd_pair const &y) { return cost(x) > cost(y); });
    // wavefronts per launch: a grid's worth (the register-resident classes hold one or two wavefronts per SIMD and
    // leave some waiting, the wide sweep one), striding over the class's list
    for (int k = 0; k < 4; ++k)
    {
        b.waves[k] = (unsigned)std::min<uint64_t>(b.count[k], (uint64_t)(k == 3 ? 4u : 12u) * c->num_cus);
        if (c->sweeps.waves_cap) b.waves[k] = std::min(b.waves[k], c->sweeps.waves_cap);
    }
}

// Pairs [i0, i0 + n) of the list as a round: bucketed by class at d_pairs and, if listed, in list order behind that, and
// the stride of the wide sweep's work areas for them (a.work_stride).  The copies are queued from b: the caller
// synchronises, with whatever it queues of its own, before b leaves scope.
static int upload_round(dcp_gpu_ctx *c, uint32_t const *seq_idx, uint32_t const *profile_idx, unsigned i0, unsigned n,
                        bool listed, ForwardBuckets &b, dcp_fwd_args &a)
{
    auto &W = c->sweeps;
    forward_bucket(c, seq_idx + i0, profile_idx + i0, n, i0, b);
    b.list.resize(listed ? n : 0u);
    for (unsigned i = 0; i < b.list.size(); ++i)
        b.list[i] = dcp_fwd_pair{seq_idx[i0 + i], profile_idx[i0 + i], i0 + i};
    a.work_stride = (uint64_t)DCP_FWD_WORK_ROWS * b.wide_chunks * DCP_FWD_CHUNK;
    HIP_TRY(c, W.d_pairs.reserve((size_t)n + b.list.size()));
    HIP_TRY(c, hipMemcpyAsync(W.d_pairs.p, b.pairs.data(), (size_t)n * sizeof(dcp_fwd_pair), hipMemcpyHostToDevice, c->stream));
    if (listed)
        HIP_TRY(c, hipMemcpyAsync(W.d_pairs.p + n, b.list.data(), (size_t)n * sizeof(dcp_fwd_pair), hipMemcpyHostToDevice, c->stream));
    return DCP_OK;
}

// The round's sweeps over its classes: Forward (alt into the list's second score array), then, of two, Backward (into
// the third).  store: what a sweep leaves beside the scores (dcp_forward.h) -- sweep s's records at d_rec + s x nrows
// records, its two matrices at d_mat + 2 s x ncells.
static int run_sweeps(dcp_gpu_ctx *c, dcp_fwd_args &a, ForwardBuckets const &b, int nsweeps, int store, unsigned npairs,
                      uint64_t nrows, uint64_t ncells)
{
    auto &W = c->sweeps;
    for (int sweep = 0; sweep < nsweeps; ++sweep)
    {
        if (store >= DCP_FWD_STORE_ROWS) a.rows = W.d_rec.p + (sweep ? (size_t)DCP_POST_REC * nrows : 0u);
        if (store >= DCP_FWD_STORE_MATS) a.mat0 = W.d_mat.p + (sweep ? 2u * ncells : 0u), a.mat1 = a.mat0 + ncells;
        a.out_alt = a.out_null + (size_t)(1 + sweep) * npairs;
        for (int k = 0; k < 4; ++k)
        {
            if (b.count[k] == 0) continue;
            a.pairs = W.d_pairs.p + b.first[k];
            a.npairs = b.count[k];
            a.nwaves = b.waves[k];
            if ((sweep ? dcp_backward_launch : dcp_forward_launch)(c->precision, kFwdR[k], store, &a, c->stream))
                return c->fail(DCP_EFAIL, "no %s kernel for %d nodes per lane", sweep ? "Backward" : "Forward", kFwdR[k]);
            HIP_TRY(c, hipGetLastError());
        }
    }
    return DCP_OK;
}

int dcp_gpu_forward_pairs(dcp_gpu_ctx *c, int multi_hits, int hmmer3_compat, uint32_t const *seq_idx,
                          uint32_t const *profile_idx, unsigned npairs, double *null_out, double *alt_out)
{
    if (!c) return DCP_EINVAL;
    if (int rc = forward_check_list(c, seq_idx, profile_idx, npairs, null_out && alt_out)) return rc;
    if (npairs == 0) return DCP_OK;
    auto &W = c->sweeps;
    dcp_fwd_args a{};
    if (int rc = sweeps_setup(c, multi_hits, hmmer3_compat, wide_of_list(c, profile_idx, npairs), (size_t)2u * npairs, {}, &a)) return rc;
    ForwardBuckets b;
    if (int rc = upload_round(c, seq_idx, profile_idx, 0u, npairs, false, b, a)) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // the transitions and the list are up (and whatever was outstanding is done)
    HIP_TRY(c, hipEventRecord(W.ev[0], c->stream));
    if (int rc = run_sweeps(c, a, b, 1, DCP_FWD_STORE_NONE, npairs, 0u, 0u)) return rc;
    HIP_TRY(c, hipEventRecord(W.ev[1], c->stream));
    // into a buffer of the call's own first: the caller's arrays stay untouched if the copy fails
    std::vector<double> out(2u * (size_t)npairs);
    HIP_TRY(c, hipMemcpyAsync(out.data(), W.d_score.p, out.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    float ms = 0.0f;
    HIP_TRY(c, hipEventElapsedTime(&ms, W.ev[0], W.ev[1]));
    W.fwd_ms = ms;
    std::memcpy(null_out, out.data(), (size_t)npairs * sizeof(double));
    std::memcpy(alt_out, out.data() + npairs, (size_t)npairs * sizeof(double));
    return DCP_OK;
}

float dcp_gpu_forward_kernel_ms(dcp_gpu_ctx *c) { return c ? c->sweeps.fwd_ms : -1.0f; }

// ---- The scaled probability-space sweeps (dcp_forward_scaled.hip) ----------------------------------------
// A round's scaled launches over its classes, the pairs at d_pairs as run_sweeps takes them; alt goes `stride` scores
// behind null.  The round's redo list starts empty and has room for every pair of the round.
static int run_scaled_sweeps(dcp_gpu_ctx *c, dcp_fwd_args &a, ForwardBuckets const &b, size_t stride)
{
    auto &W = c->sweeps;
    unsigned const n = b.first[4];
    HIP_TRY(c, W.d_redo.reserve(n));
    HIP_TRY(c, W.d_nredo.reserve(1u));
    HIP_TRY(c, hipMemsetAsync(W.d_nredo.p, 0, sizeof(uint32_t), c->stream));
    a.out_alt = a.out_null + stride;
    for (int k = 0; k < 4; ++k)
    {
        if (b.count[k] == 0) continue;
        a.pairs = W.d_pairs.p + b.first[k];
        a.npairs = b.count[k];
        a.nwaves = b.waves[k];
        if (dcp_forward_scaled_launch(c->precision, kFwdR[k], DCP_FWD_STORE_NONE, &a, W.d_redo.p, W.d_nredo.p, n, W.band ? W.band : (int)DCP_FWS_BAND,
                                      c->stream))
            return c->fail(DCP_EFAIL, "no scaled Forward kernel for %d nodes per lane", kFwdR[k]);
        HIP_TRY(c, hipGetLastError());
    }
    return DCP_OK;
}

// The redo list of the round just launched: waits for the round, and reruns the pairs on it -- those whose values left
// the double range -- by the log-space kernels into the same score arrays.  cap: the round's pairs.  The launches are
// queued; *redone grows by their pairs.
static int rerun_scaled_redo(dcp_gpu_ctx *c, dcp_fwd_args &a, unsigned cap, size_t stride, unsigned *redone)
{
    auto &W = c->sweeps;
    uint32_t n = 0;
    HIP_TRY(c, hipMemcpyAsync(&n, W.d_nredo.p, sizeof n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (n == 0) return DCP_OK;
    if (n > cap) return c->fail(DCP_EFAIL, "the scaled sweeps' redo list holds %u pairs of a round of %u", n, cap);
    std::vector<dcp_fwd_pair> rec(n);
    HIP_TRY(c, hipMemcpy(rec.data(), W.d_redo.p, (size_t)n * sizeof(dcp_fwd_pair), hipMemcpyDeviceToHost));
    // (the device appended them in whatever order the wavefronts ended: by position, so that a call repeats itself)
    std::sort(rec.begin(), rec.end(), [](dcp_fwd_pair const &x, dcp_fwd_pair const &y) { return x.pos < y.pos; });
    std::vector<uint32_t> sq(n), pr(n);
    for (uint32_t i = 0; i < n; ++i)
        sq[i] = rec[i].q, pr[i] = rec[i].prof;
    ForwardBuckets b;
    forward_bucket(c, sq.data(), pr.data(), n, 0u, b);
    for (dcp_fwd_pair &p : b.pairs)
        p.pos = rec[p.pos].pos;
    HIP_TRY(c, W.d_redo_pairs.reserve(n));
    HIP_TRY(c, hipMemcpyAsync(W.d_redo_pairs.p, b.pairs.data(), (size_t)n * sizeof(dcp_fwd_pair), hipMemcpyHostToDevice, c->stream));
    uint64_t const stride_was = a.work_stride;
    a.work_stride = (uint64_t)DCP_FWD_WORK_ROWS * b.wide_chunks * DCP_FWD_CHUNK; // at most the round's: its pairs are of the round
    a.out_alt = a.out_null + stride;
    for (int k = 0; k < 4; ++k)
    {
        if (b.count[k] == 0) continue;
        a.pairs = W.d_redo_pairs.p + b.first[k];
        a.npairs = b.count[k];
        a.nwaves = b.waves[k];
        if (dcp_forward_launch(c->precision, kFwdR[k], DCP_FWD_STORE_NONE, &a, c->stream))
            return c->fail(DCP_EFAIL, "no Forward kernel for %d nodes per lane", kFwdR[k]);
        HIP_TRY(c, hipGetLastError());
    }
    a.work_stride = stride_was;
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // b's records are up
    *redone += n;
    return DCP_OK;
}

int dcp_gpu_forward_pairs_scaled(dcp_gpu_ctx *c, int multi_hits, int hmmer3_compat, uint32_t const *seq_idx,
                                 uint32_t const *profile_idx, unsigned npairs, double *null_out, double *alt_out)
{
    if (!c) return DCP_EINVAL;
    if (int rc = forward_check_list(c, seq_idx, profile_idx, npairs, null_out && alt_out)) return rc;
    if (npairs == 0) return DCP_OK;
    auto &W = c->sweeps;
    dcp_fwd_args a{};
    if (int rc = sweeps_setup(c, multi_hits, hmmer3_compat, wide_of_list(c, profile_idx, npairs), (size_t)2u * npairs, {}, &a,
                              DCP_FWS_WORK_ROWS))
        return rc;
    ForwardBuckets b;
    if (int rc = upload_round(c, seq_idx, profile_idx, 0u, npairs, false, b, a)) return rc;
    a.work_stride = (uint64_t)DCP_FWS_WORK_ROWS * b.wide_chunks * DCP_FWD_CHUNK; // the scaled wide sweep's rows
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // the transitions and the list are up (and whatever was outstanding is done)
    HIP_TRY(c, hipEventRecord(W.ev[0], c->stream));
    if (int rc = run_scaled_sweeps(c, a, b, npairs)) return rc;
    unsigned redone = 0;
    if (int rc = rerun_scaled_redo(c, a, npairs, npairs, &redone)) return rc;
    HIP_TRY(c, hipEventRecord(W.ev[1], c->stream));
    // into a buffer of the call's own first: the caller's arrays stay untouched if the copy fails
    std::vector<double> out(2u * (size_t)npairs);
    HIP_TRY(c, hipMemcpyAsync(out.data(), W.d_score.p, out.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    float ms = 0.0f;
    HIP_TRY(c, hipEventElapsedTime(&ms, W.ev[0], W.ev[1]));
    W.scaled_ms = ms;
    W.scaled_redo = redone;
    std::memcpy(null_out, out.data(), (size_t)npairs * sizeof(double));
    std::memcpy(alt_out, out.data() + npairs, (size_t)npairs * sizeof(double));
    return DCP_OK;
}

unsigned dcp_gpu_forward_scaled_redo_pairs(dcp_gpu_ctx *c) { return c ? c->sweeps.scaled_redo : 0u; }
float dcp_gpu_forward_scaled_kernel_ms(dcp_gpu_ctx *c) { return c ? c->sweeps.scaled_ms : -1.0f; }

// ---- The dense Forward scan: every resident sequence x every resident profile --------------------------
// The host orders the profiles (by class, the wide ones by falling chunk count) and the sequences (by falling length),
// nothing per pair: the outer product is a line of positions (dcp_fwd_dense_args), a round is at most kDenseRound
// consecutive positions of it, its records written by dense_pairs_kernel into d_pairs, where the classes of a round lie
// back to back for run_sweeps.  Everything is queued on the stream without a wait between rounds: the list kernel of
// round r + 1 runs behind the sweeps of round r that read d_pairs.
static constexpr unsigned kDenseRound = 1u << 22; // pairs: 48 MiB of records

static int forward_dense(dcp_gpu_ctx *c, int multi_hits, int hmmer3_compat, bool scaled)
{
    if (!c) return DCP_EINVAL;
    if (c->nprof == 0) return c->fail(DCP_EINVAL, "no profile DB resident");
    if (c->nseqs == 0) return c->fail(DCP_EINVAL, "no sequences resident");
    if (int rc = check_xtrans_precision(c)) return rc;
    uint64_t const total64 = (uint64_t)c->nseqs * c->nprof;
    if (total64 > 0xffffffffull)
        return c->fail(DCP_EINVAL, "%u sequences x %u profiles exceed the 2^32 - 1 pairs of one dense Forward scan", c->nseqs, c->nprof);
    unsigned const total = (unsigned)total64, nseqs = c->nseqs, nprof = c->nprof;
    auto &W = c->sweeps;
    W.dense_valid = false; // the buffer is about to be written

    // the two orders: [nseqs] sequences by falling length, [nprof] profiles by class, the wide ones by falling chunk count
    // (equals keep the caller's order)
    ForwardBuckets b;
    std::vector<uint32_t> order(nseqs);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return c->seq_len[x] > c->seq_len[y]; });
    unsigned cfirst[5];
    std::vector<unsigned> porder = sort_into_classes(nprof, 4, cfirst, [&](unsigned i) { return fwd_class(c->core_sizes[i]); });
    std::stable_sort(porder.begin() + cfirst[3], porder.end(),
                     [&](unsigned x, unsigned y) { return chunks_of(c->core_sizes[x]) > chunks_of(c->core_sizes[y]); });
    order.insert(order.end(), porder.begin(), porder.end());
    WidePairs wide;
    if (cfirst[4] > cfirst[3]) wide.pairs = (uint64_t)nseqs * (cfirst[4] - cfirst[3]), wide.chunks = chunks_of(c->core_sizes[porder[cfirst[3]]]);

    dcp_fwd_args a{};
    unsigned const work_rows = scaled ? (unsigned)DCP_FWS_WORK_ROWS : (unsigned)DCP_FWD_WORK_ROWS;
    if (int rc = sweeps_setup(c, multi_hits, hmmer3_compat, wide, 0u, {}, &a, work_rows)) return rc;
    HIP_TRY(c, W.d_dense.reserve(2u * (size_t)total));
    HIP_TRY(c, W.d_order.reserve(order.size()));
    unsigned const round = std::min(W.dense_round ? W.dense_round : kDenseRound, kDenseRound);
    HIP_TRY(c, W.d_pairs.reserve(std::min(round, total)));
    HIP_TRY(c, hipMemcpyAsync(W.d_order.p, order.data(), order.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // the transitions and the orders are up (and whatever was outstanding is done)
    a.out_null = W.d_dense.p;
    a.work_stride = (uint64_t)work_rows * wide.chunks * DCP_FWD_CHUNK;
    dcp_fwd_dense_args d{};
    d.seq_order = W.d_order.p, d.prof_order = W.d_order.p + nseqs;
    std::copy(cfirst, cfirst + 5, d.class_first);
    d.nseqs = nseqs, d.nprof = nprof;
    d.pairs = W.d_pairs.p;
    HIP_TRY(c, hipEventRecord(W.ev[0], c->stream));
    unsigned redone = 0;
    for (uint64_t t0 = 0; t0 < total; t0 += round)
    {
        uint64_t const t1 = std::min<uint64_t>(t0 + round, total);
        d.t0 = (uint32_t)t0, d.n = (uint32_t)(t1 - t0);
        if (dcp_forward_dense_pairs_launch(&d, c->stream)) return c->fail(DCP_EFAIL, "the dense scan's list kernel refused its round");
        HIP_TRY(c, hipGetLastError());
        // the part of each class in [t0, t1): the classes follow each other on the line, so in d_pairs too
        for (int k = 0; k < 4; ++k)
        {
            uint64_t const lo = std::max<uint64_t>(t0, (uint64_t)nseqs * cfirst[k]), hi = std::min<uint64_t>(t1, (uint64_t)nseqs * cfirst[k + 1]);
            b.count[k] = hi > lo ? (unsigned)(hi - lo) : 0u;
            b.first[k + 1] = b.first[k] + b.count[k];
            b.waves[k] = (unsigned)std::min<uint64_t>(b.count[k], (uint64_t)(k == 3 ? 4u : 12u) * c->num_cus);
            if (W.waves_cap) b.waves[k] = std::min(b.waves[k], W.waves_cap);
        }
        if (!scaled)
        {
            if (int rc = run_sweeps(c, a, b, 1, DCP_FWD_STORE_NONE, total, 0u, 0u)) return rc;
            continue;
        }
        // the scaled sweeps, and the round's redo list before the next round's records overwrite d_pairs' order
        if (int rc = run_scaled_sweeps(c, a, b, total)) return rc;
        if (int rc = rerun_scaled_redo(c, a, d.n, total, &redone)) return rc;
    }
    HIP_TRY(c, hipEventRecord(W.ev[1], c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    float ms = 0.0f;
    HIP_TRY(c, hipEventElapsedTime(&ms, W.ev[0], W.ev[1]));
    W.dense_ms = ms;
    W.dense_valid = true;
    W.dense_scaled = scaled;
    if (scaled) W.scaled_redo = redone;
    return DCP_OK;
}

int dcp_gpu_forward_dense(dcp_gpu_ctx *c, int multi_hits, int hmmer3_compat) { return forward_dense(c, multi_hits, hmmer3_compat, false); }
int dcp_gpu_forward_dense_scaled(dcp_gpu_ctx *c, int multi_hits, int hmmer3_compat) { return forward_dense(c, multi_hits, hmmer3_compat, true); }
int dcp_gpu_forward_dense_is_scaled(dcp_gpu_ctx *c) { return c && c->sweeps.dense_valid && c->sweeps.dense_scaled ? 1 : 0; }

static int forward_dense_ready(dcp_gpu_ctx *c)
{
    if (c->sweeps.dense_valid) return DCP_OK;
    return c->fail(DCP_EINVAL, "no dense Forward scores: none computed by dcp_gpu_forward_dense since the DB, the batch or the "
                               "explicit transitions last changed");
}

int dcp_gpu_fetch_forward_scores(dcp_gpu_ctx *c, double *null_out, double *alt_out)
{
    if (!c) return DCP_EINVAL;
    if (!null_out || !alt_out) return c->fail(DCP_EINVAL, "dcp_gpu_fetch_forward_scores: a null output");
    if (int rc = forward_dense_ready(c)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    size_t const total = (size_t)c->nseqs * c->nprof;
    // into a buffer of the call's own first: the caller's arrays stay untouched if the copy fails
    std::vector<double> out(2u * total);
    HIP_TRY(c, hipMemcpy(out.data(), c->sweeps.d_dense.p, out.size() * sizeof(double), hipMemcpyDeviceToHost));
    std::memcpy(null_out, out.data(), total * sizeof(double));
    std::memcpy(alt_out, out.data() + total, total * sizeof(double));
    return DCP_OK;
}

float dcp_gpu_forward_dense_kernel_ms(dcp_gpu_ctx *c) { return c ? c->sweeps.dense_ms : -1.0f; }

// ---- Backward sweep and posterior rows of a pair list (dcp_posterior.hip) -------------------------------------------
// The list runs in rounds of consecutive pairs whose row records -- 2 x DCP_POST_REC doubles a row -- fit the budget (a
// single pair that exceeds it gets a round of its own).  A round: the row-storing Forward launches by class, the
// Backward launches by class, the combining kernel, the round's rows copied out; then the next.
//
// The scaled call differs in the sweeps alone: the row-storing scaled Forward and the scaled Backward by class,
// then one wait for the round's redo list -- the pairs either sweep could not return -- which the log-space sweeps rerun
// into the same record and score slots before the combining kernel runs.
static int run_scaled_posterior_sweeps(dcp_gpu_ctx *c, dcp_fwd_args &a, ForwardBuckets const &b, unsigned npairs, uint64_t nrows,
                                       unsigned *redone)
{
    auto &W = c->sweeps;
    unsigned const n = b.first[4], cap = 2u * n; // both sweeps may flag the same pair
    int const band = W.band ? W.band : (int)DCP_FWS_BAND;
    double *const rows_f = W.d_rec.p, *const rows_b = W.d_rec.p + (size_t)DCP_POST_REC * nrows;
    double *const alt_fwd = a.out_null + npairs, *const alt_bwd = a.out_null + 2u * (size_t)npairs;
    uint64_t const chunk_cols = (uint64_t)b.wide_chunks * DCP_FWD_CHUNK, stride_was = a.work_stride;
    HIP_TRY(c, W.d_redo.reserve(cap));
    HIP_TRY(c, W.d_nredo.reserve(1u));
    HIP_TRY(c, hipMemsetAsync(W.d_nredo.p, 0, sizeof(uint32_t), c->stream));
    for (int sweep = 0; sweep < 2; ++sweep)
    {
        a.rows = sweep ? rows_b : rows_f;
        a.out_alt = sweep ? alt_bwd : alt_fwd;
        a.work_stride = (uint64_t)(sweep ? DCP_BWS_WORK_ROWS : DCP_FWS_WORK_ROWS) * chunk_cols;
        for (int k = 0; k < 4; ++k)
        {
            if (b.count[k] == 0) continue;
            a.pairs = W.d_pairs.p + b.first[k];
            a.npairs = b.count[k];
            a.nwaves = b.waves[k];
            int const rc = sweep ? dcp_backward_scaled_launch(c->precision, kFwdR[k], &a, rows_f, alt_fwd, W.d_redo.p, W.d_nredo.p, cap,
                                                              band, c->stream)
                                 : dcp_forward_scaled_launch(c->precision, kFwdR[k], DCP_FWD_STORE_ROWS, &a, W.d_redo.p, W.d_nredo.p,
                                                             cap, band, c->stream);
            if (rc) return c->fail(DCP_EFAIL, "no scaled %s kernel for %d nodes per lane", sweep ? "Backward" : "Forward", kFwdR[k]);
            HIP_TRY(c, hipGetLastError());
        }
    }
    a.work_stride = stride_was;
    // the round's redo list: sorted by position and without the pairs both sweeps flagged, so that a call repeats itself
    uint32_t nr = 0;
    HIP_TRY(c, hipMemcpyAsync(&nr, W.d_nredo.p, sizeof nr, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (nr == 0) return DCP_OK;
    if (nr > cap) return c->fail(DCP_EFAIL, "the scaled sweeps' redo list holds %u pairs of a round of %u", nr, n);
    std::vector<dcp_fwd_pair> rec(nr);
    HIP_TRY(c, hipMemcpy(rec.data(), W.d_redo.p, (size_t)nr * sizeof(dcp_fwd_pair), hipMemcpyDeviceToHost));
    std::sort(rec.begin(), rec.end(), [](dcp_fwd_pair const &x, dcp_fwd_pair const &y) { return x.pos < y.pos; });
    rec.erase(std::unique(rec.begin(), rec.end(), [](dcp_fwd_pair const &x, dcp_fwd_pair const &y) { return x.pos == y.pos; }), rec.end());
    nr = (uint32_t)rec.size();
    std::vector<uint32_t> sq(nr), pr(nr);
    for (uint32_t i = 0; i < nr; ++i)
        sq[i] = rec[i].q, pr[i] = rec[i].prof;
    ForwardBuckets rb;
    forward_bucket(c, sq.data(), pr.data(), nr, 0u, rb);
    for (dcp_fwd_pair &p : rb.pairs)
        p.pos = rec[p.pos].pos;
    HIP_TRY(c, W.d_redo_pairs.reserve(nr));
    HIP_TRY(c, hipMemcpyAsync(W.d_redo_pairs.p, rb.pairs.data(), (size_t)nr * sizeof(dcp_fwd_pair), hipMemcpyHostToDevice, c->stream));
    // both sweeps in log space, so that the two records agree: dcp_gpu_posterior_pairs' launches over the redo list
    a.work_stride = (uint64_t)DCP_FWD_WORK_ROWS * rb.wide_chunks * DCP_FWD_CHUNK; // at most the round's: its pairs are of the round
    for (int sweep = 0; sweep < 2; ++sweep)
    {
        a.rows = sweep ? rows_b : rows_f;
        a.out_alt = sweep ? alt_bwd : alt_fwd;
        for (int k = 0; k < 4; ++k)
        {
            if (rb.count[k] == 0) continue;
            a.pairs = W.d_redo_pairs.p + rb.first[k];
            a.npairs = rb.count[k];
            a.nwaves = rb.waves[k];
            if ((sweep ? dcp_backward_launch : dcp_forward_launch)(c->precision, kFwdR[k], DCP_FWD_STORE_ROWS, &a, c->stream))
                return c->fail(DCP_EFAIL, "no %s kernel for %d nodes per lane", sweep ? "Backward" : "Forward", kFwdR[k]);
            HIP_TRY(c, hipGetLastError());
        }
    }
    a.work_stride = stride_was;
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // rb's records are up
    *redone += nr;
    return DCP_OK;
}

// What becomes of a round's rows: copied out into the caller's arrays (dcp_gpu_posterior_pairs), or turned into envelope
// records on the device, of which the counts and the records alone are copied out (dcp_gpu_envelope_pairs).
struct PosteriorSink
{
    uint64_t *row_off = nullptr;
    double *begin_out = nullptr, *end_out = nullptr, *core_out = nullptr;
    uint64_t cap_rows = 0;
    bool envelopes = false;
    double hi = 0.0, lo = 0.0;
    unsigned min_len = 0;
    dcp_envelope *env_out = nullptr;
    uint64_t cap_env = 0;
    uint64_t *env_off = nullptr;
};

// A round's envelopes from its rows on the device: the count pass, the counts copied out and scanned on the host, the
// write pass, the records copied out behind those of the rounds before.  ea: the round's row offsets, list length, planes,
// thresholds and first pair.  count_out [ea.nlist].  The wavefronts take dcp_gpu_test_set_forward_waves' cap.  *own_ms
// grows by the two passes' time, by events of their own (ev_env).  Returns synchronised.
static int envelope_round(dcp_gpu_ctx *c, dcp_env_args ea, uint32_t *count_out, std::vector<dcp_envelope> &recs, float *own_ms)
{
    auto &W = c->sweeps;
    unsigned const n = ea.nlist;
    for (hipEvent_t &e : W.ev_env)
        if (!e) HIP_TRY(c, hipEventCreate(&e));
    ea.nwaves = (unsigned)std::min<uint64_t>(n, 32ull * c->num_cus); // eight wavefronts per SIMD: the passes wait for memory
    if (W.waves_cap) ea.nwaves = std::min(ea.nwaves, W.waves_cap);
    HIP_TRY(c, W.d_env_count.reserve(n));
    HIP_TRY(c, W.d_env_at.reserve((size_t)n + 1u));
    ea.count = W.d_env_count.p, ea.env_at = W.d_env_at.p;
    HIP_TRY(c, hipEventRecord(W.ev_env[0], c->stream));
    if (dcp_envelopes_count_launch(&ea, c->stream)) return c->fail(DCP_EFAIL, "the envelope count pass refused a round of %u pairs", n);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(W.ev_env[1], c->stream));
    HIP_TRY(c, hipMemcpyAsync(count_out, W.d_env_count.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    float ms = 0.0f;
    HIP_TRY(c, hipEventElapsedTime(&ms, W.ev_env[0], W.ev_env[1]));
    *own_ms += ms;
    std::vector<uint64_t> at((size_t)n + 1u, 0u);
    for (unsigned i = 0; i < n; ++i)
        at[i + 1u] = at[i] + count_out[i];
    uint64_t const total = at[n];
    if (total == 0u) return DCP_OK;
    HIP_TRY(c, W.d_env.reserve(total));
    ea.env = W.d_env.p;
    HIP_TRY(c, hipMemcpyAsync(W.d_env_at.p, at.data(), at.size() * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipEventRecord(W.ev_env[0], c->stream));
    if (dcp_envelopes_write_launch(&ea, c->stream)) return c->fail(DCP_EFAIL, "the envelope write pass refused a round of %u pairs", n);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(W.ev_env[1], c->stream));
    size_t const had = recs.size();
    recs.resize(had + total);
    HIP_TRY(c, hipMemcpyAsync(recs.data() + had, W.d_env.p, total * sizeof(dcp_envelope), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // (and `at` is up)
    HIP_TRY(c, hipEventElapsedTime(&ms, W.ev_env[0], W.ev_env[1]));
    *own_ms += ms;
    return DCP_OK;
}

static int posterior_pairs(dcp_gpu_ctx *c, bool scaled, int multi_hits, int hmmer3_compat, uint32_t const *seq_idx,
                           uint32_t const *profile_idx, unsigned npairs, PosteriorSink const &s, double *alt_fwd_out,
                           double *alt_bwd_out)
{
    if (!c) return DCP_EINVAL;
    if (int rc = forward_check_list(c, seq_idx, profile_idx, npairs, alt_fwd_out && alt_bwd_out)) return rc;
    if (s.envelopes)
    {
        if (!s.env_off) return c->fail(DCP_EINVAL, "a pair list without its envelope offsets");
        if (dcp_env_thresholds_refused(s.hi, s.lo))
            return c->fail(DCP_EINVAL, "envelope thresholds hi %g, lo %g: neither may be NaN, and lo may not exceed hi", s.hi, s.lo);
        if (npairs && s.cap_env && !s.env_out) return c->fail(DCP_EINVAL, "a pair list without its envelope array");
    }
    else if (!s.row_off) return c->fail(DCP_EINVAL, "a pair list without its row offsets");
    std::vector<uint64_t> off((size_t)npairs + 1u, 0u);
    for (unsigned i = 0; i < npairs; ++i)
        off[i + 1u] = off[i] + c->seq_len[seq_idx[i]] + 1u;
    if (!s.envelopes)
    {
        uint64_t const need = off[npairs];
        if (need > s.cap_rows)
            return c->fail(DCP_EINVAL, "the list needs %llu rows, the arrays hold %llu", (unsigned long long)need,
                           (unsigned long long)s.cap_rows);
        if (npairs && (!s.begin_out || !s.end_out || !s.core_out)) return c->fail(DCP_EINVAL, "a pair list without its row arrays");
    }
    if (npairs == 0)
    {
        (s.envelopes ? s.env_off : s.row_off)[0] = 0u;
        return DCP_OK;
    }
    auto &W = c->sweeps;
    dcp_fwd_args a{};
    if (int rc = sweeps_setup(c, multi_hits, hmmer3_compat, wide_of_list(c, profile_idx, npairs), (size_t)3u * npairs, off, &a,
                              scaled ? (unsigned)DCP_FWS_WORK_ROWS : (unsigned)DCP_FWD_WORK_ROWS)) // (the widest of a round's sweeps)
        return rc;
    // a round's row records fit the budget; room for the largest round's before the first one runs
    uint64_t const budget = W.post_budget ? W.post_budget : (uint64_t)1u << 30;
    auto const bytes_of = [&](unsigned i0, unsigned i1) { return (off[i1] - off[i0]) * (2u * DCP_POST_REC * sizeof(double)); };
    uint64_t round_rows = 0;
    for (unsigned i0 = 0, i1; i0 < npairs; i0 = i1)
    {
        i1 = round_end(i0, npairs, budget, bytes_of);
        round_rows = std::max(round_rows, off[i1] - off[i0]);
    }
    HIP_TRY(c, W.d_rec.reserve(2u * DCP_POST_REC * round_rows));
    HIP_TRY(c, W.d_rows.reserve(3u * round_rows));

    double *const d_fwd = W.d_score.p + npairs;
    dcp_post_args pa{};
    pa.profs = a.profs, pa.en = a.en;
    pa.seq_words = a.seq_words, pa.seq_woff = a.seq_woff, pa.seq_len = a.seq_len;
    pa.alt_fwd = d_fwd;

    std::vector<double> rows;
    std::vector<uint32_t> env_count(s.envelopes ? npairs : 0u, 0u); // the call's own copy of every pair's count and of the
    std::vector<dcp_envelope> env;                                   // records: the caller's arrays wait for the total
    float ms_total = 0.0f, env_own_ms = 0.0f;
    unsigned redone = 0;
    for (unsigned i0 = 0, i1; i0 < npairs; i0 = i1)
    {
        i1 = round_end(i0, npairs, budget, bytes_of);
        unsigned const n = i1 - i0;
        uint64_t const nrows = off[i1] - off[i0];
        ForwardBuckets b;
        if (int rc = upload_round(c, seq_idx, profile_idx, i0, n, true, b, a)) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        a.row_base = off[i0];
        HIP_TRY(c, hipEventRecord(W.ev[0], c->stream));
        if (int rc = scaled ? run_scaled_posterior_sweeps(c, a, b, npairs, nrows, &redone)
                            : run_sweeps(c, a, b, 2, DCP_FWD_STORE_ROWS, npairs, nrows, 0u))
            return rc;
        pa.list = W.d_pairs.p + n, pa.nlist = n, pa.row_off = W.d_off.p + i0;
        pa.rows_f = W.d_rec.p, pa.rows_b = W.d_rec.p + (size_t)DCP_POST_REC * nrows;
        pa.begin = W.d_rows.p, pa.end = pa.begin + nrows, pa.core = pa.end + nrows;
        if (dcp_posterior_combine_launch(c->precision, &pa, nrows, c->stream))
            return c->fail(DCP_EFAIL, "no combining kernel for a round of %llu rows", (unsigned long long)nrows);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipEventRecord(W.ev[1], c->stream));
        if (s.envelopes)
        {
            // the rows stay where they are: the round's counts and records alone are copied out
            dcp_env_args ea{};
            ea.row_off = pa.row_off, ea.nlist = n, ea.begin = pa.begin, ea.end = pa.end, ea.core = pa.core;
            ea.hi = s.hi, ea.lo = s.lo, ea.min_len = s.min_len, ea.pair_base = i0;
            if (int rc = envelope_round(c, ea, env_count.data() + i0, env, &env_own_ms)) return rc;
            float ms = 0.0f;
            HIP_TRY(c, hipEventElapsedTime(&ms, W.ev[0], W.ev[1]));
            ms_total += ms;
            continue;
        }
        // into a buffer of the call's own first: the caller's arrays stay untouched if this round's copy fails
        rows.resize(3u * (size_t)nrows);
        HIP_TRY(c, hipMemcpyAsync(rows.data(), W.d_rows.p, rows.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        float ms = 0.0f;
        HIP_TRY(c, hipEventElapsedTime(&ms, W.ev[0], W.ev[1]));
        ms_total += ms;
        std::memcpy(s.begin_out + off[i0], rows.data(), (size_t)nrows * sizeof(double));
        std::memcpy(s.end_out + off[i0], rows.data() + nrows, (size_t)nrows * sizeof(double));
        std::memcpy(s.core_out + off[i0], rows.data() + 2u * nrows, (size_t)nrows * sizeof(double));
    }
    std::vector<double> score(2u * (size_t)npairs);
    HIP_TRY(c, hipMemcpy(score.data(), d_fwd, score.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (s.envelopes)
    {
        W.env_ms = ms_total + env_own_ms, W.env_own_ms = env_own_ms; // the call ran all its rounds, whatever cap_env makes of it
        if (scaled) W.post_scaled_redo = redone;
        s.env_off[0] = 0u;
        for (unsigned i = 0; i < npairs; ++i)
            s.env_off[i + 1u] = s.env_off[i] + env_count[i];
        uint64_t const total = s.env_off[npairs];
        if (total != env.size()) return c->fail(DCP_EFAIL, "the rounds counted %llu envelopes and wrote %llu", (unsigned long long)total,
                                                (unsigned long long)env.size());
        if (total > s.cap_env)
            return c->fail(DCP_ENOMEM, "the list has %llu envelopes, the array holds %llu", (unsigned long long)total,
                           (unsigned long long)s.cap_env);
        if (total) std::memcpy(s.env_out, env.data(), (size_t)total * sizeof(dcp_envelope));
        std::memcpy(alt_fwd_out, score.data(), (size_t)npairs * sizeof(double));
        std::memcpy(alt_bwd_out, score.data() + npairs, (size_t)npairs * sizeof(double));
        return DCP_OK;
    }
    std::memcpy(alt_fwd_out, score.data(), (size_t)npairs * sizeof(double));
    std::memcpy(alt_bwd_out, score.data() + npairs, (size_t)npairs * sizeof(double));
    std::memcpy(s.row_off, off.data(), off.size() * sizeof(uint64_t));
    if (scaled) W.post_scaled_ms = ms_total, W.post_scaled_redo = redone;
    else W.post_ms = ms_total;
    return DCP_OK;
}

int dcp_gpu_posterior_pairs(dcp_gpu_ctx *c, int multi_hits, int hmmer3_compat, uint32_t const *seq_idx,
                            uint32_t const *profile_idx, unsigned npairs, uint64_t *row_off, double *begin_out,
                            double *end_out, double *core_out, uint64_t cap_rows, double *alt_fwd_out, double *alt_bwd_out)
{
    PosteriorSink s;
    s.row_off = row_off, s.begin_out = begin_out, s.end_out = end_out, s.core_out = core_out, s.cap_rows = cap_rows;
    return posterior_pairs(c, false, multi_hits, hmmer3_compat, seq_idx, profile_idx, npairs, s, alt_fwd_out, alt_bwd_out);
}

int dcp_gpu_posterior_pairs_scaled(dcp_gpu_ctx *c, int multi_hits, int hmmer3_compat, uint32_t const *seq_idx,
                                   uint32_t const *profile_idx, unsigned npairs, uint64_t *row_off, double *begin_out,
                                   double *end_out, double *core_out, uint64_t cap_rows, double *alt_fwd_out, double *alt_bwd_out)
{
    PosteriorSink s;
    s.row_off = row_off, s.begin_out = begin_out, s.end_out = end_out, s.core_out = core_out, s.cap_rows = cap_rows;
    return posterior_pairs(c, true, multi_hits, hmmer3_compat, seq_idx, profile_idx, npairs, s, alt_fwd_out, alt_bwd_out);
}

float dcp_gpu_posterior_kernel_ms(dcp_gpu_ctx *c) { return c ? c->sweeps.post_ms : -1.0f; }
unsigned dcp_gpu_posterior_scaled_redo_pairs(dcp_gpu_ctx *c) { return c ? c->sweeps.post_scaled_redo : 0u; }
float dcp_gpu_posterior_scaled_kernel_ms(dcp_gpu_ctx *c) { return c ? c->sweeps.post_scaled_ms : -1.0f; }

// ---- Posterior envelopes of a pair list (dcp_envelopes.hip) ----------------------------------------------
// posterior_pairs with the other sink: everything up to a round's combining kernel is the posterior call's of the same
// sweeps; the round's rows then stay in d_rows, where the two envelope passes read them (envelope_round).
int dcp_gpu_envelope_pairs(dcp_gpu_ctx *c, int multi_hits, int hmmer3_compat, int scaled, uint32_t const *seq_idx,
                           uint32_t const *profile_idx, unsigned npairs, double hi, double lo, unsigned min_len,
                           struct dcp_envelope *env_out, uint64_t cap_env, uint64_t *env_off, double *alt_fwd_out,
                           double *alt_bwd_out)
{
    PosteriorSink s;
    s.envelopes = true, s.hi = hi, s.lo = lo, s.min_len = min_len;
    s.env_out = env_out, s.cap_env = cap_env, s.env_off = env_off;
    return posterior_pairs(c, scaled != 0, multi_hits, hmmer3_compat, seq_idx, profile_idx, npairs, s, alt_fwd_out, alt_bwd_out);
}

float dcp_gpu_envelope_kernel_ms(dcp_gpu_ctx *c) { return c ? c->sweeps.env_ms : -1.0f; }

// ---- The posterior-decoded alignment of a pair list (dcp_mea.hip) ---------------------------------------------------
// The list runs in rounds of consecutive pairs whose matrices (P, Q, bM, bI: 32 bytes a cell), cell choices (2 bytes a
// cell), row records (80 bytes a row) and row choices (8 bytes a row) fit the budget (a single pair that exceeds it gets
// a round of its own).  A round: the matrix-storing Forward launches by class, the Backward launches by class, the
// max-plus sweep and the walk over the round's pairs in list order; a pair whose path is longer than the first estimate
// (L + M + 16 steps) makes the round's walk run once more at the exact counts; the round's steps copied out; then the next.
static constexpr uint64_t kMeaCellBytes = 4u * sizeof(double) + sizeof(uint16_t);
static constexpr uint64_t kMeaRowBytes = 2u * DCP_POST_REC * sizeof(double) + DCP_MEA_ROWC * sizeof(uint32_t);

int dcp_gpu_mea_pairs(dcp_gpu_ctx *c, int multi_hits, int hmmer3_compat, uint32_t const *seq_idx, uint32_t const *profile_idx,
                      unsigned npairs, struct dcp_step *steps_out, unsigned cap_steps, uint32_t *step_off, double *post_out,
                      double *gain_out, double *alt_fwd_out)
{
    if (!c) return DCP_EINVAL;
    if (int rc = forward_check_list(c, seq_idx, profile_idx, npairs, gain_out && alt_fwd_out)) return rc;
    if (!step_off) return c->fail(DCP_EINVAL, "a pair list without its step offsets");
    if (npairs && cap_steps && !steps_out) return c->fail(DCP_EINVAL, "a pair list without its step array");
    if (npairs == 0)
    {
        step_off[0] = 0u;
        return DCP_OK;
    }
    // rows and cells of the list, one array: [npairs + 1] row offsets, then [npairs + 1] cell offsets
    size_t const no = (size_t)npairs + 1u;
    std::vector<uint64_t> off(2u * no, 0u);
    uint64_t *const roff = off.data(), *const coff = off.data() + no;
    for (unsigned i = 0; i < npairs; ++i)
    {
        uint64_t const rows = (uint64_t)c->seq_len[seq_idx[i]] + 1u;
        roff[i + 1u] = roff[i] + rows;
        coff[i + 1u] = coff[i] + rows * c->core_sizes[profile_idx[i]];
    }
    auto &W = c->sweeps;
    dcp_fwd_args a{};
    if (int rc = sweeps_setup(c, multi_hits, hmmer3_compat, wide_of_list(c, profile_idx, npairs), (size_t)4u * npairs, off, &a)) return rc;
    a.cell_off = W.d_off.p + no;
    uint64_t const budget = W.mea_budget ? W.mea_budget : (uint64_t)8u << 30;
    auto const bytes_of = [&](unsigned i0, unsigned i1) {
        return (coff[i1] - coff[i0]) * kMeaCellBytes + (roff[i1] - roff[i0]) * kMeaRowBytes;
    };
    double *const d_fwd = W.d_score.p + npairs, *const d_gain = d_fwd + 2u * (size_t)npairs;
    dcp_mea_args ma{};
    ma.profs = a.profs, ma.tab = a.tab, ma.trans = a.trans, ma.ei = a.ei, ma.en = a.en;
    ma.seq_words = a.seq_words, ma.seq_woff = a.seq_woff, ma.seq_len = a.seq_len, ma.xtrans = a.xtrans;
    ma.alt_fwd = d_fwd, ma.gain = d_gain;

    // the call's own copy of every pair's steps, in list order: the caller's arrays stay untouched until all is known
    std::vector<uint32_t> steps, round_steps;
    std::vector<double> post, round_post;
    std::vector<uint64_t> count((size_t)npairs, 0u), idx;
    float ms_total = 0.0f;
    for (unsigned i0 = 0, i1; i0 < npairs; i0 = i1)
    {
        i1 = round_end(i0, npairs, budget, bytes_of);
        unsigned const n = i1 - i0;
        uint64_t const nrows = roff[i1] - roff[i0], ncells = coff[i1] - coff[i0];
        unsigned chunks = 0; // of the round's widest profile
        idx.assign(3u * (size_t)n, 0u); // where a pair's steps go, how many fit, how many there are
        uint64_t nsteps_cap = 0;
        for (unsigned i = 0; i < n; ++i)
        {
            unsigned const M = c->core_sizes[profile_idx[i0 + i]];
            chunks = std::max(chunks, chunks_of(M));
            idx[i] = nsteps_cap, idx[n + i] = (uint64_t)c->seq_len[seq_idx[i0 + i]] + M + 16u;
            nsteps_cap += idx[n + i];
        }
        unsigned mea_waves = (unsigned)std::min<uint64_t>(n, 4ull * c->num_cus); // one wavefront per SIMD
        if (W.waves_cap) mea_waves = std::min(mea_waves, W.waves_cap);
        uint64_t const mea_stride = (uint64_t)DCP_MEA_WORK_ROWS * chunks * DCP_FWD_CHUNK;
        HIP_TRY(c, W.d_mea_work.reserve(mea_stride * mea_waves));
        HIP_TRY(c, W.d_rec.reserve(2u * DCP_POST_REC * nrows));
        HIP_TRY(c, W.d_mat.reserve(4u * ncells));
        HIP_TRY(c, W.d_cell.reserve(ncells));
        HIP_TRY(c, W.d_rowc.reserve(DCP_MEA_ROWC * nrows));
        HIP_TRY(c, W.d_start.reserve(n));
        HIP_TRY(c, W.d_step_idx.reserve(idx.size()));
        HIP_TRY(c, W.d_steps.reserve(nsteps_cap));
        HIP_TRY(c, W.d_post.reserve(nsteps_cap));
        ForwardBuckets b;
        if (int rc = upload_round(c, seq_idx, profile_idx, i0, n, true, b, a)) return rc;
        HIP_TRY(c, hipMemcpyAsync(W.d_step_idx.p, idx.data(), idx.size() * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream)); // the lists may leave scope on any error below
        a.row_base = roff[i0], a.cell_base = coff[i0];
        HIP_TRY(c, hipEventRecord(W.ev[0], c->stream));
        if (int rc = run_sweeps(c, a, b, 2, DCP_FWD_STORE_MATS, npairs, nrows, ncells)) return rc;
        ma.list = W.d_pairs.p + n, ma.nlist = n, ma.nwaves = mea_waves;
        ma.row_off = W.d_off.p + i0, ma.cell_off = W.d_off.p + no + i0;
        ma.P = W.d_mat.p, ma.Q = ma.P + ncells, ma.bM = ma.Q + ncells, ma.bI = ma.bM + ncells;
        ma.rows_f = W.d_rec.p, ma.rows_b = W.d_rec.p + (size_t)DCP_POST_REC * nrows;
        ma.cell = W.d_cell.p, ma.rowc = W.d_rowc.p, ma.start = W.d_start.p;
        ma.work = W.d_mea_work.p, ma.work_stride = mea_stride;
        if (dcp_mea_sweep_launch(c->precision, &ma, c->stream)) return c->fail(DCP_EFAIL, "no max-plus sweep kernel");
        HIP_TRY(c, hipGetLastError());
        for (int walk = 0; walk < 2; ++walk)
        {
            ma.steps = W.d_steps.p, ma.post = W.d_post.p;
            ma.step_at = W.d_step_idx.p, ma.step_cap = W.d_step_idx.p + n, ma.nsteps = W.d_step_idx.p + 2u * (size_t)n;
            if (dcp_mea_walk_launch(c->precision, &ma, c->stream)) return c->fail(DCP_EFAIL, "no walk kernel");
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipEventRecord(W.ev[1], c->stream));
            HIP_TRY(c, hipMemcpyAsync(idx.data() + 2u * (size_t)n, ma.nsteps, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            float ms = 0.0f;
            HIP_TRY(c, hipEventElapsedTime(&ms, W.ev[0], W.ev[1]));
            ms_total += ms;
            bool fits = true;
            for (unsigned i = 0; i < n; ++i)
                fits = fits && idx[2u * (size_t)n + i] <= idx[n + i];
            if (fits) break;
            if (walk) return c->fail(DCP_EFAIL, "a path grew between two walks of the same choices");
            // once more at the exact counts
            nsteps_cap = 0;
            for (unsigned i = 0; i < n; ++i)
            {
                idx[i] = nsteps_cap, idx[n + i] = idx[2u * (size_t)n + i];
                nsteps_cap += idx[n + i];
            }
            HIP_TRY(c, W.d_steps.reserve(nsteps_cap));
            HIP_TRY(c, W.d_post.reserve(nsteps_cap));
            HIP_TRY(c, hipMemcpyAsync(W.d_step_idx.p, idx.data(), 2u * (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipEventRecord(W.ev[0], c->stream));
        }
        round_steps.resize(nsteps_cap), round_post.resize(nsteps_cap);
        HIP_TRY(c, hipMemcpyAsync(round_steps.data(), W.d_steps.p, nsteps_cap * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(round_post.data(), W.d_post.p, nsteps_cap * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (unsigned i = 0; i < n; ++i)
        {
            uint64_t const ns = idx[2u * (size_t)n + i];
            count[i0 + i] = ns;
            steps.insert(steps.end(), round_steps.begin() + idx[i], round_steps.begin() + idx[i] + ns);
            post.insert(post.end(), round_post.begin() + idx[i], round_post.begin() + idx[i] + ns);
        }
    }
    std::vector<double> score(3u * (size_t)npairs); // alt by Forward, alt by Backward, gain
    HIP_TRY(c, hipMemcpy(score.data(), d_fwd, score.size() * sizeof(double), hipMemcpyDeviceToHost));
    double const *const gain = score.data() + 2u * (size_t)npairs;
    uint64_t total = 0;
    for (unsigned i = 0; i < npairs; ++i)
    {
        if (count[i] == 0u && gain[i] != -std::numeric_limits<double>::infinity())
            return c->fail(DCP_EFAIL, "pair %u has a gain and no path", i);
        total += count[i];
    }
    if (total > 0xffffffffull) return c->fail(DCP_EFAIL, "the list's paths hold %llu steps, more than 32 bits count", (unsigned long long)total);
    W.mea_ms = ms_total; // the call ran all its rounds, whatever cap_steps makes of it
    step_off[0] = 0u;
    for (unsigned i = 0; i < npairs; ++i)
        step_off[i + 1u] = step_off[i] + (uint32_t)count[i];
    if (total > cap_steps)
        return c->fail(DCP_ENOMEM, "the list's paths hold %llu steps, the arrays hold %u", (unsigned long long)total, cap_steps);
    static_assert(sizeof(dcp_step) == sizeof(uint32_t), "a step is one word: state_id | seqlen << 16");
    if (total) std::memcpy(steps_out, steps.data(), (size_t)total * sizeof(uint32_t));
    if (total && post_out) std::memcpy(post_out, post.data(), (size_t)total * sizeof(double));
    std::memcpy(alt_fwd_out, score.data(), (size_t)npairs * sizeof(double));
    std::memcpy(gain_out, gain, (size_t)npairs * sizeof(double));
    return DCP_OK;
}

float dcp_gpu_mea_kernel_ms(dcp_gpu_ctx *c) { return c ? c->sweeps.mea_ms : -1.0f; }

// A redo list was full and lost pairs: the scan is repeated with the row-sweep kernel, which needs no list.
static int rerun_with_rowsweep(dcp_gpu_ctx *c)
{
    // (copies: the new scan begins with a fresh record)
    struct dcp_scan_params prm = c->last.prm;
    unsigned const q0 = c->last.q0, q1 = c->last.q1;
    prm.kernel = 1;
    if (int rc = dcp_gpu_scan_range(c, &prm, q0, q1)) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return DCP_OK;
}

// (declared ahead of the shared templates)
// Wait for the stream; after a query-lane scan also look at the redo counters.  A redo list
// that overflowed (> 2^26 pairs of one size class needed the row sweep) lost pairs: the scan is
// repeated with the row-sweep kernel (rerun_with_rowsweep).
static int finish_scan(dcp_gpu_ctx *c)
{
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->last.redo_pending64) // the f64 query-lane kernel's lists: [4] pairs appended, [1] overflow flag
    {
        c->last.redo_pending64 = false;
        unsigned n[5];
        HIP_TRY(c, hipMemcpy(n, c->f64.d_redo_n.p, sizeof n, hipMemcpyDeviceToHost));
        c->last.redo_pairs = (unsigned)std::min<uint64_t>((uint64_t)n[0] + n[1] + n[2] + n[3], 0xffffffffull);
        if (n[4] == 0) return DCP_OK;
        // the double scan's rerun begins with a fresh record, the count 0 (scan64): what the lists took stays the figure
        // reported.  (The float row sweep's does the same, and there 0 is what is reported.)
        unsigned const redone = c->last.redo_pairs;
        if (int rc = rerun_with_rowsweep(c)) return rc;
        c->last.redo_pairs = redone;
        return DCP_OK;
    }
    if (!c->last.redo_pending && !c->last.ring_check_pending) return DCP_OK;
    bool const redo = c->last.redo_pending;
    c->last.redo_pending = false;
    c->last.ring_check_pending = false;
    unsigned n[DCP_MAX_CLASSES + 2];
    HIP_TRY(c, hipMemcpy(n, c->d_redo_n.p, sizeof n, hipMemcpyDeviceToHost));
    // the two-stage kernel's ring hand-shake ran into its poll bound (dcp_qlane.hip, ring_wait): the stages drained,
    // but rows were computed from values their partner never wrote -- nothing of this scan can be used
    if (n[DCP_MAX_CLASSES + 1])
    {
        c->last.scanned = false;
        return c->fail(DCP_EFAIL, "query-lane kernel: the LDS ring hand-shake between the two stages timed out; the scan's results are invalid");
    }
    if (!redo) return DCP_OK;
    uint64_t tot = 0;
    for (int k = 0; k < kNumClasses; ++k)
        tot += n[k];
    c->last.redo_pairs = (unsigned)std::min<uint64_t>(tot, 0xffffffffull);
    if (n[DCP_MAX_CLASSES] == 0) return DCP_OK;
    return rerun_with_rowsweep(c);
}

#ifdef DCP_TEST_HOOKS
int dcp_gpu_test_set_rowsweep_variant(dcp_gpu_ctx *c, int stg, unsigned bw)
{
    if (!c) return DCP_EINVAL;
    c->rs_force_stg = stg;
    c->rs_force_bw = bw & 0xffu;
    c->rs_pad_lds = ((bw >> 8) & 0xffu) * 1024u; // bits 8..15: KiB of unused LDS per block (fewer blocks per CU)
    c->rs_force_pf = (int)((bw >> 16) & 1u);      // bit 16: the two-rows-ahead prefetch variant
    c->rs_force_R = (int)((bw >> 20) & 15u);      // bits 20..23: only the class with this many nodes per lane (0: all)
    c->seg_mode = ((bw >> 24) & 3u) == 1u ? 0 : ((bw >> 24) & 3u) == 2u ? 1 : -1; // bits 24..25: 1 = never the segmented sweep, 2 = always
    c->mp_mode = ((bw >> 26) & 3u) == 1u ? 0 : ((bw >> 26) & 3u) == 2u ? 1 : -1;  // bits 26..27: 1 = never K profiles per wavefront, 2 = always
    return DCP_OK;
}
int dcp_gpu_test_last_rowsweep_plan(dcp_gpu_ctx *c, unsigned *out, unsigned cap, unsigned *nwords)
{
    if (!c || !nwords) return DCP_EINVAL;
    if (!c->last.scanned || c->last.kernel != 1 || c->last.f64) return c->fail(DCP_EINVAL, "the last scan was no float row sweep");
    *nwords = 2u + DCP_RS_PLAN_WORDS * (unsigned)kNumClasses;
    if (!out || cap < *nwords) return DCP_ENOMEM;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    unsigned redo[DCP_MAX_CLASSES] = {0};
    bool segmented = false;
    for (int k = 0; k < kNumClasses; ++k)
        segmented = segmented || c->last.rs_plan[k].path == DCP_RS_PATH_SEGMENTED;
    if (segmented) HIP_TRY(c, hipMemcpy(redo, c->d_seg_redo_n.p, sizeof redo, hipMemcpyDeviceToHost));
    out[0] = c->last.overlapped ? 1u : 0u;
    out[1] = (unsigned)kNumClasses;
    for (int k = 0; k < kNumClasses; ++k)
    {
        unsigned *w = out + 2u + DCP_RS_PLAN_WORDS * (unsigned)k;
        LastScan::RowsweepClassPlan const &r = c->last.rs_plan[k];
        w[0] = (unsigned)kClasses[k].R, w[1] = (unsigned)kClasses[k].W, w[2] = r.path, w[3] = r.stage, w[4] = r.waves;
        w[5] = r.prefetch, w[6] = r.chunk, w[7] = r.path == DCP_RS_PATH_SEGMENTED ? redo[k] : 0u, w[8] = r.flagged_rest;
    }
    return DCP_OK;
}
int dcp_gpu_test_last_pair_launches(dcp_gpu_ctx *c, unsigned *out, unsigned cap, unsigned *nwords)
{
    if (!c || !nwords) return DCP_EINVAL;
    if (!c->last.scanned) return c->fail(DCP_EINVAL, "no scan yet");
    *nwords = 1u + DCP_PL_WORDS * (unsigned)c->last.pair_launches.size();
    if (!out || cap < *nwords) return DCP_ENOMEM;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    out[0] = (unsigned)c->last.pair_launches.size();
    unsigned *w = out + 1u;
    for (LastScan::PairLaunch const &l : c->last.pair_launches)
    {
        w[0] = l.kind, w[1] = l.precision, w[2] = l.a, w[3] = l.b, w[4] = l.units, w[5] = l.tpb, w[6] = l.cap;
        w += DCP_PL_WORDS;
    }
    return DCP_OK;
}
int dcp_gpu_test_set_seg_col_bytes(dcp_gpu_ctx *c, unsigned long long bytes)
{
    if (!c) return DCP_EINVAL;
    c->seg_col_bytes = bytes ? bytes : (uint64_t)6 << 30;
    return DCP_OK;
}
int dcp_gpu_test_set_ring_stall(dcp_gpu_ctx *c, int on)
{
    if (!c) return DCP_EINVAL;
    c->ring_stall = on ? 1u : 0u;
    return DCP_OK;
}
int dcp_gpu_test_set_trace_mode(dcp_gpu_ctx *c, int own_forward, unsigned long long budget_floats)
{
    if (!c) return DCP_EINVAL;
    c->trace_mode = own_forward ? 1 : 0;
    c->trace_budget = budget_floats;
    return DCP_OK;
}
int dcp_gpu_test_set_posterior_budget(dcp_gpu_ctx *c, unsigned long long bytes)
{
    if (!c) return DCP_EINVAL;
    c->sweeps.post_budget = bytes;
    return DCP_OK;
}

int dcp_gpu_test_envelopes_of_rows(dcp_gpu_ctx *c, uint64_t const *row_off, double const *begin, double const *end,
                                   double const *core, unsigned npairs, double hi, double lo, unsigned min_len,
                                   struct dcp_envelope *out, uint64_t cap, uint64_t *env_off)
{
    if (!c) return DCP_EINVAL;
    if (!env_off || !row_off || (cap && !out) || (npairs && (!begin || !end || !core)) || dcp_env_thresholds_refused(hi, lo))
        return c->fail(DCP_EINVAL, "rows without their arrays or thresholds");
    for (unsigned i = 0; i < npairs; ++i)
        if (row_off[i + 1u] <= row_off[i] || row_off[i + 1u] - row_off[i] > 0xffffffffull)
            return c->fail(DCP_EINVAL, "pair %u has no row 0", i);
    if (npairs == 0)
    {
        env_off[0] = 0u;
        return DCP_OK;
    }
    uint64_t const nrows = row_off[npairs] - row_off[0];
    HIP_TRY(c, hipSetDevice(c->device));
    auto &W = c->sweeps;
    HIP_TRY(c, W.d_rows.reserve(3u * nrows));
    HIP_TRY(c, W.d_off.reserve((size_t)npairs + 1u));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(W.d_off.p, row_off, ((size_t)npairs + 1u) * sizeof(uint64_t), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(W.d_rows.p, begin + row_off[0], nrows * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(W.d_rows.p + nrows, end + row_off[0], nrows * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(W.d_rows.p + 2u * nrows, core + row_off[0], nrows * sizeof(double), hipMemcpyHostToDevice));
    dcp_env_args ea{};
    ea.row_off = W.d_off.p, ea.nlist = npairs;
    ea.begin = W.d_rows.p, ea.end = ea.begin + nrows, ea.core = ea.end + nrows;
    ea.hi = hi, ea.lo = lo, ea.min_len = min_len, ea.pair_base = 0u;
    std::vector<uint32_t> count(npairs, 0u);
    std::vector<dcp_envelope> env;
    float ms = 0.0f;
    if (int rc = envelope_round(c, ea, count.data(), env, &ms)) return rc;
    env_off[0] = 0u; // (only now: an error above leaves every output as it was)
    for (unsigned i = 0; i < npairs; ++i)
        env_off[i + 1u] = env_off[i] + count[i];
    if (env_off[npairs] != env.size()) return c->fail(DCP_EFAIL, "the passes counted %llu envelopes and wrote %llu",
                                                      (unsigned long long)env_off[npairs], (unsigned long long)env.size());
    if (env.size() > cap) return c->fail(DCP_ENOMEM, "the rows have %llu envelopes, the array holds %llu", (unsigned long long)env.size(),
                                         (unsigned long long)cap);
    if (!env.empty()) std::memcpy(out, env.data(), env.size() * sizeof(dcp_envelope));
    return DCP_OK;
}

float dcp_gpu_test_envelope_records_kernel_ms(dcp_gpu_ctx *c) { return c ? c->sweeps.env_own_ms : -1.0f; }

int dcp_gpu_test_set_mea_budget(dcp_gpu_ctx *c, unsigned long long bytes)
{
    if (!c) return DCP_EINVAL;
    c->sweeps.mea_budget = bytes;
    return DCP_OK;
}

int dcp_gpu_test_set_forward_waves(dcp_gpu_ctx *c, unsigned nwaves)
{
    if (!c) return DCP_EINVAL;
    c->sweeps.waves_cap = nwaves;
    return DCP_OK;
}

int dcp_gpu_test_set_forward_scale_band(dcp_gpu_ctx *c, unsigned bits)
{
    if (!c || bits > 500u) return DCP_EINVAL;
    c->sweeps.band = (int)bits;
    return DCP_OK;
}

int dcp_gpu_test_set_dense_round(dcp_gpu_ctx *c, unsigned npairs)
{
    if (!c) return DCP_EINVAL;
    c->sweeps.dense_round = npairs;
    return DCP_OK;
}

int dcp_gpu_test_set_redo_cap(dcp_gpu_ctx *c, unsigned cap)
{
    if (!c) return DCP_EINVAL;
    c->redo_cap_limit = cap ? cap : 1u << 26;
    return DCP_OK;
}
int dcp_gpu_test_fetch_table_span(dcp_gpu_ctx *c, unsigned p, void *out, unsigned long long cap_bytes,
                                  unsigned *span, unsigned *ldk, unsigned *elem_bytes)
{
    if (!c || !span || !ldk || !elem_bytes || p >= c->nprof) return DCP_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    // the span's first value, its width and the row stride, in elements of the DB's precision
    void const *src = nullptr;
    unsigned w = 0, ld = 0, eb = 0;
    if (c->precision == 64)
    {
        for (dcp_f64_prof const &m : c->f64.profs)
            if (m.pidx == p) src = c->f64.d_tab.p + m.tab_off, w = m.ldk, ld = m.ldk, eb = sizeof(double);
    }
    else
    {
        if (int rc = ensure_rowsweep_layout(c)) return rc;
        for (dcp_prof_meta const &m : c->metas)
            if (m.pidx == p) src = c->d_emis_match.p + m.emis_off, w = m.width, ld = m.ldk, eb = sizeof(float);
    }
    if (!src) return DCP_EINVAL;
    *span = w, *ldk = ld, *elem_bytes = eb;
    if (!out) return DCP_OK;
    if (cap_bytes < (unsigned long long)DCP_NCODES * w * eb) return c->fail(DCP_ENOMEM, "span needs more room");
    HIP_TRY(c, hipMemcpy2D(out, (size_t)w * eb, src, (size_t)ld * eb, (size_t)w * eb, DCP_NCODES, hipMemcpyDeviceToHost));
    return DCP_OK;
}
#endif

int dcp_gpu_sync(dcp_gpu_ctx *c)
{
    if (!c) return DCP_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    return finish_scan(c);
}

int dcp_gpu_last_scan_redo_pairs(dcp_gpu_ctx *c, unsigned *npairs)
{
    if (!c || !npairs) return DCP_EINVAL;
    if (!c->last.scanned) return c->fail(DCP_EINVAL, "no scan yet");
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = finish_scan(c)) return rc;
    *npairs = c->last.redo_pairs;
    return DCP_OK;
}

int dcp_gpu_last_scan_query_plan(dcp_gpu_ctx *c, unsigned *nblocks, unsigned long long *sum_block_rows,
                                 unsigned *plane_rows, unsigned *max_groups_per_slot)
{
    if (!c) return DCP_EINVAL;
    if (!c->last.scanned) return c->fail(DCP_EINVAL, "no scan yet");
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = finish_scan(c)) return rc; // an overflowed kernel-4 scan is repeated with the row sweep
    if (!c->last.f64 || c->last.kernel_variant != 4)
        return c->fail(DCP_EINVAL, "the last scan did not run the f64 query-lane kernel (kernel = 4): it has no batch plan");
    if (nblocks) *nblocks = c->f64.plan_blocks;
    if (sum_block_rows) *sum_block_rows = c->f64.plan_sum_rows;
    if (plane_rows) *plane_rows = c->f64.plan_rows;
    if (max_groups_per_slot) *max_groups_per_slot = c->f64.plan_max_groups;
    return DCP_OK;
}

float dcp_gpu_last_scan_ms(dcp_gpu_ctx *c)
{
    if (!c || !c->last.scanned) return -1.0f;
    float ms = -1.0f;
    if (hipEventSynchronize(c->ev_stop) != hipSuccess) return -1.0f;
    if (hipEventElapsedTime(&ms, c->ev_start, c->ev_stop) != hipSuccess) return -1.0f;
    return ms;
}

unsigned dcp_gpu_last_scan_launches(dcp_gpu_ctx const *c) { return c ? c->last.launches : 0; }
int dcp_gpu_last_scan_kernel(dcp_gpu_ctx const *c) { return c && c->last.scanned ? c->last.kernel_variant : 0; }

int dcp_gpu_last_scan_launch_info(dcp_gpu_ctx *c, unsigned i, struct dcp_launch_info *out)
{
    if (!c || !out || !c->last.scanned) return DCP_EINVAL;
    if (i >= c->last.n_launched) return DCP_EINVAL;
    int const k = c->last.launched_class[i];
    // overlapped row-sweep launches all start at ev_start
    hipEvent_t const before = i == 0 || (c->last.kernel == 1 && c->last.overlapped) ? c->ev_start : c->ev_class[i - 1];
    if (hipEventSynchronize(c->ev_class[i]) != hipSuccess) return DCP_EFAIL;
    float ms = 0;
    if (hipEventElapsedTime(&ms, before, c->ev_class[i]) != hipSuccess) return DCP_EFAIL;
    out->ms = ms;
    if (k < 0) // the query-lane launch: every pair of the scan
    {
        out->nodes_per_lane = 4 * c->ql_G; // KT nodes per tile, one query per lane
        out->waves_per_pair = 0;
        out->nprofiles = c->nprof;
        out->cells = dcp_gpu_scan_cells(c);
        out->algorithmic_bytes = dcp_gpu_scan_algorithmic_bytes(c);
        return DCP_OK;
    }
    uint64_t const np = c->class_first[k + 1] - c->class_first[k];
    out->nodes_per_lane = kClasses[k].R;
    out->waves_per_pair = kClasses[k].W;
    out->nprofiles = (unsigned)np;
    out->cells = out->algorithmic_bytes = 0;
    if (c->last.kernel == 2 || c->last.launched_redo[i]) return DCP_OK; // a redo launch: its pairs are counted in the launch before it
    if (c->last.pair_scan) // dcp_gpu_scan_pairs: the class's listed pairs
    {
        out->cells = c->last.pair_class_cells[k];
        out->algorithmic_bytes = c->last.pair_class_bytes[k];
        return DCP_OK;
    }
    uint64_t sumM = 0, len = 0;
    for (unsigned j = c->class_first[k]; j < c->class_first[k + 1]; ++j)
        sumM += c->metas[j].core_size;
    for (unsigned q = c->last.q0; q < c->last.q1; ++q)
        len += c->seq_len[q];
    uint64_t const nq = c->last.q1 - c->last.q0;
    out->cells = sumM * len;
    out->algorithmic_bytes = 20ull * sumM * len + 32ull * (sumM + np) * nq + len * np + 8ull * np * nq;
    return DCP_OK;
}

int dcp_gpu_fetch_scores(dcp_gpu_ctx *c, float *null_out, float *alt_out)
{
    if (!c) return DCP_EINVAL;
    if (c->last.scanned && c->last.f64)
        return c->fail(DCP_EINVAL, "the last scan ran on a double DB: fetch its scores with dcp_gpu_fetch_scores64");
    return fetch_scores(c, c->res, null_out, alt_out);
}

int dcp_gpu_fetch_hits(dcp_gpu_ctx *c, struct dcp_hit *hits, unsigned cap, unsigned *nhits)
{
    if (!c || !nhits) return DCP_EINVAL;
    if (!c->last.scanned) return c->fail(DCP_EINVAL, "no scan to fetch hits from");
    if (c->last.f64)
        return c->fail(DCP_EINVAL, "the last scan ran on a double DB: fetch its hits with dcp_gpu_fetch_hits64");
    return fetch_hits(c, c->res, hits, cap, nhits);
}

int dcp_gpu_fetch_scores64(dcp_gpu_ctx *c, double *null_out, double *alt_out)
{
    if (!c) return DCP_EINVAL;
    if (c->last.scanned && !c->last.f64)
        return c->fail(DCP_EINVAL, "the last scan ran on a float DB: fetch its scores with dcp_gpu_fetch_scores");
    return fetch_scores(c, c->f64.res, null_out, alt_out);
}

// What either fit needs: a scan of the whole batch that kept its dense scores, completed.
static int fit_ready(dcp_gpu_ctx *c)
{
    if (!c->last.scanned) return c->fail(DCP_EINVAL, "no scan yet: the fit is over the last scan's dense scores");
    bool const have = c->last.f64 ? c->f64.res.have_scores : c->res.have_scores;
    if (c->last.pair_scan || !have)
        return c->fail(DCP_EINVAL, "no dense scores kept by the last scan (keep_scores = 0, or a scan of a pair list)");
    if (c->last.q0 != 0 || c->last.q1 != c->nseqs)
        return c->fail(DCP_EINVAL, "the last scan covered sequences [%u, %u) of %u: the fit is over the whole batch", c->last.q0,
                       c->last.q1, c->nseqs);
    if (c->nseqs < 2u) return c->fail(DCP_EINVAL, "a fit needs at least 2 sequences: %u resident", c->nseqs);
    HIP_TRY(c, hipSetDevice(c->device));
    return finish_scan(c); // a query-lane scan completes its redo pairs there
}

// One Gumbel fit per resident profile over the last scan's dense scores (dcp_calib.hip).
int dcp_gpu_fit_gumbel(dcp_gpu_ctx *c, double *mu_out, double *lambda_out, uint8_t *status_out)
{
    if (!c) return DCP_EINVAL;
    if (!mu_out || !lambda_out || !status_out) return c->fail(DCP_EINVAL, "dcp_gpu_fit_gumbel: a null output");
    if (int rc = fit_ready(c)) return rc;
    unsigned const np = c->nprof;
    HIP_TRY(c, c->d_fit.reserve(2u * (size_t)np));
    HIP_TRY(c, c->d_fit_status.reserve(np));
    for (hipEvent_t &e : c->ev_calib)
        if (!e) HIP_TRY(c, hipEventCreate(&e));
    void const *nl = c->last.f64 ? (void const *)c->f64.res.d_null.p : (void const *)c->res.d_null.p;
    void const *al = c->last.f64 ? (void const *)c->f64.res.d_alt.p : (void const *)c->res.d_alt.p;
    HIP_TRY(c, hipEventRecord(c->ev_calib[2], c->stream));
    HIP_TRY(c, (hipError_t)dcp_launch_gumbel_fit(nl, al, c->nseqs, np, c->last.f64 ? 8 : 4, c->d_fit.p, c->d_fit.p + np,
                                                  c->d_fit_status.p, c->stream));
    HIP_TRY(c, hipEventRecord(c->ev_calib[3], c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->calib_timed[1] = true;
    // into buffers of the call's own first: the caller's arrays stay untouched if a copy fails
    std::vector<double> fit(2u * (size_t)np);
    std::vector<uint8_t> st(np);
    HIP_TRY(c, hipMemcpy(fit.data(), c->d_fit.p, fit.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(st.data(), c->d_fit_status.p, np, hipMemcpyDeviceToHost));
    std::memcpy(mu_out, fit.data(), np * sizeof(double));
    std::memcpy(lambda_out, fit.data() + np, np * sizeof(double));
    std::memcpy(status_out, st.data(), np);
    return DCP_OK;
}

// The first two steps of a calibration: the random batch, and its scan with dense scores and no hit records.
static int calibration_scan(dcp_gpu_ctx *c, unsigned nseqs, unsigned len, uint64_t seed, double const probs[4], int multi_hits,
                            int hmmer3_compat, int kernel)
{
    if (int rc = dcp_gpu_seqs_random(c, nseqs, len, seed, probs)) return rc;
    struct dcp_scan_params prm = {};
    prm.multi_hits = multi_hits, prm.hmmer3_compat = hmmer3_compat;
    prm.lrt_threshold = std::numeric_limits<float>::infinity(); // no hit records
    prm.keep_scores = 1, prm.kernel = kernel;
    // a double DB filters by its own threshold: +inf for this scan -- to its end, the re-run of an overflowed
    // query-lane scan included -- then the caller's again
    double const thr64 = c->lrt_threshold64;
    c->lrt_threshold64 = std::numeric_limits<double>::infinity();
    int rc = dcp_gpu_scan(c, &prm);
    if (!rc) rc = dcp_gpu_sync(c);
    c->lrt_threshold64 = thr64;
    return rc;
}

int dcp_gpu_db_calibrate(dcp_gpu_ctx *c, unsigned nseqs, unsigned len, uint64_t seed, double const probs[4], int multi_hits,
                         int hmmer3_compat, int kernel, double *mu_out, double *lambda_out, uint8_t *status_out)
{
    if (!c) return DCP_EINVAL;
    if (int rc = calibration_scan(c, nseqs, len, seed, probs, multi_hits, hmmer3_compat, kernel)) return rc;
    return dcp_gpu_fit_gumbel(c, mu_out, lambda_out, status_out);
}

// The tail fit: the k-th largest score per profile, then the censored fit over the scores from it up (dcp_calib.hip).
int dcp_gpu_fit_gumbel_tail(dcp_gpu_ctx *c, unsigned k, double *mu_out, double *lambda_out, uint8_t *status_out,
                            double *tau_out, uint32_t *k_eff_out)
{
    if (!c) return DCP_EINVAL;
    if (!mu_out || !lambda_out || !status_out || !tau_out || !k_eff_out)
        return c->fail(DCP_EINVAL, "dcp_gpu_fit_gumbel_tail: a null output");
    if (int rc = fit_ready(c)) return rc;
    if (k < 2u || k > c->nseqs)
        return c->fail(DCP_EINVAL, "the tail count k = %u is outside 2 .. %u, the resident sequences", k, c->nseqs);
    unsigned const np = c->nprof;
    HIP_TRY(c, c->d_fit.reserve(2u * (size_t)np));
    HIP_TRY(c, c->d_fit_status.reserve(np));
    HIP_TRY(c, c->d_tail_tau.reserve(np));
    HIP_TRY(c, c->d_tail_keff.reserve(np));
    for (hipEvent_t &e : c->ev_tail)
        if (!e) HIP_TRY(c, hipEventCreate(&e));
    void const *nl = c->last.f64 ? (void const *)c->f64.res.d_null.p : (void const *)c->res.d_null.p;
    void const *al = c->last.f64 ? (void const *)c->f64.res.d_alt.p : (void const *)c->res.d_alt.p;
    int const real_bytes = c->last.f64 ? 8 : 4;
    HIP_TRY(c, hipEventRecord(c->ev_tail[0], c->stream));
    HIP_TRY(c, (hipError_t)dcp_launch_tail_select(nl, al, c->nseqs, np, real_bytes, k, c->d_tail_tau.p, c->d_tail_keff.p,
                                                   c->stream));
    HIP_TRY(c, hipEventRecord(c->ev_tail[1], c->stream));
    HIP_TRY(c, hipEventRecord(c->ev_tail[2], c->stream));
    HIP_TRY(c, (hipError_t)dcp_launch_gumbel_fit_tail(nl, al, c->nseqs, np, real_bytes, c->d_tail_tau.p, c->d_tail_keff.p,
                                                       c->d_fit.p, c->d_fit.p + np, c->d_fit_status.p, c->stream));
    HIP_TRY(c, hipEventRecord(c->ev_tail[3], c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->tail_timed = true;
    // into buffers of the call's own first: the caller's arrays stay untouched if a copy fails
    std::vector<double> fit(3u * (size_t)np);
    std::vector<uint32_t> ke(np);
    std::vector<uint8_t> st(np);
    HIP_TRY(c, hipMemcpy(fit.data(), c->d_fit.p, 2u * (size_t)np * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(fit.data() + 2u * (size_t)np, c->d_tail_tau.p, np * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(ke.data(), c->d_tail_keff.p, np * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(st.data(), c->d_fit_status.p, np, hipMemcpyDeviceToHost));
    std::memcpy(mu_out, fit.data(), np * sizeof(double));
    std::memcpy(lambda_out, fit.data() + np, np * sizeof(double));
    std::memcpy(tau_out, fit.data() + 2u * (size_t)np, np * sizeof(double));
    std::memcpy(k_eff_out, ke.data(), np * sizeof(uint32_t));
    std::memcpy(status_out, st.data(), np);
    return DCP_OK;
}

int dcp_gpu_db_calibrate_tail(dcp_gpu_ctx *c, unsigned nseqs, unsigned len, uint64_t seed, double const probs[4],
                              int multi_hits, int hmmer3_compat, int kernel, unsigned k, double *mu_out, double *lambda_out,
                              uint8_t *status_out, double *tau_out, uint32_t *k_eff_out)
{
    if (!c) return DCP_EINVAL;
    if (!mu_out || !lambda_out || !status_out || !tau_out || !k_eff_out)
        return c->fail(DCP_EINVAL, "dcp_gpu_db_calibrate_tail: a null output");
    if (nseqs != 0 && (k < 2u || k > nseqs)) // before the batch is replaced (nseqs == 0 is the generator's refusal)
        return c->fail(DCP_EINVAL, "the tail count k = %u is outside 2 .. %u, the sequences asked for", k, nseqs);
    if (int rc = calibration_scan(c, nseqs, len, seed, probs, multi_hits, hmmer3_compat, kernel)) return rc;
    return dcp_gpu_fit_gumbel_tail(c, k, mu_out, lambda_out, status_out, tau_out, k_eff_out);
}

// The exponential tail fit: the same selection, then the closed-form fit (dcp_calib.hip), over the last scan's dense
// matrices or the last dense Forward ones.
int dcp_gpu_fit_exp_tail(dcp_gpu_ctx *c, int source, unsigned k, double *mu_out, double *lambda_out, uint8_t *status_out,
                         double *tau_out, uint32_t *k_eff_out)
{
    if (!c) return DCP_EINVAL;
    if (!mu_out || !lambda_out || !status_out || !tau_out || !k_eff_out)
        return c->fail(DCP_EINVAL, "dcp_gpu_fit_exp_tail: a null output");
    void const *nl = nullptr, *al = nullptr;
    int real_bytes = 8;
    if (source == DCP_SCORES_SCAN)
    {
        if (int rc = fit_ready(c)) return rc;
        nl = c->last.f64 ? (void const *)c->f64.res.d_null.p : (void const *)c->res.d_null.p;
        al = c->last.f64 ? (void const *)c->f64.res.d_alt.p : (void const *)c->res.d_alt.p;
        real_bytes = c->last.f64 ? 8 : 4;
    }
    else if (source == DCP_SCORES_FORWARD)
    {
        if (int rc = forward_dense_ready(c)) return rc;
        if (c->nseqs < 2u) return c->fail(DCP_EINVAL, "a fit needs at least 2 sequences: %u resident", c->nseqs);
        HIP_TRY(c, hipSetDevice(c->device));
        nl = c->sweeps.d_dense.p, al = c->sweeps.d_dense.p + (size_t)c->nseqs * c->nprof;
    }
    else return c->fail(DCP_EINVAL, "dcp_gpu_fit_exp_tail: source %d is neither DCP_SCORES_SCAN nor DCP_SCORES_FORWARD", source);
    if (k < 2u || k > c->nseqs)
        return c->fail(DCP_EINVAL, "the tail count k = %u is outside 2 .. %u, the resident sequences", k, c->nseqs);
    unsigned const np = c->nprof;
    HIP_TRY(c, c->d_fit.reserve(2u * (size_t)np));
    HIP_TRY(c, c->d_fit_status.reserve(np));
    HIP_TRY(c, c->d_tail_tau.reserve(np));
    HIP_TRY(c, c->d_tail_keff.reserve(np));
    for (hipEvent_t &e : c->ev_exp)
        if (!e) HIP_TRY(c, hipEventCreate(&e));
    HIP_TRY(c, hipEventRecord(c->ev_exp[0], c->stream));
    HIP_TRY(c, (hipError_t)dcp_launch_tail_select(nl, al, c->nseqs, np, real_bytes, k, c->d_tail_tau.p, c->d_tail_keff.p,
                                                   c->stream));
    HIP_TRY(c, hipEventRecord(c->ev_exp[1], c->stream));
    HIP_TRY(c, hipEventRecord(c->ev_exp[2], c->stream));
    HIP_TRY(c, (hipError_t)dcp_launch_exp_tail_fit(nl, al, c->nseqs, np, real_bytes, c->d_tail_tau.p, c->d_tail_keff.p,
                                                    c->d_fit.p, c->d_fit.p + np, c->d_fit_status.p, c->stream));
    HIP_TRY(c, hipEventRecord(c->ev_exp[3], c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->exp_timed = true;
    // into buffers of the call's own first: the caller's arrays stay untouched if a copy fails
    std::vector<double> fit(3u * (size_t)np);
    std::vector<uint32_t> ke(np);
    std::vector<uint8_t> st(np);
    HIP_TRY(c, hipMemcpy(fit.data(), c->d_fit.p, 2u * (size_t)np * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(fit.data() + 2u * (size_t)np, c->d_tail_tau.p, np * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(ke.data(), c->d_tail_keff.p, np * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(st.data(), c->d_fit_status.p, np, hipMemcpyDeviceToHost));
    std::memcpy(mu_out, fit.data(), np * sizeof(double));
    std::memcpy(lambda_out, fit.data() + np, np * sizeof(double));
    std::memcpy(tau_out, fit.data() + 2u * (size_t)np, np * sizeof(double));
    std::memcpy(k_eff_out, ke.data(), np * sizeof(uint32_t));
    std::memcpy(status_out, st.data(), np);
    return DCP_OK;
}

int dcp_gpu_db_calibrate_forward(dcp_gpu_ctx *c, unsigned nseqs, unsigned len, uint64_t seed, double const probs[4],
                                 int multi_hits, int hmmer3_compat, unsigned k, double *mu_out, double *lambda_out,
                                 uint8_t *status_out, double *tau_out, uint32_t *k_eff_out)
{
    if (!c) return DCP_EINVAL;
    if (!mu_out || !lambda_out || !status_out || !tau_out || !k_eff_out)
        return c->fail(DCP_EINVAL, "dcp_gpu_db_calibrate_forward: a null output");
    if (nseqs != 0 && (k < 2u || k > nseqs)) // before the batch is replaced (nseqs == 0 is the generator's refusal)
        return c->fail(DCP_EINVAL, "the tail count k = %u is outside 2 .. %u, the sequences asked for", k, nseqs);
    if (int rc = dcp_gpu_seqs_random(c, nseqs, len, seed, probs)) return rc;
    if (int rc = dcp_gpu_forward_dense(c, multi_hits, hmmer3_compat)) return rc;
    return dcp_gpu_fit_exp_tail(c, DCP_SCORES_FORWARD, k, mu_out, lambda_out, status_out, tau_out, k_eff_out);
}

float dcp_gpu_exp_tail_kernel_ms(dcp_gpu_ctx *c, int which)
{
    float ms = -1.0f;
    if (!c || which < 0 || which > 1 || !c->exp_timed) return -1.0f;
    if (hipEventElapsedTime(&ms, c->ev_exp[2 * which], c->ev_exp[2 * which + 1]) != hipSuccess) return -1.0f;
    return ms;
}

float dcp_gpu_calib_tail_kernel_ms(dcp_gpu_ctx *c, int which)
{
    float ms = -1.0f;
    if (!c || which < 0 || which > 1 || !c->tail_timed) return -1.0f;
    if (hipEventElapsedTime(&ms, c->ev_tail[2 * which], c->ev_tail[2 * which + 1]) != hipSuccess) return -1.0f;
    return ms;
}

float dcp_gpu_calib_kernel_ms(dcp_gpu_ctx *c, int which)
{
    float ms = -1.0f;
    if (!c || which < 0 || which > 1 || !c->calib_timed[which]) return -1.0f;
    if (hipEventElapsedTime(&ms, c->ev_calib[2 * which], c->ev_calib[2 * which + 1]) != hipSuccess) return -1.0f;
    return ms;
}

int dcp_gpu_fetch_hits64(dcp_gpu_ctx *c, struct dcp_hit64 *hits, unsigned cap, unsigned *nhits)
{
    if (!c || !nhits) return DCP_EINVAL;
    if (!c->last.scanned) return c->fail(DCP_EINVAL, "no scan to fetch hits from");
    if (!c->last.f64)
        return c->fail(DCP_EINVAL, "the last scan ran on a float DB: fetch its hits with dcp_gpu_fetch_hits");
    return fetch_hits(c, c->f64.res, hits, cap, nhits);
}

// ---------------------------------------------------------------------------
// Hits -> alt paths (device traceback)
// ---------------------------------------------------------------------------
int dcp_gpu_trace_paths(dcp_gpu_ctx *c, struct dcp_hit const *hits, unsigned nhits,
                        int multi_hits, int hmmer3_compat, int null_model,
                        struct dcp_step *steps_out, unsigned cap_steps, uint32_t *step_off,
                        float *alt_out)
{
    if (!c || !step_off || (nhits && !hits)) return DCP_EINVAL;
    if (c->nprof == 0 || c->nseqs == 0) return c->fail(DCP_EINVAL, "no DB / sequences resident");
    if (c->precision == 64) return c->fail(DCP_EINVAL, "no traceback on a double DB");
    // step_off[nhits] stays 0 unless the paths are traced: a DCP_ENOMEM of a device allocation then reads as no shortfall
    step_off[0] = step_off[nhits] = 0;
    HIP_TRY(c, hipSetDevice(c->device));
    if (nhits == 0) return DCP_OK;
    if (int rc = check_pairs(c, &hits->seq_idx, &hits->profile_idx, sizeof *hits / sizeof(uint32_t), nhits, true)) return rc;
    if (int rc = check_xtrans_precision(c)) return rc;
    if (int rc = ensure_xtrans(c, multi_hits, hmmer3_compat)) return rc;
    if (int rc = ensure_rowsweep_layout(c)) return rc;

    // Forward pass: the row-sweep kernel of the profile's size class in pair mode, every row's values written to the
    // hit's work area (viterbi_rowsweep_kernel<R, W, 0, false, TRACE>: the scan's own rows, ~0.1 us each); then one
    // wavefront per hit walks back (viterbi_trace_kernel).  Until round 4 the forward pass was that kernel's own
    // one-wavefront loop over rows held in global memory (5-7 us per row: a job of 3 000 sequences of up to 10 kbp spent
    // 5 of its 23 s there, profiles/r04/host_scan_probe.txt); it is kept as the tests' second implementation
    // (trace_mode) and for the null model's one-state path.
    bool const sweep_forward = !null_model && c->trace_mode != 1;
    // per-hit work area and step capacity.  2L + 2M + 16 steps is an estimate, not a bound: a multi-hit path crosses up
    // to M + 1 silent states per domain.
    std::vector<uint64_t> need(nhits);
    std::vector<uint32_t> cap(nhits), wld(nhits);
    std::vector<int> cls(nhits);
    for (unsigned h = 0; h < nhits; ++h)
    {
        unsigned const slot = c->slot_of_pidx[hits[h].profile_idx];
        dcp_prof_meta const &m = c->metas[slot];
        uint64_t const L = c->seq_len[hits[h].seq_idx];
        int const k = cls[h] = range_of(c->class_first, kNumClasses, slot);
        wld[h] = sweep_forward ? 64u * (unsigned)kClasses[k].R * (unsigned)kClasses[k].W : m.width;
        need[h] = 3ull * (L + 1) * wld[h] + 5ull * (L + 1);
        cap[h] = (uint32_t)(2 * L + 2ull * m.core_size + 16);
    }
    uint64_t const budget = c->trace_budget ? c->trace_budget : 1ull << 31; // floats (8 GiB) of work area per round of launches
    DevBuf<uint32_t> d_ld, d_counts; // a round's own buffers: in use until trace_rounds has waited for the stream
    DevBuf<dcp_hit> d_hits;
    DevBuf<dcp_pair> d_pairs;
    auto round = [&](TraceRound<float> const &r) -> int {
        unsigned const n = r.n, *const cfirst = r.first.data();
        std::vector<uint32_t> ld(n);
        std::vector<dcp_hit> shits(n);
        std::vector<dcp_pair> pairs(n);
        for (unsigned i = 0; i < n; ++i)
        {
            unsigned const h = r.ord[i];
            ld[i] = wld[h];
            shits[i] = hits[h];
            pairs[i] = dcp_pair{hits[h].seq_idx, c->slot_of_pidx[hits[h].profile_idx]}; // {q, slot}
        }
        HIP_TRY(c, d_ld.alloc(n));
        HIP_TRY(c, d_hits.alloc(n));
        HIP_TRY(c, hipMemcpy(d_ld.p, ld.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(d_hits.p, shits.data(), n * sizeof(dcp_hit), hipMemcpyHostToDevice));
        if (sweep_forward)
        {
            unsigned counts[kNumClasses];
            for (int k = 0; k < kNumClasses; ++k)
                counts[k] = cfirst[k + 1] - cfirst[k];
            HIP_TRY(c, d_pairs.alloc(n));
            HIP_TRY(c, d_counts.alloc(kNumClasses));
            HIP_TRY(c, hipMemcpy(d_pairs.p, pairs.data(), n * sizeof(dcp_pair), hipMemcpyHostToDevice));
            HIP_TRY(c, hipMemcpy(d_counts.p, counts, sizeof counts, hipMemcpyHostToDevice));
            dcp_scan_args fa = scan_inputs(c, 0, c->nseqs);
            fa.nprof = c->nprof;
            fa.trace_work = r.work;
            // the classes' launches side by side on their own streams, largest profiles first: a class's launch lasts as
            // long as its longest hit and seldom fills the chip (one after the other they took 0.31 of a job's 0.40 s of
            // traceback, profiles/r04/host_scan_probe_mixed_kernel_stats.csv)
            for (int k = 0; k <= kNumClasses; ++k)
                if (!c->ev_trace[k]) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_trace[k], hipEventDisableTiming));
            HIP_TRY(c, hipEventRecord(c->ev_trace[kNumClasses], c->stream));
            for (int k = kNumClasses - 1; k >= 0; --k)
            {
                if (counts[k] == 0u) continue;
                SizeClass const sc = kClasses[k];
                hipStream_t const ls = c->class_stream[k];
                HIP_TRY(c, hipStreamWaitEvent(ls, c->ev_trace[kNumClasses], 0));
                fa.pairs = d_pairs.p + cfirst[k];
                fa.npairs = d_counts.p + k;
                fa.pair_cap = counts[k];
                fa.trace_woff = r.woff.p + cfirst[k];
                fa.trace_alt = r.alt.p + cfirst[k];
                unsigned const tpb = dcp_rowsweep_tasks_per_block(sc.W);
                unsigned const nb = ((counts[k] + tpb - 1u) / tpb + 7u) / 8u * 8u;
                if (dcp_launch_trace_forward(sc.R, sc.W, &fa, nb, ls))
                    return c->fail(DCP_EFAIL, "no traceback kernel for class R=%d W=%d", sc.R, sc.W);
                HIP_TRY(c, hipEventRecord(c->ev_trace[k], ls));
                HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_trace[k], 0));
            }
            HIP_TRY(c, hipGetLastError());
        }
        dcp_trace_args ta{};
        ta.profs = c->d_metas.p;
        ta.slot_of_pidx = c->d_slot_of_pidx.p;
        ta.emis_match = c->d_emis_match.p;
        ta.emis_insert = c->d_emis_insert.p;
        ta.emis_null = c->d_emis_null.p;
        ta.trans8 = c->d_trans8.p;
        ta.seq_words = c->d_seq_words.p;
        ta.seq_woff = c->d_seq_woff.p;
        ta.seq_len = c->d_seq_len.p;
        ta.xtrans = c->d_xtrans.p;
        ta.hits = d_hits.p;
        ta.nhits = n;
        ta.work = r.work;
        ta.work_off = r.woff.p;
        ta.steps = r.steps.p;
        ta.step_off = r.soff.p;
        ta.nsteps = r.nsteps.p;
        ta.alt_out = r.alt.p;
        ta.null_model = null_model ? 1 : 0;
        ta.skip_forward = sweep_forward ? 1 : 0;
        ta.work_ld = d_ld.p;
        dcp_launch_trace(&ta, n, c->stream);
        return DCP_OK;
    };
    return trace_rounds(c, hits, nhits, need, cap, cls, kNumClasses, sweep_forward, budget, "alt", steps_out, cap_steps, step_off,
                        alt_out, round);
}

// The double DB's traceback: dcp_gpu_trace_paths' contract on dcp_hit64 records.  Forward pass: viterbi64_kernel<R,
// TRACE> of each launch group over the round's pair list, every row written to the hit's work area in double
// (3 [L + 1][ldk] matrices + 5 [L + 1] vectors); then one wavefront per hit walks back (trace64_kernel).  The null
// model's one-state path needs no forward launch: the walk's lane 0 runs that recursion in the work area itself.
int dcp_gpu_trace_paths64(dcp_gpu_ctx *c, struct dcp_hit64 const *hits, unsigned nhits,
                          int multi_hits, int hmmer3_compat, int null_model,
                          struct dcp_step *steps_out, unsigned cap_steps, uint32_t *step_off,
                          double *alt_out)
{
    if (!c || !step_off || (nhits && !hits)) return DCP_EINVAL;
    if (c->nprof == 0 || c->nseqs == 0) return c->fail(DCP_EINVAL, "no DB / sequences resident");
    if (c->precision != 64)
        return c->fail(DCP_EINVAL, "dcp_gpu_trace_paths64 traces on a double DB: trace a float DB's hits with dcp_gpu_trace_paths");
    // step_off[nhits] stays 0 unless the paths are traced: a DCP_ENOMEM of a device allocation then reads as no shortfall
    step_off[0] = step_off[nhits] = 0;
    HIP_TRY(c, hipSetDevice(c->device));
    if (nhits == 0) return DCP_OK;
    if (int rc = check_pairs(c, &hits->seq_idx, &hits->profile_idx, sizeof *hits / sizeof(uint32_t), nhits, true)) return rc;
    auto &F = c->f64;
    std::vector<uint32_t> const &slot = F.slot_of_pidx;
    // per-hit work area (doubles) and step capacity: 2L + 2M + 16 is an estimate, not a bound
    std::vector<uint64_t> need(nhits);
    std::vector<uint32_t> cap(nhits);
    std::vector<int> grp(nhits);
    for (unsigned h = 0; h < nhits; ++h)
    {
        dcp_f64_prof const &m = F.profs[slot[hits[h].profile_idx]];
        uint64_t const L = c->seq_len[hits[h].seq_idx];
        grp[h] = range_of(F.group_first, 4, slot[hits[h].profile_idx]);
        need[h] = null_model ? L + 1 : 3ull * (L + 1) * m.ldk + 5ull * (L + 1);
        cap[h] = (uint32_t)(2 * L + 2ull * m.core_size + 16);
    }
    // the budget of dcp_gpu_trace_paths in bytes (its test hook counts 4-byte units); the work area is the same buffer
    uint64_t const budget = (c->trace_budget ? c->trace_budget : 1ull << 31) * sizeof(float) / sizeof(double);
    DevBuf<double> d_xt; // a round's own buffers: in use until trace_rounds has waited for the stream
    DevBuf<dcp_f64_pair> d_pairs;
    auto round = [&](TraceRound<double> const &r) -> int {
        unsigned const n = r.n, *const gfirst = r.first.data();
        std::vector<dcp_f64_pair> pairs(n);
        std::vector<uint32_t> seqs(n);
        uint32_t seg_lmax = 0;
        for (unsigned i = 0; i < n; ++i)
        {
            unsigned const h = r.ord[i];
            seqs[i] = hits[h].seq_idx;
            pairs[i] = dcp_f64_pair{hits[h].seq_idx, slot[hits[h].profile_idx]};
            if (grp[h] == 3) seg_lmax = std::max(seg_lmax, c->seq_len[hits[h].seq_idx]);
        }
        std::vector<double> xt; // protein_profile_setup in double, as scan64 does
        if (int e = fill_xtrans(c, seqs, multi_hits, hmmer3_compat, DCP_F64_XSTRIDE, xt)) return e;
        HIP_TRY(c, d_xt.alloc(xt.size()));
        HIP_TRY(c, d_pairs.alloc(n));
        HIP_TRY(c, hipMemcpy(d_xt.p, xt.data(), xt.size() * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(d_pairs.p, pairs.data(), n * sizeof(dcp_f64_pair), hipMemcpyHostToDevice));
        if (!null_model)
        {
            F64Seg seg;
            if (int e = f64_seg_columns(c, seg_lmax, gfirst[4] - gfirst[3], &seg)) return e;
            dcp_f64_trace_args fa{};
            fa.profs = F.d_profs.p;
            fa.nprof_total = c->nprof;
            fa.tab = F.d_tab.p;
            fa.trans = F.d_trans.p;
            fa.xe = F.d_xe.p;
            fa.seq_words = c->d_seq_words.p;
            fa.seq_woff = c->d_seq_woff.p;
            fa.seq_len = c->d_seq_len.p;
            fa.trace_work = r.work;
            // one launch per non-empty group on the context stream, one wavefront per pair (the segmented group
            // strides over its pairs with one boundary column per wavefront)
            for (int g = 0; g < 4; ++g)
            {
                unsigned const cnt = gfirst[g + 1] - gfirst[g];
                if (cnt == 0) continue;
                fa.pairs = d_pairs.p + gfirst[g];
                fa.npairs = cnt;
                fa.xtrans = d_xt.p + (size_t)gfirst[g] * DCP_F64_XSTRIDE;
                fa.trace_woff = r.woff.p + gfirst[g];
                fa.trace_alt = r.alt.p + gfirst[g];
                if (dcp_f64_launch_trace_forward(kF64R[g], &fa, f64_group_geometry(c, g, cnt, seg, fa), c->stream))
                    return c->fail(DCP_EFAIL, "no f64 traceback kernel for %d nodes per lane", kF64R[g]);
            }
            HIP_TRY(c, hipGetLastError());
        }
        dcp_f64_walk_args wa{};
        wa.profs = F.d_profs.p;
        wa.pairs = d_pairs.p;
        wa.nhits = n;
        wa.tab = F.d_tab.p;
        wa.trans = F.d_trans.p;
        wa.xe = F.d_xe.p;
        wa.seq_words = c->d_seq_words.p;
        wa.seq_woff = c->d_seq_woff.p;
        wa.seq_len = c->d_seq_len.p;
        wa.xtrans = d_xt.p;
        wa.work = r.work;
        wa.work_off = r.woff.p;
        wa.steps = r.steps.p;
        wa.step_off = r.soff.p;
        wa.nsteps = r.nsteps.p;
        wa.alt_out = r.alt.p;
        wa.null_model = null_model ? 1 : 0;
        dcp_f64_launch_walk(&wa, c->stream);
        return DCP_OK;
    };
    return trace_rounds(c, hits, nhits, need, cap, grp, 4, true, budget, null_model ? "null" : "alt", steps_out, cap_steps, step_off,
                        alt_out, round);
}

// ---------------------------------------------------------------------------
// Hit paths -> domains (dcp_domains.hip)
// ---------------------------------------------------------------------------
} // extern "C": one template serves the float and the double call

namespace
{
char const *const kSpecialNames[8] = {"R", "S", "N", "B", "E", "J", "C", "T"};
void step_name(unsigned id, char out[16])
{
    unsigned const kind = id >> 14, x = id & 0x3fffu;
    if (kind == 3u) snprintf(out, 16, "%s", x < 8u ? kSpecialNames[x] : "?");
    else snprintf(out, 16, "%c%u", "MID"[kind], x);
}

template <class Real>
int path_domains(dcp_gpu_ctx *c, uint32_t const *seq_idx, uint32_t const *profile_idx, unsigned npaths,
                 struct dcp_step const *steps, uint32_t const *step_off, int multi_hits, int hmmer3_compat,
                 struct dcp_domain *dom_out, unsigned cap_domains, uint32_t *dom_off, Real *core_out, Real *null_out,
                 Real *total_out)
{
    constexpr bool f64 = std::is_same<Real, double>::value;
    if (!c) return DCP_EINVAL;
    if (c->nprof == 0) return c->fail(DCP_EINVAL, "no profile DB resident: nothing to score the paths on");
    if (c->nseqs == 0) return c->fail(DCP_EINVAL, "no sequences resident: nothing the paths emit");
    if ((c->precision == 64) != f64)
        return c->fail(DCP_EINVAL, f64 ? "dcp_gpu_path_domains64 works on a double DB: the resident DB is float (dcp_gpu_path_domains)"
                                       : "dcp_gpu_path_domains works on a float DB: the resident DB is double (dcp_gpu_path_domains64)");
    if (npaths == 0) return DCP_OK;
    if (!seq_idx || !profile_idx || !step_off || !dom_off) return c->fail(DCP_EINVAL, "null index array");
    if (int rc = check_xtrans_precision(c)) return rc;
    // everything integers decide is checked before anything is launched or written
    uint64_t nemit = 0;
    if (int rc = check_path_steps(c, seq_idx, profile_idx, npaths, steps, step_off, true, &nemit)) return rc;
    std::vector<uint32_t> doff(npaths + 1u, 0u);
    uint64_t ndom = 0;
    for (unsigned h = 0; h < npaths; ++h)
    {
        uint32_t const b = step_off[h], e = step_off[h + 1];
        doff[h] = (uint32_t)ndom;
        if (b == e) return c->fail(DCP_EINVAL, "path %u is empty", h);
        unsigned const R = 3u << 14, S = R | 1u, B = R | 3u, E = R | 4u, T = R | 7u;
        if (steps[b].state_id == R) // a null path: all R
        {
            for (uint32_t i = b; i < e; ++i)
                if (steps[i].state_id != R)
                    return c->fail(DCP_EINVAL, "path %u, step %u: a null path holds R steps only", h, i - b);
            continue;
        }
        if (steps[b].state_id != S) return c->fail(DCP_EINVAL, "path %u: an alt path starts with S (a null path with R)", h);
        if (steps[e - 1u].state_id != T) return c->fail(DCP_EINVAL, "path %u: an alt path ends with T", h);
        bool open = false;
        for (uint32_t i = b; i < e; ++i)
        {
            unsigned const id = steps[i].state_id;
            if (id == R) return c->fail(DCP_EINVAL, "path %u, step %u: R in an alt path", h, i - b);
            if (id == B)
            {
                if (open) return c->fail(DCP_EINVAL, "path %u, step %u: a B before the E of the B before it", h, i - b);
                open = true;
                ++ndom;
            }
            else if (id == E)
            {
                if (!open) return c->fail(DCP_EINVAL, "path %u, step %u: an E without a B", h, i - b);
                open = false;
            }
        }
        if (open) return c->fail(DCP_EINVAL, "path %u: a B without an E", h);
        if (ndom > 0xffffffffull) return c->fail(DCP_EINVAL, "too many domains");
    }
    doff[npaths] = (uint32_t)ndom;
    if (ndom > cap_domains)
    {
        dom_off[npaths] = (uint32_t)ndom; // the need; nothing else is written
        return c->fail(DCP_ENOMEM, "the paths hold %llu domains: the buffers hold %u", (unsigned long long)ndom, cap_domains);
    }
    if (ndom && (!dom_out || !core_out || !null_out)) return c->fail(DCP_EINVAL, "null output");
    uint32_t const first = step_off[0], total = step_off[npaths] - step_off[0];

    HIP_TRY(c, hipSetDevice(c->device));
    std::vector<dcp_dom_path> recs(npaths + 1u);
    std::vector<Real> xt; // a double DB: one row per path
    if (f64)
    {
        std::vector<uint32_t> seqs(seq_idx, seq_idx + npaths);
        if (int rc = fill_xtrans(c, seqs, multi_hits, hmmer3_compat, DCP_F64_XSTRIDE, xt)) return rc;
        for (unsigned h = 0; h < npaths; ++h)
            recs[h] = dcp_dom_path{seq_idx[h], c->f64.slot_of_pidx[profile_idx[h]], step_off[h] - first, doff[h]};
    }
    else
    {
        if (int rc = ensure_xtrans(c, multi_hits, hmmer3_compat)) return rc;
        if (int rc = ensure_rowsweep_layout(c)) return rc;
        for (unsigned h = 0; h < npaths; ++h)
            recs[h] = dcp_dom_path{seq_idx[h], c->slot_of_pidx[profile_idx[h]], step_off[h] - first, doff[h]};
    }
    recs[npaths] = dcp_dom_path{0u, 0u, total, (uint32_t)ndom};

    // sums: [ndom] core, [ndom] null, [npaths] total, then the error word, in 8-byte units
    size_t const nsums = 2u * (size_t)ndom + npaths + 1u;
    HIP_TRY(c, c->d_dom_steps.reserve(total));
    HIP_TRY(c, c->d_dom_paths.reserve(recs.size()));
    HIP_TRY(c, c->d_dom_sums.reserve(nsums));
    HIP_TRY(c, c->d_dom_recs.reserve(12u * (size_t)ndom));
    HIP_TRY(c, c->d_dom_xt.reserve(xt.size())); // a float DB: none
    for (hipEvent_t &e : c->ev_dom)
        if (!e) HIP_TRY(c, hipEventCreate(&e));
    unsigned long long const none = ~0ull;
    unsigned long long *const d_bad = (unsigned long long *)(c->d_dom_sums.p + nsums - 1u);
    HIP_TRY(c, hipMemcpyAsync(c->d_dom_steps.p, steps + first, (size_t)total * sizeof(dcp_step), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_dom_paths.p, recs.data(), recs.size() * sizeof(dcp_dom_path), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_bad, &none, sizeof none, hipMemcpyHostToDevice, c->stream));
    if (f64) HIP_TRY(c, hipMemcpyAsync(c->d_dom_xt.p, xt.data(), xt.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    dcp_domains_args a{};
    a.paths = c->d_dom_paths.p, a.npaths = npaths, a.steps = c->d_dom_steps.p;
    a.words = c->d_seq_words.p, a.woff = c->d_seq_woff.p;
    if (f64)
    {
        a.profs = c->f64.d_profs.p, a.match = c->f64.d_tab.p, a.trans = c->f64.d_trans.p, a.insert = c->f64.d_xe.p;
        a.xtrans = c->d_dom_xt.p, a.xt_per_path = 1;
    }
    else
    {
        a.profs = c->d_metas.p, a.match = c->d_emis_match.p, a.trans = c->d_trans8.p;
        a.insert = c->d_emis_insert.p, a.null_tab = c->d_emis_null.p;
        a.xtrans = c->d_xtrans.p, a.xt_per_path = 0;
    }
    Real *const d_core = (Real *)c->d_dom_sums.p, *const d_null = (Real *)(c->d_dom_sums.p + ndom),
               *const d_total = (Real *)(c->d_dom_sums.p + 2u * (size_t)ndom);
    a.dom_out = c->d_dom_recs.p, a.core_out = d_core, a.null_out = d_null, a.total_out = d_total, a.bad = d_bad;
    HIP_TRY(c, hipEventRecord(c->ev_dom[0], c->stream));
    HIP_TRY(c, (hipError_t)dcp_launch_domains(&a, f64, c->stream));
    HIP_TRY(c, hipEventRecord(c->ev_dom[1], c->stream));
    c->dom_timed = true;
    std::vector<dcp_domain> h_dom(ndom);
    std::vector<Real> h_core(ndom), h_null(ndom), h_total(npaths);
    unsigned long long bad = none;
    if (ndom)
    {
        static_assert(sizeof(dcp_domain) == 48, "a domain record is 12 words");
        HIP_TRY(c, hipMemcpyAsync(h_dom.data(), c->d_dom_recs.p, ndom * sizeof(dcp_domain), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(h_core.data(), d_core, ndom * sizeof(Real), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(h_null.data(), d_null, ndom * sizeof(Real), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipMemcpyAsync(h_total.data(), d_total, npaths * sizeof(Real), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (bad != none)
    {
        unsigned const h = (unsigned)(bad >> 32), i = (unsigned)bad;
        char from[16], to[16];
        step_name(steps[step_off[h] + i - 1u].state_id, from);
        step_name(steps[step_off[h] + i].state_id, to);
        return c->fail(DCP_EINVAL, "path %u, step %u: %s -> %s is no edge of the model graph", h, i, from, to);
    }
    std::memcpy(dom_off, doff.data(), doff.size() * sizeof(uint32_t));
    if (ndom)
    {
        std::memcpy(dom_out, h_dom.data(), ndom * sizeof(dcp_domain));
        std::memcpy(core_out, h_core.data(), ndom * sizeof(Real));
        std::memcpy(null_out, h_null.data(), ndom * sizeof(Real));
    }
    if (total_out) std::memcpy(total_out, h_total.data(), npaths * sizeof(Real));
    return DCP_OK;
}
} // namespace

extern "C" {

int dcp_gpu_path_domains(dcp_gpu_ctx *c, uint32_t const *seq_idx, uint32_t const *profile_idx, unsigned npaths,
                         struct dcp_step const *steps, uint32_t const *step_off, int multi_hits, int hmmer3_compat,
                         struct dcp_domain *dom_out, unsigned cap_domains, uint32_t *dom_off, float *core_out,
                         float *null_out, float *total_out)
{
    return path_domains<float>(c, seq_idx, profile_idx, npaths, steps, step_off, multi_hits, hmmer3_compat, dom_out,
                               cap_domains, dom_off, core_out, null_out, total_out);
}

int dcp_gpu_path_domains64(dcp_gpu_ctx *c, uint32_t const *seq_idx, uint32_t const *profile_idx, unsigned npaths,
                           struct dcp_step const *steps, uint32_t const *step_off, int multi_hits, int hmmer3_compat,
                           struct dcp_domain *dom_out, unsigned cap_domains, uint32_t *dom_off, double *core_out,
                           double *null_out, double *total_out)
{
    return path_domains<double>(c, seq_idx, profile_idx, npaths, steps, step_off, multi_hits, hmmer3_compat, dom_out,
                                cap_domains, dom_off, core_out, null_out, total_out);
}

float dcp_gpu_path_domains_kernel_ms(dcp_gpu_ctx *c)
{
    float ms = 0.0f;
    if (!c || !c->dom_timed || hipEventElapsedTime(&ms, c->ev_dom[0], c->ev_dom[1]) != hipSuccess) return 0.0f;
    return ms;
}

int dcp_gpu_domains_locate(dcp_gpu_ctx *c, uint32_t const *res_idx, struct dcp_domain const *dom, unsigned n,
                           uint32_t *src_out, uint64_t *begin_out, uint64_t *end_out, uint8_t *minus_out)
{
    if (!c) return DCP_EINVAL;
    if (c->nseqs == 0) return c->fail(DCP_EINVAL, "no sequences resident: nothing to locate the domains on");
    if (!c->reg_src.empty()) // a batch of regions: through the region map
    {
        int const rrc = dcp_domains_locate_regions(res_idx, dom, n, c->seq_len.data(), c->nseqs, c->reg_src.data(), c->reg_begin.data(),
                                                   c->reg_minus.data(), src_out, begin_out, end_out, minus_out);
        return rrc ? c->fail(rrc, "a domain lies outside the resident batch (%u regions), or a null pointer", c->nseqs) : DCP_OK;
    }
    bool const cut = c->win_window != 0;
    int const rc = dcp_domains_locate(res_idx, dom, n, c->seq_len.data(), c->nseqs / c->strands, c->strands,
                                      cut ? c->win_src.data() : nullptr, cut ? c->win_off.data() : nullptr, src_out,
                                      begin_out, end_out, minus_out);
    return rc ? c->fail(rc, "a domain lies outside the resident batch (%u sequences), or a null pointer", c->nseqs) : DCP_OK;
}

static void last_range(dcp_gpu_ctx const *c, uint64_t *sumM, uint64_t *len, uint64_t *nq)
{
    *sumM = *len = 0;
    for (unsigned m : c->core_sizes)
        *sumM += m;
    unsigned q0 = c->last.scanned ? c->last.q0 : 0, q1 = c->last.scanned ? c->last.q1 : c->nseqs;
    for (unsigned q = q0; q < q1; ++q)
        *len += c->seq_len[q];
    *nq = q1 - q0;
}

uint64_t dcp_gpu_scan_cells(dcp_gpu_ctx const *c)
{
    if (!c) return 0;
    if (c->last.scanned && c->last.pair_scan) return c->last.pair_cells; // dcp_gpu_scan_pairs: the listed pairs
    uint64_t sumM, len, nq;
    last_range(c, &sumM, &len, &nq);
    return sumM * len;
}

uint64_t dcp_gpu_scan_algorithmic_bytes(dcp_gpu_ctx const *c)
{
    // per pair 20*M*L + 32*(M+1) + L + 8
    if (!c) return 0;
    if (c->last.scanned && c->last.pair_scan) return c->last.pair_bytes;
    uint64_t sumM, len, Q, P = c->core_sizes.size();
    last_range(c, &sumM, &len, &Q);
    return 20ull * sumM * len + 32ull * (sumM + P) * Q + len * P + 8ull * P * Q;
}

} // extern "C"
