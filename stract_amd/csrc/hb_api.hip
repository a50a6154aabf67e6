// hb_api.hip - C ABI (include/hyperball.h) + pass driver of the HyperBall library.
//
// Replaces HarmonicCentrality::calculate / calculate_centrality
// (crates/core/src/webgraph/centrality/harmonic.rs:215-287,292) behind a C boundary.
// Host orchestration only: every arithmetic step of the path runs in the gfx950 kernels
// of hb_kernels.hip.h.  There is no CPU fallback.
#include "hb_guard_alloc.h" // FIRST: no-op unless built with -DHB_GUARD_ALLOC=<mode> (debug allocators: guard pages / poison / red zones)
#include "hb_pool.h"        // then: every hipMalloc / hipFree below goes through the caching device allocator (shipped build)
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "hb_owned.h" // (after hb_pool.h: DevPtr frees through the allocator this file sees)
#include "hb_internal.h"
#include "hb_experiments.h" // HB_XBITS: the switches of the experiments build (none in the product library)
#include "hb_kernels.hip.h"
#include "hb_walk.hip.h"
#include "hb_sample.hip.h"
#include "hb_bfs.hip.h"
#include "hb_betweenness.hip.h"
#include "hb_similarity.hip.h"
#include "hb_nearest_seed.hip.h"
#include "hb_links.hip.h"
#include "hb_similar.hip.h"
#include "hb_similarity_limit.hip.h"
#include "hb_score.hip.h"
#ifdef HB_EXPERIMENTS
#include "hb_experiments.hip.h"
#endif
#include "hll64_tables.inc"

using namespace hb;

namespace {
thread_local std::string g_create_error;

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
};

// DevPtr<T> (hb_owned.h) is the one owner of a hipMalloc'ed buffer that is not on a context's `allocs` list (dev_alloc below): scratch of
// a single call, the input CSR of a load, the sampled operator's state.

// DeviceCsr (hb_internal.h: a plain struct, the host-only sources include it too) with an owner: the device ingest or hb_load_dense fills
// `d`, plan_and_upload takes the whole thing by move and frees it when the plan exists
struct OwnedCsr {
    DeviceCsr d;
    OwnedCsr() = default;
    OwnedCsr(OwnedCsr &&o) noexcept : d(o.d) { o.d = DeviceCsr{}; }
    OwnedCsr(const OwnedCsr &) = delete;
    OwnedCsr &operator=(const OwnedCsr &) = delete;
    ~OwnedCsr() { reset(); }
    void reset()
    {
        for (void *q : {(void *)d.d_row_ptr, (void *)d.d_src, (void *)d.d_id_lo})
            if (q) (void)hipFree(q);
        d = DeviceCsr{};
    }
};
} // namespace

// The tail end of a node-valued operator (hb_distances, hb_betweenness, hb_nearest_seed): one value per node in sid order, and the
// compacted list of the sids that have one, which is all that hb_*_copy downloads.  Allocated, compacted and read by node_result_*
// (hb_api_walk.inc).  T = uint8_t (distances): the values ARE the select's flag bytes and its byte output ARE the selected values, so
// d_flag_sid / d_sel_val alias d_val_sid / d_sel_flag - no second value buffer, no gather
template <class T>
struct NodeResult {
    static constexpr bool kBytes = std::is_same<T, uint8_t>::value;
    bool valid = false;            // the buffers hold the result of a finished call (an empty graph: no buffers, count == 0)
    bool compacted = false;        // d_sel_* and d_val_sid describe that result (distances: made by the first reader that needs them)
    T *d_val_sid = nullptr;        // n: value per sid
    uint8_t *d_flag_sid = nullptr; // n: 255 = no value (the select's input)
    uint32_t *d_sel_sid = nullptr; // n: the sids that have a value, ascending
    uint8_t *d_sel_flag = nullptr; // n: the select's byte output
    T *d_sel_val = nullptr;        // n: their values
    uint64_t *d_sel_cnt = nullptr; // the select's count word
    uint64_t count = 0;            // entries of the compacted list
    void reset() // a new call begins: nothing to read until it has finished
    {
        valid = compacted = false;
        count = 0;
    }
};

// ---- graph lifetime ---------------------------------------------------------------------------------------------------------------
// What describes the loaded graph on the device: written by plan_and_upload (and, on first use after a load, by the operators), gone
// with the graph.  free_graph_buffers() frees what owns memory here and then assigns a default-constructed state: a member added to
// this struct cannot survive a reload.  The d_* pointers are carved from hb_ctx::allocs (dev_alloc) unless they say otherwise.
struct GraphDeviceState {
    uint64_t *d_row_ptr = nullptr;
    uint32_t *d_src = nullptr;
    uint16_t *d_src_jp = nullptr; // parallel to d_src: the sources' initial register (pass 0 streams it, hb_kernels.hip.h)
    bool level0_all_real = false;    // no row of the first hub-chunk level reads virtual rows (checked at load): pass 0 may run init_level1_kernel there
    uint32_t *d_virt_rows = nullptr; // one bit per work row: its sources are virtual rows (pass 0, PassParams::virt_rows)
    uint16_t *d_self_jp = nullptr; // per node row: its OWN initial register in the same format (the lean pass 0 reads it instead of the counters)
    uint32_t *d_sat = nullptr;     // saturated rows (PassParams::sat): one bit per work row, cleared by hb_begin.  NULL: the context is outside the gate
    uint32_t *d_sat_u = nullptr;   // U of the saturation bound, one word per register (sat_bound_kernel at load)
    // early exit: the dense passes of this run that follow enough saturation leave a row's gather loop once its
    // accumulator has reached U (the EARLY instances of pass_kernel)
    unsigned long long *d_early = nullptr; // kStripes words: rows of the last EARLY pass that left their loop early (allocated with d_sat)
    uint64_t sat_out_sum = 0;      // out-degree sum of the rows saturated so far in this run (word 1 of the dense passes' counters)
    bool early_now = false;        // the dense pass being launched runs the EARLY instances
    bool last_dense_early = false; // ... and so did the last dense pass that was launched (hb_debug_saturation)
    uint4 *d_regs[2] = {nullptr, nullptr};
    uint4 *d_part = nullptr;
    uint32_t *d_bits[2] = {nullptr, nullptr};
    uint32_t *d_kdirty = nullptr;
    double *d_ksum = nullptr, *d_kerr = nullptr;
    uint64_t *d_size = nullptr;
    uint64_t *d_idlow = nullptr;
    uint32_t *d_dev_of = nullptr;
    uint32_t *d_sid_of = nullptr; // device row -> sid, kNone for padding rows
    uint32_t *d_outdeg = nullptr; // device row -> (global) out-degree
    unsigned long long *d_counters = nullptr; // (max_passes + 1) * kCounterWords, striped (hb_kernels.hip.h)
    double *d_raw = nullptr, *d_bias = nullptr;
    uint8_t *d_lc = nullptr;
    // sparse (data-driven) tail passes: transposed work-row graph + worklists.  The transpose (row -> readers) is also what hb_distances
    // and hb_betweenness walk: a context without sweep support gets it at their first call (ensure_transpose, hb_api_walk.inc) -
    // sparse_ok, not a non-null d_out_ptr, says that the sweep support exists
    uint64_t *d_out_ptr = nullptr;
    uint32_t *d_out_rows = nullptr;
    uint32_t *d_touch = nullptr;
    uint32_t *d_seeds = nullptr, *d_heavy = nullptr;
    unsigned int *d_sparse_counts = nullptr;
    bool sparse_ok = false;
    // changed-only exchange (HB_FLAG_CHANGED_ONLY): packed changed counters, popcounts / prefix of the bitmap words
    uint4 *d_pack = nullptr;
    uint32_t *d_wpop = nullptr;
    uint64_t *d_wprefix = nullptr;
    // edge partition + HB_FLAG_CHANGED_ONLY: rows the local merge changed, the ranks' bitmaps gathered, their union
    uint32_t *d_lbits = nullptr, *d_lbits_all = nullptr, *d_ubits = nullptr;
    bool ubits_valid = false; // d_ubits holds this pass' union (set by the exchange, consumed by the epilogue)
    unsigned long long *d_rank_cnt = nullptr; // world words: every rank's changed rows of this pass (summed over the ranks)
    // HB_FLAG_PACKED_WIRE: 48-byte rows, world x slice_rows of them each - [0] the packed rows / gathered slices, [1] the pieces an
    // all-to-all delivered (edge partition only); allocated by the first pass that exchanges (ensure_wire6_buffers)
    uint32_t *d_w6[2] = {nullptr, nullptr};
    // the far tail as one workgroup (hb_tail.hip.h): work lists, their counts / status words, and whether the lists describe the
    // bitmaps as they are now (any pass run by other kernels invalidates them: the next entry collects them again)
    uint32_t *d_tl_changed[2] = {nullptr, nullptr}, *d_tl_vchanged[2] = {nullptr, nullptr}, *d_tl_dirty[2] = {nullptr, nullptr};
    uint32_t *d_tl_work = nullptr, *d_tl_count = nullptr;
    bool tl_valid = false;
    // reference-tail mode (HB_FLAG_REFERENCE_TAIL): the reference's changed-node machinery as written
    uint64_t *d_tail_ptr = nullptr; // page-level records by source device row (hb_load_tail_edges), n_pad + 1
    uint32_t *d_tail_to = nullptr;
    uint64_t tail_count = 0;
    std::vector<uint64_t> tail_keys; // records of the closed segments, mapped (hb_host.cpp tail_close_segment)
    std::vector<TailDoc> tail_open;  // documents of the segment being appended (hb_tail_segment_end closes it)
    bool tail_dirty = false;         // tail_keys differ from what d_tail_* hold: rebuilt by hb_begin
    TailIndex *tail_index = nullptr; // id -> sid index for the batches of tail records (built at the first batch); tail_index_free
    uint32_t *d_bloom = nullptr;    // new_changed_nodes of the last pass (U64BloomFilter), bloom_bits bits
    unsigned long long *d_bloom_ones = nullptr; // [0] count_ones, [1] (low word) length of d_list
    uint32_t *d_list = nullptr;     // exact_changed_nodes as device rows, <= ref_threshold entries
    // results: one f64 per node in ascending-NodeID order, -1.0 = absent (centrality <= 0)
    double *d_out = nullptr;
    double *h_out = nullptr; // pinned (hipHostFree), n entries
    uint64_t h_out_len = 0;
    // [r6] the image's layout: out_len live entries.  Identity (out_len = n, index = sid, d_cid_of = d_sid_of) or, when the results travel in
    // stages (rs.on: single rank), COMPACT: one entry per node with in-edges, ascending NodeID (hb_aux.hip.h "the compact result image");
    // h_in_bits = those nodes as a bitmap over the sids (empty = identity)
    uint64_t out_len = 0;
    uint32_t *d_cid_of = nullptr; // n_pad: device row -> index into out[] (kNone = not in the image)
    std::vector<uint64_t> h_in_bits;
    // results that travel while the passes still run (results_stage; hb_aux.hip.h results_sync_kernel).  The side stream and its two events
    // are the context's (hb_ctx::rs_stream)
    struct ResultSync {
        bool on = false;          // this graph ships its results in stages (single rank, large enough or forced by HB_X_SNAPSHOT_EVERY_PASS)
        bool valid = false;       // d_out / d_sent (and h_out, once `copied` has fired) hold one consistent snapshot of the sums
        uint64_t changed_since = 0; // (run) counters changed since that snapshot (= sums that moved, give or take a `+= 0.0` flush)
        uint32_t stages = 0;      // (run) snapshots shipped during the current run
        double *d_sent = nullptr; // device order: the sum out[] was last built from
        uint32_t *d_sid = nullptr; // the final list: (sid, value) of what moved after the last snapshot
        double *d_val = nullptr;
        unsigned long long *d_count = nullptr;
        unsigned long long *d_kept = nullptr; // kCounterWords scratch words of the snapshots' kernel (side stream)
        uint32_t *h_sid = nullptr; // pinned (hipHostFree)
        double *h_val = nullptr;
        unsigned long long *h_count = nullptr;
        uint64_t cap = 0;
    } rs;
    // hb_sampled_harmonic (hb_api_sample.inc): per-level histograms and scratch, allocated on first use.  The holders own them: they are
    // not on the `allocs` list and hb_stats.device_bytes does not count them
    struct SampleState {
        DevPtr<uint16_t> d_hist;              // levels x n_pad, level-major: c_d of device row r at [(d - 1) n_pad + r]
        uint32_t levels = 0;                  // D of d_hist (0 = no sampled result)
        DevPtr<unsigned long long> d_cnt;     // (kMaxLevels + 1) x 4 counters of the current batch
        DevPtr<uint32_t> d_srcs;              // sids of a batch's sources (<= 512)
        DevPtr<uint32_t> d_rows;              // ... their device rows
        DevPtr<double> d_w;                   // w_d as f64, kMaxLevels entries
        std::vector<uint32_t> cand;           // the sampler's candidates (sids with an out-edge), ascending
        bool cand_valid = false;              // cand describes the loaded graph (built by the first sampler call after a load)
    } smp;
    // hb_distances (hb_api_distance.inc): the BFS state and the last result, dev_alloc'ed at the first call after a load
    struct DistanceState {
        bool ready = false;     // the buffers below exist
        uint8_t *d_dist = nullptr;                                       // n_pad: distance per device row, 255 = unreached
        uint32_t *d_vis = nullptr, *d_front = nullptr, *d_next = nullptr; // one bit per row (hb_bfs.hip.h)
        uint32_t *d_heavy = nullptr;
        uint32_t heavy_cap = 0;
        unsigned int *d_heavy_cnt = nullptr;
        unsigned long long *d_cnt = nullptr; // 256 levels x 4 counters
        uint32_t *d_indeg = nullptr;         // rows_total: node sources under every row (reversed switch rule), built at the first reversed call
        bool indeg_valid = false;
        uint64_t words_total = 0;            // words of d_vis / d_next
        NodeResult<uint8_t> res;             // distance per sid and the reached sids; count = reached, known before the lazy compaction
    } dst;
    // hb_betweenness (hb_api_betweenness.inc): the per-batch state, the sums and the last result, dev_alloc'ed at the first call after a load
    struct BetweennessState {
        bool ready = false; // the buffers below exist
        uint8_t *d_dist = nullptr;             // n_pad x 8: distance per device row and lane of the current batch, 255 = unreached
        unsigned long long *d_sigma = nullptr; // n_pad x 8: shortest-path counts
        double *d_delta = nullptr;             // n_pad x 8: dependencies
        uint8_t *d_reached = nullptr;          // n_pad: the row is a result
        double *d_sum = nullptr;               // n_pad: sum(v) over the batches so far
        unsigned long long *d_cnt = nullptr;   // 257 levels x 4 counters of the current batch
        uint32_t *d_srcs = nullptr;            // sids of a batch's sources (<= 8)
        uint32_t *d_heavy = nullptr;           // backward: node rows whose reader list the grid sums
        unsigned int *d_heavy_cnt = nullptr;
        uint32_t heavy_cap = 0;                // such rows in the loaded graph (0 = none: no list, no launches)
        hbk::bc_d2 *d_seg = nullptr;           // ... their per-segment partial sums
        NodeResult<double> res;                // value per sid, -1.0 = no result; flag 0 = result
        uint64_t bytes = 0;                    // device bytes of the above
        uint32_t last_lanes = 0;               // sources of the last batch run (0 = none)
    } btw;
    // hb_inbound_similarity (hb_api_similarity.inc): the per-graph state (position bytes, blooms; the in-degrees are dst.d_indeg), the
    // sums and the last result, dev_alloc'ed at the first call after a load
    struct SimilarityState {
        bool ready = false;      // the buffers below exist and the per-graph state is built
        bool valid = false;      // they hold the result of a finished hb_inbound_similarity (its last batch's counts lie in d_regs[1] / d_bits[1]
                                 // while rows == RowsOf::Similarity)
        uint8_t *d_pos = nullptr;              // n_pad: h & 63 of the row's low id word
        uint64_t *d_bloom = nullptr;           // rows_total: OR of 1 << pos over the in-list (chunk rows: their partial)
        uint32_t *d_vmask = nullptr;           // nv: seed: the anchor slots whose in-list runs through the chunk row
        double *d_acc = nullptr;               // n_pad x 2: sum of the liked / disliked terms so far
        uint32_t *d_anchor_rows = nullptr;     // 16: device rows of the batch's anchors, kNone = no node
        uint32_t *d_anchor_sids = nullptr;     // 16: ... their sids, kNone = no node
        unsigned long long *d_cnt = nullptr;   // 2 x 4 counters: the seed's, the count level's
        double *d_score = nullptr;             // n: score per sid
        uint8_t *d_anchor = nullptr;           // n: 1 = the sid is a liked / disliked host
        uint64_t *d_key = nullptr;             // n: hb_similarity_top's sort keys
        uint8_t *d_keep = nullptr;             // n: ... and which sids take part
        std::vector<hb_u128> liked, disliked;  // the entries of the last call (hb_similarity_lookup of ids that are no node)
        bool normalized = false;
        double self_score = 1.0;
        uint32_t last_slots = 0;               // slots of the last batch
        uint32_t limit = 0;                    // hb_similarity_options.limit of the last call (0 = whole in-lists)
        uint64_t bytes = 0;                    // device bytes of the above (and of dst.d_indeg when this operator built it)
    } sim;
    // hb_nearest_seed (hb_api_nearest_seed.inc): the candidates, the seeds, the double-buffered values and the last result, dev_alloc'ed at
    // the first call after a load.  The operator borrows nothing of the HyperBall state
    struct NearestSeedState {
        bool ready = false; // the buffers below exist
        uint4 *d_cand = nullptr;                 // n_pad: {key, sid} of the row's node, {~0, kNone} for padding rows
        uint4 *d_part = nullptr;                 // nv x 2: the two best distinct candidates under a chunk row
        uint32_t *d_seed_row = nullptr;          // n_pad: device row of the seed, kNone = none
        double *d_val[2] = {nullptr, nullptr};   // n_pad: the value after the previous / this round
        uint8_t *d_has[2] = {nullptr, nullptr};  // n_pad: ... and whether there is one
        unsigned long long *d_up_key = nullptr;  // n: the caller's keys by sid, ~0 = not listed
        double *d_up_val = nullptr;              // n: the caller's original values by sid
        uint8_t *d_up_has = nullptr;             // n: ... and which sids have one
        unsigned long long *d_cnt = nullptr;     // kCounterWords striped words of a round + 4 plain counters
        NodeResult<double> res;                  // value per sid, -1.0 = no result; flag 0 = result
        uint32_t *d_seed_sid = nullptr;          // n: the seed of every sid as a sid, kNone = none
        uint64_t *d_top_key = nullptr;           // n: hb_nearest_seed_top's sort keys, reversed sid order
        uint8_t *d_top_keep = nullptr;           // n: ... and which entries are results
        uint64_t bytes = 0;                      // device bytes of the above
    } nst;
    // hb_links_set_keys / hb_backlinks / hb_forwardlinks (hb_api_links.inc): the key set and its dense order, the buffers of a batch and the last result.
    // The holders own them (they grow with the limit, the slots of a batch and the queries of a call): freed by the next load, counted in
    // `bytes` and in hb_stats.device_bytes.  Here and in the three states below a holder is a GrowPtr, which knows how many entries it
    // has, and hold() is the one place that allocates and books it.  The operator borrows nothing of the HyperBall state
    struct LinksState {
        bool ready = false; // key / ord / inv / ord_row exist and describe the current key set (none: NodeID order)
        bool valid = false; // the result below is that of a finished hb_backlinks / hb_forwardlinks
        GrowPtr<unsigned long long> d_key; // n: key by sid, ~0 = not listed
        GrowPtr<uint32_t> d_ord;           // n: position of the sid in the sort by (key, sid)
        GrowPtr<uint32_t> d_inv;           // n: the sid at a position
        GrowPtr<uint32_t> d_ord_row;       // n_pad: ord by device row, kNone for padding rows
        GrowPtr<uint2> d_items;            // slots + nv + 16: (slot, row) of a batch, level by level
        GrowPtr<uint32_t> d_ctl;           // 5 x slots (deg, sel_k, sel_prefix, thr, cursor) + 64 level counts + 8 flag words (+ forward: slots lengths, slots + 1 segment offsets)
        GrowPtr<uint32_t> d_hist;          // slots x 256
        GrowPtr<uint32_t> d_out;           // slots x limit: the kept ords of a batch
        GrowPtr<uint32_t> d_slot_row;      // distinct: device row of every distinct queried node (ascending sid)
        GrowPtr<uint32_t> d_slot_self;     // distinct: the row its list must not hold (kNone: HB_LINKS_KEEP_SELF)
        GrowPtr<uint32_t> d_res_sid;       // distinct x limit: the lists as sids
        GrowPtr<unsigned long long> d_res_key; // distinct x limit: ... and their keys
        GrowPtr<uint32_t> d_top_row;       // nv: hb_forwardlinks: the node row at the top of every chunk row's tree (kNone: a padding row)
        bool top_ready = false;            // d_top_row describes the loaded graph (built by the first hb_forwardlinks after a load)
        uint32_t limit = 0;                // of the result
        std::vector<uint32_t> query_slot; // per query of the last call: its distinct node, kNone = no node of the graph
        std::vector<uint32_t> degree;     // per distinct node: degree(v)
        uint64_t entries = 0;             // entries of all lists of the result
        uint64_t bytes = 0;               // device bytes of the above
    } lnk;
    // hb_similar_hosts (hb_api_similar.inc): its four sets of lists, the counters and the last result.  The holders own them (they grow
    // with the liked hosts and the co-citation sources of a call): freed by the next load, counted in `bytes` and in
    // hb_stats.device_bytes.  The operator borrows nothing and leaves the links result as it is; the buffers of a batch of the list
    // builder are the links state's
    struct SimilarHostsState {
        bool valid = false; // the result below is that of a finished hb_similar_hosts
        GrowPtr<uint32_t> d_in, d_in_len;         // liked x 512: In512 of the distinct liked hosts (sorted by sid once scored), their degrees
        GrowPtr<unsigned long long> d_in_mask;    // liked: their bloom masks
        GrowPtr<uint32_t> d_src;                  // liked x 128: B, the distinct sources of the 128-prefixes
        GrowPtr<uint32_t> d_fw, d_fw_len;         // nb x 512: their forward lists, the degrees
        GrowPtr<uint32_t> d_count;                // n: the flag words of B, then count[v]
        GrowPtr<uint32_t> d_touched;              // min(n, nb x 512): the distinct targets
        GrowPtr<uint32_t> d_cand, d_cand_count;   // 1024: the pre-selection and its counts
        GrowPtr<uint32_t> d_cin, d_cin_len;       // 1024 x 512: In512 of the candidates
        GrowPtr<unsigned long long> d_cin_mask;   // 1024
        GrowPtr<unsigned long long> d_keys;       // the lists' keys (the list builder writes them; nobody reads them here)
        GrowPtr<uint32_t> d_liked, d_anchor;      // liked: the distinct liked sids ascending; N: the entries in caller order as slots
        GrowPtr<double> d_score, d_top_score;     // 1024
        GrowPtr<uint32_t> d_top_sid;              // 1024
        GrowPtr<unsigned long long> d_cnt;        // 8 words: cursors (as u32) and the pair counters
        std::vector<uint32_t> cand_sid, cand_count, top_sid; // the result on the host: at most 1024 entries each
        std::vector<double> top_score;
        uint64_t bytes = 0;
    } shs;
    // hb_inbound_similarity with a limit (hb_api_similarity.inc, hb_similarity_limit.hip.h): the cut lists of the LISTED rows - degree > limit,
    // or a self link - for one graph, one key set and one limit.  Built at the first limited call, kept while the three stay the same:
    // dropped by hb_links_set_keys, by a call with another limit (similarity_limit_drop) and by the next load.  The holders own them,
    // counted in `bytes` and in hb_stats.device_bytes.  The state borrows nothing
    struct SimilarityLimitState {
        bool ready = false;               // the buffers below describe the loaded graph under the current key set and `limit`
        uint32_t limit = 0;
        uint64_t listed = 0, entries = 0; // listed rows, the entries of their lists
        GrowPtr<uint32_t> d_idx;           // n_pad: the list index of a node row, kNone = not listed (the plan's list is its cut)
        GrowPtr<uint32_t> d_list_row;      // listed: the device row of list k
        GrowPtr<uint32_t> d_lists;         // listed x limit: list k at k x limit, device rows in the order (key, NodeID)
        GrowPtr<uint32_t> d_len;           // listed: min(degree, limit)
        GrowPtr<uint64_t> d_bloom;         // listed: the bloom mask over the list's entries
        GrowPtr<uint32_t> d_seed_rows;     // 16: the batch's anchors that seed from the plan's lists
        GrowPtr<unsigned long long> d_cnt; // 4 counters of the list-count kernel
        uint64_t bytes = 0;
    } lim;
    // hb_score_hosts (hb_api_score.inc): the BitVecs of the distinct known hosts of a call, the entries of its requests, one piece of
    // the pair space and the last result.  The holders own them (they grow with the hosts and entries of a call and with the limit):
    // freed by the next load, counted in `bytes` and in hb_stats.device_bytes.  The operator borrows nothing; the buffers of a batch of
    // the list builder are the links state's
    struct ScoreState {
        bool valid = false; // the result below is that of a finished hb_score_hosts
        GrowPtr<uint32_t> d_lists, d_len;          // distinct x limit: the backlinks of the distinct known hosts (sorted by sid), their degrees
        GrowPtr<unsigned long long> d_mask;        // distinct: their bloom masks
        GrowPtr<unsigned long long> d_keys;        // the lists' keys of one call of the list builder (nobody reads them here)
        GrowPtr<uint32_t> d_node_idx, d_anchor_idx; // the nodes / the anchors of all requests as indices of the call's distinct ids
        GrowPtr<hbk::ScRequest> d_req;
        GrowPtr<hbk::ScRect> d_rect;               // the rectangles of one piece
        GrowPtr<uint32_t> d_pair;                  // the pair words of one piece
        GrowPtr<double> d_acc, d_score;            // nodes x 2: the running sums; nodes: the scores
        GrowPtr<unsigned long long> d_cnt;         // the four pair counters
        std::vector<uint64_t> offsets;            // the result on the host: requests + 1 offsets into scores
        std::vector<double> scores;
        uint64_t bytes = 0;
    } sco;
};

// The timing events of a pass (one set: hb_ctx::ev, or an EvSet), in the order a pass records them; kEvLevel1 lies between kEvStart and
// kEvLevels.
enum PassEvent {
    kEvStart,      // the pass begins
    kEvLevels,     // the virtual levels (hub chunks) are done
    kEvEnd = kEvLevels, // what is no HyperBall pass (load warm-up, sampled walks, distances, the tail kernel) times itself from kEvStart to here
    kEvMerge,      // the node rows' local merge is done
    kEvCollective, // the exchange with the other ranks is done
    kEvEpilogue,   // the unfused epilogue is done
    kEvLevel1,     // the first hub-chunk level is done (sweep passes: seed collection + expansion)
    kEvSlots
};

enum class RowsOf : uint8_t { Nobody, HyperBall, Sampled, Brandes, Similarity }; // hb_ctx::rows
enum class Image : uint8_t { None, HyperBall, Sampled };                        // hb_ctx::image

struct hb_ctx : GraphDeviceState {
    // ---- context lifetime: hb_create .. hb_destroy ------------------------------------------------------------------------------------
    hb_options opt{};
    int device = 0;
    int num_cu = 256;
    hipStream_t stream = nullptr;
    ncclComm_t comm = nullptr;
    hb_collectives coll{}; // hb_set_collectives: the per-pass exchanges go through these instead of RCCL (HB_FLAG_NO_RCCL contexts)
    int (*coll_a2a)(void *user, const void *send, void *recv, uint64_t bytes_per_rank, void *stream) = nullptr; // hb_set_all_to_all
    std::string err;
    std::string arch;
    uint64_t lim_records = 0, lim_bytes = 0, lim_chunk = 0; // hb_debug_set_ingest_limits (0 = no limit / default)
    uint32_t max_passes = 4096;
    void *h_block = nullptr;                  // ONE page-locked block, allocated by hb_create, that h_counters / h_slot / h_tl_count / h_rank_cnt are
                                              // carved from: no hipHostMalloc ever happens inside a run (the first hb_run of a process is the ONLY one
                                              // a drop-in user makes, entrypoint/centrality.rs:49)
    unsigned long long *h_counters = nullptr; // kCounterWords words; [0..3] hold the stripe sums after a pass
    unsigned long long *h_slot = nullptr;     // 2 x kCounterWords: the counters of the two passes in flight
    uint32_t *h_tl_count = nullptr;           // kTcWords
    unsigned long long *h_rank_cnt = nullptr; // world words
    hipEvent_t ev[kEvSlots] = {}; // indexed by PassEvent
    // destination partition + changed-only: the pass' only host round trip sits in the MIDDLE of the pass (counters + run lengths,
    // before the broadcasts); what follows it is left in flight, so the pass' timing events are read later (resolve_pass_times)
    struct EvSet {
        hipEvent_t e[kEvSlots];
    };
    std::vector<EvSet> ev_pool;         // deferred timing (destination partition + changed-only on a communicator): one set per pass of a run
    EvSet ev_ring[4]{};                 // hb_run's tail pipeline (two passes in flight): pass t uses set t & 3; created by hb_create
    hipEvent_t tl_ev[2] = {nullptr, nullptr}; // the tail kernel's launch: kEvStart, kEvEnd
    hipEvent_t slot_done[2] = {nullptr, nullptr};   // pass q's counters have arrived in h_slot[q & 1]
    // edge partition with a communicator: the node rows are merged, all-reduced and finished in kOverlap row ranges - range
    // k's ncclAllReduce runs on comm_stream while range k + 1 is still being merged, its epilogue while k + 1 is reduced
    static constexpr int kOverlap = 4;
    hipStream_t comm_stream = nullptr;
    hipEvent_t ov_merged[kOverlap] = {nullptr, nullptr, nullptr, nullptr}, ov_reduced[kOverlap] = {nullptr, nullptr, nullptr, nullptr};
    hipStream_t rs_stream = nullptr;                    // the result snapshots' downloads run here, beside the passes (GraphDeviceState::rs)
    hipEvent_t rs_ready = nullptr, rs_copied = nullptr; // out[] built (main stream) / downloaded (side stream)

    // ---- load lifetime: the input and the plan on the host, and the sizes plan_and_upload derives from them.  Every load rewrites them
    // before `loaded` is set again; free_graph_buffers() does not touch them -------------------------------------------------------------
    std::vector<hb_edge> pending;  // hb_append_edges, host-ingest mode only
    // hb_append_edges, default: records are unpacked on the device as they arrive (2 x 16-byte endpoint keys + 1
    // flag byte each); nothing is buffered on the host
    IngestStream app;
    DenseGraph g;                  // ids kept; row_ptr/src kept only for hb_debug_copy_graph
    Plan plan;
    bool loaded = false;
    // who wrote d_regs / d_part / d_bits / the touch bitmap / the sweep scratch last, what d_out / h_out / res_count hold, and whether a
    // HyperBall run is open (hb_begin .. hb_finish).  Written by hb_begin, hb_finish, claim_rows and take_image (hb_api_walk.inc) and by
    // a load, by nobody else; DESIGN.md section 18 has the table of calls and states
    RowsOf rows = RowsOf::Nobody;
    Image image = Image::None;
    bool run_open = false;
    std::vector<DevBuf> allocs;   // what dev_alloc / adopt gave the graph state above; hb_stats.device_bytes is their sum
    uint64_t m_global = 0;        // edges of the whole graph (all ranks)
    uint64_t plan_entries = 0; // entries of all work rows' source lists
    uint64_t bits_words = 0;
    uint64_t ksum_len = 0; // entries allocated for ksum (world * slice in RCCL mode)
    uint64_t slice_rows = 0;
    uint64_t bloom_bits = 0;        // (hb_begin) bits of d_bloom
    uint64_t ref_threshold = 0;     // (hb_begin) exact_counting_threshold (harmonic.rs:228)
    hb_stats stats{};

    // ---- run lifetime: hb_begin .. hb_finish (or one call of hb_sampled_harmonic / hb_distances) ------------------------------------
    bool lean_init = false; // hb_begin left the initial counters / Kahan words / sizes to pass 0 (PassParams::rd_init); cleared by pass 0, or by
                            // ensure_initial_state() when something wants to look at the state before pass 0
    uint64_t t = 0;
    int cur = 0; // d_regs[cur] = "old"
    bool has_changes = false;
    bool pending_local = false; // between hb_step_local and hb_step_finish
    uint64_t last_changed = 0;
    uint64_t last_active = 0;     // out-degree sum of the nodes changed in the previous pass
    std::vector<hb_pass_stats> pstats;
    uint64_t co_rows = 0;     // rows in the union of this pass
    std::vector<uint64_t> ex_off; // world + 1: first packed position of every rank's slice
    std::vector<uint64_t> pending_times; // passes whose ms_* fields still have to be read from their events
    // hb_run's tail pipeline: pass q + 1 is queued (guarded on the device by pass q's changed count) before pass q's counters are
    // read, so the convergence tail runs without a host round trip between passes
    const unsigned long long *spec_guard = nullptr; // set while step_local queues a guarded pass
    bool pipelined = false;                         // step_local: take this pass' events from ev_pool
    uint64_t pipelined_passes = 0;                  // passes of this run queued ahead of their predecessor's read-back
    bool tl_declined = false;       // the tail kernel found the next pass too large for its lists: do not ask again before an ordinary pass has run
    uint64_t tail_kernel_passes = 0;
    uint64_t wire_bytes = 0;      // counter bytes this rank received over the run (changed-only accounting)
    bool exact_counting = false;    // harmonic.rs:231,277-279
    bool exact_valid = false;       // the previous pass filled exact_changed_nodes (ran with Some(..) or was a tail pass)
    bool stale = false;             // a tail pass has run: host-level edges may have been skipped, the bloom filter's
                                    // false positives are no longer results-inert
    uint64_t ov_lo[kOverlap + 1] = {0, 0, 0, 0, 0};
    int ov_ranges = 0; // ranges of the pending pass (0 = one launch over all rows, no overlap)
    uint32_t cur_mode = 0;
    uint64_t res_count = 0;
};

namespace {

int fail(hb_ctx *c, int code, const std::string &msg)
{
    if (c) c->err = msg;
    else g_create_error = msg;
    return code;
}

#define HB_HIP(call)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail(c, HB_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));        \
    } while (0)

#define HB_NCCL(call)                                                                             \
    do {                                                                                          \
        ncclResult_t r_ = (call);                                                                 \
        if (r_ != ncclSuccess)                                                                    \
            return fail(c, HB_ERR_RCCL, std::string(#call) + ": " + ncclGetErrorString(r_));      \
    } while (0)

template <typename T>
int dev_alloc(hb_ctx *c, T **out, size_t count)
{
    size_t bytes = std::max<size_t>(count * sizeof(T), 256);
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess)
        return fail(c, HB_ERR_NOMEM, "hipMalloc(" + std::to_string(bytes) + " bytes): " + hipGetErrorString(e));
    c->allocs.push_back({p, bytes});
    c->stats.device_bytes += bytes;
    *out = (T *)p;
    return HB_OK;
}

// A holder of an operator's state (LinksState, SimilarHostsState, SimilarityLimitState, ScoreState) with at least `need` entries: it
// only grows.  Its bytes are booked in the state's own count (`booked`) and in hb_stats.device_bytes
template <class T>
int hold(hb_ctx *c, uint64_t &booked, GrowPtr<T> &h, uint64_t need)
{
    if (h && h.have >= need) return HB_OK;
    const uint64_t old_bytes = h ? std::max<uint64_t>(h.have * sizeof(T), 256) : 0;
    h.reset();
    booked -= old_bytes;
    c->stats.device_bytes -= old_bytes;
    h.have = 0;
    const uint64_t bytes = std::max<uint64_t>(need * sizeof(T), 256);
    const hipError_t e = h.alloc((bytes + sizeof(T) - 1) / sizeof(T));
    if (e != hipSuccess) return fail(c, HB_ERR_NOMEM, "hipMalloc(" + std::to_string(bytes) + " bytes): " + hipGetErrorString(e));
    h.have = need;
    booked += bytes;
    c->stats.device_bytes += bytes;
    return HB_OK;
}

// The lap timer of the operators that time a step between kEvMerge and kEvCollective: lap_start marks the beginning on the stream; lap
// records the end, drains the stream and adds the elapsed GPU time to *ms_out
int lap_start(hb_ctx *c)
{
    HB_HIP(hipEventRecord(c->ev[kEvMerge], c->stream));
    return HB_OK;
}

int lap(hb_ctx *c, double *ms_out)
{
    HB_HIP(hipEventRecord(c->ev[kEvCollective], c->stream));
    HB_HIP(hipStreamSynchronize(c->stream));
    float ms = 0.f;
    HB_HIP(hipEventElapsedTime(&ms, c->ev[kEvMerge], c->ev[kEvCollective]));
    *ms_out += ms;
    return HB_OK;
}

// The same, but the failure is reported as `what` + the error string (messages that name the step rather than the call)
#define HB_HIP_AS(what, call)                                                                     \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) return fail(c, HB_ERR_HIP, std::string(what) + hipGetErrorString(e_)); \
    } while (0)

void free_graph_buffers(hb_ctx *c)
{
    if (c->rs_stream) (void)hipStreamSynchronize(c->rs_stream); // (a snapshot may still be landing in h_out)
    for (auto &b : c->allocs) (void)hipFree(b.p);
    c->allocs.clear();
    for (void *q : {(void *)c->h_out, (void *)c->rs.h_sid, (void *)c->rs.h_val, (void *)c->rs.h_count})
        if (q) (void)hipHostFree(q);
    tail_index_free(c->tail_index);
    static_cast<GraphDeviceState &>(*c) = GraphDeviceState{}; // (the DevPtr / GrowPtr holders of the operators' states free their buffers here)
    c->stats.device_bytes = 0;
}

// ---- the operators' common prologue ----------------------------------------------------------------------------------------------
// Versioned structs of the C ABI (include/hyperball.h): the caller says how much of the struct it knows in struct_size (0 = all of it);
// that many bytes are copied, the rest of an input keeps its defaults, and an output's struct_size says how many were written.
template <class T>
void copy_in(const T *from, T *to)
{
    if (from) std::memcpy(to, from, from->struct_size ? std::min<size_t>(from->struct_size, sizeof(T)) : sizeof(T));
}
template <class T>
void copy_out(T *to, T &from)
{
    if (!to) return;
    const size_t sz = to->struct_size ? std::min<size_t>(to->struct_size, sizeof(T)) : sizeof(T);
    from.struct_size = (uint32_t)sz;
    std::memcpy(to, &from, sz);
}

// an unchecked failure of an earlier call on this thread would be reported by the first HB_HIP(hipGetLastError()) of `who`
int refuse_stale_error(hb_ctx *c, const char *who)
{
    const hipError_t stale = hipGetLastError();
    if (stale != hipSuccess) return fail(c, HB_ERR_HIP, std::string("stale HIP error before ") + who + ": " + hipGetErrorString(stale));
    return HB_OK;
}

// NodeID -> sid of the loaded graph (c->g.ids is ascending); false = not a node
bool find_sid(const hb_ctx *c, const hb_u128 &id, uint32_t *sid)
{
    const auto it = std::lower_bound(c->g.ids.begin(), c->g.ids.end(), id, u128_less);
    if (it == c->g.ids.end() || !u128_eq(*it, id)) return false;
    *sid = (uint32_t)(it - c->g.ids.begin());
    return true;
}

// the bit-per-row kernels of the operators walk the plan in 32-row words: the node rows and every virtual level begin on one
int plan_rows_word_aligned(hb_ctx *c, const char *who)
{
    const Plan &p = c->plan;
    if (p.n_pad % 32 || std::any_of(p.level_begin.begin(), p.level_begin.end(), [](uint64_t b) { return b % 32 != 0; }))
        return fail(c, HB_ERR_INVALID, std::string(who) + ": unexpected plan layout (a level does not begin on a 32-row word)");
    return HB_OK;
}

// hb_options.chunk / tune[3..5] -> planner knobs
PlanTune plan_tune(uint32_t chunk, const uint32_t *tune)
{
    PlanTune t;
    t.chunk = chunk ? chunk : kDefaultChunk;
    if (tune) {
        if (tune[3] == 1) t.band_w = 0;                     // banding off
        else if (tune[3] >= 4 && tune[3] < 31) t.band_w = 1u << tune[3];
        if (tune[4]) t.minc = tune[4];
        if (tune[5]) t.direct_max = tune[5];
    }
    return t;
}

// live-first device order (HB_FLAG_LIVE_FIRST), the part of the rule the option flags and the size decide: fused passes that do not
// count their gathers, a reordered plan; on from 2^20 nodes (the size from which the result image is staged), the two flags force it
// on below / off above.  A context adds what it alone knows (plan_and_upload: one rank, no communicator, no destination partition)
bool live_first_by_flags(uint32_t flags, uint64_t n)
{
    if (flags & (HB_FLAG_NO_REORDER | HB_FLAG_PASS_STATS | HB_FLAG_UNFUSED | HB_FLAG_REFERENCE_TAIL | HB_FLAG_NO_LIVE_FIRST)) return false;
    return n >= (1u << 20) || (flags & HB_FLAG_LIVE_FIRST);
}
// saturated rows, the part of the gate the option flags decide: fused passes that do not count their gathers.
// On by default; a context adds what it alone knows (plan_and_upload: one rank, no communicator, no destination partition)
bool saturation_by_flags(uint32_t flags)
{
    return !(flags & (HB_FLAG_PASS_STATS | HB_FLAG_UNFUSED | HB_FLAG_REFERENCE_TAIL | HB_FLAG_NO_SATURATION));
}

bool multi_rank(const hb_ctx *c) { return c->opt.world_size > 1; }
// a switch of the experiments build (hb_experiments.h HB_X_*; several or-ed: any of them); always off in the product library
bool xbit(const hb_ctx *c, uint32_t bits) { return (HB_XBITS(c->opt.tune[1]) & bits) != 0; }
// blocks for `groups` groups of work items, at most `per_cu` per CU and at least `floor`
unsigned grid_blocks(const hb_ctx *c, uint64_t groups, uint64_t per_cu, uint64_t floor = 0)
{
    return (unsigned)std::max<uint64_t>(std::min<uint64_t>(groups, (uint64_t)c->num_cu * per_cu), floor);
}
// the context can exchange with the other ranks by itself: an RCCL communicator, or the caller's collectives
bool linked(const hb_ctx *c) { return c->comm != nullptr || c->coll.all_reduce != nullptr; }

#define HB_COLL(call)                 \
    do {                              \
        const int rc_coll_ = (call);  \
        if (rc_coll_) return rc_coll_; \
    } while (0)
int coll_dtype(ncclDataType_t dt) { return dt == ncclUint8 ? HB_COLL_U8 : dt == ncclUint32 ? HB_COLL_U32 : dt == ncclUint64 ? HB_COLL_U64 : HB_COLL_F64; }
uint64_t coll_size(ncclDataType_t dt) { return dt == ncclUint8 ? 1 : dt == ncclUint32 ? 4 : 8; }
// in place, like every exchange of the pass driver
int coll_all_reduce(hb_ctx *c, void *buf, uint64_t count, ncclDataType_t dt, ncclRedOp_t op, hipStream_t s)
{
    if (c->comm) {
        HB_NCCL(ncclAllReduce(buf, buf, count, dt, op, c->comm, s));
        return HB_OK;
    }
    if (c->coll.all_reduce(c->coll.user, buf, count, coll_dtype(dt), op == ncclMax ? HB_COLL_MAX : HB_COLL_SUM, (void *)s))
        return fail(c, HB_ERR_RCCL, "the caller's all_reduce (hb_set_collectives) failed");
    return HB_OK;
}
// recv holds world x count elements, send = this rank's count elements (may lie inside recv at its place)
int coll_all_gather(hb_ctx *c, const void *send, void *recv, uint64_t count, ncclDataType_t dt, hipStream_t s)
{
    if (c->comm) {
        HB_NCCL(ncclAllGather(send, recv, count, dt, c->comm, s));
        return HB_OK;
    }
    if (c->coll.all_gather(c->coll.user, send, recv, count * coll_size(dt), (void *)s))
        return fail(c, HB_ERR_RCCL, "the caller's all_gather (hb_set_collectives) failed");
    return HB_OK;
}
int coll_broadcast(hb_ctx *c, void *buf, uint64_t count, ncclDataType_t dt, int root, hipStream_t s)
{
    if (c->comm) {
        HB_NCCL(ncclBroadcast(buf, buf, count, dt, root, c->comm, s));
        return HB_OK;
    }
    if (c->coll.broadcast(c->coll.user, buf, count * coll_size(dt), root, (void *)s))
        return fail(c, HB_ERR_RCCL, "the caller's broadcast (hb_set_collectives) failed");
    return HB_OK;
}
// piece k of send (world x bytes_per_rank) to rank k, piece k of recv from rank k; send != recv (HB_FLAG_PACKED_WIRE, edge partition)
int coll_all_to_all(hb_ctx *c, const void *send, void *recv, uint64_t bytes_per_rank, hipStream_t s)
{
    if (c->comm) {
        const int world = std::max(c->opt.world_size, 1);
        if (world == 1) { // (HB_FLAG_RCCL_SELF: the one piece is this rank's own)
            if (bytes_per_rank) HB_HIP(hipMemcpyAsync(recv, send, bytes_per_rank, hipMemcpyDeviceToDevice, s));
            return HB_OK;
        }
#ifdef NCCL_VERSION_CODE
        // NEVER RUN: two ranks of a communicator need two GPUs, and no test of this repository has had them.  The grouped
        // point-to-point form is RCCL's documented all-to-all (one send and one receive per peer inside one group).
        HB_NCCL(ncclGroupStart());
        for (int k = 0; k < world; k++) {
            HB_NCCL(ncclSend((const uint8_t *)send + (uint64_t)k * bytes_per_rank, bytes_per_rank, ncclUint8, k, c->comm, s));
            HB_NCCL(ncclRecv((uint8_t *)recv + (uint64_t)k * bytes_per_rank, bytes_per_rank, ncclUint8, k, c->comm, s));
        }
        HB_NCCL(ncclGroupEnd());
        return HB_OK;
#else
        return fail(c, HB_ERR_RCCL, "all-to-all between the ranks of a communicator: this build's RCCL header has no ncclSend / ncclRecv");
#endif
    }
    if (!c->coll_a2a) return fail(c, HB_ERR_INVALID, "HB_FLAG_PACKED_WIRE on the edge partition needs hb_set_all_to_all beside hb_set_collectives");
    if (c->coll_a2a(c->coll.user, send, recv, bytes_per_rank, (void *)s)) return fail(c, HB_ERR_RCCL, "the caller's all_to_all (hb_set_all_to_all) failed");
    return HB_OK;
}
int coll_group_start(hb_ctx *c)
{
    if (c->comm) HB_NCCL(ncclGroupStart());
    return HB_OK;
}
int coll_group_end(hb_ctx *c)
{
    if (c->comm) HB_NCCL(ncclGroupEnd());
    return HB_OK;
}
// destination partition: this rank owns the rows (nodes) with sid % world == rank and holds all their
// in-edges; one all-gather of the owned counter slices per pass
// (also with a 1-rank communicator, HB_FLAG_RCCL_SELF: the grouped all-gathers run for real on one GPU)
bool dest_mode(const hb_ctx *c)
{
    return (c->opt.flags & HB_FLAG_DEST_PARTITION) && (multi_rank(c) || (c->opt.flags & HB_FLAG_RCCL_SELF));
}
// edge partition: every rank holds some in-edges of every row; one all-reduce(max) of all counters per pass
bool edge_partitioned(const hb_ctx *c) { return multi_rank(c) && !dest_mode(c); }
bool ref_tail(const hb_ctx *c) { return (c->opt.flags & HB_FLAG_REFERENCE_TAIL) != 0; }
// rel-flag bits that drop a record at ingest: SKIPPED_REL (harmonic.rs:131), none with HB_FLAG_ALL_RELS (ForwardlinksQuery has no
// rel filter, query/forwardlink.rs:44-53: the page graph of approx_harmonic.rs follows every edge)
uint64_t skip_mask(const hb_ctx *c) { return (c->opt.flags & HB_FLAG_ALL_RELS) ? 0ull : HB_SKIPPED_REL_MASK; }
// HB_FLAG_PACKED_WIRE: whole counters travel as 48-byte rows; a context that exchanges nothing ignores the flag
bool packed_wire(const hb_ctx *c) { return (c->opt.flags & HB_FLAG_PACKED_WIRE) && (multi_rank(c) || linked(c)); }
bool unfused(const hb_ctx *c)
{
    return edge_partitioned(c) || (linked(c) && !dest_mode(c)) || (c->opt.flags & HB_FLAG_UNFUSED) || ref_tail(c);
}

// Transposed work-row graph (who reads each node / virtual row), touch bitmap and seed lists for the
// sweep-mode passes; built on the device from the uploaded plan, prefix sum on the host.
int build_sparse_support(hb_ctx *c)
{
    const Plan &p = c->plan;
    c->sparse_ok = false;
    if (unfused(c) || multi_rank(c) || (c->opt.flags & HB_FLAG_NO_SPARSE) || p.n == 0) return HB_OK;
    const uint64_t rows_total = p.n_pad + p.nv;
    const uint64_t entries = c->plan_entries;
    int rc;
    uint32_t *d_count = nullptr;
    if ((rc = dev_alloc(c, &c->d_out_ptr, rows_total + 1))) return rc;
    if ((rc = dev_alloc(c, &c->d_out_rows, entries))) return rc;
    if ((rc = dev_alloc(c, &c->d_touch, c->bits_words + 64))) return rc; // + 64: a wave reads 64 words at a time
    if ((rc = dev_alloc(c, &c->d_seeds, p.n_pad))) return rc;
    if ((rc = dev_alloc(c, &c->d_heavy, p.n_pad))) return rc;
    if ((rc = dev_alloc(c, &c->d_sparse_counts, 64))) return rc;
#ifdef HB_EXPERIMENTS
    for (int k = 0; k < 2; k++) { // the tail kernel's lists (hb_tail.hip.h): 2.7 MB in all
        if ((rc = dev_alloc(c, &c->d_tl_changed[k], hbk::kTailCap))) return rc;
        if ((rc = dev_alloc(c, &c->d_tl_vchanged[k], hbk::kTailCap))) return rc;
        if ((rc = dev_alloc(c, &c->d_tl_dirty[k], hbk::kTailCap))) return rc;
    }
    if ((rc = dev_alloc(c, &c->d_tl_work, (size_t)(hbk::kTailLevels + 1) * hbk::kTailCap))) return rc;
    if ((rc = dev_alloc(c, &c->d_tl_count, hbk::kTcWords))) return rc;
#endif
    HB_HIP(hipMemsetAsync(c->d_touch, 0, (c->bits_words + 64) * sizeof(uint32_t), c->stream));
    {   // [r6] by sorting (hb_plan.hip gpu_transpose_rows: streaming traffic only); the scatter form below only when the device cannot
        // lend the sort 16 bytes per entry, or on request (HB_X_SCATTER_TRANSPOSE: A/B runs and the parity variant that
        // keeps the fallback exact)
        if (!xbit(c, HB_X_SCATTER_TRANSPOSE)) {
            const std::string e = gpu_transpose_rows((void *)c->stream, c->d_row_ptr, c->d_src, rows_total, entries, c->d_out_ptr, c->d_out_rows);
            if (e.empty()) {
                c->sparse_ok = true;
                return HB_OK;
            }
            if (e.find("out of memory") == std::string::npos) return fail(c, HB_ERR_HIP, e);
            (void)hipGetLastError();
        }
    }
    if ((rc = dev_alloc(c, &d_count, rows_total))) return rc; // stays allocated (small next to out_rows)
    HB_HIP(hipMemsetAsync(d_count, 0, rows_total * sizeof(uint32_t), c->stream));
    const unsigned blocks = grid_blocks(c, (rows_total * 4 + 255) / 256, 16);
    hipLaunchKernelGGL(hbk::transpose_count_kernel, dim3(blocks), dim3(256), 0, c->stream, (const uint64_t *)c->d_row_ptr,
                       (const uint32_t *)c->d_src, rows_total, d_count);
    HB_HIP(hipGetLastError());
    {   // out_ptr = exclusive prefix sums of the reader counts (rows_total + 1 entries), on the device
        std::string e = device_offsets((void *)c->stream, d_count, rows_total, c->d_out_ptr, entries);
        if (!e.empty()) return fail(c, HB_ERR_HIP, e);
    }
    HB_HIP(hipMemsetAsync(d_count, 0, rows_total * sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(hbk::transpose_fill_kernel, dim3(blocks), dim3(256), 0, c->stream, (const uint64_t *)c->d_row_ptr,
                       (const uint32_t *)c->d_src, rows_total, (const uint64_t *)c->d_out_ptr, d_count, c->d_out_rows);
    HB_HIP(hipGetLastError());
    HB_HIP(hipStreamSynchronize(c->stream));
    c->sparse_ok = true;
    return HB_OK;
}

#include "hb_api_load.inc"

#include "hb_api_pass.inc"

// The C ABI never unwinds (include/hyperball.h): every entry point that can allocate runs under this guard.
template <class F>
int guarded(hb_ctx *c, F &&f)
{
    try {
        const int rc = f();
        HB_GUARD_CHECK("exit of a C-ABI entry point"); // red-zone debug build only (hb_guard_alloc.h)
#ifdef HB_DEBUG_BOUNDS
        if (c) { // a device-side index check failed somewhere in this call (hb_kernels.hip.h HB_DBG_ASSERT)
            unsigned int line = 0;
            (void)hipDeviceSynchronize();
            if (hipMemcpyFromSymbol(&line, HIP_SYMBOL(hbk::g_dbg_line), sizeof(line)) == hipSuccess && line)
                return fail(c, HB_ERR_INVALID, "HB_DEBUG_BOUNDS: device-side index check failed at kernel source line " + std::to_string(line));
        }
#endif
        return rc;
    } catch (const std::bad_alloc &) {
        try { return fail(c, HB_ERR_NOMEM, "out of host memory"); } catch (...) { return HB_ERR_NOMEM; }
    } catch (const std::exception &e) {
        try { return fail(c, HB_ERR_INVALID, std::string("C++ exception: ") + e.what()); } catch (...) { return HB_ERR_INVALID; }
    } catch (...) {
        try { return fail(c, HB_ERR_INVALID, "unknown C++ exception"); } catch (...) { return HB_ERR_INVALID; }
    }
}

// the device cannot hold the stream (memory, or a debug limit): the records appended so far come back as hb_edge records
// (hb_ingest.hip gpu_ingest_spill) and the stream continues on the host path
int spill_appended_to_host(hb_ctx *c)
{
    const std::string e = gpu_ingest_spill((void *)c->stream, &c->app, &c->pending);
    if (!e.empty()) return fail(c, e.find("memory") != std::string::npos ? HB_ERR_NOMEM : HB_ERR_HIP, e);
    return HB_OK;
}

int set_device(hb_ctx *c)
{
    HB_HIP(hipSetDevice(c->device));
    return HB_OK;
}

} // namespace

// =============================================================================================
extern "C" {

int hb_abi_version(void) { return HB_ABI_VERSION; }

const char *hb_last_error(const hb_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int hb_device_count(int *count)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) n = 0;
    if (count) *count = n;
    return HB_OK;
}

int hb_rccl_unique_id(uint8_t out[128])
{
    return guarded(nullptr, [&]() -> int {
        hb_ctx *c = nullptr;
        if (!out) return fail(c, HB_ERR_INVALID, "out == NULL");
        static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
        ncclUniqueId id;
        HB_NCCL(ncclGetUniqueId(&id));
        std::memcpy(out, &id, 128);
        return HB_OK;
    });
}

int hb_create(const hb_options *opt, hb_ctx **out)
{
    return guarded(nullptr, [&]() -> int {
        hb_ctx *c = nullptr; // errors before the ctx exists go to the thread-local slot
        if (!out) return fail(c, HB_ERR_INVALID, "out == NULL");
        *out = nullptr;
        hb_options o{};
        if (!opt) o.device = -1;
        copy_in(opt, &o);
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
            return fail(c, HB_ERR_NO_DEVICE, "no HIP device visible: this library has no CPU fallback");
        int dev = o.device;
        if (dev < 0) {
            if (hipGetDevice(&dev) != hipSuccess) dev = 0;
        }
        if (dev >= ndev) return fail(c, HB_ERR_INVALID, "device ordinal out of range");
        hipDeviceProp_t prop;
        HB_HIP(hipGetDeviceProperties(&prop, dev));
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
            return fail(c, HB_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
        if (o.world_size > 1 && (o.rank < 0 || o.rank >= o.world_size)) return fail(c, HB_ERR_INVALID, "rank out of range");
#ifndef HB_EXPERIMENTS
        if ((o.tune[1] & ~HB_TUNE1_UNROLL) || o.tune[7])
            return fail(c, HB_ERR_INVALID, "hb_options.tune[1] bits above the low byte and tune[7] are switches of the experiments build (libhyperball_exp.so, "
                                           "-DHB_EXPERIMENTS: stract_amd/csrc/hb_experiments.h); the product library has none of them");
#endif
        if ((o.flags & HB_FLAG_REFERENCE_TAIL) && (o.world_size > 1 || (o.flags & (HB_FLAG_RCCL_SELF | HB_FLAG_DEST_PARTITION))))
            return fail(c, HB_ERR_INVALID, "HB_FLAG_REFERENCE_TAIL is a single-rank mode (no partition / RCCL flags)");
        if ((o.flags & HB_FLAG_PACKED_WIRE) && (o.flags & HB_FLAG_REFERENCE_TAIL))
            return fail(c, HB_ERR_INVALID, "HB_FLAG_PACKED_WIRE and HB_FLAG_REFERENCE_TAIL exclude each other (the tail mode is a single-rank mode: it has no wire)");
#ifdef HB_EXPERIMENTS
        if ((o.flags & HB_FLAG_PACKED_WIRE) && (HB_XBITS(o.tune[1]) & HB_X_WIRE_64B))
            return fail(c, HB_ERR_INVALID, "HB_FLAG_PACKED_WIRE and HB_X_WIRE_64B exclude each other (48-byte rows everywhere against 64-byte rows in the changed-only exchange)");
#endif
        if ((o.flags & HB_FLAG_ALL_RELS) && (o.flags & HB_FLAG_REFERENCE_TAIL))
            return fail(c, HB_ERR_INVALID, "HB_FLAG_ALL_RELS and HB_FLAG_REFERENCE_TAIL exclude each other (the tail mode replays the rel filter)");
        hb_ctx *ctx = new (std::nothrow) hb_ctx();
        if (!ctx) return fail(c, HB_ERR_NOMEM, "out of host memory");
        ctx->opt = o;
        ctx->device = dev;
        ctx->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        ctx->arch = prop.gcnArchName;
        ctx->max_passes = o.max_passes ? o.max_passes : 4096;
        c = ctx;
        auto bail = [&](int code) {
            std::string m = ctx->err;
            hb_destroy(ctx);
            g_create_error = m;
            return code;
        };
        if (hipSetDevice(dev) != hipSuccess) { ctx->err = "hipSetDevice failed"; return bail(HB_ERR_HIP); }
        if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { ctx->err = "hipStreamCreate failed"; return bail(HB_ERR_HIP); }
        for (int i = 0; i < kEvSlots; i++)
            if (hipEventCreate(&ctx->ev[i]) != hipSuccess) { ctx->err = "hipEventCreate failed"; return bail(HB_ERR_HIP); }
        {   // every small page-locked word the pass driver will ever read back, in one block, NOW: a hipHostMalloc inside the first run
            // cost that run 13 ms at C3 and ~200 ms at C4 under a loaded page cache (profiles/r05j_e2e_C4_first_run_and_store_phases.txt)
            const size_t world = (size_t)std::max(o.world_size, 1);
            const size_t words = (size_t)hbk::kCounterWords * 3 + 32 + world + 1; // h_counters | h_slot (2 sets) | h_tl_count (kTcWords x u32) | h_rank_cnt
            if (hipHostMalloc(&ctx->h_block, words * sizeof(unsigned long long)) != hipSuccess) { ctx->h_block = nullptr; ctx->err = "hipHostMalloc failed"; return bail(HB_ERR_NOMEM); }
            std::memset(ctx->h_block, 0, words * sizeof(unsigned long long));
            unsigned long long *w = (unsigned long long *)ctx->h_block;
            ctx->h_counters = w;
            ctx->h_slot = w + hbk::kCounterWords;
            ctx->h_tl_count = (uint32_t *)(w + 3 * (size_t)hbk::kCounterWords);
            ctx->h_rank_cnt = w + 3 * (size_t)hbk::kCounterWords + 32;
#ifdef HB_EXPERIMENTS
            static_assert(hbk::kTcWords * sizeof(uint32_t) <= 32 * sizeof(unsigned long long), "h_tl_count slot too small");
#endif
        }
        for (auto &e : ctx->slot_done)
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { ctx->err = "hipEventCreate failed"; return bail(HB_ERR_HIP); }
        for (auto &e : ctx->tl_ev)
            if (hipEventCreate(&e) != hipSuccess) { ctx->err = "hipEventCreate failed"; return bail(HB_ERR_HIP); }
        for (auto &es : ctx->ev_ring)
            for (auto &e : es.e)
                if (hipEventCreate(&e) != hipSuccess) { ctx->err = "hipEventCreate failed"; return bail(HB_ERR_HIP); }
        if (hipStreamCreateWithFlags(&ctx->rs_stream, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&ctx->rs_ready, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&ctx->rs_copied, hipEventDisableTiming) != hipSuccess) { ctx->err = "hipStreamCreate / hipEventCreate failed"; return bail(HB_ERR_HIP); }
        if ((o.world_size > 1 && !(o.flags & HB_FLAG_NO_RCCL)) || (o.flags & HB_FLAG_RCCL_SELF)) {
            if (hipStreamCreateWithFlags(&ctx->comm_stream, hipStreamNonBlocking) != hipSuccess) { ctx->err = "hipStreamCreate failed"; return bail(HB_ERR_HIP); }
            for (int i = 0; i < hb_ctx::kOverlap; i++)
                if (hipEventCreateWithFlags(&ctx->ov_merged[i], hipEventDisableTiming) != hipSuccess ||
                    hipEventCreateWithFlags(&ctx->ov_reduced[i], hipEventDisableTiming) != hipSuccess) { ctx->err = "hipEventCreate failed"; return bail(HB_ERR_HIP); }
        }
        if (o.world_size > 1 && !(o.flags & HB_FLAG_NO_RCCL)) {
            ncclUniqueId id;
            std::memcpy(&id, o.rccl_id, 128);
            ncclResult_t r = ncclCommInitRank(&ctx->comm, o.world_size, id, o.rank);
            if (r != ncclSuccess) { ctx->err = std::string("ncclCommInitRank: ") + ncclGetErrorString(r); ctx->comm = nullptr; return bail(HB_ERR_RCCL); }
        } else if (o.world_size == 1 && (o.flags & HB_FLAG_RCCL_SELF)) {
            ncclUniqueId id;
            std::memcpy(&id, o.rccl_id, 128);
            ncclResult_t r = ncclCommInitRank(&ctx->comm, 1, id, 0);
            if (r != ncclSuccess) { ctx->err = std::string("ncclCommInitRank: ") + ncclGetErrorString(r); ctx->comm = nullptr; return bail(HB_ERR_RCCL); }
        }
        *out = ctx;
        return HB_OK;
    });
}

void hb_destroy(hb_ctx *ctx)
{
    if (!ctx) return;
    struct Trim { // after everything below has gone back to the caching allocator: free blocks return to the runtime
        ~Trim() { HB_POOL_TRIM(); }
    } trim_at_exit;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->comm) (void)ncclCommDestroy(ctx->comm);
    ctx->app.free_all();
    free_graph_buffers(ctx);
    if (ctx->h_block) (void)hipHostFree(ctx->h_block); // h_counters, h_slot, h_tl_count, h_rank_cnt
    for (auto &es : ctx->ev_ring)
        for (hipEvent_t e : es.e)
            if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->tl_ev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->slot_done)
        if (e) (void)hipEventDestroy(e);
    for (auto &es : ctx->ev_pool)
        for (hipEvent_t e : es.e)
            if (e) (void)hipEventDestroy(e);
    for (int i = 0; i < kEvSlots; i++)
        if (ctx->ev[i]) (void)hipEventDestroy(ctx->ev[i]);
    for (int i = 0; i < hb_ctx::kOverlap; i++) {
        if (ctx->ov_merged[i]) (void)hipEventDestroy(ctx->ov_merged[i]);
        if (ctx->ov_reduced[i]) (void)hipEventDestroy(ctx->ov_reduced[i]);
    }
    if (ctx->comm_stream) {
        (void)hipStreamSynchronize(ctx->comm_stream);
        (void)hipStreamDestroy(ctx->comm_stream);
    }
    if (ctx->rs_ready) (void)hipEventDestroy(ctx->rs_ready);
    if (ctx->rs_copied) (void)hipEventDestroy(ctx->rs_copied);
    if (ctx->rs_stream) (void)hipStreamDestroy(ctx->rs_stream);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int hb_release_cached_memory(uint64_t *released)
{
    try {
        const size_t before = HB_POOL_RESERVED();
        HB_POOL_TRIM();
        if (released) *released = (uint64_t)(before - std::min<size_t>(before, HB_POOL_RESERVED()));
        return HB_OK;
    } catch (...) {
        return HB_ERR_NOMEM;
    }
}

int hb_device_name(const hb_ctx *ctx, char *name, uint64_t cap)
{
    if (!ctx || !name || !cap) return HB_ERR_INVALID;
    std::snprintf(name, (size_t)cap, "%s", ctx->arch.c_str());
    return HB_OK;
}

int hb_device_synchronize(hb_ctx *c)
{
    return guarded(c, [&]() -> int {
        if (!c) return HB_ERR_INVALID;
        int rc = set_device(c);
        if (rc) return rc;
        HB_HIP(hipStreamSynchronize(c->stream));
        return HB_OK;
    });
}

// ---- input --------------------------------------------------------------------------------
int hb_load_edges(hb_ctx *c, const hb_u128 *node_ids, uint64_t n, const hb_edge *edges, uint64_t m)
{
    return guarded(c, [&]() -> int {
        if (!c) return HB_ERR_INVALID;
        int rc = set_device(c);
        if (rc) return rc;
        c->stats = hb_stats{};
        HB_POOL_RESET_PEAK(); // hb_stats.pool_peak_bytes counts from the beginning of this load
        double t0 = now_ms();
        // node/edge-set reduction: on the GPU (hb_ingest.hip) unless the host path is forced; identical output
        // The device pipeline keeps ~18 B per record resident at its peak (9 B held, 16 B during the sort):
        // when that cannot fit, or an allocation fails anyway, the host path produces the same graph.
        bool on_host = (c->opt.flags & HB_FLAG_HOST_INGEST) != 0 || (c->lim_records && m >= c->lim_records);
        if (!on_host) {
            size_t free_b = 0, total_b = 0;
            // held: 9 B per record + the endpoint table; sort: 16 B per record; ~60 B per node while the ids are sorted
            // + the endpoint table: 20 B per slot at a load factor of 1/4 .. 1/2 = up to 160 B per distinct endpoint;
            // their number is not known before the records are read - the caller's node list if there is one, else at most
            // two per record and (what every graph this library is meant for satisfies) no more than a tenth of the records
            const double endpoints = (node_ids && n) ? (double)n : std::min(2.0 * (double)m, std::max(0.1 * (double)m, 1e6));
            const double need = 18.0 * (double)m + 48.0 * (double)((node_ids && n) ? n : 0) + 160.0 * endpoints + 1024e6;
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need > (double)free_b + (double)HB_POOL_CACHED_FREE()) on_host = true;
        }
        OwnedCsr csr;
        const bool keep_on_device = !on_host && device_plan(c);
        uint64_t peak = 0;
        const uint64_t skip = skip_mask(c);
        std::string e = on_host ? ingest_edges(node_ids, n, edges, m, &c->g, skip)
                                : gpu_ingest_edges((void *)c->stream, node_ids, n, edges, m, &c->g, keep_on_device ? &csr.d : nullptr, &peak, skip);
        // (the id space of the device table exhausted is a limit of the DEVICE ingest only: endpoints outside a caller-supplied
        // node list are legal and ignored by the reference, store.rs:338-357 - the host path takes over, like for memory)
        if (!on_host && !e.empty() && (e.find("out of memory") != std::string::npos || e.find("OutOfMemory") != std::string::npos ||
                                       e.find("too many nodes for the device ingest") != std::string::npos)) {
            (void)hipGetLastError(); // clear the sticky allocation error
            peak = 0;
            e = ingest_edges(node_ids, n, edges, m, &c->g, skip);
        }
        if (!e.empty())
            return fail(c, e.find("memory") != std::string::npos ? HB_ERR_NOMEM : (e.find("hip") != std::string::npos ? HB_ERR_HIP : HB_ERR_LIMIT), e);
        if ((rc = keep_owned(c, &csr.d))) return rc;
        const uint64_t nn = c->g.ids.size();
        const uint64_t m_eff = csr.d.d_row_ptr ? csr.d.m : (nn && c->g.row_ptr.size() == nn + 1 ? c->g.row_ptr[nn] : 0);
        c->stats.ms_ingest = now_ms() - t0;
        double ing = c->stats.ms_ingest;
        rc = plan_and_upload(c, std::move(csr), m_eff);
        c->stats.ms_ingest = ing;
        c->stats.ingest_peak_bytes = peak;
        return rc;
    });
}

int hb_append_edges(hb_ctx *c, const hb_edge *edges, uint64_t m)
{
    return guarded(c, [&]() -> int {
        if (!c || (m && !edges)) return c ? fail(c, HB_ERR_INVALID, "edges == NULL") : HB_ERR_INVALID;
        if (!m) return HB_OK;
        int rc = set_device(c);
        if (rc) return rc;
        const bool on_host = (c->opt.flags & HB_FLAG_HOST_INGEST) != 0 || !c->pending.empty();
        if (!on_host) {
            // unpack this batch behind what is already on the device (chunked: no reallocation, 33 bytes per record)
            c->app.max_records = c->lim_records;
            c->app.max_bytes = c->lim_bytes;
            c->app.chunk_records = c->lim_chunk;
            c->app.skip_mask = skip_mask(c);
            const std::string err = gpu_ingest_append((void *)c->stream, &c->app, edges, m);
            if (err.empty()) return HB_OK;
            if (err.find("out of memory") == std::string::npos && err.find("too many records") == std::string::npos &&
                err.find("too many nodes for the device ingest") == std::string::npos)
                return fail(c, HB_ERR_HIP, err);
            // the device cannot hold the stream (memory, or the 2^32-record limit of the device reduction): bring back
            // what is there and continue on the host
            rc = spill_appended_to_host(c);
            if (rc) return rc;
        }
        c->pending.insert(c->pending.end(), edges, edges + m);
        return HB_OK;
    });
}

int hb_finalize(hb_ctx *c, const hb_u128 *node_ids, uint64_t n)
{
    return guarded(c, [&]() -> int {
        if (!c) return HB_ERR_INVALID;
        int rc = set_device(c);
        if (rc) return rc;
        if (c->app.chunks.empty()) { // host mode (or nothing appended)
            const uint64_t keep_lim = c->lim_records;
            if (!c->pending.empty()) c->lim_records = 1; // the stream was spilled: it stays on the host path (m >= 1)
            rc = hb_load_edges(c, node_ids, n, c->pending.data(), c->pending.size());
            c->lim_records = keep_lim;
            std::vector<hb_edge>().swap(c->pending);
            return rc;
        }
        c->stats = hb_stats{};
        const double t0 = now_ms();
        const bool trace = std::getenv("HB_TRACE_INGEST") != nullptr;
        OwnedCsr csr;
        const bool keep_on_device = device_plan(c);
        uint64_t peak = 0;
        const std::string e = gpu_ingest_reduce((void *)c->stream, node_ids, n, &c->app, &c->g, keep_on_device ? &csr.d : nullptr, &peak);
        if (trace) std::fprintf(stderr, "[hb finalize] gpu_ingest_reduce returned after %.1f ms\n", now_ms() - t0);
        if (!e.empty())
            return fail(c, e.find("memory") != std::string::npos ? HB_ERR_NOMEM : (e.find("hip") != std::string::npos ? HB_ERR_HIP : HB_ERR_LIMIT), e);
        if ((rc = keep_owned(c, &csr.d))) return rc;
        const uint64_t nn = c->g.ids.size();
        const uint64_t m_eff = csr.d.d_row_ptr ? csr.d.m : (nn && c->g.row_ptr.size() == nn + 1 ? c->g.row_ptr[nn] : 0);
        const double ing = now_ms() - t0;
        rc = plan_and_upload(c, std::move(csr), m_eff);
        c->stats.ms_ingest = ing;
        c->stats.ingest_peak_bytes = peak;
        if (trace) std::fprintf(stderr, "[hb finalize] done after %.1f ms (plan %.1f ms, state %.1f ms)\n", now_ms() - t0, c->stats.ms_plan, c->stats.ms_h2d);
        return rc;
    });
}

int hb_discard_appended(hb_ctx *c)
{
    return guarded(c, [&]() -> int {
        if (!c) return HB_ERR_INVALID;
        int rc = set_device(c);
        if (rc) return rc;
        HB_HIP(hipStreamSynchronize(c->stream));
        c->app.free_all();
        std::vector<hb_edge>().swap(c->pending);
        return HB_OK;
    });
}

int hb_set_collectives(hb_ctx *c, const hb_collectives *ops)
{
    return guarded(c, [&]() -> int {
        if (!c) return HB_ERR_INVALID;
        if (c->comm) return fail(c, HB_ERR_INVALID, "hb_set_collectives: the context already has an RCCL communicator (create it with HB_FLAG_NO_RCCL)");
        if (c->loaded) return fail(c, HB_ERR_INVALID, "hb_set_collectives: set the collectives before the graph is loaded");
        c->coll_a2a = nullptr; // (hb_set_all_to_all comes after this call)
        if (!ops) {
            c->coll = hb_collectives{};
            return HB_OK;
        }
        if (!ops->all_reduce || !ops->all_gather || !ops->broadcast) return fail(c, HB_ERR_INVALID, "hb_set_collectives: all three functions are required");
        int rc = set_device(c);
        if (rc) return rc;
        if (!c->comm_stream) { // the merge / all-reduce / epilogue pipeline of the edge partition runs the exchange on its own stream
            HB_HIP(hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking));
            for (int i = 0; i < hb_ctx::kOverlap; i++) {
                HB_HIP(hipEventCreateWithFlags(&c->ov_merged[i], hipEventDisableTiming));
                HB_HIP(hipEventCreateWithFlags(&c->ov_reduced[i], hipEventDisableTiming));
            }
        }
        c->coll = *ops;
        return HB_OK;
    });
}

int hb_set_all_to_all(hb_ctx *c, int (*all_to_all)(void *user, const void *send, void *recv, uint64_t bytes_per_rank, void *stream))
{
    return guarded(c, [&]() -> int {
        if (!c) return HB_ERR_INVALID;
        if (c->comm) return fail(c, HB_ERR_INVALID, "hb_set_all_to_all: the context has an RCCL communicator and exchanges by itself (create it with HB_FLAG_NO_RCCL)");
        if (c->loaded) return fail(c, HB_ERR_INVALID, "hb_set_all_to_all: set it before the graph is loaded");
        if (all_to_all && !c->coll.all_reduce) return fail(c, HB_ERR_INVALID, "hb_set_all_to_all: call hb_set_collectives first (its `user` pointer is passed on)");
        c->coll_a2a = all_to_all;
        return HB_OK;
    });
}

int hb_debug_staged_copy(void *dst, const void *src, uint64_t bytes, int to_device, void *stream)
{
    hipError_t e = hipSuccess;
    if (bytes) e = hipMemcpyAsync(dst, src, bytes, to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) (void)hipGetLastError();
    return e == hipSuccess ? HB_OK : HB_ERR_HIP;
}

int hb_pinned_alloc(uint64_t bytes, void **out)
{
    if (!out) return HB_ERR_INVALID;
    *out = nullptr;
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? (size_t)bytes : 1, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return HB_ERR_NOMEM;
    }
    *out = p;
    return HB_OK;
}

void hb_pinned_free(void *p)
{
    if (p) (void)hipHostFree(p);
}

int hb_debug_h2d_rate(hb_ctx *c, const void *host, uint64_t bytes, int reps, double *gb_per_s)
{
    return guarded(c, [&]() -> int {
        if (!c || !host || !bytes || reps < 1 || !gb_per_s) return HB_ERR_INVALID;
        int rc = set_device(c);
        if (rc) return rc;
        DevPtr<uint8_t> d;
        HB_HIP(d.alloc(bytes));
        HB_HIP_AS("hb_debug_h2d_rate: ", hipMemcpyAsync(d.get(), host, bytes, hipMemcpyHostToDevice, c->stream)); // warm-up (first touch of the mapping)
        HB_HIP_AS("hb_debug_h2d_rate: ", hipStreamSynchronize(c->stream));
        const double t0 = now_ms();
        for (int r = 0; r < reps; r++) HB_HIP_AS("hb_debug_h2d_rate: ", hipMemcpyAsync(d.get(), host, bytes, hipMemcpyHostToDevice, c->stream));
        HB_HIP_AS("hb_debug_h2d_rate: ", hipStreamSynchronize(c->stream));
        const double ms = now_ms() - t0;
        *gb_per_s = (double)bytes * reps / (ms * 1e-3) / 1e9;
        return HB_OK;
    });
}

int hb_debug_set_ingest_limits(hb_ctx *c, uint64_t max_records, uint64_t max_device_bytes, uint64_t chunk_records)
{
    if (!c) return HB_ERR_INVALID;
    c->lim_records = max_records;
    c->lim_bytes = max_device_bytes;
    c->lim_chunk = chunk_records;
    return HB_OK;
}

int hb_append_tail_edges(hb_ctx *c, const hb_edge *records, uint64_t count)
{
    return guarded(c, [&]() -> int {
        if (!c) return HB_ERR_INVALID;
        if (!ref_tail(c)) return fail(c, HB_ERR_INVALID, "tail records: create the context with HB_FLAG_REFERENCE_TAIL");
        if (!c->loaded) return fail(c, HB_ERR_INVALID, "tail records: load the graph first");
        if (count && !records) return fail(c, HB_ERR_INVALID, "records == NULL with count > 0");
        int rc = set_device(c);
        if (rc) return rc;
        if ((rc = need_host_dev_of(c))) return rc;
        if (!c->tail_index && count) c->tail_index = tail_index_build(c->g.ids.data(), c->g.ids.size());
        if (!c->tail_index && count) return fail(c, HB_ERR_NOMEM, "out of host memory indexing the node ids");
        const std::string e = tail_collect(c->tail_index, c->g.ids.size(), records, count, &c->tail_open);
        if (!e.empty()) return fail(c, HB_ERR_NOMEM, e);
        c->tail_dirty = true;
        return HB_OK;
    });
}

int hb_tail_segment_end(hb_ctx *c)
{
    return guarded(c, [&]() -> int {
        if (!c) return HB_ERR_INVALID;
        if (!ref_tail(c)) return fail(c, HB_ERR_INVALID, "tail records: create the context with HB_FLAG_REFERENCE_TAIL");
        if (c->tail_open.empty()) return HB_OK;
        int rc = need_host_dev_of(c);
        if (rc) return rc;
        const std::string e = tail_close_segment(c->tail_index, c->g.ids.data(), c->plan.dev_of.data(), &c->tail_open, &c->tail_keys);
        if (!e.empty()) return fail(c, HB_ERR_NOMEM, e);
        c->tail_dirty = true;
        return HB_OK;
    });
}

int hb_load_tail_edges(hb_ctx *c, const hb_edge *records, uint64_t count)
{
    if (c && ref_tail(c) && c->loaded) {
        c->tail_keys.clear();
        c->tail_open.clear();
        c->tail_dirty = true;
    }
    return hb_append_tail_edges(c, records, count);
}

int hb_load_dense(hb_ctx *c, const hb_u128 *sorted_ids, uint64_t n, const uint64_t *row_ptr, const uint32_t *src,
                  uint64_t m_eff)
{
    return guarded(c, [&]() -> int {
        if (!c) return HB_ERR_INVALID;
        int rc = set_device(c);
        if (rc) return rc;
        c->stats = hb_stats{};
        HB_POOL_RESET_PEAK();
        double t0 = now_ms();
        std::string e = check_dense(sorted_ids, n, row_ptr, src, m_eff);
        if (!e.empty()) return fail(c, e.find("too many") != std::string::npos ? HB_ERR_LIMIT : HB_ERR_INVALID, e);
        const bool on_device = device_plan(c);
        const bool keep_host = !on_device || m_eff <= kKeepHostGraph; // host copies: host planner, hb_debug_copy_graph
        try {
            c->g.ids.assign(sorted_ids, sorted_ids + n);
            if (keep_host) {
                c->g.row_ptr.assign(row_ptr, row_ptr + n + 1);
                if (n == 0) c->g.row_ptr.assign(1, 0);
                c->g.src.assign(src, src + m_eff);
            } else {
                std::vector<uint64_t>().swap(c->g.row_ptr);
                std::vector<uint32_t>().swap(c->g.src);
            }
        } catch (const std::bad_alloc &) {
            return fail(c, HB_ERR_NOMEM, "out of host memory copying the graph");
        }
        c->g.m_input = m_eff;
        c->g.m_unique = m_eff;
        OwnedCsr csr;
        if (on_device && n) { // straight from the caller's arrays to the device: no host copy of a multi-GB CSR
            HB_HIP(hipMalloc((void **)&csr.d.d_row_ptr, (n + 1) * sizeof(uint64_t)));
            hipError_t he = hipMalloc((void **)&csr.d.d_src, std::max<uint64_t>(m_eff, 1) * sizeof(uint32_t));
            if (he == hipSuccess) he = hipMemcpyAsync(csr.d.d_row_ptr, row_ptr, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream);
            if (he == hipSuccess && m_eff) he = hipMemcpyAsync(csr.d.d_src, src, m_eff * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
            if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
            if (he != hipSuccess) // (one message and the out-of-memory code for whichever step failed)
                return fail(c, he == hipErrorOutOfMemory ? HB_ERR_NOMEM : HB_ERR_HIP, std::string("uploading the graph: ") + hipGetErrorString(he));
            csr.d.m = m_eff;
        }
        if ((rc = keep_owned(c, &csr.d))) return rc;
        const uint64_t m_local = csr.d.d_row_ptr ? csr.d.m : ((dest_mode(c) && n) ? c->g.row_ptr[n] : m_eff);
        double ing = now_ms() - t0;
        rc = plan_and_upload(c, std::move(csr), m_local);
        c->stats.ms_ingest = ing;
        return rc;
    });
}

// ---- compute ------------------------------------------------------------------------------
int hb_begin(hb_ctx *c)
{
    return guarded(c, [&]() -> int {
        if (!c) return HB_ERR_INVALID;
        if (!c->loaded) return fail(c, HB_ERR_INVALID, "hb_begin: no graph loaded");
        int rc = set_device(c);
        if (rc) return rc;
        const Plan &p = c->plan;
        if (p.n_pad * 4 >= 0xFFFFFFFFull) return fail(c, HB_ERR_LIMIT, "more than 2^30 nodes: init_kernel is one quad per node in one dispatch");
        if ((rc = refuse_stale_error(c, "hb_begin"))) return rc;
        if (packed_wire(c) && edge_partitioned(c) && c->coll.all_reduce && !c->coll_a2a)
            return fail(c, HB_ERR_INVALID, "hb_begin: HB_FLAG_PACKED_WIRE on the edge partition with caller collectives needs hb_set_all_to_all (the packed "
                                           "all-reduce is an all-to-all of slices, a local maximum and an all-gather)");
        // the rows are nobody's until the initial state is complete (an error return below leaves them so)
        c->rows = RowsOf::Nobody;
        c->run_open = false;
        c->tl_valid = c->tl_declined = false;
        // d_part needs no clearing: pass 0 is always dense, and a dense pass overwrites every partial without
        // reading it (hb_kernels.hip.h)
        HB_HIP(hipMemsetAsync(c->d_bits[0], 0, c->bits_words * 4, c->stream));
        HB_HIP(hipMemsetAsync(c->d_bits[1], 0, c->bits_words * 4, c->stream));
        if (c->d_sat) HB_HIP(hipMemsetAsync(c->d_sat, 0, c->bits_words * 4, c->stream)); // nothing is saturated yet: pass 0 gathers and overwrites every partial
        HB_HIP(hipMemsetAsync(c->d_counters, 0, ((size_t)c->max_passes + 1) * hbk::kCounterWords * sizeof(unsigned long long), c->stream));
        if (c->d_sparse_counts) HB_HIP(hipMemsetAsync(c->d_sparse_counts, 0, 64 * sizeof(unsigned int), c->stream));
        if (c->ksum_len > p.n_pad) // slice padding beyond the rows init_kernel writes (all-reduce mode)
            HB_HIP(hipMemsetAsync(c->d_ksum + p.n_pad, 0, (c->ksum_len - p.n_pad) * sizeof(double), c->stream));
        c->cur = 0;
        c->t = 0;
        c->lean_init = false;
        c->sat_out_sum = 0;
        c->early_now = c->last_dense_early = false;
        if (p.n_pad) {
            if (lean_pass0(c)) {
                // [r6] pass 0 produces the initial state itself (hb_kernels.hip.h PassParams::rd_init): hb_begin writes two bitmaps instead of
                // 88 bytes per node (C4: 8.7 GB, 3.3 ms of every run)
                hipLaunchKernelGGL(hbk::init_lean_kernel, dim3((unsigned)((p.n_pad + 255) / 256)), dim3(256), 0, c->stream, (const uint32_t *)c->d_sid_of, p.n_pad,
                                   c->d_bits[0], c->d_kdirty);
                HB_HIP(hipGetLastError());
                c->lean_init = true;
            } else if ((rc = launch_full_init(c))) {
                return rc;
            }
        }
        if (ref_tail(c)) {
            // harmonic.rs:221,228: U64BloomFilter::new(num_nodes, 0.05); threshold = sqrt(num_nodes).max(0).round()
            c->bloom_bits = bloom_num_bits(p.n, 0.05);
            c->ref_threshold = (uint64_t)std::round(std::max(std::sqrt((double)p.n), 0.0));
            if (!c->d_bloom) {
                if ((rc = dev_alloc(c, &c->d_bloom, (c->bloom_bits + 31) / 32 + 2))) return rc;
                if ((rc = dev_alloc(c, &c->d_bloom_ones, 2))) return rc;
                if ((rc = dev_alloc(c, &c->d_list, c->ref_threshold + 2))) return rc;
            }
            // the segment still open ends here; no records given: the forward-links query finds nothing (an empty index)
            if (!c->tail_open.empty() && (rc = hb_tail_segment_end(c))) return rc;
            if ((c->tail_dirty || !c->d_tail_ptr) && (rc = upload_tail_index(c))) return rc;
            c->exact_counting = c->exact_valid = c->stale = false;
        }
        HB_HIP(hipStreamSynchronize(c->stream));
        if (c->rs_stream) HB_HIP(hipStreamSynchronize(c->rs_stream)); // (a download of an abandoned run)
        c->rs.valid = false;
        c->rs.changed_since = 0;
        c->rs.stages = 0;
        c->t = 0;
        c->cur = 0;
        c->wire_bytes = 0;
        c->has_changes = true; // harmonic.rs:232
        c->last_changed = p.n;
        c->last_active = c->m_global;
        c->pending_local = false;
        c->pstats.clear();
        c->pending_times.clear();
        c->pipelined_passes = 0;
        c->tail_kernel_passes = 0;
        c->rows = RowsOf::HyperBall;
        c->run_open = true;
        c->image = Image::None;
        c->res_count = 0;
        return HB_OK;
    });
}

int hb_step_local(hb_ctx *c)
{
    return guarded(c, [&]() -> int {
        if (!c) return HB_ERR_INVALID;
        int rc = set_device(c);
        if (rc) return rc;
        return step_local(c);
    });
}

int hb_step_finish(hb_ctx *c, int *has_changes)
{
    return guarded(c, [&]() -> int {
        if (!c) return HB_ERR_INVALID;
        int rc = set_device(c);
        if (rc) return rc;
        return step_finish(c, has_changes);
    });
}

int hb_step(hb_ctx *c, int *has_changes)
{
    return guarded(c, [&]() -> int {
        if (!c) return HB_ERR_INVALID;
        int rc = set_device(c);
        if (rc) return rc;
        if (tail_kernel_ready(c)) { // the far tail: one single-workgroup launch runs the pass from work lists (hb_tail.hip.h)
            uint32_t ran = 0;
            if ((rc = tail_kernel_run(c, 1, &ran))) return rc;
            if (ran) {
                if (has_changes) *has_changes = c->has_changes ? 1 : 0;
                return HB_OK;
            }
        }
        if ((rc = step_local(c))) return rc;
        return step_finish(c, has_changes);
    });
}

int hb_finish(hb_ctx *c)
{
    return guarded(c, [&]() -> int {
        if (!c) return HB_ERR_INVALID;
        if (c->rows != RowsOf::HyperBall) return fail(c, HB_ERR_INVALID, "hb_finish: call hb_begin first");
        int rc = set_device(c);
        if (rc) return rc;
        const Plan &p = c->plan;
        double t0 = now_ms();
        if ((rc = ensure_initial_state(c))) return rc; // (hb_finish right behind hb_begin)
        if (linked(c) && p.n_pad) {
            // every rank ends with all Kahan sums: in-place all-gather of the owned slices
            HB_COLL(coll_all_gather(c, c->d_ksum + (uint64_t)c->opt.rank * c->slice_rows, c->d_ksum, c->slice_rows, ncclDouble, c->stream));
        }
        // normalize_centralities (harmonic.rs:178-195) on the device, in ascending-NodeID order;
        // norm_factor = (num_nodes - 1) as f64 (:229)
        const double norm = (double)(p.n ? p.n - 1 : 0);
        unsigned long long *cnt = c->d_counters + (size_t)c->max_passes * hbk::kCounterWords; // the spare slot
        HB_HIP(hipMemsetAsync(cnt, 0, hbk::kCounterWords * sizeof(unsigned long long), c->stream));
        bool shipped = false;
        if (p.n && c->rs.on && c->rs.valid) {
            // the bulk is already on the host (results_stage): what moved since follows as a (sid, value) list
            auto &rs = c->rs;
            HB_HIP(hipMemsetAsync(rs.d_count, 0, sizeof(unsigned long long), c->stream));
            // [r6] the list kernel does NOT wait for the last snapshot's download any more (C4: that copy - 794 MB, 14 ms - outlasts the four
            // sweep passes behind it by ~3 ms, and the kernel's 1.1 ms then came on top).  It rewrites out[sid] only for the entries it also
            // puts on the list, and the host applies the list AFTER the download has landed (hipEventSynchronize below): whichever of the
            // two values of such an entry the copy carried, the list's is the one that stays.  If the list overflows, out[] is shipped
            // whole behind the download instead.
            const unsigned blocks = grid_blocks(c, (p.n_pad + 2047) / 2048, 8);
            hipLaunchKernelGGL(hbk::results_sync_kernel, dim3(blocks), dim3(256), 0, c->stream, (const double *)c->d_ksum, rs.d_sent,
                               (const uint32_t *)c->d_cid_of, p.n_pad, norm, 0, c->d_out, rs.d_sid, rs.d_val, (unsigned long long)rs.cap, rs.d_count, cnt);
            HB_HIP(hipGetLastError());
            HB_HIP(hipMemcpyAsync(rs.h_count, rs.d_count, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
            HB_HIP(hipMemcpyAsync(c->h_counters, cnt, hbk::kCounterWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
            HB_HIP(hipStreamSynchronize(c->stream));
            const uint64_t moved = *rs.h_count;
            if (moved <= rs.cap) {
                if (moved) {
                    HB_HIP(hipMemcpyAsync(rs.h_sid, rs.d_sid, moved * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
                    HB_HIP(hipMemcpyAsync(rs.h_val, rs.d_val, moved * sizeof(double), hipMemcpyDeviceToHost, c->stream));
                    HB_HIP(hipStreamSynchronize(c->stream));
                }
                HB_HIP(hipEventSynchronize(c->rs_copied)); // the snapshot's download is over before the list is applied on top of it
                host_scatter_f64(c->h_out, rs.h_sid, rs.h_val, moved); // every sid occurs once: the shares are independent (hb_host.cpp, OpenMP team)
            } else { // more moved than the list holds: out[] on the device is complete anyway, ship it whole
                HB_HIP(hipStreamWaitEvent(c->stream, c->rs_copied, 0)); // (behind the snapshot's download: both write h_out)
                HB_HIP(hipMemcpyAsync(c->h_out, c->d_out, c->out_len * sizeof(double), hipMemcpyDeviceToHost, c->stream));
                HB_HIP(hipStreamSynchronize(c->stream));
            }
            shipped = true;
        }
        if (p.n && !shipped) {
            if (c->rs.on) {
                // no snapshot was taken (the loop ended before the policy asked for one): the compact image whole, from the same kernel
                // (all rows, no list; sent[] is rewritten - nobody reads it before the next run's first snapshot does the same)
                const unsigned blocks = grid_blocks(c, (p.n_pad + 2047) / 2048, 8);
                hipLaunchKernelGGL(hbk::results_sync_kernel, dim3(blocks), dim3(256), 0, c->stream, (const double *)c->d_ksum, c->rs.d_sent,
                                   (const uint32_t *)c->d_cid_of, p.n_pad, norm, 1, c->d_out, (uint32_t *)nullptr, (double *)nullptr, 0ull, c->rs.d_count, cnt);
            } else {
                unsigned blocks = grid_blocks(c, (p.n + 255) / 256, 8);
                hipLaunchKernelGGL(hbk::finish_kernel, dim3(blocks), dim3(256), 0, c->stream, (const double *)c->d_ksum,
                                   (const uint32_t *)c->d_dev_of, p.n, norm, c->d_out, cnt);
            }
            HB_HIP(hipGetLastError());
            HB_HIP(hipMemcpyAsync(c->h_out, c->d_out, c->out_len * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        }
        if (!shipped) {
            HB_HIP(hipMemcpyAsync(c->h_counters, cnt, hbk::kCounterWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
            HB_HIP(hipStreamSynchronize(c->stream));
        }
        if (std::getenv("HB_TRACE_RESULTS"))
            std::fprintf(stderr, "[hb results] hb_finish: entered at %.3f ms, done at %.3f ms (host clock); %u snapshots, list %llu\n", t0, now_ms(), c->rs.stages,
                         shipped ? (unsigned long long)*c->rs.h_count : 0ull);
        c->stats.pipelined_passes = c->pipelined_passes;
        c->stats.tail_kernel_passes = c->tail_kernel_passes;
        c->stats.result_stages = c->rs.stages;
        c->stats.result_list = shipped ? *c->rs.h_count : 0;
        c->rs.valid = false;
        c->res_count = 0;
        for (int s = 0; s < hbk::kStripes; s++) c->res_count += c->h_counters[4 * s];
        c->stats.ms_d2h = now_ms() - t0;
        c->stats.results = c->res_count;
        c->stats.passes = c->t;
        if ((rc = resolve_pass_times(c))) return rc;
        double g = 0, coll = 0;
        for (auto &ps : c->pstats) { g += ps.ms_gpu; coll += ps.ms_collective; }
        c->stats.ms_loop_gpu = g;
        c->stats.ms_collective = coll;
        c->stats.wire_bytes = c->wire_bytes;
        c->run_open = false;
        c->image = Image::HyperBall;
        return HB_OK;
    });
}

int hb_run(hb_ctx *c, hb_stats *stats)
{
    return guarded(c, [&]() -> int {
        if (!c) return HB_ERR_INVALID;
        int rc = hb_begin(c);
        if (rc) return rc;
        double t0 = now_ms();
        int has = 1;
        const bool trace = std::getenv("HB_TRACE_RESULTS") != nullptr;
        // harmonic.rs:237-240: loop { if !has_changes { break } ... }
        while (has) {
            if (tail_kernel_ready(c)) { // passes from work lists, several per launch, until the loop ends or the changed set outgrows the lists
                uint32_t ran = 0;
                if ((rc = tail_kernel_run(c, 64, &ran))) return rc;
                has = c->has_changes ? 1 : 0;
                if (ran) continue;
            }
            if (tail_pipeline_ready(c)) {
                if ((rc = tail_pipeline(c, &has))) return rc; // runs passes until the loop ends or the changed set grows again
                continue;
            }
            if ((rc = hb_step(c, &has))) return rc;
            if (trace) std::fprintf(stderr, "[hb results] pass %llu returned at %.3f ms (host clock)\n", (unsigned long long)c->t - 1, now_ms());
        }
        c->stats.ms_loop = now_ms() - t0;
        if ((rc = hb_finish(c))) return rc;
        if (stats) *stats = c->stats;
        return HB_OK;
    });
}

int hb_get_stats(const hb_ctx *c, hb_stats *out)
{
    if (!c || !out) return HB_ERR_INVALID;
    *out = c->stats;
    out->passes = c->t;
    return HB_OK;
}

int hb_get_pass_stats(const hb_ctx *cc, uint64_t t, hb_pass_stats *out)
{
    if (!cc || !out || t >= cc->pstats.size()) return HB_ERR_INVALID;
    if (!cc->pending_times.empty()) {
        // timing events left in flight by a pass whose host round trip sits in its middle (destination partition + changed-only on a
        // communicator): read now, on the context's device and under the guard like every other call that talks to the runtime
        // (hb_finish resolves them too, so this only happens between hb_step calls)
        hb_ctx *c = const_cast<hb_ctx *>(cc);
        const int rc = guarded(c, [&]() -> int {
            const int rc_dev = set_device(c);
            return rc_dev ? rc_dev : resolve_pass_times(c);
        });
        if (rc) return rc;
    }
    *out = cc->pstats[t];
    return HB_OK;
}

// ---- results ------------------------------------------------------------------------------
int hb_result_count(hb_ctx *c, uint64_t *count)
{
    return guarded(c, [&]() -> int {
        if (!c || !count) return HB_ERR_INVALID;
        if (c->image == Image::None) return fail(c, HB_ERR_INVALID, "no results: hb_run / hb_finish not called");
        *count = c->res_count;
        return HB_OK;
    });
}

int hb_result_copy(hb_ctx *c, hb_u128 *ids, double *vals, uint64_t cap)
{
    return guarded(c, [&]() -> int {
        if (!c) return HB_ERR_INVALID;
        if (c->image == Image::None) return fail(c, HB_ERR_INVALID, "no results: hb_run / hb_finish not called");
        // compaction of the per-node array (absent = negative) into the caller's buffers, on the host cores the process may use
        // (C4: 99 M nodes -> 79 M results = 1.9 GB written; one thread took 1.3 s of the 15 s chain store -> load -> run -> store)
        host_compact_results(c->h_out, c->g.ids.data(), c->plan.n, ids, vals, cap, c->h_in_bits.empty() ? nullptr : c->h_in_bits.data());
        return HB_OK;
    });
}

int hb_result_ranks(hb_ctx *c, uint64_t *ranks, uint64_t cap)
{
    return guarded(c, [&]() -> int {
        if (!c || (cap && !ranks)) return HB_ERR_INVALID;
        if (c->image == Image::None) return fail(c, HB_ERR_INVALID, "no results: hb_run / hb_finish not called");
        if (cap < c->res_count) return fail(c, HB_ERR_INVALID, "hb_result_ranks: cap < hb_result_count");
        int rc = set_device(c);
        if (rc) return rc;
        std::string e = gpu_rank_results((void *)c->stream, c->d_out, c->out_len, c->res_count, ranks); // (the compact image keeps NodeID order: same ranks)
        if (!e.empty()) return fail(c, HB_ERR_HIP, e);
        return HB_OK;
    });
}

int hb_result_top(hb_ctx *c, uint64_t k, hb_u128 *ids, double *vals, uint64_t *written)
{
    return guarded(c, [&]() -> int {
        if (!c) return HB_ERR_INVALID;
        if (c->image == Image::None) return fail(c, HB_ERR_INVALID, "no results: hb_run / hb_finish not called");
        int rc = set_device(c);
        if (rc) return rc;
        const uint64_t top = std::min<uint64_t>(k, c->res_count);
        if (written) *written = top;
        if (!top || (!ids && !vals)) return HB_OK;
        std::vector<uint64_t> order(top);
        std::string e = gpu_rank_results((void *)c->stream, c->d_out, c->out_len, c->res_count, nullptr, order.data(), top);
        if (!e.empty()) return fail(c, HB_ERR_HIP, e);
        // result index (ascending NodeID among the kept ones) -> (sid, index into the image); compact image: the k-th set bit of h_in_bits
        std::vector<uint32_t> kept, at;
        kept.reserve(c->res_count);
        const bool compact = !c->h_in_bits.empty();
        if (compact) at.reserve(c->res_count);
        uint64_t cid = 0;
        for (uint64_t sid = 0; sid < c->plan.n; sid++) {
            if (compact && !((c->h_in_bits[sid >> 6] >> (sid & 63u)) & 1ull)) continue;
            const uint64_t pos = compact ? cid++ : sid;
            if (c->h_out[pos] >= 0.0) {
                kept.push_back((uint32_t)sid);
                if (compact) at.push_back((uint32_t)pos);
            }
        }
        if (kept.size() != c->res_count) return fail(c, HB_ERR_INVALID, "hb_result_top: result buffer changed since hb_finish");
        for (uint64_t i = 0; i < top; i++) {
            const uint32_t sid = kept[order[i]];
            if (ids) ids[i] = c->g.ids[sid];
            if (vals) vals[i] = c->h_out[compact ? at[order[i]] : sid];
        }
        return HB_OK;
    });
}

// store_harmonic (centrality/mod.rs:72-114) straight from the context that computed the results [ABI 5]
int hb_store_harmonic_results(hb_ctx *c, const char *output, char *err, uint64_t err_len)
{
    if (err && err_len) err[0] = 0;
    const int rc = guarded(c, [&]() -> int {
        if (!c || !output || !*output) return c ? fail(c, HB_ERR_INVALID, "hb_store_harmonic_results: output is empty") : HB_ERR_INVALID;
        if (c->image == Image::None) return fail(c, HB_ERR_INVALID, "no results: hb_run / hb_finish not called");
        int rc2 = set_device(c);
        if (rc2) return rc2;
        const uint64_t k = c->res_count;
        // the (NodeID, f64) list and the ranks, as hb_result_copy / hb_result_ranks return them
        RawVec<hb_u128> ids(k); // (uninitialised: hb_result_copy fills them on all host cores, the ranks come off the device)
        RawVec<double> vals(k);
        RawVec<uint64_t> ranks(k);
        const bool trace = std::getenv("HB_TRACE_STORE") != nullptr;
        double t_lap = now_ms();
        auto lap = [&](const char *what) {
            if (trace) std::fprintf(stderr, "[hb store] %-28s %8.3f s\n", what, (now_ms() - t_lap) * 1e-3);
            t_lap = now_ms();
        };
        if ((rc2 = hb_result_copy(c, ids.data(), vals.data(), k))) return rc2;
        lap("result list (host cores)");
        if ((rc2 = hb_result_ranks(c, ranks.data(), k))) return rc2;
        lap("ranks (device sort)");
        // the key order of both databases: one radix sort on the device instead of a comparison sort of 24-byte records on the host
        StoreKeyVec sorted(k);
        const std::string e = gpu_store_keys((void *)c->stream, ids.data(), k, sorted.data());
        if (!e.empty()) return fail(c, e.find("memory") != std::string::npos ? HB_ERR_NOMEM : HB_ERR_HIP, "hb_store_harmonic_results: " + e);
        lap("key order (device sort)");
        RawVec<hb_u128>().swap(ids);
        char msg[512] = {0};
        const int rc3 = store_harmonic_presorted(output, &sorted, vals.data(), ranks.data(), msg, sizeof(msg));
        if (rc3) return fail(c, rc3, msg);
        return HB_OK;
    });
    if (rc && err && err_len && c) std::snprintf(err, (size_t)err_len, "%s", c->err.c_str());
    return rc;
}

#include "hb_api_debug.inc"

} // extern "C"

#include "hb_api_walk.inc"

#include "hb_api_sample.inc"

#include "hb_api_distance.inc"

#include "hb_api_betweenness.inc"

#include "hb_api_nearest_seed.inc"

#include "hb_api_links.inc"
#include "hb_api_similarity.inc" // (after the links: the limited mode builds its cut lists with their list builder)
#include "hb_api_similar.inc"
#include "hb_api_score.inc"
