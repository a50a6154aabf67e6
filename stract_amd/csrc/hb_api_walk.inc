// hb_api_walk.inc - part of the hb_api.hip translation unit (included before the operator files; uses its hb_ctx and helpers).
// What the operators share on the host: who holds the shared rows and the result image, their entry and its refusals, the virtual levels
// in order, the sources as sids, the row -> readers transpose; the entry of a reader, the result record of the node-valued operators
// (NodeResult: d_val_sid / d_flag_sid, the compacted d_sel_sid / d_sel_val, count, valid, compacted) with its allocation, compaction and
// three readers, the shared _top reader - and, for the operators that walk 64-byte rows (device side: hb_walk.hip.h), the launcher and
// one forward level.

namespace {

// ---- the four operators --------------------------------------------------------------------------------------------------------------
// The only place outside hb_begin that changes hb_ctx::rows (DESIGN.md section 18): an operator calls it immediately before its first
// write to d_regs / d_part / d_bits / the touch bitmap / the sweep scratch, so an error return after that never leaves its rows marked
// as HyperBall state for hb_step, hb_finish or the debug exports.  The tail kernel's lists describe the bitmaps no longer.
void claim_rows(hb_ctx *c, RowsOf who)
{
    c->rows = who;
    c->tl_valid = false;
}

// the result image (d_out / h_out / res_count) is about to be rewritten by somebody who is not hb_finish: no result snapshot of an earlier
// run may still be landing in h_out, and nothing is served from it until the writer says what it holds
int take_image(hb_ctx *c)
{
    if (c->rs_stream) HB_HIP(hipStreamSynchronize(c->rs_stream));
    c->rs.valid = false;
    c->image = Image::None;
    return HB_OK;
}

// The entry of hb_sampled_harmonic, hb_distances, hb_betweenness and hb_inbound_similarity: the context's device, then what each of them
// refuses before it looks at its options - an open run (between hb_begin and hb_finish the HyperBall state, the pinned counter words, the
// stream's event pair and a result snapshot on its way to h_out belong to that run), more than one rank, no graph, a plan whose node rows
// or virtual levels do not begin on a 32-row word or lie outside [n_pad, n_pad + nv] (the planner produces neither), an unchecked HIP error
// of an earlier call - then the body
template <class BODY>
int operator_entry(hb_ctx *c, const char *who, BODY body, const char *boundary_note = " (virtual level boundary)")
{
    return guarded(c, [&]() -> int {
        if (!c) return HB_ERR_INVALID;
        int rc = set_device(c);
        if (rc) return rc;
        if (c->run_open) return fail(c, HB_ERR_INVALID, std::string(who) + ": a HyperBall run is in progress (hb_begin without hb_finish)");
        if (multi_rank(c)) return fail(c, HB_ERR_INVALID, std::string(who) + ": single rank only (world_size > 1)");
        if (!c->loaded) return fail(c, HB_ERR_INVALID, std::string(who) + ": no graph loaded");
        if ((rc = plan_rows_word_aligned(c, who))) return rc;
        for (uint64_t b : c->plan.level_begin)
            if (b < c->plan.n_pad || b > c->plan.n_pad + c->plan.nv) return fail(c, HB_ERR_INVALID, std::string(who) + ": unexpected plan layout" + boundary_note);
        if ((rc = refuse_stale_error(c, who))) return rc;
        return body();
    });
}

// The virtual levels of the plan in order, fn(lo, hi) for every level that has rows.  The order is part of each caller's correctness: a
// chunk row feeds the higher levels (and its hub), so values that flow from the sources to the readers need `ascending`, values that
// flow from a hub down its chunk tree need the highest level first.
template <class FN>
void for_each_virtual_level(const Plan &p, bool ascending, FN fn)
{
    const size_t nlev = p.level_begin.size() > 1 ? p.level_begin.size() - 1 : 0;
    for (size_t k = 0; k < nlev; k++) {
        const size_t l = ascending ? k : nlev - 1 - k;
        if (p.level_begin[l + 1] > p.level_begin[l]) fn(p.level_begin[l], p.level_begin[l + 1]);
    }
}

// NodeIDs -> the distinct sids among them, ascending; *unknown = ids that are no node of the graph, *first_unknown = the first such index
void resolve_sources(const hb_ctx *c, const hb_u128 *ids, uint64_t count, std::vector<uint32_t> *sids, uint64_t *unknown, uint64_t *first_unknown = nullptr)
{
    sids->clear();
    sids->reserve(count);
    *unknown = 0;
    for (uint64_t i = 0; i < count; i++) {
        uint32_t sid;
        if (find_sid(c, ids[i], &sid)) sids->push_back(sid);
        else if (!(*unknown)++ && first_unknown) *first_unknown = i;
    }
    std::sort(sids->begin(), sids->end());
    sids->erase(std::unique(sids->begin(), sids->end()), sids->end());
}

// The row -> readers transpose of the plan (GraphDeviceState::d_out_ptr / d_out_rows): the sweep passes' when the context has sweep
// support (sparse_ok); else (HB_FLAG_NO_SPARSE, unfused passes) built here at the first call of hb_distances / hb_betweenness after a
// load, and counted in that call's device bytes.  The pointers are set only once the transpose is complete; sparse_ok, not they, says
// whether the sweep support exists.
int ensure_transpose(hb_ctx *c, const char *who)
{
    if (c->d_out_ptr) return HB_OK;
    const uint64_t rows_total = c->plan.n_pad + c->plan.nv;
    uint64_t *op = nullptr;
    uint32_t *orow = nullptr;
    int rc;
    if ((rc = dev_alloc(c, &op, rows_total + 1))) return rc;
    if ((rc = dev_alloc(c, &orow, c->plan_entries))) return rc;
    const std::string e = gpu_transpose_rows((void *)c->stream, c->d_row_ptr, c->d_src, rows_total, c->plan_entries, op, orow);
    if (!e.empty()) return fail(c, e.find("out of memory") != std::string::npos ? HB_ERR_NOMEM : HB_ERR_HIP, std::string(who) + ": " + e);
    c->d_out_ptr = op;
    c->d_out_rows = orow;
    return HB_OK;
}

// ---- results and their readers --------------------------------------------------------------------------------------------------------
// a result is there to be read: `missing` = what to say when it is not
int result_ready(hb_ctx *c, bool valid, const char *who, const char *missing)
{
    if (!c->loaded || !valid) return fail(c, HB_ERR_INVALID, std::string(who) + ": " + missing);
    return set_device(c);
}

// The entry of a reader or a debug export of an operator's result: the context, `zeroed` (an output that is 0 whatever happens: the
// _top readers' *written), that the result is there - callers write `valid` as `c && c->x.valid` -, then the body.  A reader that tests
// an argument BEFORE the result (result_count, result_all, hb_similarity_lookup) keeps its own order and does not come through here
template <class BODY>
int reader_entry(hb_ctx *c, bool valid, const char *who, const char *missing, BODY body, uint64_t *zeroed = nullptr)
{
    return guarded(c, [&]() -> int {
        if (!c) return HB_ERR_INVALID;
        if (zeroed) *zeroed = 0;
        const int rc = result_ready(c, valid, who, missing);
        return rc ? rc : body();
    });
}

// hb_*_count: the number of entries of a compacted result
int result_count(hb_ctx *c, bool valid, const char *who, const char *missing, uint64_t *count, uint64_t value)
{
    if (!count) return fail(c, HB_ERR_INVALID, std::string(who) + ": count == NULL");
    const int rc = result_ready(c, valid, who, missing);
    if (!rc) *count = value;
    return rc;
}

// hb_*_all: one value per node in sid order, from d_val_sid (`prepare`, if given, fills it first); `arg` = the caller's name of `out`
template <class T>
int result_all(hb_ctx *c, bool valid, const char *who, const char *arg, const char *missing, T *out, uint64_t cap, const T *d_val_sid, int (*prepare)(hb_ctx *) = nullptr)
{
    if (!out) return fail(c, HB_ERR_INVALID, std::string(who) + ": " + arg + " == NULL");
    int rc = result_ready(c, valid, who, missing);
    if (rc) return rc;
    const uint64_t n = c->plan.n;
    if (cap < n) return fail(c, HB_ERR_INVALID, std::string(who) + ": cap < n");
    if (!n) return HB_OK;
    if (prepare && (rc = prepare(c))) return rc;
    HB_HIP(hipMemcpyAsync(out, d_val_sid, n * sizeof(T), hipMemcpyDeviceToHost, c->stream));
    HB_HIP(hipStreamSynchronize(c->stream));
    return HB_OK;
}

// the ids of a compacted result: only its k sids come down, the ids are looked up in the host's sorted id array
int copy_selected_ids(hb_ctx *c, const uint32_t *d_sel_sid, uint64_t k, hb_u128 *ids)
{
    std::vector<uint32_t> sid(k);
    HB_HIP(hipMemcpyAsync(sid.data(), d_sel_sid, k * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HB_HIP(hipStreamSynchronize(c->stream));
    for (uint64_t i = 0; i < k; i++) ids[i] = c->g.ids[sid[i]];
    return HB_OK;
}

// ---- the node-valued operators' result (NodeResult, hb_api.hip): hb_distances, hb_betweenness, hb_nearest_seed --------------------------
// its buffers, once per loaded graph, on the context's `allocs` list (the caller's `bytes` count and hb_stats.device_bytes see them)
template <class T>
int node_result_alloc(hb_ctx *c, NodeResult<T> &r)
{
    const uint64_t n = c->plan.n;
    int rc;
    constexpr bool own = !NodeResult<T>::kBytes; // flags and selected values have buffers of their own
    if ((rc = dev_alloc(c, &r.d_val_sid, n))) return rc;
    if constexpr (own) rc = dev_alloc(c, &r.d_flag_sid, n);
    else r.d_flag_sid = r.d_val_sid;
    if (rc || (rc = dev_alloc(c, &r.d_sel_sid, n)) || (rc = dev_alloc(c, &r.d_sel_flag, n))) return rc;
    if constexpr (own) rc = dev_alloc(c, &r.d_sel_val, n);
    else r.d_sel_val = r.d_sel_flag;
    return rc ? rc : dev_alloc(c, &r.d_sel_cnt, 8);
}

// The compacted form of d_val_sid / d_flag_sid: the select, its count read back, the check against the operator's own count (`expect`;
// `counters` = what the refusal calls its source), the gather of the selected values, and the stream drained.  Sets count and compacted
template <class T>
int node_result_compact(hb_ctx *c, NodeResult<T> &r, const char *who, const uint64_t *expect = nullptr, const char *counters = "counters")
{
    const std::string e = gpu_select_reached((void *)c->stream, r.d_flag_sid, c->plan.n, r.d_sel_sid, r.d_sel_flag, r.d_sel_cnt);
    if (!e.empty()) return fail(c, HB_ERR_HIP, std::string(who) + ": " + e);
    uint64_t got = 0;
    HB_HIP(hipMemcpyAsync(&got, r.d_sel_cnt, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HB_HIP(hipStreamSynchronize(c->stream));
    if (expect && got != *expect) return fail(c, HB_ERR_INVALID, std::string(who) + ": the compacted list and the " + counters + " disagree");
    if constexpr (!NodeResult<T>::kBytes) {
        if (got) {
            hipLaunchKernelGGL(hbk::gather_selected_kernel, dim3(grid_blocks(c, (got + 255) / 256, 8, 1)), dim3(256), 0, c->stream, (const T *)r.d_val_sid,
                               (const uint32_t *)r.d_sel_sid, got, r.d_sel_val);
            HB_HIP(hipGetLastError());
            HB_HIP(hipStreamSynchronize(c->stream));
        }
    }
    r.count = got;
    r.compacted = true;
    return HB_OK;
}

// hb_*_count / _copy / _all of such a result.  `r` = the record of a non-NULL context (callers: c ? &c->x.res : nullptr); `compact`, if
// given, makes d_val_sid and the compacted list when the first reader needs them (the distances) - after every refusal and only when
// something is to be copied
template <class T>
int node_result_count(hb_ctx *c, const NodeResult<T> *r, const char *who, const char *missing, uint64_t *count)
{
    return guarded(c, [&]() -> int {
        if (!c) return HB_ERR_INVALID;
        return result_count(c, r->valid, who, missing, count, r->count);
    });
}

template <class T>
int node_result_copy(hb_ctx *c, const NodeResult<T> *r, const char *who, const char *missing, hb_u128 *ids, T *vals, uint64_t cap, int (*compact)(hb_ctx *) = nullptr)
{
    return reader_entry(c, r && r->valid, who, missing, [&]() -> int {
        const uint64_t k = std::min<uint64_t>(cap, r->count);
        if (!k || (!ids && !vals)) return HB_OK;
        int rc;
        if (compact && (rc = compact(c))) return rc;
        // only the entries come down: k sids and k values
        if (ids && (rc = copy_selected_ids(c, r->d_sel_sid, k, ids))) return rc;
        if (vals) {
            HB_HIP(hipMemcpyAsync(vals, r->d_sel_val, k * sizeof(T), hipMemcpyDeviceToHost, c->stream));
            HB_HIP(hipStreamSynchronize(c->stream));
        }
        return HB_OK;
    });
}

template <class T>
int node_result_all(hb_ctx *c, const NodeResult<T> *r, const char *who, const char *arg, const char *missing, T *out, uint64_t cap, int (*compact)(hb_ctx *) = nullptr)
{
    return guarded(c, [&]() -> int {
        if (!c) return HB_ERR_INVALID;
        return result_all<T>(c, r->valid, who, arg, missing, out, cap, r->d_val_sid, compact);
    });
}

// What hb_nearest_seed_top and hb_similarity_top do once their keys kernel has run: the first `top` entries of d_key (over the entries
// whose d_keep byte is set) in the order key descending, ties by entry descending; an entry is sid_of_entry(at), its value the key's bits
template <class SID>
int result_top(hb_ctx *c, const char *who, const uint64_t *d_key, const uint8_t *d_keep, uint64_t n, uint64_t top, SID sid_of_entry, hb_u128 *ids, double *vals,
               uint64_t *written)
{
    std::vector<uint32_t> at(top);
    std::vector<uint64_t> key(top);
    uint64_t got = 0;
    const std::string e = gpu_similarity_top((void *)c->stream, d_key, d_keep, n, top, at.data(), key.data(), &got);
    if (!e.empty()) return fail(c, e.find("out of memory") != std::string::npos ? HB_ERR_NOMEM : HB_ERR_HIP, std::string(who) + ": " + e);
    for (uint64_t i = 0; i < got; i++) {
        if (ids) ids[i] = c->g.ids[sid_of_entry(at[i])];
        if (vals) std::memcpy(&vals[i], &key[i], sizeof(double));
    }
    if (written) *written = got;
    return HB_OK;
}

// ---- the walks over 64-byte rows (hb_walk.hip.h) -------------------------------------------------------------------------------------
// A kernel family: its parameter struct and its six instances.  walk_kernel is the only place that names one.
struct SampleWalk {
    using Params = hbk::SampleParams;
    template <bool REAL, int MODE>
    static constexpr void (*kernel)(const Params) = hbk::sample_level_kernel<REAL, MODE>;
};
struct BrandesWalk {
    using Params = hbk::BcParams;
    template <bool REAL, int MODE>
    static constexpr void (*kernel)(const Params) = hbk::bc_forward_kernel<REAL, MODE>;
};

struct SimilarityWalk {
    using Params = hbk::SimParams;
    template <bool REAL, int MODE>
    static constexpr void (*kernel)(const Params) = hbk::sim_count_kernel<REAL, MODE>;
};

template <class W, bool REAL>
auto walk_kernel_of(hbk::PassMode mode) -> void (*)(const typename W::Params)
{
    if (mode == hbk::kModeDense) return W::template kernel<REAL, hbk::kModeDense>;
    if (mode == hbk::kModeBitmap) return W::template kernel<REAL, hbk::kModeBitmap>;
    return W::template kernel<REAL, hbk::kModeSweep>;
}
template <class W>
auto walk_kernel(bool real, hbk::PassMode mode) -> void (*)(const typename W::Params)
{
    return real ? walk_kernel_of<W, true>(mode) : walk_kernel_of<W, false>(mode);
}

// launch shape of one level: a wave per 32-row word, grid-stride; XCD-affine groups for the first hub-chunk level (as hb_run's dense pass)
template <class W>
void launch_walk(hb_ctx *c, const typename W::Params &wp, bool real, hbk::PassMode mode)
{
    const uint64_t words = (wp.row_hi - wp.row_lo + 31) / 32;
    if (!words) return;
    uint64_t blocks = std::min<uint64_t>((words + 3) / 4, (uint64_t)c->num_cu * 8);
    if (wp.xcd_map) blocks = std::max<uint64_t>((blocks + 7) / 8 * 8, 8);
    hipLaunchKernelGGL(walk_kernel<W>(real, mode), dim3((unsigned)blocks), dim3(256), 0, c->stream, wp);
}

// the first hub-chunk level may run as eight XCD-affine groups: the planner cut it into eight word-aligned groups
bool walk_xcd_ok(const Plan &p)
{
    return p.xcd_groups == 8 && p.level_begin.size() > 1 && p.xcd_begin[0] == p.level_begin[0] && p.xcd_begin[8] == p.level_begin[1] &&
           std::all_of(p.xcd_begin, p.xcd_begin + 9, [](uint64_t b) { return b % 32 == 0; });
}

// what a walk's parameters say about the loaded graph (the rest - buffers, bitmaps, counters, rows - changes per level)
void fill_walk_params(const hb_ctx *c, hbk::WalkParams *wp)
{
    const Plan &p = c->plan;
    wp->row_ptr = c->d_row_ptr;
    wp->src = c->d_src;
    wp->touch = c->d_touch;
    wp->out_ptr = c->d_out_ptr;
    wp->out_rows = c->d_out_rows;
    wp->outdeg = c->d_outdeg;
    wp->n_pad = p.n_pad;
    wp->rows_total = p.n_pad + p.nv;
    for (int x = 0; x < 8; x++) {
        wp->xcd_lo[x] = p.xcd_begin[x];
        wp->xcd_hi[x] = p.xcd_begin[x + 1];
    }
}

struct WalkLevel {
    unsigned long long cnt[4]; // the level's counters (WalkParams::cnt)
    float ms;
};

// One forward level d of a walk, timed: `wp` (the WalkParams of the parameters `launch(real)` launches with) holds this level's bits_rd /
// bits_wr / cnt; last_changed = node rows whose bit was set at d - 1.  Sweep: those rows -> touch bits of their readers first (hb_run's
// seed / expand kernels, unchanged).  Then the virtual levels - partials of level d from the rows of level d - 1 -, then the node rows.
template <class LAUNCH>
int walk_forward_level(hb_ctx *c, hbk::WalkParams &wp, hbk::PassMode mode, uint64_t last_changed, LAUNCH launch, WalkLevel *out)
{
    const Plan &p = c->plan;
    HB_HIP(hipEventRecord(c->ev[kEvStart], c->stream));
    if (mode == hbk::kModeSweep) {
        hbk::PassParams seed_pp{}; // (all the seeding kernels read of it)
        seed_pp.bits_rd = wp.bits_rd;
        seed_pp.n_pad = wp.n_pad;
        seed_pp.rows_total = wp.rows_total;
        HB_HIP(hipMemsetAsync(c->d_sparse_counts, 0, 4 * sizeof(unsigned int), c->stream));
        launch_sweep_seeding(c, make_sweep_params(c, seed_pp, 0, nullptr), last_changed <= 4096);
        HB_HIP(hipGetLastError());
    }
    const bool xcd = mode == hbk::kModeDense && walk_xcd_ok(p);
    for_each_virtual_level(p, true, [&](uint64_t lo, uint64_t hi) { // ascending: a level's partials are built from the levels below it
        wp.row_lo = lo;
        wp.row_hi = hi;
        wp.xcd_map = (xcd && lo == p.xcd_begin[0] && hi == p.xcd_begin[8]) ? 1 : 0; // (the first hub-chunk level, walk_xcd_ok)
        launch(false);
    });
    wp.xcd_map = 0;
    wp.row_lo = 0;
    wp.row_hi = p.n_pad;
    launch(true);
    HB_HIP(hipGetLastError());
    HB_HIP(hipEventRecord(c->ev[kEvEnd], c->stream));
    unsigned long long *h = c->h_counters; // (pinned words of the context; hb_run rewrites them before it reads them)
    HB_HIP(hipMemcpyAsync(h, wp.cnt, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HB_HIP(hipStreamSynchronize(c->stream));
    HB_HIP(hipEventElapsedTime(&out->ms, c->ev[kEvStart], c->ev[kEvEnd]));
    std::copy(h, h + 4, out->cnt);
    return HB_OK;
}

} // namespace
