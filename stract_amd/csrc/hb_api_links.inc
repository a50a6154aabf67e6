// hb_api_links.inc - part of the hb_api.hip translation unit (included at its end; uses its hb_ctx and helpers).
// hb_links_set_keys / hb_backlinks: HostBacklinksQuery::new(node).with_limit(EdgeLimit::Limit(L)) (webgraph/query/backlink.rs:230-360)
// for a list of hosts per call - the L best in-neighbours of every queried host in the order (key, NodeID), by a radix select on a dense
// order that stays on the device between calls (kernels: hb_links.hip.h) - and hb_forwardlinks, HostForwardlinksQuery .. Limit(L)
// (webgraph/query/forwardlink.rs:183-330), the same for the out-neighbours.  Definitions: include/hyperball.h.  Like hb_distances and
// hb_nearest_seed the operator borrows nothing: no claim_rows, no take_image; every buffer is its own (GraphDeviceState::lnk).

namespace {

constexpr uint64_t kLinksDefaultSlots = 1024, kLinksMaxSlots = 65536;

// the virtual levels of the plan; a plan with more than the list builder's 64 level counters can follow is refused
int links_levels(hb_ctx *c, const std::string &who, size_t *nlev)
{
    *nlev = 0;
    for_each_virtual_level(c->plan, true, [&](uint64_t, uint64_t) { (*nlev)++; });
    if (*nlev + 2 > 64) return fail(c, HB_ERR_INVALID, who + ": unexpected plan layout (more than 62 virtual levels)");
    return HB_OK;
}

// A list of ids as the operators of this family want it: each distinct known node is looked up once, every entry that names it finds it
struct ResolvedIds {
    std::vector<uint32_t> distinct; // the distinct known sids, ascending
    std::vector<uint32_t> slot;     // per entry: its position in `distinct`, kNone = no node of the graph
    uint64_t unknown = 0;           // entries that are no node of the graph
};

ResolvedIds resolve_ids(const hb_ctx *c, const hb_u128 *ids, uint64_t count)
{
    ResolvedIds r;
    r.slot.resize(count);
    host_find_sids(c->g.ids.data(), c->plan.n, ids, count, r.slot.data()); // (the sids for now)
    for (uint32_t sid : r.slot)
        if (sid != kNone) r.distinct.push_back(sid);
    std::sort(r.distinct.begin(), r.distinct.end());
    r.distinct.erase(std::unique(r.distinct.begin(), r.distinct.end()), r.distinct.end());
    for (uint32_t &v : r.slot) {
        if (v == kNone) r.unknown++;
        else v = (uint32_t)(std::lower_bound(r.distinct.begin(), r.distinct.end(), v) - r.distinct.begin());
    }
    return r;
}

// ord / inv / ord_row from the keys in d_key (`sorted`: false = no key set, NodeID order)
int links_build_order(hb_ctx *c, bool sorted, double *ms)
{
    auto &s = c->lnk;
    const Plan &p = c->plan;
    const uint64_t n = p.n;
    DevPtr<uint64_t> d_order, d_rank;
    if (sorted) {
        if (d_order.alloc(n) != hipSuccess || d_rank.alloc(n) != hipSuccess) return fail(c, HB_ERR_NOMEM, "hb_links_set_keys: out of device memory for the sort");
    }
    if (const int rc = lap_start(c)) return rc;
    if (sorted) { // stable: equal keys keep ascending sid order, which is ascending NodeID order
        const std::string e = gpu_rank_keys_device((void *)c->stream, (const uint64_t *)s.d_key.get(), n, d_order.get(), d_rank.get());
        if (!e.empty()) return fail(c, e.find("memory") != std::string::npos ? HB_ERR_NOMEM : HB_ERR_HIP, "hb_links_set_keys: " + e);
    }
    hipLaunchKernelGGL(hbk::lk_ord_kernel, dim3(grid_blocks(c, (n + 255) / 256, 8, 1)), dim3(256), 0, c->stream, (const uint64_t *)d_rank.get(),
                       (const uint64_t *)d_order.get(), n, s.d_ord.get(), s.d_inv.get());
    hipLaunchKernelGGL(hbk::lk_ord_row_kernel, dim3(grid_blocks(c, (p.n_pad + 255) / 256, 8, 1)), dim3(256), 0, c->stream, (const uint32_t *)s.d_ord.get(),
                       (const uint32_t *)c->d_sid_of, p.n_pad, s.d_ord_row.get());
    HB_HIP(hipGetLastError());
    return lap(c, ms); // (drains the stream: the sort's buffers may go)
}

// the per-graph holders; a context that never saw hb_links_set_keys gets the order of "every key is u64::MAX"
int links_alloc(hb_ctx *c, bool default_order)
{
    auto &s = c->lnk;
    if (s.ready) return HB_OK;
    const Plan &p = c->plan;
    int rc;
    if ((rc = hold(c, s.bytes, s.d_key, p.n))) return rc;
    if ((rc = hold(c, s.bytes, s.d_ord, p.n))) return rc;
    if ((rc = hold(c, s.bytes, s.d_inv, p.n))) return rc;
    if ((rc = hold(c, s.bytes, s.d_ord_row, p.n_pad))) return rc;
    if (default_order) {
        HB_HIP(hipMemsetAsync(s.d_key.get(), 0xFF, p.n * sizeof(unsigned long long), c->stream));
        double ms = 0;
        if ((rc = links_build_order(c, false, &ms))) return rc;
    }
    s.ready = true;
    return HB_OK;
}

void similarity_limit_drop(hb_ctx *c); // hb_api_similarity.inc: the cut lists of the limited inbound similarity follow the key set

int links_set_keys(hb_ctx *c, const hb_links_key_options *opt_in, hb_links_key_stats *st_out)
{
    const double t0 = now_ms();
    hb_links_key_options o{};
    copy_in(opt_in, &o);
    // ---- refusals
    const bool from_ranks = (o.flags & HB_LINKS_KEYS_FROM_RANKS) != 0;
    if (from_ranks && (o.key_ids || o.keys || o.key_count)) return fail(c, HB_ERR_INVALID, "hb_links_set_keys: HB_LINKS_KEYS_FROM_RANKS together with a key list");
    if (o.key_count && (!o.key_ids || !o.keys)) return fail(c, HB_ERR_INVALID, "hb_links_set_keys: key_count without key_ids / keys");
    if (from_ranks && c->image == Image::None)
        return fail(c, HB_ERR_INVALID, "hb_links_set_keys: HB_LINKS_KEYS_FROM_RANKS without a live result (call hb_run or hb_sampled_harmonic)");
    const Plan &p = c->plan;
    const uint64_t n = p.n;
    auto &s = c->lnk;
    hb_links_key_stats st{};
    int rc;
    // ---- the keys by sid
    std::vector<unsigned long long> key(n, ~0ull);
    if (from_ranks) { // what hb_result_ranks reports, by the sid of the result (as hb_result_top finds it)
        std::vector<uint64_t> ranks(c->res_count);
        const std::string e = gpu_rank_results((void *)c->stream, c->d_out, c->out_len, c->res_count, ranks.data());
        if (!e.empty()) return fail(c, HB_ERR_HIP, "hb_links_set_keys: " + e);
        const bool compact = !c->h_in_bits.empty();
        uint64_t cid = 0, k = 0;
        for (uint64_t sid = 0; sid < n; sid++) {
            if (compact && !((c->h_in_bits[sid >> 6] >> (sid & 63u)) & 1ull)) continue;
            const uint64_t pos = compact ? cid++ : sid;
            if (c->h_out[pos] >= 0.0) {
                if (k >= ranks.size()) return fail(c, HB_ERR_INVALID, "hb_links_set_keys: result buffer changed since hb_finish");
                key[sid] = ranks[k++];
            }
        }
        if (k != c->res_count) return fail(c, HB_ERR_INVALID, "hb_links_set_keys: result buffer changed since hb_finish");
        st.listed = k;
    } else {
        std::vector<uint32_t> sids(o.key_count);
        std::vector<uint8_t> has(n, 0);
        host_find_sids(c->g.ids.data(), n, o.key_ids, o.key_count, sids.data());
        for (uint64_t i = 0; i < o.key_count; i++) {
            if (sids[i] == kNone) {
                st.unknown_keys++;
                continue;
            }
            key[sids[i]] = o.keys[i]; // (a duplicate: the last one wins)
            st.listed += has[sids[i]] ? 0 : 1;
            has[sids[i]] = 1;
        }
    }
    similarity_limit_drop(c); // (the order is about to change)
    if (n) {
        s.ready = false; // (an error below leaves no half-built order behind: the next call builds the default one)
        if ((rc = links_alloc(c, false))) return rc;
        s.ready = false;
        HB_HIP(hipMemcpyAsync(s.d_key.get(), key.data(), n * sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream));
        if ((rc = links_build_order(c, true, &st.ms_order))) return rc;
        s.ready = true;
    }
    st.device_bytes = s.bytes;
    st.ms_total = now_ms() - t0;
    copy_out(st_out, st);
    return HB_OK;
}

// hb_forwardlinks: the transpose (built here for a context without sweep support) and top_row, once per load.  A reader list names the
// chunk row an edge enters a hub's tree at; top_row[chunk row - n_pad] = the hub's node row.  One launch per virtual level from the
// highest down: a chunk row's single reader is its hub or a chunk row of a higher level.  A chunk row with a list and a reader count
// other than one (or a reader that is no higher level) is refused, not resolved.
int links_top_rows(hb_ctx *c, const std::string &who, double *ms)
{
    auto &s = c->lnk;
    const Plan &p = c->plan;
    int rc;
    if ((rc = ensure_transpose(c, who.c_str()))) return rc;
    if (s.top_ready) return HB_OK;
    if ((rc = hold(c, s.bytes, s.d_top_row, p.nv + 1))) return rc; // (+ 1: the flag word behind the table)
    uint32_t *top = s.d_top_row.get(), *flag = top + p.nv;
    HB_HIP(hipMemsetAsync(top, 0xFF, p.nv * sizeof(uint32_t), c->stream));
    HB_HIP(hipMemsetAsync(flag, 0, sizeof(uint32_t), c->stream));
    if ((rc = lap_start(c))) return rc;
    for_each_virtual_level(p, false, [&](uint64_t lo, uint64_t hi) { // the highest level first: a level reads the tops of the levels above it
        hipLaunchKernelGGL(hbk::fw_top_row_kernel, dim3(grid_blocks(c, (hi - lo + 255) / 256, 8, 1)), dim3(256), 0, c->stream, (const uint64_t *)c->d_row_ptr,
                           (const uint64_t *)c->d_out_ptr, (const uint32_t *)c->d_out_rows, p.n_pad, p.n_pad + p.nv, lo, hi, top, flag);
    });
    HB_HIP(hipGetLastError());
    uint32_t *h32 = (uint32_t *)c->h_counters;
    HB_HIP(hipMemcpyAsync(h32, flag, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if ((rc = lap(c, ms))) return rc;
    if (h32[0]) return fail(c, HB_ERR_INVALID, who + ": unexpected plan layout (a chunk row with a list does not have exactly one reader above it)");
    s.top_ready = true;
    return HB_OK;
}

int links_lists(hb_ctx *c, const std::string &who, size_t nlev, bool forward, const uint32_t *h_sids, const uint32_t *d_sids, uint64_t U,
                const hb_links_options &o, uint32_t *res_sid, unsigned long long *res_key, uint32_t *d_len, std::vector<uint32_t> &degree, hb_links_stats &st);

// The list builds an operator makes for itself (hb_similar_hosts, hb_score_hosts, the limited hb_inbound_similarity): the options with
// the operator's two debug flags, statistics of which only the GPU time is reported, and the degrees of the last build's hosts
struct ListBuild {
    hb_links_options lo{};
    hb_links_stats ls{};
    std::vector<uint32_t> degree;
    size_t nlev; // of links_levels
    ListBuild(size_t nlev_, uint32_t limit, uint32_t flags = 0, uint64_t slots_per_batch = 0) : nlev(nlev_)
    {
        lo.flags = flags & (HB_LINKS_SPREAD_ORDS | HB_LINKS_NO_SHORTCUT);
        lo.limit = limit;
        lo.slots_per_batch = slots_per_batch;
    }
    double gpu_ms() const { return ls.ms_expand + ls.ms_select + ls.ms_emit; }
    int run(hb_ctx *c, const std::string &who, bool forward, const uint32_t *h_sids, const uint32_t *d_sids, uint64_t U, uint32_t *res_sid, unsigned long long *res_key,
            uint32_t *d_len)
    {
        degree.assign(U, 0);
        return links_lists(c, who, nlev, forward, h_sids, d_sids, U, lo, res_sid, res_key, d_len, degree, ls);
    }
};

// hb_backlinks (forward = false) and hb_forwardlinks: the refusals, the distinct queried nodes, the holders and the result are the same;
// a batch is the in-lists' item walk or the out-lists' segment walk
int links_query(hb_ctx *c, const hb_links_options *opt_in, hb_links_stats *st_out, bool forward)
{
    const double t0 = now_ms();
    const std::string who = forward ? "hb_forwardlinks" : "hb_backlinks";
    hb_links_options o{};
    copy_in(opt_in, &o);
    // ---- refusals: all of them before anything of the previous result is touched
    if (!opt_in) return fail(c, HB_ERR_INVALID, who + ": opt == NULL (limit has no default)");
    if (o.limit < 1 || o.limit > hbk::kLkMaxLimit) return fail(c, HB_ERR_INVALID, who + ": limit must be 1 .. 1024");
    if (o.slots_per_batch > kLinksMaxSlots) return fail(c, HB_ERR_INVALID, who + ": slots_per_batch > 65536");
    if (o.node_count && !o.nodes) return fail(c, HB_ERR_INVALID, who + ": node_count without nodes");
    if (o.node_count >= (1ull << 32)) return fail(c, HB_ERR_INVALID, who + ": too many queries");
    const uint64_t limit = o.limit;
    size_t nlev;
    int rc;
    if ((rc = links_levels(c, who, &nlev))) return rc;
    auto &s = c->lnk;
    hb_links_stats st{};
    // ---- the distinct queried nodes, ascending: each is looked up once, every query that names it gets its list
    ResolvedIds ids = resolve_ids(c, o.nodes, o.node_count);
    const uint64_t U = ids.distinct.size();
    st.queries = o.node_count;
    st.distinct = U;
    st.unknown = ids.unknown;
    std::vector<uint32_t> degree(U, 0);
    if (forward && U && (rc = links_top_rows(c, who, &st.ms_expand))) return rc; // (it may refuse: before the previous result is touched)
    s.valid = false;
    auto finish = [&]() {
        s.query_slot.swap(ids.slot);
        s.degree.swap(degree);
        s.limit = o.limit;
        s.entries = 0;
        for (uint32_t q : s.query_slot)
            if (q != kNone) s.entries += std::min<uint64_t>(s.degree[q], limit);
        s.valid = true;
        st.entries = s.entries;
        st.device_bytes = s.bytes;
        st.ms_total = now_ms() - t0;
        copy_out(st_out, st);
        return HB_OK;
    };
    if (!U) return finish();
    if ((rc = hold(c, s.bytes, s.d_res_sid, U * limit))) return rc;
    if ((rc = hold(c, s.bytes, s.d_res_key, U * limit))) return rc;
    if ((rc = links_lists(c, who, nlev, forward, ids.distinct.data(), nullptr, U, o, s.d_res_sid.get(), s.d_res_key.get(), nullptr, degree, st))) return rc;
    return finish();
}

// The lists of U distinct nodes - their sids on the host (h_sids) or on the device (d_sids) - into res_sid / res_key (U x limit each,
// list order; the caller's buffers) and their degrees; d_len, if given, gets the degrees on the device as well.  nlev = the virtual levels
// that links_levels counted (and accepted) before the caller touched its previous result.  The batch loop of
// hb_backlinks / hb_forwardlinks, and what hb_similar_hosts builds its four sets of lists with.  The buffers of a batch are the links
// state's: they hold nothing between two calls.
int links_lists(hb_ctx *c, const std::string &who, size_t nlev, bool forward, const uint32_t *h_sids, const uint32_t *d_sids, uint64_t U,
                const hb_links_options &o, uint32_t *res_sid, unsigned long long *res_key, uint32_t *d_len, std::vector<uint32_t> &degree, hb_links_stats &st)
{
    const Plan &p = c->plan;
    const uint64_t n = p.n, limit = o.limit;
    auto &s = c->lnk;
    int rc;
    if ((rc = links_alloc(c, true))) return rc;
    const uint64_t slots_max = std::min<uint64_t>(o.slots_per_batch ? o.slots_per_batch : kLinksDefaultSlots, U);
    // (forward: no items; behind the backlinks' control words the lengths of the reader lists and the segment offsets, slots + 1)
    const uint64_t item_cap = slots_max + p.nv + 16, ctl_words = 5 * slots_max + 64 + 8 + (forward ? 2 * slots_max + 1 : 0);
    if (!forward && (rc = hold(c, s.bytes, s.d_items, item_cap))) return rc;
    if ((rc = hold(c, s.bytes, s.d_hist, slots_max * 256))) return rc;
    if ((rc = hold(c, s.bytes, s.d_ctl, ctl_words))) return rc;
    if ((rc = hold(c, s.bytes, s.d_out, slots_max * limit))) return rc;
    if ((rc = hold(c, s.bytes, s.d_slot_row, U))) return rc;
    if ((rc = hold(c, s.bytes, s.d_slot_self, U))) return rc;
    // the rows of the distinct nodes (the plan's sid -> row table is on the device: gathered there, from the sids in d_slot_self)
    {
        HB_HIP(hipMemcpyAsync(s.d_slot_self.get(), h_sids ? h_sids : d_sids, U * sizeof(uint32_t), h_sids ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->stream));
        hipLaunchKernelGGL(hbk::lk_rows_kernel, dim3(grid_blocks(c, (U + 255) / 256, 8, 1)), dim3(256), 0, c->stream, (const uint32_t *)c->d_dev_of, U,
                           (o.flags & HB_LINKS_KEEP_SELF) ? 1u : 0u, s.d_slot_row.get(), s.d_slot_self.get());
        HB_HIP(hipGetLastError());
    }
    const bool spread = (o.flags & HB_LINKS_SPREAD_ORDS) != 0, no_shortcut = (o.flags & HB_LINKS_NO_SHORTCUT) != 0;
    const uint64_t mult = spread ? (1ull << 32) / n : 1ull, max_value = (n - 1) * mult;
    const int top_digit = max_value >= (1ull << 24) ? 3 : max_value >= (1ull << 16) ? 2 : max_value >= (1ull << 8) ? 1 : 0; // the rounds n's bits need
    uint32_t *h32 = (uint32_t *)c->h_counters; // (pinned words of the context; hb_run rewrites them before it reads them)
    std::vector<uint32_t> deg(slots_max), seg_base(forward ? slots_max + 1 : 0);

    for (uint64_t base = 0; base < U; base += slots_max) {
        const uint64_t S = std::min<uint64_t>(slots_max, U - base);
        uint32_t *ctl = s.d_ctl.get();
        hbk::LkBatch b{};
        b.row_ptr = c->d_row_ptr;
        b.src = c->d_src;
        b.ord_row = s.d_ord_row.get();
        b.items = s.d_items.get();
        b.slot_row = s.d_slot_row.get() + base;
        b.slot_self = s.d_slot_self.get() + base;
        b.deg = ctl;
        b.sel_k = ctl + slots_max;
        b.sel_prefix = ctl + 2 * slots_max;
        b.thr = ctl + 3 * slots_max;
        b.cursor = ctl + 4 * slots_max;
        uint32_t *lvl_cnt = ctl + 5 * slots_max;
        b.flag = lvl_cnt + 64;
        b.hist = s.d_hist.get();
        b.out = s.d_out.get();
        b.n_pad = p.n_pad;
        b.rows_total = p.n_pad + p.nv;
        b.item_cap = item_cap;
        b.mult = mult;
        b.slots = (uint32_t)S;
        b.limit = o.limit;
        const unsigned slot_blocks = (unsigned)((S + 255) / 256);
        st.batches++;

        // ---- expand and count: level by level down the queried hosts' trees; forward: the reader lists, cut into segments
        HB_HIP(hipMemsetAsync(ctl, 0, ctl_words * sizeof(uint32_t), c->stream));
        HB_HIP(hipMemsetAsync(b.hist, 0, S * 256 * sizeof(uint32_t), c->stream));
        if ((rc = lap_start(c))) return rc;
        uint64_t lo = 0, hi = S;
        hbk::FwBatch f{};
        unsigned seg_blocks = 1;
        if (forward) {
            uint32_t *raw = b.flag + 8, *d_seg_base = raw + slots_max;
            f.out_ptr = c->d_out_ptr;
            f.out_rows = c->d_out_rows;
            f.top_row = s.d_top_row.get();
            f.seg_base = d_seg_base;
            hipLaunchKernelGGL(hbk::fw_len_kernel, dim3(slot_blocks), dim3(256), 0, c->stream, b, f, raw);
            HB_HIP(hipGetLastError());
            HB_HIP(hipMemcpyAsync(deg.data(), raw, S * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
            HB_HIP(hipStreamSynchronize(c->stream));
            uint64_t segs = 0;
            for (uint64_t i = 0; i < S; i++) {
                seg_base[i] = (uint32_t)segs;
                segs += (deg[i] + hbk::kFwSegment - 1) / hbk::kFwSegment;
            }
            seg_base[S] = (uint32_t)segs;
            if (segs >= (1ull << 32)) return fail(c, HB_ERR_INVALID, who + ": unexpected plan layout (the reader lists of a batch exceed the plan's entries)");
            f.segs = (uint32_t)segs;
            hi = segs; // (what rows_walked counts: the segments scanned)
            HB_HIP(hipMemcpyAsync(d_seg_base, seg_base.data(), (S + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
            seg_blocks = grid_blocks(c, std::max<uint64_t>(segs, 1), 8, 1);
            if (segs) hipLaunchKernelGGL(hbk::fw_count_kernel, dim3(seg_blocks), dim3(256), 0, c->stream, b, f);
            HB_HIP(hipGetLastError());
        } else {
            hipLaunchKernelGGL(hbk::lk_seed_kernel, dim3(slot_blocks), dim3(256), 0, c->stream, b);
            for (size_t lev = 0; lo < hi; lev++) {
                if (lev > nlev) return fail(c, HB_ERR_INVALID, who + ": unexpected plan layout (a chunk tree is deeper than the virtual levels)");
                hipLaunchKernelGGL(hbk::lk_expand_kernel, dim3(grid_blocks(c, (hi - lo + hbk::kLkItems - 1) / hbk::kLkItems, 8, 1)), dim3(256), 0, c->stream, b, lo, hi, hi,
                                   lvl_cnt + lev);
                HB_HIP(hipGetLastError());
                HB_HIP(hipMemcpyAsync(h32, lvl_cnt + lev, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
                HB_HIP(hipMemcpyAsync(h32 + 1, b.flag, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
                HB_HIP(hipStreamSynchronize(c->stream));
                if (h32[1] || hi + h32[0] > item_cap) return fail(c, HB_ERR_INVALID, who + ": unexpected plan layout (the chunk rows of a batch outnumber the plan's)");
                lo = hi;
                hi += h32[0];
            }
        }
        const uint64_t total = hi;
        st.rows_walked += total;
        HB_HIP(hipMemcpyAsync(deg.data(), b.deg, S * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        if ((rc = lap(c, &st.ms_expand))) return rc;
        uint64_t selecting = 0;
        for (uint64_t i = 0; i < S; i++) {
            degree[base + i] = deg[i];
            st.edges_gathered += deg[i];
            selecting += (deg[i] > limit || (no_shortcut && deg[i] > 0)) ? 1 : 0;
        }
        st.selected += selecting;

        // ---- select: the threshold of every slot that has more than it may keep
        uint64_t blocks = 1, per_block = 0; // (backlinks: contiguous item ranges per workgroup)
        if (!forward) {
            blocks = grid_blocks(c, (total + hbk::kLkItems - 1) / hbk::kLkItems, 4, 1);
            per_block = ((total + blocks - 1) / blocks + hbk::kLkItems - 1) / hbk::kLkItems * hbk::kLkItems;
            blocks = (total + per_block - 1) / per_block;
        }
        if ((rc = lap_start(c))) return rc;
        hipLaunchKernelGGL(hbk::lk_plan_kernel, dim3(slot_blocks), dim3(256), 0, c->stream, b, no_shortcut ? 1u : 0u);
        if (selecting) {
            for (int d = top_digit; d >= 0; d--) {
                if (forward) hipLaunchKernelGGL(hbk::fw_hist_kernel, dim3(seg_blocks), dim3(256), 0, c->stream, b, f, d);
                else hipLaunchKernelGGL(hbk::lk_hist_kernel, dim3((unsigned)blocks), dim3(256), 0, c->stream, b, total, per_block, d);
                hipLaunchKernelGGL(hbk::lk_pick_kernel, dim3(slot_blocks), dim3(256), 0, c->stream, b, d);
            }
        }
        HB_HIP(hipGetLastError());
        if ((rc = lap(c, &st.ms_select))) return rc;

        // ---- emit, sort, translate
        if ((rc = lap_start(c))) return rc;
        if (!forward) hipLaunchKernelGGL(hbk::lk_emit_kernel, dim3(grid_blocks(c, (total + hbk::kLkItems - 1) / hbk::kLkItems, 8, 1)), dim3(256), 0, c->stream, b, total);
        else if (f.segs) hipLaunchKernelGGL(hbk::fw_emit_kernel, dim3(seg_blocks), dim3(256), 0, c->stream, b, f);
        hipLaunchKernelGGL(hbk::lk_sort_kernel, dim3((unsigned)S), dim3(256), 0, c->stream, b, (const uint32_t *)s.d_inv.get(),
                           (const unsigned long long *)s.d_key.get(), n, res_sid + base * limit, res_key + base * limit);
        HB_HIP(hipGetLastError());
        if (d_len) HB_HIP(hipMemcpyAsync(d_len + base, b.deg, S * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
        if ((rc = lap(c, &st.ms_emit))) return rc;
    }
    return HB_OK;
}

const char *const kNoBacklinks = "no backlinks result (call hb_backlinks)";

} // namespace

extern "C" {

int hb_links_set_keys(hb_ctx *c, const hb_links_key_options *opt, hb_links_key_stats *stats)
{
    return operator_entry(c, "hb_links_set_keys", [&]() { return links_set_keys(c, opt, stats); });
}

int hb_backlinks(hb_ctx *c, const hb_links_options *opt, hb_links_stats *stats)
{
    return operator_entry(c, "hb_backlinks", [&]() { return links_query(c, opt, stats, false); });
}

int hb_forwardlinks(hb_ctx *c, const hb_links_options *opt, hb_links_stats *stats)
{
    return operator_entry(c, "hb_forwardlinks", [&]() { return links_query(c, opt, stats, true); });
}

int hb_links_count(hb_ctx *c, uint64_t *queries, uint64_t *entries)
{
    return reader_entry(c, c && c->lnk.valid, "hb_links_count", kNoBacklinks, [&]() -> int {
        if (queries) *queries = c->lnk.query_slot.size();
        if (entries) *entries = c->lnk.entries;
        return HB_OK;
    });
}

int hb_links_copy(hb_ctx *c, uint64_t *offsets, uint64_t *degrees, hb_u128 *ids, uint64_t *keys, uint64_t cap)
{
    return reader_entry(c, c && c->lnk.valid, "hb_links_copy", kNoBacklinks, [&]() -> int {
        auto &s = c->lnk;
        const uint64_t q = s.query_slot.size(), limit = s.limit, U = s.degree.size();
        if ((ids || keys) && cap < s.entries) return fail(c, HB_ERR_INVALID, "hb_links_copy: cap < the entries of hb_links_count");
        // only what is asked for comes down: the lists as sids for ids, their keys for keys; offsets and degrees are on the host
        std::vector<uint32_t> sid;
        std::vector<uint64_t> key;
        if (ids && s.entries) {
            sid.resize(U * limit);
            HB_HIP(hipMemcpyAsync(sid.data(), s.d_res_sid.get(), U * limit * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        }
        if (keys && s.entries) {
            key.resize(U * limit);
            HB_HIP(hipMemcpyAsync(key.data(), s.d_res_key.get(), U * limit * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        }
        if (!sid.empty() || !key.empty()) HB_HIP(hipStreamSynchronize(c->stream));
        uint64_t at = 0;
        for (uint64_t i = 0; i < q; i++) {
            const uint32_t slot = s.query_slot[i];
            const uint64_t deg = slot != kNone ? s.degree[slot] : 0, len = std::min<uint64_t>(deg, limit);
            if (offsets) offsets[i] = at;
            if (degrees) degrees[i] = deg;
            for (uint64_t j = 0; j < len; j++) {
                if (!sid.empty()) {
                    const uint32_t v = sid[slot * limit + j];
                    if (v >= c->g.ids.size()) return fail(c, HB_ERR_INVALID, "hb_links_copy: a list entry is no node (internal error)");
                    ids[at + j] = c->g.ids[v];
                }
                if (!key.empty()) keys[at + j] = key[slot * limit + j];
            }
            at += len;
        }
        if (offsets) offsets[q] = at;
        return HB_OK;
    });
}

} // extern "C"
