// hb_api_similarity.inc - part of the hb_api.hip translation unit (included at its end; uses its hb_ctx and helpers).
// hb_inbound_similarity: Scorer (crates/core/src/ranking/inbound_similarity.rs:61-138) over BitVec (ranking/bitvec_similarity.rs:131-189)
// for every node of the loaded graph - sixteen liked / disliked hosts per batch in the 64-byte rows of the HyperBall plan, one level of
// the shared walk per batch (kernels: hb_similarity.hip.h).  Definitions: include/hyperball.h.  The walk borrows d_regs / d_part / the
// changed bitmaps / the sweep scratch as hb_betweenness does (claim_rows); the per-graph state, the sums and the result live
// in buffers of their own.  With hb_similarity_options.limit the BitVecs are those of the limit best backlinks: the rows whose cut
// differs from their list as loaded get explicit cut lists (GraphDeviceState::lim, built here with the list builder of hb_api_links.inc),
// a seed and a count kernel of their own (hb_similarity_limit.hip.h); the walk level, the accumulate and the readers are shared.

namespace {

// the buffers of the operator and the per-graph state (position bytes, in-degrees, blooms), once per loaded graph; *ms = its GPU time
int similarity_alloc(hb_ctx *c, double *ms_out)
{
    auto &s = c->sim;
    if (s.ready) return HB_OK;
    const Plan &p = c->plan;
    const uint64_t rows_total = p.n_pad + p.nv;
    const uint64_t before = c->stats.device_bytes;
    int rc;
    if ((rc = dev_alloc(c, &s.d_pos, p.n_pad))) return rc;
    if ((rc = dev_alloc(c, &s.d_bloom, rows_total))) return rc;
    if ((rc = dev_alloc(c, &s.d_vmask, p.nv))) return rc;
    if ((rc = dev_alloc(c, &s.d_acc, p.n_pad * 2))) return rc;
    if ((rc = dev_alloc(c, &s.d_anchor_rows, hbk::kSimSlots))) return rc;
    if ((rc = dev_alloc(c, &s.d_anchor_sids, hbk::kSimSlots))) return rc;
    if ((rc = dev_alloc(c, &s.d_cnt, 8))) return rc;
    if ((rc = dev_alloc(c, &s.d_score, p.n))) return rc;
    if ((rc = dev_alloc(c, &s.d_anchor, p.n))) return rc;
    if ((rc = dev_alloc(c, &s.d_key, p.n))) return rc;
    if ((rc = dev_alloc(c, &s.d_keep, p.n))) return rc;
    if ((rc = lap_start(c))) return rc;
    if ((rc = distance_indegrees(c))) return rc; // len = the in-degree through the chunk trees (bfs_indegree_kernel), shared with hb_distances
    hipLaunchKernelGGL(hbk::sim_pos_kernel, dim3(grid_blocks(c, (p.n_pad + 255) / 256, 8, 1)), dim3(256), 0, c->stream, (const uint64_t *)c->d_idlow,
                       (const uint32_t *)c->d_sid_of, p.n_pad, s.d_pos);
    auto bloom = [&](uint64_t lo, uint64_t hi) { // a quad per row
        hipLaunchKernelGGL(hbk::sim_bloom_kernel, dim3(grid_blocks(c, (hi - lo + 63) / 64, 8, 1)), dim3(256), 0, c->stream, (const uint64_t *)c->d_row_ptr,
                           (const uint32_t *)c->d_src, (const uint8_t *)s.d_pos, s.d_bloom, p.n_pad, rows_total, lo, hi);
    };
    for_each_virtual_level(p, true, bloom); // ascending: a chunk row ORs the partials of the chunk rows below it
    if (p.n_pad) bloom(0, p.n_pad);
    HB_HIP(hipGetLastError());
    *ms_out = 0.0; // (its GPU time alone: set, not added to)
    if ((rc = lap(c, ms_out))) return rc;
    s.bytes = c->stats.device_bytes - before;
    s.ready = true;
    return HB_OK;
}

// ---- the limited mode (hb_similarity_options.limit > 0; kernels: hb_similarity_limit.hip.h) ------------------------------------------
// the cut lists describe one graph, one key set and one limit: hb_links_set_keys and a call with another limit end here (a load frees
// the whole graph state)
void similarity_limit_drop(hb_ctx *c)
{
    c->stats.device_bytes -= c->lim.bytes;
    c->lim = GraphDeviceState::SimilarityLimitState{};
}

// The listed rows and their cut lists under the current key set, once per (graph, key set, limit); *ms_out += its GPU time.  The list
// builder's result buffers are this function's (the keys) and the state's (the lists): the user's hb_backlinks / hb_forwardlinks result
// stays readable.  Needs the per-graph state of similarity_alloc (pos, the in-degrees), links_top_rows and the nlev of links_levels.
int similarity_limit_build(hb_ctx *c, uint32_t limit, size_t nlev, double *ms_out)
{
    auto &s = c->lim;
    if (s.ready && s.limit == limit) return HB_OK;
    similarity_limit_drop(c);
    const Plan &p = c->plan;
    const std::string who = "hb_inbound_similarity";
    const uint64_t n_pad = p.n_pad, rows_total = n_pad + p.nv;
    int rc;
    if ((rc = hold(c, s.bytes, s.d_idx, n_pad))) return rc;
    if ((rc = hold(c, s.bytes, s.d_seed_rows, hbk::kSimSlots))) return rc;
    if ((rc = hold(c, s.bytes, s.d_cnt, 4))) return rc;
    DevPtr<uint32_t> d_flag, d_sids, d_deg; // (work memory of the build: gone at its end)
    DevPtr<uint64_t> d_off;
    DevPtr<unsigned long long> d_keys;
    if (d_flag.alloc(std::max<uint64_t>(n_pad, 64)) != hipSuccess || d_off.alloc(n_pad + 1) != hipSuccess)
        return fail(c, HB_ERR_NOMEM, who + ": out of device memory for the listed rows");
    // ---- which rows are listed: a self link, or more in-neighbours than the limit
    HB_HIP(hipMemsetAsync(d_flag.get(), 0, std::max<uint64_t>(n_pad, 64) * sizeof(uint32_t), c->stream));
    if ((rc = lap_start(c))) return rc;
    hipLaunchKernelGGL(hbk::siml_self_kernel, dim3(grid_blocks(c, (rows_total + 63) / 64, 8, 1)), dim3(256), 0, c->stream, (const uint64_t *)c->d_row_ptr,
                       (const uint32_t *)c->d_src, (const uint32_t *)c->lnk.d_top_row.get(), n_pad, rows_total, d_flag.get());
    hipLaunchKernelGGL(hbk::siml_mark_kernel, dim3(grid_blocks(c, (n_pad + 255) / 256, 8, 1)), dim3(256), 0, c->stream, (const uint32_t *)c->d_sid_of,
                       (const uint32_t *)c->dst.d_indeg, limit, n_pad, d_flag.get());
    HB_HIP(hipGetLastError());
    const std::string e = device_prefix((void *)c->stream, d_flag.get(), n_pad, d_off.get());
    if (!e.empty()) return fail(c, HB_ERR_HIP, who + ": " + e);
    uint64_t listed = 0;
    HB_HIP(hipMemcpyAsync(&listed, d_off.get() + n_pad, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if ((rc = lap(c, ms_out))) return rc;
    if (listed > n_pad) return fail(c, HB_ERR_INVALID, who + ": more listed rows than node rows (internal error)");
    if ((rc = hold(c, s.bytes, s.d_list_row, listed))) return rc;
    if ((rc = hold(c, s.bytes, s.d_lists, listed * limit))) return rc;
    if ((rc = hold(c, s.bytes, s.d_len, listed))) return rc;
    if ((rc = hold(c, s.bytes, s.d_bloom, listed))) return rc;
    const uint64_t piece_max = xbit(c, HB_X_SIM_SMALL_PIECES) ? 64 : kLinksMaxSlots;
    if (d_sids.alloc(std::max<uint64_t>(listed, 64)) != hipSuccess || d_deg.alloc(std::max<uint64_t>(listed, 64)) != hipSuccess ||
        d_keys.alloc(std::max<uint64_t>(std::min(listed, piece_max) * limit, 64)) != hipSuccess)
        return fail(c, HB_ERR_NOMEM, who + ": out of device memory for the list builder's keys");
    if ((rc = lap_start(c))) return rc;
    hipLaunchKernelGGL(hbk::siml_assign_kernel, dim3(grid_blocks(c, (n_pad + 255) / 256, 8, 1)), dim3(256), 0, c->stream, (const uint32_t *)c->d_sid_of,
                       (const uint32_t *)d_flag.get(), (const uint64_t *)d_off.get(), n_pad, listed, s.d_idx.get(), s.d_list_row.get(), d_sids.get());
    HB_HIP(hipGetLastError());
    if ((rc = lap(c, ms_out))) return rc;
    // ---- their cut lists: the list builder of hb_backlinks, a piece of hosts at a time; then sid -> device row, len and bloom per list
    ListBuild lists(nlev, limit);
    uint64_t entries = 0;
    for (uint64_t base = 0; base < listed; base += piece_max) {
        const uint64_t P = std::min(piece_max, listed - base);
        if ((rc = lists.run(c, who, false, nullptr, d_sids.get() + base, P, s.d_lists.get() + base * limit, d_keys.get(), d_deg.get() + base))) return rc;
        for (uint32_t d : lists.degree) entries += std::min<uint64_t>(d, limit);
        if ((rc = lap_start(c))) return rc;
        hipLaunchKernelGGL(hbk::siml_finish_kernel, dim3(grid_blocks(c, (P + 3) / 4, 8, 1)), dim3(256), 0, c->stream, s.d_lists.get() + base * limit,
                           (const uint32_t *)d_deg.get() + base, (const uint32_t *)c->d_dev_of, (const uint8_t *)c->sim.d_pos, P, limit, p.n, n_pad,
                           s.d_len.get() + base, s.d_bloom.get() + base);
        HB_HIP(hipGetLastError());
        if ((rc = lap(c, ms_out))) return rc;
    }
    *ms_out += lists.gpu_ms();
    s.listed = listed;
    s.entries = entries;
    s.limit = limit;
    s.ready = true;
    return HB_OK;
}

// Scorer::calculate_score for an id that is no node of the graph: an empty BitVec, so only the entries equal to the id contribute
double similarity_unknown_score(const hb_ctx *c, const hb_u128 &id)
{
    const auto &s = c->sim;
    double liked = 0.0, disliked = 0.0;
    for (const hb_u128 &e : s.liked)
        if (u128_eq(e, id) && s.self_score != 0.0) liked += s.self_score;
    for (const hb_u128 &e : s.disliked)
        if (u128_eq(e, id) && s.self_score != 0.0) disliked += s.self_score;
    double v = (double)s.disliked.size() + (liked - disliked);
    if (s.normalized) v = v / (double)std::max<size_t>(s.liked.size(), 1);
    return v > 0.0 ? v : 0.0;
}

int inbound_similarity(hb_ctx *c, const hb_similarity_options *opt_in, hb_similarity_stats *st_out)
{
    const double t0 = now_ms();
    hb_similarity_options o{};
    copy_in(opt_in, &o);
    int rc;
    if ((o.flags & HB_SIM_DENSE_ONLY) && (o.flags & HB_SIM_SPARSE_ONLY))
        return fail(c, HB_ERR_INVALID, "hb_inbound_similarity: HB_SIM_DENSE_ONLY and HB_SIM_SPARSE_ONLY exclude each other");
    if ((o.liked_count && !o.liked) || (o.disliked_count && !o.disliked))
        return fail(c, HB_ERR_INVALID, "hb_inbound_similarity: a count without its list");
    const uint64_t L = o.liked_count, D = o.disliked_count, E = L + D;
    if (!E) return fail(c, HB_ERR_INVALID, "hb_inbound_similarity: no liked and no disliked host");
    if (o.limit > hbk::kLkMaxLimit) return fail(c, HB_ERR_INVALID, "hb_inbound_similarity: limit must be 0 (whole in-lists) or 1 .. 1024");
    const Plan &p = c->plan;
    auto &s = c->sim;
    hb_similarity_stats st{};
    const bool limited = o.limit != 0 && p.n != 0;
    size_t nlev = 0;
    if (limited) { // what the list builder may refuse: before the previous result is touched
        if ((rc = links_levels(c, "hb_inbound_similarity", &nlev))) return rc;
        if ((rc = links_top_rows(c, "hb_inbound_similarity", &st.ms_lists))) return rc;
    }
    s.valid = false;
    st.liked = L;
    st.disliked = D;
    // entry e = liked[e] below L, disliked[e - L] above: its sid, kNone = no node of the graph
    std::vector<uint32_t> sids(E, kNone);
    for (uint64_t e = 0; e < E; e++)
        if (!find_sid(c, e < L ? o.liked[e] : o.disliked[e - L], &sids[e])) st.unknown++;
    s.liked.assign(o.liked, o.liked + L);
    s.disliked.assign(o.disliked, o.disliked + D);
    s.normalized = (o.flags & HB_SIM_NORMALIZED) != 0;
    s.self_score = (o.flags & HB_SIM_SELF_SCORE) ? o.self_score : 1.0;
    s.last_slots = 0;
    s.limit = limited ? o.limit : 0;
    auto finish = [&]() {
        st.device_bytes = s.bytes + c->lim.bytes;
        st.ms_total = now_ms() - t0;
        copy_out(st_out, st);
        return HB_OK;
    };
    if (p.n == 0) { // an empty graph: nothing to score
        s.valid = true;
        return finish();
    }
    if ((rc = similarity_alloc(c, &st.ms_bloom))) return rc;
    auto &lm = c->lim;
    if (limited) {
        if ((rc = similarity_limit_build(c, o.limit, nlev, &st.ms_lists))) return rc;
        st.listed_rows = lm.listed;
        st.list_entries = lm.entries;
    }
    const uint64_t n_pad = p.n_pad, rows_total = p.n_pad + p.nv;
    HB_HIP(hipMemsetAsync(s.d_acc, 0, n_pad * 2 * sizeof(double), c->stream));
    HB_HIP(hipMemsetAsync(s.d_anchor, 0, p.n, c->stream));
    claim_rows(c, RowsOf::Similarity);
    unsigned long long *h = c->h_counters; // (pinned words of the context; hb_run rewrites them before it reads them)
    for (uint64_t b0 = 0; b0 < E; b0 += hbk::kSimSlots) {
        const uint32_t count = (uint32_t)std::min<uint64_t>(hbk::kSimSlots, E - b0);
        st.batches++;
        s.last_slots = count;
        const bool any_known = std::any_of(sids.begin() + b0, sids.begin() + b0 + count, [](uint32_t v) { return v != kNone; });
        // ---- seed: the indicators (all-zero outside the marked rows), the level-0 bitmap, the anchors' rows
        if ((rc = lap_start(c))) return rc;
        HB_HIP(hipMemsetAsync(c->d_bits[1], 0, c->bits_words * 4, c->stream)); // (a batch that runs no level has no count rows)
        uint64_t marked = 0, active = 0;
        if (any_known) {
            HB_HIP(hipMemsetAsync(c->d_regs[0], 0, n_pad * 64, c->stream));
            HB_HIP(hipMemsetAsync(c->d_bits[0], 0, c->bits_words * 4, c->stream));
            if (p.nv) HB_HIP(hipMemsetAsync(s.d_vmask, 0, p.nv * sizeof(uint32_t), c->stream));
            HB_HIP(hipMemsetAsync(s.d_cnt, 0, 8 * sizeof(unsigned long long), c->stream));
            HB_HIP(hipMemcpyAsync(s.d_anchor_sids, sids.data() + b0, count * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
            hipLaunchKernelGGL(hbk::sim_anchor_rows_kernel, dim3(1), dim3(64), 0, c->stream, (const uint32_t *)s.d_anchor_sids, count, (const uint32_t *)c->d_dev_of,
                               s.d_anchor_rows, s.d_anchor);
            const uint32_t *seed_rows = s.d_anchor_rows; // the anchors that seed from the plan's lists: all of them, or the unlisted ones
            if (limited) {
                hipLaunchKernelGGL(hbk::sim_seed_rows_kernel, dim3(1), dim3(64), 0, c->stream, (const uint32_t *)s.d_anchor_rows, count, (const uint32_t *)lm.d_idx.get(),
                                   lm.d_seed_rows.get());
                seed_rows = lm.d_seed_rows.get();
            }
            hipLaunchKernelGGL(hbk::sim_seed_node_kernel, dim3(count), dim3(256), 0, c->stream, seed_rows, count, (const uint64_t *)c->d_row_ptr,
                               (const uint32_t *)c->d_src, (uint32_t *)c->d_regs[0], c->d_bits[0], s.d_vmask, (const uint32_t *)c->d_outdeg, n_pad, rows_total, s.d_cnt);
            for_each_virtual_level(p, false, [&](uint64_t lo, uint64_t hi) { // the chunk rows of the anchors' lists, the highest virtual level first
                hipLaunchKernelGGL(hbk::sim_seed_virt_kernel, dim3(grid_blocks(c, (hi - lo + 3) / 4, 8, 1)), dim3(256), 0, c->stream, (const uint64_t *)c->d_row_ptr,
                                   (const uint32_t *)c->d_src, (uint32_t *)c->d_regs[0], c->d_bits[0], s.d_vmask, (const uint32_t *)c->d_outdeg, n_pad, rows_total, lo,
                                   hi, s.d_cnt);
            });
            if (limited && lm.listed) // a listed anchor: its stored cut list
                hipLaunchKernelGGL(hbk::sim_seed_list_kernel, dim3(count), dim3(256), 0, c->stream, (const uint32_t *)s.d_anchor_rows, count,
                                   (const uint32_t *)lm.d_idx.get(), (const uint32_t *)lm.d_lists.get(), (const uint32_t *)lm.d_len.get(), lm.limit,
                                   (uint32_t *)c->d_regs[0], c->d_bits[0], s.d_vmask, (const uint32_t *)c->d_outdeg, n_pad, rows_total, s.d_cnt);
            HB_HIP(hipGetLastError());
            HB_HIP(hipMemcpyAsync(h, s.d_cnt, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        }
        if ((rc = lap(c, &st.ms_score))) return rc;
        if (any_known) {
            marked = h[0];
            active = h[1];
        }
        // ---- count: ONE level of the shared walk; dense / bitmap / sweep by the A_t rule on the out-degree sum of the marked rows
        if (marked) {
            PassMode mode = pass_mode(c, active);
            if (o.flags & HB_SIM_DENSE_ONLY) mode = kModeDense;
            if (o.flags & HB_SIM_SPARSE_ONLY) mode = c->sparse_ok ? kModeSweep : kModeBitmap;
            hbk::SimParams sp{};
            fill_walk_params(c, &sp);
            sp.rd = c->d_regs[0];
            sp.wr = c->d_regs[1];
            sp.part = c->d_part;
            sp.bits_rd = c->d_bits[0];
            sp.bits_wr = c->d_bits[1];
            sp.cnt = s.d_cnt + 4;
            WalkLevel lv{};
            if ((rc = walk_forward_level(c, sp, mode, marked, [&](bool real) { launch_walk<SimilarityWalk>(c, sp, real, mode); }, &lv))) return rc;
            st.levels_mode[mode]++;
            st.ms_mode[mode] += lv.ms;
            st.ms_count += lv.ms;
            st.rows_nonzero += lv.cnt[0];
            st.edges_gathered += lv.cnt[2];
            if (limited && lm.listed) { // the walk summed the WHOLE lists of the listed rows: their counts again, from the cut lists
                hbk::SimListParams lp{};
                lp.rd = c->d_regs[0];
                lp.bits_rd = c->d_bits[0];
                lp.wr = c->d_regs[1];
                lp.bits_wr = c->d_bits[1];
                lp.list_row = lm.d_list_row.get();
                lp.lists = lm.d_lists.get();
                lp.len_l = lm.d_len.get();
                lp.cnt = lm.d_cnt.get();
                lp.listed = lm.listed;
                lp.n_pad = n_pad;
                lp.limit = lm.limit;
                HB_HIP(hipMemsetAsync(lm.d_cnt.get(), 0, 4 * sizeof(unsigned long long), c->stream));
                if ((rc = lap_start(c))) return rc;
                hipLaunchKernelGGL(hbk::sim_list_count_kernel, dim3(grid_blocks(c, (lm.listed + 3) / 4, 8, 1)), dim3(256), 0, c->stream, lp);
                HB_HIP(hipGetLastError());
                HB_HIP(hipMemcpyAsync(h, lm.d_cnt.get(), 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
                double lms = 0.0;
                if ((rc = lap(c, &lms))) return rc;
                st.ms_list_count += lms;
                st.ms_count += lms;
                st.rows_nonzero += h[0];
                st.rows_nonzero -= h[1];
                st.edges_gathered += h[2];
            }
        }
        // ---- accumulate: the slots in order (an anchor without in-links still scores itself)
        if (any_known) {
            hbk::SimAccParams ap{};
            ap.anchor_rows = s.d_anchor_rows;
            ap.count = count;
            ap.liked = (uint32_t)(b0 >= L ? 0 : std::min<uint64_t>(L - b0, count));
            ap.counts = (const uint32_t *)c->d_regs[1];
            ap.bits = c->d_bits[1];
            ap.len = c->dst.d_indeg;
            ap.bloom = s.d_bloom;
            if (limited) {
                ap.lidx = lm.d_idx.get();
                ap.len_l = lm.d_len.get();
                ap.bloom_l = lm.d_bloom.get();
            }
            ap.acc = s.d_acc;
            ap.self_score = s.self_score;
            ap.n_pad = n_pad;
            if ((rc = lap_start(c))) return rc;
            hipLaunchKernelGGL(hbk::sim_accumulate_kernel, dim3(grid_blocks(c, (n_pad + 255) / 256, 8, 1)), dim3(256), 0, c->stream, ap);
            HB_HIP(hipGetLastError());
            if ((rc = lap(c, &st.ms_score))) return rc;
        }
    }
    if ((rc = lap_start(c))) return rc;
    hipLaunchKernelGGL(hbk::sim_score_kernel, dim3(grid_blocks(c, (p.n + 255) / 256, 8, 1)), dim3(256), 0, c->stream, (const double *)s.d_acc, (const uint32_t *)c->d_dev_of,
                       p.n, (double)D, s.normalized ? (double)std::max<uint64_t>(L, 1) : 0.0, s.d_score);
    HB_HIP(hipGetLastError());
    if ((rc = lap(c, &st.ms_score))) return rc;
    s.valid = true;
    return finish();
}

const char *const kNoSimilarity = "no similarity result (call hb_inbound_similarity)";

} // namespace

extern "C" {

int hb_inbound_similarity(hb_ctx *c, const hb_similarity_options *opt, hb_similarity_stats *stats)
{
    return operator_entry(c, "hb_inbound_similarity", [&]() { return inbound_similarity(c, opt, stats); });
}

int hb_similarity_all(hb_ctx *c, double *vals, uint64_t cap)
{
    return guarded(c, [&]() -> int {
        if (!c) return HB_ERR_INVALID;
        return result_all<double>(c, c->sim.valid, "hb_similarity_all", "vals", kNoSimilarity, vals, cap, c->sim.d_score);
    });
}

int hb_similarity_lookup(hb_ctx *c, const hb_u128 *ids, uint64_t count, double *vals)
{
    return guarded(c, [&]() -> int {
        if (!c || (count && (!ids || !vals))) return c ? fail(c, HB_ERR_INVALID, "hb_similarity_lookup: ids / vals == NULL") : HB_ERR_INVALID;
        int rc = result_ready(c, c->sim.valid, "hb_similarity_lookup", kNoSimilarity);
        if (rc) return rc;
        if (!count) return HB_OK;
        std::vector<uint32_t> sids(count, kNone);
        uint64_t known = 0;
        for (uint64_t i = 0; i < count; i++) known += find_sid(c, ids[i], &sids[i]) ? 1 : 0;
        if (known) { // the scores of the nodes are gathered on the device: only `count` values come down
            DevPtr<uint32_t> d_sids;
            DevPtr<double> d_out;
            HB_HIP(d_sids.alloc(count));
            HB_HIP(d_out.alloc(count));
            HB_HIP(hipMemcpyAsync(d_sids.get(), sids.data(), count * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
            hipLaunchKernelGGL(hbk::sim_lookup_kernel, dim3(grid_blocks(c, (count + 255) / 256, 8, 1)), dim3(256), 0, c->stream, (const double *)c->sim.d_score,
                               (const uint32_t *)d_sids.get(), count, d_out.get());
            HB_HIP(hipGetLastError());
            HB_HIP(hipMemcpyAsync(vals, d_out.get(), count * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            HB_HIP(hipStreamSynchronize(c->stream));
        }
        for (uint64_t i = 0; i < count; i++)
            if (sids[i] == kNone) vals[i] = similarity_unknown_score(c, ids[i]);
        return HB_OK;
    });
}

int hb_similarity_top(hb_ctx *c, uint64_t k, uint32_t flags, hb_u128 *ids, double *vals, uint64_t *written)
{
    return reader_entry(c, c && c->sim.valid, "hb_similarity_top", kNoSimilarity, [&]() -> int {
        const uint64_t n = c->plan.n;
        auto &s = c->sim;
        const uint64_t top = std::min<uint64_t>(k, n);
        if (!top) return HB_OK;
        hipLaunchKernelGGL(hbk::sim_top_keys_kernel, dim3(grid_blocks(c, (n + 255) / 256, 8, 1)), dim3(256), 0, c->stream, (const double *)s.d_score,
                           (const uint8_t *)s.d_anchor, (flags & HB_SIM_TOP_SKIP_ANCHORS) ? 1 : 0, n, s.d_key, s.d_keep);
        HB_HIP(hipGetLastError());
        return result_top(c, "hb_similarity_top", s.d_key, s.d_keep, n, top, [](uint32_t at) { return at; }, ids, vals, written);
    }, written);
}

int hb_debug_copy_similarity_batch(hb_ctx *c, uint32_t *counts, uint64_t *bloom, uint32_t *len)
{
    return reader_entry(c, c && c->sim.valid, "hb_debug_copy_similarity_batch", kNoSimilarity, [&]() -> int {
        const Plan &p = c->plan;
        auto &s = c->sim;
        if (!p.n) return HB_OK;
        const auto &lm = c->lim;
        if (s.limit && !(lm.ready && lm.limit == s.limit))
            return fail(c, HB_ERR_INVALID, "hb_debug_copy_similarity_batch: the cut lists of the last call are gone (hb_links_set_keys)");
        const bool counts_live = c->rows == RowsOf::Similarity; // (s.valid holds: d_regs[1] / d_bits[1] still hold the last batch's counts)
        if (counts && !counts_live)
            return fail(c, HB_ERR_INVALID, "hb_debug_copy_similarity_batch: the counts of the last batch are gone (another call has used the HyperBall state)");
        DevPtr<uint32_t> d_counts, d_len;
        DevPtr<uint64_t> d_bloom;
        HB_HIP(d_counts.alloc(p.n * hbk::kSimSlots));
        HB_HIP(d_len.alloc(p.n));
        HB_HIP(d_bloom.alloc(p.n));
        const uint32_t *bits = counts_live ? c->d_bits[1] : nullptr; // (bloom / len alone: no counts are read)
        hipLaunchKernelGGL(hbk::sim_export_kernel, dim3(grid_blocks(c, (p.n + 255) / 256, 8, 1)), dim3(256), 0, c->stream, (const uint32_t *)c->d_regs[1], bits,
                           (const uint64_t *)s.d_bloom, (const uint32_t *)c->dst.d_indeg, s.limit ? (const uint32_t *)lm.d_idx.get() : nullptr,
                           (const uint32_t *)lm.d_len.get(), (const uint64_t *)lm.d_bloom.get(), (const uint32_t *)c->d_dev_of, p.n, d_counts.get(), d_bloom.get(),
                           d_len.get());
        HB_HIP(hipGetLastError());
        if (counts) HB_HIP(hipMemcpyAsync(counts, d_counts.get(), p.n * hbk::kSimSlots * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        if (bloom) HB_HIP(hipMemcpyAsync(bloom, d_bloom.get(), p.n * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        if (len) HB_HIP(hipMemcpyAsync(len, d_len.get(), p.n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HB_HIP(hipStreamSynchronize(c->stream));
        return HB_OK;
    });
}

} // extern "C"
