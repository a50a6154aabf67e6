// hb_api_distance.inc - part of the hb_api.hip translation unit (included at its end; uses its hb_ctx and helpers).
// hb_distances: ShortestPaths (crates/core/src/webgraph/shortest_path.rs:26-227) on the loaded graph - dijkstra_multi (:57-103) with
// unit costs as one level-synchronous, direction-optimising BFS, forward or reversed (kernels: hb_bfs.hip.h).  Definitions:
// include/hyperball.h.

namespace {

// Beamer's switch rule (Beamer, Asanovic, Patterson: "Direction-Optimizing Breadth-First Search", SC 2012) on this layout's edge
// counts.  m_f = degree sum of the frontier (out-degrees forward, in-degrees reversed), m_u = the same sum over the nodes not reached
// yet, n_f = frontier size.  top-down -> bottom-up when m_f * alpha > m_u; bottom-up -> top-down when n_f * beta < n and the frontier
// shrinks.  HB_DIST_ALPHA / HB_DIST_BETA in the environment override them (tools/distance_bench.py sweeps them; DESIGN.md section 14).
constexpr uint64_t kDistAlpha = 14, kDistBeta = 24;

uint64_t dist_env(const char *name, uint64_t dflt)
{
    const char *v = std::getenv(name);
    if (!v || !*v) return dflt;
    const unsigned long long x = std::strtoull(v, nullptr, 10);
    return x ? (uint64_t)x : dflt;
}

// the buffers of the BFS, once per loaded graph
int distance_alloc(hb_ctx *c)
{
    auto &d = c->dst;
    if (d.ready) return HB_OK;
    const Plan &p = c->plan;
    const uint64_t rows_total = p.n_pad + p.nv;
    int rc;
    d.words_total = (rows_total + 31) / 32 + 64;
    if ((rc = dev_alloc(c, &d.d_dist, p.n_pad))) return rc;
    if ((rc = dev_alloc(c, &d.d_vis, d.words_total))) return rc;
    if ((rc = dev_alloc(c, &d.d_front, p.n_pad / 32 + 64))) return rc;
    if ((rc = dev_alloc(c, &d.d_next, d.words_total))) return rc;
    d.heavy_cap = (uint32_t)std::min<uint64_t>(c->plan_entries / hbk::kBfsHeavy + 64, 0x7FFFFFFFull); // rows with more than kBfsHeavy entries
    if ((rc = dev_alloc(c, &d.d_heavy, d.heavy_cap))) return rc;
    if ((rc = dev_alloc(c, &d.d_heavy_cnt, 64))) return rc;
    if ((rc = dev_alloc(c, &d.d_cnt, 256 * 4))) return rc;
    if ((rc = node_result_alloc(c, d.res))) return rc;
    if ((rc = ensure_transpose(c, "hb_distances"))) return rc;
    HB_HIP(hipMemsetAsync(d.d_next, 0, d.words_total * sizeof(uint32_t), c->stream)); // all-zero between levels from here on
    HB_HIP(hipMemsetAsync(d.d_heavy_cnt, 0, 64 * sizeof(unsigned int), c->stream));
    d.ready = true;
    return HB_OK;
}

// in-degrees through the chunk trees (the reversed switch rule): once per loaded graph
int distance_indegrees(hb_ctx *c)
{
    auto &d = c->dst;
    if (d.indeg_valid) return HB_OK;
    const Plan &p = c->plan;
    const uint64_t rows_total = p.n_pad + p.nv;
    int rc;
    if (!d.d_indeg && (rc = dev_alloc(c, &d.d_indeg, rows_total))) return rc;
    HB_HIP(hipMemsetAsync(d.d_indeg, 0, std::max<uint64_t>(rows_total, 1) * sizeof(uint32_t), c->stream));
    auto launch = [&](uint64_t lo, uint64_t hi) {
        const unsigned blocks = grid_blocks(c, (hi - lo + 255) / 256, 8);
        hipLaunchKernelGGL(hbk::bfs_indegree_kernel, dim3(blocks), dim3(256), 0, c->stream, (const uint64_t *)c->d_row_ptr, (const uint32_t *)c->d_src, d.d_indeg,
                           p.n_pad, rows_total, lo, hi);
    };
    for_each_virtual_level(p, true, launch); // ascending: a chunk row sums the counts of the chunk rows below it
    if (p.n_pad) launch(0, p.n_pad);
    HB_HIP(hipGetLastError());
    d.indeg_valid = true;
    return HB_OK;
}

int distances(hb_ctx *c, const hb_distance_options *opt_in, hb_distance_stats *st_out)
{
    const double t0 = now_ms();
    hb_distance_options o{};
    copy_in(opt_in, &o);
    int rc;
    if (!o.sources || !o.source_count) return fail(c, HB_ERR_INVALID, "hb_distances: no sources (source_count == 0)");
    if ((o.flags & HB_DIST_TOP_DOWN_ONLY) && (o.flags & HB_DIST_BOTTOM_UP_ONLY))
        return fail(c, HB_ERR_INVALID, "hb_distances: HB_DIST_TOP_DOWN_ONLY and HB_DIST_BOTTOM_UP_ONLY exclude each other");
    if ((o.flags & HB_DIST_WITH_MAX) && o.max_dist > 255) return fail(c, HB_ERR_INVALID, "hb_distances: max_dist > 255 (the reference's is a u8)");
    const Plan &p = c->plan;
    auto &d = c->dst;
    d.res.reset();
    hb_distance_stats st{};
    auto finish = [&]() {
        st.ms_total = now_ms() - t0;
        copy_out(st_out, st);
        return HB_OK;
    };
    std::vector<uint32_t> sids;
    resolve_sources(c, o.sources, o.source_count, &sids, &st.unknown_sources);
    if (p.n == 0) { // an empty graph: every source is unknown
        d.res.valid = true;
        return finish();
    }
    if ((rc = distance_alloc(c))) return rc;
    const bool reversed = (o.flags & HB_DIST_REVERSED) != 0;
    if (reversed && (rc = distance_indegrees(c))) return rc;
    const uint64_t n_pad = p.n_pad, rows_total = p.n_pad + p.nv;
    const uint32_t d_max = (o.flags & HB_DIST_WITH_MAX) ? std::min<uint32_t>(sample_levels(o.max_dist), 254u) : 254u; // cost + 1 < u8::MAX
    const uint64_t alpha = dist_env("HB_DIST_ALPHA", kDistAlpha), beta = dist_env("HB_DIST_BETA", kDistBeta);

    hbk::BfsParams bp{};
    bp.push_ptr = reversed ? c->d_row_ptr : c->d_out_ptr;
    bp.push_idx = reversed ? c->d_src : c->d_out_rows;
    bp.pull_ptr = reversed ? c->d_out_ptr : c->d_row_ptr;
    bp.pull_idx = reversed ? c->d_out_rows : c->d_src;
    bp.deg = reversed ? d.d_indeg : c->d_outdeg;
    bp.dist = d.d_dist;
    bp.vis = d.d_vis;
    bp.front = d.d_front;
    bp.next = d.d_next;
    bp.heavy = d.d_heavy;
    bp.heavy_cnt = d.d_heavy_cnt;
    bp.heavy_cap = 0;
    bp.cnt = d.d_cnt;
    bp.n_pad = n_pad;
    bp.rows_total = rows_total;

    HB_HIP(hipMemsetAsync(d.d_dist, 0xFF, n_pad, c->stream));
    HB_HIP(hipMemsetAsync(d.d_vis, 0, d.words_total * sizeof(uint32_t), c->stream));
    HB_HIP(hipMemsetAsync(d.d_front, 0, (n_pad / 32 + 64) * sizeof(uint32_t), c->stream));
    HB_HIP(hipMemsetAsync(d.d_cnt, 0, 256 * 4 * sizeof(unsigned long long), c->stream));
    unsigned long long *h = c->h_counters; // (pinned words of the context; hb_run rewrites them before it reads them)
    uint64_t n_f = 0, m_f = 0;
    if (!sids.empty()) {
        const char *const what = "hb_distances: seeding the sources: ";
        DevPtr<uint32_t> d_srcs;
        HB_HIP(d_srcs.alloc(sids.size()));
        HB_HIP_AS(what, hipMemcpyAsync(d_srcs.get(), sids.data(), sids.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(hbk::bfs_seed_kernel, dim3((unsigned)((sids.size() + 255) / 256)), dim3(256), 0, c->stream, (const uint32_t *)d_srcs.get(),
                           (uint32_t)sids.size(), (const uint32_t *)c->d_dev_of, bp);
        HB_HIP_AS(what, hipGetLastError());
        HB_HIP_AS(what, hipMemcpyAsync(h, d.d_cnt, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HB_HIP_AS(what, hipStreamSynchronize(c->stream));
        n_f = h[0];
        m_f = h[1];
    }
    st.frontier[0] = n_f;
    st.reached = n_f;
    uint64_t m_seen = m_f; // degree sum of the reached nodes
    uint64_t prev_n_f = 0;
    bool bottom_up = false;
    const unsigned wblocks = grid_blocks(c, (n_pad / 32 + 255) / 256, 8, 1);
    auto grid_words = [&](uint64_t lo, uint64_t hi, uint64_t words_per_block) {
        const uint64_t words = (hi - lo + 31) / 32;
        return dim3(grid_blocks(c, (words + words_per_block - 1) / words_per_block, 8, 1));
    };
    HB_HIP(hipEventRecord(c->ev[kEvStart], c->stream));
    for (uint32_t lvl = 1; lvl <= d_max && n_f; lvl++) {
        // the step: Beamer's rule, with hysteresis (a bottom-up phase ends only when the frontier is small AND shrinking)
        const uint64_t m_u = c->m_global > m_seen ? c->m_global - m_seen : 0;
        if (o.flags & HB_DIST_TOP_DOWN_ONLY) bottom_up = false;
        else if (o.flags & HB_DIST_BOTTOM_UP_ONLY) bottom_up = true;
        else if (!bottom_up) bottom_up = m_f * alpha > m_u && m_f > 0;
        else if (n_f * beta < p.n && n_f < prev_n_f) bottom_up = false;
        bp.level = lvl;
        bp.cnt = d.d_cnt + 4 * (uint64_t)lvl;
        if (!bottom_up) {
            // node rows of the frontier, then the virtual levels relay: ascending forward (a chunk feeds higher levels and its hub),
            // descending reversed (a hub feeds its chunks, a chunk the lower levels)
            bp.row_lo = 0;
            bp.row_hi = n_pad;
            bp.heavy_cap = m_f > hbk::kBfsHeavy ? d.heavy_cap : 0; // (no frontier row can be heavy otherwise)
            hipLaunchKernelGGL((hbk::bfs_push_kernel<false>), grid_words(0, n_pad, 256), dim3(256), 0, c->stream, bp);
            if (bp.heavy_cap) hipLaunchKernelGGL(hbk::bfs_push_heavy_kernel, dim3((unsigned)c->num_cu * 4), dim3(256), 0, c->stream, bp);
            bp.heavy_cap = 0;
            for_each_virtual_level(p, !reversed, [&](uint64_t lo, uint64_t hi) {
                bp.row_lo = lo;
                bp.row_hi = hi;
                hipLaunchKernelGGL((hbk::bfs_push_kernel<true>), grid_words(lo, hi, 256), dim3(256), 0, c->stream, bp);
            });
        } else {
            // the virtual rows' bits first (ascending forward: a chunk looks at its sources; descending reversed: at its readers)
            for_each_virtual_level(p, !reversed, [&](uint64_t lo, uint64_t hi) {
                bp.row_lo = lo;
                bp.row_hi = hi;
                hipLaunchKernelGGL((hbk::bfs_pull_kernel<true>), grid_words(lo, hi, 4), dim3(256), 0, c->stream, bp);
            });
            bp.row_lo = 0;
            bp.row_hi = n_pad;
            hipLaunchKernelGGL((hbk::bfs_pull_kernel<false>), grid_words(0, n_pad, 4), dim3(256), 0, c->stream, bp);
        }
        hipLaunchKernelGGL(hbk::bfs_finalize_kernel, dim3(wblocks), dim3(256), 0, c->stream, bp);
        HB_HIP(hipGetLastError());
        HB_HIP(hipMemcpyAsync(h, bp.cnt, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HB_HIP(hipStreamSynchronize(c->stream));
        prev_n_f = n_f;
        n_f = h[0];
        m_f = h[1];
        m_seen += m_f;
        st.levels = lvl;
        st.step[lvl] = bottom_up ? 1 : 0;
        st.frontier[lvl] = n_f;
        st.reached += n_f;
        st.edges_inspected += h[2];
        if (n_f) st.max_distance = lvl;
    }
    HB_HIP(hipEventRecord(c->ev[kEvEnd], c->stream));
    HB_HIP(hipStreamSynchronize(c->stream));
    float ms = 0.f;
    HB_HIP(hipEventElapsedTime(&ms, c->ev[kEvStart], c->ev[kEvEnd]));
    st.ms_levels = ms;
    d.res.count = st.reached; // (the compaction, made by the first reader, checks its own count against this one)
    d.res.valid = true;
    return finish();
}

// the result in sid order and its compacted form, on the device: once per result, made by the first reader that copies something
int distance_compact(hb_ctx *c)
{
    auto &d = c->dst;
    if (d.res.compacted) return HB_OK;
    const Plan &p = c->plan;
    hipLaunchKernelGGL(hbk::bfs_by_sid_kernel, dim3(grid_blocks(c, (p.n + 255) / 256, 8, 1)), dim3(256), 0, c->stream, (const uint8_t *)d.d_dist, (const uint32_t *)c->d_dev_of,
                       p.n, p.n_pad, d.res.d_val_sid);
    HB_HIP(hipGetLastError());
    return node_result_compact(c, d.res, "hb_distance_copy", &d.res.count, "level counters"); // (count = what the levels reached)
}

NodeResult<uint8_t> *distance_result(hb_ctx *c) { return c ? &c->dst.res : nullptr; }

const char *const kNoDistances = "no distances (call hb_distances)";

} // namespace

extern "C" {

int hb_distances(hb_ctx *c, const hb_distance_options *opt, hb_distance_stats *stats)
{
    return operator_entry(c, "hb_distances", [&]() { return distances(c, opt, stats); });
}

int hb_distance_count(hb_ctx *c, uint64_t *count) { return node_result_count(c, distance_result(c), "hb_distance_count", kNoDistances, count); }

int hb_distance_copy(hb_ctx *c, hb_u128 *ids, uint8_t *dist, uint64_t cap)
{
    return node_result_copy(c, distance_result(c), "hb_distance_copy", kNoDistances, ids, dist, cap, distance_compact);
}

int hb_distance_all(hb_ctx *c, uint8_t *dist, uint64_t cap)
{
    return node_result_all(c, distance_result(c), "hb_distance_all", "dist", kNoDistances, dist, cap, distance_compact);
}

} // extern "C"
