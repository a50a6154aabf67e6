// hb_api_betweenness.inc - part of the hb_api.hip translation unit (included at its end; uses its hb_ctx and helpers).
// hb_betweenness: Betweenness::calculate (crates/core/src/webgraph/centrality/betweenness.rs:29-146) on the loaded graph - Brandes'
// algorithm, eight sources per batch in the 64-byte rows of the HyperBall plan (kernels: hb_betweenness.hip.h).  Definitions:
// include/hyperball.h.  The walk borrows d_regs / d_part / the changed bitmaps / the sweep scratch as hb_sampled_harmonic does
// (claim_rows); everything it keeps - the per-batch state, the sums, the result - lives in buffers of its own.

namespace {

// the buffers of the operator, once per loaded graph
int betweenness_alloc(hb_ctx *c)
{
    auto &b = c->btw;
    if (b.ready) return HB_OK;
    const Plan &p = c->plan;
    const uint64_t before = c->stats.device_bytes;
    int rc;
    if ((rc = dev_alloc(c, &b.d_dist, p.n_pad * 8))) return rc;
    if ((rc = dev_alloc(c, &b.d_sigma, p.n_pad * 8))) return rc;
    if ((rc = dev_alloc(c, &b.d_delta, p.n_pad * 8))) return rc;
    if ((rc = dev_alloc(c, &b.d_reached, p.n_pad))) return rc;
    if ((rc = dev_alloc(c, &b.d_sum, p.n_pad))) return rc;
    if ((rc = dev_alloc(c, &b.d_cnt, 257 * 4))) return rc;
    if ((rc = dev_alloc(c, &b.d_srcs, hbk::kBcLanes))) return rc;
    if ((rc = node_result_alloc(c, b.res))) return rc;
    if ((rc = ensure_transpose(c, "hb_betweenness"))) return rc;
    // node rows whose reader list the grid sums: their number is the capacity of the heavy list (0 = those kernels are never launched)
    HB_HIP(hipMemsetAsync(b.d_cnt, 0, 4 * sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(hbk::bc_count_heavy_kernel, dim3(grid_blocks(c, (p.n_pad + 255) / 256, 8, 1)), dim3(256), 0, c->stream, (const uint64_t *)c->d_out_ptr, p.n_pad, b.d_cnt);
    HB_HIP(hipGetLastError());
    unsigned long long heavy = 0;
    HB_HIP(hipMemcpyAsync(&heavy, b.d_cnt, sizeof(heavy), hipMemcpyDeviceToHost, c->stream));
    HB_HIP(hipStreamSynchronize(c->stream));
    b.heavy_cap = (uint32_t)std::min<uint64_t>(heavy, 0x7FFFFFFFull);
    if (b.heavy_cap) {
        if ((rc = dev_alloc(c, &b.d_heavy, b.heavy_cap))) return rc;
        if ((rc = dev_alloc(c, &b.d_heavy_cnt, 64))) return rc;
        if ((rc = dev_alloc(c, &b.d_seg, 2 * (c->plan_entries / hbk::kBcSegment + 2) * 4))) return rc;
    }
    b.bytes = c->stats.device_bytes - before;
    b.ready = true;
    return HB_OK;
}

// the result of the finished batches in sid order, and its compacted form (only the results are downloaded)
int betweenness_extract(hb_ctx *c, uint64_t S, bool raw)
{
    auto &b = c->btw;
    const Plan &p = c->plan;
    const double s = (double)S;
    const double norm = s * (s - 1.0); // betweenness.rs:128-129
    hipLaunchKernelGGL(hbk::bc_result_kernel, dim3(grid_blocks(c, (p.n + 255) / 256, 8, 1)), dim3(256), 0, c->stream, (const double *)b.d_sum,
                       (const uint8_t *)b.d_reached, (const uint32_t *)c->d_dev_of, p.n, p.n_pad, raw ? 1 : 0, norm, b.res.d_val_sid, b.res.d_flag_sid);
    HB_HIP(hipGetLastError());
    return node_result_compact(c, b.res, "hb_betweenness"); // (no counter of the operator's own: the select says how many results there are)
}

int betweenness(hb_ctx *c, const hb_betweenness_options *opt_in, hb_betweenness_stats *st_out)
{
    const double t0 = now_ms();
    hb_betweenness_options o{};
    copy_in(opt_in, &o);
    int rc;
    if ((o.flags & HB_BC_DENSE_ONLY) && (o.flags & HB_BC_SPARSE_ONLY))
        return fail(c, HB_ERR_INVALID, "hb_betweenness: HB_BC_DENSE_ONLY and HB_BC_SPARSE_ONLY exclude each other");
    const Plan &p = c->plan;
    if (!o.sources && p.n > 100000)
        return fail(c, HB_ERR_INVALID, "hb_betweenness: sources == NULL means every node, which the reference limits to 100000 (betweenness.rs:34); name the sources");
    auto &b = c->btw;
    b.res.reset();
    b.last_lanes = 0;
    hb_betweenness_stats st{};
    // the sources as distinct ascending sids
    std::vector<uint32_t> sids;
    if (o.sources) {
        resolve_sources(c, o.sources, o.source_count, &sids, &st.unknown_sources);
    } else {
        sids.resize(p.n);
        for (uint64_t i = 0; i < p.n; i++) sids[i] = (uint32_t)i;
    }
    const uint64_t S = sids.size();
    st.sources = S;
    auto finish = [&]() {
        st.device_bytes = b.bytes;
        st.ms_total = now_ms() - t0;
        copy_out(st_out, st);
        return HB_OK;
    };
    if (p.n == 0) { // an empty graph: an empty result
        b.res.valid = true;
        return finish();
    }
    if ((rc = betweenness_alloc(c))) return rc;
    const uint64_t n_pad = p.n_pad, rows_total = p.n_pad + p.nv;
    HB_HIP(hipMemsetAsync(b.d_sum, 0, n_pad * sizeof(double), c->stream));
    HB_HIP(hipMemsetAsync(b.d_reached, 0, n_pad, c->stream));
    claim_rows(c, RowsOf::Brandes);
    unsigned long long *h = c->h_counters; // (pinned words of the context; hb_run rewrites them before it reads them)
    auto virt_grid = [&](uint64_t lo, uint64_t hi) { return dim3(grid_blocks(c, ((hi - lo + 31) / 32 + 3) / 4, 8, 1)); };
    for (uint64_t b0 = 0; b0 < S; b0 += hbk::kBcLanes) {
        const uint32_t count = (uint32_t)std::min<uint64_t>(hbk::kBcLanes, S - b0);
        st.batches++;
        b.last_lanes = count;
        // level -1: no distance anywhere, F = 0 in both buffers, no bit set; level 0: every source's own lane
        HB_HIP(hipMemsetAsync(c->d_regs[0], 0, n_pad * 64, c->stream));
        HB_HIP(hipMemsetAsync(c->d_regs[1], 0, n_pad * 64, c->stream));
        HB_HIP(hipMemsetAsync(c->d_bits[0], 0, c->bits_words * 4, c->stream));
        HB_HIP(hipMemsetAsync(c->d_bits[1], 0, c->bits_words * 4, c->stream));
        HB_HIP(hipMemsetAsync(b.d_dist, 0xFF, n_pad * 8, c->stream));
        HB_HIP(hipMemsetAsync(b.d_sigma, 0, n_pad * 64, c->stream));
        HB_HIP(hipMemsetAsync(b.d_delta, 0, n_pad * 64, c->stream));
        HB_HIP(hipMemsetAsync(b.d_cnt, 0, 257 * 4 * sizeof(unsigned long long), c->stream));
        HB_HIP(hipMemcpyAsync(b.d_srcs, sids.data() + b0, count * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        hbk::BcParams bp{};
        fill_walk_params(c, &bp);
        bp.part = (hbk::bc_u2 *)c->d_part;
        bp.dist = b.d_dist;
        bp.sigma = b.d_sigma;
        bp.reached = b.d_reached;
        bp.cnt = b.d_cnt;
        hipLaunchKernelGGL(hbk::bc_seed_kernel, dim3(1), dim3(64), 0, c->stream, (const uint32_t *)b.d_srcs, count, (const uint32_t *)c->d_dev_of,
                           (unsigned long long *)c->d_regs[0], c->d_bits[0], bp);
        HB_HIP(hipGetLastError());
        HB_HIP(hipMemcpyAsync(h, b.d_cnt, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HB_HIP(hipStreamSynchronize(c->stream));
        uint64_t last_changed = h[0], last_active = h[1];
        uint32_t L = 0; // the deepest level of this batch
        bool saturated = false;
        int cur = 0;
        for (uint32_t d = 1; d <= 255 && last_changed; d++) {
            // dense / bitmap / sweep as in hb_run (pass_mode): the A_t rule on the out-degree sum of the rows that changed at d - 1;
            // level 1 of a batch (<= 8 rows changed) is a sweep wherever the sweep support exists
            PassMode mode = (d == 1 && c->sparse_ok) ? kModeSweep : pass_mode(c, last_active);
            if (o.flags & HB_BC_DENSE_ONLY) mode = kModeDense;
            if (o.flags & HB_BC_SPARSE_ONLY) mode = c->sparse_ok ? kModeSweep : kModeBitmap;
            bp.rd = (const hbk::bc_u2 *)c->d_regs[cur];
            bp.wr = (hbk::bc_u2 *)c->d_regs[cur ^ 1];
            bp.bits_rd = c->d_bits[cur];
            bp.bits_wr = c->d_bits[cur ^ 1];
            bp.cnt = b.d_cnt + 4 * (uint64_t)d;
            bp.level = d;
            WalkLevel lv{};
            if ((rc = walk_forward_level(c, bp, mode, last_changed, [&](bool real) { launch_walk<BrandesWalk>(c, bp, real, mode); }, &lv))) return rc;
            st.levels_forward++;
            st.levels_mode[mode]++;
            st.ms_mode[mode] += lv.ms;
            st.ms_forward += lv.ms;
            if (mode == kModeDense) st.ms_dense_max = std::max(st.ms_dense_max, (double)lv.ms);
            st.edges_gathered += lv.cnt[2];
            last_changed = lv.cnt[0];
            last_active = lv.cnt[1];
            saturated = saturated || lv.cnt[3] != 0;
            if (last_changed) L = d;
            cur ^= 1;
        }
        // nothing is truncated: a truncated betweenness would be wrong
        if (L == 255) return fail(c, HB_ERR_LIMIT, "hb_betweenness: a shortest path longer than 254 edges (the distances are bytes)");
        if (saturated) return fail(c, HB_ERR_LIMIT, "hb_betweenness: a shortest-path count reached 2^64 - 1");
        st.max_dist = std::max(st.max_dist, L);

        // backward: level d gives the sources at dist == d - 1 their delta; C double buffered in the F buffers, the bits in the changed bitmaps
        HB_HIP(hipMemsetAsync(c->d_bits[0], 0, c->bits_words * 4, c->stream));
        HB_HIP(hipMemsetAsync(c->d_bits[1], 0, c->bits_words * 4, c->stream));
        hbk::BcBackParams kp{};
        kp.out_ptr = c->d_out_ptr;
        kp.out_rows = c->d_out_rows;
        kp.cpart = (hbk::bc_d2 *)c->d_part;
        kp.dist = b.d_dist;
        kp.sigma = b.d_sigma;
        kp.delta = b.d_delta;
        kp.heavy = b.d_heavy;
        kp.heavy_cnt = b.d_heavy_cnt;
        kp.heavy_cap = b.heavy_cap;
        kp.seg = b.d_seg;
        kp.n_pad = n_pad;
        kp.rows_total = rows_total;
        HB_HIP(hipEventRecord(c->ev[kEvStart], c->stream));
        int cb = 0;
        for (uint32_t d = L + 1; d >= 1; d--) {
            kp.crd = (const hbk::bc_d2 *)c->d_regs[cb];
            kp.cwr = (hbk::bc_d2 *)c->d_regs[cb ^ 1];
            kp.bits_rd = c->d_bits[cb];
            kp.bits_wr = c->d_bits[cb ^ 1];
            kp.level = d;
            kp.row_lo = 0;
            kp.row_hi = n_pad;
            if (kp.heavy_cap) HB_HIP(hipMemsetAsync(kp.heavy_cnt, 0, sizeof(unsigned int), c->stream));
            hipLaunchKernelGGL(hbk::bc_back_node_kernel, virt_grid(0, n_pad), dim3(256), 0, c->stream, kp);
            if (kp.heavy_cap) {
                hipLaunchKernelGGL(hbk::bc_back_heavy_partial_kernel, dim3((unsigned)c->num_cu * 4), dim3(256), 0, c->stream, kp);
                hipLaunchKernelGGL(hbk::bc_back_heavy_finish_kernel, dim3((kp.heavy_cap * 4 + 255) / 256), dim3(256), 0, c->stream, kp);
            }
            if (d > 1) { // the coefficients of level d - 1 down the chunk trees: the highest virtual level first
                for_each_virtual_level(p, false, [&](uint64_t lo, uint64_t hi) {
                    kp.row_lo = lo;
                    kp.row_hi = hi;
                    hipLaunchKernelGGL(hbk::bc_back_virt_kernel, virt_grid(lo, hi), dim3(256), 0, c->stream, kp, (const hbk::bc_d2 *)c->d_regs[cb ^ 1], c->d_bits[cb ^ 1]);
                });
            }
            HB_HIP(hipGetLastError());
            st.levels_backward++;
            cb ^= 1;
        }
        hipLaunchKernelGGL(hbk::bc_accumulate_kernel, dim3(grid_blocks(c, (n_pad + 255) / 256, 8, 1)), dim3(256), 0, c->stream, (const uint8_t *)b.d_dist,
                           (const double *)b.d_delta, n_pad, b.d_sum);
        HB_HIP(hipGetLastError());
        HB_HIP(hipEventRecord(c->ev[kEvEnd], c->stream));
        HB_HIP(hipStreamSynchronize(c->stream));
        float ms = 0.f;
        HB_HIP(hipEventElapsedTime(&ms, c->ev[kEvStart], c->ev[kEvEnd]));
        st.ms_backward += ms;
    }
    if ((rc = betweenness_extract(c, S, (o.flags & HB_BC_RAW) != 0))) return rc;
    st.results = b.res.count;
    b.res.valid = true;
    return finish();
}

const char *const kNoBetweenness = "no betweenness result (call hb_betweenness)";

NodeResult<double> *betweenness_result(hb_ctx *c) { return c ? &c->btw.res : nullptr; }

} // namespace

extern "C" {

int hb_betweenness(hb_ctx *c, const hb_betweenness_options *opt, hb_betweenness_stats *stats)
{
    return operator_entry(c, "hb_betweenness", [&]() { return betweenness(c, opt, stats); });
}

int hb_betweenness_count(hb_ctx *c, uint64_t *count) { return node_result_count(c, betweenness_result(c), "hb_betweenness_count", kNoBetweenness, count); }

int hb_betweenness_copy(hb_ctx *c, hb_u128 *ids, double *vals, uint64_t cap)
{
    return node_result_copy(c, betweenness_result(c), "hb_betweenness_copy", kNoBetweenness, ids, vals, cap);
}

int hb_betweenness_all(hb_ctx *c, double *vals, uint64_t cap)
{
    return node_result_all(c, betweenness_result(c), "hb_betweenness_all", "vals", kNoBetweenness, vals, cap);
}

int hb_debug_copy_betweenness_batch(hb_ctx *c, uint8_t *dist, uint64_t *sigma, double *delta)
{
    return reader_entry(c, c && c->btw.res.valid, "hb_debug_copy_betweenness_batch", kNoBetweenness, [&]() -> int {
        const Plan &p = c->plan;
        auto &b = c->btw;
        if (!p.n) return HB_OK;
        if (!b.last_lanes) return fail(c, HB_ERR_INVALID, "hb_debug_copy_betweenness_batch: the last hb_betweenness ran no batch (no known source)");
        std::vector<uint32_t> sid_of(p.n_pad);
        std::vector<uint8_t> h_dist(p.n_pad * 8);
        std::vector<uint64_t> h_sigma(p.n_pad * 8);
        std::vector<double> h_delta(p.n_pad * 8);
        HB_HIP(hipMemcpyAsync(sid_of.data(), c->d_sid_of, p.n_pad * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HB_HIP(hipMemcpyAsync(h_dist.data(), b.d_dist, p.n_pad * 8, hipMemcpyDeviceToHost, c->stream));
        HB_HIP(hipMemcpyAsync(h_sigma.data(), b.d_sigma, p.n_pad * 64, hipMemcpyDeviceToHost, c->stream));
        HB_HIP(hipMemcpyAsync(h_delta.data(), b.d_delta, p.n_pad * 64, hipMemcpyDeviceToHost, c->stream));
        HB_HIP(hipStreamSynchronize(c->stream));
        for (uint64_t r = 0; r < p.n_pad; r++) {
            const uint32_t sid = sid_of[r];
            if (sid == kNone) continue;
            for (uint32_t l = 0; l < hbk::kBcLanes; l++) {
                if (dist) dist[(uint64_t)sid * 8 + l] = h_dist[r * 8 + l];
                if (sigma) sigma[(uint64_t)sid * 8 + l] = h_sigma[r * 8 + l];
                if (delta) delta[(uint64_t)sid * 8 + l] = h_delta[r * 8 + l];
            }
        }
        return HB_OK;
    });
}

} // extern "C"
