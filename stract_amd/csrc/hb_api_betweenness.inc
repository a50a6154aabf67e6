// hb_api_betweenness.inc - part of the hb_api.hip translation unit (included at its end; uses its hb_ctx and helpers).
// hb_betweenness: Betweenness::calculate (crates/core/src/webgraph/centrality/betweenness.rs:29-146) on the loaded graph - Brandes'
// algorithm, eight sources per batch in the 64-byte rows of the HyperBall plan (kernels: hb_betweenness.hip.h).  Definitions:
// include/hyperball.h.  The walk borrows d_regs / d_part / the changed bitmaps / the sweep scratch as hb_sampled_harmonic does (hb_begin
// rewrites them); everything it keeps - the per-batch state, the sums, the result - lives in buffers of its own.

namespace {

// the buffers of the operator, once per loaded graph
int betweenness_alloc(hb_ctx *c)
{
    auto &b = c->btw;
    if (b.ready) return HB_OK;
    const Plan &p = c->plan;
    const uint64_t rows_total = p.n_pad + p.nv;
    const uint64_t before = c->stats.device_bytes;
    int rc;
    if ((rc = dev_alloc(c, &b.d_dist, p.n_pad * 8))) return rc;
    if ((rc = dev_alloc(c, &b.d_sigma, p.n_pad * 8))) return rc;
    if ((rc = dev_alloc(c, &b.d_delta, p.n_pad * 8))) return rc;
    if ((rc = dev_alloc(c, &b.d_reached, p.n_pad))) return rc;
    if ((rc = dev_alloc(c, &b.d_sum, p.n_pad))) return rc;
    if ((rc = dev_alloc(c, &b.d_cnt, 257 * 4))) return rc;
    if ((rc = dev_alloc(c, &b.d_srcs, hbk::kBcLanes))) return rc;
    if ((rc = dev_alloc(c, &b.d_val_sid, p.n))) return rc;
    if ((rc = dev_alloc(c, &b.d_flag_sid, p.n))) return rc;
    if ((rc = dev_alloc(c, &b.d_sel_sid, p.n))) return rc;
    if ((rc = dev_alloc(c, &b.d_sel_flag, p.n))) return rc;
    if ((rc = dev_alloc(c, &b.d_sel_val, p.n))) return rc;
    if ((rc = dev_alloc(c, &b.d_sel_cnt, 8))) return rc;
    if (c->sparse_ok) { // the sweep passes' transpose
        b.d_out_ptr = c->d_out_ptr;
        b.d_out_rows = c->d_out_rows;
    } else if (c->dst.ready) { // hb_distances built one for the same reason
        b.d_out_ptr = c->dst.d_out_ptr;
        b.d_out_rows = c->dst.d_out_rows;
    } else { // a context without sweep support (HB_FLAG_NO_SPARSE, unfused passes): the same transpose, owned by this state
        uint64_t *op = nullptr;
        uint32_t *orow = nullptr;
        if ((rc = dev_alloc(c, &op, rows_total + 1))) return rc;
        if ((rc = dev_alloc(c, &orow, c->plan_entries))) return rc;
        const std::string e = gpu_transpose_rows((void *)c->stream, c->d_row_ptr, c->d_src, rows_total, c->plan_entries, op, orow);
        if (!e.empty()) return fail(c, e.find("out of memory") != std::string::npos ? HB_ERR_NOMEM : HB_ERR_HIP, "hb_betweenness: " + e);
        b.d_out_ptr = op;
        b.d_out_rows = orow;
    }
    // node rows whose reader list the grid sums: their number is the capacity of the heavy list (0 = those kernels are never launched)
    HB_HIP(hipMemsetAsync(b.d_cnt, 0, 4 * sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(hbk::bc_count_heavy_kernel, dim3(grid_blocks(c, (p.n_pad + 255) / 256, 8, 1)), dim3(256), 0, c->stream, b.d_out_ptr, p.n_pad, b.d_cnt);
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

// launch shape of one forward level: a wave per 32-row word, grid-stride; XCD-affine groups for the first hub-chunk level (as the
// sampled walk's)
void betweenness_launch(hb_ctx *c, const hbk::BcParams &bp, bool real, int mode)
{
    const uint64_t words = (bp.row_hi - bp.row_lo + 31) / 32;
    if (!words) return;
    uint64_t blocks = std::min<uint64_t>((words + 3) / 4, (uint64_t)c->num_cu * 8);
    if (bp.xcd_map) blocks = std::max<uint64_t>((blocks + 7) / 8 * 8, 8);
    const dim3 grid((unsigned)blocks), blk(256);
#define HB_BC_LAUNCH(R, M) hipLaunchKernelGGL((hbk::bc_forward_kernel<R, M>), grid, blk, 0, c->stream, bp)
    if (real) {
        if (mode == hbk::kBcDense) HB_BC_LAUNCH(true, hbk::kBcDense);
        else if (mode == hbk::kBcBitmap) HB_BC_LAUNCH(true, hbk::kBcBitmap);
        else HB_BC_LAUNCH(true, hbk::kBcSweep);
    } else {
        if (mode == hbk::kBcDense) HB_BC_LAUNCH(false, hbk::kBcDense);
        else if (mode == hbk::kBcBitmap) HB_BC_LAUNCH(false, hbk::kBcBitmap);
        else HB_BC_LAUNCH(false, hbk::kBcSweep);
    }
#undef HB_BC_LAUNCH
}

// the result of the finished batches in sid order, and its compacted form (only the results are downloaded)
int betweenness_extract(hb_ctx *c, uint64_t S, bool raw)
{
    auto &b = c->btw;
    const Plan &p = c->plan;
    const double s = (double)S;
    const double norm = s * (s - 1.0); // betweenness.rs:128-129
    hipLaunchKernelGGL(hbk::bc_result_kernel, dim3(grid_blocks(c, (p.n + 255) / 256, 8, 1)), dim3(256), 0, c->stream, (const double *)b.d_sum,
                       (const uint8_t *)b.d_reached, (const uint32_t *)c->d_dev_of, p.n, p.n_pad, raw ? 1 : 0, norm, b.d_val_sid, b.d_flag_sid);
    HB_HIP(hipGetLastError());
    const std::string e = gpu_select_reached((void *)c->stream, b.d_flag_sid, p.n, b.d_sel_sid, b.d_sel_flag, b.d_sel_cnt);
    if (!e.empty()) return fail(c, HB_ERR_HIP, "hb_betweenness: " + e);
    uint64_t got = 0;
    HB_HIP(hipMemcpyAsync(&got, b.d_sel_cnt, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HB_HIP(hipStreamSynchronize(c->stream));
    if (got) {
        hipLaunchKernelGGL(hbk::bc_gather_kernel, dim3(grid_blocks(c, (got + 255) / 256, 8, 1)), dim3(256), 0, c->stream, (const double *)b.d_val_sid,
                           (const uint32_t *)b.d_sel_sid, got, b.d_sel_val);
        HB_HIP(hipGetLastError());
        HB_HIP(hipStreamSynchronize(c->stream));
    }
    b.results = got;
    return HB_OK;
}

int betweenness(hb_ctx *c, const hb_betweenness_options *opt_in, hb_betweenness_stats *st_out)
{
    const double t0 = now_ms();
    hb_betweenness_options o{};
    copy_in(opt_in, &o);
    if (multi_rank(c)) return fail(c, HB_ERR_INVALID, "hb_betweenness: single rank only (world_size > 1)");
    if (!c->loaded) return fail(c, HB_ERR_INVALID, "hb_betweenness: no graph loaded");
    if ((o.flags & HB_BC_DENSE_ONLY) && (o.flags & HB_BC_SPARSE_ONLY))
        return fail(c, HB_ERR_INVALID, "hb_betweenness: HB_BC_DENSE_ONLY and HB_BC_SPARSE_ONLY exclude each other");
    const Plan &p = c->plan;
    if (!o.sources && p.n > 100000)
        return fail(c, HB_ERR_INVALID, "hb_betweenness: sources == NULL means every node, which the reference limits to 100000 (betweenness.rs:34); name the sources");
    int rc;
    if ((rc = plan_rows_word_aligned(c, "hb_betweenness"))) return rc;
    for (uint64_t lb : p.level_begin)
        if (lb < p.n_pad || lb > p.n_pad + p.nv) return fail(c, HB_ERR_INVALID, "hb_betweenness: unexpected plan layout (virtual level boundary)");
    if ((rc = refuse_stale_error(c, "hb_betweenness"))) return rc;
    auto &b = c->btw;
    b.valid = false;
    b.results = 0;
    b.last_lanes = 0;
    hb_betweenness_stats st{};
    // the sources as distinct ascending sids
    std::vector<uint32_t> sids;
    if (o.sources) {
        sids.reserve(o.source_count);
        for (uint64_t i = 0; i < o.source_count; i++) {
            uint32_t sid;
            if (find_sid(c, o.sources[i], &sid)) sids.push_back(sid);
            else st.unknown_sources++;
        }
        std::sort(sids.begin(), sids.end());
        sids.erase(std::unique(sids.begin(), sids.end()), sids.end());
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
        b.valid = true;
        return finish();
    }
    if ((rc = betweenness_alloc(c))) return rc;
    const uint64_t n_pad = p.n_pad, rows_total = p.n_pad + p.nv;
    const size_t nlev = p.level_begin.size() > 1 ? p.level_begin.size() - 1 : 0;
    const bool xcd_ok = p.xcd_groups == 8 && p.level_begin.size() > 1 && p.xcd_begin[0] == p.level_begin[0] && p.xcd_begin[8] == p.level_begin[1] &&
                        std::all_of(p.xcd_begin, p.xcd_begin + 9, [](uint64_t x) { return x % 32 == 0; });
    HB_HIP(hipMemsetAsync(b.d_sum, 0, n_pad * sizeof(double), c->stream));
    HB_HIP(hipMemsetAsync(b.d_reached, 0, n_pad, c->stream));
    // from here on the HyperBall state is gone: hb_step needs a new hb_begin, the tail kernel's lists describe nothing
    c->begun = false;
    c->tl_valid = false;
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
        bp.row_ptr = c->d_row_ptr;
        bp.src = c->d_src;
        bp.part = (hbk::bc_u2 *)c->d_part;
        bp.touch = c->d_touch;
        bp.out_ptr = b.d_out_ptr;
        bp.out_rows = b.d_out_rows;
        bp.outdeg = c->d_outdeg;
        bp.dist = b.d_dist;
        bp.sigma = b.d_sigma;
        bp.reached = b.d_reached;
        bp.cnt = b.d_cnt;
        bp.n_pad = n_pad;
        bp.rows_total = rows_total;
        for (int x = 0; x < 8; x++) {
            bp.xcd_lo[x] = p.xcd_begin[x];
            bp.xcd_hi[x] = p.xcd_begin[x + 1];
        }
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
            static_assert(hbk::kBcDense == kModeDense && hbk::kBcBitmap == kModeBitmap && hbk::kBcSweep == kModeSweep, "one numbering of the modes");
            int mode = (d == 1 && c->sparse_ok) ? hbk::kBcSweep : (int)pass_mode(c, last_active);
            if (o.flags & HB_BC_DENSE_ONLY) mode = hbk::kBcDense;
            if (o.flags & HB_BC_SPARSE_ONLY) mode = c->sparse_ok ? hbk::kBcSweep : hbk::kBcBitmap;
            bp.rd = (const hbk::bc_u2 *)c->d_regs[cur];
            bp.wr = (hbk::bc_u2 *)c->d_regs[cur ^ 1];
            bp.bits_rd = c->d_bits[cur];
            bp.bits_wr = c->d_bits[cur ^ 1];
            bp.cnt = b.d_cnt + 4 * (uint64_t)d;
            bp.level = d;
            HB_HIP(hipEventRecord(c->ev[kEvStart], c->stream));
            if (mode == hbk::kBcSweep) {
                // the rows changed at d - 1 -> touch bits of their readers: hb_run's seed / expand kernels, unchanged (launch_sweep_seeding)
                hbk::PassParams seed_pp{}; // (all the seeding kernels read of it)
                seed_pp.bits_rd = c->d_bits[cur];
                seed_pp.n_pad = n_pad;
                seed_pp.rows_total = rows_total;
                HB_HIP(hipMemsetAsync(c->d_sparse_counts, 0, 4 * sizeof(unsigned int), c->stream));
                launch_sweep_seeding(c, make_sweep_params(c, seed_pp, 0, nullptr), last_changed <= 4096);
                HB_HIP(hipGetLastError());
            }
            for (size_t l = 0; l < nlev; l++) { // virtual levels: partials of level d from the rows of level d - 1
                bp.row_lo = p.level_begin[l];
                bp.row_hi = p.level_begin[l + 1];
                bp.xcd_map = (l == 0 && xcd_ok && mode == hbk::kBcDense) ? 1 : 0;
                betweenness_launch(c, bp, false, mode);
            }
            bp.xcd_map = 0;
            bp.row_lo = 0;
            bp.row_hi = n_pad;
            betweenness_launch(c, bp, true, mode);
            HB_HIP(hipGetLastError());
            HB_HIP(hipEventRecord(c->ev[kEvEnd], c->stream));
            HB_HIP(hipMemcpyAsync(h, bp.cnt, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
            HB_HIP(hipStreamSynchronize(c->stream));
            float ms = 0.f;
            HB_HIP(hipEventElapsedTime(&ms, c->ev[kEvStart], c->ev[kEvEnd]));
            st.levels_forward++;
            st.levels_mode[mode]++;
            st.ms_mode[mode] += ms;
            st.ms_forward += ms;
            if (mode == hbk::kBcDense) st.ms_dense_max = std::max(st.ms_dense_max, (double)ms);
            st.edges_gathered += h[2];
            last_changed = h[0];
            last_active = h[1];
            saturated = saturated || h[3] != 0;
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
        kp.out_ptr = b.d_out_ptr;
        kp.out_rows = b.d_out_rows;
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
                for (size_t k = 0; k < nlev; k++) {
                    const size_t l = nlev - 1 - k;
                    kp.row_lo = p.level_begin[l];
                    kp.row_hi = p.level_begin[l + 1];
                    if (kp.row_hi > kp.row_lo)
                        hipLaunchKernelGGL(hbk::bc_back_virt_kernel, virt_grid(kp.row_lo, kp.row_hi), dim3(256), 0, c->stream, kp, (const hbk::bc_d2 *)c->d_regs[cb ^ 1],
                                           c->d_bits[cb ^ 1]);
                }
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
    st.results = b.results;
    b.valid = true;
    return finish();
}

int betweenness_result_ready(hb_ctx *c, const char *who)
{
    if (!c->loaded || !c->btw.valid) return fail(c, HB_ERR_INVALID, std::string(who) + ": no betweenness result (call hb_betweenness)");
    return set_device(c);
}

} // namespace

extern "C" {

int hb_betweenness(hb_ctx *c, const hb_betweenness_options *opt, hb_betweenness_stats *stats)
{
    return guarded(c, [&]() -> int {
        if (!c) return HB_ERR_INVALID;
        int rc = set_device(c);
        if (rc) return rc;
        // between hb_begin and hb_finish the HyperBall state (and the pinned counter words) belong to that run
        if (c->begun && !c->finished) return fail(c, HB_ERR_INVALID, "hb_betweenness: a HyperBall run is in progress (hb_begin without hb_finish)");
        return betweenness(c, opt, stats);
    });
}

int hb_betweenness_count(hb_ctx *c, uint64_t *count)
{
    return guarded(c, [&]() -> int {
        if (!c || !count) return c ? fail(c, HB_ERR_INVALID, "hb_betweenness_count: count == NULL") : HB_ERR_INVALID;
        int rc = betweenness_result_ready(c, "hb_betweenness_count");
        if (rc) return rc;
        *count = c->btw.results;
        return HB_OK;
    });
}

int hb_betweenness_copy(hb_ctx *c, hb_u128 *ids, double *vals, uint64_t cap)
{
    return guarded(c, [&]() -> int {
        if (!c) return HB_ERR_INVALID;
        int rc = betweenness_result_ready(c, "hb_betweenness_copy");
        if (rc) return rc;
        auto &b = c->btw;
        const uint64_t k = std::min<uint64_t>(cap, b.results);
        if (!k || (!ids && !vals)) return HB_OK;
        // only the results come down: k sids and k values; the ids are looked up in the host's sorted id array
        if (ids) {
            std::vector<uint32_t> sid(k);
            HB_HIP(hipMemcpyAsync(sid.data(), b.d_sel_sid, k * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
            HB_HIP(hipStreamSynchronize(c->stream));
            for (uint64_t i = 0; i < k; i++) ids[i] = c->g.ids[sid[i]];
        }
        if (vals) {
            HB_HIP(hipMemcpyAsync(vals, b.d_sel_val, k * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            HB_HIP(hipStreamSynchronize(c->stream));
        }
        return HB_OK;
    });
}

int hb_betweenness_all(hb_ctx *c, double *vals, uint64_t cap)
{
    return guarded(c, [&]() -> int {
        if (!c || !vals) return c ? fail(c, HB_ERR_INVALID, "hb_betweenness_all: vals == NULL") : HB_ERR_INVALID;
        int rc = betweenness_result_ready(c, "hb_betweenness_all");
        if (rc) return rc;
        const uint64_t n = c->plan.n;
        if (cap < n) return fail(c, HB_ERR_INVALID, "hb_betweenness_all: cap < n");
        if (!n) return HB_OK;
        HB_HIP(hipMemcpyAsync(vals, c->btw.d_val_sid, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HB_HIP(hipStreamSynchronize(c->stream));
        return HB_OK;
    });
}

int hb_debug_copy_betweenness_batch(hb_ctx *c, uint8_t *dist, uint64_t *sigma, double *delta)
{
    return guarded(c, [&]() -> int {
        if (!c) return HB_ERR_INVALID;
        int rc = betweenness_result_ready(c, "hb_debug_copy_betweenness_batch");
        if (rc) return rc;
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
