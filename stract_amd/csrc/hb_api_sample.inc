// hb_api_sample.inc - part of the hb_api.hip translation unit (included at its end; uses its hb_ctx and helpers).
// hb_sampled_harmonic: ApproxHarmonic::build (crates/core/src/webgraph/centrality/approx_harmonic.rs:40-89) on the loaded graph.
// The reference runs k single-source dijkstra_multi walks (shortest_path.rs:57-103, max_dist 7) over ForwardlinksQuery lookups
// (query/forwardlink.rs:44-53); here all k walks run at once, 512 per batch, as one bit per source in the 64-byte rows of the
// HyperBall plan (kernels: hb_sample.hip.h).  Definitions: include/hyperball.h.

namespace {

// dijkstra_multi returns when it POPS a cost above max_dist; by then the nodes one hop further have already been inserted into its
// map (shortest_path.rs:85-95), and approx_harmonic.rs:62-70 counts every entry but the source.  So distances 1 .. max_dist + 1 count.
uint32_t sample_levels(uint32_t max_dist) { return max_dist + 1; }

// splitmix64 (Steele, Lea, Flood 2014): the sampler's generator
uint64_t splitmix64_next(uint64_t &state)
{
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// k = ceil(log2(N) / eps^2) (approx_harmonic.rs:49), with Rust's saturating float -> integer cast (NaN / negative -> 0)
uint64_t sample_count_formula(uint64_t num_nodes, double eps)
{
    const double x = std::ceil(std::log2((double)num_nodes) / (eps * eps));
    if (!(x > 0.0)) return 0;
    if (x >= 18446744073709551615.0) return ~0ull;
    return (uint64_t)x;
}

// the seeded sampler: candidates = nodes with an out-edge (page_edges().map(from).unique(): self links count), ascending NodeID;
// min(k, candidates) distinct indices by Floyd's algorithm, index j = splitmix64() % (i + 1); the chosen sids, ascending
int sample_sids(hb_ctx *c, uint64_t seed, uint64_t k, std::vector<uint32_t> *sids)
{
    const Plan &p = c->plan;
    sids->clear();
    if (!p.n || !k) return HB_OK;
    auto &sm = c->smp;
    if (!sm.cand_valid) { // once per loaded graph: one flag byte per node from the device, then the ascending list
        std::vector<uint8_t> has_out(p.n);
        DevPtr<uint8_t> d_flags;
        HB_HIP(d_flags.alloc(p.n));
        const unsigned blocks = grid_blocks(c, (p.n_pad + 255) / 256, 8);
        hipLaunchKernelGGL(hbk::sample_candidates_kernel, dim3(blocks), dim3(256), 0, c->stream, (const uint32_t *)c->d_outdeg, (const uint32_t *)c->d_sid_of,
                           p.n_pad, d_flags.get());
        HB_HIP_AS("hb_sampled_harmonic: candidate flags: ", hipGetLastError());
        HB_HIP_AS("hb_sampled_harmonic: candidate flags: ", hipMemcpyAsync(has_out.data(), d_flags.get(), p.n, hipMemcpyDeviceToHost, c->stream));
        HB_HIP_AS("hb_sampled_harmonic: candidate flags: ", hipStreamSynchronize(c->stream));
        sm.cand.clear();
        for (uint64_t s = 0; s < p.n; s++)
            if (has_out[s]) sm.cand.push_back((uint32_t)s);
        sm.cand_valid = true;
    }
    const std::vector<uint32_t> &cand = sm.cand;
    const uint64_t C = cand.size(), K = std::min<uint64_t>(k, C);
    // Floyd: K distinct indices out of C with K draws (a set of the taken ones: K <= 65535 is small next to C)
    std::vector<uint64_t> taken;
    taken.reserve(K);
    auto has = [&](uint64_t x) { return std::find(taken.begin(), taken.end(), x) != taken.end(); };
    std::vector<uint8_t> seen; // (membership by bytes when K is large)
    const bool dense = K > 4096;
    if (dense) seen.assign(C, 0);
    uint64_t state = seed;
    for (uint64_t i = C - K; i < C; i++) {
        const uint64_t j = splitmix64_next(state) % (i + 1);
        const bool j_taken = dense ? seen[j] != 0 : has(j);
        const uint64_t pick = j_taken ? i : j;
        taken.push_back(pick);
        if (dense) seen[pick] = 1;
    }
    std::sort(taken.begin(), taken.end());
    for (uint64_t i : taken) sids->push_back(cand[i]);
    return HB_OK;
}

int sample_alloc(hb_ctx *c, uint32_t levels)
{
    auto &s = c->smp;
    const uint64_t n_pad = c->plan.n_pad;
    if (s.levels != levels) s.d_hist.reset(); // (another level count: another size)
    s.levels = 0;
    if (!s.d_hist) HB_HIP(s.d_hist.alloc(std::max<uint64_t>((uint64_t)levels * n_pad, 64)));
    if (!s.d_cnt) HB_HIP(s.d_cnt.alloc((hbk::kSampleMaxLevels + 1) * 4));
    if (!s.d_srcs) HB_HIP(s.d_srcs.alloc(hbk::kSampleBatch));
    if (!s.d_rows) HB_HIP(s.d_rows.alloc(hbk::kSampleBatch));
    if (!s.d_w) HB_HIP(s.d_w.alloc(hbk::kSampleMaxLevels));
    return HB_OK;
}

int sampled_harmonic(hb_ctx *c, const hb_sample_options *opt_in, hb_sample_stats *st_out)
{
    const double t0 = now_ms();
    hb_sample_options o{};
    copy_in(opt_in, &o);
    int rc;
    c->smp.levels = 0; // (no histogram while this call runs, and none after a refusal; an earlier result image stays until take_image)
    const uint32_t max_dist = o.max_dist ? o.max_dist : 7; // approx_harmonic.rs:62
    if (max_dist > hbk::kSampleMaxLevels - 1) return fail(c, HB_ERR_LIMIT, "hb_sampled_harmonic: max_dist > 15");
    const uint32_t D = sample_levels(max_dist);
    const Plan &p = c->plan;
    const uint64_t N = o.num_nodes ? o.num_nodes : p.n;
    const double eps = o.epsilon != 0.0 ? o.epsilon : 0.3; // approx_harmonic.rs:29
    if (o.sources && !o.source_count) return fail(c, HB_ERR_INVALID, "hb_sampled_harmonic: sources given with source_count == 0");
    const uint64_t k_req = o.samples ? o.samples : (o.sources ? o.source_count : sample_count_formula(N, eps));
    if (k_req > 65535 || (o.sources && o.source_count > 65535)) return fail(c, HB_ERR_LIMIT, "hb_sampled_harmonic: more than 65535 sources");
    // the sources, as ascending sids
    std::vector<uint32_t> sids;
    if (o.sources) {
        uint64_t unknown = 0, first_unknown = 0;
        resolve_sources(c, o.sources, o.source_count, &sids, &unknown, &first_unknown);
        if (unknown) return fail(c, HB_ERR_INVALID, "hb_sampled_harmonic: source " + std::to_string(first_unknown) + " is not a node of the graph");
        if (sids.size() != o.source_count) return fail(c, HB_ERR_INVALID, "hb_sampled_harmonic: duplicate sources");
    } else if ((rc = sample_sids(c, o.seed, k_req, &sids))) {
        return rc;
    }
    if ((rc = take_image(c))) return rc; // (every refusal lies above: a refused call leaves the earlier result where it is)
    // weights, f32 exactly as approx_harmonic.rs:57,69 writes them (norm from the REQUESTED sample count)
    const float norm = (float)N / ((float)k_req * ((float)N - 1.0f));
    double w[hbk::kSampleMaxLevels] = {0};
    for (uint32_t d = 1; d <= D; d++) w[d - 1] = (double)((1.0f / (float)d) * norm);
    if ((rc = sample_alloc(c, D))) return rc;
    auto &sm = c->smp;
    const uint64_t n_pad = p.n_pad;
    HB_HIP(hipMemsetAsync(sm.d_hist.get(), 0, std::max<uint64_t>((uint64_t)D * n_pad, 64) * sizeof(uint16_t), c->stream));
    HB_HIP(hipMemcpyAsync(sm.d_w.get(), w, sizeof(w), hipMemcpyHostToDevice, c->stream));
    hb_sample_stats st{};
    st.levels = D;
    st.k_req = k_req;
    st.sources = sids.size();
    const uint64_t S = sids.size();
    unsigned long long *h = c->h_counters; // (pinned words of the context; hb_run rewrites them before it reads them)
    claim_rows(c, RowsOf::Sampled);
    for (uint64_t b0 = 0; b0 < S; b0 += hbk::kSampleBatch) {
        const uint32_t count = (uint32_t)std::min<uint64_t>(hbk::kSampleBatch, S - b0);
        st.batches++;
        // level -1 = all rows empty (both buffers, the partials, the changed bits); level 0 = every source's own bit
        HB_HIP(hipMemsetAsync(c->d_regs[0], 0, n_pad * 64, c->stream));
        HB_HIP(hipMemsetAsync(c->d_regs[1], 0, n_pad * 64, c->stream));
        if (p.nv) HB_HIP(hipMemsetAsync(c->d_part, 0, p.nv * 64, c->stream));
        HB_HIP(hipMemsetAsync(c->d_bits[0], 0, c->bits_words * 4, c->stream));
        HB_HIP(hipMemsetAsync(c->d_bits[1], 0, c->bits_words * 4, c->stream));
        HB_HIP(hipMemsetAsync(sm.d_cnt.get(), 0, (hbk::kSampleMaxLevels + 1) * 4 * sizeof(unsigned long long), c->stream));
        HB_HIP(hipMemcpyAsync(sm.d_srcs.get(), sids.data() + b0, count * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(hbk::sample_rows_of_kernel, dim3((count + 255) / 256), dim3(256), 0, c->stream, (const uint32_t *)sm.d_srcs.get(), count,
                           (const uint32_t *)c->d_dev_of, sm.d_rows.get()); // (only the sources' rows: no n-entry map to the host)
        hipLaunchKernelGGL(hbk::sample_seed_kernel, dim3((count * 4 + 255) / 256), dim3(256), 0, c->stream, (const uint32_t *)sm.d_rows.get(), count, c->d_regs[0],
                           c->d_bits[0], (const uint32_t *)c->d_outdeg, sm.d_cnt.get());
        HB_HIP(hipGetLastError());
        HB_HIP(hipMemcpyAsync(h, sm.d_cnt.get(), 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HB_HIP(hipStreamSynchronize(c->stream));
        uint64_t last_changed = h[0], last_active = h[1];
        hbk::SampleParams sp{};
        fill_walk_params(c, &sp);
        sp.part = c->d_part;
        int cur = 0;
        for (uint32_t d = 1; d <= D && last_changed; d++) {
            // dense / bitmap / sweep as in hb_run (pass_mode): the A_t rule on the out-degree sum of the rows changed at d - 1
            const PassMode mode = pass_mode(c, last_active);
            sp.rd = c->d_regs[cur];
            sp.wr = c->d_regs[cur ^ 1];
            sp.bits_rd = c->d_bits[cur];
            sp.bits_wr = c->d_bits[cur ^ 1];
            sp.hist = sm.d_hist.get() + (uint64_t)(d - 1) * n_pad;
            sp.cnt = sm.d_cnt.get() + 4 * d;
            WalkLevel lv{};
            if ((rc = walk_forward_level(c, sp, mode, last_changed, [&](bool real) { launch_walk<SampleWalk>(c, sp, real, mode); }, &lv))) return rc;
            st.level_changed[d - 1] += lv.cnt[0];
            st.level_modes[d - 1] |= 1u << mode;
            st.level_ms[d - 1] += lv.ms;
            last_changed = lv.cnt[0]; // no node row grew: nothing can change at d + 1 either (the batch has converged)
            last_active = lv.cnt[1];
            cur ^= 1;
        }
    }
    // the result image
    if (c->out_len) {
        unsigned long long *cnt = sm.d_cnt.get(); // (slot 0 is free again)
        HB_HIP(hipMemsetAsync(cnt, 0, 4 * sizeof(unsigned long long), c->stream));
        const unsigned blocks = grid_blocks(c, (n_pad + 255) / 256, 8);
        hipLaunchKernelGGL(hbk::sample_result_kernel, dim3(std::max(blocks, 1u)), dim3(256), 0, c->stream, (const uint16_t *)sm.d_hist.get(), D, n_pad,
                           (const double *)sm.d_w.get(), (const uint32_t *)c->d_cid_of, c->d_out, cnt);
        HB_HIP(hipGetLastError());
        HB_HIP(hipMemcpyAsync(c->h_out, c->d_out, c->out_len * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HB_HIP(hipMemcpyAsync(h, cnt, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HB_HIP(hipStreamSynchronize(c->stream));
        c->res_count = h[0];
    } else {
        c->res_count = 0;
    }
    sm.levels = D;
    c->image = Image::Sampled;
    st.results = c->res_count;
    st.ms_total = now_ms() - t0;
    copy_out(st_out, st);
    return HB_OK;
}

} // namespace

extern "C" {

int hb_sampled_harmonic(hb_ctx *c, const hb_sample_options *opt, hb_sample_stats *stats)
{
    return operator_entry(c, "hb_sampled_harmonic", [&]() { return sampled_harmonic(c, opt, stats); }, "");
}

int hb_sample_sources(hb_ctx *c, uint64_t seed, uint64_t k, hb_u128 *out, uint64_t *written)
{
    return guarded(c, [&]() -> int {
        if (!c || !written) return c ? fail(c, HB_ERR_INVALID, "hb_sample_sources: written == NULL") : HB_ERR_INVALID;
        if (!c->loaded) return fail(c, HB_ERR_INVALID, "hb_sample_sources: no graph loaded");
        int rc = set_device(c);
        if (rc) return rc;
        std::vector<uint32_t> sids;
        if ((rc = sample_sids(c, seed, k, &sids))) return rc;
        *written = sids.size();
        if (out)
            for (size_t i = 0; i < sids.size(); i++) out[i] = c->g.ids[sids[i]];
        return HB_OK;
    });
}

int hb_debug_sample_histogram(hb_ctx *c, uint16_t *out)
{
    return guarded(c, [&]() -> int {
        if (!c || !out) return HB_ERR_INVALID;
        if (!c->smp.levels) return fail(c, HB_ERR_INVALID, "hb_debug_sample_histogram: no sampled result (call hb_sampled_harmonic)");
        int rc = set_device(c);
        if (rc) return rc;
        const Plan &p = c->plan;
        const uint32_t D = c->smp.levels;
        std::vector<uint16_t> hist((size_t)D * p.n_pad);
        std::vector<uint32_t> sid_of(p.n_pad);
        if (p.n_pad) {
            HB_HIP(hipMemcpyAsync(hist.data(), c->smp.d_hist.get(), hist.size() * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
            HB_HIP(hipMemcpyAsync(sid_of.data(), c->d_sid_of, p.n_pad * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
            HB_HIP(hipStreamSynchronize(c->stream));
        }
        for (uint64_t r = 0; r < p.n_pad; r++) {
            const uint32_t sid = sid_of[r];
            if (sid == kNone) continue;
            for (uint32_t d = 0; d < D; d++) out[(uint64_t)sid * D + d] = hist[(uint64_t)d * p.n_pad + r];
        }
        return HB_OK;
    });
}

} // extern "C"
