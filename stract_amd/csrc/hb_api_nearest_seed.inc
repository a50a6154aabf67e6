// hb_api_nearest_seed.inc - part of the hb_api.hip translation unit (included at its end; uses its hb_ctx and helpers).
// hb_nearest_seed: HarmonicNearestSeed (crates/core/src/entrypoint/centrality.rs:126-201) for every node of the loaded graph - the seed
// of every node by one pull over the plan with a lexicographic min as the join, then one streaming kernel per round (kernels:
// hb_nearest_seed.hip.h).  Definitions: include/hyperball.h.  Like hb_distances the operator borrows nothing: no claim_rows, no
// take_image; every buffer is its own, allocated at the first call after a load and freed by the next load.

namespace {

int nearest_seed_alloc(hb_ctx *c)
{
    auto &s = c->nst;
    if (s.ready) return HB_OK;
    const Plan &p = c->plan;
    const uint64_t before = c->stats.device_bytes;
    int rc;
    if ((rc = dev_alloc(c, &s.d_cand, p.n_pad))) return rc;
    if ((rc = dev_alloc(c, &s.d_part, p.nv * 2))) return rc;
    if ((rc = dev_alloc(c, &s.d_seed_row, p.n_pad))) return rc;
    for (int k = 0; k < 2; k++) {
        if ((rc = dev_alloc(c, &s.d_val[k], p.n_pad))) return rc;
        if ((rc = dev_alloc(c, &s.d_has[k], p.n_pad))) return rc;
    }
    if ((rc = dev_alloc(c, &s.d_up_key, p.n))) return rc;
    if ((rc = dev_alloc(c, &s.d_up_val, p.n))) return rc;
    if ((rc = dev_alloc(c, &s.d_up_has, p.n))) return rc;
    if ((rc = dev_alloc(c, &s.d_cnt, hbk::kCounterWords + 8))) return rc;
    if ((rc = dev_alloc(c, &s.d_seed_sid, p.n))) return rc;
    if ((rc = node_result_alloc(c, s.res))) return rc;
    if ((rc = dev_alloc(c, &s.d_top_key, p.n))) return rc;
    if ((rc = dev_alloc(c, &s.d_top_keep, p.n))) return rc;
    s.bytes = c->stats.device_bytes - before;
    s.ready = true;
    return HB_OK;
}

int nearest_seed(hb_ctx *c, const hb_nearest_seed_options *opt_in, hb_nearest_seed_stats *st_out)
{
    const double t0 = now_ms();
    hb_nearest_seed_options o{};
    copy_in(opt_in, &o);
    int rc;
    // ---- refusals: all of them before anything of the previous result is touched
    if (!opt_in) return fail(c, HB_ERR_INVALID, "hb_nearest_seed: opt == NULL (discount_factor has no default)");
    if (!std::isfinite(o.discount_factor) || std::signbit(o.discount_factor))
        return fail(c, HB_ERR_INVALID, "hb_nearest_seed: discount_factor must be finite and >= 0");
    if (o.rounds > 255) return fail(c, HB_ERR_INVALID, "hb_nearest_seed: rounds > 255");
    const bool from_image = (o.flags & HB_SEED_FROM_IMAGE) != 0;
    if (from_image && (o.orig_ids || o.orig_vals || o.orig_count))
        return fail(c, HB_ERR_INVALID, "hb_nearest_seed: HB_SEED_FROM_IMAGE together with an orig list");
    if (o.orig_count && (!o.orig_ids || !o.orig_vals)) return fail(c, HB_ERR_INVALID, "hb_nearest_seed: orig_count without orig_ids / orig_vals");
    if (o.key_count && (!o.key_ids || !o.keys)) return fail(c, HB_ERR_INVALID, "hb_nearest_seed: key_count without key_ids / keys");
    if (from_image && c->image == Image::None)
        return fail(c, HB_ERR_INVALID, "hb_nearest_seed: HB_SEED_FROM_IMAGE without a live result (call hb_run or hb_sampled_harmonic)");
    for (uint64_t i = 0; i < o.orig_count; i++)
        if (std::isnan(o.orig_vals[i]) || std::signbit(o.orig_vals[i]))
            return fail(c, HB_ERR_INVALID, "hb_nearest_seed: orig_vals[" + std::to_string(i) + "] is NaN or has its sign bit set");
    const Plan &p = c->plan;
    auto &s = c->nst;
    hb_nearest_seed_stats st{};
    const uint32_t rounds = o.rounds ? o.rounds : 1;
    auto finish = [&]() {
        st.device_bytes = s.bytes;
        st.ms_total = now_ms() - t0;
        copy_out(st_out, st);
        return HB_OK;
    };
    // ---- the lists by sid (the ids are resolved on the host cores: hb_host.cpp host_find_sids)
    const uint64_t n = p.n;
    std::vector<uint32_t> sids(std::max(o.orig_count, o.key_count));
    std::vector<unsigned long long> up_key(n, ~0ull);
    std::vector<double> up_val;
    std::vector<uint8_t> up_has;
    host_find_sids(c->g.ids.data(), n, o.key_ids, o.key_count, sids.data());
    for (uint64_t i = 0; i < o.key_count; i++) {
        if (sids[i] == kNone) st.unknown_keys++;
        else up_key[sids[i]] = o.keys[i]; // (a duplicate: the last one wins, like the orig list)
    }
    if (!from_image) {
        up_val.assign(n, 0.0);
        up_has.assign(n, 0);
        host_find_sids(c->g.ids.data(), n, o.orig_ids, o.orig_count, sids.data());
        for (uint64_t i = 0; i < o.orig_count; i++) {
            if (sids[i] == kNone) {
                st.unknown_orig++;
                continue;
            }
            up_val[sids[i]] = o.orig_vals[i]; // Db::insert: the last one wins
            up_has[sids[i]] = 1;
        }
    }
    s.res.reset();
    if (n == 0) { // an empty graph: an empty result
        s.res.valid = true;
        return finish();
    }
    if ((rc = nearest_seed_alloc(c))) return rc;
    const uint64_t n_pad = p.n_pad, rows_total = p.n_pad + p.nv;
    const unsigned row_blocks = grid_blocks(c, (n_pad + 255) / 256, 8, 1), sid_blocks = grid_blocks(c, (n + 255) / 256, 8, 1);
    unsigned long long *h = c->h_counters; // (pinned words of the context; hb_run rewrites them before it reads them)
    unsigned long long *cnt4 = s.d_cnt + hbk::kCounterWords; // four plain counters behind the striped ones

    // ---- seed level: candidates, the chunk rows' pairs (virtual levels ascending), the node rows' seeds
    HB_HIP(hipMemcpyAsync(s.d_up_key, up_key.data(), n * sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream));
    if ((rc = lap_start(c))) return rc;
    hipLaunchKernelGGL(hbk::ns_key_kernel, dim3(row_blocks), dim3(256), 0, c->stream, (const unsigned long long *)s.d_up_key, (const uint32_t *)c->d_sid_of, n_pad, s.d_cand);
    for_each_virtual_level(p, true, [&](uint64_t lo, uint64_t hi) { // ascending: a chunk row joins the pairs of the chunk rows below it
        hipLaunchKernelGGL(hbk::ns_seed_kernel<false>, dim3(grid_blocks(c, (hi - lo + 63) / 64, 8, 1)), dim3(256), 0, c->stream, (const uint64_t *)c->d_row_ptr,
                           (const uint32_t *)c->d_src, (const uint4 *)s.d_cand, s.d_part, (const uint32_t *)c->d_sid_of, (const uint32_t *)c->d_dev_of, s.d_seed_row, n_pad,
                           rows_total, lo, hi);
    });
    hipLaunchKernelGGL(hbk::ns_seed_kernel<true>, dim3(grid_blocks(c, (n_pad + 63) / 64, 8, 1)), dim3(256), 0, c->stream, (const uint64_t *)c->d_row_ptr,
                       (const uint32_t *)c->d_src, (const uint4 *)s.d_cand, s.d_part, (const uint32_t *)c->d_sid_of, (const uint32_t *)c->d_dev_of, s.d_seed_row, n_pad,
                       rows_total, (uint64_t)0, n_pad);
    HB_HIP(hipGetLastError());
    if ((rc = lap(c, &st.ms_seed))) return rc;

    // ---- round 0: the original values
    if (!from_image) {
        HB_HIP(hipMemcpyAsync(s.d_up_val, up_val.data(), n * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HB_HIP(hipMemcpyAsync(s.d_up_has, up_has.data(), n, hipMemcpyHostToDevice, c->stream));
    }
    HB_HIP(hipMemsetAsync(cnt4, 0, 4 * sizeof(unsigned long long), c->stream));
    if ((rc = lap_start(c))) return rc;
    if (from_image)
        hipLaunchKernelGGL(hbk::ns_init_image_kernel, dim3(row_blocks), dim3(256), 0, c->stream, (const double *)c->d_out, (const uint32_t *)c->d_cid_of, c->out_len, n_pad,
                           s.d_val[0], s.d_has[0], cnt4);
    else
        hipLaunchKernelGGL(hbk::ns_init_list_kernel, dim3(row_blocks), dim3(256), 0, c->stream, (const double *)s.d_up_val, (const uint8_t *)s.d_up_has,
                           (const uint32_t *)c->d_sid_of, n_pad, s.d_val[0], s.d_has[0], cnt4);
    HB_HIP(hipGetLastError());
    HB_HIP(hipMemcpyAsync(h, cnt4, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    if ((rc = lap(c, &st.ms_fill))) return rc;
    st.with_original = h[0];

    // ---- the rounds: synchronous, state after r - 1 read, state after r written; the first round that fills nothing is the last
    int cur = 0;
    for (uint32_t r = 1; r <= rounds; r++) {
        HB_HIP(hipMemsetAsync(s.d_cnt, 0, hbk::kCounterWords * sizeof(unsigned long long), c->stream));
        if ((rc = lap_start(c))) return rc;
        hipLaunchKernelGGL(hbk::ns_fill_kernel, dim3(row_blocks), dim3(256), 0, c->stream, (const double *)s.d_val[cur], (const uint8_t *)s.d_has[cur],
                           (const uint32_t *)s.d_seed_row, n_pad, o.discount_factor, s.d_val[cur ^ 1], s.d_has[cur ^ 1], s.d_cnt);
        HB_HIP(hipGetLastError());
        HB_HIP(hipMemcpyAsync(h, s.d_cnt, hbk::kCounterWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        if ((rc = lap(c, &st.ms_fill))) return rc;
        uint64_t filled = 0;
        for (int k = 0; k < hbk::kStripes; k++) filled += h[4 * k];
        st.filled[std::min<uint32_t>(r - 1, 15)] += filled;
        st.rounds_run = r;
        cur ^= 1;
        if (!filled) break;
    }

    // ---- the result by sid, its compacted form (only the results are downloaded by hb_nearest_seed_copy), the final counters
    HB_HIP(hipMemsetAsync(cnt4, 0, 4 * sizeof(unsigned long long), c->stream));
    if ((rc = lap_start(c))) return rc;
    hipLaunchKernelGGL(hbk::ns_by_sid_kernel, dim3(sid_blocks), dim3(256), 0, c->stream, (const double *)s.d_val[cur], (const uint8_t *)s.d_has[cur],
                       (const uint32_t *)s.d_seed_row, (const uint32_t *)c->d_dev_of, (const uint32_t *)c->d_sid_of, n, n_pad, s.res.d_val_sid, s.res.d_flag_sid, s.d_seed_sid, cnt4);
    HB_HIP(hipGetLastError());
    HB_HIP(hipMemcpyAsync(h, cnt4, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    if ((rc = lap(c, &st.ms_fill))) return rc;
    st.results = h[0];
    st.no_seed = h[1];
    st.seed_without_value = h[2];
    if ((rc = node_result_compact(c, s.res, "hb_nearest_seed", &st.results))) return rc;
    s.res.valid = true;
    return finish();
}

const char *const kNoNearestSeed = "no nearest-seed result (call hb_nearest_seed)";

NodeResult<double> *nearest_seed_result(hb_ctx *c) { return c ? &c->nst.res : nullptr; }

} // namespace

extern "C" {

int hb_nearest_seed(hb_ctx *c, const hb_nearest_seed_options *opt, hb_nearest_seed_stats *stats)
{
    return operator_entry(c, "hb_nearest_seed", [&]() { return nearest_seed(c, opt, stats); });
}

int hb_nearest_seed_count(hb_ctx *c, uint64_t *count) { return node_result_count(c, nearest_seed_result(c), "hb_nearest_seed_count", kNoNearestSeed, count); }

int hb_nearest_seed_copy(hb_ctx *c, hb_u128 *ids, double *vals, uint64_t cap)
{
    return node_result_copy(c, nearest_seed_result(c), "hb_nearest_seed_copy", kNoNearestSeed, ids, vals, cap);
}

int hb_nearest_seed_all(hb_ctx *c, double *vals, uint64_t cap)
{
    return node_result_all(c, nearest_seed_result(c), "hb_nearest_seed_all", "vals", kNoNearestSeed, vals, cap);
}

int hb_nearest_seed_top(hb_ctx *c, uint64_t k, hb_u128 *ids, double *vals, uint64_t *written)
{
    return reader_entry(c, c && c->nst.res.valid, "hb_nearest_seed_top", kNoNearestSeed, [&]() -> int {
        const uint64_t n = c->plan.n;
        auto &s = c->nst;
        const uint64_t top = std::min<uint64_t>(k, s.res.count);
        if (!top) return HB_OK;
        hipLaunchKernelGGL(hbk::ns_top_keys_kernel, dim3(grid_blocks(c, (n + 255) / 256, 8, 1)), dim3(256), 0, c->stream, (const double *)s.res.d_val_sid,
                           (const uint8_t *)s.res.d_flag_sid, n, s.d_top_key, s.d_top_keep);
        HB_HIP(hipGetLastError());
        // (entry i of the keys is sid n - 1 - i: ns_top_keys_kernel)
        return result_top(c, "hb_nearest_seed_top", s.d_top_key, s.d_top_keep, n, top, [n](uint32_t at) { return n - 1 - at; }, ids, vals, written);
    }, written);
}

int hb_nearest_seed_seeds(hb_ctx *c, hb_u128 *seed, uint8_t *has_seed, uint64_t cap)
{
    return reader_entry(c, c && c->nst.res.valid, "hb_nearest_seed_seeds", kNoNearestSeed, [&]() -> int {
        const uint64_t n = c->plan.n;
        if (cap < n) return fail(c, HB_ERR_INVALID, "hb_nearest_seed_seeds: cap < n");
        if (!n || (!seed && !has_seed)) return HB_OK;
        std::vector<uint32_t> sid(n);
        HB_HIP(hipMemcpyAsync(sid.data(), c->nst.d_seed_sid, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HB_HIP(hipStreamSynchronize(c->stream));
        for (uint64_t v = 0; v < n; v++) {
            const bool has = sid[v] != kNone;
            if (seed) seed[v] = has ? c->g.ids[sid[v]] : hb_u128{0, 0};
            if (has_seed) has_seed[v] = has ? 1 : 0;
        }
        return HB_OK;
    });
}

} // extern "C"
