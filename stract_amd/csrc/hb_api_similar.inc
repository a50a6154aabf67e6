// hb_api_similar.inc - part of the hb_api.hip translation unit (included after hb_api_links.inc; uses its list builder).
// hb_similar_hosts: scored_nodes of SimilarHostsFinder::find_similar_hosts (crates/core/src/similar_hosts.rs:54-272) for a list of liked
// hosts - co-citation candidates from limited backlinks and forward links, scored by the inbound similarity of 512-backlink BitVecs.
// Kernels: hb_similar.hip.h.  Definitions: include/hyperball.h.  The operator borrows nothing (no claim_rows, no take_image) and leaves
// the links result alone: every list goes to a holder of GraphDeviceState::shs.

namespace {

constexpr uint64_t kSimilarMaxLiked = 256;

int similar_hosts(hb_ctx *c, const hb_similar_options *opt_in, hb_similar_stats *st_out)
{
    const double t0 = now_ms();
    const std::string who = "hb_similar_hosts";
    hb_similar_options o{};
    copy_in(opt_in, &o);
    // ---- refusals: all of them before anything of the previous result is touched
    if (!opt_in) return fail(c, HB_ERR_INVALID, who + ": opt == NULL (limit has no default)");
    if (o.limit < 1 || o.limit > hbk::kShMaxCand) return fail(c, HB_ERR_INVALID, who + ": limit must be 1 .. 1024");
    if (!o.node_count) return fail(c, HB_ERR_INVALID, who + ": node_count == 0");
    if (!o.nodes) return fail(c, HB_ERR_INVALID, who + ": node_count without nodes");
    if (o.node_count >= (1ull << 32)) return fail(c, HB_ERR_INVALID, who + ": too many liked hosts");
    const Plan &p = c->plan;
    const uint64_t n = p.n, N = o.node_count, W = hbk::kShList;
    size_t nlev;
    int rc;
    if ((rc = links_levels(c, who, &nlev))) return rc;
    const ResolvedIds ids = resolve_ids(c, o.nodes, N);
    const std::vector<uint32_t> &liked = ids.distinct, &anchor = ids.slot; // the distinct liked sids; the entries in caller order as slots
    const uint64_t D = liked.size();
    if (D > kSimilarMaxLiked) return fail(c, HB_ERR_INVALID, who + ": more than 256 distinct liked hosts");
    auto &s = c->shs;
    hb_similar_stats st{};
    st.liked_distinct = D;
    st.unknown = ids.unknown;
    if (D && (rc = links_top_rows(c, who, &st.ms_gpu_lists))) return rc; // (it may refuse: before the previous result is touched)
    s.valid = false;
    std::vector<uint32_t> cand_sid, cand_count, top_sid;
    std::vector<double> top_score;
    auto finish = [&]() {
        st.candidates = cand_sid.size();
        st.written = top_sid.size();
        s.cand_sid.swap(cand_sid);
        s.cand_count.swap(cand_count);
        s.top_sid.swap(top_sid);
        s.top_score.swap(top_score);
        s.valid = true;
        st.device_bytes = s.bytes;
        st.ms_total = now_ms() - t0;
        copy_out(st_out, st);
        return HB_OK;
    };
    if (!D) return finish();
    ListBuild lists(nlev, (uint32_t)W, o.flags);
    uint32_t *h32 = (uint32_t *)c->h_counters; // (pinned words of the context; hb_run rewrites them before it reads them)

    // ---- steps 1 and 2: In512 of the liked hosts, the distinct sources of their 128-prefixes
    double t = now_ms();
    if ((rc = hold(c, s.bytes, s.d_in, D * W))) return rc;
    if ((rc = hold(c, s.bytes, s.d_in_len, D))) return rc;
    if ((rc = hold(c, s.bytes, s.d_in_mask, D))) return rc;
    if ((rc = hold(c, s.bytes, s.d_keys, D * W))) return rc;
    if ((rc = hold(c, s.bytes, s.d_src, D * hbk::kShPrefix))) return rc;
    if ((rc = hold(c, s.bytes, s.d_count, n))) return rc;
    if ((rc = hold(c, s.bytes, s.d_cnt, 8))) return rc;
    if ((rc = hold(c, s.bytes, s.d_liked, D))) return rc;
    if ((rc = hold(c, s.bytes, s.d_anchor, N))) return rc;
    if ((rc = lists.run(c, who, false, liked.data(), nullptr, D, s.d_in.get(), s.d_keys.get(), s.d_in_len.get()))) return rc;
    uint32_t *cnt32 = (uint32_t *)s.d_cnt.get(); // [0] |B|, [1] distinct targets, [2] eligible targets, [3] candidates; words 2, 3 as u64: the pair counters
    HB_HIP(hipMemsetAsync(s.d_cnt.get(), 0, 8 * sizeof(unsigned long long), c->stream));
    HB_HIP(hipMemsetAsync(s.d_count.get(), 0, n * sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(hbk::sh_sources_kernel, dim3(grid_blocks(c, (D * hbk::kShPrefix + 255) / 256, 8, 1)), dim3(256), 0, c->stream, (const uint32_t *)s.d_in.get(),
                       (const uint32_t *)s.d_in_len.get(), D, n, s.d_count.get(), s.d_src.get(), cnt32);
    HB_HIP(hipGetLastError());
    HB_HIP(hipMemcpyAsync(h32, cnt32, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HB_HIP(hipStreamSynchronize(c->stream));
    const uint64_t nb = h32[0];
    st.nb = nb;
    st.apply = nb > 32 ? 1u : 0u;
    st.count_bound = (nb + 3) / 4;
    st.ms_in = now_ms() - t;
    if (!nb) { // no liked host has an in-link: B and the result are empty
        st.ms_gpu_lists += lists.gpu_ms();
        return finish();
    }

    // ---- step 3: the forward lists of B
    t = now_ms();
    if ((rc = hold(c, s.bytes, s.d_fw, nb * W))) return rc;
    if ((rc = hold(c, s.bytes, s.d_fw_len, nb))) return rc;
    if ((rc = hold(c, s.bytes, s.d_keys, nb * W))) return rc;
    if ((rc = lists.run(c, who, true, nullptr, s.d_src.get(), nb, s.d_fw.get(), s.d_keys.get(), s.d_fw_len.get()))) return rc;
    for (uint32_t d : lists.degree) st.forward_entries += std::min<uint64_t>(d, W);
    st.ms_forward = now_ms() - t;

    // ---- step 4: count, filter, order, take, drop the liked hosts
    t = now_ms();
    const uint64_t touched_cap = std::max<uint64_t>(std::min<uint64_t>(n, st.forward_entries), 1);
    if ((rc = hold(c, s.bytes, s.d_touched, touched_cap))) return rc;
    if ((rc = hold(c, s.bytes, s.d_cand, hbk::kShMaxCand))) return rc;
    if ((rc = hold(c, s.bytes, s.d_cand_count, hbk::kShMaxCand))) return rc;
    HB_HIP(hipMemsetAsync(s.d_count.get(), 0, n * sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(hbk::sh_count_kernel, dim3(grid_blocks(c, (nb * W + 255) / 256, 8, 1)), dim3(256), 0, c->stream, (const uint32_t *)s.d_fw.get(),
                       (const uint32_t *)s.d_fw_len.get(), nb, n, s.d_count.get(), s.d_touched.get(), touched_cap, cnt32 + 1);
    HB_HIP(hipGetLastError());
    HB_HIP(hipMemcpyAsync(h32, cnt32 + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HB_HIP(hipStreamSynchronize(c->stream));
    const uint64_t m = h32[0];
    if (m > touched_cap) return fail(c, HB_ERR_INVALID, who + ": the distinct targets outnumber the forward entries (internal error)");
    st.distinct_targets = m;
    uint64_t C = 0;
    if (m) {
        DevPtr<uint64_t> d_key, d_order, d_rank; // (work memory of the order: gone at the end of the step)
        if (d_key.alloc(m) != hipSuccess || d_order.alloc(m) != hipSuccess || d_rank.alloc(m) != hipSuccess)
            return fail(c, HB_ERR_NOMEM, who + ": out of device memory for the candidates' order");
        hipLaunchKernelGGL(hbk::sh_key_kernel, dim3(grid_blocks(c, (m + 255) / 256, 8, 1)), dim3(256), 0, c->stream, (const uint32_t *)s.d_touched.get(), m,
                           (const uint32_t *)s.d_count.get(), st.apply, (uint32_t)st.count_bound, d_key.get(), cnt32 + 2);
        HB_HIP(hipGetLastError());
        const std::string e = gpu_rank_keys_device((void *)c->stream, (const uint64_t *)d_key.get(), m, d_order.get(), d_rank.get());
        if (!e.empty()) return fail(c, e.find("memory") != std::string::npos ? HB_ERR_NOMEM : HB_ERR_HIP, who + ": " + e);
        HB_HIP(hipMemcpyAsync(h32, cnt32 + 2, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HB_HIP(hipStreamSynchronize(c->stream));
        const uint64_t take = std::min<uint64_t>(h32[0], st.apply ? 256 : 1024);
        st.taken = take;
        HB_HIP(hipMemcpyAsync(s.d_liked.get(), liked.data(), D * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(hbk::sh_take_kernel, dim3(1), dim3(256), 0, c->stream, (const uint64_t *)d_key.get(), (const uint64_t *)d_order.get(), (uint32_t)take,
                           (const uint32_t *)s.d_liked.get(), (uint32_t)D, s.d_cand.get(), s.d_cand_count.get(), cnt32 + 3);
        HB_HIP(hipGetLastError());
        HB_HIP(hipMemcpyAsync(h32, cnt32 + 3, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HB_HIP(hipStreamSynchronize(c->stream)); // (also: the work memory may go)
        C = h32[0];
    }
    st.ms_count = now_ms() - t;
    if (!C) {
        st.ms_gpu_lists += lists.gpu_ms();
        return finish();
    }
    cand_sid.resize(C);
    cand_count.resize(C);
    HB_HIP(hipMemcpyAsync(cand_sid.data(), s.d_cand.get(), C * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HB_HIP(hipMemcpyAsync(cand_count.data(), s.d_cand_count.get(), C * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HB_HIP(hipStreamSynchronize(c->stream)); // (the vectors are this function's: no copy may be pending when a later step returns early)

    // ---- step 5: the BitVecs - In512 of the candidates; every list sorted by sid, its bloom mask
    t = now_ms();
    if ((rc = hold(c, s.bytes, s.d_cin, hbk::kShMaxCand * W))) return rc;
    if ((rc = hold(c, s.bytes, s.d_cin_len, hbk::kShMaxCand))) return rc;
    if ((rc = hold(c, s.bytes, s.d_cin_mask, hbk::kShMaxCand))) return rc;
    if ((rc = hold(c, s.bytes, s.d_keys, hbk::kShMaxCand * W))) return rc;
    if ((rc = lists.run(c, who, false, nullptr, s.d_cand.get(), C, s.d_cin.get(), s.d_keys.get(), s.d_cin_len.get()))) return rc;
    st.ms_gpu_lists += lists.gpu_ms();
    hipLaunchKernelGGL(hbk::sh_bitvec_kernel, dim3((unsigned)D), dim3(256), 0, c->stream, s.d_in.get(), (const uint32_t *)s.d_in_len.get(), (const uint32_t *)c->d_dev_of,
                       (const uint64_t *)c->d_idlow, n, s.d_in_mask.get());
    hipLaunchKernelGGL(hbk::sh_bitvec_kernel, dim3((unsigned)C), dim3(256), 0, c->stream, s.d_cin.get(), (const uint32_t *)s.d_cin_len.get(), (const uint32_t *)c->d_dev_of,
                       (const uint64_t *)c->d_idlow, n, s.d_cin_mask.get());
    HB_HIP(hipGetLastError());
    HB_HIP(hipStreamSynchronize(c->stream));
    st.ms_bitvec = now_ms() - t;

    // ---- steps 6 and 7: the scores, the top k
    t = now_ms();
    const uint64_t k = std::min<uint64_t>(o.limit, C);
    if ((rc = hold(c, s.bytes, s.d_score, hbk::kShMaxCand))) return rc;
    if ((rc = hold(c, s.bytes, s.d_top_score, hbk::kShMaxCand))) return rc;
    if ((rc = hold(c, s.bytes, s.d_top_sid, hbk::kShMaxCand))) return rc;
    HB_HIP(hipMemcpyAsync(s.d_anchor.get(), anchor.data(), N * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    if ((rc = lap_start(c))) return rc;
    hipLaunchKernelGGL(hbk::sh_score_kernel, dim3((unsigned)C), dim3(256), 0, c->stream, (const uint32_t *)s.d_cin.get(), (const uint32_t *)s.d_cin_len.get(),
                       (const unsigned long long *)s.d_cin_mask.get(), (const uint32_t *)s.d_in.get(), (const uint32_t *)s.d_in_len.get(),
                       (const unsigned long long *)s.d_in_mask.get(), (const uint32_t *)s.d_anchor.get(), N, s.d_score.get(), s.d_cnt.get() + 2);
    hipLaunchKernelGGL(hbk::sh_top_kernel, dim3(1), dim3(256), 0, c->stream, (const uint32_t *)s.d_cand.get(), (const double *)s.d_score.get(), (uint32_t)C, (uint32_t)k,
                       s.d_top_sid.get(), s.d_top_score.get());
    HB_HIP(hipGetLastError());
    top_sid.resize(k);
    top_score.resize(k);
    unsigned long long *h64 = c->h_counters;
    HB_HIP(hipMemcpyAsync(top_sid.data(), s.d_top_sid.get(), k * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HB_HIP(hipMemcpyAsync(top_score.data(), s.d_top_score.get(), k * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HB_HIP(hipMemcpyAsync(h64, s.d_cnt.get() + 2, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    if ((rc = lap(c, &st.ms_gpu_score))) return rc;
    st.pairs_gated = h64[0];
    st.pairs_intersected = h64[1];
    st.ms_score = now_ms() - t;
    return finish();
}

const char *const kNoSimilarHosts = "no similar-hosts result (call hb_similar_hosts)";

} // namespace

extern "C" {

int hb_similar_hosts(hb_ctx *c, const hb_similar_options *opt, hb_similar_stats *stats)
{
    return operator_entry(c, "hb_similar_hosts", [&]() { return similar_hosts(c, opt, stats); });
}

int hb_similar_count(hb_ctx *c, uint64_t *count)
{
    return guarded(c, [&]() -> int {
        if (!c) return HB_ERR_INVALID;
        return result_count(c, c->shs.valid, "hb_similar_count", kNoSimilarHosts, count, c->shs.top_sid.size());
    });
}

int hb_similar_copy(hb_ctx *c, hb_u128 *ids, double *scores, uint64_t cap)
{
    return reader_entry(c, c && c->shs.valid, "hb_similar_copy", kNoSimilarHosts, [&]() -> int {
        const auto &s = c->shs;
        if (cap < s.top_sid.size()) return fail(c, HB_ERR_INVALID, "hb_similar_copy: cap < the entries of hb_similar_count");
        for (size_t i = 0; i < s.top_sid.size(); i++) {
            if (s.top_sid[i] >= c->g.ids.size()) return fail(c, HB_ERR_INVALID, "hb_similar_copy: a list entry is no node (internal error)");
            if (ids) ids[i] = c->g.ids[s.top_sid[i]];
            if (scores) scores[i] = s.top_score[i];
        }
        return HB_OK;
    });
}

int hb_similar_candidates(hb_ctx *c, hb_u128 *ids, uint64_t *counts, uint64_t cap, uint64_t *written)
{
    return reader_entry(c, c && c->shs.valid, "hb_similar_candidates", kNoSimilarHosts, [&]() -> int {
        const auto &s = c->shs;
        if (written) *written = s.cand_sid.size();
        if ((ids || counts) && cap < s.cand_sid.size()) return fail(c, HB_ERR_INVALID, "hb_similar_candidates: cap < the candidates");
        for (size_t i = 0; i < s.cand_sid.size(); i++) {
            if (s.cand_sid[i] >= c->g.ids.size()) return fail(c, HB_ERR_INVALID, "hb_similar_candidates: an entry is no node (internal error)");
            if (ids) ids[i] = c->g.ids[s.cand_sid[i]];
            if (counts) counts[i] = s.cand_count[i];
        }
        return HB_OK;
    });
}

} // extern "C"
