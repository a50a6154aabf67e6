// hb_api_score.inc - part of the hb_api.hip translation unit (included after hb_api_similar.inc; uses the list builder of
// hb_api_links.inc).  hb_score_hosts: inbound_similarity::Scorer::score (crates/core/src/ranking/inbound_similarity.rs:44-50,99-118) of the
// result hosts of one or several searches against each search's liked / disliked hosts, as searcher/api/mod.rs:467-501 and the
// InboundScorer stage (ranking/pipeline/scorers/inbound_similarity.rs:38-54) use it - work proportional to (result hosts + anchors) x
// limit, where hb_inbound_similarity + hb_similarity_lookup walk the graph.  Kernels: hb_score.hip.h.  Definitions: include/hyperball.h.
// The operator borrows nothing (no claim_rows, no take_image) and leaves every other result alone: every buffer is a holder of
// GraphDeviceState::sco.

namespace {

constexpr uint64_t kScoreMaxRequests = 4096, kScoreMaxEntries = 1ull << 24, kScoreMaxDistinct = 262144;
constexpr uint64_t kScorePiece = 1ull << 20, kScoreSmallPiece = 64; // pairs of a piece (HB_SCORE_SMALL_PIECES: the small one)

// The pieces of the pair space: rectangles (request, node range, anchor range) in request order, at most `cap` pairs per piece.  A
// request that fits goes into one rectangle; one that does not is cut into node ranges of whole anchor lists, and where one anchor list
// alone is too long, into anchor ranges of one node.  The ranges of a node come in ascending anchor order in DIFFERENT pieces: the
// finish kernel of a piece reads the sums its predecessor left.
struct ScorePieces {
    std::vector<hbk::ScRect> rect;
    std::vector<uint64_t> piece_begin; // pieces + 1 offsets into rect
};

ScorePieces score_pieces(const std::vector<hbk::ScRequest> &req, const std::vector<uint64_t> &node_count, uint64_t cap)
{
    ScorePieces out;
    uint64_t used = 0; // pairs of the open piece
    out.piece_begin.push_back(0);
    auto close = [&]() {
        if (out.piece_begin.back() != out.rect.size()) out.piece_begin.push_back(out.rect.size());
        used = 0;
    };
    auto add = [&](uint32_t r, uint64_t node0, uint64_t nodes, uint64_t anchor0, uint64_t anchors) {
        if (used + nodes * anchors > cap) close();
        hbk::ScRect x{};
        x.req = r;
        x.node0 = (uint32_t)node0;
        x.nodes = (uint32_t)nodes;
        x.anchor0 = (uint32_t)anchor0;
        x.anchors = (uint32_t)anchors;
        x.tiles = (uint32_t)((anchors + hbk::kScTile - 1) / hbk::kScTile);
        out.rect.push_back(x);
        used += nodes * anchors;
        if (anchor0 + anchors != req[r].anchors) close(); // (the node's next range reads this one's sums)
    };
    for (uint32_t r = 0; r < req.size(); r++) {
        const uint64_t N = node_count[r], E = req[r].anchors;
        if (!N) continue;
        if (N * E <= cap) add(r, 0, N, 0, E);
        else if (E <= cap) {
            const uint64_t step = cap / E;
            for (uint64_t j = 0; j < N; j += step) add(r, j, std::min(step, N - j), 0, E);
        } else {
            for (uint64_t j = 0; j < N; j++)
                for (uint64_t a = 0; a < E; a += cap) add(r, j, 1, a, std::min(cap, E - a));
        }
    }
    close();
    // the bases of every piece's rectangles: pair words, workgroups of the pair kernel, lanes of the finish kernel
    for (size_t k = 0; k + 1 < out.piece_begin.size(); k++) {
        uint64_t pairs = 0, groups = 0, lanes = 0;
        for (uint64_t i = out.piece_begin[k]; i < out.piece_begin[k + 1]; i++) {
            hbk::ScRect &x = out.rect[i];
            x.pair_base = pairs;
            x.group_base = groups;
            x.lane_base = lanes;
            pairs += (uint64_t)x.nodes * x.anchors;
            groups += (uint64_t)x.nodes * x.tiles;
            lanes += x.nodes;
        }
    }
    return out;
}

int score_hosts(hb_ctx *c, const hb_score_options *opt_in, hb_score_stats *st_out)
{
    const double t0 = now_ms();
    const std::string who = "hb_score_hosts";
    hb_score_options o{};
    copy_in(opt_in, &o);
    // ---- refusals: all of them before anything of the previous result is touched
    if (!opt_in) return fail(c, HB_ERR_INVALID, who + ": opt == NULL (limit has no default)");
    if (o.limit < 1 || o.limit > hbk::kScMaxList) return fail(c, HB_ERR_INVALID, who + ": limit must be 1 .. 1024");
    if (o.slots_per_batch > kLinksMaxSlots) return fail(c, HB_ERR_INVALID, who + ": slots_per_batch > 65536");
    if (!o.request_count) return fail(c, HB_ERR_INVALID, who + ": request_count == 0");
    if (o.request_count > kScoreMaxRequests) return fail(c, HB_ERR_INVALID, who + ": more than 4096 requests");
    if (!o.requests) return fail(c, HB_ERR_INVALID, who + ": request_count without requests");
    const uint64_t R = o.request_count, limit = o.limit;
    uint64_t A = 0, N = 0;
    for (uint64_t r = 0; r < R; r++) {
        const hb_score_request &q = o.requests[r];
        if ((q.liked_count && !q.liked) || (q.disliked_count && !q.disliked) || (q.node_count && !q.nodes))
            return fail(c, HB_ERR_INVALID, who + ": a count without its list (request " + std::to_string(r) + ")");
        if (q.liked_count > kScoreMaxEntries || q.disliked_count > kScoreMaxEntries || q.node_count > kScoreMaxEntries || A + N > kScoreMaxEntries)
            return fail(c, HB_ERR_INVALID, who + ": more than 2^24 anchor and node entries");
        A += q.liked_count + q.disliked_count;
        N += q.node_count;
    }
    if (A + N > kScoreMaxEntries) return fail(c, HB_ERR_INVALID, who + ": more than 2^24 anchor and node entries");
    const Plan &p = c->plan;
    const uint64_t n = p.n;
    size_t nlev;
    int rc;
    if ((rc = links_levels(c, who, &nlev))) return rc;
    // ---- every id once: the anchors of all requests (liked, then disliked), then the nodes of all requests
    std::vector<hb_u128> ids;
    ids.reserve(A + N);
    for (uint64_t r = 0; r < R; r++) {
        const hb_score_request &q = o.requests[r];
        ids.insert(ids.end(), q.liked, q.liked + q.liked_count);
        ids.insert(ids.end(), q.disliked, q.disliked + q.disliked_count);
    }
    for (uint64_t r = 0; r < R; r++) ids.insert(ids.end(), o.requests[r].nodes, o.requests[r].nodes + o.requests[r].node_count);
    ResolvedIds known = resolve_ids(c, ids.data(), A + N);
    const std::vector<uint32_t> &distinct = known.distinct;
    std::vector<uint32_t> &idx = known.slot; // index of entry i: the slot of a known host, U + its position among the strangers otherwise (below)
    std::vector<hb_u128> strangers; // the distinct ids that are no node: self is decided on the index of an id, known or not
    for (uint64_t i = 0; i < A + N; i++)
        if (idx[i] == kNone) strangers.push_back(ids[i]);
    std::sort(strangers.begin(), strangers.end(), u128_less);
    strangers.erase(std::unique(strangers.begin(), strangers.end(), u128_eq), strangers.end());
    const uint64_t U = distinct.size();
    if (U > kScoreMaxDistinct) return fail(c, HB_ERR_INVALID, who + ": more than 262144 distinct known hosts");
    hb_score_stats st{};
    if (U && (rc = links_top_rows(c, who, &st.ms_lists))) return rc; // (it may refuse: before the previous result is touched)
    st.requests = R;
    st.anchors = A;
    st.nodes = N;
    st.distinct = U;
    for (uint64_t i = 0; i < A + N; i++) {
        if (idx[i] != kNone) continue;
        idx[i] = (uint32_t)(U + (std::lower_bound(strangers.begin(), strangers.end(), ids[i], u128_less) - strangers.begin()));
        (i < A ? st.unknown_anchors : st.unknown_nodes)++;
    }
    std::vector<hbk::ScRequest> req(R);
    std::vector<uint64_t> node_count(R), offsets(R + 1, 0);
    uint64_t a_at = 0, n_at = 0;
    for (uint64_t r = 0; r < R; r++) {
        const hb_score_request &q = o.requests[r];
        hbk::ScRequest &x = req[r];
        x.node_off = n_at;
        x.anchor_off = a_at;
        x.liked = (uint32_t)q.liked_count;
        x.anchors = (uint32_t)(q.liked_count + q.disliked_count);
        x.self_score = (q.flags & HB_SIM_SELF_SCORE) ? q.self_score : 1.0;
        x.n_disliked = (double)q.disliked_count;
        x.norm = (q.flags & HB_SIM_NORMALIZED) ? (double)std::max<uint64_t>(q.liked_count, 1) : 0.0;
        node_count[r] = q.node_count;
        offsets[r] = n_at;
        a_at += x.anchors;
        n_at += q.node_count;
        st.pairs += (uint64_t)x.anchors * q.node_count;
    }
    offsets[R] = N;
    const uint64_t piece_cap = (o.flags & HB_SCORE_SMALL_PIECES) ? kScoreSmallPiece : kScorePiece;
    const ScorePieces pieces = score_pieces(req, node_count, piece_cap);
    uint64_t rects_max = 1;
    for (size_t k = 0; k + 1 < pieces.piece_begin.size(); k++) rects_max = std::max(rects_max, pieces.piece_begin[k + 1] - pieces.piece_begin[k]);

    auto &s = c->sco;
    std::vector<double> scores(N);
    auto finish = [&]() { // (the previous result - two host vectors - stays readable until here: also a call that fails below leaves it)
        s.offsets.swap(offsets);
        s.scores.swap(scores);
        s.valid = true;
        st.device_bytes = s.bytes;
        st.ms_total = now_ms() - t0;
        copy_out(st_out, st);
        return HB_OK;
    };
    if (!N) return finish();

    // ---- the BitVecs of the distinct known hosts: their `limit` backlinks, sorted, the bloom masks
    const uint64_t lists_piece = std::min<uint64_t>(U, kLinksMaxSlots);
    if ((rc = hold(c, s.bytes, s.d_lists, U * limit))) return rc;
    if ((rc = hold(c, s.bytes, s.d_len, U))) return rc;
    if ((rc = hold(c, s.bytes, s.d_mask, U))) return rc;
    if ((rc = hold(c, s.bytes, s.d_keys, lists_piece * limit))) return rc;
    if ((rc = hold(c, s.bytes, s.d_node_idx, N))) return rc;
    if ((rc = hold(c, s.bytes, s.d_anchor_idx, A))) return rc;
    if ((rc = hold(c, s.bytes, s.d_req, R))) return rc;
    if ((rc = hold(c, s.bytes, s.d_rect, rects_max))) return rc;
    if ((rc = hold(c, s.bytes, s.d_pair, std::min(st.pairs, piece_cap)))) return rc;
    if ((rc = hold(c, s.bytes, s.d_acc, N * 2))) return rc;
    if ((rc = hold(c, s.bytes, s.d_score, N))) return rc;
    if ((rc = hold(c, s.bytes, s.d_cnt, 4))) return rc;
    if (U) {
        ListBuild lists(nlev, o.limit, o.flags, o.slots_per_batch);
        for (uint64_t base = 0; base < U; base += lists_piece) { // (one call unless the hosts outnumber the list builder's largest batch)
            const uint64_t P = std::min(lists_piece, U - base);
            if ((rc = lists.run(c, who, false, distinct.data() + base, nullptr, P, s.d_lists.get() + base * limit, s.d_keys.get(), s.d_len.get() + base))) return rc;
        }
        st.ms_lists += lists.gpu_ms();
        uint32_t sort_n = 2;
        while (sort_n < o.limit) sort_n <<= 1;
        if ((rc = lap_start(c))) return rc;
        hipLaunchKernelGGL(hbk::sc_bitvec_kernel, dim3((unsigned)U), dim3(256), 0, c->stream, s.d_lists.get(), (const uint32_t *)s.d_len.get(), o.limit, sort_n,
                           (const uint32_t *)c->d_dev_of, (const uint64_t *)c->d_idlow, n, s.d_mask.get());
        HB_HIP(hipGetLastError());
        if ((rc = lap(c, &st.ms_bitvec))) return rc;
    }

    // ---- the pairs, a piece at a time: classes and counts, then the sums of the piece's nodes
    if (A) HB_HIP(hipMemcpyAsync(s.d_anchor_idx.get(), idx.data(), A * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HB_HIP(hipMemcpyAsync(s.d_node_idx.get(), idx.data() + A, N * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HB_HIP(hipMemcpyAsync(s.d_req.get(), req.data(), R * sizeof(hbk::ScRequest), hipMemcpyHostToDevice, c->stream));
    HB_HIP(hipMemsetAsync(s.d_cnt.get(), 0, 4 * sizeof(unsigned long long), c->stream));
    hbk::ScParams sp{};
    sp.req = s.d_req.get();
    sp.rect = s.d_rect.get();
    sp.limit = o.limit;
    sp.slots = U;
    sp.node_idx = s.d_node_idx.get();
    sp.anchor_idx = s.d_anchor_idx.get();
    sp.lists = s.d_lists.get();
    sp.len = s.d_len.get();
    sp.mask = s.d_mask.get();
    sp.pair = s.d_pair.get();
    sp.cnt = s.d_cnt.get();
    sp.acc = s.d_acc.get();
    sp.score = s.d_score.get();
    for (size_t k = 0; k + 1 < pieces.piece_begin.size(); k++) {
        const hbk::ScRect *first = pieces.rect.data() + pieces.piece_begin[k];
        const uint64_t rects = pieces.piece_begin[k + 1] - pieces.piece_begin[k];
        const hbk::ScRect &last = first[rects - 1];
        const uint64_t groups = last.group_base + (uint64_t)last.nodes * last.tiles;
        if (groups >= (1ull << 31)) return fail(c, HB_ERR_INVALID, who + ": a piece with too many workgroups (internal error)");
        sp.rects = (uint32_t)rects;
        sp.lanes = last.lane_base + last.nodes;
        st.pieces++;
        HB_HIP(hipMemcpyAsync(s.d_rect.get(), first, rects * sizeof(hbk::ScRect), hipMemcpyHostToDevice, c->stream)); // (pageable: the copy is done when it returns)
        if (groups) {
            if ((rc = lap_start(c))) return rc;
            hipLaunchKernelGGL(hbk::sc_pair_kernel, dim3((unsigned)groups), dim3(256), 0, c->stream, sp);
            HB_HIP(hipGetLastError());
            if ((rc = lap(c, &st.ms_pairs))) return rc;
        }
        if ((rc = lap_start(c))) return rc;
        hipLaunchKernelGGL(hbk::sc_finish_kernel, dim3(grid_blocks(c, (sp.lanes + 255) / 256, 8, 1)), dim3(256), 0, c->stream, sp);
        HB_HIP(hipGetLastError());
        if ((rc = lap(c, &st.ms_finish))) return rc; // (drains the stream: the next piece may overwrite the rectangles)
    }
    unsigned long long *h64 = c->h_counters; // (pinned words of the context; hb_run rewrites them before it reads them)
    HB_HIP(hipMemcpyAsync(h64, s.d_cnt.get(), 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HB_HIP(hipMemcpyAsync(scores.data(), s.d_score.get(), N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HB_HIP(hipStreamSynchronize(c->stream));
    st.pairs_self = h64[0];
    st.pairs_empty = h64[1];
    st.pairs_gated = h64[2];
    st.pairs_intersected = h64[3];
    return finish();
}

const char *const kNoScores = "no score result (call hb_score_hosts)";

} // namespace

extern "C" {

int hb_score_hosts(hb_ctx *c, const hb_score_options *opt, hb_score_stats *stats)
{
    return operator_entry(c, "hb_score_hosts", [&]() { return score_hosts(c, opt, stats); });
}

int hb_score_count(hb_ctx *c, uint64_t *requests, uint64_t *scores)
{
    return reader_entry(c, c && c->sco.valid, "hb_score_count", kNoScores, [&]() -> int {
        if (requests) *requests = c->sco.offsets.size() - 1;
        if (scores) *scores = c->sco.scores.size();
        return HB_OK;
    });
}

int hb_score_copy(hb_ctx *c, uint64_t *offsets, double *scores, uint64_t cap)
{
    return reader_entry(c, c && c->sco.valid, "hb_score_copy", kNoScores, [&]() -> int {
        const auto &s = c->sco;
        if (scores && cap < s.scores.size()) return fail(c, HB_ERR_INVALID, "hb_score_copy: cap < the scores of hb_score_count");
        if (offsets) std::copy(s.offsets.begin(), s.offsets.end(), offsets);
        if (scores) std::copy(s.scores.begin(), s.scores.end(), scores);
        return HB_OK;
    });
}

} // extern "C"
