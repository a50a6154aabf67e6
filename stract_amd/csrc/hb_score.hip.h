// hb_score.hip.h - device code of hb_score_hosts: inbound_similarity::Scorer::score (crates/core/src/ranking/inbound_similarity.rs:44-50,
// 99-118) of the result hosts of a search against its liked / disliked hosts, as the InboundScorer stage calls it
// (ranking/pipeline/scorers/inbound_similarity.rs:38-54) - several searches per call.  Part of the hb_api.hip translation unit (included
// after hb_similar.hip.h and hb_similarity.hip.h).  Driver: hb_api_score.inc.  Definitions: include/hyperball.h.  DESIGN.md section 30.
//
// Every distinct known host of a call has a SLOT: its list of `limit` backlinks (links_lists, hb_api_links.inc) at lists[slot x limit],
// its degree and its bloom mask.  Every distinct id of a call, known or not, has an INDEX: the slot for a known host, a number from
// `slots` upwards for an id that is no node - two entries are the same NodeID exactly when their indices are equal.
//   bitvec:  sh_bitvec_body (hb_similar.hip.h) with the list stride `limit` and a sort of the next power of two.
//   pair:    the pair space of a call is walked in PIECES, a piece is a set of rectangles (request, node range, anchor range) of at most
//            `piece` pairs.  A workgroup takes one node of a rectangle and a tile of kScTile anchors; the node's sorted list is staged in
//            LDS once; each of the four waves takes anchors of the tile in turn.  Self, empty and gate are integer tests on values that
//            are the same in every lane of the wave, made before the anchor's list is touched.  For an intersected pair the lanes take
//            the ANCHOR's entries, 64 per step with one coalesced load, and binary-search each in the node's list in LDS - the
//            intersection is symmetric, and this way the searches run in LDS and the global loads are contiguous -; the step's hits are
//            counted with a ballot and a popcount.  No LDS atomics, no workgroup barrier inside the anchor loop.  One u32 per pair - the
//            count or a class code - goes to pair[base + anchor x nodes + node]: the finish kernel's lanes are nodes, so its reads
//            of one anchor are contiguous.
//   finish:  a lane per (rectangle, node): the anchors of the rectangle in caller order, the liked entries before the disliked ones, each
//            stored count turned into count / (sqrt(len_a) x sqrt(len_v)) and added in f64 to one of two sums; the sums of a node whose
//            anchors span several rectangles wait in acc[] between them, so the order of the additions is the caller's whatever the
//            piece size.  The last rectangle of a node applies sim_score (hb_similarity.hip.h): the score kernel of
//            hb_inbound_similarity and this one share the arithmetic.  A zero term is skipped as sim_accumulate_kernel skips it.
// Vector loads and stores only; the only atomics are vector atomic adds on the four u64 pair counters.  No inline assembly.
#pragma once

namespace hbk {

constexpr uint32_t kScMaxList = 1024; // entries of a list: hb_score_options.limit <= kLkMaxLimit
constexpr uint32_t kScTile = 16;      // anchors of a workgroup's tile: four per wave
constexpr uint32_t kScSelf = 0xFFFFFFFFu, kScEmpty = 0xFFFFFFFEu, kScGated = 0xFFFFFFFDu; // class codes of a pair; below them: the count

struct ScRequest {
    uint64_t node_off, anchor_off; // its nodes in node_idx, its anchors (liked, then disliked) in anchor_idx
    uint32_t liked, anchors;       // L, L + D
    double self_score, n_disliked, norm; // norm = max(L, 1) with HB_SIM_NORMALIZED, 0 = not (sim_score)
};

struct ScRect {
    uint32_t req, node0, nodes, anchor0, anchors, tiles; // tiles = ceil(anchors / kScTile)
    uint64_t pair_base;                                  // of its nodes x anchors words in the piece's pair array
    uint64_t group_base, lane_base;                      // its first workgroup of the pair kernel, its first lane of the finish kernel
};

struct ScParams {
    const ScRequest *req;
    const ScRect *rect;
    uint32_t rects, limit;
    uint64_t slots;
    const uint32_t *node_idx, *anchor_idx;
    const uint32_t *lists, *len;
    const unsigned long long *mask;
    uint32_t *pair;
    unsigned long long *cnt; // [0] self, [1] empty, [2] gated, [3] intersected
    double *acc, *score;     // per node of the call: 2 sums; the score
    uint64_t lanes;          // finish: nodes of all rectangles of the piece
};

// a workgroup per list: sorted by sid in place, its bloom mask; sort_n = the power of two the limit rounds up to
__global__ __launch_bounds__(256) void sc_bitvec_kernel(uint32_t *lists, const uint32_t *len, uint32_t limit, uint32_t sort_n, const uint32_t *dev_of,
                                                        const uint64_t *idlow, uint64_t n, unsigned long long *mask)
{
    __shared__ uint32_t s_v[kScMaxList];
    __shared__ unsigned long long s_mask;
    sh_bitvec_body(s_v, &s_mask, sort_n, limit, lists, len, dev_of, idlow, n, mask);
}

// the rectangle that holds position `at` of the ascending bases base(r) (group_base or lane_base); rectangles without a position repeat
// the base of their successor and are passed over
template <class BASE>
__device__ __forceinline__ uint32_t sc_find_rect(const ScRect *rect, uint32_t rects, uint64_t at, BASE base)
{
    uint32_t lo = 0, hi = rects;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (base(rect[mid]) <= at) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void sc_pair_kernel(const ScParams p)
{
    __shared__ uint32_t s_v[kScMaxList];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const ScRect r = p.rect[sc_find_rect(p.rect, p.rects, blockIdx.x, [](const ScRect &x) { return x.group_base; })];
    const uint64_t group = blockIdx.x - r.group_base;
    HB_DBG_ASSERT(r.tiles && group < (uint64_t)r.nodes * r.tiles);
    const uint32_t node = (uint32_t)(group / r.tiles), tile = (uint32_t)(group % r.tiles);
    const ScRequest q = p.req[r.req];
    const uint32_t vidx = p.node_idx[q.node_off + r.node0 + node];
    uint32_t lv = 0;
    unsigned long long mv = 0ull;
    if (vidx < p.slots) {
        lv = p.len[vidx] < p.limit ? p.len[vidx] : p.limit;
        mv = p.mask[vidx];
        for (uint32_t i = threadIdx.x; i < lv; i += 256) s_v[i] = p.lists[(uint64_t)vidx * p.limit + i];
    }
    __syncthreads();
    const uint32_t pv = (uint32_t)__popcll(mv);
    const uint32_t a_end = (tile + 1) * kScTile < r.anchors ? (tile + 1) * kScTile : r.anchors;
    unsigned long long c_self = 0, c_empty = 0, c_gated = 0, c_inter = 0;
    for (uint32_t a = tile * kScTile + (uint32_t)wave; a < a_end; a += 4) { // the same pair in every lane of the wave
        const uint32_t aidx = p.anchor_idx[q.anchor_off + r.anchor0 + a];
        uint32_t code;
        if (aidx == vidx) {
            code = kScSelf;
            c_self++;
        } else {
            const uint32_t la = aidx < p.slots ? (p.len[aidx] < p.limit ? p.len[aidx] : p.limit) : 0u;
            const unsigned long long ma = la ? p.mask[aidx] : 0ull;
            const uint32_t pa = (uint32_t)__popcll(ma);
            if (!la || !lv) {
                code = kScEmpty;
                c_empty++;
            } else if (4u * (uint32_t)__popcll(ma & mv) < (pa > pv ? pa : pv)) {
                code = kScGated;
                c_gated++;
            } else {
                // the lanes split the ANCHOR's entries (one coalesced load a step) and search the NODE's list in LDS: the count is that of
                // the other split - the node's entries searched in the anchor's list in global memory - with the probes in LDS
                const uint32_t *alist = p.lists + (uint64_t)aidx * p.limit;
                code = 0;
                for (uint32_t j0 = 0; j0 < la; j0 += 64) {
                    const uint32_t j = j0 + (uint32_t)lane;
                    const bool hit = j < la && sh_contains(s_v, lv, alist[j]);
                    code += (uint32_t)__popcll(__ballot(hit));
                }
                c_inter++;
            }
        }
        if (lane == 0) p.pair[r.pair_base + (uint64_t)a * r.nodes + node] = code;
    }
    if (lane == 0) {
        if (c_self) atomicAdd(&p.cnt[0], c_self);
        if (c_empty) atomicAdd(&p.cnt[1], c_empty);
        if (c_gated) atomicAdd(&p.cnt[2], c_gated);
        if (c_inter) atomicAdd(&p.cnt[3], c_inter);
    }
}

__global__ __launch_bounds__(256) void sc_finish_kernel(const ScParams p)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t at = (uint64_t)blockIdx.x * 256 + threadIdx.x; at < p.lanes; at += stride) {
        const ScRect r = p.rect[sc_find_rect(p.rect, p.rects, at, [](const ScRect &x) { return x.lane_base; })];
        const uint32_t node = (uint32_t)(at - r.lane_base);
        HB_DBG_ASSERT(node < r.nodes);
        const ScRequest q = p.req[r.req];
        const uint64_t g = q.node_off + r.node0 + node;
        const uint32_t vidx = p.node_idx[g];
        const uint32_t lv = vidx < p.slots ? (p.len[vidx] < p.limit ? p.len[vidx] : p.limit) : 0u;
        double liked = 0.0, disliked = 0.0;
        if (r.anchor0) {
            liked = p.acc[g * 2];
            disliked = p.acc[g * 2 + 1];
        }
        for (uint32_t a = 0; a < r.anchors; a++) {
            const uint32_t code = p.pair[r.pair_base + (uint64_t)a * r.nodes + node];
            double term = 0.0;
            if (code == kScSelf) term = q.self_score;
            else if (code < kScGated && code) {
                const uint32_t aidx = p.anchor_idx[q.anchor_off + r.anchor0 + a];
                HB_DBG_ASSERT(aidx < p.slots && code <= lv);
                const uint32_t la = p.len[aidx] < p.limit ? p.len[aidx] : p.limit;
                term = (double)code / (sqrt((double)la) * sqrt((double)lv));
            }
            if (term == 0.0) continue;
            if (r.anchor0 + a < q.liked) liked += term;
            else disliked += term;
        }
        if (r.anchor0 + r.anchors == q.anchors) p.score[g] = sim_score(liked, disliked, q.n_disliked, q.norm);
        else {
            p.acc[g * 2] = liked;
            p.acc[g * 2 + 1] = disliked;
        }
    }
}

} // namespace hbk
