// hb_similarity.hip.h - device code of hb_inbound_similarity (Scorer, crates/core/src/ranking/inbound_similarity.rs:61-138, over BitVec,
// ranking/bitvec_similarity.rs:131-189): the inbound similarity of EVERY node to 16 anchors (liked / disliked hosts) at once over the
// HyperBall device plan.  Part of the hb_api.hip translation unit (included after hb_betweenness.hip.h; the count level is a walk of
// hb_walk.hip.h).  Driver: hb_api_similarity.inc.  Definitions: include/hyperball.h.
//
// Defined differences from the reference: with hb_similarity_options.limit == 0 the in-neighbour set of a node is its WHOLE in-list in
// the loaded graph (unique edges, self links as loaded, the relation filter of the load: HB_SKIPPED_REL_MASK, nothing with
// HB_FLAG_ALL_RELS); the reference takes EdgeLimit::Limit(512) backlinks in search order before it filters.  limit = L cuts every list as
// hb_backlinks defines the cut (hb_similarity_limit.hip.h: explicit cut lists for the rows whose cut differs from their list as loaded);
// the differences that remain are that operator's.
//
// Per graph: pos[row] = (low id word x 11400714819323198549) & 63 - both bloom indices of VeryJankyBloomFilter::hash come from that one
// product and 16 divides 64, so the word is determined by the bit and the 16-word bloom is exactly one u64 mask; bloom[row] = OR of
// 1 << pos[src] over the in-list, pulled through the chunk trees like a pass (a u64 partial per chunk row); len[row] = the in-degree
// (bfs_indegree_kernel, hb_bfs.hip.h).
// Per batch of 16 anchors: a row of 64 bytes holds sixteen u32, lane q of the quad owning slots 4 q .. 4 q + 3.
//   seed:  row u gets indicator 1 in word j when u -> anchor j, and its bit in the level-0 bitmap.  An anchor's in-list is its node row's
//          list with the chunk rows resolved downwards (a mask of anchor slots per chunk row, the highest virtual level first).  Every
//          (row, slot) word has one writer: edges are unique, a chunk row has one reader, a duplicate anchor has a slot of its own.
//   count: ONE forward level of hb_walk.hip.h with a plain add as the join (a count is bounded by the in-degree < 2^30): the row that
//          arrives at v holds |in(v) & in(anchor j)| in word j.  A row's bit at level 1 = "its count row is non-zero"; only such rows are
//          stored, and only they are read afterwards.
//   accumulate: per node row, in slot order, each slot's term - self_score, sim, or nothing - into acc_liked / acc_disliked.  f64
//          arithmetic exactly as BitVec::sim writes it: one multiply of the two square roots (IEEE sqrt of an exact integer), one
//          division, no FMA contraction, no floating-point atomics.  A zero term is skipped: x + 0.0 == x for every sum that can occur.
// After the last batch the score kernel writes max(0, (D + (acc_liked - acc_disliked)) [/ max(L, 1)]) per node in ascending-NodeID order.
#pragma once

namespace hbk {

constexpr uint32_t kSimSlots = 16;                          // anchors per batch: the u32 words of one 64-byte row
constexpr uint64_t kSimBloomMul = 11400714819323198549ull;  // bitvec_similarity.rs:38-39

struct SimParams : WalkParams { // a row's bit = "its count row is non-zero"; cnt[0] = such node rows, cnt[2] = entries gathered
    const uint4 *rd;          // node rows: the indicators (level 0)
    uint4 *wr;                // node rows: the counts (level 1), stored where non-zero
    uint4 *part;              // virtual rows, indexed by vid - n_pad
};

__device__ __forceinline__ uint4 u4_add(uint4 a, uint4 b) { return make_uint4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// ---- per graph ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sim_pos_kernel(const uint64_t *idlow, const uint32_t *sid_of, uint64_t n_pad, uint8_t *pos)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n_pad; r += stride)
        pos[r] = sid_of[r] != kNone ? (uint8_t)((idlow[r] * kSimBloomMul) & 63ull) : (uint8_t)0;
}

// bloom of the rows [row_lo, row_hi) of one kind (the virtual levels ascending, then the node rows): a quad per row, lane q takes the
// entries q, q + 4, ...; node sources contribute 1 << pos, virtual sources their partial
__global__ __launch_bounds__(256) void sim_bloom_kernel(const uint64_t *row_ptr, const uint32_t *src, const uint8_t *pos, uint64_t *bloom, uint64_t n_pad,
                                                        uint64_t rows_total, uint64_t row_lo, uint64_t row_hi)
{
    const int q = threadIdx.x & 3;
    const uint64_t quad = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 2, stride = (uint64_t)gridDim.x * 64;
    for (uint64_t r0 = row_lo; r0 < row_hi; r0 += stride) { // wave-uniform trip count
        const uint64_t row = r0 + quad;
        unsigned long long m = 0;
        if (row < row_hi) {
            const uint64_t end = row_ptr[row + 1];
            for (uint64_t e = row_ptr[row] + q; e < end; e += 4) {
                const uint32_t s = src[e];
                if (s == kNone) continue;
                HB_DBG_ASSERT(s < rows_total);
                m |= s < n_pad ? 1ull << pos[s] : (unsigned long long)bloom[s];
            }
        }
        m |= __shfl_xor(m, 1);
        m |= __shfl_xor(m, 2);
        if (row < row_hi && q == 0) bloom[row] = m;
    }
    (void)rows_total;
}

// ---- seed --------------------------------------------------------------------------------------------------------------------------
// source `s` of a list that belongs to the anchor slots in `mask`: a node row gets its indicators and its level-0 bit (the lane that
// sets the bit counts the row), a chunk row collects the mask
__device__ __forceinline__ void sim_mark(uint32_t s, uint32_t mask, uint32_t *ind, uint32_t *bits, uint32_t *vmask, const uint32_t *outdeg, uint64_t n_pad,
                                         uint64_t rows_total, unsigned long long &rows, unsigned long long &out)
{
    if (s == kNone) return;
    HB_DBG_ASSERT(s < rows_total);
    (void)rows_total;
    if (s >= n_pad) {
        atomicOr(&vmask[s - n_pad], mask);
        return;
    }
    for (uint32_t m = mask; m; m &= m - 1) ind[(uint64_t)s * kSimSlots + (uint32_t)(__ffs((int)m) - 1)] = 1u;
    const uint32_t bit = 1u << (s & 31u);
    if (!(atomicOr(&bits[s >> 5], bit) & bit)) {
        rows++;
        out += outdeg[s];
    }
}

// the anchors' own node rows: workgroup j walks the list of anchor j (rows[j] = its device row, kNone = no node of the graph)
__global__ __launch_bounds__(256) void sim_seed_node_kernel(const uint32_t *rows, uint32_t count, const uint64_t *row_ptr, const uint32_t *src, uint32_t *ind,
                                                            uint32_t *bits, uint32_t *vmask, const uint32_t *outdeg, uint64_t n_pad, uint64_t rows_total,
                                                            unsigned long long *cnt)
{
    unsigned long long c_rows = 0, c_out = 0;
    const uint32_t j = blockIdx.x;
    const uint32_t row = j < count ? rows[j] : kNone;
    if (row != kNone) {
        HB_DBG_ASSERT(row < n_pad);
        const uint64_t end = row_ptr[row + 1];
        for (uint64_t e = row_ptr[row] + threadIdx.x; e < end; e += 256) sim_mark(src[e], 1u << j, ind, bits, vmask, outdeg, n_pad, rows_total, c_rows, c_out);
    }
    wave_add_counters(cnt, c_rows, c_out, 0ull);
}

// one virtual level (the launches run from the highest level to the first): a chunk row some anchor's list reaches hands its mask down.
// A wave per row, grid-stride.
__global__ __launch_bounds__(256) void sim_seed_virt_kernel(const uint64_t *row_ptr, const uint32_t *src, uint32_t *ind, uint32_t *bits, uint32_t *vmask,
                                                            const uint32_t *outdeg, uint64_t n_pad, uint64_t rows_total, uint64_t row_lo, uint64_t row_hi,
                                                            unsigned long long *cnt)
{
    unsigned long long c_rows = 0, c_out = 0;
    const int lane = threadIdx.x & 63;
    const uint64_t wid = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * 4;
    for (uint64_t row = row_lo + wid; row < row_hi; row += nwaves) { // wave-uniform
        const uint32_t mask = vmask[row - n_pad]; // (written by earlier launches only: a row's readers lie on higher levels)
        if (!mask) continue;
        const uint64_t end = row_ptr[row + 1];
        for (uint64_t e = row_ptr[row] + lane; e < end; e += 64) sim_mark(src[e], mask, ind, bits, vmask, outdeg, n_pad, rows_total, c_rows, c_out);
    }
    wave_add_counters(cnt, c_rows, c_out, 0ull);
}

// ---- count: one forward level over the rows [row_lo, row_hi) of one kind -------------------------------------------------------------
//   !REAL: virtual rows: partial = sum of the sources (dense: all of them, the partial is rebuilt; else those with a set bit, stored
//          when non-zero); sweep: a non-zero partial touches its readers.
//   REAL:  node rows: the counts, stored when non-zero.
template <bool REAL, int MODE>
__global__ __launch_bounds__(256) void sim_count_kernel(const SimParams p)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 2, q = lane & 3, qshift = lane & ~3;
    const WalkSpan sp = walk_span<REAL>(p, wave);
    const uint4 *vbase = walk_virtual_base<uint4>(p.part, p.n_pad);
    unsigned long long c_rows = 0, c_gath = 0;
    for (uint64_t wi = sp.wid; wi < sp.nwords; wi += sp.wstride) { // wave-uniform trip count
        const uint64_t w = sp.w_lo + wi;
        const uint32_t tw = walk_take_touch<MODE>(p, w, lane);
        if (MODE == kModeSweep && tw == 0) { // nothing to visit in this word
            walk_store_bits<REAL>(p, w, 0u, lane);
            continue;
        }
        uint32_t chw = 0;
        for (int h = 0; h < 2; h++) {
            const uint32_t bit = (uint32_t)(h * 16 + g);
            const uint64_t row = (w << 5) + bit;
            const bool valid = row < sp.row_hi;
            const bool active = valid && ((tw >> bit) & 1u);
            const uint4 acc = walk_gather<MODE>(p, p.rd, vbase, row, active, q, make_uint4(0, 0, 0, 0), u4_add, [&] {
                if (q == 0) c_gath++;
            });
            const uint64_t bal = __ballot(active && (acc.x | acc.y | acc.z | acc.w) != 0u);
            const bool nonzero = ((bal >> qshift) & 0xFull) != 0;
            if (REAL) {
                if (nonzero) p.wr[row * 4 + q] = acc;
                if (nonzero && q == 0) c_rows++;
            } else {
                if (active && (MODE == kModeDense || nonzero)) p.part[(row - p.n_pad) * 4 + q] = acc;
                if (MODE == kModeSweep && nonzero) walk_touch_readers(p, row, q);
            }
            chw |= pack16(bal) << (16 * h);
        }
        walk_store_bits<REAL>(p, w, chw, lane);
    }
    wave_add_counters(p.cnt, c_rows, 0ull, c_gath);
}

// ---- accumulate and score ------------------------------------------------------------------------------------------------------------
struct SimAccParams {
    const uint32_t *anchor_rows; // kSimSlots: device row of the batch's anchor j, kNone = no node of the graph
    uint32_t count;              // slots of this batch
    uint32_t liked;              // the slots below this one are liked entries, the others disliked ones
    const uint32_t *counts;      // n_pad x 16, valid where the row's bit is set
    const uint32_t *bits;        // the level-1 bitmap
    const uint32_t *len;         // in-degree per row
    const uint64_t *bloom;
    const uint32_t *lidx;        // limited mode (hb_similarity_limit.hip.h): the list index per node row, kNone = the row keeps len / bloom
                                 // above; NULL = whole in-lists
    const uint32_t *len_l;       // ... per list: min(degree, limit)
    const uint64_t *bloom_l;     // ... and the bloom over the cut entries
    double *acc;                 // n_pad x 2: liked, disliked
    double self_score;
    uint64_t n_pad;
};

// BitVec::sim (bitvec_similarity.rs:165-180) of a node (len_v, bloom_v) and an anchor with `inter` common in-neighbours; the ratio test
// intersect_ones / max_ones < 0.25 in integers (for max_ones <= 1024 the f64 quotient is never within an ulp of 0.25)
__device__ __forceinline__ double sim_term(uint32_t inter, uint32_t len_v, unsigned long long bloom_v, uint32_t len_a, unsigned long long bloom_a)
{
    if (len_v == 0 || len_a == 0) return 0.0;
    const int ones_v = __popcll(bloom_v), ones_a = __popcll(bloom_a);
    const int max_ones = ones_v > ones_a ? ones_v : ones_a;
    if (4 * __popcll(bloom_v & bloom_a) < max_ones) return 0.0;
    return (double)inter / (sqrt((double)len_a) * sqrt((double)len_v));
}

// len and bloom of a node row: the cut list's where the row has one
__device__ __forceinline__ void sim_len_bloom(const uint32_t *len, const uint64_t *bloom, const uint32_t *lidx, const uint32_t *len_l, const uint64_t *bloom_l,
                                              uint64_t row, uint32_t &len_v, unsigned long long &bloom_v)
{
    const uint32_t k = lidx ? lidx[row] : kNone;
    len_v = k != kNone ? len_l[k] : len[row];
    bloom_v = k != kNone ? bloom_l[k] : bloom[row];
}

// a thread per node row; the slots in order, so every sum is the reference's sequential one
__global__ __launch_bounds__(256) void sim_accumulate_kernel(const SimAccParams p)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t row = (uint64_t)blockIdx.x * 256 + threadIdx.x; row < p.n_pad; row += stride) {
        const bool has = (p.bits[row >> 5] >> (row & 31u)) & 1u;
        uint32_t len_v, len_a;
        unsigned long long bloom_v, bloom_a;
        sim_len_bloom(p.len, p.bloom, p.lidx, p.len_l, p.bloom_l, row, len_v, bloom_v);
        double liked = p.acc[row * 2], disliked = p.acc[row * 2 + 1];
        for (uint32_t j = 0; j < p.count; j++) {
            const uint32_t a = p.anchor_rows[j];
            if (a == kNone) continue; // an empty BitVec: sim == 0
            double term;
            if (a == row) term = p.self_score;
            else if (!has) continue;
            else {
                sim_len_bloom(p.len, p.bloom, p.lidx, p.len_l, p.bloom_l, a, len_a, bloom_a);
                term = sim_term(p.counts[row * kSimSlots + j], len_v, bloom_v, len_a, bloom_a);
            }
            if (term == 0.0) continue;
            if (j < p.liked) liked += term;
            else disliked += term;
        }
        p.acc[row * 2] = liked;
        p.acc[row * 2 + 1] = disliked;
    }
}

// Scorer::calculate_score (inbound_similarity.rs:99-118) from the two sums
__device__ __forceinline__ double sim_score(double liked, double disliked, double n_disliked, double norm)
{
    double s = n_disliked + (liked - disliked);
    if (norm != 0.0) s = s / norm;
    return s > 0.0 ? s : 0.0;
}

// the result in ascending-NodeID (sid) order; norm = max(L, 1) when normalized, 0 = not
__global__ __launch_bounds__(256) void sim_score_kernel(const double *acc, const uint32_t *dev_of, uint64_t n, double n_disliked, double norm, double *score)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s < n; s += stride) {
        const uint64_t row = dev_of[s];
        score[s] = sim_score(acc[row * 2], acc[row * 2 + 1], n_disliked, norm);
    }
}

// the anchors of a batch: rows[j] = the device row of entry j (kNone = no node of the graph), and anchor[sid] = 1 for the known ones
// (HB_SIM_TOP_SKIP_ANCHORS); a sid that fills several slots is flagged by the first of them
__global__ __launch_bounds__(64) void sim_anchor_rows_kernel(const uint32_t *sids, uint32_t count, const uint32_t *dev_of, uint32_t *rows, uint8_t *anchor)
{
    const uint32_t j = threadIdx.x;
    if (j >= kSimSlots) return;
    const uint32_t sid = j < count ? sids[j] : kNone;
    rows[j] = sid != kNone ? dev_of[sid] : kNone;
    if (sid == kNone) return;
    for (uint32_t i = 0; i < j; i++)
        if (sids[i] == sid) return;
    anchor[sid] = 1;
}

// hb_similarity_lookup: out[i] = score[sids[i]]; kNone (no node) is left to the host
__global__ __launch_bounds__(256) void sim_lookup_kernel(const double *score, const uint32_t *sids, uint64_t count, double *out)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += stride) out[i] = sids[i] != kNone ? score[sids[i]] : 0.0;
}

// hb_similarity_top: the sort key of every sid (a score is never negative: its bits order like its value) and whether it takes part
__global__ __launch_bounds__(256) void sim_top_keys_kernel(const double *score, const uint8_t *anchor, int skip_anchors, uint64_t n, uint64_t *key, uint8_t *keep)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s < n; s += stride) {
        key[s] = (uint64_t)__double_as_longlong(score[s]);
        keep[s] = (skip_anchors && anchor[s]) ? 0 : 1;
    }
}

// debug export: counts / bloom / len of device row -> sid order (rows without a set bit have no counts; bits == NULL: no counts at all;
// lidx / len_l / bloom_l as in SimAccParams)
__global__ __launch_bounds__(256) void sim_export_kernel(const uint32_t *counts, const uint32_t *bits, const uint64_t *bloom, const uint32_t *len,
                                                         const uint32_t *lidx, const uint32_t *len_l, const uint64_t *bloom_l, const uint32_t *dev_of, uint64_t n,
                                                         uint32_t *o_counts, uint64_t *o_bloom, uint32_t *o_len)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s < n; s += stride) {
        const uint64_t row = dev_of[s];
        const bool has = bits && ((bits[row >> 5] >> (row & 31u)) & 1u);
        for (uint32_t j = 0; j < kSimSlots; j++) o_counts[s * kSimSlots + j] = has ? counts[row * kSimSlots + j] : 0u;
        uint32_t len_v;
        unsigned long long bloom_v;
        sim_len_bloom(len, bloom, lidx, len_l, bloom_l, row, len_v, bloom_v);
        o_bloom[s] = bloom_v;
        o_len[s] = len_v;
    }
}

} // namespace hbk
