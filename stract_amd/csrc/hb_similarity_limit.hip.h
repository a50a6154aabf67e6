// hb_similarity_limit.hip.h - device code of the limited mode of hb_inbound_similarity (hb_similarity_options.limit = L, 1 .. 1024): the
// BitVec of every node v is built from backlinks(v, L) as hb_backlinks defines it under the current key set - the in-neighbours u != v
// in the order (key[u], NodeID u), the first min(L, degree(v)) of them - instead of the whole in-list.  Part of the hb_api.hip translation
// unit (included after hb_similarity.hip.h and hb_links.hip.h).  Driver: hb_api_similarity.inc.  Definitions: include/hyperball.h.
// DESIGN.md section 29.
//
// A node row is LISTED when its cut list differs from its list as loaded: degree(v) > L, or v has a self link.  Listed rows get an
// explicit cut list of stride L (list k = lists[k L .. k L + len_l[k]), entries are device rows), their len and bloom; every other row
// keeps the plan's list, in-degree and bloom, which are already those of its cut.  Per graph, key set and limit:
//   self:    one pass over the plan's lists (a quad per row); a chunk row answers for the node row at the top of its tree (top_row,
//            fw_top_row_kernel).  flag[row] = 1 where the row's list holds the row itself.
//   mark:    flag[row] = listed, from the self flag and the plan's in-degree minus it.
//   assign:  idx[row] = the list index (kNone: not listed) from the exclusive prefix sums of the flags - the lists lie in row order -,
//            list_row[k] = the row, sids[k] = its sid: what the list builder is asked for.
//   finish:  (per piece of the list builder) a wave per list: the sids become device rows, len_l = min(degree, L), bloom_l = OR of
//            1 << pos[entry] over THOSE entries.
// Per batch of 16 anchors:
//   seed:    a listed anchor marks its indicators from its stored list (sim_seed_list_kernel; every entry is a node row); the others
//            seed as ever (seed_rows = the anchors' rows with the listed ones taken out).
//   count:   after the shared walk level - right for every unlisted row - a wave per listed row sums the 64-byte indicator rows of its
//            list entries whose level-0 bit is set, a lane quad per such entry, and OVERWRITES the row's count row and its bit of the
//            level-1 bitmap (the counters say how many bits it set and cleared: rows_nonzero follows).
// Vector loads and stores, wave shuffles and u32 / u64 vector atomics only; no LDS, no scratch, no floating point.
#pragma once

namespace hbk {

__global__ __launch_bounds__(256) void siml_self_kernel(const uint64_t *row_ptr, const uint32_t *src, const uint32_t *top_row, uint64_t n_pad, uint64_t rows_total,
                                                        uint32_t *flag)
{
    const int q = threadIdx.x & 3;
    const uint64_t quad = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 2, stride = (uint64_t)gridDim.x * 64;
    for (uint64_t row = quad; row < rows_total; row += stride) {
        const uint32_t owner = row < n_pad ? (uint32_t)row : top_row[row - n_pad];
        if (owner == kNone) continue; // (a padding chunk row: no list)
        HB_DBG_ASSERT(owner < n_pad);
        const uint64_t end = row_ptr[row + 1];
        for (uint64_t e = row_ptr[row] + q; e < end; e += 4)
            if (src[e] == owner) flag[owner] = 1u; // (edges are unique: one writer)
    }
}

// flag: in = the row has a self link, out = the row is listed
__global__ __launch_bounds__(256) void siml_mark_kernel(const uint32_t *sid_of, const uint32_t *indeg, uint32_t limit, uint64_t n_pad, uint32_t *flag)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n_pad; r += stride) {
        const uint32_t self = flag[r];
        HB_DBG_ASSERT(self <= 1u && indeg[r] >= self);
        flag[r] = (sid_of[r] != kNone && (self || indeg[r] - self > limit)) ? 1u : 0u;
    }
}

__global__ __launch_bounds__(256) void siml_assign_kernel(const uint32_t *sid_of, const uint32_t *flag, const uint64_t *off, uint64_t n_pad, uint64_t listed,
                                                          uint32_t *idx, uint32_t *list_row, uint32_t *sids)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n_pad; r += stride) {
        if (!flag[r]) {
            idx[r] = kNone;
            continue;
        }
        const uint64_t k = off[r];
        HB_DBG_ASSERT(k < listed);
        (void)listed;
        idx[r] = (uint32_t)k;
        list_row[k] = (uint32_t)r;
        sids[k] = sid_of[r];
    }
}

// the lists [0, count) of a piece as the list builder left them (sids in list order, deg = degree(v) without the self link)
__global__ __launch_bounds__(256) void siml_finish_kernel(uint32_t *lists, const uint32_t *deg, const uint32_t *dev_of, const uint8_t *pos, uint64_t count,
                                                          uint32_t limit, uint64_t n, uint64_t n_pad, uint32_t *len_l, uint64_t *bloom_l)
{
    const int lane = threadIdx.x & 63;
    const uint64_t wid = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * 4;
    for (uint64_t k = wid; k < count; k += nwaves) { // wave-uniform
        const uint32_t len = deg[k] < limit ? deg[k] : limit;
        uint32_t *list = lists + k * limit;
        unsigned long long m = 0;
        for (uint32_t i = lane; i < len; i += 64) {
            const uint32_t sid = list[i];
            HB_DBG_ASSERT(sid < n);
            const uint32_t row = dev_of[sid];
            HB_DBG_ASSERT(row < n_pad);
            list[i] = row;
            m |= 1ull << pos[row];
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) m |= __shfl_xor(m, off);
        if (lane == 0) {
            len_l[k] = len;
            bloom_l[k] = m;
        }
    }
    (void)n;
    (void)n_pad;
}

// ---- seed --------------------------------------------------------------------------------------------------------------------------
// seed_rows[j] = the anchor's row where sim_seed_node_kernel walks the plan's list, kNone where the anchor is listed (or no node)
__global__ __launch_bounds__(64) void sim_seed_rows_kernel(const uint32_t *rows, uint32_t count, const uint32_t *idx, uint32_t *seed_rows)
{
    const uint32_t j = threadIdx.x;
    if (j >= kSimSlots) return;
    const uint32_t row = j < count ? rows[j] : kNone;
    seed_rows[j] = (row != kNone && idx[row] == kNone) ? row : kNone;
}

// workgroup j marks the stored list of anchor j, if it has one
__global__ __launch_bounds__(256) void sim_seed_list_kernel(const uint32_t *rows, uint32_t count, const uint32_t *idx, const uint32_t *lists, const uint32_t *len_l,
                                                            uint32_t limit, uint32_t *ind, uint32_t *bits, uint32_t *vmask, const uint32_t *outdeg, uint64_t n_pad,
                                                            uint64_t rows_total, unsigned long long *cnt)
{
    unsigned long long c_rows = 0, c_out = 0;
    const uint32_t j = blockIdx.x;
    const uint32_t row = j < count ? rows[j] : kNone;
    const uint32_t k = row != kNone ? idx[row] : kNone;
    if (k != kNone) {
        const uint32_t len = len_l[k];
        const uint32_t *list = lists + (uint64_t)k * limit;
        for (uint32_t i = threadIdx.x; i < len; i += 256) {
            HB_DBG_ASSERT(list[i] < n_pad);
            sim_mark(list[i], 1u << j, ind, bits, vmask, outdeg, n_pad, rows_total, c_rows, c_out);
        }
    }
    wave_add_counters(cnt, c_rows, c_out, 0ull);
}

// ---- count -------------------------------------------------------------------------------------------------------------------------
struct SimListParams {
    const uint4 *rd;          // node rows: the indicators (level 0)
    const uint32_t *bits_rd;  // the level-0 bitmap: a row without its bit holds no indicator
    uint4 *wr;                // node rows: the counts (level 1)
    uint32_t *bits_wr;        // the level-1 bitmap
    const uint32_t *list_row; // listed: the device row of list k
    const uint32_t *lists;    // listed x limit
    const uint32_t *len_l;    // listed
    unsigned long long *cnt;  // [0] += bits set, [1] += bits cleared, [2] += entries gathered
    uint64_t listed, n_pad;
    uint32_t limit;
};

// a wave per listed row.  64 entries a step (four steps loaded at once), a lane each: the entry and its level-0 bit (a row without the bit holds no indicator: 4
// bytes of list and a bit instead of 64 bytes of row - the seed marks few rows of a graph).  The marked entries of the step are then
// gathered sixteen a round: lane quad g takes the g-th of them, lane q of it the words 4 q .. 4 q + 3 of its indicator row
__global__ __launch_bounds__(256) void sim_list_count_kernel(const SimListParams p)
{
    const int lane = threadIdx.x & 63, g = lane >> 2, q = lane & 3;
    const uint64_t wid = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * 4;
    unsigned long long c_set = 0, c_clr = 0, c_gath = 0;
    for (uint64_t k = wid; k < p.listed; k += nwaves) { // wave-uniform
        const uint32_t len = p.len_l[k];
        const uint32_t *list = p.lists + k * p.limit;
        uint4 acc = make_uint4(0, 0, 0, 0);
        for (uint32_t i0 = 0; i0 < len; i0 += 256) { // wave-uniform; four steps' entries, then their bit words: independent loads in flight
            uint32_t s[4], w[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint32_t i = i0 + 64u * u + (uint32_t)lane;
                s[u] = i < len ? list[i] : kNone;
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                HB_DBG_ASSERT(s[u] == kNone || s[u] < p.n_pad);
                w[u] = s[u] != kNone ? p.bits_rd[s[u] >> 5] : 0u;
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                uint64_t m = __ballot((w[u] >> (s[u] & 31u)) & 1u); // the marked entries of this step, by lane
                while (m) { // wave-uniform: m is the same in every lane
                    int from = -1;
                    for (int t = 0; t < 16 && m; t++) { // the sixteen lowest set bits, the t-th to quad t
                        if (t == g) from = __ffsll((long long)m) - 1;
                        m &= m - 1;
                    }
                    const uint32_t sv = __shfl(s[u], from < 0 ? lane : from);
                    if (from >= 0) {
                        acc = u4_add(acc, p.rd[(uint64_t)sv * 4 + q]);
                        if (q == 0) c_gath++;
                    }
                }
            }
        }
#pragma unroll
        for (int off = 4; off <= 32; off <<= 1)
            acc = u4_add(acc, make_uint4(__shfl_xor(acc.x, off), __shfl_xor(acc.y, off), __shfl_xor(acc.z, off), __shfl_xor(acc.w, off)));
        const bool nonzero = (__ballot((acc.x | acc.y | acc.z | acc.w) != 0u) & 0xFull) != 0; // (every quad holds the sums)
        const uint32_t row = p.list_row[k];
        HB_DBG_ASSERT(row < p.n_pad);
        if (nonzero && g == 0) p.wr[(uint64_t)row * 4 + q] = acc;
        if (lane == 0) {
            const uint32_t bit = 1u << (row & 31u);
            const uint32_t old = nonzero ? atomicOr(&p.bits_wr[row >> 5], bit) : atomicAnd(&p.bits_wr[row >> 5], ~bit);
            if (nonzero && !(old & bit)) c_set++;
            if (!nonzero && (old & bit)) c_clr++;
        }
    }
    wave_add_counters(p.cnt, c_set, c_clr, c_gath);
}

} // namespace hbk
