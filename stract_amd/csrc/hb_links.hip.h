// hb_links.hip.h - device code of hb_links_set_keys / hb_backlinks (HostBacklinksQuery::new(node).with_limit(EdgeLimit::Limit(L)),
// webgraph/query/backlink.rs:230-360): the first L in-neighbours of each QUERIED host in the order (key, NodeID), listed in that order.
// Part of the hb_api.hip translation unit (included after hb_nearest_seed.hip.h).  Driver: hb_api_links.inc.  Definitions:
// include/hyperball.h.  DESIGN.md section 27.  The mirror, hb_forwardlinks (the first L OUT-neighbours: DESIGN.md section 28), shares
// the order, the select arithmetic (lk_value, lk_plan_kernel, lk_pick_kernel) and lk_sort_kernel; its own kernels are at the end of
// this file.
//
// The order is dense: ord[sid] = the position of the node in the sort by (key, sid), a u32 permutation built once per key set
// (lk_ord_kernel, from the device sort hb_ingest.hip exposes), inv = its inverse, ord_row = ord by device row.  ord values are unique,
// so the L-best list of a host is defined by ONE number - the L-th smallest ord of its in-list, its threshold - and its order by a sort
// of at most 1024 u32.  A batch holds `slots` distinct queried hosts:
//   expand: an item is (slot, row).  Level 0 = the queried node rows; a launch per level scans its items (16 lanes per item: a row is at
//           most a chunk long) and appends (slot, child row) for every entry >= n_pad behind the level - the children of a workgroup are
//           counted in LDS, reserved with ONE global atomic add and written on a second scan - and counts the node entries that are not the
//           slot's own node into deg[slot] (summed per item in LDS first).  Nothing assumes that a chunk row has one owner; an append past
//           the item buffer raises a flag instead of writing.
//   select: (slots with deg > limit) a most-significant-digit-first radix select on the 32-bit ord: per round a 256-bin histogram per
//           slot over the entries that match the prefix chosen so far - a workgroup walks a contiguous range of items and keeps the bins of
//           the slot its range is in in LDS, flushed with vector atomic adds when the slot changes - then lk_pick_kernel takes the digit
//           that holds the k-th entry and the k that remains.  After the last round thr[slot] = the limit-th smallest ord.
//   emit:   entries with ord <= thr[slot] go to the slot's `limit` output words through a per-slot cursor (exactly min(limit, deg) of
//           them: ord is unique), then a workgroup per slot sorts them in LDS (bitonic, padded with ~0) and writes sid = inv[ord] and
//           key[sid] to the result.
// The only atomics are vector atomic adds on counters, cursors and histogram bins; every store is an ordinary vector store.
#pragma once

namespace hbk {

constexpr int kLkLanes = 16;                // lanes per item
constexpr int kLkItems = 256 / kLkLanes;    // items per workgroup and step
constexpr uint32_t kLkMaxLimit = 1024;

// what a select round compares: ord, or ord * floor(2^32 / n) (HB_LINKS_SPREAD_ORDS: strictly monotone, so the same threshold entry)
__device__ __forceinline__ uint32_t lk_value(uint32_t ord, uint64_t mult) { return (uint32_t)((uint64_t)ord * mult); }

// ---- the order ------------------------------------------------------------------------------------------------------------------------
// rank[sid] / order[i] from gpu_rank_keys_device (NULL: no keys, the order is NodeID order)
__global__ __launch_bounds__(256) void lk_ord_kernel(const uint64_t *rank, const uint64_t *order, uint64_t n, uint32_t *ord, uint32_t *inv)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        HB_DBG_ASSERT(!rank || (rank[i] < n && order[i] < n));
        ord[i] = rank ? (uint32_t)rank[i] : (uint32_t)i;
        inv[i] = order ? (uint32_t)order[i] : (uint32_t)i;
    }
}

__global__ __launch_bounds__(256) void lk_ord_row_kernel(const uint32_t *ord, const uint32_t *sid_of, uint64_t n_pad, uint32_t *ord_row)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n_pad; r += stride) {
        const uint32_t sid = sid_of[r];
        ord_row[r] = sid != kNone ? ord[sid] : kNone;
    }
}

// ---- a batch --------------------------------------------------------------------------------------------------------------------------
struct LkBatch {
    const uint64_t *row_ptr;
    const uint32_t *src;
    const uint32_t *ord_row;   // n_pad
    uint2 *items;              // item_cap x (slot, row)
    const uint32_t *slot_row;  // slots: the queried node rows of this batch
    const uint32_t *slot_self; // slots: the row an entry must not be (the node's own row; kNone with HB_LINKS_KEEP_SELF)
    uint32_t *deg;             // slots
    uint32_t *sel_k;           // slots: the k of the select that remains, 0 = the slot does not select
    uint32_t *sel_prefix;      // slots: the digits chosen so far
    uint32_t *thr;             // slots: entries with value <= thr are kept
    uint32_t *cursor;          // slots: entries emitted
    uint32_t *hist;            // slots x 256
    uint32_t *out;             // slots x limit: the kept ords
    uint32_t *flag;            // [0] != 0: an append did not fit into items
    uint64_t n_pad, rows_total, item_cap, mult;
    uint32_t slots, limit;
};

// the distinct queried nodes of a call: slot_self holds their sids on entry
__global__ __launch_bounds__(256) void lk_rows_kernel(const uint32_t *dev_of, uint64_t count, uint32_t keep_self, uint32_t *slot_row, uint32_t *slot_self)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += stride) {
        const uint32_t row = dev_of[slot_self[i]];
        slot_row[i] = row;
        slot_self[i] = keep_self ? kNone : row;
    }
}

__global__ __launch_bounds__(256) void lk_seed_kernel(const LkBatch b)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < b.slots) b.items[i] = make_uint2(i, b.slot_row[i]);
}

// one level: the items [lo, hi) are scanned, their children appended at next_base + (*next_cnt)++
__global__ __launch_bounds__(256) void lk_expand_kernel(const LkBatch b, uint64_t lo, uint64_t hi, uint64_t next_base, uint32_t *next_cnt)
{
    __shared__ uint32_t s_children, s_base;
    __shared__ uint32_t s_deg[kLkItems];
    const int g = threadIdx.x / kLkLanes, l = threadIdx.x % kLkLanes;
    const uint64_t stride = (uint64_t)gridDim.x * kLkItems;
    for (uint64_t it0 = lo + (uint64_t)blockIdx.x * kLkItems; it0 < hi; it0 += stride) { // workgroup-uniform
        if (threadIdx.x < kLkItems) s_deg[threadIdx.x] = 0;
        if (threadIdx.x == 0) s_children = 0;
        __syncthreads();
        const uint64_t item = it0 + g;
        uint32_t nchild = 0, ndeg = 0, slot = 0;
        uint64_t beg = 0, end = 0;
        if (item < hi) {
            const uint2 it = b.items[item];
            HB_DBG_ASSERT(it.x < b.slots && it.y < b.rows_total);
            slot = it.x;
            const uint32_t self = b.slot_self[slot];
            beg = b.row_ptr[it.y];
            end = b.row_ptr[it.y + 1];
            for (uint64_t e = beg + l; e < end; e += kLkLanes) {
                const uint32_t s = b.src[e];
                if (s == kNone) continue;
                HB_DBG_ASSERT(s < b.rows_total);
                if (s < b.n_pad) ndeg += s != self ? 1u : 0u;
                else nchild++;
            }
        }
        uint32_t off = 0;
        if (nchild) off = atomicAdd(&s_children, nchild);
        if (ndeg) atomicAdd(&s_deg[g], ndeg);
        __syncthreads();
        if (threadIdx.x == 0 && s_children) s_base = atomicAdd(next_cnt, s_children);
        if (threadIdx.x < kLkItems && s_deg[threadIdx.x]) atomicAdd(&b.deg[b.items[it0 + threadIdx.x].x], s_deg[threadIdx.x]);
        __syncthreads();
        if (nchild) {
            uint64_t pos = next_base + s_base + off;
            for (uint64_t e = beg + l; e < end; e += kLkLanes) {
                const uint32_t s = b.src[e];
                if (s == kNone || s < b.n_pad) continue;
                if (pos < b.item_cap) b.items[pos] = make_uint2(slot, s);
                else b.flag[0] = 1;
                pos++;
            }
        }
    }
}

// per slot: does it select, and what keeps everything when it does not
__global__ __launch_bounds__(256) void lk_plan_kernel(const LkBatch b, uint32_t no_shortcut)
{
    const uint32_t slot = blockIdx.x * 256 + threadIdx.x;
    if (slot >= b.slots) return;
    const uint32_t d = b.deg[slot];
    const bool select = d > b.limit || (no_shortcut && d > 0);
    b.sel_k[slot] = select ? (d < b.limit ? d : b.limit) : 0u;
    b.sel_prefix[slot] = 0;
    b.thr[slot] = select ? 0u : kNone;
}

// one round of the select on digit `d` (3 = the most significant byte): the items [0, total) in contiguous ranges of per_block
__global__ __launch_bounds__(256) void lk_hist_kernel(const LkBatch b, uint64_t total, uint64_t per_block, int d)
{
    __shared__ uint32_t s_hist[256];
    const int g = threadIdx.x / kLkLanes, l = threadIdx.x % kLkLanes;
    s_hist[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t lo = (uint64_t)blockIdx.x * per_block, hi = lo + per_block < total ? lo + per_block : total;
    uint32_t cur = kNone; // the slot whose bins are in LDS (workgroup-uniform)
    for (uint64_t it0 = lo; it0 < hi; it0 += kLkItems) {
        const uint32_t first = b.items[it0].x;
        if (first != cur) {
            if (cur != kNone) {
                __syncthreads();
                const uint32_t v = s_hist[threadIdx.x];
                if (v) atomicAdd(&b.hist[(size_t)cur * 256 + threadIdx.x], v);
                s_hist[threadIdx.x] = 0;
                __syncthreads();
            }
            cur = first;
        }
        const uint64_t item = it0 + g;
        if (item >= hi) continue;
        const uint2 it = b.items[item];
        const uint32_t k = b.sel_k[it.x];
        if (!k) continue;
        const uint32_t self = b.slot_self[it.x], prefix = b.sel_prefix[it.x];
        const uint64_t end = b.row_ptr[it.y + 1];
        for (uint64_t e = b.row_ptr[it.y] + l; e < end; e += kLkLanes) {
            const uint32_t s = b.src[e];
            if (s >= b.n_pad || s == self) continue; // (kNone and the child rows are >= n_pad)
            const uint32_t v = lk_value(b.ord_row[s], b.mult);
            if (d < 3 && (v >> (8 * (d + 1))) != prefix) continue;
            const uint32_t dig = (v >> (8 * d)) & 255u;
            if (it.x == cur) atomicAdd(&s_hist[dig], 1u);
            else atomicAdd(&b.hist[(size_t)it.x * 256 + dig], 1u);
        }
    }
    __syncthreads();
    if (cur != kNone) {
        const uint32_t v = s_hist[threadIdx.x];
        if (v) atomicAdd(&b.hist[(size_t)cur * 256 + threadIdx.x], v);
    }
}

// the digit that holds the k-th entry of the slot, the k that remains inside it; the bins are cleared for the next round
__global__ __launch_bounds__(256) void lk_pick_kernel(const LkBatch b, int d)
{
    const uint32_t slot = blockIdx.x * 256 + threadIdx.x;
    if (slot >= b.slots) return;
    const uint32_t k = b.sel_k[slot];
    if (!k) return;
    uint32_t *h = b.hist + (size_t)slot * 256;
    uint32_t before = 0, dig = 255, rest = 1;
    bool found = false;
    for (uint32_t bin = 0; bin < 256; bin++) {
        const uint32_t c = h[bin];
        h[bin] = 0;
        if (!found && before + c >= k) {
            found = true;
            dig = bin;
            rest = k - before;
        }
        before += found ? 0u : c;
    }
    HB_DBG_ASSERT(found);
    const uint32_t prefix = (b.sel_prefix[slot] << 8) | dig;
    b.sel_prefix[slot] = prefix;
    b.sel_k[slot] = rest;
    if (d == 0) b.thr[slot] = prefix;
}

__global__ __launch_bounds__(256) void lk_emit_kernel(const LkBatch b, uint64_t total)
{
    const int g = threadIdx.x / kLkLanes, l = threadIdx.x % kLkLanes;
    const uint64_t stride = (uint64_t)gridDim.x * kLkItems;
    for (uint64_t item = (uint64_t)blockIdx.x * kLkItems + g; item < total; item += stride) {
        const uint2 it = b.items[item];
        const uint32_t self = b.slot_self[it.x], thr = b.thr[it.x];
        const uint64_t end = b.row_ptr[it.y + 1];
        for (uint64_t e = b.row_ptr[it.y] + l; e < end; e += kLkLanes) {
            const uint32_t s = b.src[e];
            if (s >= b.n_pad || s == self) continue;
            const uint32_t o = b.ord_row[s];
            if (lk_value(o, b.mult) <= thr) {
                const uint32_t pos = atomicAdd(&b.cursor[it.x], 1u);
                HB_DBG_ASSERT(pos < b.limit);
                if (pos < b.limit) b.out[(size_t)it.x * b.limit + pos] = o;
            }
        }
    }
}

// a workgroup per slot: its kept ords in ascending order -> (sid, key) at res_*[slot * limit + j]
__global__ __launch_bounds__(256) void lk_sort_kernel(const LkBatch b, const uint32_t *inv, const unsigned long long *key, uint64_t n, uint32_t *res_sid,
                                                      unsigned long long *res_key)
{
    __shared__ uint32_t s_v[kLkMaxLimit];
    const uint32_t slot = blockIdx.x;
    const uint32_t d = b.deg[slot], len = d < b.limit ? d : b.limit;
    uint32_t P = 2;
    while (P < len) P <<= 1;
    for (uint32_t i = threadIdx.x; i < P; i += 256) s_v[i] = i < len ? b.out[(size_t)slot * b.limit + i] : kNone;
    __syncthreads();
    if (len > 1) { // (workgroup-uniform)
        for (uint32_t k = 2; k <= P; k <<= 1)
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                for (uint32_t i = threadIdx.x; i < P; i += 256) {
                    const uint32_t x = i ^ j;
                    if (x > i) {
                        const uint32_t a = s_v[i], c = s_v[x];
                        if ((a > c) == ((i & k) == 0)) {
                            s_v[i] = c;
                            s_v[x] = a;
                        }
                    }
                }
                __syncthreads();
            }
    }
    for (uint32_t i = threadIdx.x; i < len; i += 256) {
        const uint32_t o = s_v[i];
        HB_DBG_ASSERT(o < n);
        const uint32_t sid = o < n ? inv[o] : kNone;
        res_sid[(size_t)slot * b.limit + i] = sid;
        res_key[(size_t)slot * b.limit + i] = sid < n ? key[sid] : ~0ull;
    }
}

// ---- forward links (hb_forwardlinks) --------------------------------------------------------------------------------------------------
// HostForwardlinksQuery::new(u).with_limit(EdgeLimit::Limit(L)) (webgraph/query/forwardlink.rs:183-330): the first L out-neighbours of
// each queried host in the same order.  The out-list of node row r is the reader list out_rows[out_ptr[r] .. out_ptr[r + 1]) of the
// plan's transpose.  A reader >= n_pad is a chunk row of some hub's tree: the edge's target is the node row at the top of that tree,
// top_row[chunk row - n_pad], a per-graph table built once per load from the highest virtual level down (fw_top_row_kernel).  The table
// exists because the alternative - climbing out_rows of the chunk row, level by level, per entry and per select round - costs up to
// `depth` dependent loads for every entry of a hub-bound edge, five times per call.
// An out-list has no length bound, so a slot's work is cut into SEGMENTS of kFwSegment entries and a workgroup takes one segment at a
// time: seg_base[slot] = the number of segments before the slot (an exclusive scan of ceil(length / kFwSegment) over the batch, slots + 1
// words), a workgroup finds the slot of segment g by bisection.  No list of pieces is stored: memory does not grow with the out-degrees.
//   count:  deg[slot] += the entries of the segment whose resolved target is not the slot's own row (summed in LDS, one atomic add).
//   select: the radix select of the backlinks (lk_plan_kernel, lk_pick_kernel) with fw_hist_kernel as its histogram: a segment belongs
//           to ONE slot, so the 256 bins live in LDS and are flushed once per segment.
//   emit:   as lk_emit_kernel, per segment; lk_sort_kernel orders and translates.  The cursor hands out positions in workgroup order, the
//           sort makes the list independent of it (ord is unique).
struct FwBatch {
    const uint64_t *out_ptr;   // rows_total + 1
    const uint32_t *out_rows;
    const uint32_t *top_row;   // nv
    const uint32_t *seg_base;  // slots + 1
    uint32_t segs;             // seg_base[slots]
};

constexpr uint32_t kFwSegment = 2048; // out-list entries of one segment (8 per lane)

// one virtual level [lo, hi), the highest first.  A chunk row with a list has exactly ONE reader - its hub's node row, or a chunk row
// of a higher level whose top is known already; a chunk row without a list (the padding that fills a level to whole tiles) has none
// and no top.  Anything else raises flag[0]: the caller refuses, it does not pick a reader.
__global__ __launch_bounds__(256) void fw_top_row_kernel(const uint64_t *row_ptr, const uint64_t *out_ptr, const uint32_t *out_rows, uint64_t n_pad, uint64_t rows_total,
                                                         uint64_t lo, uint64_t hi, uint32_t *top_row, uint32_t *flag)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t r = lo + (uint64_t)blockIdx.x * 256 + threadIdx.x; r < hi; r += stride) {
        const uint64_t readers = out_ptr[r + 1] - out_ptr[r], len = row_ptr[r + 1] - row_ptr[r];
        uint32_t top = kNone;
        if (readers == 1) {
            const uint32_t up = out_rows[out_ptr[r]];
            if (up < n_pad) top = up;
            else if (up >= hi && up < rows_total) top = top_row[up - n_pad]; // (a higher level: written by an earlier launch)
            if (top >= n_pad) flag[0] = 1;
        } else if (readers != 0 || len != 0) {
            flag[0] = 1;
        }
        top_row[r - n_pad] = top < n_pad ? top : kNone;
    }
}

// raw[slot] = the length of the slot's reader list (self link and chunk rows included: what the segments are cut from)
__global__ __launch_bounds__(256) void fw_len_kernel(const LkBatch b, const FwBatch f, uint32_t *raw)
{
    const uint32_t slot = blockIdx.x * 256 + threadIdx.x;
    if (slot >= b.slots) return;
    const uint32_t r = b.slot_row[slot];
    HB_DBG_ASSERT(r < b.n_pad);
    raw[slot] = (uint32_t)(f.out_ptr[r + 1] - f.out_ptr[r]);
}

struct FwPiece {
    uint32_t slot, self;
    uint64_t beg, end; // its entries of out_rows
};

// the slot that segment `seg` belongs to - the last one whose base is <= seg (empty slots in front of it share its base) - and its entries
__device__ __forceinline__ FwPiece fw_piece(const LkBatch &b, const FwBatch &f, uint32_t seg)
{
    uint32_t lo = 0, hi = b.slots; // seg_base[lo] <= seg < seg_base[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (f.seg_base[mid] <= seg) lo = mid;
        else hi = mid;
    }
    FwPiece p;
    p.slot = lo;
    p.self = b.slot_self[lo];
    const uint32_t r = b.slot_row[lo];
    const uint64_t all_end = f.out_ptr[r + 1];
    p.beg = f.out_ptr[r] + (uint64_t)(seg - f.seg_base[lo]) * kFwSegment;
    p.end = p.beg + kFwSegment < all_end ? p.beg + kFwSegment : all_end;
    HB_DBG_ASSERT(p.beg < all_end);
    return p;
}

// the node row an entry of a reader list stands for; kNone = none (cannot happen on a table that fw_top_row_kernel accepted)
__device__ __forceinline__ uint32_t fw_target(const LkBatch &b, const FwBatch &f, uint64_t e)
{
    const uint32_t t = f.out_rows[e];
    if (t < b.n_pad) return t;
    HB_DBG_ASSERT(t < b.rows_total);
    return t < b.rows_total ? f.top_row[t - b.n_pad] : kNone;
}

__global__ __launch_bounds__(256) void fw_count_kernel(const LkBatch b, const FwBatch f)
{
    __shared__ uint32_t s_cnt;
    for (uint32_t seg = blockIdx.x; seg < f.segs; seg += gridDim.x) { // workgroup-uniform
        if (threadIdx.x == 0) s_cnt = 0;
        __syncthreads();
        const FwPiece p = fw_piece(b, f, seg);
        uint32_t mine = 0;
        for (uint64_t e = p.beg + threadIdx.x; e < p.end; e += 256) {
            const uint32_t t = fw_target(b, f, e);
            mine += (t < b.n_pad && t != p.self) ? 1u : 0u;
        }
        if (mine) atomicAdd(&s_cnt, mine);
        __syncthreads();
        if (threadIdx.x == 0 && s_cnt) atomicAdd(&b.deg[p.slot], s_cnt);
        __syncthreads();
    }
}

// one round of the select on digit `d`, a segment at a time
__global__ __launch_bounds__(256) void fw_hist_kernel(const LkBatch b, const FwBatch f, int d)
{
    __shared__ uint32_t s_hist[256];
    s_hist[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t seg = blockIdx.x; seg < f.segs; seg += gridDim.x) { // workgroup-uniform
        const FwPiece p = fw_piece(b, f, seg);
        if (!b.sel_k[p.slot]) continue; // (uniform: one slot per segment)
        const uint32_t prefix = b.sel_prefix[p.slot];
        for (uint64_t e = p.beg + threadIdx.x; e < p.end; e += 256) {
            const uint32_t t = fw_target(b, f, e);
            if (t >= b.n_pad || t == p.self) continue;
            const uint32_t v = lk_value(b.ord_row[t], b.mult);
            if (d < 3 && (v >> (8 * (d + 1))) != prefix) continue;
            atomicAdd(&s_hist[(v >> (8 * d)) & 255u], 1u);
        }
        __syncthreads();
        const uint32_t v = s_hist[threadIdx.x];
        if (v) atomicAdd(&b.hist[(size_t)p.slot * 256 + threadIdx.x], v);
        s_hist[threadIdx.x] = 0;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void fw_emit_kernel(const LkBatch b, const FwBatch f)
{
    for (uint32_t seg = blockIdx.x; seg < f.segs; seg += gridDim.x) {
        const FwPiece p = fw_piece(b, f, seg);
        const uint32_t thr = b.thr[p.slot];
        for (uint64_t e = p.beg + threadIdx.x; e < p.end; e += 256) {
            const uint32_t t = fw_target(b, f, e);
            if (t >= b.n_pad || t == p.self) continue;
            const uint32_t o = b.ord_row[t];
            if (lk_value(o, b.mult) <= thr) {
                const uint32_t pos = atomicAdd(&b.cursor[p.slot], 1u);
                HB_DBG_ASSERT(pos < b.limit);
                if (pos < b.limit) b.out[(size_t)p.slot * b.limit + pos] = o;
            }
        }
    }
}

} // namespace hbk
