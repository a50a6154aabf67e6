// hb_bfs.hip.h - device code of hb_distances (ShortestPaths, crates/core/src/webgraph/shortest_path.rs:26-227): one exact multi-source
// BFS over the HyperBall device plan, forward or reversed.  Part of the hb_api.hip translation unit (included after hb_sample.hip.h;
// uses the plan layout, the quad helpers of hb_regs.hip.h and touch_set of hb_sweep.hip.h).  Driver: hb_api_distance.inc.
//
// State: dist[] one byte per device row (255 = unreached), and one-bit-per-row bitmaps: `vis` over all work rows, `front` over the node
// rows (the nodes first reached at the previous level), `next` over all work rows (this level's candidates; all-zero between levels).
// A level is "push" (top-down: the frontier marks its neighbours in `next`) or "pull" (bottom-up: every unvisited node row scans its
// neighbours for a visited one), then one finalize pass over the node words: new = next & ~vis, dist = level, vis |= new, front = new.
// The two adjacencies are the plan's own: forward pushes along out_ptr / out_rows (a row's readers) and pulls along row_ptr / src;
// reversed swaps them.  Hub rows are chunk trees, so an edge u -> hub runs through virtual rows:
//   push: a marked virtual row relays to ITS neighbours inside the level, one launch per virtual level (ascending forward, descending
//         reversed), the way the sweep passes expand touches;
//   pull: vis of a virtual row = "a visited node feeds this chunk" (forward) / "the hub this chunk belongs to is visited" (reversed),
//         recomputed level by level before the node rows look at it.  A row that is unvisited after level d - 1 has no neighbour
//         visited before d - 1, so "a neighbour is visited" and "a neighbour is in the frontier" are the same test at level d: the
//         virtual bits only ever go from 0 to 1, a set one is never scanned again, and a push level keeps them right by setting the bit
//         of every virtual row it relays through.
// Exactness: by induction over the levels `front` is exactly the set of nodes at distance d - 1 and `vis` the set at distance < d;
// both kinds of level add exactly the unvisited rows with an edge from (to, reversed) `front`.
#pragma once

namespace hbk {

constexpr uint32_t kDistUnreached = 255u; // HB_DIST_UNREACHED
constexpr uint64_t kBfsHeavy = 4096;      // push: a longer neighbour list goes to the grid-wide kernel
constexpr uint64_t kBfsWaveList = 8;      // push: a longer neighbour list is walked by the whole wave, a shorter one by its lane
constexpr uint64_t kBfsLongPull = 256;    // pull: a longer neighbour list is scanned by the whole wave, a shorter one by its quad

struct BfsParams {
    const uint64_t *push_ptr; // rows_total + 1
    const uint32_t *push_idx;
    const uint64_t *pull_ptr; // rows_total + 1
    const uint32_t *pull_idx;
    const uint32_t *deg;      // per node row: out-degree (forward) / in-degree (reversed): the switch rule's edge counts
    uint8_t *dist;            // n_pad
    uint32_t *vis;            // rows_total bits
    uint32_t *front;          // n_pad bits
    uint32_t *next;           // rows_total bits
    uint32_t *heavy;          // node rows whose neighbour list the grid expands together
    unsigned int *heavy_cnt;
    uint32_t heavy_cap;       // 0 = no deferral in this launch
    unsigned long long *cnt;  // this level: [0] nodes first reached, [1] their degree sum, [2] neighbour entries read
    uint64_t n_pad, rows_total;
    uint64_t row_lo, row_hi;  // rows of this launch (multiples of 32)
    uint32_t level;
};

__device__ __forceinline__ bool bfs_bit(const uint32_t *bits, uint32_t r) { return (bits[r >> 5] >> (r & 31u)) & 1u; }

// push: row r is a neighbour of a frontier / relaying row.  Visited rows are dropped here (their vis words do not change while a
// push launch that could mark them runs); the rest become candidates.
__device__ __forceinline__ void bfs_mark(const BfsParams &p, uint32_t r)
{
    if (r == kNone) return;
    HB_DBG_ASSERT(r < p.rows_total);
    if (bfs_bit(p.vis, r)) return;
    touch_set(p.next, r, p.rows_total);
}

// Level 0: the sources (distinct sids).  One thread each.
__global__ __launch_bounds__(256) void bfs_seed_kernel(const uint32_t *sids, uint32_t count, const uint32_t *dev_of, const BfsParams p)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    unsigned long long one = 0, dg = 0;
    if (i < count) {
        const uint32_t row = dev_of[sids[i]];
        HB_DBG_ASSERT(row < p.n_pad);
        p.dist[row] = 0; // (one writer per row: the sources are distinct)
        atomicOr(&p.vis[row >> 5], 1u << (row & 31u));
        atomicOr(&p.front[row >> 5], 1u << (row & 31u));
        one = 1;
        dg = p.deg[row];
    }
    wave_add_counters(p.cnt, one, dg, 0ull);
}

// One push launch over the rows [row_lo, row_hi): VIRT = false: the node rows of `front`; VIRT = true: one virtual level - the rows
// marked in `next` (consumed: the words are zero again afterwards) that have not relayed before.  A lane takes one bitmap word; the
// short neighbour lists of its rows it walks itself, the longer ones the whole wave walks, the heavy ones go to bfs_push_heavy_kernel.
template <bool VIRT>
__global__ __launch_bounds__(256) void bfs_push_kernel(const BfsParams p)
{
    const int lane = threadIdx.x & 63;
    const uint64_t w_lo = p.row_lo >> 5, w_hi = (p.row_hi + 31) >> 5;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    unsigned long long insp = 0;
    for (uint64_t w0 = w_lo + (uint64_t)blockIdx.x * 256; w0 < w_hi; w0 += stride) { // wave-uniform trip count
        const uint64_t w = w0 + threadIdx.x;
        uint32_t act = 0;
        if (w < w_hi) {
            if (VIRT) { // this lane owns the word: nobody marks rows of this virtual level while the launch runs
                const uint32_t t = p.next[w];
                if (t) {
                    p.next[w] = 0;
                    const uint32_t v = p.vis[w];
                    act = t & ~v;
                    if (act) p.vis[w] = v | act;
                }
            } else {
                act = p.front[w];
            }
        }
        if (!__ballot(act != 0)) continue;
        uint32_t lng = 0; // this lane's rows with longer lists
        while (act) {
            const int b = __ffs((int)act) - 1;
            act &= act - 1;
            const uint64_t u = (w << 5) + (uint64_t)b;
            HB_DBG_ASSERT(u < p.rows_total);
            const uint64_t kb = p.push_ptr[u], ke = p.push_ptr[u + 1];
            if (ke - kb > kBfsWaveList) {
                lng |= 1u << b;
            } else {
                for (uint64_t k = kb; k < ke; k++) bfs_mark(p, p.push_idx[k]);
                insp += ke - kb;
            }
        }
        uint64_t owners;
        while ((owners = __ballot(lng != 0)) != 0) {
            const int src = __ffsll((long long)owners) - 1;
            const uint32_t m = __shfl(lng, src);
            const int b = __ffs((int)m) - 1;
            if (lane == src) lng &= lng - 1;
            const uint64_t u = ((w0 + (uint64_t)(threadIdx.x & ~63) + (uint64_t)src) << 5) + (uint64_t)b;
            const uint64_t kb = p.push_ptr[u], ke = p.push_ptr[u + 1];
            if (p.heavy_cap && ke - kb > kBfsHeavy) {
                if (lane == 0) {
                    const unsigned int pos = atomicAdd(p.heavy_cnt, 1u);
                    HB_DBG_ASSERT(pos < p.heavy_cap);
                    if (pos < p.heavy_cap) p.heavy[pos] = (uint32_t)u;
                }
                continue;
            }
            for (uint64_t k = kb + lane; k < ke; k += 64) bfs_mark(p, p.push_idx[k]);
            if (lane == 0) insp += ke - kb;
        }
    }
    wave_add_counters(p.cnt, 0ull, 0ull, insp);
}

// the heavy rows of a push level, each expanded by the whole grid
__global__ __launch_bounds__(256) void bfs_push_heavy_kernel(const BfsParams p)
{
    const unsigned int have = *p.heavy_cnt;
    const uint32_t nheavy = have < p.heavy_cap ? have : p.heavy_cap;
    const uint64_t wbase = ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64, nthreads = (uint64_t)gridDim.x * 256;
    const int lane = threadIdx.x & 63;
    unsigned long long insp = 0;
    for (uint32_t i = 0; i < nheavy; i++) {
        const uint32_t u = p.heavy[i];
        HB_DBG_ASSERT(u < p.rows_total);
        const uint64_t b = p.push_ptr[u], e = p.push_ptr[u + 1];
        for (uint64_t k0 = b + wbase; k0 < e; k0 += nthreads) { // wave-uniform trip count
            const uint64_t k = k0 + lane;
            if (k < e) {
                bfs_mark(p, p.push_idx[k]);
                insp++;
            }
        }
    }
    wave_add_counters(p.cnt, 0ull, 0ull, insp);
}

// One pull launch over the rows [row_lo, row_hi): a wave owns one 32-row word per iteration (two rounds of 16 rows, a quad per row).
// Every row of the word whose vis bit is clear scans its neighbour list for a row with a set vis bit; a lane stops at its first hit.
//   VIRT:  the word's new bits go straight into vis (the rows it reads belong to other levels, already final for this level);
//   !VIRT: the hits become the word of `next` (vis must stay the level d - 1 picture while other waves still read it).
// Lists longer than kBfsLongPull (reversed: a node with very many out-links; a forward list is a chunk, never that long) are left to
// the whole wave, 64 entries per step, which stops at the first step with a hit.
template <bool VIRT>
__global__ __launch_bounds__(256) void bfs_pull_kernel(const BfsParams p)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 2, q = lane & 3;
    const uint64_t w_lo = p.row_lo >> 5, nwords = (p.row_hi - p.row_lo + 31) >> 5;
    const uint64_t wid = (uint64_t)blockIdx.x * 4 + wave, wstride = (uint64_t)gridDim.x * 4;
    unsigned long long insp = 0;
    for (uint64_t wi = wid; wi < nwords; wi += wstride) { // wave-uniform trip count
        const uint64_t w = w_lo + wi;
        const uint32_t visw = p.vis[w];
        const uint64_t left = p.row_hi - (w << 5);
        const uint32_t inrange = left >= 32 ? 0xFFFFFFFFu : ((1u << left) - 1u);
        const uint32_t todo = ~visw & inrange;
        if (!todo) continue;
        uint32_t found = 0, longm = 0;
        for (int h = 0; h < 2; h++) {
            const uint32_t bit = (uint32_t)(h * 16 + g);
            const uint64_t row = (w << 5) + bit;
            const bool active = (todo >> bit) & 1u;
            uint64_t beg = 0, end = 0;
            if (active) {
                beg = p.pull_ptr[row];
                end = p.pull_ptr[row + 1];
            }
            const bool is_long = end - beg > kBfsLongPull;
            bool hit = false;
            if (!is_long) {
                for (uint64_t e = beg + q; e < end && !hit; e += 4) {
                    const uint32_t r = p.pull_idx[e];
                    insp++;
                    if (r != kNone) {
                        HB_DBG_ASSERT(r < p.rows_total);
                        hit = bfs_bit(p.vis, r);
                    }
                }
            }
            found |= pack16(__ballot(hit)) << (16 * h);
            longm |= pack16(__ballot(is_long)) << (16 * h);
        }
        while (longm) { // wave-uniform
            const int b = __ffs((int)longm) - 1;
            longm &= longm - 1;
            const uint64_t row = (w << 5) + (uint64_t)b;
            const uint64_t kb = p.pull_ptr[row], ke = p.pull_ptr[row + 1];
            for (uint64_t k0 = kb; k0 < ke; k0 += 64) {
                const uint64_t k = k0 + lane;
                bool hit = false;
                if (k < ke) {
                    const uint32_t r = p.pull_idx[k];
                    insp++;
                    if (r != kNone) {
                        HB_DBG_ASSERT(r < p.rows_total);
                        hit = bfs_bit(p.vis, r);
                    }
                }
                if (__ballot(hit)) {
                    found |= 1u << b;
                    break;
                }
            }
        }
        if (lane == 0 && found) {
            if (VIRT) p.vis[w] = visw | found;
            else p.next[w] = found; // (the node words of `next` are zero between levels, and a pull level has no other writer)
        }
    }
    wave_add_counters(p.cnt, 0ull, 0ull, insp);
}

// The end of every level, a lane per node word: the candidates that were not visited yet are the nodes at distance `level`.
// The distance bytes are ordinary stores with ONE writer each (the lane that owns the row's word, at the one level that reaches the
// row), so no two stores to a byte ever race.  Also leaves `next` zero and the heavy list empty for the next level.
__global__ __launch_bounds__(256) void bfs_finalize_kernel(const BfsParams p)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) *p.heavy_cnt = 0u;
    const uint64_t words = p.n_pad >> 5;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    unsigned long long c_new = 0, c_deg = 0;
    for (uint64_t w0 = (uint64_t)blockIdx.x * 256; w0 < words; w0 += stride) { // wave-uniform trip count
        const uint64_t w = w0 + threadIdx.x;
        if (w >= words) continue;
        const uint32_t cand = p.next[w];
        const uint32_t oldf = p.front[w];
        if (!cand && !oldf) continue;
        uint32_t nw = 0;
        if (cand) {
            p.next[w] = 0;
            const uint32_t v = p.vis[w];
            nw = cand & ~v;
            if (nw) p.vis[w] = v | nw;
        }
        p.front[w] = nw;
        while (nw) {
            const int b = __ffs((int)nw) - 1;
            nw &= nw - 1;
            const uint64_t row = (w << 5) + (uint64_t)b;
            p.dist[row] = (uint8_t)p.level;
            c_new++;
            c_deg += p.deg[row];
        }
    }
    wave_add_counters(p.cnt, c_new, c_deg, 0ull);
}

// in-degree per device row through the chunk trees (once per loaded graph; the reversed switch rule's edge counts): entries[row] =
// the node sources under the row.  One launch per virtual level, ascending, then the node rows; a thread per row (<= chunk entries).
__global__ __launch_bounds__(256) void bfs_indegree_kernel(const uint64_t *row_ptr, const uint32_t *src, uint32_t *entries, uint64_t n_pad, uint64_t rows_total,
                                                           uint64_t row_lo, uint64_t row_hi)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t row = row_lo + (uint64_t)blockIdx.x * 256 + threadIdx.x; row < row_hi; row += stride) {
        uint64_t sum = 0;
        for (uint64_t e = row_ptr[row]; e < row_ptr[row + 1]; e++) {
            const uint32_t s = src[e];
            if (s == kNone) continue;
            HB_DBG_ASSERT(s < rows_total);
            sum += s < n_pad ? 1u : entries[s];
        }
        entries[row] = sum > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)sum;
    }
    (void)rows_total;
}

// result extraction, step 1: the distance bytes in ascending-NodeID (sid) order; step 2 is a rocPRIM select (hb_plan.hip)
__global__ __launch_bounds__(256) void bfs_by_sid_kernel(const uint8_t *dist, const uint32_t *dev_of, uint64_t n, uint64_t n_pad, uint8_t *out)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s < n; s += stride) {
        const uint32_t row = dev_of[s];
        HB_DBG_ASSERT(row < n_pad);
        out[s] = dist[row];
    }
    (void)n_pad;
}

} // namespace hbk
