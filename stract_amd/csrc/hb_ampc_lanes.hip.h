// hb_ampc_lanes.hip.h - device code of the 64-lane distance rows of the AMPC shard (include/hb_ampc.h: HBU_KIND_DIST64, HBU_OP_DIST64_MIN,
// hbu_round_lane_distances, hbu_fold_harmonic_lanes): RelaxEdges (shortest_path/mapper.rs:105-190) and the fold of the approximated harmonic
// centrality coordinator (approximated_harmonic_centrality/coordinator.rs:139-145) for up to 64 sampled sources in one walk over a worker's
// edges.  A row is 64 bytes, byte l = the distance from the batch's source l, HBU_DIST_NONE = none: the row of a HyperLogLog<64> counter
// with `max` turned into `min` and "set one register" into "+ 1 on every present byte", so the upsert is hbe::upsert_edges_kernel's walk (one
// quad per destination group, kEdgesAhead gathers in flight, pairs folded in batch order).  Included by hb_ampc.hip only; gfx950.  The source
// table is only read, through its index and below its `committed`; the destination table has one writer per key group.  Atomics: the key
// index's own and the counts - never on a value table.  No LDS, no scratch (every row index below is a compile-time constant).
// The fold needs the translation unit's -ffp-contract=off, as hb_ampc_fold.hip.h does.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hb_ampc.h"
#include "hb_ampc_edges.hip.h"
#include "hb_ampc_round.hip.h"
#include "hb_ampc_values.hip.h"
#include "hb_table.hip.h"

namespace hbl {
using hbt::kEmpty;
using hbt::Table;
using hbt::u128;
using hbv::Kahan;
using hbv::Side;

// ---- four lanes in a 32-bit word, sixteen in a quad's uint4 ----------------------------------------------------------------------------
__device__ __forceinline__ uint32_t min_u8x4(uint32_t a, uint32_t b)
{
    uint32_t r = 0;
#pragma unroll
    for (int s = 0; s < 32; s += 8) {
        const uint32_t x = (a >> s) & 0xFFu, y = (b >> s) & 0xFFu;
        r |= (x < y ? x : y) << s;
    }
    return r;
}
// the `+ 1` of update_distances on every lane that has a distance: 254 + 1 is HBU_DIST_NONE (no candidate), HBU_DIST_NONE stays
__device__ __forceinline__ uint32_t step_u8x4(uint32_t a)
{
    uint32_t r = 0;
#pragma unroll
    for (int s = 0; s < 32; s += 8) {
        const uint32_t x = (a >> s) & 0xFFu;
        r |= (x == HBU_DIST_NONE ? (uint32_t)HBU_DIST_NONE : x + 1u) << s;
    }
    return r;
}
__device__ __forceinline__ uint4 min_lanes(const uint4 &a, const uint4 &b) { return make_uint4(min_u8x4(a.x, b.x), min_u8x4(a.y, b.y), min_u8x4(a.z, b.z), min_u8x4(a.w, b.w)); }
__device__ __forceinline__ uint4 step_lanes(const uint4 &a) { return make_uint4(step_u8x4(a.x), step_u8x4(a.y), step_u8x4(a.z), step_u8x4(a.w)); }
__device__ __forceinline__ bool lanes_ne(const uint4 &a, const uint4 &b) { return a.x != b.x || a.y != b.y || a.z != b.z || a.w != b.w; }
__device__ __forceinline__ uint4 no_lanes() { return make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu); }

// Where the row of pair i comes from in the round step: prev[slot[i]] with the `+ 1`.  Per edge only the slot is kept (as
// hbe::CounterSource does); the 64 bytes are gathered when the pair is folded.
struct LaneSource {
    const uint4 *table;   // the source table's rows (read only; never the table the batch writes)
    const uint32_t *slot; // per selected edge: the slot of edge.from in the source table (a selected edge's source has one)
};

// HBU_OP_DIST64_MIN over a batch: one quad per key group, its pairs (positions perm[begin .. end) of the batch, batch order kept) applied
// in order to the stored row; a fresh key (slot >= first_new) takes its first pair's row verbatim, all-HBU_DIST_NONE included.  GATHER:
// the pair's row is step_lanes(src.table[src.slot[pos]]) (the round step), else values[pos] (hbu_batch_upsert_values).  The walk is
// hbe::upsert_edges_kernel's: hbe::kEdgesAhead pairs of a group have their position -> slot -> row chains in flight before the first is
// folded, because a hub destination is one quad's serial walk here as there.
template <bool GATHER>
__global__ __launch_bounds__(256) void upsert_lanes_kernel(uint4 *table, const uint32_t *sorted_slot, const uint32_t *heads, const uint32_t *d_groups, uint32_t count,
                                                           uint32_t first_new, const uint32_t *perm, const uint4 *values, LaneSource src, uint8_t *actions)
{
    constexpr uint32_t kAhead = hbe::kEdgesAhead;
    const uint32_t groups = *d_groups;
    const int q = (int)(threadIdx.x & 3), qshift = (int)((threadIdx.x & 63) & ~3);
    const uint32_t stride = gridDim.x * 64;
    for (uint32_t g0 = blockIdx.x * 64; g0 < groups; g0 += stride) { // block-uniform trip count; every lane of a wave stays in
        const uint32_t gidx = g0 + (threadIdx.x >> 2);
        const bool valid = gidx < groups;
        uint32_t b = 0, e = 0, slot = 0;
        bool fresh = false;
        if (valid) {
            b = heads[gidx];
            e = gidx + 1 < groups ? heads[gidx + 1] : count;
            slot = sorted_slot[b];
            fresh = slot >= first_new;
        }
        uint4 cur = no_lanes();
        if (valid && !fresh) cur = table[(uint64_t)slot * 4 + q];
        // the ballot below needs every lane of the wave in the loop: iterate to the longest group of the wave
        uint32_t len = e - b, maxlen = len;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) maxlen = max(maxlen, (uint32_t)__shfl_xor((int)maxlen, off));
        for (uint32_t i0 = 0; i0 < maxlen; i0 += kAhead) {
            uint32_t pos[kAhead], s[kAhead];
            uint4 v[kAhead];
#pragma unroll
            for (uint32_t u = 0; u < kAhead; u++) pos[u] = (valid && i0 + u < len) ? perm[b + i0 + u] : kEmpty;
            if (GATHER) {
#pragma unroll
                for (uint32_t u = 0; u < kAhead; u++) {
                    s[u] = kEmpty;
                    if (pos[u] != kEmpty) s[u] = src.slot[pos[u]];
                }
            }
#pragma unroll
            for (uint32_t u = 0; u < kAhead; u++) {
                v[u] = no_lanes();
                if (GATHER) {
                    if (s[u] != kEmpty) v[u] = step_lanes(src.table[(uint64_t)s[u] * 4 + q]);
                } else {
                    if (pos[u] != kEmpty) v[u] = values[(uint64_t)pos[u] * 4 + q];
                }
            }
#pragma unroll
            for (uint32_t u = 0; u < kAhead; u++) {
                const uint32_t i = i0 + u;
                if (i < maxlen) { // wave-uniform: the ballot below has every lane of the wave
                    const bool act = pos[u] != kEmpty;
                    const bool first = fresh && i == 0;
                    const uint4 merged = first ? v[u] : min_lanes(cur, v[u]);
                    const uint64_t bal = __ballot(act && lanes_ne(merged, cur));
                    const bool changed = ((bal >> qshift) & 0xFull) != 0;
                    if (act) {
                        if (q == 0) actions[pos[u]] = first ? HBU_INSERTED : (changed ? HBU_MERGED : HBU_NO_CHANGE);
                        cur = merged;
                    }
                }
            }
        }
        if (valid) table[(uint64_t)slot * 4 + q] = cur;
    }
}

// batch_get of lane rows: an absent key reads as 64 x HBU_DIST_NONE ("no distance", not zero, is this kind's default)
__global__ __launch_bounds__(256) void get_lanes_kernel(const uint4 *table, const uint32_t *slots, uint32_t count, uint4 *out)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    const uint32_t i = t >> 2;
    if (i >= count) return;
    const uint32_t s = slots[i];
    out[t] = s == kEmpty ? no_lanes() : table[(uint64_t)s * 4 + (t & 3)];
}

// relax_*_edges' filter (shortest_path/mapper.rs:121,167) for lane rows, as hbr::select_distance_edges_kernel: flag = `changed` contains
// the source AND the source has a row in prev (an edge without one is skipped, mapper.rs:70-72); slot = that row's.
__global__ __launch_bounds__(256) void select_lane_edges_kernel(const hb_u128 *from, uint32_t count, hbr::Filter changed, Side<uint4> prev, uint8_t *flag, uint32_t *slot)
{
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < count; i += gridDim.x * 256) {
        const hb_u128 f = from[i];
        uint32_t s = kEmpty;
        if (hbr::filter_contains(changed, f)) s = hbv::side_find(prev, hbr::id_key(f));
        flag[i] = s != kEmpty ? 1 : 0;
        slot[i] = s;
    }
}

// One addend of the fold: KahanSum::from(v) written if the key is new to the table and this is its first lane, else AddAssign<KahanSum>
// as written (kahan_sum.rs:65-72), every operation rounded on its own.
__device__ __forceinline__ void fold_term(Kahan &k, bool &write, double v)
{
    if (write) {
        k.sum = v;
        k.err = 0.0;
        write = false;
    } else {
        const double y = (v + 0.0) - k.err; // rhs.sum + rhs.err of a KahanSum::from(v)
        const double t = k.sum + y;
        k.err = (t - k.sum) - y;
        k.sum = t;
    }
}

// hbf::fold_distances_kernel for lane rows: one thread per slot of the LANE table's key index.  Whether the row has a lane to fold (below
// n_lanes, not HBU_DIST_NONE, not a skipped zero) is decided BEFORE the key finds or claims its entry in `dst`: a key without one is not
// inserted.  The lanes are folded in ascending order - the order of the sources, which is a node's summation order and therefore its bits.
// An entry number at or above dst_committed is a key this launch inserted: its first addend is WRITTEN and the row is never read.
// counts[0] += the lanes folded, counts[1] += the keys inserted.
__global__ __launch_bounds__(256) void fold_lanes_kernel(const u128 *src_keys, const uint32_t *src_pids, uint64_t src_slots, uint32_t src_committed, const uint4 *rows,
                                                         uint32_t n_lanes, Table dst, uint32_t dst_committed, Kahan *centralities, double norm, uint32_t flags,
                                                         unsigned long long *counts)
{
    unsigned long long folded = 0, inserted = 0;
    const bool skip_zero = (flags & HBU_FOLD_SKIP_ZERO) != 0;
    const uint64_t below = n_lanes >= HBU_DIST_LANES ? ~0ull : (1ull << n_lanes) - 1ull; // the lanes below n_lanes
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < src_slots; i += (uint64_t)gridDim.x * 256) {
        const uint32_t p = src_pids[i];
        if (p < src_committed) {
            uint32_t w[16];
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const uint4 r = rows[(uint64_t)p * 4 + c];
                w[c * 4 + 0] = r.x;
                w[c * 4 + 1] = r.y;
                w[c * 4 + 2] = r.z;
                w[c * 4 + 3] = r.w;
            }
            uint64_t todo = 0; // bit l: lane l is folded
#pragma unroll
            for (uint32_t l = 0; l < HBU_DIST_LANES; l++) {
                const uint32_t d = (w[l >> 2] >> ((l & 3u) * 8u)) & 0xFFu;
                todo |= (uint64_t)(d != HBU_DIST_NONE && !(d == 0 && skip_zero)) << l;
            }
            todo &= below;
            if (todo) {
                const uint32_t s = hbt::table_get(dst, src_keys[i], kEmpty);
                bool write = s >= dst_committed;
                Kahan k;
                k.sum = 0.0;
                k.err = 0.0;
                if (write) inserted++;
                else k = centralities[s];
#pragma unroll
                for (uint32_t l = 0; l < HBU_DIST_LANES; l++) {
                    if ((todo >> l) & 1ull) {
                        const uint32_t d = (w[l >> 2] >> ((l & 3u) * 8u)) & 0xFFu;
                        fold_term(k, write, (1.0 / (double)d) * norm); // d == 0: inf, as the reference's `1.0 / distance as f64`
                    }
                }
                folded += (unsigned long long)__popcll(todo);
                centralities[s] = k;
            }
        }
    }
    hbr::wave_add(&counts[0], folded);
    hbr::wave_add(&counts[1], inserted);
}
} // namespace hbl
