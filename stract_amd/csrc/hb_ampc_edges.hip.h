// hb_ampc_edges.hip.h - device code of the two edge steps of the AMPC shard (include/hb_ampc.h): CentralityMapper::update_counters
// (harmonic_centrality/mapper.rs:89-111) and ShortestPathMapper::update_distances (shortest_path/mapper.rs:64-86) over two resident
// tables.  The source table is only read, through its index and below its `committed`; the destination table has one writer per key
// group, as in every other upsert.  Included by hb_ampc.hip only; gfx950.  No floating point, no atomics on a value table.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hb_ampc.h"
#include "hb_ampc_values.hip.h"
#include "hb_regs.hip.h"
#include "hb_table.hip.h"

namespace hbe {
using hbt::kEmpty;
using hbt::u128;
using hbv::Side;

__device__ __forceinline__ u128 edge_key(const hb_u128 &v) { return ((u128)v.hi << 64) | (u128)v.lo; }

// ---- the counter job ---------------------------------------------------------------------------------------------------------
// Where the counter of pair i comes from: (table[slot[i]] or HyperLogLog::default()) with the register jp[i] merged in.  Nothing of it
// is stored per edge but the slot and the register: the 64 bytes are gathered when the pair is folded.
struct CounterSource {
    const uint4 *table;   // the source table's values (read only; never the table the batch writes)
    const uint32_t *slot; // per edge: slot of edge.from in the source table, kEmpty = absent (unwrap_or_default, mapper.rs:98)
    const uint16_t *jp;   // per edge: the register add_u128(edge.from) sets, index | value << 8 (hb_regs.hip.h)
};

// get_old_counters without the counters: the slot of every edge.from (slots >= committed do not count) and the register its add sets.
// Only the low 64 bits of the id are hashed (hyperloglog.rs:4398-4400); the table key is all 128.
__global__ __launch_bounds__(256) void counter_sources_kernel(const hb_u128 *from, uint32_t count, Side<uint4> prev, uint32_t *slot, uint16_t *jp)
{
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < count; i += gridDim.x * 256) {
        const hb_u128 f = from[i];
        slot[i] = hbv::side_find(prev, edge_key(f));
        jp[i] = hbk::initial_register_jp(f.lo);
    }
}

constexpr uint32_t kEdgesAhead = 8; // pairs of a group whose loads a quad issues before it folds the first of them

// upsert_kernel<0> of hb_ampc.hip with the pair's counter gathered from `src` instead of read from a staged array: one quad per key
// group, its pairs (positions perm[begin .. end) of the batch, batch order kept) applied in order to the stored counter; a fresh key
// (slot >= first_new) takes its first pair's counter verbatim.
__global__ __launch_bounds__(256) void upsert_edges_kernel(uint4 *table, const uint32_t *sorted_slot, const uint32_t *heads, const uint32_t *d_groups, uint32_t count,
                                                           uint32_t first_new, const uint32_t *perm, CounterSource src, uint8_t *actions)
{
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
        uint4 cur = make_uint4(0, 0, 0, 0);
        if (valid && !fresh) cur = table[(uint64_t)slot * 4 + q];
        // the ballot below needs every lane of the wave in the loop: iterate to the longest group of the wave
        uint32_t len = e - b, maxlen = len;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) maxlen = max(maxlen, (uint32_t)__shfl_xor((int)maxlen, off));
        // kEdgesAhead pairs per turn: position, source slot and register, then the source's counter are three loads that depend on
        // each other but not on the fold, so a turn has all of its pairs' chains in flight before it folds the first (a destination
        // with half of a batch's edges is one quad's serial walk: one pair per turn made it three memory round trips per pair)
        for (uint32_t i0 = 0; i0 < maxlen; i0 += kEdgesAhead) {
            uint32_t pos[kEdgesAhead], s[kEdgesAhead], jp[kEdgesAhead];
            uint4 v[kEdgesAhead];
#pragma unroll
            for (uint32_t u = 0; u < kEdgesAhead; u++) pos[u] = (valid && i0 + u < len) ? perm[b + i0 + u] : kEmpty;
#pragma unroll
            for (uint32_t u = 0; u < kEdgesAhead; u++) {
                s[u] = kEmpty;
                jp[u] = 0;
                if (pos[u] != kEmpty) {
                    s[u] = src.slot[pos[u]];
                    jp[u] = src.jp[pos[u]];
                }
            }
#pragma unroll
            for (uint32_t u = 0; u < kEdgesAhead; u++) { // the source's old counter, or the default
                v[u] = make_uint4(0, 0, 0, 0);
                if (s[u] != kEmpty) v[u] = src.table[(uint64_t)s[u] * 4 + q];
            }
#pragma unroll
            for (uint32_t u = 0; u < kEdgesAhead; u++) {
                const uint32_t i = i0 + u;
                if (i < maxlen) { // wave-uniform: the ballot below has every lane of the wave
                    const bool act = pos[u] != kEmpty;
                    hbk::Acc a; // the pair's counter: the old one with the source itself added
                    hbk::acc_zero(a);
                    hbk::acc_merge(a, v[u]);
                    hbk::acc_merge(a, hbk::counter_quarter_of_jp(jp[u], q));
                    const uint4 pair = hbk::acc_value(a);
                    const bool first = fresh && i == 0;
                    hbk::Acc acc;
                    hbk::acc_zero(acc);
                    hbk::acc_merge(acc, cur);
                    if (!first) hbk::acc_merge(acc, pair);
                    const uint4 merged = first ? pair : hbk::acc_value(acc);
                    const uint64_t bal = __ballot(act && hbk::u4_ne(merged, cur));
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

// ---- the distance job --------------------------------------------------------------------------------------------------------
// get_old_distances + the `+ 1`: has[i] = edge.from has a distance in prev (an edge without one is skipped, mapper.rs:70-72),
// cand[i] = that distance + 1, wrapping at 2^64 as HBU_OP_U64_ADD does.
__global__ __launch_bounds__(256) void distance_candidates_kernel(const hb_u128 *from, uint32_t count, Side<uint64_t> prev, uint64_t *cand, uint8_t *has)
{
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < count; i += gridDim.x * 256) {
        const uint32_t s = hbv::side_find(prev, edge_key(from[i]));
        cand[i] = s != kEmpty ? prev.values[s] + 1ull : 0ull;
        has[i] = s != kEmpty;
    }
}

// What one U64Min upsert of a destination's smallest candidate answers, from the actions of its candidates folded in batch order
// (group_apply_kernel<OpU64Min>): Inserted if the first one inserted the key, else Merged if any of them lowered the stored value,
// else NoChange.  Writes (key, action) of group g to out_keys[g] / out_actions[g].  A thread per group up to hbv::kWaveGroupLen
// pairs, a wave for a longer one (a hub destination), as in the fold itself.
__global__ __launch_bounds__(256) void group_actions_kernel(const uint32_t *heads, const uint32_t *d_groups, uint32_t count, const uint32_t *perm, const hb_u128 *keys,
                                                            const uint8_t *pair_actions, hb_u128 *out_keys, uint8_t *out_actions)
{
    const uint32_t groups = *d_groups;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t stride = gridDim.x * 256;
    for (uint32_t g0 = blockIdx.x * 256; g0 < groups; g0 += stride) { // block-uniform trip count: every lane of a wave stays in
        const uint32_t gidx = g0 + threadIdx.x;
        const bool valid = gidx < groups;
        uint32_t b = 0, len = 0;
        if (valid) {
            b = heads[gidx];
            len = (gidx + 1 < groups ? heads[gidx + 1] : count) - b;
        }
        if (valid && len <= hbv::kWaveGroupLen) {
            const uint32_t pos0 = perm[b];
            const uint8_t first = pair_actions[pos0];
            bool merged = first == HBU_MERGED;
            for (uint32_t i = 1; i < len; i++) merged |= pair_actions[perm[b + i]] == HBU_MERGED;
            out_keys[gidx] = keys[pos0];
            out_actions[gidx] = first == HBU_INSERTED ? HBU_INSERTED : (merged ? HBU_MERGED : HBU_NO_CHANGE);
        }
        uint64_t todo = __ballot(valid && len > hbv::kWaveGroupLen);
        while (todo) { // wave-uniform
            const int owner = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const uint32_t wb = __shfl(b, owner), wlen = __shfl(len, owner), wg = __shfl(gidx, owner);
            const uint32_t pos0 = perm[wb];
            const uint8_t first = pair_actions[pos0];
            bool merged = false;
            for (uint32_t c = 0; c < wlen; c += 64) { // wave-uniform trip count
                const uint32_t i = c + lane;
                const bool mine = i < wlen && pair_actions[perm[wb + i]] == HBU_MERGED;
                merged |= __ballot(mine) != 0ull;
            }
            if (lane == 0) {
                out_keys[wg] = keys[pos0];
                out_actions[wg] = first == HBU_INSERTED ? HBU_INSERTED : (merged ? HBU_MERGED : HBU_NO_CHANGE);
            }
        }
    }
}
} // namespace hbe
