// hb_ampc_round.hip.h - device code of the resident worker graph and the resident changed-node filter of the AMPC shard
// (include/hb_ampc.h): the filter kernels (U64BloomFilter, crates/bloom/src/lib.rs:60-130; the Exact arm of UpdatedNodes,
// shortest_path/updated_nodes.rs:27-44, as a set of whole ids in the key index of hb_table.hip.h), the selection kernels of the mapper steps
// (map_cardinalities, harmonic_centrality/mapper.rs:253-296; relax_all_edges / relax_exact_edges, shortest_path/mapper.rs:105-190;
// map_centralities, mapper.rs:298-333) and the kernel that turns a batch's actions into the next round's filter (update_changed_nodes,
// mapper.rs:114-125; map_batch, shortest_path/mapper.rs:88-103).  Included by hb_ampc.hip only; gfx950.  Atomics: OR into a filter's
// words, the key index's own, and the counts - never on a value table.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hb_ampc.h"
#include "hb_ampc_values.hip.h"
#include "hb_bloom.hip.h"
#include "hb_regs.hip.h"
#include "hb_table.hip.h"

namespace hbr {
using hbt::kEmpty;
using hbt::Table;
using hbt::u128;
using hbv::Side;

constexpr uint32_t kNoFilter = 0xFFFFFFFFu;

__device__ __forceinline__ u128 id_key(const hb_u128 &v) { return ((u128)v.hi << 64) | (u128)v.lo; }

// A filter as the kernels see it.  Bloom: bit i of the bit vector is bit i % 32 of 32-bit word i / 32 (= bit i % 64 of little-endian
// 64-bit word i / 64, the bit vector's own data words).  Exact: an id is a member iff the index holds it below `committed`.
struct Filter {
    uint32_t kind;     // HBU_FILTER_BLOOM, HBU_FILTER_EXACT or kNoFilter (a sink that takes nothing)
    uint32_t num_bits; // bloom: 1 .. 2^32 - 1
    uint32_t *bits;    // bloom
    Table index;       // exact
    uint32_t committed;
};

__device__ __forceinline__ bool filter_contains(const Filter &f, const hb_u128 &id)
{
    if (f.kind == HBU_FILTER_BLOOM) {
        const uint64_t s = hbk::bloom_slot(id.lo, f.num_bits);
        return (f.bits[s >> 5] >> (s & 31u)) & 1u;
    }
    return hbt::table_find(f.index, id_key(id)) < f.committed; // (kEmpty is above every count)
}
// Bloom: one OR.  Exact: the id finds or claims its entry; the index has room for every id the launch can bring (the host grows it first).
__device__ __forceinline__ void filter_insert(const Filter &f, const hb_u128 &id)
{
    if (f.kind == HBU_FILTER_BLOOM) {
        const uint64_t s = hbk::bloom_slot(id.lo, f.num_bits);
        atomicOr(&f.bits[s >> 5], 1u << (s & 31u));
    } else {
        (void)hbt::table_get(f.index, id_key(id), kEmpty);
    }
}

// the wave's sum of c reaches *out with one atomic (every lane of the wave calls it)
__device__ __forceinline__ void wave_add(unsigned long long *out, unsigned long long c)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
}

// ---- the filter's own calls ------------------------------------------------------------------------------------------------------
// fill(): every bit below num_bits; the tail bits of the last 64-bit word stay zero.  words = 32-bit words of the allocation.
__global__ __launch_bounds__(256) void bloom_fill_kernel(uint32_t *bits, uint64_t words, uint64_t num_bits)
{
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (uint64_t)gridDim.x * 256) {
        const uint64_t first = w * 32;
        uint32_t v = 0;
        if (first + 32 <= num_bits) v = 0xFFFFFFFFu;
        else if (first < num_bits) v = (1u << (uint32_t)(num_bits - first)) - 1u;
        bits[w] = v;
    }
}
// union: a word-wise OR
__global__ __launch_bounds__(256) void bloom_or_kernel(uint32_t *dst, const uint32_t *src, uint64_t words)
{
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (uint64_t)gridDim.x * 256) dst[w] |= src[w];
}
// count_ones()
__global__ __launch_bounds__(256) void bloom_popcount_kernel(const uint32_t *bits, uint64_t words, unsigned long long *out)
{
    unsigned long long c = 0;
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (uint64_t)gridDim.x * 256) c += (unsigned)__popc(bits[w]);
    wave_add(out, c);
}
__global__ __launch_bounds__(256) void filter_insert_kernel(const hb_u128 *ids, uint32_t count, Filter f)
{
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < count; i += gridDim.x * 256) filter_insert(f, ids[i]);
}
__global__ __launch_bounds__(256) void filter_contains_kernel(const hb_u128 *ids, uint32_t count, Filter f, uint8_t *out)
{
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < count; i += gridDim.x * 256) out[i] = filter_contains(f, ids[i]) ? 1 : 0;
}
// exact set: every member of `src` (entries below src_committed) into the index `dst`
__global__ __launch_bounds__(256) void set_union_kernel(const u128 *src_keys, const uint32_t *src_pids, uint64_t src_slots, uint32_t src_committed, Table dst)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < src_slots; i += (uint64_t)gridDim.x * 256)
        if (src_pids[i] < src_committed) (void)hbt::table_get(dst, src_keys[i], kEmpty);
}
// exact set: the members, each at the position its entry number gives (entry numbers below `committed` are dense)
__global__ __launch_bounds__(256) void set_export_kernel(const u128 *keys, const uint32_t *pids, uint64_t slots, uint32_t committed, hb_u128 *out)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < slots; i += (uint64_t)gridDim.x * 256) {
        const uint32_t p = pids[i];
        if (p < committed) {
            hb_u128 v;
            v.lo = (uint64_t)keys[i];
            v.hi = (uint64_t)(keys[i] >> 64);
            out[p] = v;
        }
    }
}

// ---- the selection kernels: one thread per edge or node of the chunk -------------------------------------------------------------
// map_cardinalities' filter (mapper.rs:273) and, for the selected edges, what hbe::counter_sources_kernel writes: the source's slot in
// prev and the register its add sets - the source id is read once.
__global__ __launch_bounds__(256) void select_counter_edges_kernel(const hb_u128 *from, uint32_t count, Filter changed, Side<uint4> prev, uint8_t *flag,
                                                                   uint32_t *slot, uint16_t *jp)
{
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < count; i += gridDim.x * 256) {
        const hb_u128 f = from[i];
        const bool sel = filter_contains(changed, f);
        flag[i] = sel ? 1 : 0;
        slot[i] = sel ? hbv::side_find(prev, id_key(f)) : kEmpty;
        jp[i] = sel ? hbk::initial_register_jp(f.lo) : (uint16_t)0;
    }
}
// relax_*_edges' filter (shortest_path/mapper.rs:121,167) and what hbe::distance_candidates_kernel writes: flag = selected AND the source
// has a distance (mapper.rs:73), cand = that distance + 1 (wrapping).  *selected counts the edges the filter passes, with or without one.
__global__ __launch_bounds__(256) void select_distance_edges_kernel(const hb_u128 *from, uint32_t count, Filter changed, Side<uint64_t> prev, uint8_t *flag,
                                                                    uint64_t *cand, unsigned long long *selected)
{
    unsigned long long mine = 0;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < count; i += gridDim.x * 256) {
        const hb_u128 f = from[i];
        const bool sel = filter_contains(changed, f);
        uint32_t s = kEmpty;
        if (sel) s = hbv::side_find(prev, id_key(f));
        mine += sel ? 1u : 0u;
        flag[i] = s != kEmpty ? 1 : 0;
        cand[i] = s != kEmpty ? prev.values[s] + 1ull : 0ull;
    }
    wave_add(selected, mine);
}
// map_centralities' filter (mapper.rs:318)
__global__ __launch_bounds__(256) void select_nodes_kernel(const hb_u128 *nodes, uint32_t count, Filter changed, uint8_t *flag)
{
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < count; i += gridDim.x * 256) flag[i] = filter_contains(changed, nodes[i]) ? 1 : 0;
}

// ---- actions -> the next round's filter ------------------------------------------------------------------------------------------
// One entry per pair (the counter step) or per destination (the distance step): counts[a] += the entries with action a, and the key of
// every entry whose action is in insert_mask (bit a) goes into `sink`.  The counter step inserts Merged only (mapper.rs:120-124), the
// distance step Merged and Inserted (is_changed(), upsert.rs:31-33).  The number of entries is *d_count if given, else count.
__global__ __launch_bounds__(256) void note_actions_kernel(const hb_u128 *keys, const uint8_t *actions, const uint32_t *d_count, uint32_t count, uint32_t insert_mask,
                                                           Filter sink, unsigned long long *counts)
{
    const uint32_t n = d_count ? *d_count : count;
    unsigned long long c0 = 0, c1 = 0, c2 = 0;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const uint32_t a = actions[i];
        c0 += a == HBU_NO_CHANGE;
        c1 += a == HBU_MERGED;
        c2 += a == HBU_INSERTED;
        if (sink.kind != kNoFilter && ((insert_mask >> a) & 1u)) filter_insert(sink, keys[i]);
    }
    wave_add(&counts[HBU_NO_CHANGE], c0);
    wave_add(&counts[HBU_MERGED], c1);
    wave_add(&counts[HBU_INSERTED], c2);
}

// ---- setup_counters (mapper.rs:63-85): HyperLogLog::default() + add_u128(node) for every node, a quad per node --------------------
__global__ __launch_bounds__(256) void setup_values_kernel(const hb_u128 *nodes, uint32_t count, uint4 *out)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    const uint32_t i = t >> 2;
    if (i >= count) return;
    out[t] = hbk::counter_quarter_of_jp(hbk::initial_register_jp(nodes[i].lo), (int)(t & 3));
}
} // namespace hbr
