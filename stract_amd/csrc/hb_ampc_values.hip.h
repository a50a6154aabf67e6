// hb_ampc_values.hip.h - device code of the scalar value tables of the AMPC shard (include/hb_ampc.h): the five scalar upsert
// operators of the reference (dht/upsert.rs:92-152) applied per key in batch order (dht/store.rs:159-190), set / get of 4-, 8- and
// 16-byte values, and CentralityMapper::update_centralities (harmonic_centrality/mapper.rs:157-209) over four resident tables.
// Included by hb_ampc.hip only; gfx950.  No floating-point atomics and no atomics on a value table: a key group has one writer.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/hb_ampc.h"
#include "hb_table.hip.h"
#include "hll64_tables.inc"
namespace hbk {
constexpr int kTableLen = HLL64_TABLE_LEN; // (hb_kernels.hip.h defines it for the pass kernels' translation unit; this one has its own)
}
#include "hb_estimator.hip.h"

namespace hbv {
using hbt::kEmpty;
using hbt::Table;
using hbt::u128;

// A key group of up to this many pairs is folded by one thread, a longer one by a whole wave (its lanes load 64 pairs' values
// through `perm` in one step).  hbu_wave_group_length() reports it: the tests put groups of this length and of one more / less.
constexpr uint32_t kWaveGroupLen = 32;
constexpr uint32_t kWaveAhead = 8; // chunks of 64 pairs whose loads a wave issues before it folds the first of them

struct alignas(16) Kahan { // KahanSum, kahan_sum.rs:30-33
    double sum, err;
};

// ---- the operators: merge(old, new), the action's `merged != old` (Rust's derived PartialEq = IEEE comparison) ---------------
// kScan: associative and exact, so a wave-wide prefix gives every pair of a chunk its `old` at once; the float operators are a
// serial chain by definition (one rounding per pair, in batch order) - only their loads are batched.
struct OpU64Add {
    using V = uint64_t;
    static constexpr bool kScan = true;
    static __device__ __forceinline__ V identity() { return 0; }
    static __device__ __forceinline__ V merge(V a, V b) { return a + b; } // wrapping (the reference: panic in a debug build, wrap in release)
    static __device__ __forceinline__ bool ne(V a, V b) { return a != b; }
};
struct OpU64Min {
    using V = uint64_t;
    static constexpr bool kScan = true;
    static __device__ __forceinline__ V identity() { return ~0ull; }
    static __device__ __forceinline__ V merge(V a, V b) { return b < a ? b : a; }
    static __device__ __forceinline__ bool ne(V a, V b) { return a != b; }
};
struct OpF32Add {
    using V = float;
    static constexpr bool kScan = false;
    static __device__ __forceinline__ V merge(V a, V b) { return a + b; }
    static __device__ __forceinline__ bool ne(V a, V b) { return a != b; } // NaN != NaN: Merged; -0.0 == +0.0: NoChange
    static __device__ __forceinline__ V lane_value(V v, int l) { return __shfl(v, l); }
};
struct OpF64Add {
    using V = double;
    static constexpr bool kScan = false;
    static __device__ __forceinline__ V merge(V a, V b) { return a + b; }
    static __device__ __forceinline__ bool ne(V a, V b) { return a != b; }
    static __device__ __forceinline__ V lane_value(V v, int l) { return __shfl(v, l); }
};
struct OpKahanAdd { // old += new.sum (kahan_sum.rs:47-54); new.err is ignored (upsert.rs:143-151) - it only arrives with an insert
    using V = Kahan;
    static constexpr bool kScan = false;
    static __device__ __forceinline__ V merge(V a, V b)
    {
        const double y = b.sum - a.err;
        const double t = a.sum + y;
        V r;
        r.err = (t - a.sum) - y;
        r.sum = t;
        return r;
    }
    static __device__ __forceinline__ bool ne(V a, V b) { return a.sum != b.sum || a.err != b.err; }
    static __device__ __forceinline__ V lane_value(V v, int l)
    {
        V r;
        r.sum = __shfl(v.sum, l);
        r.err = __shfl(v.err, l);
        return r;
    }
};

// One chunk (pairs c .. c + n of a group, n <= 64; lane l holds pair c + l's value, `act` = it has one) of a wave-folded group.
// Every lane of the wave calls these with wave-uniform cur / c / n / fresh and leaves with the same new cur; my_action = the
// action of this lane's pair.
template <class Op>
__device__ __forceinline__ void wave_chunk_scan(typename Op::V &cur, typename Op::V v, bool act, uint32_t c, bool fresh, uint32_t lane, uint8_t &my_action)
{
    using V = typename Op::V;
    V inc = act ? v : Op::identity();
#pragma unroll
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const V o = __shfl_up(inc, off);
        if (lane >= off) inc = Op::merge(o, inc);
    }
    V exc = __shfl_up(inc, 1u);
    if (lane == 0) exc = Op::identity();
    // (a fresh group starts from the identity: its first pair's value comes out verbatim)
    const V before = Op::merge(cur, exc), after = Op::merge(before, v);
    my_action = (fresh && c + lane == 0) ? HBU_INSERTED : (Op::ne(after, before) ? HBU_MERGED : HBU_NO_CHANGE);
    cur = Op::merge(cur, __shfl(inc, 63));
}
template <class Op>
__device__ __forceinline__ void wave_chunk_serial(typename Op::V &cur, typename Op::V v, uint32_t c, uint32_t n, bool fresh, uint32_t lane, uint8_t &my_action)
{
    using V = typename Op::V;
    // eight lanes' values are fetched before the first of them is added: the fetches do not depend on the chain, and one at a
    // time each addition would wait for a cross-lane round trip
    for (uint32_t l0 = 0; l0 < n; l0 += 8) { // wave-uniform trip count; every lane walks the same chain
        V vl[8];
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) vl[j] = Op::lane_value(v, (int)((l0 + j) & 63));
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) {
            const uint32_t l = l0 + j;
            if (l < n) { // wave-uniform
                uint8_t a;
                if (fresh && c + l == 0) {
                    a = HBU_INSERTED;
                    cur = vl[j];
                } else {
                    const V m = Op::merge(cur, vl[j]);
                    a = Op::ne(m, cur) ? HBU_MERGED : HBU_NO_CHANGE;
                    cur = m;
                }
                if (lane == l) my_action = a;
            }
        }
    }
}

// The upsert of one batch on a scalar table: group g = the pairs perm[heads[g] .. heads[g + 1]) of the batch (one key, batch
// order kept by the stable sort), folded into table[slot] strictly in that order; a fresh key (slot >= first_new) takes its
// first pair verbatim.  A thread per group up to kWaveGroupLen pairs; the longer groups of a wave's 64 are then folded by the
// whole wave, one after the other.
template <class Op>
__global__ __launch_bounds__(256) void group_apply_kernel(typename Op::V *table, const uint32_t *sorted_slot, const uint32_t *heads, const uint32_t *d_groups,
                                                          uint32_t count, uint32_t first_new, const uint32_t *perm, const typename Op::V *values, uint8_t *actions)
{
    using V = typename Op::V;
    const uint32_t groups = *d_groups;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t stride = gridDim.x * 256;
    for (uint32_t g0 = blockIdx.x * 256; g0 < groups; g0 += stride) { // block-uniform trip count: every lane of a wave stays in
        const uint32_t gidx = g0 + threadIdx.x;
        const bool valid = gidx < groups;
        uint32_t b = 0, len = 0, slot = 0;
        bool fresh = false;
        if (valid) {
            b = heads[gidx];
            len = (gidx + 1 < groups ? heads[gidx + 1] : count) - b;
            slot = sorted_slot[b];
            fresh = slot >= first_new;
        }
        if (valid && len <= kWaveGroupLen) {
            uint32_t i = 0;
            V cur;
            if (fresh) {
                const uint32_t pos = perm[b];
                cur = values[pos];
                actions[pos] = HBU_INSERTED;
                i = 1;
            } else {
                cur = table[slot];
            }
            for (; i < len; i++) {
                const uint32_t pos = perm[b + i];
                const V m = Op::merge(cur, values[pos]);
                actions[pos] = Op::ne(m, cur) ? HBU_MERGED : HBU_NO_CHANGE;
                cur = m;
            }
            table[slot] = cur;
        }
        uint64_t todo = __ballot(valid && len > kWaveGroupLen);
        while (todo) { // wave-uniform
            const int owner = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const uint32_t wb = __shfl(b, owner), wlen = __shfl(len, owner), wslot = __shfl(slot, owner);
            const bool wfresh = __shfl((int)fresh, owner) != 0;
            V cur = V();
            if constexpr (Op::kScan) cur = wfresh ? Op::identity() : table[wslot];
            else if (!wfresh) cur = table[wslot]; // (a fresh group's first pair sets it)
            // kWaveAhead chunks of 64 pairs per turn: their loads (position through perm, then the value) do not depend on the
            // fold, so all of them are in flight before the first chunk is folded
            uint32_t pos[kWaveAhead], pos_next[kWaveAhead];
#pragma unroll
            for (uint32_t k = 0; k < kWaveAhead; k++) pos[k] = 64 * k + lane < wlen ? perm[wb + 64 * k + lane] : kEmpty;
            for (uint32_t c0 = 0; c0 < wlen; c0 += 64 * kWaveAhead) {
                V v[kWaveAhead];
#pragma unroll
                for (uint32_t k = 0; k < kWaveAhead; k++) {
                    v[k] = V();
                    if (pos[k] != kEmpty) v[k] = values[pos[k]];
                }
#pragma unroll
                for (uint32_t k = 0; k < kWaveAhead; k++) { // the next turn's positions, under way while this turn is folded
                    const uint32_t i = c0 + 64 * (kWaveAhead + k) + lane;
                    pos_next[k] = i < wlen ? perm[wb + i] : kEmpty;
                }
#pragma unroll
                for (uint32_t k = 0; k < kWaveAhead; k++) {
                    const uint32_t c = c0 + 64 * k;
                    if (c < wlen) { // wave-uniform
                        const uint32_t n = wlen - c < 64u ? wlen - c : 64u;
                        const bool act = lane < n;
                        uint8_t a = 0;
                        if constexpr (Op::kScan) wave_chunk_scan<Op>(cur, v[k], act, c, wfresh, lane, a);
                        else wave_chunk_serial<Op>(cur, v[k], c, n, wfresh, lane, a);
                        if (act) actions[pos[k]] = a;
                    }
                }
#pragma unroll
                for (uint32_t k = 0; k < kWaveAhead; k++) pos[k] = pos_next[k];
            }
            if (lane == 0) table[wslot] = cur;
        }
    }
}

// batch_set on a scalar table: the last pair of a group wins.  RAW = the value as 4, 8 or 16 bytes.
template <class RAW>
__global__ __launch_bounds__(256) void group_set_kernel(RAW *table, const uint32_t *sorted_slot, const uint32_t *heads, const uint32_t *d_groups, uint32_t count,
                                                        const uint32_t *perm, const RAW *values)
{
    const uint32_t groups = *d_groups;
    for (uint32_t g = blockIdx.x * 256 + threadIdx.x; g < groups; g += gridDim.x * 256) {
        const uint32_t e = g + 1 < groups ? heads[g + 1] : count;
        table[sorted_slot[heads[g]]] = values[perm[e - 1]];
    }
}
template <class RAW>
__global__ __launch_bounds__(256) void get_values_kernel(const RAW *table, const uint32_t *slots, uint32_t count, RAW *out)
{
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < count; i += gridDim.x * 256) {
        const uint32_t s = slots[i];
        RAW v = RAW(); // 0 / 0.0 / KahanSum::default()
        if (s != kEmpty) v = table[s];
        out[i] = v;
    }
}

// the tables one side of update_centralities reads: index, visible keys, values
template <class V>
struct Side {
    Table index;
    uint32_t committed;
    const V *values;
};
template <class V>
__device__ __forceinline__ uint32_t side_find(const Side<V> &s, u128 key)
{
    const uint32_t slot = hbt::table_find(s.index, key);
    return slot < s.committed ? slot : kEmpty;
}

// CentralityMapper::update_centralities, a quad per node: found in both counter tables -> d = next.size() saturating-minus
// prev.size(); d != 0 -> (node, prev centrality or default + d / (round + 1)) is appended to out_keys / out_vals (lane 0 of the quad; the
// order of the output is the order of the atomic counter - the set that follows does not depend on it, duplicates of a node
// carry the same value).
__global__ __launch_bounds__(256) void update_centralities_kernel(const hb_u128 *nodes, uint32_t count, Side<uint4> prev_counters, Side<uint4> next_counters,
                                                                  Side<Kahan> prev_centrality, const double *raw, const double *bias, const uint8_t *lc,
                                                                  double round_plus_1, hb_u128 *out_keys, Kahan *out_vals, unsigned long long *out_count)
{
    const uint32_t q = threadIdx.x & 3;
    const uint32_t stride = gridDim.x * 64;
    for (uint32_t n0 = blockIdx.x * 64; n0 < count; n0 += stride) { // block-uniform: hll_size_quad holds a wave-wide ballot
        const uint32_t i = n0 + (threadIdx.x >> 2);
        u128 key = 0;
        uint32_t sp = kEmpty, sn = kEmpty;
        if (i < count) {
            key = ((u128)nodes[i].hi << 64) | (u128)nodes[i].lo;
            sp = side_find(prev_counters, key);
            sn = side_find(next_counters, key);
        }
        const bool both = sp != kEmpty && sn != kEmpty;
        uint4 vp = make_uint4(0, 0, 0, 0), vn = make_uint4(0, 0, 0, 0);
        if (both) {
            vp = prev_counters.values[(uint64_t)sp * 4 + q];
            vn = next_counters.values[(uint64_t)sn * 4 + q];
        }
        const uint64_t size_prev = hbk::hll_size_quad(vp, raw, bias, lc), size_next = hbk::hll_size_quad(vn, raw, bias, lc);
        const uint64_t d = size_next >= size_prev ? size_next - size_prev : 0; // saturating_sub
        if (both && d != 0 && q == 0) {
            Kahan k;
            k.sum = 0.0;
            k.err = 0.0;
            const uint32_t sv = side_find(prev_centrality, key);
            if (sv != kEmpty) k = prev_centrality.values[sv];
            const double rhs = (double)d / round_plus_1;
            const double y = rhs - k.err; // KahanSum += f64
            const double t = k.sum + y;
            k.err = (t - k.sum) - y;
            k.sum = t;
            const unsigned long long o = atomicAdd(out_count, 1ull);
            out_keys[o] = nodes[i];
            out_vals[o] = k;
        }
    }
}
} // namespace hbv
