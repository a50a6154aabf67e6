// hb_ampc_fold.hip.h - device code of the approximated-harmonic job on the AMPC shard (include/hb_ampc.h): the per-source fold of a finished
// shortest-path job's distance table into the KahanSum centrality table (approximated_harmonic_centrality/coordinator.rs:139-145 with
// AddAssign<KahanSum>, kahan_sum.rs:65-72) and a worker's node sketch (HyperLogLog<4096>::add_u128 over its nodes, shortest_path/worker.rs:
// 44-49, hyperloglog.rs:4385-4400).  Included by hb_ampc.hip only; gfx950.  Atomics: the key index's own, the two counts, the maximum on
// the sketch's 32-bit words - never on a value table, never on a floating-point number.  No LDS.
// The fold needs the translation unit's -ffp-contract=off: `(1 / d) * norm - err` as one fused operation rounds once where the reference
// rounds twice (tests/test_ampc_approx_ref.py keeps an input on which the two differ).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hb_ampc.h"
#include "hb_ampc_round.hip.h"
#include "hb_ampc_values.hip.h"
#include "hb_bloom.hip.h"
#include "hb_table.hip.h"

namespace hbf {
using hbt::kEmpty;
using hbt::Table;
using hbt::u128;
using hbv::Kahan;

// One thread per slot of the DISTANCE table's key index (the keys of one table are distinct: nothing is sorted or grouped, and an entry of
// the centrality table has exactly one writer).  An entry below src_committed finds or claims its key in the centrality index `dst`, which
// has room for every key of the launch (the host grows it first).  An entry number at or above dst_committed is a key this launch
// inserted: the row is WRITTEN, {v, 0.0} = KahanSum::from(v), and never read (rows above `committed` may hold what a failed batch left).
// Anything else is read-add-write.  counts[0] += the entries folded, counts[1] += the keys inserted among them.
__global__ __launch_bounds__(256) void fold_distances_kernel(const u128 *src_keys, const uint32_t *src_pids, uint64_t src_slots, uint32_t src_committed,
                                                             const uint64_t *distances, Table dst, uint32_t dst_committed, Kahan *centralities, double norm,
                                                             uint32_t flags, unsigned long long *counts)
{
    unsigned long long folded = 0, inserted = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < src_slots; i += (uint64_t)gridDim.x * 256) {
        const uint32_t p = src_pids[i];
        const uint64_t d = p < src_committed ? distances[p] : 0;
        if (p < src_committed && !(d == 0 && (flags & HBU_FOLD_SKIP_ZERO))) {
            const uint32_t s = hbt::table_get(dst, src_keys[i], kEmpty);
            const double v = (1.0 / (double)d) * norm; // d == 0: inf, as the reference's `1.0 / distance as f64`
            Kahan k;
            if (s >= dst_committed) {
                k.sum = v;
                k.err = 0.0;
                inserted++;
            } else {
                k = centralities[s];
                const double y = (v + 0.0) - k.err; // rhs.sum + rhs.err of a KahanSum::from(v)
                const double t = k.sum + y;
                k.err = (t - k.sum) - y;
                k.sum = t;
            }
            centralities[s] = k;
            folded++;
        }
    }
    hbr::wave_add(&counts[0], folded);
    hbr::wave_add(&counts[1], inserted);
}

// HyperLogLog<4096>::add (b = 12) of every node's low half: h = lo * 11400714819323198549 (wrapping; add_u128 drops the high half),
// register h >> 52 takes the maximum with clz(h << 12) + 1 (65 where h << 12 is zero).  The registers are 32-bit words here: a byte-wise
// maximum is no word-wide atomicMax on packed bytes.  Most adds change nothing once a register has grown, and a register only grows: a
// value read first that is already large enough spares the atomic (a stale read is a lower bound and costs at most an atomic too many).
__global__ __launch_bounds__(256) void node_sketch_kernel(const hb_u128 *nodes, uint64_t count, uint32_t *registers)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (uint64_t)gridDim.x * 256) {
        const uint64_t h = nodes[i].lo * hbk::kBloomPrime;
        const uint32_t j = (uint32_t)(h >> 52);
        const uint64_t w = h << 12;
        const uint32_t p = (w ? (uint32_t)__clzll((long long)w) : 64u) + 1u;
        if (__hip_atomic_load(&registers[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < p) atomicMax(&registers[j], p);
    }
}
__global__ __launch_bounds__(256) void sketch_narrow_kernel(const uint32_t *registers, uint8_t *out)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < HBU_NODE_SKETCH_REGISTERS) out[i] = (uint8_t)registers[i];
}
} // namespace hbf
