// hb_ampc_finish.hip.h - device code of the finish of an AMPC job on the shard (include/hb_ampc.h: hbu_finish_centralities,
// hbu_top_centralities, hbu_store_centralities): what the two coordinators do with the finished centrality table
// (harmonic_centrality/coordinator.rs:204-233, approximated_harmonic_centrality/coordinator.rs:152-177; store_harmonic and top_nodes,
// webgraph/centrality/mod.rs:33-114).  Included by hb_ampc.hip only; gfx950.  No LDS, no atomics: every output element has one writer.
// The sorts between the kernels are hb_ingest.hip's (gpu_sort_ids_device, gpu_rank_keys_device, gpu_store_keys_device).
// The division needs the translation unit's -fno-fast-math: the quotient is the IEEE one, correctly rounded, subnormals kept.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hb_ampc.h"

namespace hbn {

// f64::total_cmp as unsigned integer order (the mapping of hb_ingest.hip's rank_keys_kernel), inverted: ascending keys = descending
// values, +NaN first and -NaN last.  Every bit pattern is a result here: nothing is dropped.
__device__ __forceinline__ uint64_t descending_key(double v)
{
    uint64_t b = (uint64_t)__double_as_longlong(v);
    b ^= (b >> 63) ? ~0ull : 0x8000000000000000ull;
    return ~b;
}

// One thread per entry, in OUTPUT order (position j of the ascending-NodeID order, which the id sort has just produced): entry[j] is the
// entry number = the row of the value table.  STRIDE = doubles per row: 2 for a KahanSum {sum, err}, of which only `sum` is read
// (f64::from(KahanSum), kahan_sum.rs:35-39), 1 for an f64.  vals[j] = the quotient; key[j] = its sort key, taken from the QUOTIENT (a
// negative divisor reverses the order, a zero one folds everything onto inf / NaN).  The reads of the table are a gather (the entry
// numbers are a permutation), the two writes are coalesced.
template <int STRIDE>
__global__ __launch_bounds__(256) void finish_values_kernel(const double *table, const uint32_t *entry, uint64_t n, double divisor, double *vals, uint64_t *key)
{
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (uint64_t)gridDim.x * 256) {
        const double q = table[(uint64_t)entry[j] * STRIDE] / divisor;
        vals[j] = q;
        key[j] = descending_key(q);
    }
}

// top_nodes: position i of the rank order holds entry order[i] of the ascending-NodeID arrays; the first k of them are gathered so that
// only k ids and values cross the link.  ids_out / vals_out: k entries each, either may be NULL.
__global__ __launch_bounds__(256) void top_gather_kernel(const uint64_t *order, uint64_t k, const hb_u128 *ids, const double *vals, hb_u128 *ids_out, double *vals_out)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < k; i += (uint64_t)gridDim.x * 256) {
        const uint64_t j = order[i];
        if (ids_out) ids_out[i] = ids[j];
        if (vals_out) vals_out[i] = vals[j];
    }
}

} // namespace hbn
