// hb_bloom.hip.h - the slot arithmetic of U64BloomFilter (crates/bloom/src/lib.rs:85-106), shared by the reference-tail mode of the pass
// driver (hb_aux.hip.h) and the changed-node filter of the AMPC shard (hb_ampc_round.hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hbk {
// insert_u128 / contains_u128: slot = (low 64 bits of the id * LARGE_PRIME, wrapping) % num_bits; the high half of the id is ignored
constexpr unsigned long long kBloomPrime = 11400714819323198549ull;
__device__ __forceinline__ uint64_t bloom_slot(uint64_t id_low, uint64_t num_bits) { return (id_low * kBloomPrime) % num_bits; }
} // namespace hbk
