// hb_ampc.hip - GPU-resident shard of the AMPC tables: the HyperLogLog<64> counter table with HyperLogLog64Upsert semantics, the
// scalar value tables with the five scalar upsert operators, a device copy of a table, the update_centralities step and the two edge
// steps update_counters / update_distances (include/hb_ampc.h cites the reference operations this serves; the scalar kernels live in
// hb_ampc_values.hip.h, those of the edge steps in hb_ampc_edges.hip.h), and a worker's resident graph and changed-node filter with the
// mapper steps that work between them and the tables (kernels in hb_ampc_round.hip.h), and what the approximated-harmonic job adds: the
// fold of a distance table into the centrality table, the worker's node sketch (kernels in hb_ampc_fold.hip.h) and the export of a table,
// and the 64-lane distance rows that walk a batch of sampled sources at once (kernels in hb_ampc_lanes.hip.h), and the finish of both jobs:
// a centrality table's values, ranks, top nodes and store (kernels in hb_ampc_finish.hip.h, the sorts are hb_ingest.hip's).
#include "hb_guard_alloc.h" // FIRST: no-op unless built with -DHB_GUARD_ALLOC=<mode> (debug allocators: guard pages / poison / red zones)
#include "hb_pool.h"        // then: every hipMalloc / hipFree below goes through the caching device allocator (shipped build)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "../../include/hb_ampc.h"
#include "hb_ampc_values.hip.h"
#include "hb_ampc_edges.hip.h"
#include "hb_ampc_round.hip.h"
#include "hb_ampc_fold.hip.h"
#include "hb_ampc_lanes.hip.h"
#include "hb_ampc_finish.hip.h"
#include "hb_internal.h"
#include "hb_regs.hip.h"
#include "hb_table.hip.h"

namespace {
thread_local std::string g_hbu_error;
using hbt::kEmpty;
using hbt::Table;
using hbt::u128;

__device__ __forceinline__ u128 make_key(const hb_u128 &v) { return ((u128)v.hi << 64) | (u128)v.lo; }

// ---- the key index lives on the device [r5] (rounds 2-4: a std::unordered_map on the host, one probe per pair on one core) ----
// key -> slot = hb_table.hip.h (the ingest's endpoint table: open addressing, one compare-and-swap per new key, slot ids in
// order of first arrival).  A batch: keys + values cross the link once; every pair finds or claims its slot; a STABLE radix
// sort of (slot, position) groups the pairs of one key in batch order; one quad per group applies them in that order.
__global__ __launch_bounds__(256) void slots_insert_kernel(const hb_u128 *keys, uint32_t count, Table t, uint32_t *slot)
{
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < count; i += gridDim.x * 256) slot[i] = hbt::table_get(t, make_key(keys[i]), kEmpty);
}
// read-only: slots >= committed are keys of a batch that failed half-way (never visible)
__global__ __launch_bounds__(256) void slots_find_kernel(const hb_u128 *keys, uint32_t count, Table t, uint32_t committed, uint32_t *slot, uint8_t *found)
{
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < count; i += gridDim.x * 256) {
        uint32_t s = hbt::table_find(t, make_key(keys[i]));
        if (s >= committed) s = kEmpty;
        slot[i] = s;
        if (found) found[i] = s != kEmpty;
    }
}
__global__ __launch_bounds__(256) void table_clear_kernel(uint32_t *pids, uint64_t slots)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < slots; i += (uint64_t)gridDim.x * 256) pids[i] = kEmpty;
}
// grow / repair: every entry whose slot id is below `keep` goes to the new table with its id
__global__ __launch_bounds__(256) void rehash_kernel(const u128 *old_keys, const uint32_t *old_pids, uint64_t old_slots, uint32_t keep, Table t)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < old_slots; i += (uint64_t)gridDim.x * 256) {
        const uint32_t p = old_pids[i];
        if (p < keep) (void)hbt::table_get(t, old_keys[i], p);
    }
}
// head of a group in the sorted order: the first pair of its slot
struct HeadFlag {
    const uint32_t *sorted;
    __host__ __device__ uint8_t operator()(uint32_t i) const { return (i == 0 || sorted[i] != sorted[i - 1]) ? 1 : 0; }
};

// One quad per key group: its pairs (positions perm[begin .. end) of the batch, batch order kept) are applied in
// order to the stored counter - absent (fresh: slot >= first_new) keys take the first pair as is.  MODE 0 = upsert, 1 = set.
template <int MODE>
__global__ __launch_bounds__(256) void upsert_kernel(uint4 *table, const uint32_t *sorted_slot, const uint32_t *heads, const uint32_t *d_groups, uint32_t count,
                                                     uint32_t first_new, const uint32_t *perm, const uint4 *values, uint8_t *actions)
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
        // the ballots below need every lane of the wave in the loop: iterate to the longest group of the wave
        uint32_t len = e - b, maxlen = len;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) maxlen = max(maxlen, (uint32_t)__shfl_xor((int)maxlen, off));
        for (uint32_t i = 0; i < maxlen; i++) {
            const bool act = valid && i < len;
            const uint32_t pos = act ? perm[b + i] : 0u;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (act) v = values[(uint64_t)pos * 4 + q];
            hbk::Acc acc;
            hbk::acc_zero(acc);
            hbk::acc_merge(acc, cur);
            if (MODE == 0 && !(fresh && i == 0)) hbk::acc_merge(acc, v);
            const uint4 merged = (MODE == 1 || (fresh && i == 0)) ? v : hbk::acc_value(acc);
            const uint64_t bal = __ballot(act && hbk::u4_ne(merged, cur));
            const bool changed = ((bal >> qshift) & 0xFull) != 0;
            if (act) {
                if (MODE == 0 && q == 0) actions[pos] = (fresh && i == 0) ? HBU_INSERTED : (changed ? HBU_MERGED : HBU_NO_CHANGE);
                cur = merged;
            }
        }
        if (valid) table[(uint64_t)slot * 4 + q] = cur;
    }
}

__global__ __launch_bounds__(256) void get_kernel(const uint4 *table, const uint32_t *slots, uint32_t count, uint4 *out)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    const uint32_t i = t >> 2;
    if (i >= count) return;
    const uint32_t s = slots[i];
    out[t] = s == 0xFFFFFFFFu ? make_uint4(0, 0, 0, 0) : table[(uint64_t)s * 4 + (t & 3)];
}
} // namespace

struct hbu_table {
    int device = 0;
    hipStream_t stream = nullptr;
    // key index (device): open-addressing table of `slots` entries, load factor <= 1/2
    u128 *d_keys = nullptr;
    uint32_t *d_pids = nullptr;
    uint64_t slots = 0;
    unsigned long long *d_next = nullptr; // slot ids handed out so far (device counter of the index)
    unsigned long long *h_word = nullptr; // pinned: read-backs of the counter / the group count
    uint64_t committed = 0;               // keys visible to the caller (= d_next outside a failed batch)
    bool broken = false;                  // a failed batch could not be undone: every further call is refused
    uint32_t kind = HBU_KIND_HLL64;
    uint32_t vbytes = 64; // bytes of one value of that kind
    void *d_table = nullptr; // cap x vbytes, value of slot s at s * vbytes
    uint64_t cap = 0;        // values allocated
    std::string err;
    // work memory of one batch, kept between calls (a mapper sends thousands of equally sized batches)
    void *d_work = nullptr;
    size_t work_bytes = 0;
};

namespace {
int fail(hbu_table *t, int code, const std::string &msg)
{
    (t ? t->err : g_hbu_error) = msg;
    return code;
}
#define HBU_HIP(call)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) return fail(t, e_ == hipErrorOutOfMemory ? HB_ERR_NOMEM : HB_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

template <class F>
int guarded(hbu_table *t, F &&f)
{
    try {
        return f();
    } catch (const std::bad_alloc &) {
        try { return fail(t, HB_ERR_NOMEM, "out of host memory"); } catch (...) { return HB_ERR_NOMEM; }
    } catch (...) {
        try { return fail(t, HB_ERR_INVALID, "unexpected C++ exception"); } catch (...) { return HB_ERR_INVALID; }
    }
}

unsigned grid_for(uint64_t items) { return (unsigned)std::min<uint64_t>(std::max<uint64_t>((items + 255) / 256, 1), 1u << 16); }
Table table_of(const hbu_table *t) { return Table{t->d_keys, t->d_pids, t->slots - 1, t->d_next}; }

// values for `need` keys
int reserve(hbu_table *t, uint64_t need)
{
    if (need <= t->cap) return HB_OK;
    const uint64_t cap = std::max<uint64_t>(need, std::max<uint64_t>(2 * t->cap, 1024));
    void *n = nullptr;
    if (hipMalloc((void **)&n, cap * t->vbytes) != hipSuccess) return fail(t, HB_ERR_NOMEM, "hipMalloc(value table) failed");
    hipError_t e = hipMemsetAsync(n, 0, cap * t->vbytes, t->stream);
    if (e == hipSuccess && t->cap) e = hipMemcpyAsync(n, t->d_table, t->cap * t->vbytes, hipMemcpyDeviceToDevice, t->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
    if (e != hipSuccess) {
        (void)hipFree(n);
        return fail(t, HB_ERR_HIP, hipGetErrorString(e));
    }
    if (t->d_table) (void)hipFree(t->d_table);
    t->d_table = n;
    t->cap = cap;
    return HB_OK;
}

// a key index with room for `keys` keys at load factor <= 1/2, holding the entries with ids < keep of the present one
int rebuild_index(hbu_table *t, uint64_t keys, uint64_t keep)
{
    uint64_t slots = 1024;
    while (slots < 2 * keys) slots <<= 1;
    u128 *nk = nullptr;
    uint32_t *np = nullptr;
    if (hipMalloc((void **)&nk, slots * sizeof(u128)) != hipSuccess || hipMalloc((void **)&np, slots * sizeof(uint32_t)) != hipSuccess) {
        if (nk) (void)hipFree(nk);
        (void)hipGetLastError();
        return fail(t, HB_ERR_NOMEM, "hipMalloc(key index) failed");
    }
    hipLaunchKernelGGL(table_clear_kernel, dim3(grid_for(slots)), dim3(256), 0, t->stream, np, slots);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && t->slots && keep) {
        const Table nt{nk, np, slots - 1, t->d_next};
        hipLaunchKernelGGL(rehash_kernel, dim3(grid_for(t->slots)), dim3(256), 0, t->stream, (const u128 *)t->d_keys, (const uint32_t *)t->d_pids, t->slots,
                           (uint32_t)keep, nt);
        e = hipGetLastError();
    }
    const unsigned long long next = keep;
    if (e == hipSuccess) e = hipMemcpyAsync(t->d_next, &next, sizeof(next), hipMemcpyHostToDevice, t->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
    if (e != hipSuccess) {
        (void)hipFree(nk);
        (void)hipFree(np);
        return fail(t, HB_ERR_HIP, hipGetErrorString(e));
    }
    if (t->d_keys) (void)hipFree(t->d_keys);
    if (t->d_pids) (void)hipFree(t->d_pids);
    t->d_keys = nk;
    t->d_pids = np;
    t->slots = slots;
    return HB_OK;
}

int work_memory(hbu_table *t, size_t bytes)
{
    if (bytes <= t->work_bytes) return HB_OK;
    if (t->d_work) (void)hipFree(t->d_work);
    t->d_work = nullptr;
    t->work_bytes = 0;
    if (hipMalloc(&t->d_work, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(t, HB_ERR_NOMEM, "hipMalloc(batch work memory) failed");
    }
    t->work_bytes = bytes;
    return HB_OK;
}
struct Carve { // consecutive 256-byte aligned pieces of the work buffer
    char *p;
    size_t used = 0;
    template <class T>
    T *take(size_t count)
    {
        T *r = (T *)((uintptr_t)p + used); // (integer arithmetic: the sizing pass carves from a null base)
        used += (count * sizeof(T) + 255) & ~(size_t)255;
        return r;
    }
};

constexpr uint32_t kOpSet = 0xFFFFFFFFu; // batch_set: no operator, the last pair of a key wins
uint32_t bytes_of_kind(uint32_t kind)
{
    switch (kind) {
    case HBU_KIND_HLL64: return 64;
    case HBU_KIND_U64: return 8;
    case HBU_KIND_F32: return 4;
    case HBU_KIND_F64: return 8;
    case HBU_KIND_KAHAN: return 16;
    case HBU_KIND_DIST64: return 64;
    default: return 0;
    }
}
uint32_t kind_of_op(uint32_t op)
{
    switch (op) {
    case HBU_OP_HLL64: return HBU_KIND_HLL64;
    case HBU_OP_U64_ADD:
    case HBU_OP_U64_MIN: return HBU_KIND_U64;
    case HBU_OP_F32_ADD: return HBU_KIND_F32;
    case HBU_OP_F64_ADD: return HBU_KIND_F64;
    case HBU_OP_KAHAN_ADD: return HBU_KIND_KAHAN;
    case HBU_OP_DIST64_MIN: return HBU_KIND_DIST64;
    default: return 0xFFFFFFFFu;
    }
}
const char *const kBrokenMsg = "the table is unusable: an earlier failed batch could not be undone";

// the pairs of a batch: in host memory (they cross the link once), or already in device memory and complete with respect to the
// table's stream (update_centralities hands its compacted result over this way)
struct Pairs {
    const hb_u128 *keys;
    const void *values;
    bool on_device;
    // update_counters: `values` is NULL and the counter of pair i is gathered from another table while the pair is folded
    const hbe::CounterSource *gather = nullptr;
    // round_lane_distances: `values` is NULL and the row of pair i is gathered from another lane table, with the `+ 1`, likewise
    const hbl::LaneSource *lanes = nullptr;
};
// update_distances: what comes back is one (key, action) per key GROUP of the batch instead of one action per pair (host memory,
// room for `count` entries each; the number of groups is *distinct)
struct GroupOut {
    hb_u128 *keys;
    uint8_t *actions;
};
// the round steps: the actions never leave the device.  `note` is called on the table's stream once the batch's kernels are queued,
// with one (key, action) per pair, or per key group if per_group (then *d_count of them); nothing is copied back but the counts.
struct DeviceSink {
    bool per_group;
    std::function<hipError_t(const hb_u128 *keys, const uint8_t *actions, const uint32_t *d_count)> note;
};

// shared body of batch_set (op = kOpSet) / batch_upsert; *distinct = the number of distinct keys of the batch
int apply(hbu_table *t, uint32_t op, Pairs in, uint64_t count, uint8_t *actions, uint64_t *distinct = nullptr, const GroupOut *per_group = nullptr,
          const DeviceSink *sink = nullptr)
{
    const bool upsert = op != kOpSet;
    if (!t || (count && (!in.keys || (!in.values && !in.gather && !in.lanes))) || (upsert && count && !actions && !per_group && !sink))
        return t ? fail(t, HB_ERR_INVALID, "NULL argument") : HB_ERR_INVALID;
    if (t->broken) return fail(t, HB_ERR_INVALID, kBrokenMsg);
    if (upsert && kind_of_op(op) != t->kind) return fail(t, HB_ERR_INVALID, "the upsert operator does not belong to the table's kind");
    // the kernels index 4 threads per pair / group with 32-bit thread ids
    if (count >= (1ull << 30)) return fail(t, HB_ERR_LIMIT, "batch too large (< 2^30 pairs per call)");
    if (distinct) *distinct = 0;
    if (!count) return HB_OK;
    HBU_HIP(hipSetDevice(t->device));
    if (t->committed + count >= 0xFFFFFFFEull) return fail(t, HB_ERR_LIMIT, "too many keys in one table (< 2^32)");
    // ---- everything that can fail for lack of memory comes BEFORE the index changes: room for count new keys (every pair might
    // bring one), their values, the batch's work memory
    int rc;
    // (slots = the power of two >= 2 x keys: the rounding is what makes repeated growth geometric)
    if (2 * (t->committed + count) > t->slots && (rc = rebuild_index(t, t->committed + count, t->committed))) return rc;
    if ((rc = reserve(t, t->committed + count))) return rc;
    size_t sort_bytes = 0, select_bytes = 0;
    const uint32_t n32 = (uint32_t)count;
    {
        uint32_t *nul = nullptr;
        auto iota = rocprim::make_counting_iterator<uint32_t>(0);
        HBU_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, (const uint32_t *)nul, nul, iota, nul, (size_t)count, 0, 32, t->stream));
        auto flags = rocprim::make_transform_iterator(iota, HeadFlag{nul});
        HBU_HIP(rocprim::select(nullptr, select_bytes, iota, flags, nul, nul, (size_t)count, t->stream));
    }
    const size_t tmp_bytes = std::max(sort_bytes, select_bytes);
    const uint64_t staged = in.on_device ? 0 : count; // pairs that need room in the work memory
    const uint64_t grouped = (per_group || (sink && sink->per_group)) ? count : 0; // (key, action) of every group
    hb_u128 *d_gkeys;
    uint8_t *d_gact;
    auto layout = [&](Carve &c, hb_u128 *&dk, char *&dv, uint32_t *&slot, uint32_t *&slot_s, uint32_t *&perm, uint32_t *&heads, uint32_t *&groups,
                      uint8_t *&act, char *&tmp) {
        dk = c.take<hb_u128>(staged);
        dv = c.take<char>(staged * t->vbytes);
        slot = c.take<uint32_t>(count);
        slot_s = c.take<uint32_t>(count);
        perm = c.take<uint32_t>(count);
        heads = c.take<uint32_t>(count);
        groups = c.take<uint32_t>(2);
        act = c.take<uint8_t>(count);
        tmp = c.take<char>(tmp_bytes);
        d_gkeys = c.take<hb_u128>(grouped);
        d_gact = c.take<uint8_t>(grouped);
    };
    hb_u128 *d_k;
    char *d_v;
    uint32_t *d_slot, *d_slot_s, *d_perm, *d_heads, *d_groups;
    uint8_t *d_act;
    char *d_tmp;
    {
        Carve probe{nullptr};
        layout(probe, d_k, d_v, d_slot, d_slot_s, d_perm, d_heads, d_groups, d_act, d_tmp);
        if ((rc = work_memory(t, probe.used))) return rc;
    }
    Carve carve{(char *)t->d_work};
    layout(carve, d_k, d_v, d_slot, d_slot_s, d_perm, d_heads, d_groups, d_act, d_tmp);
    const hb_u128 *keys_d = in.on_device ? in.keys : d_k;
    const void *vals_d = in.on_device ? in.values : d_v;
    // ---- from here on a failure is a HIP error; the keys this batch may have put into the index are taken out again
    // (the index is rebuilt from the entries below `committed`) before the error is returned: the batch is transactional
    const uint32_t first_new = (uint32_t)t->committed;
    auto launch_values = [&]() {
        const uint32_t *ss = d_slot_s, *hd = d_heads, *gr = d_groups, *pm = d_perm;
        const dim3 grid((unsigned)std::min<uint64_t>((count + 255) / 256, 1u << 16)), block(256);
#define HBU_SET(RAW) hipLaunchKernelGGL(hbv::group_set_kernel<RAW>, grid, block, 0, t->stream, (RAW *)t->d_table, ss, hd, gr, n32, pm, (const RAW *)vals_d)
#define HBU_UPSERT(OP) \
    hipLaunchKernelGGL(hbv::group_apply_kernel<hbv::OP>, grid, block, 0, t->stream, (hbv::OP::V *)t->d_table, ss, hd, gr, n32, first_new, pm, (const hbv::OP::V *)vals_d, d_act)
        switch (op) {
        case kOpSet:
            if (t->vbytes == 4) HBU_SET(uint32_t);
            else if (t->vbytes == 8) HBU_SET(uint64_t);
            else HBU_SET(uint4);
            break;
        case HBU_OP_U64_ADD: HBU_UPSERT(OpU64Add); break;
        case HBU_OP_U64_MIN: HBU_UPSERT(OpU64Min); break;
        case HBU_OP_F32_ADD: HBU_UPSERT(OpF32Add); break;
        case HBU_OP_F64_ADD: HBU_UPSERT(OpF64Add); break;
        default: HBU_UPSERT(OpKahanAdd); break;
        }
#undef HBU_SET
#undef HBU_UPSERT
    };
    auto run = [&]() -> hipError_t {
        hipError_t e = hipSuccess;
        if (!in.on_device) {
            e = hipMemcpyAsync(d_k, in.keys, count * sizeof(hb_u128), hipMemcpyHostToDevice, t->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(d_v, in.values, count * t->vbytes, hipMemcpyHostToDevice, t->stream);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(slots_insert_kernel, dim3(grid_for(count)), dim3(256), 0, t->stream, keys_d, n32, table_of(t), d_slot);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        auto iota = rocprim::make_counting_iterator<uint32_t>(0);
        size_t b = tmp_bytes;
        if ((e = rocprim::radix_sort_pairs(d_tmp, b, (const uint32_t *)d_slot, d_slot_s, iota, d_perm, (size_t)count, 0, 32, t->stream)) != hipSuccess) return e;
        auto flags = rocprim::make_transform_iterator(iota, HeadFlag{d_slot_s});
        b = tmp_bytes;
        if ((e = rocprim::select(d_tmp, b, iota, flags, d_heads, d_groups, (size_t)count, t->stream)) != hipSuccess) return e;
        const unsigned blocks = (unsigned)std::min<uint64_t>((count + 63) / 64, 1u << 16);
        if (t->vbytes != 64)
            launch_values();
        else if (t->kind == HBU_KIND_DIST64 && in.lanes)
            hipLaunchKernelGGL(hbl::upsert_lanes_kernel<true>, dim3(blocks), dim3(256), 0, t->stream, (uint4 *)t->d_table, (const uint32_t *)d_slot_s, (const uint32_t *)d_heads,
                               (const uint32_t *)d_groups, n32, first_new, (const uint32_t *)d_perm, (const uint4 *)nullptr, *in.lanes, d_act);
        else if (t->kind == HBU_KIND_DIST64 && upsert)
            hipLaunchKernelGGL(hbl::upsert_lanes_kernel<false>, dim3(blocks), dim3(256), 0, t->stream, (uint4 *)t->d_table, (const uint32_t *)d_slot_s, (const uint32_t *)d_heads,
                               (const uint32_t *)d_groups, n32, first_new, (const uint32_t *)d_perm, (const uint4 *)vals_d, hbl::LaneSource{nullptr, nullptr}, d_act);
        else if (in.gather)
            hipLaunchKernelGGL(hbe::upsert_edges_kernel, dim3(blocks), dim3(256), 0, t->stream, (uint4 *)t->d_table, (const uint32_t *)d_slot_s, (const uint32_t *)d_heads,
                               (const uint32_t *)d_groups, n32, first_new, (const uint32_t *)d_perm, *in.gather, d_act);
        else if (upsert)
            hipLaunchKernelGGL(upsert_kernel<0>, dim3(blocks), dim3(256), 0, t->stream, (uint4 *)t->d_table, (const uint32_t *)d_slot_s, (const uint32_t *)d_heads,
                               (const uint32_t *)d_groups, n32, first_new, (const uint32_t *)d_perm, (const uint4 *)vals_d, d_act);
        else
            hipLaunchKernelGGL(upsert_kernel<1>, dim3(blocks), dim3(256), 0, t->stream, (uint4 *)t->d_table, (const uint32_t *)d_slot_s, (const uint32_t *)d_heads,
                               (const uint32_t *)d_groups, n32, first_new, (const uint32_t *)d_perm, (const uint4 *)vals_d, d_act);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if (per_group || (sink && sink->per_group)) {
            hipLaunchKernelGGL(hbe::group_actions_kernel, dim3(grid_for(count)), dim3(256), 0, t->stream, (const uint32_t *)d_heads, (const uint32_t *)d_groups, n32,
                               (const uint32_t *)d_perm, keys_d, (const uint8_t *)d_act, d_gkeys, d_gact);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        } else if (upsert && !sink && (e = hipMemcpyAsync(actions, d_act, count, hipMemcpyDeviceToHost, t->stream)) != hipSuccess) {
            return e;
        }
        if (sink && (e = sink->per_group ? sink->note(d_gkeys, d_gact, d_groups) : sink->note(keys_d, d_act, nullptr)) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(t->h_word, t->d_next, sizeof(unsigned long long), hipMemcpyDeviceToHost, t->stream)) != hipSuccess) return e;
        t->h_word[1] = 0;
        if ((distinct || per_group) && (e = hipMemcpyAsync(&t->h_word[1], d_groups, sizeof(uint32_t), hipMemcpyDeviceToHost, t->stream)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(t->stream)) != hipSuccess || !per_group) return e;
        // the group count is known only now: exactly that many (key, action) entries cross the link
        const uint64_t groups = t->h_word[1];
        if ((e = hipMemcpyAsync(per_group->keys, d_gkeys, groups * sizeof(hb_u128), hipMemcpyDeviceToHost, t->stream)) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(per_group->actions, d_gact, groups, hipMemcpyDeviceToHost, t->stream)) != hipSuccess) return e;
        return hipStreamSynchronize(t->stream);
    };
    const hipError_t e = run();
    if (e != hipSuccess) {
        const std::string why = hipGetErrorString(e);
        (void)hipGetLastError();
        if (rebuild_index(t, std::max<uint64_t>(t->slots / 2, 512), t->committed)) t->broken = true;
        return fail(t, e == hipErrorOutOfMemory ? HB_ERR_NOMEM : HB_ERR_HIP, why);
    }
    t->committed = *t->h_word;
    if (distinct) *distinct = t->h_word[1];
    return HB_OK;
}

// shared body of the two batch_get calls
int get(hbu_table *t, const hb_u128 *keys, uint64_t count, void *values_out, uint8_t *found)
{
    if (!t || (count && (!keys || !values_out))) return t ? fail(t, HB_ERR_INVALID, "NULL argument") : HB_ERR_INVALID;
    if (count >= (1ull << 30)) return fail(t, HB_ERR_LIMIT, "batch too large (< 2^30 keys per call)"); // 4 threads per key, 32-bit ids
    if (!count) return HB_OK;
    if (t->broken) return fail(t, HB_ERR_INVALID, kBrokenMsg);
    HBU_HIP(hipSetDevice(t->device));
    Carve probe{nullptr};
    (void)probe.take<hb_u128>(count);
    (void)probe.take<uint32_t>(count);
    (void)probe.take<char>(count * t->vbytes);
    (void)probe.take<uint8_t>(count);
    int rc = work_memory(t, probe.used);
    if (rc) return rc;
    Carve carve{(char *)t->d_work};
    hb_u128 *d_k = carve.take<hb_u128>(count);
    uint32_t *d_slots = carve.take<uint32_t>(count);
    char *d_out = carve.take<char>(count * t->vbytes);
    uint8_t *d_found = carve.take<uint8_t>(count);
    HBU_HIP(hipMemcpyAsync(d_k, keys, count * sizeof(hb_u128), hipMemcpyHostToDevice, t->stream));
    hipLaunchKernelGGL(slots_find_kernel, dim3(grid_for(count)), dim3(256), 0, t->stream, (const hb_u128 *)d_k, (uint32_t)count, table_of(t),
                       (uint32_t)t->committed, d_slots, d_found);
#define HBU_GET(RAW) \
    hipLaunchKernelGGL(hbv::get_values_kernel<RAW>, dim3(grid_for(count)), dim3(256), 0, t->stream, (const RAW *)t->d_table, (const uint32_t *)d_slots, (uint32_t)count, (RAW *)d_out)
    if (t->kind == HBU_KIND_DIST64)
        hipLaunchKernelGGL(hbl::get_lanes_kernel, dim3((unsigned)((count * 4 + 255) / 256)), dim3(256), 0, t->stream, (const uint4 *)t->d_table, (const uint32_t *)d_slots,
                           (uint32_t)count, (uint4 *)d_out);
    else if (t->vbytes == 64)
        hipLaunchKernelGGL(get_kernel, dim3((unsigned)((count * 4 + 255) / 256)), dim3(256), 0, t->stream, (const uint4 *)t->d_table, (const uint32_t *)d_slots,
                           (uint32_t)count, (uint4 *)d_out);
    else if (t->vbytes == 4) HBU_GET(uint32_t);
    else if (t->vbytes == 8) HBU_GET(uint64_t);
    else HBU_GET(uint4);
#undef HBU_GET
    HBU_HIP(hipGetLastError());
    HBU_HIP(hipMemcpyAsync(values_out, d_out, count * t->vbytes, hipMemcpyDeviceToHost, t->stream));
    if (found) HBU_HIP(hipMemcpyAsync(found, d_found, count, hipMemcpyDeviceToHost, t->stream));
    HBU_HIP(hipStreamSynchronize(t->stream));
    return HB_OK;
}

// an empty table of `kind` with an index for index_keys keys and room for value_keys values
int create(int32_t device, uint32_t kind, uint64_t index_keys, uint64_t value_keys, hbu_table **out)
{
    hbu_table *t = nullptr;
    if (!out) return fail(t, HB_ERR_INVALID, "out == NULL");
    *out = nullptr;
    if (!bytes_of_kind(kind)) return fail(t, HB_ERR_INVALID, "unknown table kind");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(t, HB_ERR_NO_DEVICE, "no HIP device visible: this library has no CPU fallback");
    int dev = device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = 0;
    if (dev >= ndev) return fail(t, HB_ERR_INVALID, "device ordinal out of range");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess || std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(t, HB_ERR_NO_DEVICE, "kernels are built for gfx950 only");
    hbu_table *tab = new hbu_table();
    tab->device = dev;
    tab->kind = kind;
    tab->vbytes = bytes_of_kind(kind);
    if (hipSetDevice(dev) != hipSuccess || hipStreamCreateWithFlags(&tab->stream, hipStreamNonBlocking) != hipSuccess) {
        delete tab;
        return fail(t, HB_ERR_HIP, "stream creation failed");
    }
    int rc = HB_OK;
    if (hipMalloc((void **)&tab->d_next, 2 * sizeof(unsigned long long)) != hipSuccess || hipHostMalloc((void **)&tab->h_word, 2 * sizeof(unsigned long long)) != hipSuccess) {
        (void)hipGetLastError();
        rc = fail(tab, HB_ERR_NOMEM, "allocation of the index counter failed");
    }
    if (!rc) rc = rebuild_index(tab, std::max<uint64_t>(index_keys, 1), 0);
    if (!rc) rc = reserve(tab, std::max<uint64_t>(value_keys, 1));
    if (rc) {
        g_hbu_error = tab->err;
        hbu_destroy(tab);
        return rc;
    }
    *out = tab;
    return HB_OK;
}

// HyperLogLog<64>::size()'s tables on a device (hll64_tables.inc + the linear-counting table of hb_internal.h): they go up once
// per device and process and stay
struct EstimatorTables {
    double *raw = nullptr, *bias = nullptr;
    uint8_t *lc = nullptr;
};
std::mutex g_estimator_mu;
std::map<int, EstimatorTables> g_estimator;
int estimator_tables(hbu_table *t, EstimatorTables *out)
{
    std::lock_guard<std::mutex> lock(g_estimator_mu);
    auto it = g_estimator.find(t->device);
    if (it == g_estimator.end()) {
        uint8_t lc[68];
        if (!hb::build_lc_table(lc)) return fail(t, HB_ERR_INVALID, "host libm log() too close to a rounding boundary for the linear-counting table");
        EstimatorTables n;
        hipError_t e = hipMalloc((void **)&n.raw, sizeof(HLL64_RAW_ESTIMATE));
        if (e == hipSuccess) e = hipMalloc((void **)&n.bias, sizeof(HLL64_BIAS));
        if (e == hipSuccess) e = hipMalloc((void **)&n.lc, 68);
        if (e == hipSuccess) e = hipMemcpy(n.raw, HLL64_RAW_ESTIMATE, sizeof(HLL64_RAW_ESTIMATE), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(n.bias, HLL64_BIAS, sizeof(HLL64_BIAS), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(n.lc, lc, 68, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            for (void *p : {(void *)n.raw, (void *)n.bias, (void *)n.lc})
                if (p) (void)hipFree(p);
            return fail(t, e == hipErrorOutOfMemory ? HB_ERR_NOMEM : HB_ERR_HIP, std::string("estimator tables: ") + hipGetErrorString(e));
        }
        it = g_estimator.emplace(t->device, n).first;
    }
    *out = it->second;
    return HB_OK;
}
template <class V>
hbv::Side<V> side_of(const hbu_table *t) { return hbv::Side<V>{table_of(t), (uint32_t)t->committed, (const V *)t->d_table}; }
} // namespace

extern "C" {

const char *hbu_last_error(const hbu_table *t) { return t ? t->err.c_str() : g_hbu_error.c_str(); }

int hbu_create(int32_t device, uint64_t capacity_hint, hbu_table **out)
{
    return guarded(nullptr, [&]() -> int { return create(device, HBU_KIND_HLL64, capacity_hint, capacity_hint, out); });
}

int hbu_create_kind(int32_t device, uint64_t capacity_hint, uint32_t kind, hbu_table **out)
{
    return guarded(nullptr, [&]() -> int { return create(device, kind, capacity_hint, capacity_hint, out); });
}

int hbu_kind(const hbu_table *t, uint32_t *kind, uint32_t *value_bytes)
{
    if (!t) return HB_ERR_INVALID;
    if (kind) *kind = t->kind;
    if (value_bytes) *value_bytes = t->vbytes;
    return HB_OK;
}

uint32_t hbu_wave_group_length(void) { return hbv::kWaveGroupLen; }

void hbu_destroy(hbu_table *t)
{
    if (!t) return;
    (void)hipSetDevice(t->device);
    if (t->stream) (void)hipStreamSynchronize(t->stream);
    for (void *p : {(void *)t->d_table, (void *)t->d_keys, (void *)t->d_pids, (void *)t->d_next, t->d_work})
        if (p) (void)hipFree(p);
    if (t->h_word) (void)hipHostFree(t->h_word);
    if (t->stream) (void)hipStreamDestroy(t->stream);
    delete t;
}

int hbu_len(const hbu_table *t, uint64_t *keys)
{
    if (!t || !keys) return HB_ERR_INVALID;
    *keys = t->committed;
    return HB_OK;
}

// the three calls of the counter table: refused on a table of another kind
#define HBU_COUNTERS_ONLY(t) \
    if ((t) && (t)->kind != HBU_KIND_HLL64) return fail((t), HB_ERR_INVALID, "not a HyperLogLog<64> table: use the _values calls")

int hbu_batch_set(hbu_table *t, const hb_u128 *keys, const uint8_t *counters, uint64_t count)
{
    return guarded(t, [&]() -> int {
        HBU_COUNTERS_ONLY(t);
        return apply(t, kOpSet, Pairs{keys, counters, false}, count, nullptr);
    });
}

int hbu_batch_upsert(hbu_table *t, const hb_u128 *keys, const uint8_t *counters, uint64_t count, uint8_t *actions)
{
    return guarded(t, [&]() -> int {
        HBU_COUNTERS_ONLY(t);
        return apply(t, HBU_OP_HLL64, Pairs{keys, counters, false}, count, actions);
    });
}

int hbu_batch_get(hbu_table *t, const hb_u128 *keys, uint64_t count, uint8_t *counters_out, uint8_t *found)
{
    return guarded(t, [&]() -> int {
        HBU_COUNTERS_ONLY(t);
        return get(t, keys, count, counters_out, found);
    });
}

int hbu_batch_set_values(hbu_table *t, const hb_u128 *keys, const void *values, uint64_t count)
{
    return guarded(t, [&]() -> int { return apply(t, kOpSet, Pairs{keys, values, false}, count, nullptr); });
}

int hbu_batch_upsert_values(hbu_table *t, uint32_t op, const hb_u128 *keys, const void *values, uint64_t count, uint8_t *actions)
{
    return guarded(t, [&]() -> int {
        if (t && kind_of_op(op) == 0xFFFFFFFFu) return fail(t, HB_ERR_INVALID, "unknown upsert operator");
        return apply(t, op, Pairs{keys, values, false}, count, actions);
    });
}

int hbu_batch_get_values(hbu_table *t, const hb_u128 *keys, uint64_t count, void *values_out, uint8_t *found)
{
    return guarded(t, [&]() -> int { return get(t, keys, count, values_out, found); });
}

int hbu_clone(hbu_table *from, hbu_table **out)
{
    return guarded(from, [&]() -> int {
        hbu_table *t = from;
        if (!t || !out) return t ? fail(t, HB_ERR_INVALID, "NULL argument") : HB_ERR_INVALID;
        *out = nullptr;
        if (t->broken) return fail(t, HB_ERR_INVALID, kBrokenMsg);
        hbu_table *tab = nullptr;
        // (slots / 2 keys give an index of exactly `slots` entries: the copy keeps every entry where it is)
        int rc = create(t->device, t->kind, t->slots / 2, t->committed, &tab);
        if (rc) return fail(t, rc, g_hbu_error);
        // everything of `from` is complete on return of every call; the synchronise covers a caller that used another thread
        hipError_t e = tab->slots == t->slots ? hipStreamSynchronize(t->stream) : hipErrorInvalidValue;
        if (e == hipSuccess) e = hipMemcpyAsync(tab->d_keys, t->d_keys, t->slots * sizeof(u128), hipMemcpyDeviceToDevice, tab->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(tab->d_pids, t->d_pids, t->slots * sizeof(uint32_t), hipMemcpyDeviceToDevice, tab->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(tab->d_next, t->d_next, sizeof(unsigned long long), hipMemcpyDeviceToDevice, tab->stream);
        if (e == hipSuccess && t->committed) e = hipMemcpyAsync(tab->d_table, t->d_table, t->committed * t->vbytes, hipMemcpyDeviceToDevice, tab->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(tab->stream);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            hbu_destroy(tab);
            return fail(t, HB_ERR_HIP, std::string("copy of the table: ") + hipGetErrorString(e));
        }
        tab->committed = t->committed;
        *out = tab;
        return HB_OK;
    });
}

int hbu_export(hbu_table *t, hb_u128 *keys_out, void *values_out, uint64_t capacity, uint64_t *written)
{
    return guarded(t, [&]() -> int {
        if (written) *written = 0;
        if (!t || !written) return t ? fail(t, HB_ERR_INVALID, "NULL argument") : HB_ERR_INVALID;
        if (t->broken) return fail(t, HB_ERR_INVALID, kBrokenMsg);
        const uint64_t n = t->committed;
        if (capacity < n) return fail(t, HB_ERR_INVALID, "capacity below the number of keys");
        if (n && (!keys_out || !values_out)) return fail(t, HB_ERR_INVALID, "NULL argument");
        if (!n) return HB_OK;
        HBU_HIP(hipSetDevice(t->device));
        Carve probe{nullptr};
        (void)probe.take<hb_u128>(n);
        int rc = work_memory(t, probe.used);
        if (rc) return rc;
        hb_u128 *d_out = (hb_u128 *)t->d_work;
        // the keys go where their entry numbers point, which is where the values already are: rows 0 .. committed of the value table
        hipLaunchKernelGGL(hbr::set_export_kernel, dim3(grid_for(t->slots)), dim3(256), 0, t->stream, (const u128 *)t->d_keys, (const uint32_t *)t->d_pids, t->slots,
                           (uint32_t)n, d_out);
        HBU_HIP(hipGetLastError());
        HBU_HIP(hipMemcpyAsync(keys_out, d_out, n * sizeof(hb_u128), hipMemcpyDeviceToHost, t->stream));
        HBU_HIP(hipMemcpyAsync(values_out, t->d_table, n * t->vbytes, hipMemcpyDeviceToHost, t->stream));
        HBU_HIP(hipStreamSynchronize(t->stream));
        *written = n;
        return HB_OK;
    });
}

// shared body of hbu_fold_harmonic (n_lanes == 0: `distances` is HBU_KIND_U64) and hbu_fold_harmonic_lanes (HBU_KIND_DIST64, 1 .. 64 lanes)
static int fold_step(hbu_table *distances, hbu_table *centralities, double norm, uint32_t n_lanes, uint32_t flags, uint64_t *folded, uint64_t *inserted)
{
    hbu_table *t = centralities; // the table that changes: its stream runs the fold, its error text reports it
    const bool lanes = n_lanes != 0;
    {
        for (uint64_t *p : {folded, inserted})
            if (p) *p = 0;
        if (!distances || !t) return t ? fail(t, HB_ERR_INVALID, "NULL argument") : HB_ERR_INVALID;
        if (distances->kind != (lanes ? HBU_KIND_DIST64 : HBU_KIND_U64) || t->kind != HBU_KIND_KAHAN)
            return fail(t, HB_ERR_INVALID, lanes ? "fold_harmonic_lanes needs a 64-lane distance table and a KahanSum table" : "fold_harmonic needs a u64 table and a KahanSum table");
        if (distances->device != t->device) return fail(t, HB_ERR_INVALID, "the two tables are not on one device");
        if (distances->broken || t->broken) return fail(t, HB_ERR_INVALID, kBrokenMsg);
        if (flags & ~HBU_FOLD_SKIP_ZERO) return fail(t, HB_ERR_INVALID, "unknown flag bits");
        const uint64_t count = distances->committed;
        if (!count) return HB_OK;
        HBU_HIP(hipSetDevice(t->device));
        if (t->committed + count >= 0xFFFFFFFEull) return fail(t, HB_ERR_LIMIT, "too many keys in one table (< 2^32)");
        // room for every key of `distances` (each might be new) before the launch: the index never grows inside one
        int rc;
        if (2 * (t->committed + count) > t->slots && (rc = rebuild_index(t, t->committed + count, t->committed))) return rc;
        if ((rc = reserve(t, t->committed + count))) return rc;
        Carve probe{nullptr};
        (void)probe.take<unsigned long long>(2);
        if ((rc = work_memory(t, probe.used))) return rc;
        unsigned long long *d_counts = (unsigned long long *)t->d_work;
        HBU_HIP(hipStreamSynchronize(distances->stream)); // distances is only read: idle before this table's stream touches it
        unsigned long long h_counts[2] = {0, 0};
        // from here on a failure is a HIP error: the keys the kernel may have put into the index are taken out again, as apply() does
        auto run = [&]() -> hipError_t {
            hipError_t e = hipMemsetAsync(d_counts, 0, 2 * sizeof(unsigned long long), t->stream);
            if (e != hipSuccess) return e;
            if (lanes)
                hipLaunchKernelGGL(hbl::fold_lanes_kernel, dim3(grid_for(distances->slots)), dim3(256), 0, t->stream, (const u128 *)distances->d_keys,
                                   (const uint32_t *)distances->d_pids, distances->slots, (uint32_t)count, (const uint4 *)distances->d_table, n_lanes, table_of(t),
                                   (uint32_t)t->committed, (hbv::Kahan *)t->d_table, norm, flags, d_counts);
            else
                hipLaunchKernelGGL(hbf::fold_distances_kernel, dim3(grid_for(distances->slots)), dim3(256), 0, t->stream, (const u128 *)distances->d_keys,
                                   (const uint32_t *)distances->d_pids, distances->slots, (uint32_t)count, (const uint64_t *)distances->d_table, table_of(t),
                                   (uint32_t)t->committed, (hbv::Kahan *)t->d_table, norm, flags, d_counts);
            if ((e = hipGetLastError()) != hipSuccess) return e;
            if ((e = hipMemcpyAsync(t->h_word, t->d_next, sizeof(unsigned long long), hipMemcpyDeviceToHost, t->stream)) != hipSuccess) return e;
            if ((e = hipMemcpyAsync(h_counts, d_counts, sizeof(h_counts), hipMemcpyDeviceToHost, t->stream)) != hipSuccess) return e;
            return hipStreamSynchronize(t->stream);
        };
        const hipError_t e = run();
        if (e != hipSuccess) {
            const std::string why = hipGetErrorString(e);
            (void)hipGetLastError();
            if (rebuild_index(t, std::max<uint64_t>(t->slots / 2, 512), t->committed)) t->broken = true;
            return fail(t, e == hipErrorOutOfMemory ? HB_ERR_NOMEM : HB_ERR_HIP, why);
        }
        t->committed = *t->h_word;
        if (folded) *folded = h_counts[0];
        if (inserted) *inserted = h_counts[1];
        return HB_OK;
    }
}

int hbu_fold_harmonic(hbu_table *distances, hbu_table *centralities, double norm, uint32_t flags, uint64_t *folded, uint64_t *inserted)
{
    return guarded(centralities, [&]() -> int { return fold_step(distances, centralities, norm, 0, flags, folded, inserted); });
}

int hbu_fold_harmonic_lanes(hbu_table *lanes, hbu_table *centralities, double norm, uint32_t n_lanes, uint32_t flags, uint64_t *folded, uint64_t *inserted)
{
    return guarded(centralities, [&]() -> int {
        if (n_lanes == 0 || n_lanes > HBU_DIST_LANES) {
            for (uint64_t *p : {folded, inserted})
                if (p) *p = 0;
            return centralities ? fail(centralities, HB_ERR_INVALID, "n_lanes must be 1 .. 64") : HB_ERR_INVALID;
        }
        return fold_step(lanes, centralities, norm, n_lanes, flags, folded, inserted);
    });
}

// hbu_update_centralities; nodes_on_device: the ids are in device memory already, complete with respect to next_centrality's stream
// (hbu_round_centralities hands its selected nodes over this way)
static int centralities_step(hbu_table *prev_counters, hbu_table *next_counters, hbu_table *prev_centrality, hbu_table *next_centrality, const hb_u128 *nodes,
                             bool nodes_on_device, uint64_t count, uint64_t round, uint64_t *written)
{
    hbu_table *t = next_centrality; // the table that changes: its stream runs the step, its error text reports it
    {
        if (written) *written = 0;
        if (!prev_counters || !next_counters || !prev_centrality || !t || (count && !nodes)) return t ? fail(t, HB_ERR_INVALID, "NULL argument") : HB_ERR_INVALID;
        if (prev_counters->kind != HBU_KIND_HLL64 || next_counters->kind != HBU_KIND_HLL64 || prev_centrality->kind != HBU_KIND_KAHAN || t->kind != HBU_KIND_KAHAN)
            return fail(t, HB_ERR_INVALID, "update_centralities needs two HyperLogLog<64> tables and two KahanSum tables");
        if (prev_centrality == t) return fail(t, HB_ERR_INVALID, "prev_centrality and next_centrality are the same table");
        hbu_table *const others[3] = {prev_counters, next_counters, prev_centrality};
        for (hbu_table *o : others) {
            if (o->device != t->device) return fail(t, HB_ERR_INVALID, "the four tables are not on one device");
            if (o->broken) return fail(t, HB_ERR_INVALID, kBrokenMsg);
        }
        if (t->broken) return fail(t, HB_ERR_INVALID, kBrokenMsg);
        if (count >= (1ull << 30)) return fail(t, HB_ERR_LIMIT, "batch too large (< 2^30 nodes per call)");
        if (!count) return HB_OK;
        HBU_HIP(hipSetDevice(t->device));
        EstimatorTables est;
        int rc = estimator_tables(t, &est);
        if (rc) return rc;
        // staging lives in next_counters' work memory (apply() below may replace next_centrality's own): the nodes, the compacted
        // (node, value) pairs, their count
        hbu_table *const w = next_counters;
        const uint64_t staged = nodes_on_device ? 0 : count; // node ids that need room in the work memory
        Carve probe{nullptr};
        (void)probe.take<hb_u128>(staged);
        (void)probe.take<hb_u128>(count);
        (void)probe.take<hbv::Kahan>(count);
        (void)probe.take<unsigned long long>(2);
        if ((rc = work_memory(w, probe.used))) return fail(t, rc, w->err);
        Carve carve{(char *)w->d_work};
        const hb_u128 *d_nodes = carve.take<hb_u128>(staged);
        hb_u128 *d_keys = carve.take<hb_u128>(count);
        hbv::Kahan *d_vals = carve.take<hbv::Kahan>(count);
        unsigned long long *d_count = carve.take<unsigned long long>(2);
        // every table has its own stream: the three that are only read are idle before this one's stream touches them
        for (hbu_table *o : others) HBU_HIP(hipStreamSynchronize(o->stream));
        if (nodes_on_device) d_nodes = nodes;
        else HBU_HIP(hipMemcpyAsync((void *)d_nodes, nodes, count * sizeof(hb_u128), hipMemcpyHostToDevice, t->stream));
        HBU_HIP(hipMemsetAsync(d_count, 0, 2 * sizeof(unsigned long long), t->stream));
        const unsigned blocks = (unsigned)std::min<uint64_t>((count + 63) / 64, 1u << 16);
        hipLaunchKernelGGL(hbv::update_centralities_kernel, dim3(blocks), dim3(256), 0, t->stream, (const hb_u128 *)d_nodes, (uint32_t)count, side_of<uint4>(prev_counters),
                           side_of<uint4>(next_counters), side_of<hbv::Kahan>(prev_centrality), (const double *)est.raw, (const double *)est.bias,
                           (const uint8_t *)est.lc, (double)(round + 1), d_keys, d_vals, d_count);
        HBU_HIP(hipGetLastError());
        HBU_HIP(hipMemcpyAsync(t->h_word, d_count, sizeof(unsigned long long), hipMemcpyDeviceToHost, t->stream));
        HBU_HIP(hipStreamSynchronize(t->stream));
        const uint64_t pairs = *t->h_word; // (a count, not a counter or a size: what apply() must know to size its sort)
        uint64_t distinct = 0;
        if ((rc = apply(t, kOpSet, Pairs{d_keys, d_vals, true}, pairs, nullptr, &distinct))) return rc;
        if (written) *written = distinct;
        return HB_OK;
    }
}

int hbu_update_centralities(hbu_table *prev_counters, hbu_table *next_counters, hbu_table *prev_centrality, hbu_table *next_centrality, const hb_u128 *nodes,
                            uint64_t count, uint64_t round, uint64_t *written)
{
    return guarded(next_centrality, [&]() -> int {
        return centralities_step(prev_counters, next_counters, prev_centrality, next_centrality, nodes, false, count, round, written);
    });
}

// what the two edge steps refuse before they look at an edge; t = the table that changes
static int edge_step_refusal(hbu_table *prev, hbu_table *t, uint32_t kind, const hb_u128 *from, const hb_u128 *to, uint64_t count, const char *kinds_msg)
{
    if (!prev || !t) return t ? fail(t, HB_ERR_INVALID, "NULL argument") : HB_ERR_INVALID;
    if (count >= (1ull << 30)) return fail(t, HB_ERR_LIMIT, "batch too large (< 2^30 edges per call)"); // 32-bit positions, 4 threads per group
    if (count && (!from || !to)) return fail(t, HB_ERR_INVALID, "NULL argument");
    if (prev->kind != kind || t->kind != kind) return fail(t, HB_ERR_INVALID, kinds_msg);
    if (prev == t) return fail(t, HB_ERR_INVALID, "prev and next are the same table");
    if (prev->device != t->device) return fail(t, HB_ERR_INVALID, "the two tables are not on one device");
    if (prev->broken || t->broken) return fail(t, HB_ERR_INVALID, kBrokenMsg);
    return HB_OK;
}

int hbu_update_counters(hbu_table *prev_counters, hbu_table *next_counters, const hb_u128 *from, const hb_u128 *to, uint64_t count, uint8_t *actions)
{
    hbu_table *t = next_counters; // the table that changes: its stream runs the step, its error text reports it
    return guarded(t, [&]() -> int {
        int rc = edge_step_refusal(prev_counters, t, HBU_KIND_HLL64, from, to, count, "update_counters needs two HyperLogLog<64> tables");
        if (rc) return rc;
        if (count && !actions) return fail(t, HB_ERR_INVALID, "NULL argument");
        if (!count) return HB_OK;
        HBU_HIP(hipSetDevice(t->device));
        // staging lives in prev's work memory (apply() below may replace next's own): both ends of every edge, the source's slot, the
        // register its add sets.  No counter is staged.
        hbu_table *const w = prev_counters;
        Carve probe{nullptr};
        (void)probe.take<hb_u128>(count);
        (void)probe.take<hb_u128>(count);
        (void)probe.take<uint32_t>(count);
        (void)probe.take<uint16_t>(count);
        if ((rc = work_memory(w, probe.used))) return fail(t, rc, w->err);
        Carve carve{(char *)w->d_work};
        hb_u128 *d_from = carve.take<hb_u128>(count);
        hb_u128 *d_to = carve.take<hb_u128>(count);
        uint32_t *d_src = carve.take<uint32_t>(count);
        uint16_t *d_jp = carve.take<uint16_t>(count);
        HBU_HIP(hipStreamSynchronize(w->stream)); // prev is only read: idle before this table's stream touches it
        HBU_HIP(hipMemcpyAsync(d_from, from, count * sizeof(hb_u128), hipMemcpyHostToDevice, t->stream));
        HBU_HIP(hipMemcpyAsync(d_to, to, count * sizeof(hb_u128), hipMemcpyHostToDevice, t->stream));
        hipLaunchKernelGGL(hbe::counter_sources_kernel, dim3(grid_for(count)), dim3(256), 0, t->stream, (const hb_u128 *)d_from, (uint32_t)count,
                           side_of<uint4>(prev_counters), d_src, d_jp);
        HBU_HIP(hipGetLastError());
        const hbe::CounterSource src{(const uint4 *)prev_counters->d_table, d_src, d_jp};
        Pairs pairs{d_to, nullptr, true};
        pairs.gather = &src;
        return apply(t, HBU_OP_HLL64, pairs, count, actions);
    });
}

int hbu_update_distances(hbu_table *prev_distances, hbu_table *next_distances, const hb_u128 *from, const hb_u128 *to, uint64_t count, hb_u128 *keys_out,
                         uint8_t *actions_out, uint64_t *written)
{
    hbu_table *t = next_distances;
    return guarded(t, [&]() -> int {
        if (written) *written = 0;
        int rc = edge_step_refusal(prev_distances, t, HBU_KIND_U64, from, to, count, "update_distances needs two u64 tables");
        if (rc) return rc;
        if (count && (!keys_out || !actions_out || !written)) return fail(t, HB_ERR_INVALID, "NULL argument");
        if (!count) return HB_OK;
        HBU_HIP(hipSetDevice(t->device));
        // staging lives in prev's work memory, as above: the edges, a candidate and a flag per edge, the compacted (destination,
        // candidate) pairs of the edges that have one, their count
        hbu_table *const w = prev_distances;
        size_t select_bytes = 0, select_bytes_v = 0;
        {
            const uint8_t *nul = nullptr;
            HBU_HIP(rocprim::select(nullptr, select_bytes, (const hb_u128 *)nullptr, nul, (hb_u128 *)nullptr, (uint32_t *)nullptr, (size_t)count, t->stream));
            HBU_HIP(rocprim::select(nullptr, select_bytes_v, (const uint64_t *)nullptr, nul, (uint64_t *)nullptr, (uint32_t *)nullptr, (size_t)count, t->stream));
            select_bytes = std::max(select_bytes, select_bytes_v);
        }
        hb_u128 *d_from, *d_to, *d_keys;
        uint64_t *d_cand, *d_vals;
        uint8_t *d_has;
        uint32_t *d_count;
        char *d_tmp;
        auto layout = [&](Carve &c) {
            d_from = c.take<hb_u128>(count);
            d_to = c.take<hb_u128>(count);
            d_cand = c.take<uint64_t>(count);
            d_has = c.take<uint8_t>(count);
            d_keys = c.take<hb_u128>(count);
            d_vals = c.take<uint64_t>(count);
            d_count = c.take<uint32_t>(2);
            d_tmp = c.take<char>(select_bytes);
        };
        Carve probe{nullptr};
        layout(probe);
        if ((rc = work_memory(w, probe.used))) return fail(t, rc, w->err);
        Carve carve{(char *)w->d_work};
        layout(carve);
        HBU_HIP(hipStreamSynchronize(w->stream));
        HBU_HIP(hipMemcpyAsync(d_from, from, count * sizeof(hb_u128), hipMemcpyHostToDevice, t->stream));
        HBU_HIP(hipMemcpyAsync(d_to, to, count * sizeof(hb_u128), hipMemcpyHostToDevice, t->stream));
        hipLaunchKernelGGL(hbe::distance_candidates_kernel, dim3(grid_for(count)), dim3(256), 0, t->stream, (const hb_u128 *)d_from, (uint32_t)count,
                           side_of<uint64_t>(prev_distances), d_cand, d_has);
        HBU_HIP(hipGetLastError());
        // the edges that have a candidate, batch order kept; only their destinations ever reach next's index
        size_t b = select_bytes;
        HBU_HIP(rocprim::select(d_tmp, b, (const hb_u128 *)d_to, (const uint8_t *)d_has, d_keys, d_count, (size_t)count, t->stream));
        b = select_bytes;
        HBU_HIP(rocprim::select(d_tmp, b, (const uint64_t *)d_cand, (const uint8_t *)d_has, d_vals, d_count + 1, (size_t)count, t->stream));
        *t->h_word = 0; // (the copy fills its low half)
        HBU_HIP(hipMemcpyAsync(t->h_word, d_count, sizeof(uint32_t), hipMemcpyDeviceToHost, t->stream));
        HBU_HIP(hipStreamSynchronize(t->stream));
        const uint64_t pairs = *t->h_word; // (a count: what apply() must know to size its sort)
        const GroupOut out{keys_out, actions_out};
        uint64_t groups = 0;
        if ((rc = apply(t, HBU_OP_U64_MIN, Pairs{d_keys, d_vals, true}, pairs, nullptr, &groups, &out))) return rc;
        *written = groups;
        return HB_OK;
    });
}

} // extern "C"

// ==== a worker's resident graph and changed-node filter, and the mapper steps between them and the tables ==========================
struct hbu_graph {
    int device = 0;
    hb_u128 *d_nodes = nullptr, *d_from = nullptr, *d_to = nullptr;
    uint64_t n_nodes = 0, n_edges = 0;
    uint64_t chunk = 0; // edges (or nodes) per internal pass
    // staging of one chunk, kept between calls (a round makes the same passes every time); mutable: the steps take the graph as const
    mutable void *d_work = nullptr;
    mutable size_t work_bytes = 0;
};

struct hbu_filter {
    int device = 0;
    uint32_t kind = HBU_FILTER_BLOOM;
    uint64_t num_bits = 0;
    uint64_t words = 0;         // bloom: 32-bit words allocated = 2 x ceil(num_bits / 64)
    uint32_t *d_bits = nullptr; // bloom
    // the filter's stream, pinned read-back words and staging memory; for an exact set also its members: the key index of this table
    // (no value is ever stored), `committed` = the members
    hbu_table *t = nullptr;
};

namespace {
constexpr uint64_t kDefaultChunk = 1ull << 22;
constexpr uint64_t kSetupChunk = 1ull << 20; // nodes per pass of setup_counters: 64 B of counter are staged per node

hbr::Filter filter_view(const hbu_filter *f)
{
    if (!f) return hbr::Filter{hbr::kNoFilter, 0, nullptr, Table{nullptr, nullptr, 0, nullptr}, 0};
    return hbr::Filter{f->kind, (uint32_t)f->num_bits, f->d_bits, table_of(f->t), (uint32_t)f->t->committed};
}
unsigned grid_capped(uint64_t items) { return (unsigned)std::min<uint64_t>(std::max<uint64_t>((items + 255) / 256, 1), 4096); }

// an exact set gets room for `more` new members before a kernel inserts them (the index never grows inside a launch)
int set_reserve(hbu_filter *f, uint64_t more)
{
    hbu_table *c = f->t;
    if (f->kind != HBU_FILTER_EXACT) return HB_OK;
    if (c->committed + more >= 0xFFFFFFFEull) return fail(c, HB_ERR_LIMIT, "too many ids in one exact filter (< 2^32)");
    if (2 * (c->committed + more) > c->slots) return rebuild_index(c, c->committed + more, c->committed);
    return HB_OK;
}
// ... and learns afterwards how many it holds; `stream`: the one the inserting kernel ran on
int set_commit(hbu_filter *f, hipStream_t stream)
{
    hbu_table *t = f->t;
    if (f->kind != HBU_FILTER_EXACT) return HB_OK;
    HBU_HIP(hipMemcpyAsync(t->h_word, t->d_next, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    HBU_HIP(hipStreamSynchronize(stream));
    t->committed = *t->h_word;
    return HB_OK;
}
// thread's error text for the graph / filter calls (hbu_last_error(NULL))
int refuse(int code, const std::string &msg) { return fail(nullptr, code, msg); }
int filter_fail(hbu_filter *f, int rc) { return refuse(rc, f->t->err); }

int graph_work(const hbu_graph *g, hbu_table *t, size_t bytes)
{
    if (bytes <= g->work_bytes) return HB_OK;
    if (g->d_work) (void)hipFree(g->d_work);
    g->d_work = nullptr;
    g->work_bytes = 0;
    if (hipMalloc(&g->d_work, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(t, HB_ERR_NOMEM, "hipMalloc(chunk work memory) failed");
    }
    g->work_bytes = bytes;
    return HB_OK;
}

// what every round step refuses before it reads an edge; t = the table that changes
int round_refusal(std::initializer_list<hbu_table *> read_only, hbu_table *t, const hbu_graph *g, const hbu_filter *changed, const hbu_filter *new_changed,
                  bool changed_required)
{
    if (!t) return HB_ERR_INVALID;
    for (hbu_table *o : read_only)
        if (!o) return fail(t, HB_ERR_INVALID, "NULL argument");
    if (!g || (changed_required && !changed)) return fail(t, HB_ERR_INVALID, "NULL argument");
    for (hbu_table *o : read_only) {
        if (o == t) return fail(t, HB_ERR_INVALID, "prev and next are the same table");
        if (o->device != t->device) return fail(t, HB_ERR_INVALID, "the objects are not on one device");
        if (o->broken) return fail(t, HB_ERR_INVALID, kBrokenMsg);
    }
    if (t->broken) return fail(t, HB_ERR_INVALID, kBrokenMsg);
    if (g->device != t->device || (changed && changed->device != t->device) || (new_changed && new_changed->device != t->device))
        return fail(t, HB_ERR_INVALID, "the objects are not on one device");
    if (changed && changed == new_changed) return fail(t, HB_ERR_INVALID, "changed and new_changed are the same filter");
    if ((changed && changed->t->broken) || (new_changed && new_changed->t->broken)) return fail(t, HB_ERR_INVALID, kBrokenMsg);
    return HB_OK;
}

// the edge steps share everything but the kernels: kRoundCounters = map_cardinalities, kRoundDistances = RelaxEdges, kRoundLanes = RelaxEdges
// for the 64 sources of a lane row (staged per edge: the source's slot, as for the counters, and no register)
enum RoundMode { kRoundCounters = 0, kRoundDistances = 1, kRoundLanes = 2 };
template <RoundMode MODE>
int round_edges(hbu_table *prev, hbu_table *t, const hbu_graph *g, hbu_filter *changed, hbu_filter *new_changed, uint64_t counts_out[4])
{
    constexpr bool DISTANCES = MODE == kRoundDistances, LANES = MODE == kRoundLanes;
    const uint64_t chunk = std::min<uint64_t>(g->chunk, std::max<uint64_t>(g->n_edges, 1));
    size_t tmp_bytes = 0;
    {
        const uint8_t *nul = nullptr;
        size_t b = 0;
        HBU_HIP(rocprim::select(nullptr, b, (const hb_u128 *)nullptr, nul, (hb_u128 *)nullptr, (uint32_t *)nullptr, (size_t)chunk, t->stream));
        tmp_bytes = std::max(tmp_bytes, b);
        HBU_HIP(rocprim::select(nullptr, b, (const uint64_t *)nullptr, nul, (uint64_t *)nullptr, (uint32_t *)nullptr, (size_t)chunk, t->stream));
        tmp_bytes = std::max(tmp_bytes, b);
        HBU_HIP(rocprim::select(nullptr, b, (const uint32_t *)nullptr, nul, (uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)chunk, t->stream));
        tmp_bytes = std::max(tmp_bytes, b);
        HBU_HIP(rocprim::select(nullptr, b, (const uint16_t *)nullptr, nul, (uint16_t *)nullptr, (uint32_t *)nullptr, (size_t)chunk, t->stream));
        tmp_bytes = std::max(tmp_bytes, b);
    }
    // one chunk's staging: a flag and the per-edge words of every edge, then the compacted destinations and words of the selected ones
    uint8_t *d_flag;
    uint32_t *d_slot, *d_slot_c, *d_n;
    uint16_t *d_jp, *d_jp_c;
    uint64_t *d_cand, *d_cand_c;
    hb_u128 *d_keys;
    unsigned long long *d_counts;
    char *d_tmp;
    auto layout = [&](Carve &c) {
        d_flag = c.take<uint8_t>(chunk);
        d_slot = c.take<uint32_t>(DISTANCES ? 0 : chunk);
        d_slot_c = c.take<uint32_t>(DISTANCES ? 0 : chunk);
        d_jp = c.take<uint16_t>(DISTANCES || LANES ? 0 : chunk);
        d_jp_c = c.take<uint16_t>(DISTANCES || LANES ? 0 : chunk);
        d_cand = c.take<uint64_t>(DISTANCES ? chunk : 0);
        d_cand_c = c.take<uint64_t>(DISTANCES ? chunk : 0);
        d_keys = c.take<hb_u128>(chunk);
        d_n = c.take<uint32_t>(4);
        d_counts = c.take<unsigned long long>(4);
        d_tmp = c.take<char>(tmp_bytes);
    };
    Carve probe{nullptr};
    layout(probe);
    int rc;
    if ((rc = graph_work(g, t, probe.used))) return rc;
    Carve carve{(char *)g->d_work};
    layout(carve);
    HBU_HIP(hipStreamSynchronize(prev->stream)); // prev and changed are only read: idle before this table's stream touches them
    HBU_HIP(hipStreamSynchronize(changed->t->stream));
    if (new_changed) HBU_HIP(hipStreamSynchronize(new_changed->t->stream));
    HBU_HIP(hipMemsetAsync(d_counts, 0, 4 * sizeof(unsigned long long), t->stream));
    const hbr::Filter in = filter_view(changed);
    uint64_t selected = 0;
    for (uint64_t b = 0; b < g->n_edges; b += chunk) {
        const uint64_t n = std::min<uint64_t>(chunk, g->n_edges - b);
        const hb_u128 *from = g->d_from + b, *to = g->d_to + b;
        size_t tb = tmp_bytes;
        if (DISTANCES) {
            hipLaunchKernelGGL(hbr::select_distance_edges_kernel, dim3(grid_capped(n)), dim3(256), 0, t->stream, from, (uint32_t)n, in, side_of<uint64_t>(prev), d_flag,
                               d_cand, d_counts + 3);
            HBU_HIP(hipGetLastError());
            HBU_HIP(rocprim::select(d_tmp, tb, to, (const uint8_t *)d_flag, d_keys, d_n, (size_t)n, t->stream));
        } else if (LANES) {
            hipLaunchKernelGGL(hbl::select_lane_edges_kernel, dim3(grid_for(n)), dim3(256), 0, t->stream, from, (uint32_t)n, in, side_of<uint4>(prev), d_flag, d_slot);
            HBU_HIP(hipGetLastError());
            HBU_HIP(rocprim::select(d_tmp, tb, to, (const uint8_t *)d_flag, d_keys, d_n, (size_t)n, t->stream));
        } else {
            hipLaunchKernelGGL(hbr::select_counter_edges_kernel, dim3(grid_for(n)), dim3(256), 0, t->stream, from, (uint32_t)n, in, side_of<uint4>(prev), d_flag, d_slot,
                               d_jp);
            HBU_HIP(hipGetLastError());
            HBU_HIP(rocprim::select(d_tmp, tb, to, (const uint8_t *)d_flag, d_keys, d_n, (size_t)n, t->stream));
        }
        *t->h_word = 0; // (the copy fills its low half)
        HBU_HIP(hipMemcpyAsync(t->h_word, d_n, sizeof(uint32_t), hipMemcpyDeviceToHost, t->stream));
        HBU_HIP(hipStreamSynchronize(t->stream));
        const uint64_t pairs = *t->h_word; // (a count: what apply() must know to size its sort)
        if (!DISTANCES) selected += pairs;
        if (!pairs) continue; // (a chunk that selects nothing has compacted its destinations only)
        // the per-edge words of the selected edges, in the same order (queued in front of apply()'s kernels on the same stream)
        if (DISTANCES) {
            tb = tmp_bytes;
            HBU_HIP(rocprim::select(d_tmp, tb, (const uint64_t *)d_cand, (const uint8_t *)d_flag, d_cand_c, d_n + 1, (size_t)n, t->stream));
        } else {
            tb = tmp_bytes;
            HBU_HIP(rocprim::select(d_tmp, tb, (const uint32_t *)d_slot, (const uint8_t *)d_flag, d_slot_c, d_n + 1, (size_t)n, t->stream));
            if (!LANES) {
                tb = tmp_bytes;
                HBU_HIP(rocprim::select(d_tmp, tb, (const uint16_t *)d_jp, (const uint8_t *)d_flag, d_jp_c, d_n + 2, (size_t)n, t->stream));
            }
        }
        if (new_changed && (rc = set_reserve(new_changed, pairs))) return fail(t, rc, new_changed->t->err);
        const hbr::Filter out = filter_view(new_changed);
        DeviceSink sink;
        sink.per_group = DISTANCES;
        sink.note = [&](const hb_u128 *keys, const uint8_t *actions, const uint32_t *d_count) -> hipError_t {
            const uint32_t mask = DISTANCES || LANES ? ((1u << HBU_MERGED) | (1u << HBU_INSERTED)) : (1u << HBU_MERGED);
            hipLaunchKernelGGL(hbr::note_actions_kernel, dim3(grid_capped(pairs)), dim3(256), 0, t->stream, keys, actions, d_count, (uint32_t)pairs, mask, out, d_counts);
            return hipGetLastError();
        };
        if (DISTANCES) {
            rc = apply(t, HBU_OP_U64_MIN, Pairs{d_keys, d_cand_c, true}, pairs, nullptr, nullptr, nullptr, &sink);
        } else if (LANES) {
            const hbl::LaneSource src{(const uint4 *)prev->d_table, d_slot_c};
            Pairs p{d_keys, nullptr, true};
            p.lanes = &src;
            rc = apply(t, HBU_OP_DIST64_MIN, p, pairs, nullptr, nullptr, nullptr, &sink);
        } else {
            const hbe::CounterSource src{(const uint4 *)prev->d_table, d_slot_c, d_jp_c};
            Pairs p{d_keys, nullptr, true};
            p.gather = &src;
            rc = apply(t, HBU_OP_HLL64, p, pairs, nullptr, nullptr, nullptr, &sink);
        }
        if (rc) return rc;
        if (new_changed && (rc = set_commit(new_changed, t->stream))) return fail(t, rc, new_changed->t->err);
    }
    unsigned long long h[4];
    HBU_HIP(hipMemcpyAsync(h, d_counts, sizeof(h), hipMemcpyDeviceToHost, t->stream));
    HBU_HIP(hipStreamSynchronize(t->stream));
    counts_out[0] = DISTANCES ? h[3] : selected;
    counts_out[1] = h[HBU_MERGED];
    counts_out[2] = h[HBU_INSERTED];
    return HB_OK;
}
} // namespace

extern "C" {

uint64_t hbu_bloom_num_bits(uint64_t estimated_items, double fp)
{
    const double ln2 = std::log(2.0);
    const double v = std::ceil((double)estimated_items * std::log(fp) / (-8.0 * (ln2 * ln2)));
    if (!(v > 0.0)) return 0; // Rust's `as u64` saturates: NaN and negatives are 0
    if (v >= 18446744073709551616.0) return ~0ull;
    return (uint64_t)v;
}

int hbu_graph_create(int32_t device, const hb_u128 *nodes, uint64_t n_nodes, const hb_u128 *from, const hb_u128 *to, uint64_t n_edges, uint64_t chunk_edges,
                     hbu_graph **out)
{
    return guarded(nullptr, [&]() -> int {
        hbu_table *t = nullptr; // (HBU_HIP reports through the thread's error text)
        if (!out) return refuse(HB_ERR_INVALID, "out == NULL");
        *out = nullptr;
        if ((n_nodes && !nodes) || (n_edges && (!from || !to))) return refuse(HB_ERR_INVALID, "NULL argument");
        if (chunk_edges >= (1ull << 30)) return refuse(HB_ERR_LIMIT, "chunk_edges too large (< 2^30)");
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return refuse(HB_ERR_NO_DEVICE, "no HIP device visible: this library has no CPU fallback");
        int dev = device;
        if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = 0;
        if (dev >= ndev) return refuse(HB_ERR_INVALID, "device ordinal out of range");
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) != hipSuccess || std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
            return refuse(HB_ERR_NO_DEVICE, "kernels are built for gfx950 only");
        HBU_HIP(hipSetDevice(dev));
        hbu_graph *g = new hbu_graph();
        g->device = dev;
        g->n_nodes = n_nodes;
        g->n_edges = n_edges;
        g->chunk = chunk_edges ? chunk_edges : kDefaultChunk;
        hipError_t e = hipSuccess;
        if (n_nodes) e = hipMalloc((void **)&g->d_nodes, n_nodes * sizeof(hb_u128));
        if (e == hipSuccess && n_edges) e = hipMalloc((void **)&g->d_from, n_edges * sizeof(hb_u128));
        if (e == hipSuccess && n_edges) e = hipMalloc((void **)&g->d_to, n_edges * sizeof(hb_u128));
        if (e == hipSuccess && n_nodes) e = hipMemcpy(g->d_nodes, nodes, n_nodes * sizeof(hb_u128), hipMemcpyHostToDevice);
        if (e == hipSuccess && n_edges) e = hipMemcpy(g->d_from, from, n_edges * sizeof(hb_u128), hipMemcpyHostToDevice);
        if (e == hipSuccess && n_edges) e = hipMemcpy(g->d_to, to, n_edges * sizeof(hb_u128), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            hbu_graph_destroy(g);
            return refuse(e == hipErrorOutOfMemory ? HB_ERR_NOMEM : HB_ERR_HIP, std::string("upload of the graph: ") + hipGetErrorString(e));
        }
        *out = g;
        return HB_OK;
    });
}

int hbu_graph_len(const hbu_graph *g, uint64_t *n_nodes, uint64_t *n_edges)
{
    if (!g) return HB_ERR_INVALID;
    if (n_nodes) *n_nodes = g->n_nodes;
    if (n_edges) *n_edges = g->n_edges;
    return HB_OK;
}

void hbu_graph_destroy(hbu_graph *g)
{
    if (!g) return;
    (void)hipSetDevice(g->device);
    for (void *p : {(void *)g->d_nodes, (void *)g->d_from, (void *)g->d_to, g->d_work})
        if (p) (void)hipFree(p);
    delete g;
}

int hbu_graph_node_sketch(const hbu_graph *g, uint8_t *registers_out)
{
    return guarded(nullptr, [&]() -> int {
        hbu_table *t = nullptr; // (HBU_HIP reports through the thread's error text)
        if (!g || !registers_out) return refuse(HB_ERR_INVALID, "NULL argument");
        HBU_HIP(hipSetDevice(g->device));
        // 4096 words for the maxima, then the bytes; a graph has no stream of its own: the device's default one, and the copy waits for it
        Carve probe{nullptr};
        (void)probe.take<uint32_t>(HBU_NODE_SKETCH_REGISTERS);
        (void)probe.take<uint8_t>(HBU_NODE_SKETCH_REGISTERS);
        int rc = graph_work(g, nullptr, probe.used);
        if (rc) return rc;
        Carve carve{(char *)g->d_work};
        uint32_t *d_words = carve.take<uint32_t>(HBU_NODE_SKETCH_REGISTERS);
        uint8_t *d_bytes = carve.take<uint8_t>(HBU_NODE_SKETCH_REGISTERS);
        HBU_HIP(hipMemsetAsync(d_words, 0, HBU_NODE_SKETCH_REGISTERS * sizeof(uint32_t), nullptr));
        if (g->n_nodes) {
            hipLaunchKernelGGL(hbf::node_sketch_kernel, dim3(grid_capped(g->n_nodes)), dim3(256), 0, nullptr, (const hb_u128 *)g->d_nodes, g->n_nodes, d_words);
            HBU_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(hbf::sketch_narrow_kernel, dim3(HBU_NODE_SKETCH_REGISTERS / 256), dim3(256), 0, nullptr, (const uint32_t *)d_words, d_bytes);
        HBU_HIP(hipGetLastError());
        HBU_HIP(hipMemcpyAsync(registers_out, d_bytes, HBU_NODE_SKETCH_REGISTERS, hipMemcpyDeviceToHost, nullptr));
        HBU_HIP(hipStreamSynchronize(nullptr));
        return HB_OK;
    });
}

int hbu_filter_create(int32_t device, uint32_t kind, uint64_t num_bits, hbu_filter **out)
{
    return guarded(nullptr, [&]() -> int {
        if (!out) return refuse(HB_ERR_INVALID, "out == NULL");
        *out = nullptr;
        if (kind != HBU_FILTER_BLOOM && kind != HBU_FILTER_EXACT) return refuse(HB_ERR_INVALID, "unknown filter kind");
        if (kind == HBU_FILTER_BLOOM && num_bits == 0) return refuse(HB_ERR_INVALID, "a bloom filter needs at least one bit");
        if (kind == HBU_FILTER_BLOOM && num_bits > 0xFFFFFFFFull) return refuse(HB_ERR_LIMIT, "num_bits too large (< 2^32)");
        hbu_table *carrier = nullptr;
        int rc = create(device, HBU_KIND_F32, 0, 0, &carrier);
        if (rc) return rc;
        hbu_filter *f = new hbu_filter();
        f->device = carrier->device;
        f->kind = kind;
        f->t = carrier;
        if (kind == HBU_FILTER_BLOOM) {
            f->num_bits = num_bits;
            f->words = 2 * ((num_bits + 63) / 64);
            hipError_t e = hipMalloc((void **)&f->d_bits, f->words * sizeof(uint32_t));
            if (e == hipSuccess) e = hipMemsetAsync(f->d_bits, 0, f->words * sizeof(uint32_t), carrier->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(carrier->stream);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                hbu_filter_destroy(f);
                return refuse(e == hipErrorOutOfMemory ? HB_ERR_NOMEM : HB_ERR_HIP, std::string("bit vector: ") + hipGetErrorString(e));
            }
        }
        *out = f;
        return HB_OK;
    });
}

void hbu_filter_destroy(hbu_filter *f)
{
    if (!f) return;
    (void)hipSetDevice(f->device);
    if (f->t && f->t->stream) (void)hipStreamSynchronize(f->t->stream);
    if (f->d_bits) (void)hipFree(f->d_bits);
    hbu_destroy(f->t);
    delete f;
}

// every filter call: f given, not broken, on its device; the body runs with t = the carrier (HBU_HIP reports on it) and its text is
// copied to the thread's
#define HBU_FILTER_CALL(f, body)                                                       \
    return guarded(nullptr, [&]() -> int {                                             \
        if (!(f)) return refuse(HB_ERR_INVALID, "NULL argument");                      \
        hbu_table *t = (f)->t;                                                         \
        if (t->broken) return refuse(HB_ERR_INVALID, kBrokenMsg);                      \
        const int rc_ = [&]() -> int {                                                 \
            HBU_HIP(hipSetDevice(t->device));                                          \
            body                                                                       \
        }();                                                                           \
        return rc_ ? filter_fail((f), rc_) : HB_OK;                                    \
    })

int hbu_filter_clear(hbu_filter *f)
{
    HBU_FILTER_CALL(f, {
        if (f->kind == HBU_FILTER_BLOOM) {
            HBU_HIP(hipMemsetAsync(f->d_bits, 0, f->words * sizeof(uint32_t), t->stream));
            HBU_HIP(hipStreamSynchronize(t->stream));
            return HB_OK;
        }
        const int rc = rebuild_index(t, 1, 0); // an empty index of the smallest size, entry numbers from 0
        if (!rc) t->committed = 0;
        return rc;
    });
}

int hbu_filter_fill(hbu_filter *f)
{
    HBU_FILTER_CALL(f, {
        if (f->kind != HBU_FILTER_BLOOM) return fail(t, HB_ERR_INVALID, "fill() is a bloom filter's call");
        hipLaunchKernelGGL(hbr::bloom_fill_kernel, dim3(grid_capped(f->words)), dim3(256), 0, t->stream, f->d_bits, f->words, f->num_bits);
        HBU_HIP(hipGetLastError());
        HBU_HIP(hipStreamSynchronize(t->stream));
        return HB_OK;
    });
}

int hbu_filter_insert(hbu_filter *f, const hb_u128 *ids, uint64_t count)
{
    HBU_FILTER_CALL(f, {
        if (count && !ids) return fail(t, HB_ERR_INVALID, "NULL argument");
        if (count >= (1ull << 30)) return fail(t, HB_ERR_LIMIT, "batch too large (< 2^30 ids per call)");
        if (!count) return HB_OK;
        int rc;
        if ((rc = set_reserve(f, count))) return rc;
        Carve probe{nullptr};
        (void)probe.take<hb_u128>(count);
        if ((rc = work_memory(t, probe.used))) return rc;
        hb_u128 *d_ids = (hb_u128 *)t->d_work;
        HBU_HIP(hipMemcpyAsync(d_ids, ids, count * sizeof(hb_u128), hipMemcpyHostToDevice, t->stream));
        hipLaunchKernelGGL(hbr::filter_insert_kernel, dim3(grid_for(count)), dim3(256), 0, t->stream, (const hb_u128 *)d_ids, (uint32_t)count, filter_view(f));
        HBU_HIP(hipGetLastError());
        HBU_HIP(hipStreamSynchronize(t->stream));
        return set_commit(f, t->stream);
    });
}

int hbu_filter_contains(hbu_filter *f, const hb_u128 *ids, uint64_t count, uint8_t *out_bytes)
{
    HBU_FILTER_CALL(f, {
        if (count && (!ids || !out_bytes)) return fail(t, HB_ERR_INVALID, "NULL argument");
        if (count >= (1ull << 30)) return fail(t, HB_ERR_LIMIT, "batch too large (< 2^30 ids per call)");
        if (!count) return HB_OK;
        Carve probe{nullptr};
        (void)probe.take<hb_u128>(count);
        (void)probe.take<uint8_t>(count);
        int rc = work_memory(t, probe.used);
        if (rc) return rc;
        Carve carve{(char *)t->d_work};
        hb_u128 *d_ids = carve.take<hb_u128>(count);
        uint8_t *d_out = carve.take<uint8_t>(count);
        HBU_HIP(hipMemcpyAsync(d_ids, ids, count * sizeof(hb_u128), hipMemcpyHostToDevice, t->stream));
        hipLaunchKernelGGL(hbr::filter_contains_kernel, dim3(grid_for(count)), dim3(256), 0, t->stream, (const hb_u128 *)d_ids, (uint32_t)count, filter_view(f), d_out);
        HBU_HIP(hipGetLastError());
        HBU_HIP(hipMemcpyAsync(out_bytes, d_out, count, hipMemcpyDeviceToHost, t->stream));
        HBU_HIP(hipStreamSynchronize(t->stream));
        return HB_OK;
    });
}

int hbu_filter_union(hbu_filter *dst, hbu_filter *src)
{
    HBU_FILTER_CALL(dst, {
        if (!src) return fail(t, HB_ERR_INVALID, "NULL argument");
        if (src->kind != dst->kind || src->num_bits != dst->num_bits) return fail(t, HB_ERR_INVALID, "union needs two filters of one kind and size");
        if (src->device != dst->device) return fail(t, HB_ERR_INVALID, "the filters are not on one device");
        if (src->t->broken) return fail(t, HB_ERR_INVALID, kBrokenMsg);
        if (src == dst) return HB_OK;
        HBU_HIP(hipStreamSynchronize(src->t->stream));
        if (dst->kind == HBU_FILTER_BLOOM) {
            hipLaunchKernelGGL(hbr::bloom_or_kernel, dim3(grid_capped(dst->words)), dim3(256), 0, t->stream, dst->d_bits, (const uint32_t *)src->d_bits, dst->words);
            HBU_HIP(hipGetLastError());
            HBU_HIP(hipStreamSynchronize(t->stream));
            return HB_OK;
        }
        if (!src->t->committed) return HB_OK;
        int rc = set_reserve(dst, src->t->committed);
        if (rc) return rc;
        hipLaunchKernelGGL(hbr::set_union_kernel, dim3(grid_for(src->t->slots)), dim3(256), 0, t->stream, (const u128 *)src->t->d_keys, (const uint32_t *)src->t->d_pids,
                           src->t->slots, (uint32_t)src->t->committed, table_of(t));
        HBU_HIP(hipGetLastError());
        return set_commit(dst, t->stream);
    });
}

int hbu_filter_count(hbu_filter *f, uint64_t *n)
{
    HBU_FILTER_CALL(f, {
        if (!n) return fail(t, HB_ERR_INVALID, "NULL argument");
        if (f->kind == HBU_FILTER_EXACT) {
            *n = t->committed;
            return HB_OK;
        }
        unsigned long long *d_sum = t->d_next + 1; // (the second word of the index counter's allocation: a bloom filter has no index)
        HBU_HIP(hipMemsetAsync(d_sum, 0, sizeof(unsigned long long), t->stream));
        hipLaunchKernelGGL(hbr::bloom_popcount_kernel, dim3(grid_capped(f->words)), dim3(256), 0, t->stream, (const uint32_t *)f->d_bits, f->words, d_sum);
        HBU_HIP(hipGetLastError());
        HBU_HIP(hipMemcpyAsync(t->h_word, d_sum, sizeof(unsigned long long), hipMemcpyDeviceToHost, t->stream));
        HBU_HIP(hipStreamSynchronize(t->stream));
        *n = *t->h_word;
        return HB_OK;
    });
}

int hbu_filter_export_bits(hbu_filter *f, uint64_t *words_out)
{
    HBU_FILTER_CALL(f, {
        if (f->kind != HBU_FILTER_BLOOM) return fail(t, HB_ERR_INVALID, "only a bloom filter has bits");
        if (!words_out) return fail(t, HB_ERR_INVALID, "NULL argument");
        HBU_HIP(hipMemcpyAsync(words_out, f->d_bits, f->words * sizeof(uint32_t), hipMemcpyDeviceToHost, t->stream));
        HBU_HIP(hipStreamSynchronize(t->stream));
        return HB_OK;
    });
}

int hbu_filter_import_bits(hbu_filter *f, const uint64_t *words)
{
    HBU_FILTER_CALL(f, {
        if (f->kind != HBU_FILTER_BLOOM) return fail(t, HB_ERR_INVALID, "only a bloom filter has bits");
        if (!words) return fail(t, HB_ERR_INVALID, "NULL argument");
        const uint64_t tail = f->num_bits % 64;
        if (tail && (words[f->words / 2 - 1] >> tail) != 0) return fail(t, HB_ERR_INVALID, "bits above num_bits are set in the last word");
        HBU_HIP(hipMemcpyAsync(f->d_bits, words, f->words * sizeof(uint32_t), hipMemcpyHostToDevice, t->stream));
        HBU_HIP(hipStreamSynchronize(t->stream));
        return HB_OK;
    });
}

int hbu_filter_export_ids(hbu_filter *f, hb_u128 *out, uint64_t capacity, uint64_t *written)
{
    HBU_FILTER_CALL(f, {
        if (written) *written = 0;
        if (f->kind != HBU_FILTER_EXACT) return fail(t, HB_ERR_INVALID, "only an exact filter has ids");
        if (!written || (t->committed && !out)) return fail(t, HB_ERR_INVALID, "NULL argument");
        if (capacity < t->committed) return fail(t, HB_ERR_INVALID, "capacity below the number of ids");
        if (!t->committed) return HB_OK;
        Carve probe{nullptr};
        (void)probe.take<hb_u128>(t->committed);
        int rc = work_memory(t, probe.used);
        if (rc) return rc;
        hb_u128 *d_out = (hb_u128 *)t->d_work;
        hipLaunchKernelGGL(hbr::set_export_kernel, dim3(grid_for(t->slots)), dim3(256), 0, t->stream, (const u128 *)t->d_keys, (const uint32_t *)t->d_pids, t->slots,
                           (uint32_t)t->committed, d_out);
        HBU_HIP(hipGetLastError());
        HBU_HIP(hipMemcpyAsync(out, d_out, t->committed * sizeof(hb_u128), hipMemcpyDeviceToHost, t->stream));
        HBU_HIP(hipStreamSynchronize(t->stream));
        *written = t->committed;
        return HB_OK;
    });
}
#undef HBU_FILTER_CALL

int hbu_setup_counters(hbu_table *prev_counters, hbu_table *next_counters, const hbu_graph *g, hbu_filter *changed)
{
    hbu_table *t = next_counters;
    return guarded(t, [&]() -> int {
        int rc = round_refusal({prev_counters}, t, g, changed, nullptr, false);
        if (rc) return rc;
        if (prev_counters->kind != HBU_KIND_HLL64 || t->kind != HBU_KIND_HLL64) return fail(t, HB_ERR_INVALID, "setup_counters needs two HyperLogLog<64> tables");
        if (!g->n_nodes) return HB_OK;
        HBU_HIP(hipSetDevice(t->device));
        const uint64_t chunk = std::min<uint64_t>(std::min<uint64_t>(g->chunk, kSetupChunk), g->n_nodes);
        Carve probe{nullptr};
        (void)probe.take<uint4>(chunk * 4);
        if ((rc = graph_work(g, t, probe.used))) return rc;
        uint4 *d_vals = (uint4 *)g->d_work;
        if (changed) HBU_HIP(hipStreamSynchronize(changed->t->stream));
        for (uint64_t b = 0; b < g->n_nodes; b += chunk) {
            const uint64_t n = std::min<uint64_t>(chunk, g->n_nodes - b);
            const hb_u128 *nodes = g->d_nodes + b;
            hipLaunchKernelGGL(hbr::setup_values_kernel, dim3((unsigned)((n * 4 + 255) / 256)), dim3(256), 0, t->stream, nodes, (uint32_t)n, d_vals);
            HBU_HIP(hipGetLastError());
            HBU_HIP(hipStreamSynchronize(t->stream));
            if ((rc = apply(prev_counters, kOpSet, Pairs{nodes, d_vals, true}, n, nullptr))) return fail(t, rc, prev_counters->err);
            if ((rc = apply(t, kOpSet, Pairs{nodes, d_vals, true}, n, nullptr))) return rc;
            if (changed) {
                if ((rc = set_reserve(changed, n))) return fail(t, rc, changed->t->err);
                hipLaunchKernelGGL(hbr::filter_insert_kernel, dim3(grid_for(n)), dim3(256), 0, t->stream, nodes, (uint32_t)n, filter_view(changed));
                HBU_HIP(hipGetLastError());
                HBU_HIP(hipStreamSynchronize(t->stream));
                if ((rc = set_commit(changed, t->stream))) return fail(t, rc, changed->t->err);
            }
        }
        return HB_OK;
    });
}

int hbu_round_counters(hbu_table *prev_counters, hbu_table *next_counters, const hbu_graph *g, hbu_filter *changed, hbu_filter *new_changed, uint64_t *selected,
                       uint64_t *merged, uint64_t *inserted)
{
    hbu_table *t = next_counters;
    return guarded(t, [&]() -> int {
        for (uint64_t *p : {selected, merged, inserted})
            if (p) *p = 0;
        int rc = round_refusal({prev_counters}, t, g, changed, new_changed, true);
        if (rc) return rc;
        if (prev_counters->kind != HBU_KIND_HLL64 || t->kind != HBU_KIND_HLL64) return fail(t, HB_ERR_INVALID, "round_counters needs two HyperLogLog<64> tables");
        if (!g->n_edges) return HB_OK;
        HBU_HIP(hipSetDevice(t->device));
        uint64_t c[4] = {0, 0, 0, 0};
        rc = round_edges<kRoundCounters>(prev_counters, t, g, changed, new_changed, c);
        if (selected) *selected = c[0];
        if (merged) *merged = c[1];
        if (inserted) *inserted = c[2];
        return rc;
    });
}

int hbu_round_distances(hbu_table *prev_distances, hbu_table *next_distances, const hbu_graph *g, hbu_filter *changed, hbu_filter *new_changed, uint64_t *selected,
                        uint64_t *changed_nodes)
{
    hbu_table *t = next_distances;
    return guarded(t, [&]() -> int {
        for (uint64_t *p : {selected, changed_nodes})
            if (p) *p = 0;
        int rc = round_refusal({prev_distances}, t, g, changed, new_changed, true);
        if (rc) return rc;
        if (prev_distances->kind != HBU_KIND_U64 || t->kind != HBU_KIND_U64) return fail(t, HB_ERR_INVALID, "round_distances needs two u64 tables");
        if (!g->n_edges) return HB_OK;
        HBU_HIP(hipSetDevice(t->device));
        uint64_t c[4] = {0, 0, 0, 0};
        rc = round_edges<kRoundDistances>(prev_distances, t, g, changed, new_changed, c);
        if (selected) *selected = c[0];
        if (changed_nodes) *changed_nodes = c[1] + c[2];
        return rc;
    });
}

int hbu_round_lane_distances(hbu_table *prev, hbu_table *next, const hbu_graph *g, hbu_filter *changed, hbu_filter *new_changed, uint64_t *selected, uint64_t *merged,
                             uint64_t *inserted)
{
    hbu_table *t = next;
    return guarded(t, [&]() -> int {
        for (uint64_t *p : {selected, merged, inserted})
            if (p) *p = 0;
        int rc = round_refusal({prev}, t, g, changed, new_changed, true);
        if (rc) return rc;
        if (prev->kind != HBU_KIND_DIST64 || t->kind != HBU_KIND_DIST64) return fail(t, HB_ERR_INVALID, "round_lane_distances needs two 64-lane distance tables");
        if (!g->n_edges) return HB_OK;
        HBU_HIP(hipSetDevice(t->device));
        uint64_t c[4] = {0, 0, 0, 0};
        rc = round_edges<kRoundLanes>(prev, t, g, changed, new_changed, c);
        if (selected) *selected = c[0];
        if (merged) *merged = c[1];
        if (inserted) *inserted = c[2];
        return rc;
    });
}

int hbu_round_centralities(hbu_table *prev_counters, hbu_table *next_counters, hbu_table *prev_centrality, hbu_table *next_centrality, const hbu_graph *g,
                           hbu_filter *changed, uint64_t round, uint64_t *selected, uint64_t *written)
{
    hbu_table *t = next_centrality;
    return guarded(t, [&]() -> int {
        for (uint64_t *p : {selected, written})
            if (p) *p = 0;
        int rc = round_refusal({prev_counters, next_counters, prev_centrality}, t, g, changed, nullptr, true);
        if (rc) return rc;
        if (prev_counters->kind != HBU_KIND_HLL64 || next_counters->kind != HBU_KIND_HLL64 || prev_centrality->kind != HBU_KIND_KAHAN || t->kind != HBU_KIND_KAHAN)
            return fail(t, HB_ERR_INVALID, "round_centralities needs two HyperLogLog<64> tables and two KahanSum tables");
        if (!g->n_nodes) return HB_OK;
        HBU_HIP(hipSetDevice(t->device));
        const uint64_t chunk = std::min<uint64_t>(g->chunk, g->n_nodes);
        size_t tmp_bytes = 0;
        HBU_HIP(rocprim::select(nullptr, tmp_bytes, (const hb_u128 *)nullptr, (const uint8_t *)nullptr, (hb_u128 *)nullptr, (uint32_t *)nullptr, (size_t)chunk, t->stream));
        uint8_t *d_flag;
        hb_u128 *d_sel;
        uint32_t *d_n;
        char *d_tmp;
        auto layout = [&](Carve &c) {
            d_flag = c.take<uint8_t>(chunk);
            d_sel = c.take<hb_u128>(chunk);
            d_n = c.take<uint32_t>(2);
            d_tmp = c.take<char>(tmp_bytes);
        };
        Carve probe{nullptr};
        layout(probe);
        if ((rc = graph_work(g, t, probe.used))) return rc;
        Carve carve{(char *)g->d_work};
        layout(carve);
        HBU_HIP(hipStreamSynchronize(changed->t->stream));
        const hbr::Filter in = filter_view(changed);
        uint64_t sel_total = 0, written_total = 0;
        for (uint64_t b = 0; b < g->n_nodes; b += chunk) {
            const uint64_t n = std::min<uint64_t>(chunk, g->n_nodes - b);
            hipLaunchKernelGGL(hbr::select_nodes_kernel, dim3(grid_for(n)), dim3(256), 0, t->stream, (const hb_u128 *)(g->d_nodes + b), (uint32_t)n, in, d_flag);
            HBU_HIP(hipGetLastError());
            size_t tb = tmp_bytes;
            HBU_HIP(rocprim::select(d_tmp, tb, (const hb_u128 *)(g->d_nodes + b), (const uint8_t *)d_flag, d_sel, d_n, (size_t)n, t->stream));
            *t->h_word = 0;
            HBU_HIP(hipMemcpyAsync(t->h_word, d_n, sizeof(uint32_t), hipMemcpyDeviceToHost, t->stream));
            HBU_HIP(hipStreamSynchronize(t->stream));
            const uint64_t picked = *t->h_word;
            sel_total += picked;
            if (selected) *selected = sel_total;
            if (!picked) continue;
            uint64_t w = 0;
            if ((rc = centralities_step(prev_counters, next_counters, prev_centrality, t, d_sel, true, picked, round, &w))) return rc;
            written_total += w;
            if (written) *written = written_total;
        }
        return HB_OK;
    });
}

} // extern "C"

// ---- the finish of a job: values, ranks, top nodes, store ---------------------------------------------------------------------------
namespace {
// temporaries of one finish call (the caching allocator's: they go back to it when the call returns)
struct Temps {
    std::vector<void *> ptrs;
    ~Temps()
    {
        for (void *p : ptrs)
            if (p) (void)hipFree(p);
    }
    template <class T>
    hipError_t alloc(T **out, uint64_t count)
    {
        void *p = nullptr;
        const hipError_t e = hipMalloc(&p, std::max<size_t>((size_t)count * sizeof(T), 256));
        if (e == hipSuccess) ptrs.push_back(p);
        *out = (T *)p;
        return e;
    }
    void release(void *p)
    {
        for (void *&q : ptrs)
            if (q == p && p) {
                (void)hipFree(p);
                q = nullptr;
            }
    }
};
// the entries of a centrality table in ascending-NodeID order, on the device: ids, quotients, the rank order and (if asked for) the ranks
struct Finished {
    hb_u128 *d_ids = nullptr;
    double *d_vals = nullptr;
    uint64_t *d_order = nullptr; // d_order[i] = the entry at position i of (value descending under total_cmp, NodeID ascending)
    uint64_t *d_rank = nullptr;
};

int finish_refusal(hbu_table *t)
{
    if (!t) return fail(t, HB_ERR_INVALID, "NULL table");
    if (t->kind != HBU_KIND_KAHAN && t->kind != HBU_KIND_F64) return fail(t, HB_ERR_INVALID, "a centrality table is a KahanSum or an f64 table");
    if (t->broken) return fail(t, HB_ERR_INVALID, kBrokenMsg);
    return HB_OK;
}
int sort_error(hbu_table *t, const std::string &e)
{
    (void)hipGetLastError();
    return fail(t, e.find("memory") != std::string::npos ? HB_ERR_NOMEM : HB_ERR_HIP, e);
}

// keys by entry number -> one 128-bit sort carrying the entry number -> quotient and sort key of every entry in that order -> a stable
// 64-bit sort of the sort keys -> the scatter of the ranks.  The table is only read.  n = t->committed > 0.
int finish_on_device(hbu_table *t, double divisor, bool want_ranks, Temps &m, Finished *f)
{
    const uint64_t n = t->committed;
    hb_u128 *d_raw = nullptr;
    uint32_t *d_entry = nullptr;
    uint64_t *d_key = nullptr;
    HBU_HIP(m.alloc(&d_raw, n));
    HBU_HIP(m.alloc(&f->d_ids, n));
    HBU_HIP(m.alloc(&d_entry, n));
    hipLaunchKernelGGL(hbr::set_export_kernel, dim3(grid_for(t->slots)), dim3(256), 0, t->stream, (const u128 *)t->d_keys, (const uint32_t *)t->d_pids, t->slots, (uint32_t)n,
                       d_raw);
    HBU_HIP(hipGetLastError());
    std::string e = hb::gpu_sort_ids_device((void *)t->stream, d_raw, n, f->d_ids, d_entry);
    if (!e.empty()) return sort_error(t, e);
    m.release(d_raw);
    HBU_HIP(m.alloc(&f->d_vals, n));
    HBU_HIP(m.alloc(&d_key, n));
    if (t->kind == HBU_KIND_KAHAN)
        hipLaunchKernelGGL(hbn::finish_values_kernel<2>, dim3(grid_for(n)), dim3(256), 0, t->stream, (const double *)t->d_table, (const uint32_t *)d_entry, n, divisor, f->d_vals,
                           d_key);
    else
        hipLaunchKernelGGL(hbn::finish_values_kernel<1>, dim3(grid_for(n)), dim3(256), 0, t->stream, (const double *)t->d_table, (const uint32_t *)d_entry, n, divisor, f->d_vals,
                           d_key);
    HBU_HIP(hipGetLastError());
    HBU_HIP(m.alloc(&f->d_order, n));
    if (want_ranks) HBU_HIP(m.alloc(&f->d_rank, n));
    e = hb::gpu_rank_keys_device((void *)t->stream, d_key, n, f->d_order, f->d_rank);
    if (!e.empty()) return sort_error(t, e);
    m.release(d_key);
    m.release(d_entry);
    return HB_OK;
}
} // namespace

extern "C" {

int hbu_finish_centralities(hbu_table *centrality, double divisor, hb_u128 *ids_out, double *vals_out, uint64_t *ranks_out, uint64_t capacity, uint64_t *written)
{
    hbu_table *t = centrality;
    return guarded(t, [&]() -> int {
        if (written) *written = 0;
        int rc = finish_refusal(t);
        if (rc) return rc;
        const uint64_t n = t->committed;
        const bool any = ids_out || vals_out || ranks_out;
        if (any && capacity < n) return fail(t, HB_ERR_INVALID, "capacity below the number of keys");
        if (written) *written = n;
        if (!n || !any) return HB_OK;
        HBU_HIP(hipSetDevice(t->device));
        Temps m;
        Finished f;
        if ((rc = finish_on_device(t, divisor, ranks_out != nullptr, m, &f))) {
            if (written) *written = 0;
            return rc;
        }
        if (ids_out) HBU_HIP(hipMemcpyAsync(ids_out, f.d_ids, n * sizeof(hb_u128), hipMemcpyDeviceToHost, t->stream));
        if (vals_out) HBU_HIP(hipMemcpyAsync(vals_out, f.d_vals, n * sizeof(double), hipMemcpyDeviceToHost, t->stream));
        if (ranks_out) HBU_HIP(hipMemcpyAsync(ranks_out, f.d_rank, n * sizeof(uint64_t), hipMemcpyDeviceToHost, t->stream));
        HBU_HIP(hipStreamSynchronize(t->stream));
        return HB_OK;
    });
}

int hbu_top_centralities(hbu_table *centrality, double divisor, uint64_t k, hb_u128 *ids_out, double *vals_out, uint64_t *written)
{
    hbu_table *t = centrality;
    return guarded(t, [&]() -> int {
        if (written) *written = 0;
        int rc = finish_refusal(t);
        if (rc) return rc;
        const uint64_t top = std::min<uint64_t>(k, t->committed);
        if (written) *written = top;
        if (!top || (!ids_out && !vals_out)) return HB_OK;
        HBU_HIP(hipSetDevice(t->device));
        Temps m;
        Finished f;
        if ((rc = finish_on_device(t, divisor, false, m, &f))) {
            if (written) *written = 0;
            return rc;
        }
        hb_u128 *d_top_ids = nullptr;
        double *d_top_vals = nullptr;
        if (ids_out) HBU_HIP(m.alloc(&d_top_ids, top));
        if (vals_out) HBU_HIP(m.alloc(&d_top_vals, top));
        hipLaunchKernelGGL(hbn::top_gather_kernel, dim3(grid_for(top)), dim3(256), 0, t->stream, (const uint64_t *)f.d_order, top, (const hb_u128 *)f.d_ids,
                           (const double *)f.d_vals, d_top_ids, d_top_vals);
        HBU_HIP(hipGetLastError());
        if (ids_out) HBU_HIP(hipMemcpyAsync(ids_out, d_top_ids, top * sizeof(hb_u128), hipMemcpyDeviceToHost, t->stream));
        if (vals_out) HBU_HIP(hipMemcpyAsync(vals_out, d_top_vals, top * sizeof(double), hipMemcpyDeviceToHost, t->stream));
        HBU_HIP(hipStreamSynchronize(t->stream));
        return HB_OK;
    });
}

int hbu_store_centralities(hbu_table *centrality, double divisor, const char *output, char *err, uint64_t err_len)
{
    hbu_table *t = centrality;
    if (err && err_len) err[0] = 0;
    const int rc = guarded(t, [&]() -> int {
        int rc2 = finish_refusal(t);
        if (rc2) return rc2;
        if (!output || !*output) return fail(t, HB_ERR_INVALID, "hbu_store_centralities: output is empty");
        const uint64_t n = t->committed;
        // what crosses the link: the values, the ranks and the key order of the two databases - the ids stay where they are
        hb::RawVec<double> vals(n);
        hb::RawVec<uint64_t> ranks(n);
        hb::StoreKeyVec sorted(n);
        if (n) {
            HBU_HIP(hipSetDevice(t->device));
            Temps m;
            Finished f;
            if ((rc2 = finish_on_device(t, divisor, true, m, &f))) return rc2;
            HBU_HIP(hipMemcpyAsync(vals.data(), f.d_vals, n * sizeof(double), hipMemcpyDeviceToHost, t->stream));
            HBU_HIP(hipMemcpyAsync(ranks.data(), f.d_rank, n * sizeof(uint64_t), hipMemcpyDeviceToHost, t->stream));
            HBU_HIP(hipStreamSynchronize(t->stream));
            m.release(f.d_vals);
            m.release(f.d_rank);
            m.release(f.d_order);
            const std::string e = hb::gpu_store_keys_device((void *)t->stream, f.d_ids, n, sorted.data());
            if (!e.empty()) return sort_error(t, "hbu_store_centralities: " + e);
        }
        char msg[512] = {0};
        const int rc3 = hb::store_harmonic_presorted(output, &sorted, vals.data(), ranks.data(), msg, sizeof(msg));
        if (rc3) return fail(t, rc3, msg);
        return HB_OK;
    });
    if (rc && err && err_len) std::snprintf(err, (size_t)err_len, "%s", hbu_last_error(t));
    return rc;
}

} // extern "C"
