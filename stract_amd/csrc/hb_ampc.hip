// hb_ampc.hip - GPU-resident shard of the AMPC tables (include/hb_ampc.h cites the reference operations this serves).  One translation
// unit in four host files; the kernels sit in the hb_ampc_*.hip.h headers:
//   hb_ampc.hip         the table itself: the HyperLogLog<64> counter table with HyperLogLog64Upsert semantics and the scalar value tables
//                       with the five scalar upsert operators - its buffers and their owners (hb_owned.h), the key index, the workspace
//                       step, the transaction, apply / get, create / clone / export (hb_ampc_values.hip.h, hb_ampc_lanes.hip.h: the 64-lane rows)
//   hb_ampc_steps.inc   the fold of a distance table into the centrality table, update_centralities, the two edge steps update_counters /
//                       update_distances (hb_ampc_fold.hip.h, hb_ampc_edges.hip.h)
//   hb_ampc_round.inc   a worker's resident graph and changed-node filter, and the mapper steps that work between them and the tables
//                       (hb_ampc_round.hip.h)
//   hb_ampc_finish.inc  the finish of both jobs: a centrality table's values, ranks, top nodes and store (hb_ampc_finish.hip.h, the sorts
//                       are hb_ingest.hip's)
// DESIGN.md section 26 ("Who owns what in the AMPC shard") has the rules a new entry point follows.
#include "hb_guard_alloc.h" // FIRST: no-op unless built with -DHB_GUARD_ALLOC=<mode> (debug allocators: guard pages / poison / red zones)
#include "hb_pool.h"        // then: every hipMalloc / hipFree below goes through the caching device allocator (shipped build)
#include "hb_owned.h"       // after hb_pool.h: the holders free through the allocator this file sees
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
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

namespace {
struct Carve { // consecutive 256-byte aligned pieces of a work buffer
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
// work memory of one batch or chunk, kept between calls (a mapper sends thousands of equally sized batches): it only ever grows
struct WorkBuf {
    const char *oom; // the error text of a failed grow
    DevPtr<char> p;
    size_t bytes = 0;
    bool grow(size_t need)
    {
        if (need <= bytes) return true;
        bytes = 0;
        if (p.alloc(need) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        bytes = need;
        return true;
    }
};
// (hbu_destroy & co. set the device and wait for the stream before they delete)
struct Destroy {
    void operator()(hbu_table *t) const { hbu_destroy(t); }
    void operator()(hbu_graph *g) const { hbu_graph_destroy(g); }
    void operator()(hbu_filter *f) const { hbu_filter_destroy(f); }
};
template <class T>
using Owned = std::unique_ptr<T, Destroy>;
} // namespace

struct hbu_table {
    int device = 0;
    // Members die in reverse order of declaration, and here that order matters: the device buffers first, then the pinned words, the
    // stream last.  A new buffer goes below h_word.
    StreamHolder stream;
    PinnedPtr<unsigned long long> h_word; // pinned: read-backs of the counter / the group count
    WorkBuf work{"hipMalloc(batch work memory) failed"};
    DevPtr<unsigned long long> d_next; // slot ids handed out so far (device counter of the index)
    // key index (device): open-addressing table of `slots` entries, load factor <= 1/2
    DevPtr<u128> d_keys;
    DevPtr<uint32_t> d_pids;
    uint64_t slots = 0;
    uint64_t committed = 0; // keys visible to the caller (= d_next outside a failed batch)
    bool broken = false;    // a failed batch could not be undone: every further call is refused
    uint32_t kind = HBU_KIND_HLL64;
    uint32_t vbytes = 64; // bytes of one value of that kind
    DevPtr<char> d_table; // cap x vbytes, value of slot s at s * vbytes
    uint64_t cap = 0;     // values allocated
    std::string err;
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
Table table_of(const hbu_table *t) { return Table{t->d_keys.get(), t->d_pids.get(), t->slots - 1, t->d_next.get()}; }

// values for `need` keys
int reserve(hbu_table *t, uint64_t need)
{
    if (need <= t->cap) return HB_OK;
    const uint64_t cap = std::max<uint64_t>(need, std::max<uint64_t>(2 * t->cap, 1024));
    DevPtr<char> n;
    if (n.alloc(cap * t->vbytes) != hipSuccess) return fail(t, HB_ERR_NOMEM, "hipMalloc(value table) failed");
    hipError_t e = hipMemsetAsync(n.get(), 0, cap * t->vbytes, t->stream);
    if (e == hipSuccess && t->cap) e = hipMemcpyAsync(n.get(), t->d_table.get(), t->cap * t->vbytes, hipMemcpyDeviceToDevice, t->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
    if (e != hipSuccess) return fail(t, HB_ERR_HIP, hipGetErrorString(e));
    t->d_table = std::move(n);
    t->cap = cap;
    return HB_OK;
}

// a key index with room for `keys` keys at load factor <= 1/2, holding the entries with ids < keep of the present one
int rebuild_index(hbu_table *t, uint64_t keys, uint64_t keep)
{
    uint64_t slots = 1024;
    while (slots < 2 * keys) slots <<= 1;
    DevPtr<u128> nk;
    DevPtr<uint32_t> np;
    if (nk.alloc(slots) != hipSuccess || np.alloc(slots) != hipSuccess) {
        (void)hipGetLastError();
        return fail(t, HB_ERR_NOMEM, "hipMalloc(key index) failed");
    }
    hipLaunchKernelGGL(table_clear_kernel, dim3(grid_for(slots)), dim3(256), 0, t->stream, np.get(), slots);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && t->slots && keep) {
        const Table nt{nk.get(), np.get(), slots - 1, t->d_next.get()};
        hipLaunchKernelGGL(rehash_kernel, dim3(grid_for(t->slots)), dim3(256), 0, t->stream, (const u128 *)t->d_keys.get(), (const uint32_t *)t->d_pids.get(), t->slots,
                           (uint32_t)keep, nt);
        e = hipGetLastError();
    }
    const unsigned long long next = keep;
    if (e == hipSuccess) e = hipMemcpyAsync(t->d_next.get(), &next, sizeof(next), hipMemcpyHostToDevice, t->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
    if (e != hipSuccess) return fail(t, HB_ERR_HIP, hipGetErrorString(e));
    t->d_keys = std::move(nk);
    t->d_pids = std::move(np);
    t->slots = slots;
    return HB_OK;
}

// The one workspace step of every entry point: `layout` names its pieces ONCE, as takes from the Carve it is given.  It runs on a
// null-based Carve to size the buffer, the buffer grows, and the same callable runs again on the real base - so the sizes and the
// pointers cannot disagree.  Errors are reported on `t` (NULL: the thread's text).
template <class L>
int workspace(WorkBuf &w, hbu_table *t, L &&layout)
{
    Carve probe{nullptr};
    layout(probe);
    if (!w.grow(probe.used)) return fail(t, HB_ERR_NOMEM, w.oom);
    Carve carve{w.p.get()};
    layout(carve);
    return HB_OK;
}

// ---- the transaction of a call that may put new keys into the index --------------------------------------------------------------------
//   ensure_room   everything that can fail for lack of memory comes BEFORE the index changes (the index never grows inside a launch)
//   run           from there on a failure is a HIP error; the run ends with queue_committed + a synchronise
//   rollback      on such an error the keys the call may have put into the index are taken out again before the error is returned
//   commit        otherwise the caller sees them
const char *const kTableLimit = "too many keys in one table (< 2^32)";
// room for `more` new keys (every pair might bring one), and for their values if the table stores any
int ensure_room(hbu_table *t, uint64_t more, bool with_values, const char *limit_msg = kTableLimit)
{
    const uint64_t keys = t->committed + more;
    if (keys >= 0xFFFFFFFEull) return fail(t, HB_ERR_LIMIT, limit_msg);
    int rc;
    // (slots = the power of two >= 2 x keys: the rounding is what makes repeated growth geometric)
    if (2 * keys > t->slots && (rc = rebuild_index(t, keys, t->committed))) return rc;
    return with_values ? reserve(t, keys) : HB_OK;
}
// the index is rebuilt from the entries below `committed`; if even that fails the table is unusable
int rollback(hbu_table *t, hipError_t e)
{
    const std::string why = hipGetErrorString(e);
    (void)hipGetLastError();
    if (rebuild_index(t, std::max<uint64_t>(t->slots / 2, 512), t->committed)) t->broken = true;
    return fail(t, e == hipErrorOutOfMemory ? HB_ERR_NOMEM : HB_ERR_HIP, why);
}
// the index counter on its way to h_word[0]; `stream`: the one the inserting kernel ran on
hipError_t queue_committed(hbu_table *t, hipStream_t stream)
{
    return hipMemcpyAsync(t->h_word.get(), t->d_next.get(), sizeof(unsigned long long), hipMemcpyDeviceToHost, stream);
}
void commit(hbu_table *t) { t->committed = t->h_word[0]; } // (after the synchronise that follows queue_committed)

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
    int rc;
    if ((rc = ensure_room(t, count, true))) return rc;
    size_t sort_bytes = 0, select_bytes = 0;
    const uint32_t n32 = (uint32_t)count;
    {
        uint32_t *nul = nullptr;
        auto iota = rocprim::make_counting_iterator<uint32_t>(0);
        HBU_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, (const uint32_t *)nul, nul, iota, nul, (size_t)count, 0, 32, t->stream));
        auto flags = rocprim::make_transform_iterator(iota, HeadFlag{nul});
        HBU_HIP(rocprim::select(nullptr, select_bytes, iota, flags, nul, nul, (size_t)count, t->stream.get()));
    }
    const size_t tmp_bytes = std::max(sort_bytes, select_bytes);
    const uint64_t staged = in.on_device ? 0 : count; // pairs that need room in the work memory
    const uint64_t grouped = (per_group || (sink && sink->per_group)) ? count : 0; // (key, action) of every group
    hb_u128 *d_k, *d_gkeys;
    char *d_v, *d_tmp;
    uint32_t *d_slot, *d_slot_s, *d_perm, *d_heads, *d_groups;
    uint8_t *d_act, *d_gact;
    rc = workspace(t->work, t, [&](Carve &c) {
        d_k = c.take<hb_u128>(staged);
        d_v = c.take<char>(staged * t->vbytes);
        d_slot = c.take<uint32_t>(count);
        d_slot_s = c.take<uint32_t>(count);
        d_perm = c.take<uint32_t>(count);
        d_heads = c.take<uint32_t>(count);
        d_groups = c.take<uint32_t>(2);
        d_act = c.take<uint8_t>(count);
        d_tmp = c.take<char>(tmp_bytes);
        d_gkeys = c.take<hb_u128>(grouped);
        d_gact = c.take<uint8_t>(grouped);
    });
    if (rc) return rc;
    const hb_u128 *keys_d = in.on_device ? in.keys : d_k;
    const void *vals_d = in.on_device ? in.values : d_v;
    const uint32_t first_new = (uint32_t)t->committed;
    const uint32_t *ss = d_slot_s, *hd = d_heads, *gr = d_groups, *pm = d_perm; // what every group kernel reads
    auto launch_values = [&]() {
        const dim3 grid((unsigned)std::min<uint64_t>((count + 255) / 256, 1u << 16)), block(256);
#define HBU_SET(RAW) hipLaunchKernelGGL(hbv::group_set_kernel<RAW>, grid, block, 0, t->stream, (RAW *)t->d_table.get(), ss, hd, gr, n32, pm, (const RAW *)vals_d)
#define HBU_UPSERT(OP) \
    hipLaunchKernelGGL(hbv::group_apply_kernel<hbv::OP>, grid, block, 0, t->stream, (hbv::OP::V *)t->d_table.get(), ss, hd, gr, n32, first_new, pm, (const hbv::OP::V *)vals_d, d_act)
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
        if ((e = rocprim::select(d_tmp, b, iota, flags, d_heads, d_groups, (size_t)count, t->stream.get())) != hipSuccess) return e;
        const unsigned blocks = (unsigned)std::min<uint64_t>((count + 63) / 64, 1u << 16);
        // the 64-byte group kernels: one quad per group; they differ in where a pair's value comes from (the arguments between perm and the actions)
#define HBU_GROUPS64(KERNEL, ...) \
    hipLaunchKernelGGL(KERNEL, dim3(blocks), dim3(256), 0, t->stream, (uint4 *)t->d_table.get(), ss, hd, gr, n32, first_new, pm, __VA_ARGS__, d_act)
        if (t->vbytes != 64) launch_values();
        else if (t->kind == HBU_KIND_DIST64 && in.lanes) HBU_GROUPS64(hbl::upsert_lanes_kernel<true>, (const uint4 *)nullptr, *in.lanes);
        else if (t->kind == HBU_KIND_DIST64 && upsert) HBU_GROUPS64(hbl::upsert_lanes_kernel<false>, (const uint4 *)vals_d, hbl::LaneSource{nullptr, nullptr});
        else if (in.gather) HBU_GROUPS64(hbe::upsert_edges_kernel, *in.gather);
        else if (upsert) HBU_GROUPS64(upsert_kernel<0>, (const uint4 *)vals_d);
        else HBU_GROUPS64(upsert_kernel<1>, (const uint4 *)vals_d);
#undef HBU_GROUPS64
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if (per_group || (sink && sink->per_group)) {
            hipLaunchKernelGGL(hbe::group_actions_kernel, dim3(grid_for(count)), dim3(256), 0, t->stream, hd, gr, n32, pm, keys_d, (const uint8_t *)d_act, d_gkeys, d_gact);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        } else if (upsert && !sink && (e = hipMemcpyAsync(actions, d_act, count, hipMemcpyDeviceToHost, t->stream)) != hipSuccess) {
            return e;
        }
        if (sink && (e = sink->per_group ? sink->note(d_gkeys, d_gact, d_groups) : sink->note(keys_d, d_act, nullptr)) != hipSuccess) return e;
        if ((e = queue_committed(t, t->stream)) != hipSuccess) return e;
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
    if (e != hipSuccess) return rollback(t, e);
    commit(t);
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
    hb_u128 *d_k;
    uint32_t *d_slots;
    char *d_out;
    uint8_t *d_found;
    const int rc = workspace(t->work, t, [&](Carve &c) {
        d_k = c.take<hb_u128>(count);
        d_slots = c.take<uint32_t>(count);
        d_out = c.take<char>(count * t->vbytes);
        d_found = c.take<uint8_t>(count);
    });
    if (rc) return rc;
    HBU_HIP(hipMemcpyAsync(d_k, keys, count * sizeof(hb_u128), hipMemcpyHostToDevice, t->stream));
    hipLaunchKernelGGL(slots_find_kernel, dim3(grid_for(count)), dim3(256), 0, t->stream, (const hb_u128 *)d_k, (uint32_t)count, table_of(t),
                       (uint32_t)t->committed, d_slots, d_found);
#define HBU_GET(RAW) \
    hipLaunchKernelGGL(hbv::get_values_kernel<RAW>, dim3(grid_for(count)), dim3(256), 0, t->stream, (const RAW *)t->d_table.get(), (const uint32_t *)d_slots, (uint32_t)count, (RAW *)d_out)
    if (t->kind == HBU_KIND_DIST64)
        hipLaunchKernelGGL(hbl::get_lanes_kernel, dim3((unsigned)((count * 4 + 255) / 256)), dim3(256), 0, t->stream, (const uint4 *)t->d_table.get(), (const uint32_t *)d_slots,
                           (uint32_t)count, (uint4 *)d_out);
    else if (t->vbytes == 64)
        hipLaunchKernelGGL(get_kernel, dim3((unsigned)((count * 4 + 255) / 256)), dim3(256), 0, t->stream, (const uint4 *)t->d_table.get(), (const uint32_t *)d_slots,
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

// the device of a new table or graph (device < 0: the current one); refusals go to the thread's error text
int pick_device(int32_t device, int *out)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, HB_ERR_NO_DEVICE, "no HIP device visible: this library has no CPU fallback");
    int dev = device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = 0;
    if (dev >= ndev) return fail(nullptr, HB_ERR_INVALID, "device ordinal out of range");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess || std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, HB_ERR_NO_DEVICE, "kernels are built for gfx950 only");
    *out = dev;
    return HB_OK;
}

// an empty table of `kind` with an index for index_keys keys and room for value_keys values
int create(int32_t device, uint32_t kind, uint64_t index_keys, uint64_t value_keys, hbu_table **out)
{
    if (!out) return fail(nullptr, HB_ERR_INVALID, "out == NULL");
    *out = nullptr;
    if (!bytes_of_kind(kind)) return fail(nullptr, HB_ERR_INVALID, "unknown table kind");
    int dev = 0, rc = pick_device(device, &dev);
    if (rc) return rc;
    Owned<hbu_table> tab(new hbu_table());
    tab->device = dev;
    tab->kind = kind;
    tab->vbytes = bytes_of_kind(kind);
    if (hipSetDevice(dev) != hipSuccess || tab->stream.create() != hipSuccess) return fail(nullptr, HB_ERR_HIP, "stream creation failed");
    if (tab->d_next.alloc(2) != hipSuccess || tab->h_word.alloc(2) != hipSuccess) {
        (void)hipGetLastError();
        rc = fail(tab.get(), HB_ERR_NOMEM, "allocation of the index counter failed");
    }
    if (!rc) rc = rebuild_index(tab.get(), std::max<uint64_t>(index_keys, 1), 0);
    if (!rc) rc = reserve(tab.get(), std::max<uint64_t>(value_keys, 1));
    if (rc) return fail(nullptr, rc, tab->err);
    *out = tab.release();
    return HB_OK;
}

// HyperLogLog<64>::size()'s tables on a device (hll64_tables.inc + the linear-counting table of hb_internal.h): they go up once
// per device and process and stay.  The map holds them UNOWNED on purpose: a static full of DevPtrs would call hipFree during static
// destruction, when the runtime may be gone already.  They are built in holders - a failure half-way frees itself - and released into it.
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
        DevPtr<double> raw, bias;
        DevPtr<uint8_t> d_lc;
        hipError_t e = raw.alloc(sizeof(HLL64_RAW_ESTIMATE) / sizeof(double));
        if (e == hipSuccess) e = bias.alloc(sizeof(HLL64_BIAS) / sizeof(double));
        if (e == hipSuccess) e = d_lc.alloc(68);
        if (e == hipSuccess) e = hipMemcpy(raw.get(), HLL64_RAW_ESTIMATE, sizeof(HLL64_RAW_ESTIMATE), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(bias.get(), HLL64_BIAS, sizeof(HLL64_BIAS), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_lc.get(), lc, 68, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(t, e == hipErrorOutOfMemory ? HB_ERR_NOMEM : HB_ERR_HIP, std::string("estimator tables: ") + hipGetErrorString(e));
        }
        it = g_estimator.emplace(t->device, EstimatorTables{}).first; // (first, so that a failed insertion cannot strand released buffers)
        it->second = EstimatorTables{raw.release(), bias.release(), d_lc.release()};
    }
    *out = it->second;
    return HB_OK;
}
template <class V>
hbv::Side<V> side_of(const hbu_table *t) { return hbv::Side<V>{table_of(t), (uint32_t)t->committed, (const V *)t->d_table.get()}; }
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
        hbu_table *made = nullptr;
        // (slots / 2 keys give an index of exactly `slots` entries: the copy keeps every entry where it is)
        int rc = create(t->device, t->kind, t->slots / 2, t->committed, &made);
        if (rc) return fail(t, rc, g_hbu_error);
        Owned<hbu_table> tab(made);
        // everything of `from` is complete on return of every call; the synchronise covers a caller that used another thread
        hipError_t e = tab->slots == t->slots ? hipStreamSynchronize(t->stream) : hipErrorInvalidValue;
        if (e == hipSuccess) e = hipMemcpyAsync(tab->d_keys.get(), t->d_keys.get(), t->slots * sizeof(u128), hipMemcpyDeviceToDevice, tab->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(tab->d_pids.get(), t->d_pids.get(), t->slots * sizeof(uint32_t), hipMemcpyDeviceToDevice, tab->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(tab->d_next.get(), t->d_next.get(), sizeof(unsigned long long), hipMemcpyDeviceToDevice, tab->stream);
        if (e == hipSuccess && t->committed) e = hipMemcpyAsync(tab->d_table.get(), t->d_table.get(), t->committed * t->vbytes, hipMemcpyDeviceToDevice, tab->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(tab->stream);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(t, HB_ERR_HIP, std::string("copy of the table: ") + hipGetErrorString(e));
        }
        tab->committed = t->committed;
        *out = tab.release();
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
        hb_u128 *d_out;
        const int rc = workspace(t->work, t, [&](Carve &c) { d_out = c.take<hb_u128>(n); });
        if (rc) return rc;
        // the keys go where their entry numbers point, which is where the values already are: rows 0 .. committed of the value table
        hipLaunchKernelGGL(hbr::set_export_kernel, dim3(grid_for(t->slots)), dim3(256), 0, t->stream, (const u128 *)t->d_keys.get(), (const uint32_t *)t->d_pids.get(), t->slots,
                           (uint32_t)n, d_out);
        HBU_HIP(hipGetLastError());
        HBU_HIP(hipMemcpyAsync(keys_out, d_out, n * sizeof(hb_u128), hipMemcpyDeviceToHost, t->stream));
        HBU_HIP(hipMemcpyAsync(values_out, t->d_table.get(), n * t->vbytes, hipMemcpyDeviceToHost, t->stream));
        HBU_HIP(hipStreamSynchronize(t->stream));
        *written = n;
        return HB_OK;
    });
}

} // extern "C"

// ---- the rest of the shard, in this translation unit (one set of kernel instantiations) ---------------------------------------------
#include "hb_ampc_steps.inc"  // the fold, update_centralities, the two edge steps
#include "hb_ampc_round.inc"  // a worker's resident graph and changed-node filter, the round steps
#include "hb_ampc_finish.inc" // the finish of a job: values, ranks, top nodes, store
