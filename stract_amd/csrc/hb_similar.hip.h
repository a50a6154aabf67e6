// hb_similar.hip.h - device code of hb_similar_hosts: scored_nodes of SimilarHostsFinder::find_similar_hosts
// (crates/core/src/similar_hosts.rs:54-272) for a list of liked hosts.  Part of the hb_api.hip translation unit (included after
// hb_links.hip.h).  Driver: hb_api_similar.inc.  Definitions: include/hyperball.h.  DESIGN.md section 28.
//
// The four sets of lists - In512 of the liked hosts, the forward lists of the co-citation sources, In512 of the candidates - come from
// the link operators' batch loop (links_lists, hb_api_links.inc); a list is `kShList` u32 sids per slot in (key, NodeID) order with its
// degree beside it.  The kernels here work between those calls:
//   sources:  the distinct sids of the 128-prefixes of the liked hosts' lists (a flag word per node claims a sid once, an atomic cursor
//             appends it: B is a set, its order is internal and decides nothing).
//   count:    count[v] += 1 for every entry of every forward list - an n-sized u32 counter array with vector atomic adds; the first
//             add of a node appends it to `touched`.  Chosen over a device sort of all forward entries plus run lengths: the entries
//             number up to 512 x |B| (16.8 M at the limits) and would be sorted as 64-bit keys in four passes, while the counter takes
//             one atomic per entry and leaves only the DISTINCT targets to order.
//   key:      per touched node its order key (2^32 - 1 - count) << 32 | sid, or ~0 when the popularity filter drops it (count above
//             (nb + 3) / 4).  The keys are unique, so the device sort that follows (gpu_rank_keys_device) defines the order
//             (count descending, NodeID ascending) whatever order `touched` was written in.
//   take:     the first `take` keys in that order, THEN the liked hosts dropped (similar_hosts.rs:152-164, in that order), compacted
//             in order by one workgroup (at most 1024 entries).
//   bitvec:   a workgroup per list: its first min(degree, 512) sids sorted ascending in LDS (BitVec::new sorts the ranks) and the 64-bit
//             bloom mask of those entries ((low id word x 11400714819323198549) & 63, hb_similarity.hip.h).
//   score:    a workgroup per candidate, the anchors in CALLER order: the integer gate 4 popcount(ma & mc) < max(popcount) gives 0,
//             else both sorted lists in LDS (2 x 2 KB), every lane binary-searches its entries of the candidate's list in the anchor's,
//             the counts are added in LDS, and lane 0 adds count / (sqrt(len_a) x sqrt(len_c)) to the sum - one f64 accumulator in one
//             lane, in caller order, no floating-point atomics.  score = max(0, sum / max(N, 1)).
//   top:      one workgroup: bitonic sort of at most 1024 (score bits, sid + 1) descending - scores are >= 0, so their bit patterns
//             order like the values; ties go to the larger NodeID (sorted_k over Reverse((SortableFloat, NodeID))).
// The only atomics are vector atomic adds / ors on u32 and u64 words; every store is an ordinary vector store.
#pragma once

namespace hbk {

constexpr uint32_t kShList = 512;   // entries of a list (EdgeLimit::Limit(512))
constexpr uint32_t kShPrefix = 128; // ... of which the first feed the co-citation sources (Limit(128))
constexpr uint32_t kShMaxCand = 1024;

__global__ __launch_bounds__(256) void sh_sources_kernel(const uint32_t *lists, const uint32_t *len, uint64_t slots, uint64_t n, uint32_t *mark, uint32_t *out,
                                                         uint32_t *cursor)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256, total = slots * kShPrefix;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const uint64_t slot = i / kShPrefix, j = i % kShPrefix;
        if (j >= len[slot]) continue;
        const uint32_t v = lists[slot * kShList + j];
        HB_DBG_ASSERT(v < n);
        if (v < n && atomicOr(&mark[v], 1u) == 0u) out[atomicAdd(cursor, 1u)] = v;
    }
}

__global__ __launch_bounds__(256) void sh_count_kernel(const uint32_t *lists, const uint32_t *len, uint64_t slots, uint64_t n, uint32_t *count, uint32_t *touched,
                                                       uint64_t touched_cap, uint32_t *cursor)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256, total = slots * kShList;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const uint64_t slot = i / kShList, j = i % kShList;
        if (j >= len[slot]) continue;
        const uint32_t v = lists[slot * kShList + j];
        HB_DBG_ASSERT(v < n);
        if (v < n && atomicAdd(&count[v], 1u) == 0u) {
            const uint32_t pos = atomicAdd(cursor, 1u);
            HB_DBG_ASSERT(pos < touched_cap);
            if (pos < touched_cap) touched[pos] = v;
        }
    }
}

__global__ __launch_bounds__(256) void sh_key_kernel(const uint32_t *touched, uint64_t m, const uint32_t *count, uint32_t apply, uint32_t bound, uint64_t *key,
                                                     uint32_t *eligible)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += stride) {
        const uint32_t v = touched[i], c = count[v];
        const bool ok = !apply || c <= bound;
        key[i] = ok ? ((uint64_t)(0xFFFFFFFFu - c) << 32) | v : ~0ull;
        if (ok) atomicAdd(eligible, 1u);
    }
}

// is v one of the ascending sids list[0 .. count)
__device__ __forceinline__ bool sh_contains(const uint32_t *list, uint32_t count, uint32_t v)
{
    uint32_t lo = 0, hi = count;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (list[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo < count && list[lo] == v;
}

// one workgroup: the first `take` keys of the order, the liked hosts dropped afterwards; cand / cand_count in order, *written = how many
__global__ __launch_bounds__(256) void sh_take_kernel(const uint64_t *key, const uint64_t *order, uint32_t take, const uint32_t *liked, uint32_t nliked,
                                                      uint32_t *cand, uint32_t *cand_count, uint32_t *written)
{
    __shared__ uint32_t s_v[kShMaxCand], s_c[kShMaxCand], s_keep[kShMaxCand];
    for (uint32_t i = threadIdx.x; i < take; i += 256) {
        const uint64_t k = key[order[i]];
        HB_DBG_ASSERT(k != ~0ull);
        s_v[i] = (uint32_t)k;
        s_c[i] = 0xFFFFFFFFu - (uint32_t)(k >> 32);
        s_keep[i] = sh_contains(liked, nliked, (uint32_t)k) ? 0u : 1u;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t at = 0;
        for (uint32_t i = 0; i < take; i++)
            if (s_keep[i]) {
                cand[at] = s_v[i];
                cand_count[at] = s_c[i];
                at++;
            }
        *written = at;
    }
}

// the body of a BitVec kernel, a workgroup per list (sh_bitvec_kernel here, sc_bitvec_kernel in hb_score.hip.h): the first
// min(len, stride) sids of list `slot` sorted ascending in place - a bitonic sort of `sort_n` LDS words, a power of two >= stride - and
// the bloom mask of those entries
__device__ __forceinline__ void sh_bitvec_body(uint32_t *s_v, unsigned long long *s_mask, uint32_t sort_n, uint32_t stride, uint32_t *lists, const uint32_t *len,
                                               const uint32_t *dev_of, const uint64_t *idlow, uint64_t n, unsigned long long *mask)
{
    const uint64_t slot = blockIdx.x;
    const uint32_t d = len[slot], L = d < stride ? d : stride;
    if (threadIdx.x == 0) *s_mask = 0ull;
    for (uint32_t i = threadIdx.x; i < sort_n; i += 256) s_v[i] = i < L ? lists[slot * stride + i] : kNone;
    __syncthreads();
    for (uint32_t k = 2; k <= sort_n; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = threadIdx.x; i < sort_n; i += 256) {
                const uint32_t x = i ^ j;
                if (x > i) {
                    const uint32_t a = s_v[i], c = s_v[x];
                    if ((a > c) == ((i & k) == 0)) {
                        s_v[i] = c;
                        s_v[x] = a;
                    }
                }
            }
            __syncthreads();
        }
    unsigned long long mine = 0ull;
    for (uint32_t i = threadIdx.x; i < L; i += 256) {
        const uint32_t v = s_v[i];
        HB_DBG_ASSERT(v < n);
        lists[slot * stride + i] = v;
        if (v < n) mine |= 1ull << ((idlow[dev_of[v]] * kSimBloomMul) & 63ull);
    }
    if (mine) atomicOr(s_mask, mine);
    __syncthreads();
    if (threadIdx.x == 0) mask[slot] = *s_mask;
}

// a workgroup per list: sorted by sid in place, its bloom mask
__global__ __launch_bounds__(256) void sh_bitvec_kernel(uint32_t *lists, const uint32_t *len, const uint32_t *dev_of, const uint64_t *idlow, uint64_t n,
                                                        unsigned long long *mask)
{
    __shared__ uint32_t s_v[kShList];
    __shared__ unsigned long long s_mask;
    sh_bitvec_body(s_v, &s_mask, kShList, kShList, lists, len, dev_of, idlow, n, mask);
}

// a workgroup per candidate; anchor_slot: the liked entries in caller order as slots of the anchors' lists, kNone = no node of the graph
__global__ __launch_bounds__(256) void sh_score_kernel(const uint32_t *clist, const uint32_t *clen, const unsigned long long *cmask, const uint32_t *alist,
                                                       const uint32_t *alen, const unsigned long long *amask, const uint32_t *anchor_slot, uint64_t N, double *score,
                                                       unsigned long long *pairs)
{
    __shared__ uint32_t s_c[kShList], s_a[kShList];
    __shared__ uint32_t s_cnt;
    const uint64_t c = blockIdx.x;
    const uint32_t dc = clen[c], lc = dc < kShList ? dc : kShList;
    const unsigned long long mc = cmask[c];
    for (uint32_t i = threadIdx.x; i < lc; i += 256) s_c[i] = clist[c * kShList + i];
    double sum = 0.0; // (lane 0's is the one that counts)
    unsigned long long gated = 0, intersected = 0;
    for (uint64_t i = 0; i < N; i++) { // workgroup-uniform: every branch below depends on the pair only
        const uint32_t a = anchor_slot[i];
        if (a == kNone) continue;
        const uint32_t da = alen[a], la = da < kShList ? da : kShList;
        if (!la || !lc) continue; // an empty list: sim 0
        const unsigned long long ma = amask[a];
        const uint32_t both = (uint32_t)__popcll(ma & mc), pa = (uint32_t)__popcll(ma), pc = (uint32_t)__popcll(mc);
        if (4u * both < (pa > pc ? pa : pc)) {
            gated++;
            continue;
        }
        __syncthreads(); // (the previous pair's searches are done with s_a; the first pair's s_c is complete)
        for (uint32_t j = threadIdx.x; j < la; j += 256) s_a[j] = alist[(uint64_t)a * kShList + j];
        if (threadIdx.x == 0) s_cnt = 0;
        __syncthreads();
        uint32_t mine = 0;
        for (uint32_t j = threadIdx.x; j < lc; j += 256) mine += sh_contains(s_a, la, s_c[j]) ? 1u : 0u;
        if (mine) atomicAdd(&s_cnt, mine);
        __syncthreads();
        if (threadIdx.x == 0) sum += (double)s_cnt / (sqrt((double)la) * sqrt((double)lc));
        intersected++;
    }
    if (threadIdx.x == 0) {
        const double s = sum / (double)(N > 1 ? N : 1);
        score[c] = s > 0.0 ? s : 0.0;
        if (gated) atomicAdd(&pairs[0], gated);
        if (intersected) atomicAdd(&pairs[1], intersected);
    }
}

// one workgroup: the candidates by (score descending, NodeID descending), the first k of them
__global__ __launch_bounds__(256) void sh_top_kernel(const uint32_t *cand, const double *score, uint32_t C, uint32_t k, uint32_t *top_sid, double *top_score)
{
    __shared__ unsigned long long s_s[kShMaxCand];
    __shared__ uint32_t s_v[kShMaxCand];
    for (uint32_t i = threadIdx.x; i < kShMaxCand; i += 256) {
        s_s[i] = i < C ? (unsigned long long)__double_as_longlong(score[i]) : 0ull;
        s_v[i] = i < C ? cand[i] + 1u : 0u; // (padding sorts behind a real entry with score 0 and sid 0)
    }
    __syncthreads();
    for (uint32_t kk = 2; kk <= kShMaxCand; kk <<= 1)
        for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
            for (uint32_t i = threadIdx.x; i < kShMaxCand; i += 256) {
                const uint32_t x = i ^ j;
                if (x > i) {
                    const unsigned long long sa = s_s[i], sb = s_s[x];
                    const uint32_t va = s_v[i], vb = s_v[x];
                    const bool a_behind_b = sa < sb || (sa == sb && va < vb); // descending order: a belongs behind b
                    if (a_behind_b == ((i & kk) == 0)) {
                        s_s[i] = sb;
                        s_s[x] = sa;
                        s_v[i] = vb;
                        s_v[x] = va;
                    }
                }
            }
            __syncthreads();
        }
    const uint32_t w = k < C ? k : C;
    for (uint32_t i = threadIdx.x; i < w; i += 256) {
        top_sid[i] = s_v[i] - 1u;
        top_score[i] = __longlong_as_double((long long)s_s[i]);
    }
}

} // namespace hbk
