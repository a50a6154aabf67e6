// hb_nearest_seed.hip.h - device code of hb_nearest_seed (HarmonicNearestSeed, crates/core/src/entrypoint/centrality.rs:126-201, over
// BacklinksQuery .. Limit(1), webgraph/query/backlink.rs:96-209): every node without an original centrality takes discount_factor x the
// centrality of its FIRST backlink's source.  Part of the hb_api.hip translation unit (included after hb_similarity.hip.h).  Driver:
// hb_api_nearest_seed.inc.  Definitions: include/hyperball.h.
//
// seed(v) = the in-neighbour u != v of v that minimises (key[u], NodeID u); sids ascend with the NodeIDs, so the order is that of
// (key, sid).  A candidate is 16 bytes {key u64, sid u32}; {~0, kNone} is "none" and loses against every node, a node with key ~0
// included (its sid is below kNone).
//   key:   cand[row] = {key of the row's node, its sid} per node row.
//   seed:  one pull over row_ptr / src with a lexicographic min as the join, the virtual levels ascending, then the node rows (a quad per
//          row, as sim_bloom_kernel).  A chunk row keeps the TWO best distinct candidates of its list: the hub's own candidate (a self
//          link, skipped: LinksQuery.skip_self_links) may be the minimum of one chunk and would hide the runner-up.  Edges are unique, so
//          a node's own sid occurs at most once in its tree, and the best candidate that is not the node itself is the first or the second
//          of every partial.  The join of two such pairs is associative and commutative.  seed_row[row] has one writer; no atomics.
//   fill:  one launch per round, a thread per node row, on a double buffer of (val f64, has u8): a row with a value keeps it, a row
//          without one whose seed had a value after the previous round gets that value x discount_factor - one f64 multiply per hop.
//   by sid: the values (-1.0 = none), the select flags, the seeds as sids and the final counters in ascending-NodeID order.
#pragma once

namespace hbk {

struct NsCand { // ordered by (key, sid)
    unsigned long long key;
    uint32_t sid;
};

__device__ __forceinline__ bool ns_less(unsigned long long kx, uint32_t sx, unsigned long long ky, uint32_t sy) { return kx != ky ? kx < ky : sx < sy; }
__device__ __forceinline__ NsCand ns_load(const uint4 *cand, uint64_t i)
{
    const uint4 v = cand[i];
    return NsCand{(unsigned long long)v.x | ((unsigned long long)v.y << 32), v.z};
}
__device__ __forceinline__ uint4 ns_pack(unsigned long long key, uint32_t sid) { return make_uint4((uint32_t)key, (uint32_t)(key >> 32), sid, 0u); }
// (ka, sa) < (kb, sb), or none: the two best distinct candidates so far; (k, s) joins them (equal sids are the same candidate).  Plain
// scalars and selects: the pair stays in registers (as a struct updated under branches it went to 32 bytes of scratch per lane)
__device__ __forceinline__ void ns_insert(unsigned long long &ka, uint32_t &sa, unsigned long long &kb, uint32_t &sb, unsigned long long k, uint32_t s)
{
    const bool skip = s == kNone || s == sa || s == sb;
    const bool first = !skip && ns_less(k, s, ka, sa);
    const bool second = !skip && !first && ns_less(k, s, kb, sb);
    kb = first ? ka : second ? k : kb;
    sb = first ? sa : second ? s : sb;
    ka = first ? k : ka;
    sa = first ? s : sa;
}

// ---- key -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ns_key_kernel(const unsigned long long *key_sid, const uint32_t *sid_of, uint64_t n_pad, uint4 *cand)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n_pad; r += stride) {
        const uint32_t sid = sid_of[r];
        cand[r] = sid != kNone ? ns_pack(key_sid[sid], sid) : ns_pack(~0ull, kNone);
    }
}

// ---- seed: the rows [row_lo, row_hi) of one kind ----------------------------------------------------------------------------------------
//   !REAL: chunk rows: part[(row - n_pad) * 2 + {0, 1}] = the two best distinct candidates of the list
//   REAL:  node rows: seed_row[row] = the device row of the best candidate that is not the row's own node, kNone = none
template <bool REAL>
__global__ __launch_bounds__(256) void ns_seed_kernel(const uint64_t *row_ptr, const uint32_t *src, const uint4 *cand, uint4 *part, const uint32_t *sid_of,
                                                      const uint32_t *dev_of, uint32_t *seed_row, uint64_t n_pad, uint64_t rows_total, uint64_t row_lo, uint64_t row_hi)
{
    const int q = threadIdx.x & 3;
    const uint64_t quad = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 2, stride = (uint64_t)gridDim.x * 64;
    for (uint64_t r0 = row_lo; r0 < row_hi; r0 += stride) { // wave-uniform trip count
        const uint64_t row = r0 + quad;
        unsigned long long ka = ~0ull, kb = ~0ull; // none
        uint32_t sa = kNone, sb = kNone;
        uint32_t self = kNone; // REAL: the sid no candidate may have
        if (row < row_hi) {
            if (REAL) self = sid_of[row];
            const uint64_t end = row_ptr[row + 1];
            for (uint64_t e = row_ptr[row] + q; e < end; e += 4) {
                const uint32_t s = src[e];
                if (s == kNone) continue;
                HB_DBG_ASSERT(s < rows_total);
                if (s < n_pad) {
                    const NsCand c = ns_load(cand, s);
                    if (!REAL || c.sid != self) ns_insert(ka, sa, kb, sb, c.key, c.sid);
                } else {
                    const NsCand c0 = ns_load(part, (s - n_pad) * 2), c1 = ns_load(part, (s - n_pad) * 2 + 1);
                    if (!REAL) {
                        ns_insert(ka, sa, kb, sb, c0.key, c0.sid);
                        ns_insert(ka, sa, kb, sb, c1.key, c1.sid);
                    } else { // (the row's own sid occurs at most once in its tree)
                        const bool first = c0.sid != self;
                        ns_insert(ka, sa, kb, sb, first ? c0.key : c1.key, first ? c0.sid : c1.sid);
                    }
                }
            }
        }
#pragma unroll
        for (int m = 1; m <= 2; m <<= 1) {
            const unsigned long long oka = __shfl_xor(ka, m), okb = __shfl_xor(kb, m);
            const uint32_t osa = __shfl_xor(sa, m), osb = __shfl_xor(sb, m);
            ns_insert(ka, sa, kb, sb, oka, osa);
            ns_insert(ka, sa, kb, sb, okb, osb);
        }
        if (row < row_hi && q == 0) {
            if (REAL) {
                seed_row[row] = (self != kNone && sa != kNone) ? dev_of[sa] : kNone;
            } else {
                part[(row - n_pad) * 2] = ns_pack(ka, sa);
                part[(row - n_pad) * 2 + 1] = ns_pack(kb, sb);
            }
        }
    }
    (void)rows_total;
}

// ---- values --------------------------------------------------------------------------------------------------------------------------
// round 0 from the caller's list (uploaded by sid): val / has per node row, cnt[0] = rows with an original value
__global__ __launch_bounds__(256) void ns_init_list_kernel(const double *val_sid, const uint8_t *has_sid, const uint32_t *sid_of, uint64_t n_pad, double *val,
                                                           uint8_t *has, unsigned long long *cnt)
{
    unsigned long long c = 0;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n_pad; r += stride) {
        const uint32_t sid = sid_of[r];
        const bool h = sid != kNone && has_sid[sid] != 0;
        val[r] = h ? val_sid[sid] : 0.0;
        has[r] = h ? 1 : 0;
        c += h ? 1 : 0;
    }
    wave_add_counters(cnt, c, 0ull, 0ull);
}

// round 0 from the context's live result image (HB_SEED_FROM_IMAGE): out[cid_of[row]] >= 0.0 is a result, as hb_result_copy reads it
__global__ __launch_bounds__(256) void ns_init_image_kernel(const double *out, const uint32_t *cid_of, uint64_t out_len, uint64_t n_pad, double *val, uint8_t *has,
                                                            unsigned long long *cnt)
{
    unsigned long long c = 0;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n_pad; r += stride) {
        const uint32_t cid = cid_of[r];
        HB_DBG_ASSERT(cid == kNone || cid < out_len);
        const double v = cid != kNone ? out[cid] : -1.0;
        const bool h = v >= 0.0;
        val[r] = h ? v : 0.0;
        has[r] = h ? 1 : 0;
        c += h ? 1 : 0;
    }
    (void)out_len;
    wave_add_counters(cnt, c, 0ull, 0ull);
}

// one round: the state after the previous round is read, the state after this one written (every row); the rows filled are counted per
// workgroup in LDS and added to the workgroup's stripe
__global__ __launch_bounds__(256) void ns_fill_kernel(const double *val_rd, const uint8_t *has_rd, const uint32_t *seed_row, uint64_t n_pad, double discount,
                                                      double *val_wr, uint8_t *has_wr, unsigned long long *counters)
{
    unsigned long long filled = 0;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n_pad; r += stride) {
        double v = val_rd[r];
        uint8_t h = has_rd[r];
        if (!h) {
            const uint32_t s = seed_row[r];
            if (s != kNone) {
                HB_DBG_ASSERT(s < n_pad);
                if (has_rd[s]) {
                    v = val_rd[s] * discount;
                    h = 1;
                    filled++;
                }
            }
        }
        val_wr[r] = v;
        has_wr[r] = h;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) filled += __shfl_xor(filled, off);
    const unsigned long long v4[4] = {filled, 0ull, 0ull, 0ull};
    block_add_counters(counters, v4, 0x1u);
}

// the result in ascending-NodeID (sid) order: value (-1.0 = none), the select's flag (0 = result, 255 = none), the seed as a sid;
// cnt[0] = results, cnt[1] = nodes without a value and without a seed, cnt[2] = nodes without a value whose seed has none either
__global__ __launch_bounds__(256) void ns_by_sid_kernel(const double *val, const uint8_t *has, const uint32_t *seed_row, const uint32_t *dev_of, const uint32_t *sid_of,
                                                        uint64_t n, uint64_t n_pad, double *val_sid, uint8_t *flag_sid, uint32_t *seed_sid, unsigned long long *cnt)
{
    unsigned long long c_res = 0, c_noseed = 0, c_noval = 0;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s < n; s += stride) {
        const uint32_t row = dev_of[s];
        HB_DBG_ASSERT(row < n_pad);
        const bool h = has[row] != 0;
        const uint32_t sr = seed_row[row];
        val_sid[s] = h ? val[row] : -1.0;
        flag_sid[s] = h ? 0 : 255;
        seed_sid[s] = sr != kNone ? sid_of[sr] : kNone;
        c_res += h ? 1 : 0;
        c_noseed += (!h && sr == kNone) ? 1 : 0;
        c_noval += (!h && sr != kNone) ? 1 : 0;
    }
    (void)n_pad;
    wave_add_counters(cnt, c_res, c_noseed, c_noval);
}

// hb_nearest_seed_top: the sort keys in REVERSED sid order (entry i = sid n - 1 - i), so that the select-and-sort of hb_similarity_top -
// key descending, ties by the higher entry - breaks ties by the LOWER NodeID ((Reverse(SortableFloat(c)), node_id), centrality.rs:186-195).
// A value is never negative: its bits order like the value.
__global__ __launch_bounds__(256) void ns_top_keys_kernel(const double *val_sid, const uint8_t *flag_sid, uint64_t n, uint64_t *key, uint8_t *keep)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const uint64_t s = n - 1 - i;
        key[i] = (uint64_t)__double_as_longlong(val_sid[s]);
        keep[i] = flag_sid[s] == 0 ? 1 : 0;
    }
}

} // namespace hbk
