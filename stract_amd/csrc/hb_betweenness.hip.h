// hb_betweenness.hip.h - device code of hb_betweenness (Betweenness::calculate, crates/core/src/webgraph/centrality/betweenness.rs:29-146):
// Brandes' algorithm for eight sources at once over the HyperBall device plan.  Part of the hb_api.hip translation unit (included after
// hb_bfs.hip.h; the forward half is a walk of hb_walk.hip.h, the backward half uses the plan layout, the quad helpers of hb_regs.hip.h and
// kBfsHeavy).  Driver: hb_api_betweenness.inc.  Definitions: include/hyperball.h.
//
// A row of 64 bytes holds one value per source of the batch: eight u64 path counts going forward, eight f64 coefficients going back.
// Quad per row; lane q of the quad owns bytes 16 q .. 16 q + 15 of every row = the sources 2 q and 2 q + 1 of the batch.
//
// Forward level d is a level of hb_walk.hip.h with a saturating add as the join.  F_{d-1} holds, per row and source, sigma where
// dist == d - 1 and 0 elsewhere; A[w] = sum of F_{d-1} over in(w), through the chunk trees (virtual rows level by level, their partials
// rebuilt from zero); a source that has no distance for w yet and A > 0 gets dist = d, sigma = A, F_d = A.  A row's changed bit at d =
// "its F_d row is non-zero".  F is NOT cumulative, so the double buffer needs more care than the sampled walk's: the buffer written at
// level d still holds F_{d-2}, and every row whose bit is set in the bitmap word being overwritten is rewritten (zeroed unless it is
// non-zero again).  By induction a buffer holds exactly F of its level in EVERY row, which is what the dense mode (no bit test) reads.
// Stale partials of rows a sweep level did not visit are never read: their bit is clear and the non-dense modes test it, a dense level
// rebuilds every partial first.
//
// Backward level d (d = L + 1 .. 1) is a pull over the row -> readers transpose.  C_d holds, per node row and source, (1 + delta) /
// sigma where dist == d and 0 elsewhere, copied down the chunk trees (a chunk row carries the coefficient of the rows that read it), with
// one bit per row "has a source at level d".  Every node row with a source at dist == d - 1 sums C_d over its readers whose bit is set -
// in list order, a fixed shape per list length - and stores delta = sigma * sum and its own C_{d-1} entry for those sources.  C is
// double buffered (a row can be at level d for one source and at d - 1 for another); rows without a set bit are never read, so nothing
// is cleared between levels.  Adding +0.0 to a non-negative sum is exact: skipping unset rows changes no bit of any result.
// No floating-point atomics anywhere, and no FMA contraction (the translation unit is built with -ffp-contract=off).
#pragma once

namespace hbk {

constexpr uint32_t kBcLanes = 8;       // sources per batch: the u64 / f64 values of one 64-byte row
constexpr uint64_t kBcWaveList = 256;  // backward: a longer reader list is summed by the whole wave, a shorter one by its quad
constexpr uint64_t kBcSegment = kBfsHeavy; // backward: a reader list longer than this is summed by the grid, one wave per segment

struct alignas(16) bc_u2 {
    unsigned long long a, b;
};
struct alignas(16) bc_d2 {
    double a, b;
};

struct BcParams : WalkParams { // a row's bit = "its F row is non-zero"; cnt[2] = entries gathered, cnt[3] = saturated sigmas
    const bc_u2 *rd;          // node rows: F of level d - 1
    bc_u2 *wr;                // node rows: F of level d (holds F of level d - 2 on entry, and bits_wr the bits of level d - 2)
    bc_u2 *part;              // virtual rows, indexed by vid - n_pad
    uint8_t *dist;            // n_pad x 8: distance per row and source, 255 = none
    unsigned long long *sigma; // n_pad x 8
    uint8_t *reached;         // n_pad: the row is a result (a source, or reached from one, in any batch)
    uint32_t level;
};

__device__ __forceinline__ unsigned long long bc_sat_add(unsigned long long a, unsigned long long b)
{
    const unsigned long long s = a + b;
    return s < a ? ~0ull : s; // (~0 is absorbing: order-independent for non-negative terms)
}

__device__ __forceinline__ void bc_add_counters(unsigned long long *cnt, unsigned long long a, unsigned long long b, unsigned long long c, unsigned long long d)
{
    wave_add_counters(cnt, a, b, c);
    if (d) atomicAdd(&cnt[3], d); // (a saturated path count: an error path)
}

// Level 0 of a batch (the buffers were cleared): source i gets dist 0, sigma 1 and F_0 = 1 in lane i of its own row.  A thread per source;
// the sources are distinct, so are the rows.
__global__ __launch_bounds__(64) void bc_seed_kernel(const uint32_t *sids, uint32_t count, const uint32_t *dev_of, unsigned long long *f0, uint32_t *bits,
                                                     const BcParams p)
{
    const uint32_t i = threadIdx.x;
    unsigned long long one = 0, od = 0;
    if (i < count) {
        const uint32_t row = dev_of[sids[i]];
        HB_DBG_ASSERT(row < p.n_pad);
        p.dist[(uint64_t)row * 8 + i] = 0;
        p.sigma[(uint64_t)row * 8 + i] = 1ull;
        f0[(uint64_t)row * 8 + i] = 1ull;
        p.reached[row] = 1;
        atomicOr(&bits[row >> 5], 1u << (row & 31u));
        one = 1;
        od = p.outdeg[row];
    }
    wave_add_counters(p.cnt, one, od, 0ull);
}

// One forward level over the rows [row_lo, row_hi) of one kind.
//   !REAL: virtual rows: partial = sum of the sources (dense: all of them; else those with a set bit); sweep: a non-zero partial
//          touches its readers.
//   REAL:  node rows: A = sum; sources without a distance and A > 0 get one.  The row of `wr` is stored when it is non-zero now or was
//          at level d - 2 (the bit of the word being overwritten).
template <bool REAL, int MODE>
__global__ __launch_bounds__(256) void bc_forward_kernel(const BcParams p)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 2, q = lane & 3, qshift = lane & ~3;
    const WalkSpan sp = walk_span<REAL>(p, wave);
    const bc_u2 *vbase = walk_virtual_base<bc_u2>(p.part, p.n_pad);
    unsigned long long c_changed = 0, c_out = 0, c_gath = 0, c_sat = 0;
    const auto sat_add = [](bc_u2 a, bc_u2 b) { return bc_u2{bc_sat_add(a.a, b.a), bc_sat_add(a.b, b.b)}; };
    for (uint64_t wi = sp.wid; wi < sp.nwords; wi += sp.wstride) { // wave-uniform trip count
        const uint64_t w = sp.w_lo + wi;
        const uint32_t tw = walk_take_touch<MODE>(p, w, lane);
        const uint32_t ow = REAL ? p.bits_wr[w] : 0u; // node rows whose `wr` image is a non-zero F of level d - 2
        if (MODE == kModeSweep && tw == 0 && ow == 0) { // nothing to visit or to zero in this word (a node word of bits_wr is zero already)
            if (!REAL) walk_store_bits<false>(p, w, 0u, lane);
            continue;
        }
        uint32_t chw = 0;
        for (int h = 0; h < 2; h++) {
            const uint32_t bit = (uint32_t)(h * 16 + g);
            const uint64_t row = (w << 5) + bit;
            const bool valid = row < sp.row_hi;
            const bool active = valid && ((tw >> bit) & 1u);
            const bc_u2 acc = walk_gather<MODE>(p, p.rd, vbase, row, active, q, bc_u2{0ull, 0ull}, sat_add, [&] {
                if (q == 0) c_gath++;
            });
            if (REAL) {
                bc_u2 f = {0ull, 0ull};
                if (active && (acc.a | acc.b) != 0ull) { // one writer per byte / word: this lane owns the two sources of this row
                    uint8_t *dp = p.dist + row * 8 + 2 * q;
                    unsigned long long *sg = p.sigma + row * 8 + 2 * q;
                    if (acc.a && dp[0] == kDistUnreached) {
                        dp[0] = (uint8_t)p.level;
                        sg[0] = acc.a;
                        f.a = acc.a;
                        if (acc.a == ~0ull) c_sat++;
                    }
                    if (acc.b && dp[1] == kDistUnreached) {
                        dp[1] = (uint8_t)p.level;
                        sg[1] = acc.b;
                        f.b = acc.b;
                        if (acc.b == ~0ull) c_sat++;
                    }
                }
                const uint64_t bal = __ballot((f.a | f.b) != 0ull);
                const bool changed = ((bal >> qshift) & 0xFull) != 0;
                if (valid && (changed || ((ow >> bit) & 1u))) p.wr[row * 4 + q] = f;
                if (changed && q == 0) {
                    p.reached[row] = 1;
                    c_changed++;
                    c_out += p.outdeg[row];
                }
                chw |= pack16(bal) << (16 * h);
            } else {
                const uint64_t bal = __ballot(active && (acc.a | acc.b) != 0ull);
                const bool changed = ((bal >> qshift) & 0xFull) != 0;
                if (active && (MODE == kModeDense || changed)) p.part[(row - p.n_pad) * 4 + q] = acc;
                if (MODE == kModeSweep && changed) walk_touch_readers(p, row, q);
                chw |= pack16(bal) << (16 * h);
            }
        }
        walk_store_bits<REAL>(p, w, chw, lane);
    }
    bc_add_counters(p.cnt, c_changed, c_out, c_gath, c_sat);
}

// ---- backward ----------------------------------------------------------------------------------------------------------------------
struct BcBackParams {
    const uint64_t *out_ptr;  // rows_total + 1: the readers of every work row
    const uint32_t *out_rows;
    const bc_d2 *crd;         // node rows: C of level d
    bc_d2 *cwr;               // node rows: C of level d - 1
    bc_d2 *cpart;             // virtual rows, indexed by vid - n_pad: C of the level the launch is about
    const uint32_t *bits_rd;  // "has a source at level d" (node rows) / "carries a coefficient of level d" (virtual rows)
    uint32_t *bits_wr;        // the same for level d - 1
    const uint8_t *dist;
    const unsigned long long *sigma;
    double *delta;            // n_pad x 8
    uint32_t *heavy;          // node rows of this level whose reader list the grid sums
    unsigned int *heavy_cnt;
    uint32_t heavy_cap;       // 0 = the graph has no such row
    bc_d2 *seg;               // their partial sums: 2 slots per kBcSegment entries of out_rows (a row's first segment / a later one)
    uint64_t n_pad, rows_total;
    uint64_t row_lo, row_hi;
    uint32_t level;           // d: the sources at dist == d - 1 get their delta
};

// C of reader r for this lane's two sources; +0.0 when r does not take part at this level
__device__ __forceinline__ bc_d2 bc_coef(const BcBackParams &p, uint32_t r, int q)
{
    bc_d2 c = {0.0, 0.0};
    if (r == kNone) return c;
    HB_DBG_ASSERT(r < p.rows_total);
    if (!((p.bits_rd[r >> 5] >> (r & 31u)) & 1u)) return c;
    return r < p.n_pad ? p.crd[(uint64_t)r * 4 + q] : p.cpart[((uint64_t)r - p.n_pad) * 4 + q];
}

// out_rows[kb .. ke) summed by a whole wave in a shape fixed by (kb, ke): quad g takes the entries kb + g, kb + g + 16, ... in order,
// then the sixteen quad sums meet in a butterfly (a + b == b + a: every lane ends with the same bits).  Wave-uniform.
__device__ __forceinline__ bc_d2 bc_wave_sum(const BcBackParams &p, uint64_t kb, uint64_t ke, int g, int q)
{
    bc_d2 s = {0.0, 0.0};
    for (uint64_t k0 = kb; k0 < ke; k0 += 16) {
        const uint64_t k = k0 + (uint64_t)g;
        if (k < ke) {
            const bc_d2 c = bc_coef(p, p.out_rows[k], q);
            s.a += c.a;
            s.b += c.b;
        }
    }
#pragma unroll
    for (int off = 4; off <= 32; off <<= 1) {
        const double oa = __shfl_xor(s.a, off), ob = __shfl_xor(s.b, off);
        s.a += oa;
        s.b += ob;
    }
    return s;
}

// the end of a row's pull: delta and the row's own coefficient for the sources at dist == d - 1 (this lane's two); the other sources
// of the row get +0.0 in C_{d-1}
__device__ __forceinline__ void bc_finish_row(const BcBackParams &p, uint64_t row, int q, bc_d2 sum)
{
    const uint8_t *dp = p.dist + row * 8 + 2 * q;
    const uint32_t dm1 = p.level - 1u;
    bc_d2 c = {0.0, 0.0};
    if (dp[0] == dm1) {
        const double sg = (double)p.sigma[row * 8 + 2 * q];
        const double dl = sg * sum.a;
        p.delta[row * 8 + 2 * q] = dl;
        c.a = (1.0 + dl) / sg;
    }
    if (dp[1] == dm1) {
        const double sg = (double)p.sigma[row * 8 + 2 * q + 1];
        const double dl = sg * sum.b;
        p.delta[row * 8 + 2 * q + 1] = dl;
        c.b = (1.0 + dl) / sg;
    }
    p.cwr[row * 4 + q] = c;
}

// One backward level over the node rows.  A wave owns one 32-row word (two rounds of 16 rows, a quad per row) and writes the word of
// bits_wr whole.  Reader lists of up to kBcWaveList entries are summed by the row's quad, four gathers in flight; longer ones by the
// wave; those above kBcSegment are left to bc_back_heavy_*.
__global__ __launch_bounds__(256) void bc_back_node_kernel(const BcBackParams p)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 2, q = lane & 3;
    const uint64_t w_lo = p.row_lo >> 5, nwords = (p.row_hi - p.row_lo + 31) >> 5;
    const uint64_t wid = (uint64_t)blockIdx.x * 4 + wave, wstride = (uint64_t)gridDim.x * 4;
    const uint32_t dm1 = p.level - 1u;
    for (uint64_t wi = wid; wi < nwords; wi += wstride) { // wave-uniform trip count
        const uint64_t w = w_lo + wi;
        uint32_t hasw = 0, longm = 0;
        for (int h = 0; h < 2; h++) {
            const uint32_t bit = (uint32_t)(h * 16 + g);
            const uint64_t row = (w << 5) + bit;
            bool mine = false;
            if (row < p.row_hi) {
                const uint8_t *dp = p.dist + row * 8 + 2 * q;
                mine = dp[0] == dm1 || dp[1] == dm1;
            }
            const uint32_t has16 = pack16(__ballot(mine));
            const bool has = (has16 >> g) & 1u;
            uint64_t kb = 0, ke = 0;
            if (has) {
                kb = p.out_ptr[row];
                ke = p.out_ptr[row + 1];
            }
            const bool is_long = ke - kb > kBcWaveList;
            if (is_long) ke = kb;
            bc_d2 sum = {0.0, 0.0};
            for (uint64_t k = kb; k < ke; k += 4) { // quad-uniform trip count
                const uint32_t idx = (k + q < ke) ? p.out_rows[k + q] : kNone;
                const uint32_t r0 = quad_bcast<0>(idx), r1 = quad_bcast<1>(idx), r2 = quad_bcast<2>(idx), r3 = quad_bcast<3>(idx);
                const bc_d2 c0 = bc_coef(p, r0, q), c1 = bc_coef(p, r1, q), c2 = bc_coef(p, r2, q), c3 = bc_coef(p, r3, q);
                sum.a = ((sum.a + c0.a) + c1.a) + c2.a + c3.a;
                sum.b = ((sum.b + c0.b) + c1.b) + c2.b + c3.b;
            }
            if (has && !is_long) bc_finish_row(p, row, q, sum);
            hasw |= has16 << (16 * h);
            longm |= pack16(__ballot(is_long)) << (16 * h);
        }
        while (longm) { // wave-uniform
            const int b = __ffs((int)longm) - 1;
            longm &= longm - 1;
            const uint64_t row = (w << 5) + (uint64_t)b;
            const uint64_t kb = p.out_ptr[row], ke = p.out_ptr[row + 1];
            if (p.heavy_cap && ke - kb > kBcSegment) {
                if (lane == 0) {
                    const unsigned int pos = atomicAdd(p.heavy_cnt, 1u);
                    HB_DBG_ASSERT(pos < p.heavy_cap);
                    if (pos < p.heavy_cap) p.heavy[pos] = (uint32_t)row;
                }
                continue;
            }
            const bc_d2 s = bc_wave_sum(p, kb, ke, g, q);
            if (g == 0) bc_finish_row(p, row, q, s);
        }
        if (lane == 0) p.bits_wr[w] = hasw;
    }
}

// the heavy rows of a backward level: every kBcSegment-entry segment of out_rows that a heavy row's list overlaps is summed by one wave
// (bc_wave_sum over the overlap).  Slot 1 of a segment = the row whose list begins inside it, slot 0 = the row that was already running
// (two rows longer than a segment cannot both do the same in one segment).
__global__ __launch_bounds__(256) void bc_back_heavy_partial_kernel(const BcBackParams p)
{
    const unsigned int have = *p.heavy_cnt;
    const uint32_t nheavy = have < p.heavy_cap ? have : p.heavy_cap;
    const int lane = threadIdx.x & 63, g = lane >> 2, q = lane & 3;
    const uint64_t wid = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * 4;
    for (uint32_t i = 0; i < nheavy; i++) {
        const uint32_t u = p.heavy[i];
        HB_DBG_ASSERT(u < p.n_pad);
        const uint64_t kb = p.out_ptr[u], ke = p.out_ptr[u + 1];
        const uint64_t j_last = (ke - 1) / kBcSegment;
        for (uint64_t j = kb / kBcSegment + wid; j <= j_last; j += nwaves) { // wave-uniform
            const uint64_t lo = kb > j * kBcSegment ? kb : j * kBcSegment;
            const uint64_t hi = ke < (j + 1) * kBcSegment ? ke : (j + 1) * kBcSegment;
            const bc_d2 s = bc_wave_sum(p, lo, hi, g, q);
            if (g == 0) p.seg[(2 * j + (kb > j * kBcSegment ? 1 : 0)) * 4 + q] = s;
        }
    }
}

// ... and their segments added up in list order, a quad per heavy row
__global__ __launch_bounds__(256) void bc_back_heavy_finish_kernel(const BcBackParams p)
{
    const unsigned int have = *p.heavy_cnt;
    const uint32_t nheavy = have < p.heavy_cap ? have : p.heavy_cap;
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    const uint32_t i = t >> 2;
    const int q = (int)(t & 3u);
    if (i >= nheavy) return;
    const uint32_t u = p.heavy[i];
    const uint64_t kb = p.out_ptr[u], ke = p.out_ptr[u + 1];
    bc_d2 sum = {0.0, 0.0};
    for (uint64_t j = kb / kBcSegment; j <= (ke - 1) / kBcSegment; j++) {
        const bc_d2 s = p.seg[(2 * j + (kb > j * kBcSegment ? 1 : 0)) * 4 + q];
        sum.a += s.a;
        sum.b += s.b;
    }
    bc_finish_row(p, u, q, sum);
}

// The coefficients of level d - 1 copied down one virtual level (the launches run from the highest level to the first, after the node
// rows): a chunk row carries the sum of its readers' coefficients - one reader, its hub or the chunk row above it, in the planner's
// trees - and the bit "some reader takes part".  `cnode` / `bits` are the buffers the node kernel has just written.
__global__ __launch_bounds__(256) void bc_back_virt_kernel(const BcBackParams p, const bc_d2 *cnode, uint32_t *bits)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 2, q = lane & 3;
    const uint64_t w_lo = p.row_lo >> 5, nwords = (p.row_hi - p.row_lo + 31) >> 5;
    const uint64_t wid = (uint64_t)blockIdx.x * 4 + wave, wstride = (uint64_t)gridDim.x * 4;
    for (uint64_t wi = wid; wi < nwords; wi += wstride) { // wave-uniform trip count
        const uint64_t w = w_lo + wi;
        uint32_t anyw = 0;
        for (int h = 0; h < 2; h++) {
            const uint64_t row = (w << 5) + (uint64_t)(h * 16 + g);
            bool any = false;
            bc_d2 sum = {0.0, 0.0};
            if (row < p.row_hi) {
                for (uint64_t k = p.out_ptr[row]; k < p.out_ptr[row + 1]; k++) {
                    const uint32_t r = p.out_rows[k];
                    if (r == kNone) continue;
                    HB_DBG_ASSERT(r < p.rows_total);
                    if (!((bits[r >> 5] >> (r & 31u)) & 1u)) continue;
                    const bc_d2 c = r < p.n_pad ? cnode[(uint64_t)r * 4 + q] : p.cpart[((uint64_t)r - p.n_pad) * 4 + q];
                    sum.a += c.a;
                    sum.b += c.b;
                    any = true;
                }
                if (any) p.cpart[(row - p.n_pad) * 4 + q] = sum;
            }
            anyw |= pack16(__ballot(any)) << (16 * h);
        }
        if (lane == 0) bits[w] = anyw;
    }
}

// After level 1 of a batch: sum[v] += delta_s(v) for the batch's sources in ascending order, skipping the source that is v itself
// (dist == 0).  A source that never reached v has delta +0.0.  A thread per node row.
__global__ __launch_bounds__(256) void bc_accumulate_kernel(const uint8_t *dist, const double *delta, uint64_t n_pad, double *sum)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t row = (uint64_t)blockIdx.x * 256 + threadIdx.x; row < n_pad; row += stride) {
        double s = sum[row];
        for (uint32_t l = 0; l < kBcLanes; l++)
            if (dist[row * 8 + l] != 0) s += delta[row * 8 + l];
        sum[row] = s;
    }
}

// node rows whose reader list the grid sums (once per loaded graph: the capacity of the heavy list)
__global__ __launch_bounds__(256) void bc_count_heavy_kernel(const uint64_t *out_ptr, uint64_t n_pad, unsigned long long *cnt)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    unsigned long long c = 0;
    for (uint64_t r0 = (uint64_t)blockIdx.x * 256; r0 < n_pad; r0 += stride) { // wave-uniform trip count
        const uint64_t row = r0 + threadIdx.x;
        if (row < n_pad && out_ptr[row + 1] - out_ptr[row] > kBcSegment) c++;
    }
    wave_add_counters(cnt, c, 0ull, 0ull);
}

// The result in ascending-NodeID (sid) order: value = sum / norm (one division; norm = 1 with HB_BC_RAW), -1.0 and flag 255 for a node
// that is no result; flag 0 for a result (the select of hb_plan.hip keeps the sids whose flag is not 255).
__global__ __launch_bounds__(256) void bc_result_kernel(const double *sum, const uint8_t *reached, const uint32_t *dev_of, uint64_t n, uint64_t n_pad, int raw,
                                                        double norm, double *val, uint8_t *flag)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s < n; s += stride) {
        const uint32_t row = dev_of[s];
        HB_DBG_ASSERT(row < n_pad);
        const bool in = reached[row] != 0;
        val[s] = in ? (raw ? sum[row] : sum[row] / norm) : -1.0;
        flag[s] = in ? 0 : 255;
    }
    (void)n_pad;
}

} // namespace hbk
