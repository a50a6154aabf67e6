// hb_sample.hip.h - device code of hb_sampled_harmonic (ApproxHarmonic::build, approx_harmonic.rs:40-89): k single-source BFS walks
// at once, as exact bit sets over the HyperBall device plan.  Part of the hb_api.hip translation unit (included after hb_kernels.hip.h;
// uses its plan layout, quad helpers and the sweep support of hb_sweep.hip.h).
//
// A node row of 64 bytes holds one bit per source of the batch (512 sources): row v at level d = the sources within d hops of v.  A
// level is one HyperBall pass with OR as the join: virtual (hub-chunk) rows level by level, then the node rows, quad per row, lane q
// owning bytes 16 q .. 16 q + 15 of every row.  Level d reads only the level d - 1 buffer (an in-place update would let a bit travel two
// hops in one level and corrupt the histogram).  The same three modes as hb_run, with the same exactness argument: sets only grow, so a
// source whose row did not change at d - 1 adds nothing at d and may be skipped (bitmap mode), and a row no changed source reaches
// need not be visited at all (sweep mode, touch bitmap from the unchanged seed / expand kernels of hb_sweep.hip.h).
// Lazy double buffer as in hb_kernels.hip.h: the "new" buffer holds a node row's value unless the row changed at level d - 1.
#pragma once

namespace hbk {

constexpr int kSampleMaxLevels = 16;   // max_dist <= 15 (HB_SAMPLE_MAX_LEVELS)
constexpr uint32_t kSampleBatch = 512; // sources per batch: the bits of one 64-byte row
constexpr int kSampleDense = 0, kSampleBitmap = 1, kSampleSweep = 2;

struct SampleParams {
    const uint64_t *row_ptr;
    const uint32_t *src;
    const uint4 *rd;          // node rows at level d - 1
    uint4 *wr;                // node rows at level d
    uint4 *part;              // virtual rows, indexed by vid - n_pad
    uint32_t *bits_rd;        // changed bits: node rows = level d - 1, virtual rows = level d (written by this level's launches)
    uint32_t *bits_wr;        // changed bits of the node rows at level d
    uint32_t *touch;          // sweep: one bit per work row
    const uint64_t *out_ptr;  // sweep: readers of every work row
    const uint32_t *out_rows;
    const uint32_t *outdeg;   // per node row: out-degree
    uint16_t *hist;           // c_d of this level, per device row (the level's slice of the level-major histogram)
    unsigned long long *cnt;  // this level's counters: [0] node rows that changed, [1] their out-degree sum (A of the next level), [2] rows visited
    uint64_t n_pad, rows_total;
    uint64_t row_lo, row_hi;  // rows of this launch (multiples of 32)
    int xcd_map;              // as PassParams::xcd_map: workgroup b takes its words from group b % 8
    uint64_t xcd_lo[8], xcd_hi[8];
};

__device__ __forceinline__ uint4 u4_or(uint4 a, uint4 b) { return make_uint4(a.x | b.x, a.y | b.y, a.z | b.z, a.w | b.w); }

__device__ __forceinline__ void wave_add_counters(unsigned long long *cnt, unsigned long long a, unsigned long long b, unsigned long long c)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        a += __shfl_xor(a, off);
        b += __shfl_xor(b, off);
        c += __shfl_xor(c, off);
    }
    if ((threadIdx.x & 63) == 0) {
        if (a) atomicAdd(&cnt[0], a);
        if (b) atomicAdd(&cnt[1], b);
        if (c) atomicAdd(&cnt[2], c);
    }
}

// One level over the rows [row_lo, row_hi) of one kind.  A wave owns one 32-row word of the changed bitmaps per iteration (two rounds of
// 16 rows, a quad per row) and writes that word whole: no atomics on the bitmaps, and no clearing between levels.
//   REAL:   node rows: new = self | OR(sources), stored when it changed or changed at d - 1 (lazy double buffer);
//           c_d += popcount(new & ~self) - the sources first reached at distance d.
//   !REAL:  virtual rows: dense = OR of all sources (the partial is rebuilt), else partial | OR(changed sources);
//           sweep: a changed partial touches its readers (higher levels / node rows of this level).
template <bool REAL, int MODE>
__global__ __launch_bounds__(256) void sample_level_kernel(const SampleParams p)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 2, q = lane & 3, qshift = lane & ~3;
    uint64_t row_lo = p.row_lo, row_hi = p.row_hi;
    uint64_t wid = (uint64_t)blockIdx.x * 4 + wave, wstride = (uint64_t)gridDim.x * 4;
    if (!REAL && p.xcd_map) {
        const int x = blockIdx.x & 7;
        row_lo = p.xcd_lo[x];
        row_hi = p.xcd_hi[x];
        wid = (uint64_t)(blockIdx.x >> 3) * 4 + wave;
        wstride = (uint64_t)(gridDim.x >> 3) * 4; // the grid is a multiple of 8
    }
    const uint64_t w_lo = row_lo >> 5, nwords = (row_hi - row_lo + 31) >> 5;
    const uint4 *vbase = (const uint4 *)(p.part - p.n_pad * 4);
    unsigned long long c_changed = 0, c_out = 0, c_rows = 0;
    for (uint64_t wi = wid; wi < nwords; wi += wstride) { // wave-uniform trip count
        const uint64_t w = w_lo + wi;
        uint32_t tw = 0xFFFFFFFFu;
        if (MODE == kSampleSweep) {
            tw = __shfl(p.touch[w], 0);
            if (lane == 0 && tw) p.touch[w] = 0; // consumed: the touch bitmap is all-zero again after the level
        }
        const uint32_t pw = REAL ? p.bits_rd[w] : 0u; // node rows that changed at d - 1
        if (MODE == kSampleSweep && tw == 0 && pw == 0) { // nothing to visit or carry over in this word
            if (lane == 0) {
                if (REAL) p.bits_wr[w] = 0u;
                else p.bits_rd[w] = 0u;
            }
            continue;
        }
        uint32_t chw = 0;
        for (int h = 0; h < 2; h++) {
            const uint32_t bit = (uint32_t)(h * 16 + g);
            const uint64_t row = (w << 5) + bit;
            const bool valid = row < row_hi;
            const bool active = valid && ((tw >> bit) & 1u);
            const bool self_prev = REAL && valid && ((pw >> bit) & 1u);
            uint4 selfv = make_uint4(0, 0, 0, 0);
            if (REAL) {
                if (active || self_prev) selfv = p.rd[row * 4 + q];
            } else if (MODE != kSampleDense && active) {
                selfv = p.part[(row - p.n_pad) * 4 + q];
            }
            uint4 acc = selfv;
            uint64_t beg = 0, end = 0;
            if (active) {
                beg = p.row_ptr[row];
                end = p.row_ptr[row + 1];
            }
            for (uint64_t e = beg; e < end; e += 8) { // quad-uniform trip count: 8 gathers in flight per quad
                uint32_t i0 = (e + q < end) ? p.src[e + q] : kNone;
                uint32_t i1 = (e + 4 + q < end) ? p.src[e + 4 + q] : kNone;
                if (MODE != kSampleDense) { // only sources that changed (node rows: at d - 1; virtual rows: at this level)
                    if (i0 != kNone && !((p.bits_rd[i0 >> 5] >> (i0 & 31u)) & 1u)) i0 = kNone;
                    if (i1 != kNone && !((p.bits_rd[i1 >> 5] >> (i1 & 31u)) & 1u)) i1 = kNone;
                }
                uint32_t s[8];
                s[0] = quad_bcast<0>(i0);
                s[1] = quad_bcast<1>(i0);
                s[2] = quad_bcast<2>(i0);
                s[3] = quad_bcast<3>(i0);
                s[4] = quad_bcast<0>(i1);
                s[5] = quad_bcast<1>(i1);
                s[6] = quad_bcast<2>(i1);
                s[7] = quad_bcast<3>(i1);
                uint4 r[8];
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    r[j] = make_uint4(0, 0, 0, 0);
                    if (s[j] != kNone) {
                        HB_DBG_ASSERT(s[j] < p.rows_total);
                        r[j] = (s[j] < p.n_pad) ? p.rd[(uint64_t)s[j] * 4 + q] : vbase[(uint64_t)s[j] * 4 + q];
                    }
                }
#pragma unroll
                for (int j = 0; j < 8; j++) acc = u4_or(acc, r[j]);
            }
            const uint4 nd = make_uint4(acc.x & ~selfv.x, acc.y & ~selfv.y, acc.z & ~selfv.z, acc.w & ~selfv.w);
            const bool lane_diff = (!REAL && MODE == kSampleDense) ? active : (active && (nd.x | nd.y | nd.z | nd.w) != 0u);
            const uint64_t bal = __ballot(lane_diff);
            const bool changed = ((bal >> qshift) & 0xFull) != 0;
            if (REAL) {
                if (changed || self_prev) p.wr[row * 4 + q] = acc;
                uint32_t pc = (uint32_t)(__popc(nd.x) + __popc(nd.y) + __popc(nd.z) + __popc(nd.w));
                pc += __shfl_xor(pc, 1);
                pc += __shfl_xor(pc, 2);
                if (changed && q == 0) {
                    p.hist[row] = (uint16_t)(p.hist[row] + pc); // (k <= 65535 sources in all: no wrap)
                    c_changed++;
                    c_out += p.outdeg[row];
                }
            } else {
                if (changed) p.part[(row - p.n_pad) * 4 + q] = acc;
                if (MODE == kSampleSweep && changed) {
                    const uint64_t kb = p.out_ptr[row], ke = p.out_ptr[row + 1];
                    for (uint64_t k = kb + q; k < ke; k += 4) touch_set(p.touch, p.out_rows[k], p.rows_total);
                }
            }
            if (active && q == 0) c_rows++;
            chw |= pack16(bal) << (16 * h);
        }
        if (lane == 0) {
            if (REAL) p.bits_wr[w] = chw;
            else p.bits_rd[w] = chw; // (dense levels: nobody reads these, written anyway)
        }
    }
    wave_add_counters(p.cnt, c_changed, c_out, c_rows);
}

// Level 0 of a batch (the buffers were cleared): source i of the batch gets bit i of its own row, and its changed bit.
// One quad per source; the sources are distinct, so every row is written by one quad.
__global__ __launch_bounds__(256) void sample_seed_kernel(const uint32_t *rows, uint32_t count, uint4 *rd, uint32_t *bits, const uint32_t *outdeg,
                                                          unsigned long long *cnt)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const uint32_t s = i >> 2, q = i & 3u;
    unsigned long long od = 0, one = 0;
    if (s < count) {
        const uint32_t row = rows[s];
        uint32_t wv[4] = {0u, 0u, 0u, 0u};
        if ((s >> 7) == q) wv[(s >> 5) & 3u] = 1u << (s & 31u); // bit s of the 512: word s / 32, lane (s / 32) / 4
        rd[(uint64_t)row * 4 + q] = make_uint4(wv[0], wv[1], wv[2], wv[3]);
        if (q == 0) {
            atomicOr(&bits[row >> 5], 1u << (row & 31u));
            od = outdeg[row];
            one = 1;
        }
    }
    wave_add_counters(cnt, one, od, 0ull);
}

// The sampler's candidates: flags[sid] = the node has an out-edge (every real device row writes its sid's byte)
__global__ __launch_bounds__(256) void sample_candidates_kernel(const uint32_t *outdeg, const uint32_t *sid_of, uint64_t n_pad, uint8_t *flags)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n_pad; r += stride) {
        const uint32_t sid = sid_of[r];
        if (sid != kNone) flags[sid] = outdeg[r] ? 1 : 0;
    }
}

// device rows of a batch's sources: rows[i] = dev_of[sids[i]]
__global__ __launch_bounds__(256) void sample_rows_of_kernel(const uint32_t *sids, uint32_t count, const uint32_t *dev_of, uint32_t *rows)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < count) rows[i] = dev_of[sids[i]];
}

// The value of every node from its histogram (approx_harmonic.rs:57-78 with the summation order of include/hyperball.h): S in f64, d
// ascending from +0.0, only the terms with c_d > 0 (each product is exact in f64); value = (double)(float)S; absent = -1.0.  Written to
// the result image (d_cid_of: device row -> index, kNone = not in the image), the format hb_result_* and gpu_rank_results read.
__global__ __launch_bounds__(256) void sample_result_kernel(const uint16_t *hist, uint32_t levels, uint64_t n_pad, const double *w,
                                                            const uint32_t *cid_of, double *out, unsigned long long *cnt)
{
    unsigned long long kept = 0;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t r0 = (uint64_t)blockIdx.x * 256; r0 < n_pad; r0 += stride) { // wave-uniform trip count
        const uint64_t row = r0 + threadIdx.x;
        if (row >= n_pad) continue;
        const uint32_t cid = cid_of[row];
        if (cid == kNone) continue;
        double sum = 0.0;
        uint32_t total = 0;
        for (uint32_t d = 0; d < levels; d++) {
            const uint32_t cd = hist[(uint64_t)d * n_pad + row];
            if (cd) {
                sum += (double)cd * w[d];
                total += cd;
            }
        }
        out[cid] = total ? (double)(float)sum : -1.0;
        kept += total ? 1ull : 0ull;
    }
    wave_add_counters(cnt, kept, 0ull, 0ull);
}

} // namespace hbk
