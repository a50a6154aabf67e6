// hb_sample.hip.h - device code of hb_sampled_harmonic (ApproxHarmonic::build, approx_harmonic.rs:40-89): k single-source BFS walks
// at once, as exact bit sets over the HyperBall device plan.  Part of the hb_api.hip translation unit (included after hb_walk.hip.h:
// the shape of a level, its modes and the parts of the level kernel it shares with hb_betweenness.hip.h are described there).
//
// A node row of 64 bytes holds one bit per source of the batch (512 sources): row v at level d = the sources within d hops of v, the
// join is OR (an in-place update would let a bit travel two hops in one level and corrupt the histogram: level d reads only the level
// d - 1 buffer).  A row's bit = "the row grew at this level".  The modes are exact for the reason they are in hb_run: sets only grow,
// so a source whose row did not change at d - 1 adds nothing at d and may be skipped (bitmap mode), and a row no changed source reaches
// need not be visited at all (sweep mode).
// Lazy double buffer as in hb_kernels.hip.h: the "new" buffer holds a node row's value unless the row changed at level d - 1.
#pragma once

namespace hbk {

constexpr int kSampleMaxLevels = 16;   // max_dist <= 15 (HB_SAMPLE_MAX_LEVELS)
constexpr uint32_t kSampleBatch = 512; // sources per batch: the bits of one 64-byte row

struct SampleParams : WalkParams { // cnt[2] = rows visited
    const uint4 *rd;          // node rows at level d - 1
    uint4 *wr;                // node rows at level d
    uint4 *part;              // virtual rows, indexed by vid - n_pad
    uint16_t *hist;           // c_d of this level, per device row (the level's slice of the level-major histogram)
};

__device__ __forceinline__ uint4 u4_or(uint4 a, uint4 b) { return make_uint4(a.x | b.x, a.y | b.y, a.z | b.z, a.w | b.w); }

// One level over the rows [row_lo, row_hi) of one kind.
//   REAL:   node rows: new = self | OR(sources), stored when it changed or changed at d - 1 (lazy double buffer);
//           c_d += popcount(new & ~self) - the sources first reached at distance d.
//   !REAL:  virtual rows: dense = OR of all sources (the partial is rebuilt), else partial | OR(changed sources);
//           sweep: a changed partial touches its readers.
template <bool REAL, int MODE>
__global__ __launch_bounds__(256) void sample_level_kernel(const SampleParams p)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 2, q = lane & 3, qshift = lane & ~3;
    const WalkSpan sp = walk_span<REAL>(p, wave);
    const uint4 *vbase = walk_virtual_base<uint4>(p.part, p.n_pad);
    unsigned long long c_changed = 0, c_out = 0, c_rows = 0;
    for (uint64_t wi = sp.wid; wi < sp.nwords; wi += sp.wstride) { // wave-uniform trip count
        const uint64_t w = sp.w_lo + wi;
        const uint32_t tw = walk_take_touch<MODE>(p, w, lane);
        const uint32_t pw = REAL ? p.bits_rd[w] : 0u; // node rows that changed at d - 1
        if (MODE == kModeSweep && tw == 0 && pw == 0) { // nothing to visit or carry over in this word
            walk_store_bits<REAL>(p, w, 0u, lane);
            continue;
        }
        uint32_t chw = 0;
        for (int h = 0; h < 2; h++) {
            const uint32_t bit = (uint32_t)(h * 16 + g);
            const uint64_t row = (w << 5) + bit;
            const bool valid = row < sp.row_hi;
            const bool active = valid && ((tw >> bit) & 1u);
            const bool self_prev = REAL && valid && ((pw >> bit) & 1u);
            uint4 selfv = make_uint4(0, 0, 0, 0);
            if (REAL) {
                if (active || self_prev) selfv = p.rd[row * 4 + q];
            } else if (MODE != kModeDense && active) {
                selfv = p.part[(row - p.n_pad) * 4 + q];
            }
            const uint4 acc = walk_gather<MODE>(p, p.rd, vbase, row, active, q, selfv, u4_or, [] {});
            const uint4 nd = make_uint4(acc.x & ~selfv.x, acc.y & ~selfv.y, acc.z & ~selfv.z, acc.w & ~selfv.w);
            const bool lane_diff = (!REAL && MODE == kModeDense) ? active : (active && (nd.x | nd.y | nd.z | nd.w) != 0u);
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
                if (MODE == kModeSweep && changed) walk_touch_readers(p, row, q);
            }
            if (active && q == 0) c_rows++;
            chw |= pack16(bal) << (16 * h);
        }
        walk_store_bits<REAL>(p, w, chw, lane);
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
