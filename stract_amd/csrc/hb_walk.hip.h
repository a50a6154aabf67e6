// hb_walk.hip.h - what the level kernels of the operators on top of the HyperBall plan share: hb_sampled_harmonic (hb_sample.hip.h, rows
// of 512 source bits, OR as the join) and the forward half of hb_betweenness (hb_betweenness.hip.h, rows of eight path counts, a
// saturating add).  Part of the hb_api.hip translation unit (included after hb_kernels.hip.h; uses its plan layout and quad helpers and
// touch_set of hb_sweep.hip.h).  Host side: hb_api_walk.inc.
//
// A level is one HyperBall pass with another join: the virtual (hub-chunk) rows level by level, then the node rows; a quad per 64-byte
// row, lane q owning bytes 16 q .. 16 q + 15 of every row; a wave owns one 32-row word of the row bitmaps per iteration (two rounds of
// 16 rows) and writes that word whole - no atomics on the bitmaps, no clearing between levels.  Level d reads only the level d - 1
// buffer.  What a set bit means ("the row grew" / "the row is non-zero"), what a row starts from and when it is stored is each kernel's
// own; the parts below are the same text in both.
#pragma once

namespace hbk {

// The mode of a pass or level (hb_pass_stats::mode, the bits of hb_sample_stats::level_modes, the index of
// hb_betweenness_stats::levels_mode); how the host picks one: pass_mode, hb_api_pass.inc.
//   dense:  every source of every row is gathered (no bit test);
//   bitmap: every row is visited, only the sources whose bit is set are gathered;
//   sweep:  only the rows a changed source reaches are visited (touch bitmap from the seed / expand kernels of hb_sweep.hip.h).
enum PassMode : uint32_t { kModeDense = 0, kModeBitmap = 1, kModeSweep = 2 };

struct WalkParams {
    const uint64_t *row_ptr;
    const uint32_t *src;
    uint32_t *bits_rd;        // row bits: node rows = level d - 1, virtual rows = level d (written by this level's launches)
    uint32_t *bits_wr;        // row bits of the node rows at level d
    uint32_t *touch;          // sweep: one bit per work row
    const uint64_t *out_ptr;  // sweep: readers of every work row
    const uint32_t *out_rows;
    const uint32_t *outdeg;   // per node row: out-degree
    unsigned long long *cnt;  // this level's counters: [0] node rows whose bit is set at level d, [1] their out-degree sum (A of the next level);
                              // [2], [3]: the kernel's own
    uint64_t n_pad, rows_total;
    uint64_t row_lo, row_hi;  // rows of this launch (row_lo a multiple of 32)
    int xcd_map;              // as PassParams::xcd_map: workgroup b takes its words from group b % 8
    uint64_t xcd_lo[8], xcd_hi[8];
};

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

// The 32-row words of a launch that wave `wave` of this workgroup walks: w_lo + wid, w_lo + wid + wstride, ... below w_lo + nwords
// (a wave-uniform trip count); rows at or above row_hi do not exist.  XCD-affine launches (virtual rows only) take group blockIdx % 8.
struct WalkSpan {
    uint64_t w_lo, nwords, wid, wstride, row_hi;
};
template <bool REAL>
__device__ __forceinline__ WalkSpan walk_span(const WalkParams &p, int wave)
{
    uint64_t row_lo = p.row_lo, row_hi = p.row_hi;
    uint64_t wid = (uint64_t)blockIdx.x * 4 + wave, wstride = (uint64_t)gridDim.x * 4;
    if (!REAL && p.xcd_map) {
        const int x = blockIdx.x & 7;
        row_lo = p.xcd_lo[x];
        row_hi = p.xcd_hi[x];
        wid = (uint64_t)(blockIdx.x >> 3) * 4 + wave;
        wstride = (uint64_t)(gridDim.x >> 3) * 4; // the grid is a multiple of 8
    }
    return {row_lo >> 5, (row_hi - row_lo + 31) >> 5, wid, wstride, row_hi};
}

// the rows of word w to visit: all of them, or (sweep) its touch word, consumed - the touch bitmap is all-zero again after the level
template <int MODE>
__device__ __forceinline__ uint32_t walk_take_touch(const WalkParams &p, uint64_t w, int lane)
{
    if (MODE != kModeSweep) return 0xFFFFFFFFu;
    const uint32_t tw = __shfl(p.touch[w], 0);
    if (lane == 0 && tw) p.touch[w] = 0;
    return tw;
}

// virtual row vid lives at part[vid - n_pad]: one base for "source id -> row", whichever kind the source is
template <class ROW>
__device__ __forceinline__ const ROW *walk_virtual_base(const ROW *part, uint64_t n_pad)
{
    return part - n_pad * 4;
}

// acc joined with lane q's quarter of every source row of `row` (nothing when !active): node sources from rd, virtual ones from vbase.
// The non-dense modes gather only the sources whose bit is set in bits_rd (node rows: at d - 1; virtual rows: at this level).  Eight
// gathers in flight per quad, a quad-uniform trip count.  on_gather() runs once per gathered row, before the join.
template <int MODE, class ROW, class JOIN, class HOOK>
__device__ __forceinline__ ROW walk_gather(const WalkParams &p, const ROW *rd, const ROW *vbase, uint64_t row, bool active, int q, ROW acc, JOIN join,
                                           HOOK on_gather)
{
    uint64_t beg = 0, end = 0;
    if (active) {
        beg = p.row_ptr[row];
        end = p.row_ptr[row + 1];
    }
    for (uint64_t e = beg; e < end; e += 8) {
        uint32_t i0 = (e + q < end) ? p.src[e + q] : kNone;
        uint32_t i1 = (e + 4 + q < end) ? p.src[e + 4 + q] : kNone;
        if (MODE != kModeDense) {
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
        ROW r[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            r[j] = ROW{};
            if (s[j] != kNone) {
                HB_DBG_ASSERT(s[j] < p.rows_total);
                r[j] = (s[j] < p.n_pad) ? rd[(uint64_t)s[j] * 4 + q] : vbase[(uint64_t)s[j] * 4 + q];
                on_gather();
            }
        }
#pragma unroll
        for (int j = 0; j < 8; j++) acc = join(acc, r[j]);
    }
    return acc;
}

// sweep: a virtual row whose bit is set touches its readers (higher levels / node rows of this level), the quad sharing the list
__device__ __forceinline__ void walk_touch_readers(const WalkParams &p, uint64_t row, int q)
{
    const uint64_t kb = p.out_ptr[row], ke = p.out_ptr[row + 1];
    for (uint64_t k = kb + q; k < ke; k += 4) touch_set(p.touch, p.out_rows[k], p.rows_total);
}

// the word of this level's row bits, whole: node rows in bits_wr, virtual rows in bits_rd (dense levels: nobody reads these, written anyway)
template <bool REAL>
__device__ __forceinline__ void walk_store_bits(const WalkParams &p, uint64_t w, uint32_t word, int lane)
{
    if (lane == 0) {
        if (REAL) p.bits_wr[w] = word;
        else p.bits_rd[w] = word;
    }
}

} // namespace hbk
