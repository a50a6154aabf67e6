// hb_synth_gpu.hip - the R-MAT generator of hb_synth.cpp on the GPU (bench input support, not the product).
//
// hbs_rmat (host, OpenMP) takes ~70 s for BASELINE configs[3] (2.1 G edges) on a 16-CPU share of a host, and the salted
// record stream of the same graph ~35 s more: two global sorts of 2 G 64-bit keys and 2.5 G random gathers.  This file
// produces the SAME graph and the SAME record stream on the device:
//   draw      raw edge k = rmat_edge(scale, seed, k) (counter-based, hb_synth.cpp), self loops -> ~0
//   reduce    radix sort + unique, rounds of further draws until m_target unique edges exist (hbs_rmat's loop)
//   nodes     touched vertices -> (node_id_of(v), v) sorted by id -> dense index of every vertex
//   edges     keys remapped to (dst dense << 32) | src dense and sorted: row_ptr from the run starts, src = low words
//   stream    hbs_stream_fill's record p as a pure function of (graph, salt, p), written slab by slab into a device buffer and
//             copied to the caller's (page-locked) host buffer
// Only what the record stream needs stays resident: the sorted dense keys (8 B per edge), the ids (16 B per node) and the
// row pointers.  tests/test_gpu.py compares ids, CSR and stream with hb_synth.cpp bit for bit.  Plain R-MAT only (no tail).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>

#include <rocprim/rocprim.hpp>

extern "C" {
typedef struct { uint64_t lo, hi; } hbg_u128;
typedef struct { hbg_u128 from, to; uint64_t rel_flags; } hbg_edge; // == hb_edge (include/hyperball.h)
}

namespace {

using u128 = rocprim::uint128_t;

thread_local std::string g_err;

#define HBG_HIP(x)                                                                                                     \
    do {                                                                                                               \
        hipError_t e_ = (x);                                                                                           \
        if (e_ != hipSuccess) {                                                                                        \
            g_err = std::string(#x) + ": " + hipGetErrorString(e_);                                                    \
            return false;                                                                                              \
        }                                                                                                              \
    } while (0)

__host__ __device__ inline uint64_t splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// hb_synth.cpp: rmat_edge, node_id_of (kept literally equal)
__device__ inline void rmat_edge(int scale, uint64_t seed, uint64_t k, uint32_t *from, uint32_t *to)
{
    uint64_t f = 0, t = 0;
    uint64_t ctr = seed ^ (k * 0xD1342543DE82EF95ull);
    uint64_t bits = 0;
    for (int l = 0; l < scale; l++) {
        if ((l & 3) == 0) bits = splitmix64(ctr + (uint64_t)(l >> 2));
        uint32_t r = (uint32_t)(bits & 0xFFFF);
        bits >>= 16;
        uint32_t fb, tb;
        if (r < 37356u) { fb = 0; tb = 0; }
        else if (r < 49807u) { fb = 0; tb = 1; }
        else if (r < 62259u) { fb = 1; tb = 0; }
        else { fb = 1; tb = 1; }
        f = (f << 1) | fb;
        t = (t << 1) | tb;
    }
    *from = (uint32_t)f;
    *to = (uint32_t)t;
}

constexpr int BLOCK = 256;

inline unsigned grid_for(uint64_t count)
{
    uint64_t b = (count + BLOCK - 1) / BLOCK;
    return (unsigned)(b < 65536 ? (b ? b : 1) : 65536); // grid-stride loops below
}

#define GRID_STRIDE(i, count) \
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < (count); i += (uint64_t)gridDim.x * BLOCK)

__global__ void __launch_bounds__(BLOCK) k_draw(uint64_t *out, uint64_t count, int scale, uint64_t seed, uint64_t d0)
{
    GRID_STRIDE(i, count)
    {
        uint32_t f, t;
        rmat_edge(scale, seed, d0 + i, &f, &t);
        out[i] = (f == t) ? ~0ull : (((uint64_t)t << 32) | f);
    }
}

__global__ void __launch_bounds__(BLOCK) k_touch(const uint64_t *keys, uint64_t m, uint8_t *touched)
{
    GRID_STRIDE(i, m)
    {
        touched[(uint32_t)keys[i]] = 1;
        touched[(uint32_t)(keys[i] >> 32)] = 1;
    }
}

__global__ void __launch_bounds__(BLOCK) k_node_keys(const uint32_t *vert, uint64_t n, u128 *key)
{
    GRID_STRIDE(r, n)
    {
        const uint64_t v = vert[r];
        key[r] = ((u128)splitmix64(2 * v + 1) << 64) | (u128)splitmix64(2 * v + 2); // node_id_of: hi, lo
    }
}

__global__ void __launch_bounds__(BLOCK) k_dense_of(const uint32_t *vert_sorted, uint64_t n, uint32_t *dense_of)
{
    GRID_STRIDE(r, n) dense_of[vert_sorted[r]] = (uint32_t)r;
}

__global__ void __launch_bounds__(BLOCK) k_remap(uint64_t *keys, uint64_t m, const uint32_t *dense_of)
{
    GRID_STRIDE(i, m)
    {
        const uint64_t k = keys[i];
        keys[i] = ((uint64_t)dense_of[(uint32_t)(k >> 32)] << 32) | dense_of[(uint32_t)k];
    }
}

// row_ptr[v] = first edge whose destination is >= v (keys sorted by destination), v in [0, n]
__global__ void __launch_bounds__(BLOCK) k_row_ptr(const uint64_t *keys, uint64_t m, uint64_t n, uint64_t *row_ptr)
{
    GRID_STRIDE(i, m + 1)
    {
        const uint64_t lo = i ? (keys[i - 1] >> 32) + 1 : 0;
        const uint64_t hi = i < m ? (keys[i] >> 32) : n;
        for (uint64_t v = lo; v <= hi && v <= n; v++) row_ptr[v] = i;
    }
}

// ---- the streamed export (hb_synth.cpp: stream_plan / stream_perm / stream_extra / hbs_stream_fill) -------------------
struct Plan {
    uint64_t m, n, full_blocks, len_a, len, mul, add;
};

uint64_t gcd64(uint64_t a, uint64_t b)
{
    while (b) {
        const uint64_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}

Plan stream_plan(uint64_t m, uint64_t n, uint64_t seed, int salt)
{
    Plan p;
    p.m = m;
    p.n = n;
    p.full_blocks = (salt == 2 && p.n >= 4) ? p.m / 15 : 0;
    p.len_a = p.m + p.full_blocks;
    p.len = p.len_a + 2 * p.full_blocks;
    p.mul = 1;
    p.add = 0;
    if (p.m > 2) {
        uint64_t a = (uint64_t)((long double)p.m * 0.6180339887498949L) | 1;
        while (a >= p.m || gcd64(a, p.m) != 1) a = a >= p.m ? 1 : a + 2;
        p.mul = a;
        p.add = splitmix64(seed ^ 0x57EA) % p.m;
    }
    return p;
}

__device__ inline uint64_t stream_perm(const Plan &p, uint64_t c)
{
    if (!p.m) return 0;
    if (p.m <= 0xFFFFFFFFull) return (c * p.mul + p.add) % p.m; // c, mul, add < m < 2^32: no overflow
    return (uint64_t)(((unsigned __int128)c * p.mul + p.add) % p.m);
}

__device__ inline bool in_row(const uint64_t *edges, const uint64_t *row_ptr, uint32_t t, uint32_t f)
{
    uint64_t lo = row_ptr[t], hi = row_ptr[t + 1]; // sources ascending inside the row
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        const uint32_t s = (uint32_t)edges[mid];
        if (s < f) lo = mid + 1;
        else if (s > f) hi = mid;
        else return true;
    }
    return false;
}

__device__ inline bool stream_extra(const uint64_t *edges, const uint64_t *row_ptr, uint64_t seed, const Plan &p, uint64_t j,
                                    uint32_t *from, uint32_t *to)
{
    for (int attempt = 0; attempt < 8; attempt++) {
        const uint64_t h = splitmix64(seed + 0xE17A + j * 0x2545F4914F6CDD1Dull + (uint64_t)attempt * 0x9E3779B97F4A7C15ull);
        const uint32_t f = (uint32_t)(h % p.n), t = (uint32_t)((h >> 32) % p.n);
        if (f == t) continue;
        if (in_row(edges, row_ptr, t, f)) continue;
        *from = f;
        *to = t;
        return true;
    }
    *from = *to = (uint32_t)(splitmix64(j) % p.n);
    return false;
}

__constant__ int c_skipped_bits[12] = {8, 10, 11, 13, 14, 15, 16, 17, 18, 19, 21, 22};
__constant__ int c_harmless_bits[11] = {0, 1, 2, 3, 4, 5, 6, 7, 9, 12, 20};

__global__ void __launch_bounds__(BLOCK) k_stream(const uint64_t *edges, const uint64_t *row_ptr, const hbg_u128 *ids, uint64_t seed,
                                                  Plan p, int salt, uint64_t first, uint64_t count, hbg_edge *out)
{
    GRID_STRIDE(i, count)
    {
        const uint64_t pos = first + i;
        uint32_t f, t;
        uint64_t flags = 0;
        if (pos < p.len_a) {
            const uint64_t b = pos / 16, r = pos % 16;
            if (b < p.full_blocks && r == 15) {
                stream_extra(edges, row_ptr, seed, p, b, &f, &t);
                const uint64_t h = splitmix64(b ^ 0xF1A6);
                flags = (1ull << c_skipped_bits[h % 12]) | ((h & 0x100) ? 1ull << c_harmless_bits[(h >> 16) % 11] : 0);
            } else {
                const uint64_t c = b < p.full_blocks ? 15 * b + r : pos - p.full_blocks;
                const uint64_t key = edges[stream_perm(p, c)];
                f = (uint32_t)key;
                t = (uint32_t)(key >> 32);
                if (salt == 2) {
                    const uint64_t h = splitmix64(c ^ 0xC1EA);
                    if ((h & 7) == 0) flags = 1ull << c_harmless_bits[(h >> 8) % 11];
                }
            }
        } else {
            const uint64_t q = pos - p.len_a, j = q / 2;
            if (q & 1) {
                const bool real = stream_extra(edges, row_ptr, seed, p, j, &f, &t);
                flags = real ? 0 : (1ull << c_skipped_bits[j % 12]);
            } else {
                const uint64_t key = edges[stream_perm(p, (j * 15 + 7) % p.m)];
                f = (uint32_t)key;
                t = (uint32_t)(key >> 32);
                flags = 1ull << c_skipped_bits[splitmix64(j ^ 0xD0B1) % 12];
            }
        }
        hbg_edge e;
        e.from = ids[f];
        e.to = ids[t];
        e.rel_flags = flags;
        out[i] = e;
    }
}

struct TmpBuf {
    void *p = nullptr;
    size_t bytes = 0;
    bool need(size_t b)
    {
        if (b <= bytes) return true;
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
        HBG_HIP(hipMalloc(&p, b));
        bytes = b;
        return true;
    }
    ~TmpBuf()
    {
        if (p) (void)hipFree(p);
    }
};

template <class T> struct Dev {
    T *p = nullptr;
    bool alloc(uint64_t count)
    {
        HBG_HIP(hipMalloc((void **)&p, (count ? count : 1) * sizeof(T)));
        return true;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
    ~Dev() { release(); }
};

} // namespace

struct hbg_graph {
    int device = 0, scale = 0;
    uint64_t seed = 0, n = 0, m = 0, raw_drawn = 0;
    hipStream_t stream = nullptr;
    Dev<uint64_t> edges;    // (dst dense << 32) | src dense, sorted
    Dev<hbg_u128> ids;      // ascending
    Dev<uint64_t> row_ptr;  // n + 1
    Dev<hbg_edge> slab;     // record staging for hbg_stream_fill
    uint64_t slab_cap = 0;
    ~hbg_graph()
    {
        edges.release();
        ids.release();
        row_ptr.release();
        slab.release();
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

// sorted unique 64-bit keys of d_in[0, count) into d_out (may not alias); rocprim::unique in segments of at most 2^30 keys, each
// segment but the first starting one key early (that key was the previous segment's last output: written again, same value)
bool unique_sorted(hbg_graph *g, const uint64_t *d_in, uint64_t *d_out, uint64_t count, uint64_t *n_out, TmpBuf &tmp, Dev<uint64_t> &d_n)
{
    const uint64_t SEG = 1ull << 30;
    uint64_t total = 0;
    for (uint64_t s = 0; s < count; s += SEG) {
        const uint64_t b = s ? s - 1 : 0, e = s + SEG < count ? s + SEG : count;
        uint64_t *dst = d_out + (s ? total - 1 : 0);
        size_t bytes = 0;
        HBG_HIP(rocprim::unique(nullptr, bytes, d_in + b, dst, d_n.p, (size_t)(e - b), rocprim::equal_to<uint64_t>(), g->stream));
        if (!tmp.need(bytes)) return false;
        HBG_HIP(rocprim::unique(tmp.p, bytes, d_in + b, dst, d_n.p, (size_t)(e - b), rocprim::equal_to<uint64_t>(), g->stream));
        uint64_t k = 0;
        HBG_HIP(hipMemcpyAsync(&k, d_n.p, sizeof(k), hipMemcpyDeviceToHost, g->stream));
        HBG_HIP(hipStreamSynchronize(g->stream));
        total += s ? k - 1 : k;
    }
    *n_out = total;
    return true;
}

bool sort_keys(hbg_graph *g, uint64_t *&cur, uint64_t *&alt, uint64_t count, unsigned end_bit, TmpBuf &tmp)
{
    rocprim::double_buffer<uint64_t> db(cur, alt);
    size_t bytes = 0;
    HBG_HIP(rocprim::radix_sort_keys(nullptr, bytes, db, (size_t)count, 0, end_bit, g->stream));
    if (!tmp.need(bytes)) return false;
    HBG_HIP(rocprim::radix_sort_keys(tmp.p, bytes, db, (size_t)count, 0, end_bit, g->stream));
    cur = db.current();
    alt = db.alternate();
    return true;
}

bool build(hbg_graph *g, uint64_t m_target)
{
    const int scale = g->scale;
    const uint64_t seed = g->seed;
    TmpBuf tmp;
    Dev<uint64_t> d_n;
    if (!d_n.alloc(1)) return false;
    // ---- raw draws -> sorted unique non-self keys (vertex space), hbs_rmat's rounds
    Dev<uint64_t> ka, kb; // keys, second buffer of the sort
    uint64_t have = 0, drawn = 0, want = m_target + m_target / 16 + 64;
    for (int round = 0; round < 64; round++) {
        const uint64_t total = have + want;
        Dev<uint64_t> na, nb;
        if (!na.alloc(total) || !nb.alloc(total)) return false;
        if (have) HBG_HIP(hipMemcpyAsync(na.p, ka.p, have * sizeof(uint64_t), hipMemcpyDeviceToDevice, g->stream));
        ka.release();
        kb.release();
        k_draw<<<grid_for(want), BLOCK, 0, g->stream>>>(na.p + have, want, scale, seed, drawn);
        HBG_HIP(hipGetLastError());
        drawn += want;
        uint64_t *cur = na.p, *alt = nb.p;
        if (!sort_keys(g, cur, alt, total, 64, tmp)) return false;
        uint64_t k = 0;
        if (!unique_sorted(g, cur, alt, total, &k, tmp, d_n)) return false;
        if (k) { // one ~0 (self loops) at most, at the end
            uint64_t last = 0;
            HBG_HIP(hipMemcpyAsync(&last, alt + (k - 1), sizeof(last), hipMemcpyDeviceToHost, g->stream));
            HBG_HIP(hipStreamSynchronize(g->stream));
            if (last == ~0ull) k--;
        }
        have = k;
        // unique keys now in `alt`: keep them in ka, the other buffer in kb
        ka.p = alt;
        kb.p = cur;
        na.p = nb.p = nullptr;
        if (have >= m_target) break;
        const uint64_t missing = m_target - have;
        want = missing + missing / 4 + 64;
    }
    g->raw_drawn = drawn;
    const uint64_t m = have;
    // ---- touched vertices -> nodes sorted by NodeID
    const uint64_t space = 1ull << scale;
    uint64_t n = 0;
    Dev<uint32_t> vert;
    {
        Dev<uint8_t> touched;
        if (!touched.alloc(space) || !vert.alloc(space)) return false;
        HBG_HIP(hipMemsetAsync(touched.p, 0, space, g->stream));
        k_touch<<<grid_for(m), BLOCK, 0, g->stream>>>(ka.p, m, touched.p);
        HBG_HIP(hipGetLastError());
        auto iota = rocprim::make_counting_iterator<uint32_t>(0);
        size_t bytes = 0;
        HBG_HIP(rocprim::select(nullptr, bytes, iota, touched.p, vert.p, d_n.p, (size_t)space, g->stream));
        if (!tmp.need(bytes)) return false;
        HBG_HIP(rocprim::select(tmp.p, bytes, iota, touched.p, vert.p, d_n.p, (size_t)space, g->stream));
        HBG_HIP(hipMemcpyAsync(&n, d_n.p, sizeof(n), hipMemcpyDeviceToHost, g->stream));
        HBG_HIP(hipStreamSynchronize(g->stream));
    }
    if (!g->ids.alloc(n)) return false;
    Dev<uint32_t> dense_of;
    {
        Dev<u128> key;
        Dev<uint32_t> vert_sorted;
        if (!key.alloc(n) || !vert_sorted.alloc(n)) return false;
        k_node_keys<<<grid_for(n), BLOCK, 0, g->stream>>>(vert.p, n, key.p);
        HBG_HIP(hipGetLastError());
        u128 *ids = (u128 *)g->ids.p; // (rocprim::uint128_t and {lo, hi} have the same little-endian layout)
        size_t bytes = 0;
        HBG_HIP(rocprim::radix_sort_pairs(nullptr, bytes, key.p, ids, vert.p, vert_sorted.p, (size_t)n, 0, 128, g->stream));
        if (!tmp.need(bytes)) return false;
        HBG_HIP(rocprim::radix_sort_pairs(tmp.p, bytes, key.p, ids, vert.p, vert_sorted.p, (size_t)n, 0, 128, g->stream));
        vert.release();
        if (!dense_of.alloc(space)) return false;
        HBG_HIP(hipMemsetAsync(dense_of.p, 0xFF, space * sizeof(uint32_t), g->stream));
        k_dense_of<<<grid_for(n), BLOCK, 0, g->stream>>>(vert_sorted.p, n, dense_of.p);
        HBG_HIP(hipGetLastError());
        HBG_HIP(hipStreamSynchronize(g->stream));
    }
    // ---- dense keys sorted by (dst, src), row pointers
    k_remap<<<grid_for(m), BLOCK, 0, g->stream>>>(ka.p, m, dense_of.p);
    HBG_HIP(hipGetLastError());
    uint64_t *cur = ka.p, *alt = kb.p;
    if (!sort_keys(g, cur, alt, m, 64, tmp)) return false;
    HBG_HIP(hipStreamSynchronize(g->stream));
    dense_of.release();
    ka.p = cur;
    kb.p = alt;
    kb.release();
    g->edges.p = ka.p;
    ka.p = nullptr;
    if (!g->row_ptr.alloc(n + 1)) return false;
    k_row_ptr<<<grid_for(m + 1), BLOCK, 0, g->stream>>>(g->edges.p, m, n, g->row_ptr.p);
    HBG_HIP(hipGetLastError());
    HBG_HIP(hipStreamSynchronize(g->stream));
    g->n = n;
    g->m = m;
    return true;
}

} // namespace

extern "C" {

const char *hbg_last_error(void) { return g_err.c_str(); }

// The graph hbs_rmat(scale, m_target, seed, *) builds, resident on `device`; NULL on failure (hbg_last_error).
hbg_graph *hbg_rmat(int scale, uint64_t m_target, uint64_t seed, int device)
{
    g_err.clear();
    if (scale < 1 || scale > 31) {
        g_err = "scale must be 1..31";
        return nullptr;
    }
    if (hipSetDevice(device) != hipSuccess) {
        g_err = "hipSetDevice failed";
        return nullptr;
    }
    hbg_graph *g = new hbg_graph();
    g->device = device;
    g->scale = scale;
    g->seed = seed;
    if (hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) != hipSuccess || !build(g, m_target)) {
        if (g_err.empty()) g_err = "hipStreamCreateWithFlags failed";
        delete g;
        return nullptr;
    }
    return g;
}

void hbg_free(hbg_graph *g) { delete g; }
uint64_t hbg_num_nodes(const hbg_graph *g) { return g->n; }
uint64_t hbg_num_edges(const hbg_graph *g) { return g->m; }
uint64_t hbg_raw_drawn(const hbg_graph *g) { return g->raw_drawn; }
uint64_t hbg_stream_len(const hbg_graph *g, int salt) { return stream_plan(g->m, g->n, g->seed, salt).len; }

// what = 0: ids (n x 16 B), 1: row_ptr (n + 1 x 8 B), 2: sorted dense keys (m x 8 B) -> host; 0 on success
int hbg_copy(hbg_graph *g, int what, void *out)
{
    const void *src = what == 0 ? (const void *)g->ids.p : what == 1 ? (const void *)g->row_ptr.p : (const void *)g->edges.p;
    const size_t bytes = what == 0 ? g->n * sizeof(hbg_u128) : what == 1 ? (g->n + 1) * sizeof(uint64_t) : g->m * sizeof(uint64_t);
    if (what < 0 || what > 2) return -1;
    if (hipSetDevice(g->device) != hipSuccess) return -1;
    if (bytes && hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, g->stream) != hipSuccess) return -1;
    return hipStreamSynchronize(g->stream) == hipSuccess ? 0 : -1;
}

// hbs_stream_fill: records first .. first + count of the stream into host memory `out`; returns the number written, ~0 on error
uint64_t hbg_stream_fill(hbg_graph *g, int salt, uint64_t first, uint64_t count, hbg_edge *out)
{
    g_err.clear();
    const Plan p = stream_plan(g->m, g->n, g->seed, salt);
    if (first > p.len) return 0;
    if (count > p.len - first) count = p.len - first;
    if (!count) return 0;
    if (hipSetDevice(g->device) != hipSuccess) return ~0ull;
    const uint64_t CAP = 1ull << 24; // 640 MiB of records per launch
    const uint64_t want = count < CAP ? count : CAP;
    if (g->slab_cap < want) {
        g->slab.release();
        g->slab_cap = 0;
        if (!g->slab.alloc(want)) return ~0ull;
        g->slab_cap = want;
    }
    for (uint64_t done = 0; done < count;) {
        const uint64_t k = count - done < g->slab_cap ? count - done : g->slab_cap;
        k_stream<<<grid_for(k), BLOCK, 0, g->stream>>>(g->edges.p, g->row_ptr.p, g->ids.p, g->seed, p, salt, first + done, k, g->slab.p);
        if (hipGetLastError() != hipSuccess) return ~0ull;
        if (hipMemcpyAsync(out + done, g->slab.p, k * sizeof(hbg_edge), hipMemcpyDeviceToHost, g->stream) != hipSuccess) return ~0ull;
        if (hipStreamSynchronize(g->stream) != hipSuccess) return ~0ull;
        done += k;
    }
    return count;
}

} // extern "C"
