// hb_ampc_round.inc - part of hb_ampc.hip: a worker's resident graph and changed-node filter, and the mapper steps between them and the tables
struct hbu_graph {
    int device = 0;
    DevPtr<hb_u128> d_nodes, d_from, d_to;
    uint64_t n_nodes = 0, n_edges = 0;
    uint64_t chunk = 0; // edges (or nodes) per internal pass
    // staging of one chunk, kept between calls (a round makes the same passes every time); mutable: the steps take the graph as const
    mutable WorkBuf work{"hipMalloc(chunk work memory) failed"};
};

struct hbu_filter {
    int device = 0;
    uint32_t kind = HBU_FILTER_BLOOM;
    uint64_t num_bits = 0;
    uint64_t words = 0; // bloom: 32-bit words allocated = 2 x ceil(num_bits / 64)
    // Members die in reverse order of declaration: the bit vector first, then the carrier (its buffers, its pinned words, its stream last).
    // The carrier is the filter's stream, pinned read-back words and staging memory; for an exact set also its members: the key index of
    // this table (no value is ever stored), `committed` = the members
    Owned<hbu_table> t;
    DevPtr<uint32_t> d_bits; // bloom
};

namespace {
constexpr uint64_t kDefaultChunk = 1ull << 22;
constexpr uint64_t kSetupChunk = 1ull << 20; // nodes per pass of setup_counters: 64 B of counter are staged per node

hbr::Filter filter_view(const hbu_filter *f)
{
    if (!f) return hbr::Filter{hbr::kNoFilter, 0, nullptr, Table{nullptr, nullptr, 0, nullptr}, 0};
    return hbr::Filter{f->kind, (uint32_t)f->num_bits, f->d_bits.get(), table_of(f->t.get()), (uint32_t)f->t->committed};
}
unsigned grid_capped(uint64_t items) { return (unsigned)std::min<uint64_t>(std::max<uint64_t>((items + 255) / 256, 1), 4096); }

// an exact set gets room for `more` new members before a kernel inserts them (the index never grows inside a launch)
int set_reserve(hbu_filter *f, uint64_t more)
{
    return f->kind == HBU_FILTER_EXACT ? ensure_room(f->t.get(), more, false, "too many ids in one exact filter (< 2^32)") : HB_OK;
}
// ... and learns afterwards how many it holds; `stream`: the one the inserting kernel ran on
int set_commit(hbu_filter *f, hipStream_t stream)
{
    hbu_table *t = f->t.get();
    if (f->kind != HBU_FILTER_EXACT) return HB_OK;
    HBU_HIP(queue_committed(t, stream));
    HBU_HIP(hipStreamSynchronize(stream));
    commit(t);
    return HB_OK;
}
// thread's error text for the graph / filter calls (hbu_last_error(NULL))
int refuse(int code, const std::string &msg) { return fail(nullptr, code, msg); }
int filter_fail(hbu_filter *f, int rc) { return refuse(rc, f->t->err); }

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
        HBU_HIP(rocprim::select(nullptr, b, (const hb_u128 *)nullptr, nul, (hb_u128 *)nullptr, (uint32_t *)nullptr, (size_t)chunk, t->stream.get()));
        tmp_bytes = std::max(tmp_bytes, b);
        HBU_HIP(rocprim::select(nullptr, b, (const uint64_t *)nullptr, nul, (uint64_t *)nullptr, (uint32_t *)nullptr, (size_t)chunk, t->stream.get()));
        tmp_bytes = std::max(tmp_bytes, b);
        HBU_HIP(rocprim::select(nullptr, b, (const uint32_t *)nullptr, nul, (uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)chunk, t->stream.get()));
        tmp_bytes = std::max(tmp_bytes, b);
        HBU_HIP(rocprim::select(nullptr, b, (const uint16_t *)nullptr, nul, (uint16_t *)nullptr, (uint32_t *)nullptr, (size_t)chunk, t->stream.get()));
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
    int rc = workspace(g->work, t, [&](Carve &c) {
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
    });
    if (rc) return rc;
    HBU_HIP(hipStreamSynchronize(prev->stream)); // prev and changed are only read: idle before this table's stream touches them
    HBU_HIP(hipStreamSynchronize(changed->t->stream));
    if (new_changed) HBU_HIP(hipStreamSynchronize(new_changed->t->stream));
    HBU_HIP(hipMemsetAsync(d_counts, 0, 4 * sizeof(unsigned long long), t->stream));
    const hbr::Filter in = filter_view(changed);
    uint64_t selected = 0;
    for (uint64_t b = 0; b < g->n_edges; b += chunk) {
        const uint64_t n = std::min<uint64_t>(chunk, g->n_edges - b);
        const hb_u128 *from = g->d_from.get() + b, *to = g->d_to.get() + b;
        size_t tb = tmp_bytes;
        if (DISTANCES) {
            hipLaunchKernelGGL(hbr::select_distance_edges_kernel, dim3(grid_capped(n)), dim3(256), 0, t->stream, from, (uint32_t)n, in, side_of<uint64_t>(prev), d_flag,
                               d_cand, d_counts + 3);
            HBU_HIP(hipGetLastError());
            HBU_HIP(rocprim::select(d_tmp, tb, to, (const uint8_t *)d_flag, d_keys, d_n, (size_t)n, t->stream.get()));
        } else if (LANES) {
            hipLaunchKernelGGL(hbl::select_lane_edges_kernel, dim3(grid_for(n)), dim3(256), 0, t->stream, from, (uint32_t)n, in, side_of<uint4>(prev), d_flag, d_slot);
            HBU_HIP(hipGetLastError());
            HBU_HIP(rocprim::select(d_tmp, tb, to, (const uint8_t *)d_flag, d_keys, d_n, (size_t)n, t->stream.get()));
        } else {
            hipLaunchKernelGGL(hbr::select_counter_edges_kernel, dim3(grid_for(n)), dim3(256), 0, t->stream, from, (uint32_t)n, in, side_of<uint4>(prev), d_flag, d_slot,
                               d_jp);
            HBU_HIP(hipGetLastError());
            HBU_HIP(rocprim::select(d_tmp, tb, to, (const uint8_t *)d_flag, d_keys, d_n, (size_t)n, t->stream.get()));
        }
        t->h_word[0] = 0; // (the copy fills its low half)
        HBU_HIP(hipMemcpyAsync(t->h_word.get(), d_n, sizeof(uint32_t), hipMemcpyDeviceToHost, t->stream));
        HBU_HIP(hipStreamSynchronize(t->stream));
        const uint64_t pairs = t->h_word[0]; // (a count: what apply() must know to size its sort)
        if (!DISTANCES) selected += pairs;
        if (!pairs) continue; // (a chunk that selects nothing has compacted its destinations only)
        // the per-edge words of the selected edges, in the same order (queued in front of apply()'s kernels on the same stream)
        if (DISTANCES) {
            tb = tmp_bytes;
            HBU_HIP(rocprim::select(d_tmp, tb, (const uint64_t *)d_cand, (const uint8_t *)d_flag, d_cand_c, d_n + 1, (size_t)n, t->stream.get()));
        } else {
            tb = tmp_bytes;
            HBU_HIP(rocprim::select(d_tmp, tb, (const uint32_t *)d_slot, (const uint8_t *)d_flag, d_slot_c, d_n + 1, (size_t)n, t->stream.get()));
            if (!LANES) {
                tb = tmp_bytes;
                HBU_HIP(rocprim::select(d_tmp, tb, (const uint16_t *)d_jp, (const uint8_t *)d_flag, d_jp_c, d_n + 2, (size_t)n, t->stream.get()));
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
            const hbl::LaneSource src{(const uint4 *)prev->d_table.get(), d_slot_c};
            Pairs p{d_keys, nullptr, true};
            p.lanes = &src;
            rc = apply(t, HBU_OP_DIST64_MIN, p, pairs, nullptr, nullptr, nullptr, &sink);
        } else {
            const hbe::CounterSource src{(const uint4 *)prev->d_table.get(), d_slot_c, d_jp_c};
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
        int dev = 0;
        const int rc = pick_device(device, &dev);
        if (rc) return rc;
        HBU_HIP(hipSetDevice(dev));
        Owned<hbu_graph> g(new hbu_graph());
        g->device = dev;
        g->n_nodes = n_nodes;
        g->n_edges = n_edges;
        g->chunk = chunk_edges ? chunk_edges : kDefaultChunk;
        hipError_t e = hipSuccess;
        if (n_nodes) e = g->d_nodes.alloc(n_nodes);
        if (e == hipSuccess && n_edges) e = g->d_from.alloc(n_edges);
        if (e == hipSuccess && n_edges) e = g->d_to.alloc(n_edges);
        if (e == hipSuccess && n_nodes) e = hipMemcpy(g->d_nodes.get(), nodes, n_nodes * sizeof(hb_u128), hipMemcpyHostToDevice);
        if (e == hipSuccess && n_edges) e = hipMemcpy(g->d_from.get(), from, n_edges * sizeof(hb_u128), hipMemcpyHostToDevice);
        if (e == hipSuccess && n_edges) e = hipMemcpy(g->d_to.get(), to, n_edges * sizeof(hb_u128), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return refuse(e == hipErrorOutOfMemory ? HB_ERR_NOMEM : HB_ERR_HIP, std::string("upload of the graph: ") + hipGetErrorString(e));
        }
        *out = g.release();
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
    (void)hipSetDevice(g->device); // (a graph has no stream of its own)
    delete g;
}

int hbu_graph_node_sketch(const hbu_graph *g, uint8_t *registers_out)
{
    return guarded(nullptr, [&]() -> int {
        hbu_table *t = nullptr; // (HBU_HIP reports through the thread's error text)
        if (!g || !registers_out) return refuse(HB_ERR_INVALID, "NULL argument");
        HBU_HIP(hipSetDevice(g->device));
        // 4096 words for the maxima, then the bytes; a graph has no stream of its own: the device's default one, and the copy waits for it
        uint32_t *d_words;
        uint8_t *d_bytes;
        const int rc = workspace(g->work, nullptr, [&](Carve &c) {
            d_words = c.take<uint32_t>(HBU_NODE_SKETCH_REGISTERS);
            d_bytes = c.take<uint8_t>(HBU_NODE_SKETCH_REGISTERS);
        });
        if (rc) return rc;
        HBU_HIP(hipMemsetAsync(d_words, 0, HBU_NODE_SKETCH_REGISTERS * sizeof(uint32_t), nullptr));
        if (g->n_nodes) {
            hipLaunchKernelGGL(hbf::node_sketch_kernel, dim3(grid_capped(g->n_nodes)), dim3(256), 0, nullptr, (const hb_u128 *)g->d_nodes.get(), g->n_nodes, d_words);
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
        hbu_table *made = nullptr;
        int rc = create(device, HBU_KIND_F32, 0, 0, &made);
        if (rc) return rc;
        Owned<hbu_table> carrier(made);
        Owned<hbu_filter> f(new hbu_filter());
        f->device = carrier->device;
        f->kind = kind;
        f->t = std::move(carrier);
        if (kind == HBU_FILTER_BLOOM) {
            f->num_bits = num_bits;
            f->words = 2 * ((num_bits + 63) / 64);
            hipError_t e = f->d_bits.alloc(f->words);
            if (e == hipSuccess) e = hipMemsetAsync(f->d_bits.get(), 0, f->words * sizeof(uint32_t), f->t->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(f->t->stream);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                return refuse(e == hipErrorOutOfMemory ? HB_ERR_NOMEM : HB_ERR_HIP, std::string("bit vector: ") + hipGetErrorString(e));
            }
        }
        *out = f.release();
        return HB_OK;
    });
}

void hbu_filter_destroy(hbu_filter *f)
{
    if (!f) return;
    (void)hipSetDevice(f->device);
    if (f->t && f->t->stream) (void)hipStreamSynchronize(f->t->stream);
    delete f;
}

// every filter call: f given, not broken, on its device; the body runs with t = the carrier (HBU_HIP reports on it) and its text is
// copied to the thread's
#define HBU_FILTER_CALL(f, body)                                                       \
    return guarded(nullptr, [&]() -> int {                                             \
        if (!(f)) return refuse(HB_ERR_INVALID, "NULL argument");                      \
        hbu_table *t = (f)->t.get();                                                  \
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
            HBU_HIP(hipMemsetAsync(f->d_bits.get(), 0, f->words * sizeof(uint32_t), t->stream));
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
        hipLaunchKernelGGL(hbr::bloom_fill_kernel, dim3(grid_capped(f->words)), dim3(256), 0, t->stream, f->d_bits.get(), f->words, f->num_bits);
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
        hb_u128 *d_ids;
        if ((rc = workspace(t->work, t, [&](Carve &c) { d_ids = c.take<hb_u128>(count); }))) return rc;
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
        hb_u128 *d_ids;
        uint8_t *d_out;
        const int rc = workspace(t->work, t, [&](Carve &c) {
            d_ids = c.take<hb_u128>(count);
            d_out = c.take<uint8_t>(count);
        });
        if (rc) return rc;
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
            hipLaunchKernelGGL(hbr::bloom_or_kernel, dim3(grid_capped(dst->words)), dim3(256), 0, t->stream, dst->d_bits.get(), (const uint32_t *)src->d_bits.get(), dst->words);
            HBU_HIP(hipGetLastError());
            HBU_HIP(hipStreamSynchronize(t->stream));
            return HB_OK;
        }
        if (!src->t->committed) return HB_OK;
        int rc = set_reserve(dst, src->t->committed);
        if (rc) return rc;
        hipLaunchKernelGGL(hbr::set_union_kernel, dim3(grid_for(src->t->slots)), dim3(256), 0, t->stream, (const u128 *)src->t->d_keys.get(), (const uint32_t *)src->t->d_pids.get(),
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
        unsigned long long *d_sum = t->d_next.get() + 1; // (the second word of the index counter's allocation: a bloom filter has no index)
        HBU_HIP(hipMemsetAsync(d_sum, 0, sizeof(unsigned long long), t->stream));
        hipLaunchKernelGGL(hbr::bloom_popcount_kernel, dim3(grid_capped(f->words)), dim3(256), 0, t->stream, (const uint32_t *)f->d_bits.get(), f->words, d_sum);
        HBU_HIP(hipGetLastError());
        HBU_HIP(hipMemcpyAsync(t->h_word.get(), d_sum, sizeof(unsigned long long), hipMemcpyDeviceToHost, t->stream));
        HBU_HIP(hipStreamSynchronize(t->stream));
        *n = t->h_word[0];
        return HB_OK;
    });
}

int hbu_filter_export_bits(hbu_filter *f, uint64_t *words_out)
{
    HBU_FILTER_CALL(f, {
        if (f->kind != HBU_FILTER_BLOOM) return fail(t, HB_ERR_INVALID, "only a bloom filter has bits");
        if (!words_out) return fail(t, HB_ERR_INVALID, "NULL argument");
        HBU_HIP(hipMemcpyAsync(words_out, f->d_bits.get(), f->words * sizeof(uint32_t), hipMemcpyDeviceToHost, t->stream));
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
        HBU_HIP(hipMemcpyAsync(f->d_bits.get(), words, f->words * sizeof(uint32_t), hipMemcpyHostToDevice, t->stream));
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
        hb_u128 *d_out;
        const int rc = workspace(t->work, t, [&](Carve &c) { d_out = c.take<hb_u128>(t->committed); });
        if (rc) return rc;
        hipLaunchKernelGGL(hbr::set_export_kernel, dim3(grid_for(t->slots)), dim3(256), 0, t->stream, (const u128 *)t->d_keys.get(), (const uint32_t *)t->d_pids.get(), t->slots,
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
        uint4 *d_vals;
        if ((rc = workspace(g->work, t, [&](Carve &c) { d_vals = c.take<uint4>(chunk * 4); }))) return rc;
        if (changed) HBU_HIP(hipStreamSynchronize(changed->t->stream));
        for (uint64_t b = 0; b < g->n_nodes; b += chunk) {
            const uint64_t n = std::min<uint64_t>(chunk, g->n_nodes - b);
            const hb_u128 *nodes = g->d_nodes.get() + b;
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

// what the three edge rounds share: the refusals, the kinds (both tables of `kind`, or kinds_msg) and the run; c = the counts of round_edges
static int round_call(RoundMode mode, uint32_t kind, const char *kinds_msg, hbu_table *prev, hbu_table *t, const hbu_graph *g, hbu_filter *changed,
                      hbu_filter *new_changed, uint64_t c[4])
{
    std::fill(c, c + 4, 0);
    return guarded(t, [&]() -> int {
        const int rc = round_refusal({prev}, t, g, changed, new_changed, true);
        if (rc) return rc;
        if (prev->kind != kind || t->kind != kind) return fail(t, HB_ERR_INVALID, kinds_msg);
        if (!g->n_edges) return HB_OK;
        HBU_HIP(hipSetDevice(t->device));
        switch (mode) {
        case kRoundCounters: return round_edges<kRoundCounters>(prev, t, g, changed, new_changed, c);
        case kRoundDistances: return round_edges<kRoundDistances>(prev, t, g, changed, new_changed, c);
        default: return round_edges<kRoundLanes>(prev, t, g, changed, new_changed, c);
        }
    });
}

int hbu_round_counters(hbu_table *prev_counters, hbu_table *next_counters, const hbu_graph *g, hbu_filter *changed, hbu_filter *new_changed, uint64_t *selected,
                       uint64_t *merged, uint64_t *inserted)
{
    uint64_t c[4];
    const int rc = round_call(kRoundCounters, HBU_KIND_HLL64, "round_counters needs two HyperLogLog<64> tables", prev_counters, next_counters, g, changed, new_changed, c);
    if (selected) *selected = c[0];
    if (merged) *merged = c[1];
    if (inserted) *inserted = c[2];
    return rc;
}

int hbu_round_distances(hbu_table *prev_distances, hbu_table *next_distances, const hbu_graph *g, hbu_filter *changed, hbu_filter *new_changed, uint64_t *selected,
                        uint64_t *changed_nodes)
{
    uint64_t c[4];
    const int rc = round_call(kRoundDistances, HBU_KIND_U64, "round_distances needs two u64 tables", prev_distances, next_distances, g, changed, new_changed, c);
    if (selected) *selected = c[0];
    if (changed_nodes) *changed_nodes = c[1] + c[2];
    return rc;
}

int hbu_round_lane_distances(hbu_table *prev, hbu_table *next, const hbu_graph *g, hbu_filter *changed, hbu_filter *new_changed, uint64_t *selected, uint64_t *merged,
                             uint64_t *inserted)
{
    uint64_t c[4];
    const int rc = round_call(kRoundLanes, HBU_KIND_DIST64, "round_lane_distances needs two 64-lane distance tables", prev, next, g, changed, new_changed, c);
    if (selected) *selected = c[0];
    if (merged) *merged = c[1];
    if (inserted) *inserted = c[2];
    return rc;
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
        HBU_HIP(rocprim::select(nullptr, tmp_bytes, (const hb_u128 *)nullptr, (const uint8_t *)nullptr, (hb_u128 *)nullptr, (uint32_t *)nullptr, (size_t)chunk, t->stream.get()));
        uint8_t *d_flag;
        hb_u128 *d_sel;
        uint32_t *d_n;
        char *d_tmp;
        rc = workspace(g->work, t, [&](Carve &c) {
            d_flag = c.take<uint8_t>(chunk);
            d_sel = c.take<hb_u128>(chunk);
            d_n = c.take<uint32_t>(2);
            d_tmp = c.take<char>(tmp_bytes);
        });
        if (rc) return rc;
        HBU_HIP(hipStreamSynchronize(changed->t->stream));
        const hbr::Filter in = filter_view(changed);
        uint64_t sel_total = 0, written_total = 0;
        for (uint64_t b = 0; b < g->n_nodes; b += chunk) {
            const uint64_t n = std::min<uint64_t>(chunk, g->n_nodes - b);
            hipLaunchKernelGGL(hbr::select_nodes_kernel, dim3(grid_for(n)), dim3(256), 0, t->stream, (const hb_u128 *)(g->d_nodes.get() + b), (uint32_t)n, in, d_flag);
            HBU_HIP(hipGetLastError());
            size_t tb = tmp_bytes;
            HBU_HIP(rocprim::select(d_tmp, tb, (const hb_u128 *)(g->d_nodes.get() + b), (const uint8_t *)d_flag, d_sel, d_n, (size_t)n, t->stream.get()));
            t->h_word[0] = 0;
            HBU_HIP(hipMemcpyAsync(t->h_word.get(), d_n, sizeof(uint32_t), hipMemcpyDeviceToHost, t->stream));
            HBU_HIP(hipStreamSynchronize(t->stream));
            const uint64_t picked = t->h_word[0];
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
