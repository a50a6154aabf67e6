// hb_ampc_steps.inc - part of hb_ampc.hip: the steps of a round that work on tables alone - the fold of a distance table into the
// centrality table, update_centralities, and the two edge steps update_counters / update_distances.
extern "C" {

// shared body of hbu_fold_harmonic (n_lanes == 0: `distances` is HBU_KIND_U64) and hbu_fold_harmonic_lanes (HBU_KIND_DIST64, 1 .. 64 lanes)
static int fold_step(hbu_table *distances, hbu_table *centralities, double norm, uint32_t n_lanes, uint32_t flags, uint64_t *folded, uint64_t *inserted)
{
    hbu_table *t = centralities; // the table that changes: its stream runs the fold, its error text reports it
    const bool lanes = n_lanes != 0;
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
    // room for every key of `distances` (each might be new) before the launch
    int rc;
    if ((rc = ensure_room(t, count, true))) return rc;
    unsigned long long *d_counts;
    if ((rc = workspace(t->work, t, [&](Carve &c) { d_counts = c.take<unsigned long long>(2); }))) return rc;
    HBU_HIP(hipStreamSynchronize(distances->stream)); // distances is only read: idle before this table's stream touches it
    unsigned long long h_counts[2] = {0, 0};
    auto run = [&]() -> hipError_t {
        hipError_t e = hipMemsetAsync(d_counts, 0, 2 * sizeof(unsigned long long), t->stream);
        if (e != hipSuccess) return e;
        if (lanes)
            hipLaunchKernelGGL(hbl::fold_lanes_kernel, dim3(grid_for(distances->slots)), dim3(256), 0, t->stream, (const u128 *)distances->d_keys.get(),
                               (const uint32_t *)distances->d_pids.get(), distances->slots, (uint32_t)count, (const uint4 *)distances->d_table.get(), n_lanes, table_of(t),
                               (uint32_t)t->committed, (hbv::Kahan *)t->d_table.get(), norm, flags, d_counts);
        else
            hipLaunchKernelGGL(hbf::fold_distances_kernel, dim3(grid_for(distances->slots)), dim3(256), 0, t->stream, (const u128 *)distances->d_keys.get(),
                               (const uint32_t *)distances->d_pids.get(), distances->slots, (uint32_t)count, (const uint64_t *)distances->d_table.get(), table_of(t),
                               (uint32_t)t->committed, (hbv::Kahan *)t->d_table.get(), norm, flags, d_counts);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = queue_committed(t, t->stream)) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(h_counts, d_counts, sizeof(h_counts), hipMemcpyDeviceToHost, t->stream)) != hipSuccess) return e;
        return hipStreamSynchronize(t->stream);
    };
    const hipError_t e = run();
    if (e != hipSuccess) return rollback(t, e);
    commit(t);
    if (folded) *folded = h_counts[0];
    if (inserted) *inserted = h_counts[1];
    return HB_OK;
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
    const uint64_t staged = nodes_on_device ? 0 : count; // node ids that need room in the work memory
    const hb_u128 *d_nodes;
    hb_u128 *d_keys;
    hbv::Kahan *d_vals;
    unsigned long long *d_count;
    rc = workspace(next_counters->work, t, [&](Carve &c) {
        d_nodes = c.take<hb_u128>(staged);
        d_keys = c.take<hb_u128>(count);
        d_vals = c.take<hbv::Kahan>(count);
        d_count = c.take<unsigned long long>(2);
    });
    if (rc) return fail(next_counters, rc, t->err); // (the table whose buffer it is carries the text too)
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
    HBU_HIP(hipMemcpyAsync(t->h_word.get(), d_count, sizeof(unsigned long long), hipMemcpyDeviceToHost, t->stream));
    HBU_HIP(hipStreamSynchronize(t->stream));
    const uint64_t pairs = t->h_word[0]; // (a count, not a counter or a size: what apply() must know to size its sort)
    uint64_t distinct = 0;
    if ((rc = apply(t, kOpSet, Pairs{d_keys, d_vals, true}, pairs, nullptr, &distinct))) return rc;
    if (written) *written = distinct;
    return HB_OK;
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
        hb_u128 *d_from, *d_to;
        uint32_t *d_src;
        uint16_t *d_jp;
        rc = workspace(prev_counters->work, t, [&](Carve &c) {
            d_from = c.take<hb_u128>(count);
            d_to = c.take<hb_u128>(count);
            d_src = c.take<uint32_t>(count);
            d_jp = c.take<uint16_t>(count);
        });
        if (rc) return fail(prev_counters, rc, t->err); // (the table whose buffer it is carries the text too)
        HBU_HIP(hipStreamSynchronize(prev_counters->stream)); // prev is only read: idle before this table's stream touches it
        HBU_HIP(hipMemcpyAsync(d_from, from, count * sizeof(hb_u128), hipMemcpyHostToDevice, t->stream));
        HBU_HIP(hipMemcpyAsync(d_to, to, count * sizeof(hb_u128), hipMemcpyHostToDevice, t->stream));
        hipLaunchKernelGGL(hbe::counter_sources_kernel, dim3(grid_for(count)), dim3(256), 0, t->stream, (const hb_u128 *)d_from, (uint32_t)count,
                           side_of<uint4>(prev_counters), d_src, d_jp);
        HBU_HIP(hipGetLastError());
        const hbe::CounterSource src{(const uint4 *)prev_counters->d_table.get(), d_src, d_jp};
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
        size_t select_bytes = 0, select_bytes_v = 0;
        {
            const uint8_t *nul = nullptr;
            HBU_HIP(rocprim::select(nullptr, select_bytes, (const hb_u128 *)nullptr, nul, (hb_u128 *)nullptr, (uint32_t *)nullptr, (size_t)count, t->stream.get()));
            HBU_HIP(rocprim::select(nullptr, select_bytes_v, (const uint64_t *)nullptr, nul, (uint64_t *)nullptr, (uint32_t *)nullptr, (size_t)count, t->stream.get()));
            select_bytes = std::max(select_bytes, select_bytes_v);
        }
        // staging lives in prev's work memory, as above: the edges, a candidate and a flag per edge, the compacted (destination,
        // candidate) pairs of the edges that have one, their count
        hb_u128 *d_from, *d_to, *d_keys;
        uint64_t *d_cand, *d_vals;
        uint8_t *d_has;
        uint32_t *d_count;
        char *d_tmp;
        rc = workspace(prev_distances->work, t, [&](Carve &c) {
            d_from = c.take<hb_u128>(count);
            d_to = c.take<hb_u128>(count);
            d_cand = c.take<uint64_t>(count);
            d_has = c.take<uint8_t>(count);
            d_keys = c.take<hb_u128>(count);
            d_vals = c.take<uint64_t>(count);
            d_count = c.take<uint32_t>(2);
            d_tmp = c.take<char>(select_bytes);
        });
        if (rc) return fail(prev_distances, rc, t->err); // (the table whose buffer it is carries the text too)
        HBU_HIP(hipStreamSynchronize(prev_distances->stream));
        HBU_HIP(hipMemcpyAsync(d_from, from, count * sizeof(hb_u128), hipMemcpyHostToDevice, t->stream));
        HBU_HIP(hipMemcpyAsync(d_to, to, count * sizeof(hb_u128), hipMemcpyHostToDevice, t->stream));
        hipLaunchKernelGGL(hbe::distance_candidates_kernel, dim3(grid_for(count)), dim3(256), 0, t->stream, (const hb_u128 *)d_from, (uint32_t)count,
                           side_of<uint64_t>(prev_distances), d_cand, d_has);
        HBU_HIP(hipGetLastError());
        // the edges that have a candidate, batch order kept; only their destinations ever reach next's index
        size_t b = select_bytes;
        HBU_HIP(rocprim::select(d_tmp, b, (const hb_u128 *)d_to, (const uint8_t *)d_has, d_keys, d_count, (size_t)count, t->stream.get()));
        b = select_bytes;
        HBU_HIP(rocprim::select(d_tmp, b, (const uint64_t *)d_cand, (const uint8_t *)d_has, d_vals, d_count + 1, (size_t)count, t->stream.get()));
        t->h_word[0] = 0; // (the copy fills its low half)
        HBU_HIP(hipMemcpyAsync(t->h_word.get(), d_count, sizeof(uint32_t), hipMemcpyDeviceToHost, t->stream));
        HBU_HIP(hipStreamSynchronize(t->stream));
        const uint64_t pairs = t->h_word[0]; // (a count: what apply() must know to size its sort)
        const GroupOut out{keys_out, actions_out};
        uint64_t groups = 0;
        if ((rc = apply(t, HBU_OP_U64_MIN, Pairs{d_keys, d_vals, true}, pairs, nullptr, &groups, &out))) return rc;
        *written = groups;
        return HB_OK;
    });
}

} // extern "C"
