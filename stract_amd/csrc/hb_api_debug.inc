// hb_api_debug.inc - part of the hb_api.hip translation unit (included there; uses its hb_ctx and helpers).
// Test / bench-only exports (inside the extern "C" block of hb_api.hip): state copies, host-only planner / ingest, logical-rank exchange.
// ---- debug exports ------------------------------------------------------------------------
int hb_debug_copy_registers(hb_ctx *c, uint8_t *out)
{
    return guarded(c, [&]() -> int {
        if (!c || !out) return HB_ERR_INVALID;
        if (c->rows != RowsOf::HyperBall) return fail(c, HB_ERR_INVALID, "call hb_begin first");
        int rc = set_device(c);
        if (rc) return rc;
        if ((rc = ensure_initial_state(c))) return rc;
        const uint64_t n = c->plan.n;
        if (!n) return HB_OK;
        DevPtr<uint4> tmp;
        HB_HIP(tmp.alloc(n * 4));
        unsigned blocks = (unsigned)((n * 4 + 255) / 256);
        hipLaunchKernelGGL(hbk::gather_rows_kernel, dim3(blocks), dim3(256), 0, c->stream, (const uint4 *)c->d_regs[c->cur],
                           (const uint32_t *)c->d_dev_of, n, tmp.get());
        HB_HIP_AS("", hipMemcpyAsync(out, tmp.get(), n * 64, hipMemcpyDeviceToHost, c->stream));
        HB_HIP_AS("", hipStreamSynchronize(c->stream));
        return HB_OK;
    });
}

// the saturated rows of the run in progress (DESIGN.md section 38): U, and the bitmap unpacked to one byte per node (input order) /
// per hub chunk (plan order); of the last dense pass: the work rows that left their gather loop early, and whether it ran the EARLY
// instances at all (DESIGN.md section 39)
int hb_debug_saturation(hb_ctx *c, uint64_t info[5], uint8_t *u, uint8_t *node_bits, uint8_t *virt_bits)
{
    return guarded(c, [&]() -> int {
        if (!c || !info) return HB_ERR_INVALID;
        if (!c->loaded) return fail(c, HB_ERR_INVALID, "hb_debug_saturation: no graph loaded");
        int rc = set_device(c);
        if (rc) return rc;
        const Plan &p = c->plan;
        info[0] = (c->d_sat != nullptr && !unfused(c) && !linked(c)) ? 1 : 0;
        info[1] = p.n;
        info[2] = p.nv;
        info[3] = info[4] = 0;
        if (!info[0]) return HB_OK;
        if (c->last_dense_early) {
            unsigned long long he[hbk::kStripes];
            HB_HIP(hipMemcpyAsync(he, c->d_early, sizeof(he), hipMemcpyDeviceToHost, c->stream));
            HB_HIP(hipStreamSynchronize(c->stream));
            for (int s = 0; s < hbk::kStripes; s++) info[3] += he[s];
            info[4] = 1;
        }
        if ((rc = need_host_dev_of(c))) return rc;
        uint32_t hu[64];
        std::vector<uint32_t> words(c->bits_words);
        HB_HIP(hipMemcpyAsync(hu, c->d_sat_u, sizeof(hu), hipMemcpyDeviceToHost, c->stream));
        HB_HIP(hipMemcpyAsync(words.data(), c->d_sat, words.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HB_HIP(hipStreamSynchronize(c->stream));
        auto bit = [&](uint64_t row) { return (uint8_t)((words[row >> 5] >> (row & 31u)) & 1u); };
        if (u)
            for (int k = 0; k < 64; k++) u[k] = (uint8_t)hu[k];
        if (node_bits)
            for (uint64_t s = 0; s < p.n; s++) node_bits[s] = bit(p.dev_of[s]);
        if (virt_bits)
            for (uint64_t v = 0; v < p.nv; v++) virt_bits[v] = bit(p.n_pad + v);
        return HB_OK;
    });
}

int hb_debug_copy_kahan(hb_ctx *c, double *sum, double *err)
{
    return guarded(c, [&]() -> int {
        if (!c) return HB_ERR_INVALID;
        if (c->rows != RowsOf::HyperBall) return fail(c, HB_ERR_INVALID, "call hb_begin first");
        int rc = set_device(c);
        if (rc) return rc;
        if ((rc = ensure_initial_state(c))) return rc;
        if ((rc = need_host_dev_of(c))) return rc;
        const Plan &p = c->plan;
        std::vector<double> tmp(p.n_pad ? p.n_pad : 1);
        for (int k = 0; k < 2; k++) {
            double *dst = k ? err : sum;
            if (!dst || !p.n_pad) continue;
            HB_HIP(hipMemcpyAsync(tmp.data(), k ? c->d_kerr : c->d_ksum, p.n_pad * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            HB_HIP(hipStreamSynchronize(c->stream));
            for (uint64_t sid = 0; sid < p.n; sid++) dst[sid] = tmp[p.dev_of[sid]];
        }
        return HB_OK;
    });
}

int hb_debug_copy_sizes(hb_ctx *c, uint64_t *out)
{
    return guarded(c, [&]() -> int {
        if (!c || !out) return HB_ERR_INVALID;
        if (c->rows != RowsOf::HyperBall) return fail(c, HB_ERR_INVALID, "call hb_begin first");
        int rc = set_device(c);
        if (rc) return rc;
        if ((rc = ensure_initial_state(c))) return rc;
        if ((rc = need_host_dev_of(c))) return rc;
        const Plan &p = c->plan;
        if (!p.n_pad) return HB_OK;
        std::vector<uint64_t> tmp(p.n_pad);
        HB_HIP(hipMemcpyAsync(tmp.data(), c->d_size, p.n_pad * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        HB_HIP(hipStreamSynchronize(c->stream));
        for (uint64_t sid = 0; sid < p.n; sid++) out[sid] = tmp[p.dev_of[sid]];
        return HB_OK;
    });
}

int hb_debug_hll_size(hb_ctx *c, const uint8_t *regs, uint64_t count, uint64_t *out)
{
    return guarded(c, [&]() -> int {
        if (!c || (count && (!regs || !out))) return HB_ERR_INVALID;
        int rc = set_device(c);
        if (rc) return rc;
        if (!count) return HB_OK;
        // tables may not be on the device yet (no graph loaded): stage private copies
        DevPtr<double> d_raw, d_bias;
        DevPtr<uint8_t> d_lc, d_regs;
        DevPtr<uint64_t> d_out;
        uint8_t lc[68];
        if (!build_lc_table(lc)) return fail(c, HB_ERR_INVALID, "linear-counting table not robust on this libm");
        const uint64_t rows_pad = (count + 15) & ~15ull;
        HB_HIP_AS("", d_raw.alloc(HLL64_TABLE_LEN));
        HB_HIP_AS("", d_bias.alloc(HLL64_TABLE_LEN));
        HB_HIP_AS("", d_lc.alloc(256));
        HB_HIP_AS("", d_regs.alloc(rows_pad * 64));
        HB_HIP_AS("", d_out.alloc(rows_pad));
        HB_HIP_AS("", hipMemcpyAsync(d_raw.get(), HLL64_RAW_ESTIMATE, sizeof(HLL64_RAW_ESTIMATE), hipMemcpyHostToDevice, c->stream));
        HB_HIP_AS("", hipMemcpyAsync(d_bias.get(), HLL64_BIAS, sizeof(HLL64_BIAS), hipMemcpyHostToDevice, c->stream));
        HB_HIP_AS("", hipMemcpyAsync(d_lc.get(), lc, 68, hipMemcpyHostToDevice, c->stream));
        HB_HIP_AS("", hipMemcpyAsync(d_regs.get(), regs, count * 64, hipMemcpyHostToDevice, c->stream));
        unsigned blocks = (unsigned)((rows_pad * 4 + 255) / 256);
        hipLaunchKernelGGL(hbk::hll_size_kernel, dim3(blocks), dim3(256), 0, c->stream, (const uint4 *)d_regs.get(), count, d_out.get(),
                           (const double *)d_raw.get(), (const double *)d_bias.get(), (const uint8_t *)d_lc.get());
        HB_HIP_AS("", hipGetLastError());
        HB_HIP_AS("", hipMemcpyAsync(out, d_out.get(), count * 8, hipMemcpyDeviceToHost, c->stream));
        HB_HIP_AS("", hipStreamSynchronize(c->stream));
        return HB_OK;
    });
}

// pack -> maximum over the pieces -> unpack on arbitrary rows, each launch timed (the unit-test and measurement door of the
// HB_FLAG_PACKED_WIRE kernels); rows == NULL: every piece is the resident counters of the run in progress
int hb_debug_wire6(hb_ctx *c, const uint8_t *rows, uint64_t count, uint32_t pieces, uint8_t *packed_max, uint8_t *rows_out, float ms[3])
{
    return guarded(c, [&]() -> int {
        if (!c || !pieces) return HB_ERR_INVALID;
        if (count >= (1ull << 40) / pieces) return fail(c, HB_ERR_LIMIT, "hb_debug_wire6: too many rows");
        int rc = set_device(c);
        if (rc) return rc;
        if (ms) ms[0] = ms[1] = ms[2] = 0.f;
        if (!count) return HB_OK;
        const uint4 *src = nullptr;
        DevPtr<uint4> d_rows, d_out;
        DevPtr<uint32_t> d_packed, d_max;
        if (rows) {
            HB_HIP_AS("", d_rows.alloc((uint64_t)pieces * count * 4));
            HB_HIP_AS("", hipMemcpyAsync(d_rows.get(), rows, (uint64_t)pieces * count * 64, hipMemcpyHostToDevice, c->stream));
            src = d_rows.get();
        } else {
            if (c->rows != RowsOf::HyperBall) return fail(c, HB_ERR_INVALID, "hb_debug_wire6 without rows: call hb_begin first");
            if (count > c->plan.n_pad) return fail(c, HB_ERR_INVALID, "hb_debug_wire6 without rows: count exceeds the padded row count");
            if ((rc = ensure_initial_state(c))) return rc;
            src = c->d_regs[c->cur];
        }
        HB_HIP_AS("", d_packed.alloc((uint64_t)pieces * count * 12));
        HB_HIP_AS("", d_max.alloc(count * 12));
        HB_HIP_AS("", d_out.alloc(count * 4));
        hipEvent_t *E = c->ev; // (no pass is in flight inside a debug call: kEvStart .. kEvMerge mark the four instants)
        HB_HIP(hipEventRecord(E[kEvStart], c->stream));
        if (rows) {
            hipLaunchKernelGGL(hbk::pack6_rows_kernel, dim3(wire6_blocks(c, (uint64_t)pieces * count)), dim3(256), 0, c->stream, src, (uint64_t)pieces * count, (uint64_t)pieces * count, d_packed.get());
        } else {
            for (uint32_t k = 0; k < pieces; k++)
                hipLaunchKernelGGL(hbk::pack6_rows_kernel, dim3(wire6_blocks(c, count)), dim3(256), 0, c->stream, src, count, count, d_packed.get() + (uint64_t)k * count * 12);
        }
        HB_HIP(hipEventRecord(E[kEvLevel1], c->stream));
        hipLaunchKernelGGL(hbk::max6_pieces_kernel, dim3(wire6_blocks(c, count)), dim3(256), 0, c->stream, (const uint32_t *)d_packed.get(), count * 12, pieces, count, d_max.get());
        HB_HIP(hipEventRecord(E[kEvLevels], c->stream));
        hipLaunchKernelGGL(hbk::unpack6_rows_kernel, dim3(wire6_blocks(c, count)), dim3(256), 0, c->stream, (const uint32_t *)d_max.get(), count, d_out.get());
        HB_HIP(hipEventRecord(E[kEvMerge], c->stream));
        HB_HIP(hipGetLastError());
        if (packed_max) HB_HIP_AS("", hipMemcpyAsync(packed_max, d_max.get(), count * 48, hipMemcpyDeviceToHost, c->stream));
        if (rows_out) HB_HIP_AS("", hipMemcpyAsync(rows_out, d_out.get(), count * 64, hipMemcpyDeviceToHost, c->stream));
        HB_HIP_AS("", hipStreamSynchronize(c->stream));
        if (ms) {
            HB_HIP(hipEventElapsedTime(&ms[0], E[kEvStart], E[kEvLevel1]));
            HB_HIP(hipEventElapsedTime(&ms[1], E[kEvLevel1], E[kEvLevels]));
            HB_HIP(hipEventElapsedTime(&ms[2], E[kEvLevels], E[kEvMerge]));
        }
        return HB_OK;
    });
}

int hb_debug_state_hash(hb_ctx *c, uint64_t out[2])
{
    return guarded(c, [&]() -> int {
        if (!c || !out) return HB_ERR_INVALID;
        if (c->rows != RowsOf::HyperBall) return fail(c, HB_ERR_INVALID, "call hb_begin first");
        int rc = set_device(c);
        if (rc) return rc;
        if ((rc = ensure_initial_state(c))) return rc;
        out[0] = out[1] = 0;
        const uint64_t n = c->plan.n;
        if (!n) return HB_OK;
        unsigned long long *cnt = c->d_counters + (size_t)c->max_passes * hbk::kCounterWords; // the spare slot
        HB_HIP(hipMemsetAsync(cnt, 0, hbk::kCounterWords * sizeof(unsigned long long), c->stream));
        const unsigned blocks = grid_blocks(c, (n + 255) / 256, 8);
        hipLaunchKernelGGL(hbk::state_hash_kernel, dim3(blocks), dim3(256), 0, c->stream, (const uint4 *)c->d_regs[c->cur],
                           (const double *)c->d_ksum, (const double *)c->d_kerr, (const uint32_t *)c->d_dev_of, n, cnt);
        HB_HIP(hipGetLastError());
        std::vector<unsigned long long> h(hbk::kCounterWords);
        HB_HIP(hipMemcpyAsync(h.data(), cnt, hbk::kCounterWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HB_HIP(hipStreamSynchronize(c->stream));
        for (int s = 0; s < hbk::kStripes; s++) {
            out[0] += h[4 * s];
            out[1] += h[4 * s + 1];
        }
        if (multi_rank(c)) out[1] = 0; // a rank holds the Kahan state of its own rows only
        return HB_OK;
    });
}

int hb_debug_copy_graph(hb_ctx *c, hb_u128 *ids, uint64_t *row_ptr, uint32_t *src)
{
    return guarded(c, [&]() -> int {
        if (!c) return HB_ERR_INVALID;
        if (!c->loaded) return fail(c, HB_ERR_INVALID, "no graph loaded");
        const uint64_t n = c->g.ids.size();
        if ((row_ptr || src) && c->g.row_ptr.size() != n + 1)
            return fail(c, HB_ERR_LIMIT, "the reduced graph is kept on the host only up to 2^26 edges (or with HB_FLAG_HOST_PLAN)");
        if (ids && n) std::memcpy(ids, c->g.ids.data(), n * sizeof(hb_u128));
        if (row_ptr) std::memcpy(row_ptr, c->g.row_ptr.data(), (n + 1) * sizeof(uint64_t));
        if (src && !c->g.src.empty()) std::memcpy(src, c->g.src.data(), c->g.src.size() * sizeof(uint32_t));
        return HB_OK;
    });
}

int hb_debug_copy_plan(hb_ctx *c, uint64_t sizes[4], uint32_t *order, uint64_t *plan_row_ptr, uint32_t *plan_src, uint64_t *level_begin)
{
    return guarded(c, [&]() -> int {
        if (!c || !sizes) return HB_ERR_INVALID;
        if (!c->loaded) return fail(c, HB_ERR_INVALID, "no graph loaded");
        int rc = set_device(c);
        if (rc) return rc;
        const Plan &p = c->plan;
        const uint64_t rows_total = p.n_pad + p.nv;
        sizes[0] = p.n_pad;
        sizes[1] = p.nv;
        sizes[2] = c->plan_entries;
        sizes[3] = p.level_begin.size() ? p.level_begin.size() - 1 : 0;
        if (order && p.n_pad) HB_HIP(hipMemcpyAsync(order, c->d_sid_of, p.n_pad * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        if (plan_row_ptr) HB_HIP(hipMemcpyAsync(plan_row_ptr, c->d_row_ptr, (rows_total + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        if (plan_src && c->plan_entries)
            HB_HIP(hipMemcpyAsync(plan_src, c->d_src, c->plan_entries * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HB_HIP(hipStreamSynchronize(c->stream));
        if (level_begin) std::memcpy(level_begin, p.level_begin.data(), p.level_begin.size() * sizeof(uint64_t));
        return HB_OK;
    });
}

int hb_host_ingest(const hb_u128 *node_ids, uint64_t n, const hb_edge *edges, uint64_t m, uint64_t *n_out,
                   uint64_t *m_unique, uint64_t *m_eff, hb_u128 *ids, uint64_t *row_ptr, uint32_t *src)
{
    return guarded(nullptr, [&]() -> int {
        hb_ctx *c = nullptr;
        DenseGraph g;
        std::string e = ingest_edges(node_ids, n, edges, m, &g);
        if (!e.empty()) return fail(c, HB_ERR_INVALID, e);
        const uint64_t nn = g.ids.size();
        if (n_out) *n_out = nn;
        if (m_unique) *m_unique = g.m_unique;
        if (m_eff) *m_eff = g.src.size();
        if (ids && nn) std::memcpy(ids, g.ids.data(), nn * sizeof(hb_u128));
        if (row_ptr) std::memcpy(row_ptr, g.row_ptr.data(), (nn + 1) * sizeof(uint64_t));
        if (src && !g.src.empty()) std::memcpy(src, g.src.data(), g.src.size() * sizeof(uint32_t));
        return HB_OK;
    });
}

// the host planner as hb_host_plan / hb_host_plan_live call it; "" or build_plan's error text
static std::string host_plan_of(uint64_t n, const uint64_t *row_ptr, const uint32_t *src, uint32_t flags, uint32_t chunk, const uint32_t *tune, Plan *p)
{
    std::vector<uint32_t> outdeg;
    const bool reorder = !(flags & HB_FLAG_NO_REORDER);
    static const uint64_t zero = 0;
    if (n == 0) row_ptr = &zero;
    if (reorder) count_out_degree(row_ptr, src, n, &outdeg);
    PlanTune pt = plan_tune(chunk, tune);
    if (tune && tune[7] > 1) pt.world = tune[7]; // destination-partition layout (test hook)
    pt.xcd_map = !(flags & HB_FLAG_NO_XCD_MAP);
    pt.live_first = live_first_by_flags(flags, n) && !(flags & HB_FLAG_DEST_PARTITION); // (build_plan ignores it with owner slices)
    return build_plan(n, row_ptr, src, outdeg, reorder, pt, p);
}

int hb_host_plan_live(uint64_t n, const uint64_t *row_ptr, const uint32_t *src, uint32_t flags, uint32_t chunk, const uint32_t *tune, uint64_t live[3])
{
    return guarded(nullptr, [&]() -> int {
        hb_ctx *c = nullptr;
        if (!live || (n && !row_ptr)) return fail(c, HB_ERR_INVALID, "NULL argument");
        Plan p;
        const std::string e = host_plan_of(n, row_ptr, src, flags, chunk, tune, &p);
        if (!e.empty()) return fail(c, HB_ERR_LIMIT, e);
        live[0] = p.live_first ? 1 : 0;
        live[1] = p.n_live;
        live[2] = p.n_live_pad;
        return HB_OK;
    });
}

int hb_debug_plan_live(hb_ctx *c, uint64_t live[3])
{
    return guarded(c, [&]() -> int {
        if (!c || !live) return HB_ERR_INVALID;
        if (!c->loaded) return fail(c, HB_ERR_INVALID, "hb_debug_plan_live: no graph loaded");
        live[0] = c->plan.live_first ? 1 : 0;
        live[1] = c->plan.n_live;
        live[2] = c->plan.n_live_pad;
        return HB_OK;
    });
}

int hb_host_plan(uint64_t n, const uint64_t *row_ptr, const uint32_t *src, uint32_t flags, uint32_t chunk,
                 const uint32_t *tune, uint64_t sizes[4], uint32_t *order, uint64_t *plan_row_ptr, uint32_t *plan_src,
                 uint64_t *level_begin)
{
    return guarded(nullptr, [&]() -> int {
        hb_ctx *c = nullptr;
        if (!sizes || (n && !row_ptr)) return fail(c, HB_ERR_INVALID, "NULL argument");
        Plan p;
        std::string e = host_plan_of(n, row_ptr, src, flags, chunk, tune, &p);
        if (!e.empty()) return fail(c, HB_ERR_LIMIT, e);
        sizes[0] = p.n_pad;
        sizes[1] = p.nv;
        sizes[2] = p.src.size();
        sizes[3] = p.level_begin.size() ? p.level_begin.size() - 1 : 0;
        if (order && p.n_pad) std::memcpy(order, p.order.data(), p.n_pad * sizeof(uint32_t));
        if (plan_row_ptr) std::memcpy(plan_row_ptr, p.row_ptr.data(), p.row_ptr.size() * sizeof(uint64_t));
        if (plan_src && !p.src.empty()) std::memcpy(plan_src, p.src.data(), p.src.size() * sizeof(uint32_t));
        if (level_begin) std::memcpy(level_begin, p.level_begin.data(), p.level_begin.size() * sizeof(uint64_t));
        return HB_OK;
    });
}

int hb_debug_tail_index(uint64_t n, const hb_u128 *sorted_ids, const uint32_t *dev_of, uint64_t n_pad, const hb_edge *records,
                        uint64_t count, uint64_t *ptr_out, uint32_t *to_out, uint64_t to_cap, uint64_t *to_len)
{
    return guarded(nullptr, [&]() -> int {
        hb_ctx *c = nullptr;
        if ((n && (!sorted_ids || !dev_of)) || (count && !records) || !ptr_out || !to_len) return fail(c, HB_ERR_INVALID, "NULL argument");
        TailIndex *tix = n ? tail_index_build(sorted_ids, n) : nullptr;
        std::vector<uint64_t> keys, ptr;
        std::vector<uint32_t> to;
        std::vector<TailDoc> open; // the records are one segment in doc order
        std::string e = tail_collect(tix, n, records, count, &open);
        if (e.empty()) e = tail_close_segment(tix, sorted_ids, dev_of, &open, &keys);
        tail_index_free(tix);
        if (e.empty()) e = build_tail_csr(&keys, n_pad, &ptr, &to);
        if (!e.empty()) return fail(c, HB_ERR_NOMEM, e);
        std::memcpy(ptr_out, ptr.data(), (n_pad + 1) * sizeof(uint64_t));
        *to_len = to.size();
        if (to_out && !to.empty()) std::memcpy(to_out, to.data(), std::min<uint64_t>(to.size(), to_cap) * sizeof(uint32_t));
        return HB_OK;
    });
}

int hb_debug_exchange(hb_ctx **ctxs, int count, int phase)
{
    return guarded(nullptr, [&]() -> int {
        if (!ctxs || count < 1 || !ctxs[0]) return HB_ERR_INVALID;
        hb_ctx *c = ctxs[0];
        for (int i = 0; i < count; i++) {
            hb_ctx *o = ctxs[i];
            if (!o) return fail(c, HB_ERR_INVALID, "NULL context");
            if (o->plan.n_pad != c->plan.n_pad || o->device != c->device || dest_mode(o) != dest_mode(c))
                return fail(c, HB_ERR_INVALID, "contexts differ in size, device or partition mode");
            if (phase == 0 && !o->pending_local)
                return fail(c, HB_ERR_INVALID, "every context must be between hb_step_local and hb_step_finish");
            if (dest_mode(c) && (o->opt.rank != i || o->opt.world_size != count))
                return fail(c, HB_ERR_INVALID, "destination partition: ctxs[i] must be rank i of `count`");
        }
        int rc = set_device(c);
        if (rc) return rc;
        for (int i = 0; i < count; i++) HB_HIP(hipStreamSynchronize(ctxs[i]->stream));
        const Plan &p = c->plan;
        const uint64_t S = c->slice_rows;
        if (phase == 1) {
            // what hb_finish's ncclAllGather of the Kahan-sum slices does (edge partition without a
            // communicator: every logical rank already holds all sums)
            if (!dest_mode(c)) return HB_OK;
            for (int i = 0; i < count; i++)
                for (int j = 0; j < count; j++)
                    if (i != j && S)
                        HB_HIP(hipMemcpyAsync(ctxs[i]->d_ksum + (uint64_t)j * S, ctxs[j]->d_ksum + (uint64_t)j * S, S * sizeof(double),
                                              hipMemcpyDeviceToDevice, c->stream));
            HB_HIP(hipStreamSynchronize(c->stream));
            return HB_OK;
        }
        const bool wire6 = packed_wire(c); // HB_FLAG_PACKED_WIRE: the packed forms, the same kernels and steps as the pass driver's
        for (int i = 0; i < count; i++)
            if (packed_wire(ctxs[i]) != wire6 || (wire6 && ctxs[i]->opt.world_size != count))
                return fail(c, HB_ERR_INVALID, "HB_FLAG_PACKED_WIRE: every context needs the flag, and ctxs must be all `count` ranks of the world");
        // packed_all_reduce_max between logical ranks: rows_of(ctx) = its R rows; device copies in place of the all-to-all and the all-gather
        auto packed_all_reduce = [&](auto rows_of, uint64_t R, uint64_t S) -> int {
            for (int i = 0; i < count; i++) {
                const int rc2 = wire6_pack_all(ctxs[i], rows_of(ctxs[i]), R, S, ctxs[i]->stream);
                if (rc2) return rc2;
                HB_HIP(hipStreamSynchronize(ctxs[i]->stream));
            }
            for (int i = 0; i < count && S; i++)
                for (int j = 0; j < count; j++)
                    HB_HIP(hipMemcpyAsync(ctxs[i]->d_w6[1] + (uint64_t)j * S * 12, ctxs[j]->d_w6[0] + (uint64_t)i * S * 12, S * 48, hipMemcpyDeviceToDevice, c->stream));
            HB_HIP(hipStreamSynchronize(c->stream));
            for (int i = 0; i < count; i++) {
                const int rc2 = wire6_reduce_slice(ctxs[i], S, (uint64_t)i, ctxs[i]->stream);
                if (rc2) return rc2;
                HB_HIP(hipStreamSynchronize(ctxs[i]->stream));
            }
            for (int i = 0; i < count && S; i++)
                for (int j = 0; j < count; j++)
                    if (i != j)
                        HB_HIP(hipMemcpyAsync(ctxs[i]->d_w6[0] + (uint64_t)j * S * 12, ctxs[j]->d_w6[0] + (uint64_t)j * S * 12, S * 48, hipMemcpyDeviceToDevice, c->stream));
            HB_HIP(hipStreamSynchronize(c->stream));
            for (int i = 0; i < count; i++) {
                const int rc2 = wire6_unpack_all(ctxs[i], rows_of(ctxs[i]), R, ctxs[i]->stream);
                if (rc2) return rc2;
                HB_HIP(hipStreamSynchronize(ctxs[i]->stream));
            }
            return HB_OK;
        };
        if (!dest_mode(c) && edge_changed_only(c)) {
            // the changed-only all-reduce between logical ranks: union of the locally-changed bitmaps, every context packs
            // its rows of the union, the packed buffers are max-folded (the all-reduce), every context unpacks
            const uint64_t words = p.n_pad / 32;
            for (int i = 0; i < count; i++)
                if (!ctxs[i]->d_lbits || !edge_changed_only(ctxs[i])) return fail(c, HB_ERR_INVALID, "changed-only exchange: every context needs HB_FLAG_CHANGED_ONLY");
            HB_HIP(hipMemcpyAsync(c->d_ubits, c->d_lbits, words * 4, hipMemcpyDeviceToDevice, c->stream));
            for (int i = 1; i < count && words; i++)
                hipLaunchKernelGGL(hbk::or_words_kernel, dim3((unsigned)std::min<uint64_t>((words + 255) / 256, 2048)), dim3(256), 0, c->stream, c->d_ubits,
                                   (const uint32_t *)ctxs[i]->d_lbits, words);
            HB_HIP(hipGetLastError());
            for (int i = 1; i < count; i++) HB_HIP(hipMemcpyAsync(ctxs[i]->d_ubits, c->d_ubits, words * 4, hipMemcpyDeviceToDevice, c->stream));
            HB_HIP(hipStreamSynchronize(c->stream));
            for (int i = 0; i < count; i++) {
                int rc2 = edge_co_pack(ctxs[i]);
                if (rc2) return rc2;
                HB_HIP(hipStreamSynchronize(ctxs[i]->stream));
            }
            const uint64_t count4 = c->co_rows * 4;
            if (wire6 && count4) {
                const int rc2 = packed_all_reduce([](hb_ctx *x) { return x->d_pack; }, c->co_rows, wire6_co_slice(c));
                if (rc2) return rc2;
            }
            for (int i = 1; i < count && count4 && !wire6; i++) {
                hipLaunchKernelGGL(hbk::merge_max_kernel, dim3(2048), dim3(256), 0, c->stream, c->d_pack, (const uint4 *)ctxs[i]->d_pack, count4);
                HB_HIP(hipGetLastError());
            }
            for (int i = 1; i < count && count4 && !wire6; i++) HB_HIP(hipMemcpyAsync(ctxs[i]->d_pack, c->d_pack, count4 * 16, hipMemcpyDeviceToDevice, c->stream));
            HB_HIP(hipStreamSynchronize(c->stream));
            for (int i = 0; i < count; i++) {
                int rc2 = edge_co_unpack(ctxs[i]);
                if (rc2) return rc2;
                ctxs[i]->wire_bytes += (uint64_t)(count - 1) * words * 4 + (wire6 ? wire6_co_bytes(ctxs[i]) : 2 * (uint64_t)(count - 1) * ctxs[i]->co_rows * 64 / (uint64_t)count);
                HB_HIP(hipStreamSynchronize(ctxs[i]->stream));
            }
        } else if (!dest_mode(c) && wire6) {
            // the packed all-reduce(max) of the pending counters
            const int rc2 = packed_all_reduce([](hb_ctx *x) { return x->d_regs[x->cur ^ 1]; }, p.n_pad, wire6_slice(c));
            if (rc2) return rc2;
            for (int i = 0; i < count; i++) ctxs[i]->wire_bytes += wire6_all_reduce_bytes(ctxs[i], wire6_slice(c));
        } else if (!dest_mode(c)) {
            // all-reduce(max) of the pending counters: fold everything into ctxs[0], then copy out
            const uint64_t count4 = p.n_pad * 4;
            for (int i = 1; i < count && count4; i++) {
                hipLaunchKernelGGL(hbk::merge_max_kernel, dim3(2048), dim3(256), 0, c->stream, c->d_regs[c->cur ^ 1],
                                   (const uint4 *)ctxs[i]->d_regs[ctxs[i]->cur ^ 1], count4);
                HB_HIP(hipGetLastError());
            }
            for (int i = 1; i < count && count4; i++)
                HB_HIP(hipMemcpyAsync(ctxs[i]->d_regs[ctxs[i]->cur ^ 1], c->d_regs[c->cur ^ 1], count4 * 16, hipMemcpyDeviceToDevice, c->stream));
        } else {
            // all-gather of the owned slices (counters, changed bits) + sum of the changed counts
            const size_t W = hbk::kCounterWords;
            std::vector<unsigned long long> total(W, 0), cnt((size_t)count * W, 0);
            for (int i = 0; i < count; i++) {
                HB_HIP(hipMemcpyAsync(&cnt[(size_t)i * W], ctxs[i]->d_counters + W * ctxs[i]->t, W * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
            }
            HB_HIP(hipStreamSynchronize(c->stream));
            for (int i = 0; i < count; i++)
                for (size_t k = 0; k < W; k++) total[k] += cnt[(size_t)i * W + k];
            const bool packed = changed_only(c);
            const bool whole6 = wire6 && !packed; // whole slices as 48-byte rows: pack, move S x 48 bytes, unpack the foreign slices
            for (int i = 0; i < count && whole6; i++) {
                const int rc2 = wire6_pack_own_slice(ctxs[i]);
                if (rc2) return rc2;
                HB_HIP(hipStreamSynchronize(ctxs[i]->stream));
            }
            for (int i = 0; i < count; i++) {
                hb_ctx *d = ctxs[i];
                for (int j = 0; j < count; j++) {
                    if (i == j || !S) continue;
                    hb_ctx *o = ctxs[j];
                    if (whole6)
                        HB_HIP(hipMemcpyAsync(d->d_w6[0] + (uint64_t)j * S * 12, o->d_w6[0] + (uint64_t)j * S * 12, S * 48, hipMemcpyDeviceToDevice, c->stream));
                    else if (!packed)
                        HB_HIP(hipMemcpyAsync(d->d_regs[d->cur ^ 1] + (uint64_t)j * S * 4, o->d_regs[o->cur ^ 1] + (uint64_t)j * S * 4, S * 64,
                                              hipMemcpyDeviceToDevice, c->stream));
                    HB_HIP(hipMemcpyAsync(d->d_bits[d->cur ^ 1] + (uint64_t)j * (S / 32), o->d_bits[o->cur ^ 1] + (uint64_t)j * (S / 32), S / 8,
                                          hipMemcpyDeviceToDevice, c->stream));
                }
                HB_HIP(hipMemcpyAsync(d->d_counters + W * d->t, total.data(), W * sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream));
            }
            if (whole6) {
                HB_HIP(hipStreamSynchronize(c->stream));
                for (int i = 0; i < count; i++) {
                    const int rc2 = wire6_unpack_foreign_slices(ctxs[i]);
                    if (rc2) return rc2;
                    HB_HIP(hipStreamSynchronize(ctxs[i]->stream));
                }
            }
            if (packed) {
                // the changed-only protocol with copies in place of the broadcasts: pack everywhere, move the runs, unpack
                HB_HIP(hipStreamSynchronize(c->stream));
                for (int i = 0; i < count; i++) {
                    int rc2 = exchange_pack(ctxs[i]);
                    if (rc2) return rc2;
                    HB_HIP(hipStreamSynchronize(ctxs[i]->stream));
                }
                for (int i = 0; i < count; i++)
                    for (int j = 0; j < count; j++) {
                        if (i == j) continue;
                        const uint64_t off = ctxs[j]->ex_off[j], cnt = ctxs[j]->ex_off[j + 1] - off;
                        const uint64_t rb = packed_row_bytes(c); // (48: 6 bits per register on the wire)
                        if (cnt) HB_HIP(hipMemcpyAsync((uint8_t *)ctxs[i]->d_pack + off * rb, (uint8_t *)ctxs[j]->d_pack + off * rb, cnt * rb, hipMemcpyDeviceToDevice, c->stream));
                    }
                HB_HIP(hipStreamSynchronize(c->stream));
                for (int i = 0; i < count; i++) {
                    int rc2 = exchange_unpack(ctxs[i]);
                    if (rc2) return rc2;
                    HB_HIP(hipStreamSynchronize(ctxs[i]->stream));
                }
            }
        }
        HB_HIP(hipStreamSynchronize(c->stream));
        return HB_OK;
    });
}

