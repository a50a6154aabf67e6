// hb_api_load.inc - part of the hb_api.hip translation unit (included there; uses its hb_ctx and helpers).
// Plan + upload: the common tail of every load entry point (device / host planner, device state, sweep support).
// ---- plan + upload (common tail of every load entry point) -------------------------------
// The reduced graph arrives either on the host (c->g.row_ptr / c->g.src) or already on the device (csr, e.g. from
// the GPU ingest).  Default: everything from here on happens on the device (hb_plan.hip); HB_FLAG_HOST_PLAN and the
// destination partition use the host planner (hb_host.cpp), which produces the same layout.
bool device_plan(const hb_ctx *c) { return !(c->opt.flags & HB_FLAG_HOST_PLAN); }
bool deferred_times(const hb_ctx *c); // (hb_api_pass.inc)

// destination partition: this rank keeps the in-edges of the rows it owns - in the host copy of the reduced graph (if one
// is kept) and in the device CSR (if the graph lives there)
int keep_owned(hb_ctx *c, DeviceCsr *csr)
{
    if (!dest_mode(c)) return HB_OK;
    const uint64_t world = (uint64_t)std::max(c->opt.world_size, 1), rank = (uint64_t)c->opt.rank, n = c->g.ids.size();
    if (c->g.row_ptr.size() == n + 1 && n) keep_owned_rows(&c->g, world, rank);
    if (csr && csr->d_row_ptr) {
        const std::string e = gpu_keep_owned_rows((void *)c->stream, csr, n, world, rank);
        if (!e.empty()) return fail(c, e.find("memory") != std::string::npos ? HB_ERR_NOMEM : HB_ERR_HIP, e);
    }
    return HB_OK;
}

__global__ __launch_bounds__(256) void idlow_kernel(const uint64_t *lo_by_sid, const uint32_t *order, uint64_t n_pad, uint64_t *idlow)
{
    const uint64_t d = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (d >= n_pad) return;
    const uint32_t s = order[d];
    idlow[d] = s == kNone ? 0ull : lo_by_sid[s];
}

template <class T>
T *adopt(hb_ctx *c, DevPtr<T> &b, size_t bytes) // a buffer allocated elsewhere becomes the context's
{
    c->allocs.push_back({b.get(), bytes});
    c->stats.device_bytes += bytes;
    return b.release();
}

// Page-locked result buffers are touched by the host for the first time at LOAD, not by the run: the CPU mapping of a hipHostMalloc
// block is populated page by page on first access, and the first hb_run of a context - the only one `stract centrality harmonic` makes
// (entrypoint/centrality.rs:49) - paid for it in hb_finish (658 k scattered 8-byte writes into 794 MB of never-touched pages by 8
// threads: 373-414 ms at C4 against 4.5 ms steady; hb_result_copy's first read of the same pages another 1.4 s under a loaded page
// cache: profiles/r05j_e2e_C4_first_run_and_store_phases.txt).  One background thread writes a word per page while the rest of the
// load (tables, src_jp, layout check, transposed graph) runs on the device; joined before the load returns.
// [r6] ... and they are ALLOCATED there too: page-locking 794 MB (C4's result image) takes the runtime ~0.1 s, which used to sit in front of
// the state stage; the thread starts when plan_and_upload does (n is known then) and works beside the planner.
struct HostResultBuffers {
    std::thread th;
    int device = 0;
    uint64_t n = 0, cap = 0; // result image entries; final-list entries (0 = no list)
    double *h_out = nullptr;
    uint32_t *h_sid = nullptr;
    double *h_val = nullptr;
    unsigned long long *h_count = nullptr;
    bool ok = true;
    void start(int dev, uint64_t n_, uint64_t cap_)
    {
        device = dev;
        n = n_;
        cap = cap_;
        th = std::thread([this]() {
            if (hipSetDevice(device) != hipSuccess) {
                ok = false;
                return;
            }
            auto touch = [](void *p, size_t bytes) {
                volatile unsigned char *b = (volatile unsigned char *)p;
                for (size_t off = 0; off < bytes; off += 4096) b[off] = 0;
                if (bytes) b[bytes - 1] = 0;
            };
            if (n) {
                if (hipHostMalloc((void **)&h_out, n * sizeof(double)) != hipSuccess) ok = false;
                else touch(h_out, n * sizeof(double));
            }
            if (ok && cap) {
                if (hipHostMalloc((void **)&h_sid, cap * sizeof(uint32_t)) != hipSuccess || hipHostMalloc((void **)&h_val, cap * sizeof(double)) != hipSuccess ||
                    hipHostMalloc((void **)&h_count, 2 * sizeof(unsigned long long)) != hipSuccess)
                    ok = false;
                else {
                    touch(h_sid, cap * sizeof(uint32_t));
                    touch(h_val, cap * sizeof(double));
                    touch(h_count, 2 * sizeof(unsigned long long));
                }
            }
            if (!ok) (void)hipGetLastError();
        });
    }
    void join()
    {
        if (th.joinable()) th.join();
    }
    void release() // the context has taken the buffers
    {
        h_out = nullptr;
        h_sid = nullptr;
        h_val = nullptr;
        h_count = nullptr;
    }
    ~HostResultBuffers()
    {
        join();
        for (void *q : {(void *)h_out, (void *)h_sid, (void *)h_val, (void *)h_count})
            if (q) (void)hipHostFree(q);
    }
};

// Every kernel of the default pass driver once, over zero rows: the first dispatch of a kernel creates its runtime-side function
// object (kernarg layout, code handle); done at load so that the first hb_run finds them (VERDICT r5 #1).  No state is touched: every
// launch has row_lo == row_hi (no tile, no seed, no word) and adds zero to its counter stripes.
int warm_kernels(hb_ctx *c);

// `in`: the reduced graph on the device, if the ingest left it there (else empty: uploaded here from c->g); freed when the plan exists
int plan_and_upload(hb_ctx *c, OwnedCsr in, uint64_t m_eff)
{
    const uint64_t n = c->g.ids.size();
    c->loaded = false;
    c->rows = RowsOf::Nobody;
    c->image = Image::None;
    c->run_open = false;
    free_graph_buffers(c);
    c->stats.n = n;
    c->stats.m_input = c->g.m_input;
    c->stats.m_unique = c->g.m_unique;
    c->stats.m_eff = m_eff;
    double t0 = now_ms();
    const bool on_device = device_plan(c);
    // results shipped in stages while the passes run (results_stage): one rank, a download worth hiding (>= 8 MB) or forced
    // (HB_X_SNAPSHOT_EVERY_PASS; HB_X_NO_STAGED_RESULTS = never)
    c->rs.on = n && !multi_rank(c) && !linked(c) && !ref_tail(c) && !xbit(c, HB_X_NO_STAGED_RESULTS) && (n >= (1u << 20) || xbit(c, HB_X_SNAPSHOT_EVERY_PASS));
    c->rs.cap = c->rs.on ? (xbit(c, HB_X_SHORT_FINAL_LIST) ? 16 : n / 8 + 4096) : 0;
    HostResultBuffers hostbuf; // (declared here: joined, and what the context has not taken freed, on every return path below)
    hostbuf.start(c->device, n, c->rs.cap);
    if (!in.d.d_row_ptr) in.reset(); // (no row pointers: no CSR)
    if (!on_device && n && c->g.row_ptr.size() != n + 1) {
        // host planner, but the reduced graph only exists on the device: bring it back
        try {
            c->g.row_ptr.resize(n + 1);
            c->g.src.resize(m_eff);
        } catch (const std::bad_alloc &) {
            return fail(c, HB_ERR_NOMEM, "out of host memory for the reduced graph");
        }
        HB_HIP(hipMemcpyAsync(c->g.row_ptr.data(), in.d.d_row_ptr, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        if (m_eff) HB_HIP(hipMemcpyAsync(c->g.src.data(), in.d.d_src, m_eff * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HB_HIP(hipStreamSynchronize(c->stream));
    }
    if (n && !in.d.d_src) {
        HB_HIP(hipMalloc((void **)&in.d.d_src, std::max<uint64_t>(m_eff, 1) * sizeof(uint32_t)));
        if (m_eff) HB_HIP(hipMemcpyAsync(in.d.d_src, c->g.src.data(), m_eff * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        if (on_device) {
            HB_HIP(hipMalloc((void **)&in.d.d_row_ptr, (n + 1) * sizeof(uint64_t)));
            HB_HIP(hipMemcpyAsync(in.d.d_row_ptr, c->g.row_ptr.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
        }
        in.d.m = m_eff;
    }
    // global out-degree (the device order must be identical on every rank): histogram on the device
    bool reorder = !(c->opt.flags & HB_FLAG_NO_REORDER);
    if (multi_rank(c) && !linked(c)) reorder = false; // logical ranks without a communicator
    DevPtr<uint64_t> d_lo(in.d.d_id_lo); // (from the device ingest, else NULL: uploaded below)
    in.d.d_id_lo = nullptr;
    DevPtr<uint32_t> d_deg;
    if (n) {
        HB_HIP(d_deg.alloc(n));
        HB_HIP(hipMemsetAsync(d_deg.get(), 0, n * sizeof(uint32_t), c->stream));
        if (m_eff) {
            const unsigned blocks = grid_blocks(c, (m_eff + 255) / 256, 16);
            hipLaunchKernelGGL(hbk::histogram_kernel, dim3(blocks), dim3(256), 0, c->stream, (const uint32_t *)in.d.d_src, m_eff, d_deg.get());
            HB_HIP(hipGetLastError());
        }
        if (linked(c)) HB_COLL(coll_all_reduce(c, d_deg.get(), n, ncclUint32, ncclSum, c->stream));
    }
    PlanTune pt = plan_tune(c->opt.chunk, c->opt.tune);
    pt.xcd_map = !(c->opt.flags & HB_FLAG_NO_XCD_MAP);
    if (dest_mode(c)) pt.world = (uint32_t)std::max(c->opt.world_size, 1);
    // live-first order (HB_FLAG_LIVE_FIRST): only where "no in-edge here" means "no in-edge at all" and the passes are the fused ones of
    // one rank (an edge-partitioned rank sees part of a node's in-edges; the counting kernels of HB_FLAG_PASS_STATS count every gather).
    pt.live_first = reorder && !multi_rank(c) && !linked(c) && !dest_mode(c) && !unfused(c) && live_first_by_flags(c->opt.flags, n);
    // The two counter arrays are what the passes gather from at random: allocate them BEFORE the planner churns
    // through tens of GB of work memory, while the device heap can still back them with large contiguous
    // fragments (allocated after it, the same kernels ran 1-2 % slower: more TLB misses on the gathers).
    {
        const uint64_t w = pt.world > 1 ? pt.world : 1;
        const uint64_t n_pad_pre = (((n + w - 1) / w + kRowAlign - 1) / kRowAlign * kRowAlign) * w;
        int rc0;
        if ((rc0 = dev_alloc(c, &c->d_regs[0], n_pad_pre * 4))) return rc0;
        if ((rc0 = dev_alloc(c, &c->d_regs[1], n_pad_pre * 4))) return rc0;
    }
    std::vector<uint32_t> outdeg; // host planner only
    DevicePlan dp;
    DevPtr<uint64_t> dp_row_ptr; // the planner's buffers (whatever it had allocated, if it failed), until the context adopts them below
    DevPtr<uint32_t> dp_src, dp_order, dp_dev_of, dp_outdeg;
    if (on_device) {
        std::string perr = gpu_build_plan((void *)c->stream, n, in.d.d_row_ptr, in.d.d_src, d_deg.get(), reorder, pt, &c->plan, &dp);
        dp_row_ptr.reset(dp.d_row_ptr); dp_src.reset(dp.d_src); dp_order.reset(dp.d_order); dp_dev_of.reset(dp.d_dev_of); dp_outdeg.reset(dp.d_outdeg_dev);
        if (!perr.empty()) {
            (void)hipGetLastError();
            return fail(c, perr.find("memory") != std::string::npos ? HB_ERR_NOMEM : (perr.find("exhausted") != std::string::npos ? HB_ERR_LIMIT : HB_ERR_HIP), perr);
        }
    } else {
        outdeg.assign(n, 0);
        if (n) {
            HB_HIP(hipMemcpyAsync(outdeg.data(), d_deg.get(), n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
            HB_HIP(hipStreamSynchronize(c->stream));
        }
        static const uint64_t zero = 0;
        std::string perr = build_plan(n, n ? c->g.row_ptr.data() : &zero, c->g.src.data(), outdeg, reorder, pt, &c->plan);
        if (!perr.empty()) return fail(c, perr.find("memory") != std::string::npos ? HB_ERR_NOMEM : HB_ERR_LIMIT, perr);
    }
    in.reset(); // the input CSR is no longer needed on the device
    c->stats.ms_plan = now_ms() - t0;
    const Plan &p = c->plan;
    const uint64_t rows_total = p.n_pad + p.nv;
    const uint64_t src_len = on_device ? dp.src_len : p.src.size();
    c->plan_entries = src_len;
    c->stats.work_rows = rows_total;
    c->stats.virtual_rows = p.nv;
    c->stats.levels = p.level_begin.size() > 1 ? p.level_begin.size() - 1 : 0;
    c->stats.level1_edges = p.level1_edges;
    c->stats.level1_rows = p.level1_rows;
    c->stats.direct_edges = p.direct_edges;
    c->stats.rows_with_in_edges = p.rows_with_in_edges;

    // ---- device memory
    t0 = now_ms();
    const bool trace_state = std::getenv("HB_TRACE_INGEST") != nullptr; // where the time of the state stage goes, on stderr
    double t_lap = t0;
    auto lap = [&](const char *what) {
        if (!trace_state) return;
        (void)hipStreamSynchronize(c->stream);
        std::fprintf(stderr, "[hb state] %-34s %8.1f ms\n", what, now_ms() - t_lap);
        t_lap = now_ms();
    };
    c->bits_words = (rows_total + 31) / 32 + 2;
    int rc;
    if (on_device) {
        c->d_row_ptr = adopt(c, dp_row_ptr, (rows_total + 2) * sizeof(uint64_t));
        c->d_src = adopt(c, dp_src, (src_len + 4) * sizeof(uint32_t));
        c->d_sid_of = adopt(c, dp_order, std::max<uint64_t>(p.n_pad, 64) * sizeof(uint32_t));
        c->d_dev_of = adopt(c, dp_dev_of, std::max<uint64_t>(n, 64) * sizeof(uint32_t));
        c->d_outdeg = adopt(c, dp_outdeg, std::max<uint64_t>(p.n_pad, 64) * sizeof(uint32_t));
        c->m_global = dp.m_global;
    } else {
        if ((rc = dev_alloc(c, &c->d_row_ptr, rows_total + 1))) return rc;
        if ((rc = dev_alloc(c, &c->d_src, src_len + 4))) return rc;
        if ((rc = dev_alloc(c, &c->d_dev_of, n))) return rc;
        if ((rc = dev_alloc(c, &c->d_sid_of, p.n_pad))) return rc;
        if ((rc = dev_alloc(c, &c->d_outdeg, p.n_pad))) return rc;
    }
    if ((rc = dev_alloc(c, &c->d_part, p.nv * 4))) return rc;
    if ((rc = dev_alloc(c, &c->d_bits[0], c->bits_words))) return rc;
    if ((rc = dev_alloc(c, &c->d_bits[1], c->bits_words))) return rc;
    if ((rc = dev_alloc(c, &c->d_kdirty, p.n_pad / 32 + 2))) return rc;
    // Kahan ownership: one contiguous slice of rows per rank (multiple of 64 rows)
    const uint64_t world = linked(c) ? (uint64_t)c->opt.world_size : 1;
    c->slice_rows = dest_mode(c) ? p.slice : ((p.n_pad + world - 1) / world + 63) / 64 * 64;
    c->ksum_len = std::max<uint64_t>(c->slice_rows * (dest_mode(c) ? (uint64_t)std::max(c->opt.world_size, 1) : world), p.n_pad);
    if ((rc = dev_alloc(c, &c->d_ksum, c->ksum_len))) return rc;
    if ((rc = dev_alloc(c, &c->d_kerr, p.n_pad))) return rc;
    if ((rc = dev_alloc(c, &c->d_size, p.n_pad))) return rc;
    if ((rc = dev_alloc(c, &c->d_idlow, p.n_pad))) return rc;
    if ((rc = dev_alloc(c, &c->d_counters, ((size_t)c->max_passes + 1) * hbk::kCounterWords))) return rc;
    if ((rc = dev_alloc(c, &c->d_raw, HLL64_TABLE_LEN))) return rc;
    if ((rc = dev_alloc(c, &c->d_bias, HLL64_TABLE_LEN))) return rc;
    if ((rc = dev_alloc(c, &c->d_lc, 68))) return rc;
    if ((rc = dev_alloc(c, &c->d_out, n))) return rc;
    if (c->rs.on) {
        if ((rc = dev_alloc(c, &c->rs.d_sent, p.n_pad))) return rc;
        if ((rc = dev_alloc(c, &c->rs.d_sid, c->rs.cap))) return rc;
        if ((rc = dev_alloc(c, &c->rs.d_val, c->rs.cap))) return rc;
        if ((rc = dev_alloc(c, &c->rs.d_count, 2))) return rc;
        if ((rc = dev_alloc(c, &c->rs.d_kept, hbk::kCounterWords))) return rc;
    }
    if (deferred_times(c)) { // (one timing-event set per pass is kept in this mode: the first 32 exist before the first run)
        while (c->ev_pool.size() < 32) {
            hb_ctx::EvSet es{};
            for (auto &e : es.e)
                if (hipEventCreate(&e) != hipSuccess) return fail(c, HB_ERR_HIP, "hipEventCreate failed");
            c->ev_pool.push_back(es);
        }
    }

    lap("allocations");
    uint8_t lc[68];
    if (!build_lc_table(lc)) return fail(c, HB_ERR_INVALID, "host libm log() too close to a rounding boundary for the linear-counting table");
    HB_HIP(hipMemcpyAsync(c->d_raw, HLL64_RAW_ESTIMATE, sizeof(HLL64_RAW_ESTIMATE), hipMemcpyHostToDevice, c->stream));
    HB_HIP(hipMemcpyAsync(c->d_bias, HLL64_BIAS, sizeof(HLL64_BIAS), hipMemcpyHostToDevice, c->stream));
    HB_HIP(hipMemcpyAsync(c->d_lc, lc, 68, hipMemcpyHostToDevice, c->stream));
    if (!on_device) {
        c->stats.virtual_edges = p.row_ptr.empty() ? 0 : p.row_ptr[rows_total] - p.row_ptr[p.n_pad];
        HB_HIP(hipMemcpyAsync(c->d_row_ptr, p.row_ptr.data(), (rows_total + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
        if (!p.src.empty())
            HB_HIP(hipMemcpyAsync(c->d_src, p.src.data(), p.src.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        if (p.n_pad)
            HB_HIP(hipMemcpyAsync(c->d_sid_of, p.order.data(), p.n_pad * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        std::vector<uint32_t> outdeg_dev(p.n_pad, 0);
        c->m_global = 0;
        for (uint64_t d = 0; d < p.n_pad; d++)
            if (p.order[d] != kNone) {
                outdeg_dev[d] = outdeg[p.order[d]];
                c->m_global += outdeg[p.order[d]];
            }
        if (p.n_pad)
            HB_HIP(hipMemcpyAsync(c->d_outdeg, outdeg_dev.data(), p.n_pad * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        if (n) HB_HIP(hipMemcpyAsync(c->d_dev_of, p.dev_of.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        HB_HIP(hipStreamSynchronize(c->stream)); // outdeg_dev goes out of scope
    } else {
        uint64_t ends[2] = {0, 0};
        HB_HIP(hipMemcpyAsync(&ends[0], c->d_row_ptr + p.n_pad, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        HB_HIP(hipMemcpyAsync(&ends[1], c->d_row_ptr + rows_total, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        HB_HIP(hipStreamSynchronize(c->stream));
        c->stats.virtual_edges = ends[1] - ends[0];
    }
    lap("tables / plan arrays");
    // [r6] layout of the result image (hb_ctx::out_len): compact when the results travel in stages, else one entry per sid
    c->out_len = n;
    c->d_cid_of = c->d_sid_of;
    if (c->rs.on && n) {
        DevPtr<uint32_t> d_flags;
        DevPtr<uint64_t> d_cpos;
        DevPtr<unsigned long long> d_words;
        const uint64_t nw = (n + 63) / 64;
        HB_HIP(d_flags.alloc(n + 1));
        HB_HIP(d_cpos.alloc(n + 2));
        HB_HIP(d_words.alloc(nw));
        if ((rc = dev_alloc(c, &c->d_cid_of, p.n_pad))) return rc;
        HB_HIP(hipMemsetAsync(d_flags.get(), 0, (n + 1) * sizeof(uint32_t), c->stream));
        const unsigned blocks = grid_blocks(c, (p.n_pad + 255) / 256, 16);
        hipLaunchKernelGGL(hbk::in_flags_kernel, dim3(blocks), dim3(256), 0, c->stream, (const uint64_t *)c->d_row_ptr, (const uint32_t *)c->d_sid_of, p.n_pad, d_flags.get());
        HB_HIP(hipGetLastError());
        const std::string e = device_prefix((void *)c->stream, d_flags.get(), n, d_cpos.get());
        if (!e.empty()) return fail(c, HB_ERR_HIP, e);
        hipLaunchKernelGGL(hbk::cid_of_kernel, dim3(blocks), dim3(256), 0, c->stream, (const uint64_t *)c->d_row_ptr, (const uint32_t *)c->d_sid_of,
                           (const uint64_t *)d_cpos.get(), p.n_pad, c->d_cid_of);
        HB_HIP(hipGetLastError());
        hipLaunchKernelGGL(hbk::pack_flags_kernel, dim3(grid_blocks(c, (nw + 3) / 4, 16)), dim3(256), 0, c->stream,
                           (const uint32_t *)d_flags.get(), n, d_words.get());
        HB_HIP(hipGetLastError());
        uint64_t n_c = 0;
        c->h_in_bits.assign(nw, 0);
        HB_HIP(hipMemcpyAsync(&n_c, d_cpos.get() + n, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        HB_HIP(hipMemcpyAsync(c->h_in_bits.data(), d_words.get(), nw * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        HB_HIP(hipStreamSynchronize(c->stream));
        if (n_c != p.rows_with_in_edges)
            return fail(c, HB_ERR_INVALID, "result image: " + std::to_string(n_c) + " nodes with in-edges counted on the device, the plan says " + std::to_string(p.rows_with_in_edges));
        c->out_len = n_c;
        lap("compact result image (cid per row, host bitmap)");
    }
    // low 64 bits of every NodeID in device order (HyperLogLog::add_u128 hashes only those, hyperloglog.rs:4398-4400)
    if (n) {
        if (!d_lo) {
            uvec<uint64_t> lo(n);
            host_gather_id_lo(c->g.ids.data(), n, lo.data()); // (hb_host.cpp, OpenMP team)
            HB_HIP(d_lo.alloc(n));
            HB_HIP(hipMemcpyAsync(d_lo.get(), lo.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
            HB_HIP(hipStreamSynchronize(c->stream)); // lo goes out of scope
        }
        hipLaunchKernelGGL(idlow_kernel, dim3((unsigned)((p.n_pad + 255) / 256)), dim3(256), 0, c->stream, (const uint64_t *)d_lo.get(),
                           (const uint32_t *)c->d_sid_of, p.n_pad, c->d_idlow);
        HB_HIP(hipGetLastError());
        HB_HIP(hipStreamSynchronize(c->stream));
    }
    lap("id_low");
    if (p.n_pad && saturation_by_flags(c->opt.flags) && !multi_rank(c) && !linked(c) && !dest_mode(c)) {
        // saturated rows (DESIGN.md section 38): U depends on the graph alone, the bitmap is hb_begin's to clear
        if ((rc = dev_alloc(c, &c->d_sat_u, 64))) return rc;
        if ((rc = dev_alloc(c, &c->d_sat, c->bits_words))) return rc;
        if ((rc = dev_alloc(c, &c->d_early, hbk::kStripes))) return rc; // (DESIGN.md section 39; cleared before every EARLY pass)
        HB_HIP(hipMemsetAsync(c->d_early, 0, hbk::kStripes * sizeof(unsigned long long), c->stream));
        HB_HIP(hipMemsetAsync(c->d_sat_u, 0, 64 * sizeof(uint32_t), c->stream));
        HB_HIP(hipMemsetAsync(c->d_sat, 0, c->bits_words * sizeof(uint32_t), c->stream));
        hipLaunchKernelGGL(hbk::sat_bound_kernel, dim3(grid_blocks(c, (p.n_pad + 255) / 256, 8)), dim3(256), 0, c->stream, (const uint64_t *)c->d_idlow,
                           (const uint32_t *)c->d_sid_of, (const uint32_t *)c->d_outdeg, p.n_pad, c->d_sat_u);
        HB_HIP(hipGetLastError());
        lap("saturation bound");
    }
    if (src_len && !(c->opt.flags & HB_FLAG_NO_INIT_PASS)) {
        if ((rc = dev_alloc(c, &c->d_src_jp, src_len + 4))) return rc;
        const unsigned blocks = grid_blocks(c, (src_len + 255) / 256, 16);
        if ((rc = dev_alloc(c, &c->d_self_jp, p.n_pad + 4))) return rc;
        hipLaunchKernelGGL(hbk::self_jp_kernel, dim3(grid_blocks(c, (p.n_pad + 255) / 256, 16)), dim3(256), 0, c->stream,
                           (const uint64_t *)c->d_idlow, (const uint32_t *)c->d_sid_of, p.n_pad, c->d_self_jp);
        HB_HIP(hipGetLastError());
        hipLaunchKernelGGL(hbk::src_jp_kernel, dim3(blocks), dim3(256), 0, c->stream, (const uint32_t *)c->d_src, src_len, (const uint16_t *)c->d_self_jp, p.n_pad,
                           c->d_src_jp);
        HB_HIP(hipGetLastError());
        if ((rc = dev_alloc(c, &c->d_virt_rows, c->bits_words + 4))) return rc;
        unsigned long long *d_l0 = c->d_counters + 8, h_l0 = ~0ull; // (d_counters is zeroed by hb_begin before every run)
        HB_HIP(hipMemsetAsync(d_l0, 0, sizeof(unsigned long long), c->stream));
        const uint64_t l0_lo = p.level_begin.size() > 1 ? p.level_begin[0] : 0, l0_hi = p.level_begin.size() > 1 ? p.level_begin[1] : 0;
        hipLaunchKernelGGL(hbk::virt_rows_kernel, dim3(grid_blocks(c, (rows_total + 255) / 256, 16)), dim3(256), 0, c->stream,
                           (const uint64_t *)c->d_row_ptr, (const uint32_t *)c->d_src, rows_total, p.n_pad, c->d_virt_rows, l0_lo, l0_hi, d_l0);
        HB_HIP(hipGetLastError());
        HB_HIP(hipMemcpyAsync(&h_l0, d_l0, sizeof(h_l0), hipMemcpyDeviceToHost, c->stream));
        HB_HIP(hipStreamSynchronize(c->stream));
        c->level0_all_real = h_l0 == 0;
        HB_HIP(hipStreamSynchronize(c->stream));
    }
    lap("self_jp / src_jp");
    {   // structural check of the layout the pass kernels are about to gather through (hb_aux.hip.h validate_plan_kernel)
        unsigned long long *d_bad = c->d_counters; // zeroed by hb_begin before every run
        unsigned long long h_bad[4] = {0, 0, 0, 0};
        HB_HIP(hipMemsetAsync(d_bad, 0, sizeof(h_bad), c->stream));
        if (rows_total) {
            const unsigned blocks = grid_blocks(c, (rows_total * 4 + 255) / 256, 16);
            hipLaunchKernelGGL(hbk::validate_plan_kernel, dim3(blocks), dim3(256), 0, c->stream, (const uint64_t *)c->d_row_ptr, (const uint32_t *)c->d_src,
                               rows_total, p.n_pad, src_len, d_bad);
            HB_HIP(hipGetLastError());
        }
        HB_HIP(hipMemcpyAsync(h_bad, d_bad, sizeof(h_bad), hipMemcpyDeviceToHost, c->stream));
        HB_HIP(hipStreamSynchronize(c->stream));
        if (h_bad[0] | h_bad[1] | h_bad[2] | h_bad[3])
            return fail(c, HB_ERR_INVALID, "work layout failed its structural check: " + std::to_string(h_bad[0]) + " bad row pointers, " +
                                               std::to_string(h_bad[1]) + " source ids out of range, " + std::to_string(h_bad[2]) +
                                               " rows of mixed source kind, " + std::to_string(h_bad[3]) + " virtual rows reading upwards");
    }
    lap("layout check");
    if ((rc = build_sparse_support(c))) return rc;
    lap("transposed work-row graph");
    // the plan's big host arrays are no longer needed
    decltype(c->plan.row_ptr)().swap(c->plan.row_ptr);
    decltype(c->plan.src)().swap(c->plan.src);
    {
        // the load is over: extents the ingest / planner gave back stay cached for the next load of this process unless the
        // cache is large next to the device (then they go back to the runtime now; hb_destroy returns the rest)
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b < total_b / 4) HB_POOL_TRIM();
    }
    lap("pool trim");
    hostbuf.join();
    if (!hostbuf.ok) return fail(c, HB_ERR_NOMEM, "hipHostMalloc(result buffers) failed");
    c->h_out = hostbuf.h_out;
    c->h_out_len = n;
    c->rs.h_sid = hostbuf.h_sid;
    c->rs.h_val = hostbuf.h_val;
    c->rs.h_count = hostbuf.h_count;
    hostbuf.release();
    lap("pinned result buffers (allocated + touched beside the load)");
    if ((rc = warm_kernels(c))) return rc;
    lap("kernels warmed");
    if (n) {
        // ... and the device's first writes into those pages, and the first use of everything the run's read-backs go through (the side
        // stream's copy queue, cross-stream event waits, event queries, elapsed times, the pinned counter words), happen now as well:
        // one pass over each buffer (14 ms at C4), in the order a run uses them
        HB_HIP(hipEventRecord(c->ev[kEvStart], c->stream));
        if (c->rs.on) {
            HB_HIP(hipEventRecord(c->rs_ready, c->stream));
            HB_HIP(hipStreamWaitEvent(c->rs_stream, c->rs_ready, 0));
            HB_HIP(hipMemcpyAsync(c->h_out, c->d_out, c->out_len * sizeof(double), hipMemcpyDeviceToHost, c->rs_stream));
            HB_HIP(hipEventRecord(c->rs_copied, c->rs_stream));
            HB_HIP(hipMemcpyAsync(c->rs.h_sid, c->rs.d_sid, c->rs.cap * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
            HB_HIP(hipMemcpyAsync(c->rs.h_val, c->rs.d_val, c->rs.cap * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            HB_HIP(hipMemcpyAsync(c->rs.h_count, c->rs.d_count, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
            HB_HIP(hipStreamWaitEvent(c->stream, c->rs_copied, 0));
        } else {
            HB_HIP(hipMemcpyAsync(c->h_out, c->d_out, c->out_len * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        }
        HB_HIP(hipMemcpyAsync(c->h_counters, c->d_counters, hbk::kCounterWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        for (int k = 0; k < 2; k++) {
            HB_HIP(hipMemcpyAsync(c->h_slot + (size_t)k * hbk::kCounterWords, c->d_counters, hbk::kCounterWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
            HB_HIP(hipEventRecord(c->slot_done[k], c->stream));
        }
        HB_HIP(hipEventRecord(c->ev[kEvEnd], c->stream));
        HB_HIP(hipEventSynchronize(c->slot_done[1]));
        if (c->rs.on) {
            (void)hipEventQuery(c->rs_copied);
            (void)hipGetLastError();
        }
        HB_HIP(hipStreamSynchronize(c->stream));
        float ms_warm = 0.f;
        HB_HIP(hipEventElapsedTime(&ms_warm, c->ev[kEvStart], c->ev[kEvEnd]));
    }
    HB_HIP(hipStreamSynchronize(c->stream));
    if (c->rs_stream) HB_HIP(hipStreamSynchronize(c->rs_stream));
    lap("read-back paths warmed");
    c->stats.ms_h2d = now_ms() - t0;
    c->stats.pool_peak_bytes = (uint64_t)HB_POOL_PEAK(); // since the load began (hb_append_edges of an empty stream / this call)
    c->loaded = true;
    return HB_OK;
}

// sid -> device row on the host (debug exports): downloaded on first use when the plan was built on the device
int need_host_dev_of(hb_ctx *c)
{
    const uint64_t n = c->plan.n;
    if (c->plan.dev_of.size() == n) return HB_OK;
    c->plan.dev_of.resize(n);
    if (n) {
        HB_HIP(hipMemcpyAsync(c->plan.dev_of.data(), c->d_dev_of, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HB_HIP(hipStreamSynchronize(c->stream));
    }
    return HB_OK;
}

