// hb_api_pass.inc - part of the hb_api.hip translation unit (included there; uses its hb_ctx and helpers).
// The pass driver: the kernel selectors, one pass in its three modes and how it is booked, the multi-GPU exchanges, the reference-tail
// mode, hb_run's tail pipeline, the load-time warm-up.
// ---- kernel dispatch ----------------------------------------------------------------------
// The run-time choices -> the template instance.  These selectors are the only place that names one: launch_pass, the sweep pass and
// warm_kernels all ask here, so what is warmed at load is what a run launches.
using PassKernel = void (*)(const hbk::PassParams);
using SweepKernel = void (*)(const hbk::SweepParams);

template <bool REAL, bool FUSED, bool STATS, bool INIT, bool EPI4, bool EARLY = false>
PassKernel dense_by_unroll(int unroll)
{
    if constexpr (!INIT) { // (the INIT form exists for 2 and 4 only)
        if (unroll == 1) return hbk::pass_kernel<REAL, FUSED, STATS, 1, INIT, EPI4, EARLY>;
    }
    if (unroll == 2) return hbk::pass_kernel<REAL, FUSED, STATS, 2, INIT, EPI4, EARLY>;
    return hbk::pass_kernel<REAL, FUSED, STATS, 4, INIT, EPI4, EARLY>;
}
template <bool REAL, bool FUSED>
PassKernel dense_kernel_of(bool stats, int unroll, bool init, bool epi4, bool early)
{
    if (stats) return dense_by_unroll<REAL, FUSED, true, false, false>(unroll); // (a counting pass has neither the INIT nor the EPI4 form)
    if constexpr (REAL == FUSED) {
        // EARLY: a row leaves its gather loop once its accumulator is >= U (the fused node rows and the hub chunks of a context that
        // skips saturated rows; never pass 0)
        if (early && !init) return epi4 ? dense_by_unroll<REAL, FUSED, false, false, REAL, true>(unroll) : dense_by_unroll<REAL, FUSED, false, false, false, true>(unroll);
    }
    if constexpr (REAL && FUSED) {
        // EPI4: the once-per-row estimator / Kahan epilogue (default for the fused node rows)
        if (epi4) return init ? dense_by_unroll<true, true, false, true, true>(unroll) : dense_by_unroll<true, true, false, false, true>(unroll);
    }
    return init ? dense_by_unroll<REAL, FUSED, false, true, false>(unroll) : dense_by_unroll<REAL, FUSED, false, false, false>(unroll);
}
// dense pass.  real: node rows (else hub chunks, which are never fused); init: pass 0, the sources' initial registers stream in with
// the edge list (hb_kernels.hip.h); early: the EARLY instances (launch_pass asks for them under early_exit_rule)
PassKernel dense_kernel(bool real, bool fused, bool stats, int unroll, bool init, bool epi4, bool early)
{
    init = init && unroll != 1;
    if (real && fused) return dense_kernel_of<true, true>(stats, unroll, init, epi4, early);
    if (real) return dense_kernel_of<true, false>(stats, unroll, init, false, false);
    return dense_kernel_of<false, false>(stats, unroll, init, false, early);
}

template <bool REAL, bool FUSED>
PassKernel bitmap_kernel_of(bool stats, bool compact)
{
    constexpr int W = REAL ? 4 : 16;
    if (stats) return compact ? hbk::frontier_kernel<REAL, FUSED, true, W, true> : hbk::frontier_kernel<REAL, FUSED, true, W, false>;
    return compact ? hbk::frontier_kernel<REAL, FUSED, false, W, true> : hbk::frontier_kernel<REAL, FUSED, false, W, false>;
}
// the bitmap pass: all indices / all bit words / needed gathers of a row as three batched round trips; !compact: gather slot by slot
PassKernel bitmap_kernel(bool real, bool fused, bool stats, bool compact)
{
    if (real && fused) return bitmap_kernel_of<true, true>(stats, compact);
    if (real) return bitmap_kernel_of<true, false>(stats, compact);
    return bitmap_kernel_of<false, false>(stats, compact);
}

// the rows of a sweep pass; by_rounds (experiments build): a touched row's sources 8 per round
SweepKernel sweep_rows_kernel_for(bool real, bool by_rounds)
{
#ifdef HB_EXPERIMENTS
    if (by_rounds) return real ? hbk::sweep_rows_kernel<true, true> : hbk::sweep_rows_kernel<false, true>;
#endif
    (void)by_rounds;
    return real ? hbk::sweep_rows_kernel<true> : hbk::sweep_rows_kernel<false>;
}

// gathers in flight: the low byte of tune[1], else 16 per quad for the hub chunks (pure gather loops) and 8 for the node rows, whose
// fused estimator/Kahan epilogue needs the registers (unroll 4 drops them to 3 waves/SIMD)
int pass_unroll(const hb_ctx *c, bool real)
{
    const int unroll = (int)(c->opt.tune[1] & HB_TUNE1_UNROLL);
    return (unroll == 1 || unroll == 2 || unroll == 4) ? unroll : (real ? 2 : 4);
}
// pass 0 of this context, when it is a dense pass, is the INIT launch
bool pass0_streams_initial_registers(const hb_ctx *c)
{
    return c->d_src_jp != nullptr && c->d_self_jp != nullptr && !(c->opt.flags & HB_FLAG_NO_INIT_PASS) && pass_unroll(c, true) != 1;
}

void launch_pass(hb_ctx *c, const hbk::PassParams &pp, bool real, bool frontier, bool fused, int level = -1)
{
    const bool stats = (c->opt.flags & HB_FLAG_PASS_STATS) != 0;
    const uint64_t ntiles = (pp.row_hi - pp.row_lo + 63) / 64;
    if (ntiles == 0) return;
    const bool init = c->t == 0 && !frontier && pass0_streams_initial_registers(c);
    // workgroups per CU: low byte of tune[0] = node rows, second byte = hub chunks (0 = default).  Measured
    // (profiles/r02s_sweep_bpc_*): the hub-chunk gather loop is fastest with only 2 workgroups (8 waves) per CU - each
    // quad already keeps 16 gathers in flight, more waves only add contention (dense pass -12 % at C3, -16 % at C4);
    // the bitmap pass has dependent bit tests in front of the gathers and wants 5 (83 VGPRs: 5 waves per SIMD fit).  Node rows: many small
    // workgroups, the hardware scheduler levels the uneven tiles (1.13 -> 1.05 ms at C3).
    uint32_t bpc = real ? (c->opt.tune[0] & 0xFFu) : ((c->opt.tune[0] >> 8) & 0xFFu);
    // pass 0 streams its sources: no L2 window to protect, the scratch-counter updates want every wave the CU can hold
    if (!bpc) bpc = real ? (frontier ? 32u : 64u) : (frontier ? 5u : (init ? 8u : 2u));
    PassKernel kernel;
    unsigned blocks;
    if (init && !real && level == 0 && c->level0_all_real && !stats && !xbit(c, HB_X_GENERIC_LEVEL1)) {
        kernel = hbk::init_level1_kernel; // pass 0, first level of hub chunks: the streaming kernel of its own
        blocks = grid_blocks(c, ntiles, 8);
    } else {
        blocks = grid_blocks(c, ntiles, bpc);
        if (pp.xcd_map) blocks = std::max((blocks + 7) / 8 * 8, 8u); // 8 queues, equal shares of the grid
        kernel = frontier ? bitmap_kernel(real, fused, stats, !xbit(c, HB_X_BITMAP_SLOTWISE))
                          : dense_kernel(real, fused, stats, pass_unroll(c, real), init, !xbit(c, HB_X_TILE_EPILOGUE), c->early_now && pp.sat != nullptr);
    }
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, c->stream, pp);
}

// ---- the initial state (harmonic.rs:53-73) ---------------------------------------------------------------------------------
// written by init_kernel - or, when pass 0 will be the fused INIT launch of ONE rank, left to that launch (PassParams::rd_init)
bool lean_pass0(const hb_ctx *c)
{
    return pass0_streams_initial_registers(c) && !unfused(c) && !multi_rank(c) && !linked(c) && !dest_mode(c) && !(c->opt.flags & HB_FLAG_PASS_STATS) &&
           !xbit(c, HB_X_FULL_INIT);
}
int launch_full_init(hb_ctx *c)
{
    const Plan &p = c->plan;
    if (!p.n_pad) return HB_OK;
    const unsigned blocks = (unsigned)((p.n_pad * 4 + 255) / 256);
    hipLaunchKernelGGL(hbk::init_kernel, dim3(blocks), dim3(256), 0, c->stream, c->d_idlow, (const uint32_t *)c->d_sid_of, p.n_pad, c->d_regs[0],
                       c->d_regs[1], c->d_ksum, c->d_kerr, c->d_size, c->d_bits[0], c->d_kdirty, c->d_raw, c->d_bias, c->d_lc);
    HB_HIP(hipGetLastError());
    return HB_OK;
}
// someone wants the state as hb_begin defines it before pass 0 has run (debug exports, hb_finish right behind hb_begin, a pass 0 that
// is not the lean launch after all): materialise it now
int ensure_initial_state(hb_ctx *c)
{
    if (!c->lean_init) return HB_OK;
    c->lean_init = false;
    return launch_full_init(c);
}

// live-first order (Plan::live_first, HB_FLAG_LIVE_FIRST): from pass 1 on the device rows at and behind n_live - the nodes without an
// in-edge - are neither gathered by a dense pass nor visited by the node-row launches.  Pass 0 is unchanged in both of its forms: it
// gathers every source (so every reader holds the dead sources' one register from then on), visits every row and leaves every row's
// counter in both buffers, its (0, 0) / lc[63] Kahan and size words in place and its changed / Kahan-dirty bits at zero.
bool skips_dead_rows(const hb_ctx *c) { return c->plan.live_first && c->t >= 1 && !unfused(c) && !linked(c); } // (a plan is only laid out so for such a context)

// saturated rows (DESIGN.md section 38): the dense passes t >= 1 of a context inside the gate neither gather for a row whose bit is set
// nor compute the hub chunks below it.  Pass 0 gathers everything and overwrites every partial (hb_begin relies on that).
bool skips_saturated_rows(const hb_ctx *c) { return c->d_sat != nullptr && c->t >= 1 && !unfused(c) && !linked(c); } // (d_sat exists only inside the gate)

// early exit (DESIGN.md section 39): the dense passes t >= 1 of a context that skips saturated rows run the EARLY instances - a row
// leaves its gather loop once its accumulator is >= U - when enough sources are saturated for rows to reach U before their lists end:
// the rows saturated so far hold at least 1/64 of the edges as sources (sat_out_sum, booked by step_finish).  Before that the per-round
// test only costs; a graph on which nothing saturates never launches one.  HB_FLAG_FORCE_EARLY_EXIT: from pass 1 on, whatever the sum
// says (tests); HB_FLAG_NO_EARLY_EXIT: never (A/B runs, tests).  Every choice gives the same bits.
bool early_exit_rule(const hb_ctx *c)
{
    if (!skips_saturated_rows(c) || (c->opt.flags & HB_FLAG_NO_EARLY_EXIT)) return false;
    return (c->opt.flags & HB_FLAG_FORCE_EARLY_EXIT) || (c->sat_out_sum && c->sat_out_sum * 64 >= c->m_global);
}

hbk::PassParams make_params(hb_ctx *c)
{
    const Plan &p = c->plan;
    hbk::PassParams pp{};
    pp.row_ptr = c->d_row_ptr;
    pp.src = c->d_src;
    pp.src_jp = c->d_src_jp;
    pp.rd = c->d_regs[c->cur];
    pp.wr = c->d_regs[c->cur ^ 1];
    pp.part = c->d_part;
    pp.bits_rd = c->d_bits[c->cur];
    pp.bits_wr = c->d_bits[c->cur ^ 1];
    pp.kdirty = c->d_kdirty;
    pp.ksum = c->d_ksum;
    pp.kerr = c->d_kerr;
    pp.size = c->d_size;
    pp.counters = c->d_counters + (size_t)hbk::kCounterWords * c->t;
    pp.outdeg = c->d_outdeg;
    pp.raw = c->d_raw;
    pp.bias = c->d_bias;
    pp.lc = c->d_lc;
    pp.n = p.n;
    pp.n_pad = p.n_pad;
    pp.rows_total = p.n_pad + p.nv;
    if (linked(c) || dest_mode(c)) {
        pp.slice_lo = (uint64_t)c->opt.rank * c->slice_rows;
        pp.slice_hi = std::min<uint64_t>(pp.slice_lo + c->slice_rows, p.n_pad);
    } else {
        pp.slice_lo = 0;
        pp.slice_hi = p.n_pad;
    }
    pp.t_plus_1 = (double)(c->t + 1);
    pp.rd_init = nullptr;
    pp.self_jp = c->d_self_jp;
    pp.virt_rows = c->d_virt_rows;
    pp.xflags = xbit(c, HB_X_PROBE_NO_SIZE) ? 1u : 0u;
    pp.live_limit = skips_dead_rows(c) ? (uint32_t)p.n_live : hbk::kNone;
    pp.sat = skips_saturated_rows(c) ? c->d_sat : nullptr; // (only the dense kernels read it)
    pp.sat_u = c->d_sat_u;
    pp.early_cnt = c->d_early;
    return pp;
}

bool changed_only(const hb_ctx *c) { return dest_mode(c) && (c->opt.flags & HB_FLAG_CHANGED_ONLY); }
// bytes of one packed counter in the destination partition's changed-only exchange: 6 bits per register (hb_aux.hip.h pack6_quarter:
// exact, the register set of this path has 60 members), or the 64-byte form (A/B)
uint64_t packed_row_bytes(const hb_ctx *c) { return xbit(c, HB_X_WIRE_64B) ? 64 : 48; }
// destination partition + changed-only on a communicator: the host round trip of a pass sits in its middle, the end is left in
// flight and the timing events are read later; such passes need event sets of their own (the six shared ones would be re-recorded
// by the next pass before they are read)
bool deferred_times(const hb_ctx *c) { return changed_only(c) && linked(c); }
int pass_events(hb_ctx *c, hipEvent_t **out)
{
    if (!deferred_times(c)) {
        // hb_run's tail pipeline keeps two passes in flight: pass t takes set t & 3 of a ring hb_create made (ADVICE r5: no event is created
        // inside a run, and none per pass index)
        *out = c->pipelined ? c->ev_ring[c->t & 3].e : c->ev;
        return HB_OK;
    }
    while (c->ev_pool.size() <= c->t) {
        hb_ctx::EvSet es{};
        for (auto &e : es.e)
            if (hipEventCreate(&e) != hipSuccess) return fail(c, HB_ERR_HIP, "hipEventCreate failed");
        c->ev_pool.push_back(es);
    }
    *out = c->ev_pool[c->t].e;
    return HB_OK;
}
// ms_gpu / ms_main / ms_level1 of a pass from its events (`end`: the last one it recorded); ms_collective is the caller's
int read_pass_times(hb_ctx *c, hipEvent_t *E, PassEvent end, hb_pass_stats *ps)
{
    HB_HIP(hipEventElapsedTime(&ps->ms_gpu, E[kEvStart], E[end]));
    HB_HIP(hipEventElapsedTime(&ps->ms_main, E[kEvLevels], E[kEvMerge]));
    if (ps->mode == 2 || (ps->mode < 2 && c->plan.level_begin.size() > 1)) HB_HIP(hipEventElapsedTime(&ps->ms_level1, E[kEvStart], E[kEvLevel1]));
    return HB_OK;
}
// ms_* of the passes whose end was left in flight (hb_finish, hb_get_pass_stats)
int resolve_pass_times(hb_ctx *c)
{
    for (uint64_t t : c->pending_times) {
        if (t >= c->pstats.size() || t >= c->ev_pool.size()) continue;
        hipEvent_t *E = c->ev_pool[t].e;
        hb_pass_stats &ps = c->pstats[t];
        HB_HIP(hipEventSynchronize(E[kEvCollective]));
        const int rc = read_pass_times(c, E, kEvCollective, &ps);
        if (rc) return rc;
        HB_HIP(hipEventElapsedTime(&ps.ms_collective, E[kEvMerge], E[kEvCollective]));
    }
    c->pending_times.clear();
    return HB_OK;
}
// plain edge partition on a communicator: pipeline merge / all-reduce / epilogue over row ranges
bool edge_overlap(const hb_ctx *c)
{
    // (HB_FLAG_PACKED_WIRE: one packed all-reduce over all rows; a packed form of the pipelined ranges waits for a wire to measure it on)
    return linked(c) && !dest_mode(c) && !ref_tail(c) && !(c->opt.flags & HB_FLAG_CHANGED_ONLY) && !xbit(c, HB_X_NO_EDGE_OVERLAP) && c->comm_stream && !packed_wire(c);
}
// edge partition (all-reduce) with HB_FLAG_CHANGED_ONLY: only the rows some rank's local merge changed are exchanged
bool edge_changed_only(const hb_ctx *c)
{
    return (c->opt.flags & HB_FLAG_CHANGED_ONLY) && !dest_mode(c) && !ref_tail(c) && (multi_rank(c) || linked(c));
}

// the changed-only exchanges' packed rows and the prefix sums over a row bitmap's words, allocated by the first pass that exchanges
int ensure_pack_buffers(hb_ctx *c)
{
    if (c->d_pack) return HB_OK;
    const uint64_t n_pad = c->plan.n_pad, words = n_pad / 32;
    int rc;
    if ((rc = dev_alloc(c, &c->d_pack, n_pad * 4))) return rc;
    if ((rc = dev_alloc(c, &c->d_wpop, words + 1))) return rc;
    return dev_alloc(c, &c->d_wprefix, words + 2);
}
// d_wprefix = exclusive prefix sums of the set bits in the words of `bits` (one bit per node row): the packed position of every row
int changed_word_prefix(hb_ctx *c, const uint32_t *bits)
{
    const uint64_t words = c->plan.n_pad / 32;
    if (words) {
        hipLaunchKernelGGL(hbk::popcount_words_kernel, dim3(grid_blocks(c, (words + 255) / 256, 8)), dim3(256), 0, c->stream, bits, words, c->d_wpop);
        HB_HIP(hipGetLastError());
    }
    const std::string e = device_prefix((void *)c->stream, c->d_wpop, words, c->d_wprefix);
    if (!e.empty()) return fail(c, HB_ERR_HIP, e);
    return HB_OK;
}

int edge_co_alloc(hb_ctx *c)
{
    if (c->d_lbits) return HB_OK;
    const uint64_t words = c->plan.n_pad / 32;
    const uint64_t world = (uint64_t)std::max(c->opt.world_size, 1);
    int rc;
    if ((rc = dev_alloc(c, &c->d_lbits, words + 2))) return rc;
    if ((rc = dev_alloc(c, &c->d_lbits_all, world * words + 2))) return rc;
    if ((rc = dev_alloc(c, &c->d_ubits, words + 2))) return rc;
    if ((rc = ensure_pack_buffers(c))) return rc;
    HB_HIP(hipMemsetAsync(c->d_lbits, 0, (words + 2) * 4, c->stream));
    return HB_OK;
}

// d_ubits holds the union: positions of its rows, their number (one read-back), this rank's rows packed
int edge_co_pack(hb_ctx *c)
{
    const Plan &p = c->plan;
    const uint64_t words = p.n_pad / 32;
    hbk::PassParams pp = make_params(c);
    const int rc = changed_word_prefix(c, c->d_ubits);
    if (rc) return rc;
    c->co_rows = 0;
    HB_HIP(hipMemcpyAsync(&c->co_rows, c->d_wprefix + words, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HB_HIP(hipStreamSynchronize(c->stream));
    if (c->co_rows) {
        hipLaunchKernelGGL(hbk::pack_changed_kernel, dim3((unsigned)((p.n_pad * 4 + 255) / 256)), dim3(256), 0, c->stream, (const uint4 *)pp.wr,
                           (const uint32_t *)c->d_ubits, (const uint64_t *)c->d_wprefix, (uint64_t)0, p.n_pad, c->d_pack);
        HB_HIP(hipGetLastError());
    }
    return HB_OK;
}

int edge_co_unpack(hb_ctx *c)
{
    const Plan &p = c->plan;
    hbk::PassParams pp = make_params(c);
    if (c->co_rows) {
        hipLaunchKernelGGL(hbk::unpack_rows_kernel, dim3((unsigned)((p.n_pad * 4 + 255) / 256)), dim3(256), 0, c->stream, pp.wr, (const uint32_t *)c->d_ubits,
                           (const uint64_t *)c->d_wprefix, p.n_pad, (const uint4 *)c->d_pack);
        HB_HIP(hipGetLastError());
    }
    c->ubits_valid = true;
    return HB_OK;
}

// changed-only exchange, step 1 (the changed bits of ALL slices are in bits_wr): prefix sums over the bitmap words,
// the packed position where every rank's run starts, and this rank's changed rows packed at their place
int exchange_pack(hb_ctx *c, const uint64_t *host_off = nullptr)
{
    const Plan &p = c->plan;
    const uint64_t S = c->slice_rows;
    const uint64_t world = (uint64_t)std::max(c->opt.world_size, 1), r = (uint64_t)c->opt.rank;
    int rc;
    if ((rc = ensure_pack_buffers(c))) return rc;
    hbk::PassParams pp = make_params(c);
    if ((rc = changed_word_prefix(c, pp.bits_wr))) return rc;
    c->ex_off.assign(world + 1, 0);
    if (host_off) { // the pass driver: the run offsets follow from the ranks' changed counts, which came with the pass counters
        for (uint64_t k = 0; k <= world; k++) c->ex_off[k] = host_off[k];
        static const bool check = std::getenv("HB_CHECK_EXCHANGE") != nullptr;
        if (check) {
            // ADVICE r5: the run LENGTHS come from the all-reduced per-rank counters, the pack / unpack POSITIONS from the prefix sums
            // over the all-gathered bitmap; they agree iff every rank's changed counter equals the popcount of its slice's bits.  Tests
            // (tests/conftest.py sets the variable) read the prefix sums back - the second round trip this path otherwise avoids.
            std::vector<uint64_t> dev_off(world + 1, 0);
            for (uint64_t k = 0; k <= world; k++)
                HB_HIP(hipMemcpyAsync(&dev_off[k], c->d_wprefix + std::min<uint64_t>(k * S, p.n_pad) / 32, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
            HB_HIP(hipStreamSynchronize(c->stream));
            for (uint64_t k = 0; k <= world; k++)
                if (dev_off[k] != host_off[k])
                    return fail(c, HB_ERR_INVALID, "changed-only exchange: rank " + std::to_string(k) + "'s run starts at " + std::to_string(host_off[k]) +
                                                       " by the ranks' changed counters but at " + std::to_string(dev_off[k]) + " by the changed bitmap (pass " + std::to_string(c->t) + ")");
        }
    } else {        // hb_debug_exchange (logical ranks on one device): read them back
        for (uint64_t k = 0; k <= world; k++)
            HB_HIP(hipMemcpyAsync(&c->ex_off[k], c->d_wprefix + std::min<uint64_t>(k * S, p.n_pad) / 32, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        HB_HIP(hipStreamSynchronize(c->stream));
    }
    const uint64_t lo = r * S, hi = std::min<uint64_t>(lo + S, p.n_pad);
    if (hi > lo) {
        if (packed_row_bytes(c) == 48)
            hipLaunchKernelGGL(hbk::pack6_changed_kernel, dim3((unsigned)(((hi - lo) * 4 + 255) / 256)), dim3(256), 0, c->stream, (const uint4 *)pp.wr,
                               (const uint32_t *)pp.bits_wr, (const uint64_t *)c->d_wprefix, lo, hi, (uint32_t *)c->d_pack);
        else
            hipLaunchKernelGGL(hbk::pack_changed_kernel, dim3((unsigned)(((hi - lo) * 4 + 255) / 256)), dim3(256), 0, c->stream, (const uint4 *)pp.wr,
                               (const uint32_t *)pp.bits_wr, (const uint64_t *)c->d_wprefix, lo, hi, c->d_pack);
        HB_HIP(hipGetLastError());
    }
    c->wire_bytes += (c->ex_off[world] - (c->ex_off[r + 1] - c->ex_off[r])) * packed_row_bytes(c) + (p.n_pad - (hi - lo)) / 8;
    return HB_OK;
}

// step 3 (the packed runs of all ranks are in d_pack): scatter the foreign ones
int exchange_unpack(hb_ctx *c)
{
    const Plan &p = c->plan;
    const uint64_t S = c->slice_rows, r = (uint64_t)c->opt.rank;
    hbk::PassParams pp = make_params(c);
    const uint64_t lo = r * S, hi = std::min<uint64_t>(lo + S, p.n_pad);
    const uint64_t ranges[2][2] = {{0, lo}, {hi, p.n_pad}};
    for (auto &rg : ranges) {
        if (rg[1] <= rg[0]) continue;
        if (packed_row_bytes(c) == 48)
            hipLaunchKernelGGL(hbk::unpack6_changed_kernel, dim3((unsigned)(((rg[1] - rg[0]) * 4 + 255) / 256)), dim3(256), 0, c->stream, pp.wr, pp.rd,
                               (const uint32_t *)pp.bits_wr, pp.bits_rd, (const uint64_t *)c->d_wprefix, rg[0], rg[1], (const uint32_t *)c->d_pack);
        else
            hipLaunchKernelGGL(hbk::unpack_changed_kernel, dim3((unsigned)(((rg[1] - rg[0]) * 4 + 255) / 256)), dim3(256), 0, c->stream, pp.wr, pp.rd,
                               (const uint32_t *)pp.bits_wr, pp.bits_rd, (const uint64_t *)c->d_wprefix, rg[0], rg[1], (const uint4 *)c->d_pack);
        HB_HIP(hipGetLastError());
    }
    return HB_OK;
}

// ---- whole counters as 48-byte rows (HB_FLAG_PACKED_WIRE, DESIGN.md section 40) ------------------------------------------------
// d_w6[0..nbuf): world x wire6_slice packed rows each.  The slice is >= ceil(n_pad / world) in both decompositions, so the buffers hold
// the pieces of every exchange below: the destination partition's slices, the edge partition's (plain: one slice per piece;
// changed-only: ceil(co_rows / world) rows, never more than a slice).  Allocated by the first pass that exchanges, like ensure_pack_buffers.
// rows per rank's slice: the destination partition's owner slice; on the edge partition the Kahan slice of a linked context
// (slice_rows) - which logical ranks without collectives (hb_debug_exchange) do not have, so it is restated here
uint64_t wire6_slice(const hb_ctx *c)
{
    const uint64_t world = (uint64_t)std::max(c->opt.world_size, 1);
    return dest_mode(c) ? c->slice_rows : ((c->plan.n_pad + world - 1) / world + 63) / 64 * 64;
}
int ensure_wire6_buffers(hb_ctx *c, int nbuf)
{
    const uint64_t world = (uint64_t)std::max(c->opt.world_size, 1);
    for (int k = 0; k < nbuf; k++) {
        if (c->d_w6[k]) continue;
        const int rc = dev_alloc(c, &c->d_w6[k], world * wire6_slice(c) * 12 + 4);
        if (rc) return rc;
    }
    return HB_OK;
}
unsigned wire6_blocks(const hb_ctx *c, uint64_t rows) { return grid_blocks(c, (rows * 4 + 255) / 256, 16, 1); }
// "R rows of 64 bytes, present on every rank, to be max-reduced everywhere" in its five steps; S = rows per slice (world x S >= R).
// hb_debug_exchange runs the same three launches with device copies between them.
// step 1: all R rows packed into d_w6[0], the tail of the last pieces padded with zero codes
int wire6_pack_all(hb_ctx *c, const uint4 *rows, uint64_t R, uint64_t S, hipStream_t stream)
{
    const uint64_t world = (uint64_t)std::max(c->opt.world_size, 1);
    if (world * S < R || S > wire6_slice(c)) return fail(c, HB_ERR_INVALID, "packed all-reduce: the slices do not cover the rows");
    const int rc = ensure_wire6_buffers(c, 2);
    if (rc) return rc;
    if (!S) return HB_OK;
    hipLaunchKernelGGL(hbk::pack6_rows_kernel, dim3(wire6_blocks(c, world * S)), dim3(256), 0, stream, rows, R, world * S, c->d_w6[0]);
    HB_HIP(hipGetLastError());
    return HB_OK;
}
// step 3: the maximum over the `world` pieces of rank `rank`'s slice that the all-to-all left in d_w6[1], packed, at its place in d_w6[0]
int wire6_reduce_slice(hb_ctx *c, uint64_t S, uint64_t rank, hipStream_t stream)
{
    if (!S) return HB_OK;
    hipLaunchKernelGGL(hbk::max6_pieces_kernel, dim3(wire6_blocks(c, S)), dim3(256), 0, stream, (const uint32_t *)c->d_w6[1], S * 12, (uint32_t)std::max(c->opt.world_size, 1), S,
                       c->d_w6[0] + rank * S * 12);
    HB_HIP(hipGetLastError());
    return HB_OK;
}
// step 5: d_w6[0] holds every rank's reduced slice: back to 64-byte rows
int wire6_unpack_all(hb_ctx *c, uint4 *rows, uint64_t R, hipStream_t stream)
{
    if (!R) return HB_OK;
    hipLaunchKernelGGL(hbk::unpack6_rows_kernel, dim3(wire6_blocks(c, R)), dim3(256), 0, stream, (const uint32_t *)c->d_w6[0], R, rows);
    HB_HIP(hipGetLastError());
    return HB_OK;
}
int packed_all_reduce_max(hb_ctx *c, uint4 *rows, uint64_t R, uint64_t S, hipStream_t stream)
{
    const uint64_t r = (uint64_t)c->opt.rank;
    int rc;
    if ((rc = wire6_pack_all(c, rows, R, S, stream))) return rc;
    HB_COLL(coll_all_to_all(c, c->d_w6[0], c->d_w6[1], S * 48, stream));                            // step 2
    if ((rc = wire6_reduce_slice(c, S, r, stream))) return rc;
    HB_COLL(coll_all_gather(c, c->d_w6[0] + r * S * 12, c->d_w6[0], S * 48, ncclUint8, stream));   // step 4 (in place)
    return wire6_unpack_all(c, rows, R, stream);
}
// destination partition, full form: this rank's slice of the pending counters packed at its place in d_w6[0] ...
int wire6_pack_own_slice(hb_ctx *c)
{
    const Plan &p = c->plan;
    const uint64_t S = c->slice_rows, r = (uint64_t)c->opt.rank;
    const int rc = ensure_wire6_buffers(c, 1);
    if (rc) return rc;
    const uint64_t lo = std::min<uint64_t>(r * S, p.n_pad), hi = std::min<uint64_t>(lo + S, p.n_pad);
    if (!S) return HB_OK;
    hbk::PassParams pp = make_params(c);
    hipLaunchKernelGGL(hbk::pack6_rows_kernel, dim3(wire6_blocks(c, S)), dim3(256), 0, c->stream, (const uint4 *)(pp.wr + lo * 4), hi - lo, S, c->d_w6[0] + r * S * 12);
    HB_HIP(hipGetLastError());
    return HB_OK;
}
// ... and, once the slices of all ranks are there, the foreign ones unpacked into the pending counters (the own slice is not rewritten)
int wire6_unpack_foreign_slices(hb_ctx *c)
{
    const Plan &p = c->plan;
    const uint64_t S = c->slice_rows, r = (uint64_t)c->opt.rank;
    hbk::PassParams pp = make_params(c);
    const uint64_t lo = std::min<uint64_t>(r * S, p.n_pad), hi = std::min<uint64_t>(lo + S, p.n_pad);
    const uint64_t ranges[2][2] = {{0, lo}, {hi, p.n_pad}};
    for (auto &rg : ranges) {
        if (rg[1] <= rg[0]) continue;
        hipLaunchKernelGGL(hbk::unpack6_rows_kernel, dim3(wire6_blocks(c, rg[1] - rg[0])), dim3(256), 0, c->stream, (const uint32_t *)(c->d_w6[0] + rg[0] * 12), rg[1] - rg[0],
                           pp.wr + rg[0] * 4);
        HB_HIP(hipGetLastError());
    }
    c->wire_bytes += (p.n_pad - std::min<uint64_t>(S, p.n_pad)) * 48 + (p.n_pad - std::min<uint64_t>(S, p.n_pad)) / 8;
    return HB_OK;
}
// what a rank receives in one packed all-reduce: world - 1 pieces in the all-to-all, world - 1 slices in the all-gather
uint64_t wire6_all_reduce_bytes(const hb_ctx *c, uint64_t S) { return 2 * (uint64_t)(std::max(c->opt.world_size, 1) - 1) * S * 48; }
// edge partition + changed-only: the union's co_rows rows in slices of ceil(co_rows / world); booked without the padding of the last
// piece, 3/4 of what the 64-byte all-reduce books
uint64_t wire6_co_slice(const hb_ctx *c) { return (c->co_rows + (uint64_t)std::max(c->opt.world_size, 1) - 1) / (uint64_t)std::max(c->opt.world_size, 1); }
uint64_t wire6_co_bytes(const hb_ctx *c)
{
    const uint64_t world = (uint64_t)std::max(c->opt.world_size, 1);
    return world > 1 ? 2 * (world - 1) * c->co_rows * 48 / world : 0;
}

// ---- reference-tail mode ---------------------------------------------------------------------------------
// bloom/src/lib.rs:38-41
uint64_t bloom_num_bits(uint64_t estimated_items, double fp)
{
    const double ln2 = std::log(2.0);
    return (uint64_t)std::ceil((double)estimated_items * std::log(fp) / (-8.0 * (ln2 * ln2)));
}
// bloom/src/lib.rs:108-123: the logarithm is cast to i64 BEFORE the multiplication; a negative product -> 0
uint64_t bloom_estimate_card(uint64_t num_bits, uint64_t num_ones)
{
    if (num_ones == 0 || num_bits == 0) return 0;
    if (num_ones == num_bits) return ~0ull;
    const int64_t l = (int64_t)std::log(1.0 - (double)num_ones / (double)num_bits);
    const int64_t v = -(int64_t)num_bits * l;
    return v < 0 ? 0 : (uint64_t)v;
}

// update_changed_counters (harmonic.rs:75-114): counters.new starts as the clone of counters.old (Counters::step),
// the changed nodes push their OLD counter along the page-level records; everything else (changed bits, sizes,
// Kahan) is the unfused epilogue of step_finish, like after any other pass
int tail_pass(hb_ctx *c, const hbk::PassParams &pp)
{
    const Plan &p = c->plan;
    c->cur_mode = 3;
    c->stale = true;
    unsigned int *d_len = (unsigned int *)(c->d_bloom_ones + 1);
    HB_HIP(hipMemcpyAsync(pp.wr, pp.rd, p.n_pad * 64, hipMemcpyDeviceToDevice, c->stream));
    HB_HIP(hipMemsetAsync(d_len, 0, sizeof(unsigned int), c->stream));
    hipLaunchKernelGGL(hbk::changed_list_kernel, dim3(grid_blocks(c, p.n_pad / 256, 8, 1)), dim3(256), 0, c->stream, pp.bits_rd, p.n_pad, c->d_list, d_len,
                       (uint32_t)(c->ref_threshold + 1));
    HB_HIP(hipEventRecord(c->ev[kEvLevel1], c->stream));
    HB_HIP(hipEventRecord(c->ev[kEvLevels], c->stream));
    hipLaunchKernelGGL(hbk::tail_merge_kernel, dim3(grid_blocks(c, (c->last_changed + 3) / 4, 8, 1)), dim3(256), 0, c->stream, (const uint32_t *)c->d_list, (const unsigned int *)d_len,
                       (const uint64_t *)c->d_tail_ptr, (const uint32_t *)c->d_tail_to, (const uint32_t *)pp.rd, (uint32_t *)pp.wr);
    HB_HIP(hipEventRecord(c->ev[kEvMerge], c->stream));
    HB_HIP(hipGetLastError());
    c->pending_local = true;
    return HB_OK;
}

// after a pass: new_changed_nodes as the reference builds it, and the exact-counting switch (harmonic.rs:273-279)
int reference_changed_state(hb_ctx *c, const uint32_t *bits_changed, uint64_t changed)
{
    const Plan &p = c->plan;
    const bool tracked = c->cur_mode == 3 || c->exact_counting; // this pass ran with Some(&mut exact_changed_nodes)
    if (!c->exact_counting || c->stale) {
        const uint64_t words = (c->bloom_bits + 31) / 32;
        HB_HIP(hipMemsetAsync(c->d_bloom, 0, (words + 1) * 4, c->stream));
        HB_HIP(hipMemsetAsync(c->d_bloom_ones, 0, sizeof(unsigned long long), c->stream));
        unsigned long long ones = 0;
        if (changed && c->bloom_bits) {
            hipLaunchKernelGGL(hbk::bloom_insert_kernel, dim3(grid_blocks(c, p.n_pad / 256, 8, 1)), dim3(256), 0, c->stream, bits_changed, (const uint64_t *)c->d_idlow, p.n_pad,
                               c->bloom_bits, c->d_bloom);
            if (!c->exact_counting) {
                hipLaunchKernelGGL(hbk::bloom_count_kernel, dim3(grid_blocks(c, words / 256, 8, 1)), dim3(256), 0, c->stream, (const uint32_t *)c->d_bloom, words, c->d_bloom_ones);
                HB_HIP(hipMemcpyAsync(&ones, c->d_bloom_ones, sizeof(ones), hipMemcpyDeviceToHost, c->stream));
                HB_HIP(hipStreamSynchronize(c->stream));
            }
            HB_HIP(hipGetLastError());
        }
        if (!c->exact_counting && bloom_estimate_card(c->bloom_bits, ones) <= c->ref_threshold) c->exact_counting = true;
    }
    c->exact_valid = tracked;
    return HB_OK;
}

// tail_keys -> d_tail_ptr / d_tail_to (hb_begin, when records were given since the last upload)
int upload_tail_index(hb_ctx *c)
{
    const Plan &p = c->plan;
    std::vector<uint64_t> ptr;
    std::vector<uint32_t> to;
    const std::string e = build_tail_csr(&c->tail_keys, p.n_pad, &ptr, &to);
    if (!e.empty()) return fail(c, HB_ERR_NOMEM, e);
    for (void *old : {(void *)c->d_tail_ptr, (void *)c->d_tail_to}) {
        if (!old) continue;
        for (size_t i = 0; i < c->allocs.size(); i++)
            if (c->allocs[i].p == old) {
                c->stats.device_bytes -= c->allocs[i].bytes;
                (void)hipFree(old); // (one entry leaves the `allocs` list before the graph does: the list is its owner, this its only early exit)
                c->allocs.erase(c->allocs.begin() + (long)i);
                break;
            }
    }
    c->d_tail_ptr = nullptr;
    c->d_tail_to = nullptr;
    int rc;
    if ((rc = dev_alloc(c, &c->d_tail_ptr, p.n_pad + 1))) return rc;
    if ((rc = dev_alloc(c, &c->d_tail_to, to.size() + 1))) return rc;
    HB_HIP(hipMemcpyAsync(c->d_tail_ptr, ptr.data(), (p.n_pad + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    if (!to.empty()) HB_HIP(hipMemcpyAsync(c->d_tail_to, to.data(), to.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HB_HIP(hipStreamSynchronize(c->stream));
    c->tail_count = to.size();
    c->tail_dirty = false;
    return HB_OK;
}

// ---- the mode of a pass ------------------------------------------------------------------------------------------------------------------
// A_t = edges whose source changed in the previous pass (= out-degree sum of those nodes, counted by the previous pass).  dense: every
// source is gathered (no test) - while most nodes still change the frontier test would only cost; bitmap (frontier): every index is read
// and bit-tested, only active sources are gathered (pays while A_t < ~half of the edges); sweep (sparse): only the work rows that read a
// changed node are visited at all - the convergence tail.  Every mode gives the same bits (SURVEY App. C-1).
using hbk::PassMode; // (hb_walk.hip.h: one numbering for the passes, the walks' levels, their kernels and the statistics)
using hbk::kModeDense;
using hbk::kModeBitmap;
using hbk::kModeSweep;
// A_t < tune[2] % of the edges (default 50)
bool below_dense_threshold(const hb_ctx *c, uint64_t active_edges)
{
    const uint32_t thr = c->opt.tune[2] ? c->opt.tune[2] : 50;
    return active_edges * 100ull < (uint64_t)thr * c->m_global;
}
PassMode pass_mode(const hb_ctx *c, uint64_t active_edges)
{
    if ((c->opt.flags & HB_FLAG_NO_FRONTIER) || !(below_dense_threshold(c, active_edges) || c->opt.tune[2] > 100)) return kModeDense;
    // sweep when A_t * tune[6] < edges: measured crossover with the bitmap pass at A_t = 10-12 % of the edges
    // (profiles/r02c_sweep_*: 7.4 % -> 1.25 ms vs 2.15 ms, 16 % -> 4.1 ms vs 2.1 ms on the C3-sized graphs)
    const uint64_t sparse_div = c->opt.tune[6] ? c->opt.tune[6] : 10;
    return c->sparse_ok && (active_edges * sparse_div < c->m_global || c->opt.tune[6] == 1) ? kModeSweep : kModeBitmap;
}

// ---- results that travel while the passes run ------------------------------------------------------------------------------
// A snapshot: out[] (ascending-NodeID order, normalised) is refreshed from the current sums on the MAIN stream (between two
// passes: ~2.3 ms at C4 when every row is new, 1.1 ms for a third of them) and downloaded on the side stream while the next pass
// runs; hb_finish then ships only what moved afterwards.  The kernel on the side stream as well - it may read sums the next pass
// is rewriting: an aligned 8-byte load returns the old or the new value, and whichever it returns is what sent[] records, so the
// final comparison stays exact - was built and measured (profiles/r05d_*): the pass it runs beside is request-bound and simply
// takes that much longer (C4 pass 5: 34.0 -> 36.5 ms, the C3 bitmap pass 1.48 -> 1.85 ms); only the copy overlaps for free.
int results_stage(hb_ctx *c)
{
    const Plan &p = c->plan;
    auto &rs = c->rs;
    const double norm = (double)(p.n ? p.n - 1 : 0);
    hipLaunchKernelGGL(hbk::results_sync_kernel, dim3(grid_blocks(c, (p.n_pad + 2047) / 2048, 8)), dim3(256), 0, c->stream, (const double *)c->d_ksum, rs.d_sent, (const uint32_t *)c->d_cid_of,
                       p.n_pad, norm, rs.valid ? 0 : 1, c->d_out, (uint32_t *)nullptr, (double *)nullptr, 0ull, rs.d_count, rs.d_kept);
    HB_HIP(hipGetLastError());
    HB_HIP(hipEventRecord(c->rs_ready, c->stream));
    HB_HIP(hipStreamWaitEvent(c->rs_stream, c->rs_ready, 0));
    HB_HIP(hipMemcpyAsync(c->h_out, c->d_out, c->out_len * sizeof(double), hipMemcpyDeviceToHost, c->rs_stream)); // (compact image: hb_ctx::out_len entries)
    HB_HIP(hipEventRecord(c->rs_copied, c->rs_stream));
    if (std::getenv("HB_TRACE_RESULTS")) std::fprintf(stderr, "[hb results] snapshot %u queued after pass %llu at %.3f ms (host clock)\n", rs.stages + 1, (unsigned long long)c->t - 1, now_ms());
    rs.valid = true;
    rs.changed_since = 0;
    rs.stages++;
    return HB_OK;
}
// after pass t (the loop goes on): is now the time for a snapshot?  The first one when the NEXT pass is no longer a dense one (A_{t+1}
// below_dense_threshold): the pass that just ended is then the last one that moved most sums.  [r6] Rounds 4-5 took
// it at A_{t+1} <= 90 % of the edges; at C4 that is after pass 4 (A_5 = 79 %), pass 5 then moves 35.5 M of the 99 M sums again and a
// second full image follows - the first snapshot's 2.4 ms on the main stream bought nothing (HB_TRACE_RESULTS timeline,
// profiles/r06d_*).  Again whenever more than n / 8 sums moved since and the previous download is over (hb_finish's list holds n / 8).
int results_stage_policy(hb_ctx *c, uint64_t changed)
{
    auto &rs = c->rs;
    if (!rs.on || !c->has_changes) return HB_OK;
    rs.changed_since += changed;
    const bool forced = xbit(c, HB_X_SNAPSHOT_EVERY_PASS);
    bool go;
    if (!rs.valid) go = forced || below_dense_threshold(c, c->last_active);
    else go = (forced || rs.changed_since * 8 > c->plan.n) && !xbit(c, HB_X_ONE_SNAPSHOT) && hipEventQuery(c->rs_copied) == hipSuccess;
    (void)hipGetLastError(); // (hipErrorNotReady of the query is not an error)
    return go ? results_stage(c) : HB_OK;
}

// the parameters of the sweep kernels around `pp`.  The seed / heavy counters live in two slots used by alternate passes: a pass' first
// kernel zeroes the other one (no memset launch per pass; hb_begin clears both)
hbk::SweepParams make_sweep_params(const hb_ctx *c, const hbk::PassParams &pp, unsigned slot, const unsigned long long *guard)
{
    hbk::SweepParams sp{};
    sp.p = pp;
    sp.out_ptr = c->d_out_ptr;
    sp.out_rows = c->d_out_rows;
    sp.touch = c->d_touch;
    sp.seeds = c->d_seeds;
    sp.heavy = c->d_heavy;
    sp.counts = c->d_sparse_counts + 2 * slot;
    sp.counts_next = c->d_sparse_counts + 2 * (slot ^ 1);
    sp.guard = guard;
    return sp;
}

// Sweep mode, first step: the changed node rows -> touch bits of their readers.  `small` (few changed rows): one launch instead of
// collect + expand + heavy.  Shared by sweep_pass and walk_forward_level (hb_api_walk.inc); the caller checks hipGetLastError.
void launch_sweep_seeding(hb_ctx *c, const hbk::SweepParams &sp, bool small)
{
    const unsigned sblocks = grid_blocks(c, sp.p.n_pad / 32 / 256, 4, 1);
    const unsigned wblocks = (unsigned)c->num_cu * 4;
    if (small) {
        hipLaunchKernelGGL(hbk::sweep_seed_small_kernel, dim3(sblocks), dim3(256), 0, c->stream, sp);
    } else {
        hipLaunchKernelGGL(hbk::sweep_collect_kernel, dim3(sblocks), dim3(256), 0, c->stream, sp);
        hipLaunchKernelGGL(hbk::sweep_expand_kernel, dim3(wblocks), dim3(256), 0, c->stream, sp);
        hipLaunchKernelGGL(hbk::sweep_expand_heavy_kernel, dim3(wblocks), dim3(256), 0, c->stream, sp);
    }
}

// ---- one pass, first half: its launches (step_local) -------------------------------------------------------------------------------------
// sweep mode: changed nodes -> touch bits of their readers; then the levels, then the node rows.  No bitmap is cleared: the sweep
// kernels rewrite every word of this pass' changed bits (node rows in bits_wr, virtual rows in the upper part of bits_rd) and keep the
// touch bitmap all-zero between passes
int sweep_pass(hb_ctx *c, const hbk::PassParams &pp, hipEvent_t *E)
{
    const Plan &p = c->plan;
    hbk::SweepParams sp = make_sweep_params(c, pp, (unsigned)(c->t & 1), c->spec_guard);
    launch_sweep_seeding(c, sp, c->last_changed <= 4096 && !xbit(c, HB_X_SEED_3LAUNCH)); // convergence tail: the one-launch form
    HB_HIP(hipEventRecord(E[kEvLevel1], c->stream)); // sweep passes: ms_level1 = seed collection + expansion
    const bool by_rounds = xbit(c, HB_X_SWEEP_ROUNDS);
    auto launch_rows = [&](bool real, uint64_t lo, uint64_t hi) {
        if (hi <= lo) return;
        sp.p.row_lo = lo;
        sp.p.row_hi = hi;
        const uint64_t waves = (hi - lo + 2047) / 2048; // a wave-iteration covers 16 groups of 128 rows
        hipLaunchKernelGGL(sweep_rows_kernel_for(real, by_rounds), dim3(grid_blocks(c, (waves + 3) / 4, 4, 1)), dim3(256), 0, c->stream, sp);
    };
    for (size_t l = 0; l + 1 < p.level_begin.size(); l++) launch_rows(false, p.level_begin[l], p.level_begin[l + 1]);
    HB_HIP(hipEventRecord(E[kEvLevels], c->stream));
    launch_rows(true, 0, p.n_pad);
    HB_HIP(hipEventRecord(E[kEvMerge], c->stream));
    return HB_OK;
}

// dense / bitmap mode: the hub-chunk levels bottom-up, then the node rows (in ranges when the exchange overlaps the merge: edge_overlap)
int level_pass(hb_ctx *c, hbk::PassParams pp, hipEvent_t *E, bool frontier, bool fused, bool lean)
{
    const Plan &p = c->plan;
    c->early_now = !frontier && pp.sat && early_exit_rule(c);
    if (!frontier) c->last_dense_early = c->early_now;
    if (c->early_now) HB_HIP(hipMemsetAsync(c->d_early, 0, hbk::kStripes * sizeof(unsigned long long), c->stream));
    for (size_t l = 0; l + 1 < p.level_begin.size(); l++) {
        pp.row_lo = p.level_begin[l];
        pp.row_hi = p.level_begin[l + 1];
        pp.xcd_map = (l == 0 && p.xcd_groups == 8) ? 1 : 0;
        for (int x = 0; x < 8; x++) {
            pp.xcd_lo[x] = p.xcd_begin[x];
            pp.xcd_hi[x] = p.xcd_begin[x + 1];
        }

#ifdef HB_EXPERIMENTS
        const uint32_t lds_tile = std::min<uint32_t>(c->opt.tune[7], 2048u); // experiment, see hub_lds_tile_kernel (hb_experiments.hip.h)
        if (l == 0 && !frontier && lds_tile && !(c->opt.flags & HB_FLAG_PASS_STATS) && !multi_rank(c)) {
            const uint64_t ntiles = (pp.row_hi - pp.row_lo + 63) / 64;
            const size_t lds = (size_t)lds_tile * 64;
            const uint64_t per_cu = std::max<uint64_t>(1, std::min<uint64_t>(8, (160 * 1024) / (lds + 1024)));
            unsigned blocks = grid_blocks(c, ntiles, per_cu);
            if (pp.xcd_map) blocks = std::max((blocks + 7) / 8 * 8, 8u);
            if (lds > 48 * 1024)
                HB_HIP(hipFuncSetAttribute((const void *)hbk::hub_lds_tile_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            if (ntiles) hipLaunchKernelGGL(hbk::hub_lds_tile_kernel, dim3(blocks), dim3(256), lds, c->stream, pp, lds_tile);
        } else
#endif
        {
            launch_pass(c, pp, false, frontier, false, (int)l);
        }
        if (l == 0) HB_HIP(hipEventRecord(E[kEvLevel1], c->stream));
    }
    pp.xcd_map = 0;
    HB_HIP(hipEventRecord(E[kEvLevels], c->stream));
    pp.row_lo = dest_mode(c) ? pp.slice_lo : 0; // destination partition: only the owned rows
    pp.row_hi = dest_mode(c) ? pp.slice_hi : (skips_dead_rows(c) ? p.n_live_pad : p.n_pad);
    if (edge_changed_only(c)) {
        int rc = edge_co_alloc(c);
        if (rc) return rc;
        pp.lbits = c->d_lbits; // which rows the local merge changed
        c->ubits_valid = false;
    }
    c->ov_ranges = 0;
    if (edge_overlap(c) && p.n_pad >= 64ull * hb_ctx::kOverlap) {
        // the node rows in kOverlap ranges: range k is all-reduced (step_finish, comm_stream) while k + 1 is merged here
        const uint64_t tiles = p.n_pad / 64;
        for (int k = 0; k <= hb_ctx::kOverlap; k++) c->ov_lo[k] = tiles * (uint64_t)k / hb_ctx::kOverlap * 64;
        c->ov_ranges = hb_ctx::kOverlap;
        for (int k = 0; k < hb_ctx::kOverlap; k++) {
            pp.row_lo = c->ov_lo[k];
            pp.row_hi = c->ov_lo[k + 1];
            launch_pass(c, pp, true, frontier, fused);
            HB_HIP(hipEventRecord(c->ov_merged[k], c->stream));
        }
    } else {
        if (lean) pp.rd_init = c->d_regs[c->cur];
        launch_pass(c, pp, true, frontier, fused);
        if (p.live_first && c->t == 0 && p.n_live_pad < p.n_pad) {
            // hb_begin put EVERY node into the changed set (harmonic.rs:221-225) and pass 0 has consumed it.  Nobody rewrites the dead
            // rows' words of that buffer from here on (pass 1 writes its changed bits there, for the live rows only): clear them once,
            // so that no later bitmap or sweep pass finds a dead row "changed" (n_live_pad is a multiple of 64: whole words)
            HB_HIP(hipMemsetAsync(c->d_bits[c->cur] + p.n_live_pad / 32, 0, (p.n_pad - p.n_live_pad) / 32 * sizeof(uint32_t), c->stream));
        }
        if (!frontier && pp.sat) {
            // the node rows have marked the top chunks of every hub row that is saturated now: hand the bit down the trees, top level
            // first, so that the next dense pass skips all of them (a first level known to read node rows only has nothing below it)
            for (size_t l = p.level_begin.empty() ? 0 : p.level_begin.size() - 1; l-- > 0;) {
                const uint64_t lo = p.level_begin[l], hi = p.level_begin[l + 1];
                if (hi > lo && !(l == 0 && c->level0_all_real))
                    hipLaunchKernelGGL(hbk::sat_down_kernel, dim3(grid_blocks(c, (hi - lo + 63) / 64, 8)), dim3(256), 0, c->stream, (const uint64_t *)c->d_row_ptr,
                                       (const uint32_t *)c->d_src, lo, hi, p.n_pad, c->d_sat);
            }
        }
    }
    HB_HIP(hipEventRecord(E[kEvMerge], c->stream));
    return HB_OK;
}

// reference-tail mode, the pass after a tail pass (update_all_counters): sources pass `changed_nodes.contains_u128` (harmonic.rs:133) -
// the bloom filter of the previous pass' changed nodes INCLUDING its false positives (they may hold updates a tail pass did not
// deliver) become this pass' frontier bits
int bloom_frontier_prelude(hb_ctx *c)
{
    const Plan &p = c->plan;
    hipLaunchKernelGGL(hbk::bloom_frontier_kernel, dim3((unsigned)(p.n_pad / 256 + 1)), dim3(256), 0, c->stream, (const uint32_t *)c->d_bloom,
                       (const uint64_t *)c->d_idlow, (const uint32_t *)c->d_sid_of, p.n_pad, c->bloom_bits, c->d_bits[c->cur]);
    HB_HIP(hipGetLastError());
    return HB_OK;
}

int step_local(hb_ctx *c)
{
    if (!c->run_open) return fail(c, HB_ERR_INVALID, "hb_step*: call hb_begin first");
    c->tl_valid = false;    // (the bitmaps are about to be rewritten by other kernels: the tail kernel's lists no longer describe them)
    c->tl_declined = false;
    if (c->pending_local) return fail(c, HB_ERR_INVALID, "hb_step_local called twice");
    if (c->t >= c->max_passes) return fail(c, HB_ERR_LIMIT, "max_passes exceeded");
    // a pass of hb_run's tail pipeline is ALWAYS a sweep pass: only the sweep kernels carry the device guard, and pass_mode would see
    // the A_t of two passes ago (a late change of one node with a large out-degree share could ask for a bitmap or dense pass: found
    // by tools/diff_fuzz.py on the MI355X, round 5)
    c->cur_mode = c->pipelined ? kModeSweep : (c->t > 0 ? pass_mode(c, c->last_active) : kModeDense);
    const bool fused = !unfused(c);
    // lean pass 0: only the fused dense INIT launch of one rank derives the initial state itself; anything else finds it in memory
    const bool lean = c->lean_init && c->t == 0 && c->cur_mode == kModeDense && fused && lean_pass0(c);
    if (c->lean_init && !lean) {
        const int rc_init = ensure_initial_state(c);
        if (rc_init) return rc_init;
    }
    c->lean_init = false;
    if (c->t == 0 && std::getenv("HB_TRACE_INIT")) std::fprintf(stderr, "[hb init] pass 0 runs %s\n", lean ? "lean (derives the initial state itself)" : "on the state init_kernel wrote");
    const hbk::PassParams pp = make_params(c);
    hipEvent_t *E = nullptr; // this pass' timing events (hb_ctx::ev, or a set of its own: deferred_times)
    int rc = pass_events(c, &E);
    if (rc) return rc;
    HB_HIP(hipEventRecord(E[kEvStart], c->stream));
    if (ref_tail(c)) {
        // harmonic.rs:244-246: `!exact_changed_nodes.is_empty() && exact_changed_nodes.len() <= threshold`
        if (c->exact_valid && c->last_changed != 0 && c->last_changed <= c->ref_threshold) return tail_pass(c, pp);
        if (c->stale && c->t > 0) {
            c->cur_mode = kModeBitmap; // never a dense pass (it would deliver all updates); the sweep support is never built in this mode (it runs unfused)
            if ((rc = bloom_frontier_prelude(c))) return rc;
        }
    }
    rc = c->cur_mode == kModeSweep ? sweep_pass(c, pp, E) : level_pass(c, pp, E, c->cur_mode == kModeBitmap, fused, lean);
    if (rc) return rc;
    HB_HIP(hipGetLastError());
    c->pending_local = true;
    return HB_OK;
}

// ---- one pass, second half: exchange, epilogue, read-back and booking ------------------------------------------------------------------
// the four counters of a pass - changed nodes, gathered edges (HB_FLAG_PASS_STATS), touched rows, A_{t+1} - summed over their stripes
// (hb_kernels.hip.h); sum may be h itself
void sum_stripes(const unsigned long long *h, unsigned long long *sum)
{
    for (int k = 0; k < 4; k++) {
        unsigned long long v = 0;
        for (int s = 0; s < hbk::kStripes; s++) v += h[4 * s + k];
        sum[k] = v;
    }
}
// A finished pass enters the statistics and the loop moves on: counters.step(); changed_nodes = new_changed_nodes; t += 1
// (harmonic.rs:273-275).  sum: its summed counters; ps: what the caller knows (mode, A_t, times)
void book_pass(hb_ctx *c, const unsigned long long *sum, hb_pass_stats ps)
{
    ps.pass = c->t;
    ps.changed = sum[0];
    ps.touched = sum[2];
    c->pstats.push_back(ps);
    c->last_changed = sum[0];
    c->last_active = sum[3];
    c->has_changes = sum[0] != 0;
    c->cur ^= 1;
    c->t += 1;
}

int step_finish(hb_ctx *c, int *has_changes)
{
    if (!c->pending_local) return fail(c, HB_ERR_INVALID, "hb_step_finish without hb_step_local");
    const Plan &p = c->plan;
    hipEvent_t *E = nullptr;
    {
        const int rc_ev = pass_events(c, &E);
        if (rc_ev) return rc_ev;
    }
    bool counters_read = false; // the pass' host round trip has already happened (destination partition + changed-only)
    if (unfused(c)) {
        hbk::PassParams pp = make_params(c);
        pp.row_lo = 0;
        pp.row_hi = p.n_pad;
        if (linked(c) && edge_changed_only(c)) {
            // union of the ranks' locally-changed rows (all-gather of the bitmaps + OR), then an all-reduce(max) over those
            // rows only, packed in the same order everywhere: -20 % of the bytes in the dense passes of the R-MAT configs,
            // ~ -100 % in the tail
            const uint64_t words = p.n_pad / 32;
            const int world = std::max(c->opt.world_size, 1);
            HB_COLL(coll_all_gather(c, c->d_lbits, c->d_lbits_all, words, ncclUint32, c->stream));
            HB_HIP(hipMemcpyAsync(c->d_ubits, c->d_lbits_all, words * 4, hipMemcpyDeviceToDevice, c->stream));
            for (int k = 1; k < world && words; k++) {
                hipLaunchKernelGGL(hbk::or_words_kernel, dim3((unsigned)std::min<uint64_t>((words + 255) / 256, 2048)), dim3(256), 0, c->stream, c->d_ubits,
                                   (const uint32_t *)(c->d_lbits_all + (uint64_t)k * words), words);
            }
            HB_HIP(hipGetLastError());
            int rc = edge_co_pack(c);
            if (rc) return rc;
            if (c->co_rows && packed_wire(c)) {
                if ((rc = packed_all_reduce_max(c, c->d_pack, c->co_rows, wire6_co_slice(c), c->stream))) return rc;
            } else if (c->co_rows) {
                HB_COLL(coll_all_reduce(c, c->d_pack, c->co_rows * 64, ncclUint8, ncclMax, c->stream));
            }
            if ((rc = edge_co_unpack(c))) return rc;
            c->wire_bytes += (uint64_t)(world - 1) * words * 4 +
                             (packed_wire(c) ? wire6_co_bytes(c) : (world > 1 ? 2 * (uint64_t)(world - 1) * c->co_rows * 64 / (uint64_t)world : 0));
        } else if (linked(c) && c->ov_ranges) {
            // pipelined: all-reduce of range k on comm_stream as soon as it is merged; its epilogue on the main stream as
            // soon as it is reduced (the epilogue launches below wait for ov_reduced[k])
            for (int k = 0; k < c->ov_ranges; k++) {
                const uint64_t lo = c->ov_lo[k], hi = c->ov_lo[k + 1];
                HB_HIP(hipStreamWaitEvent(c->comm_stream, c->ov_merged[k], 0));
                if (hi > lo) HB_COLL(coll_all_reduce(c, pp.wr + lo * 4, (hi - lo) * 64, ncclUint8, ncclMax, c->comm_stream));
                HB_HIP(hipEventRecord(c->ov_reduced[k], c->comm_stream));
            }
            c->wire_bytes += c->opt.world_size > 1 ? 2 * (uint64_t)(c->opt.world_size - 1) * p.n_pad * 64 / (uint64_t)c->opt.world_size : 0;
        } else if (linked(c) && packed_wire(c)) {
            const int rc = packed_all_reduce_max(c, pp.wr, p.n_pad, wire6_slice(c), c->stream);
            if (rc) return rc;
            c->wire_bytes += wire6_all_reduce_bytes(c, wire6_slice(c));
        } else if (linked(c)) {
            HB_COLL(coll_all_reduce(c, pp.wr, p.n_pad * 64, ncclUint8, ncclMax, c->stream));
            c->wire_bytes += c->opt.world_size > 1 ? 2 * (uint64_t)(c->opt.world_size - 1) * p.n_pad * 64 / (uint64_t)c->opt.world_size : 0;
        }
        if (edge_changed_only(c) && c->ubits_valid) pp.ubits = c->d_ubits; // the epilogue visits the exchanged rows only
        c->ubits_valid = false;
        const int ranges = (linked(c) && c->ov_ranges && !edge_changed_only(c)) ? c->ov_ranges : 1;
        for (int k = 0; k < ranges; k++) {
            if (ranges > 1) {
                pp.row_lo = c->ov_lo[k];
                pp.row_hi = c->ov_lo[k + 1];
                HB_HIP(hipStreamWaitEvent(c->stream, c->ov_reduced[k], 0));
            }
            if (k == ranges - 1) HB_HIP(hipEventRecord(E[kEvCollective], c->stream)); // (collective time: up to the last range reduced)
            const uint64_t ntiles = (pp.row_hi - pp.row_lo) / 64;
            if (ntiles) {
                const uint32_t bpc = (c->opt.tune[0] & 0xFFu) ? (c->opt.tune[0] & 0xFFu) : 8;
                hipLaunchKernelGGL(hbk::epilogue_kernel, dim3(grid_blocks(c, ntiles, bpc)), dim3(256), 0, c->stream, pp);
            }
        }
        c->ov_ranges = 0;
        HB_HIP(hipGetLastError());
    }
    if (dest_mode(c) && linked(c)) {
        // every rank produced the final counters, changed bits and changed count of ITS rows (fused
        // kernel): all-gather the slices in place; sum the counts
        hbk::PassParams pp = make_params(c);
        const uint64_t S = c->slice_rows, r = (uint64_t)c->opt.rank;
        if (changed_only(c)) {
            // bits and counts first, then only the counters that changed: one broadcast per rank of its packed run.
            // [r5] the runs' lengths are host-side arguments of those broadcasts; they used to be read back from the prefix sums
            // (a second host round trip per pass).  Every rank now adds its changed-row count to a world-sized vector that is
            // summed next to the pass counters, and BOTH come to the host in the one round trip a pass has anyway - which
            // therefore sits here, before the broadcasts; the rest of the pass is queued behind it and left in flight.
            const int world = std::max(c->opt.world_size, 1);
            if (!c->d_rank_cnt) {
                int rc0 = dev_alloc(c, &c->d_rank_cnt, (size_t)world + 1);
                if (rc0) return rc0;
            }
            hipLaunchKernelGGL(hbk::rank_count_kernel, dim3(1), dim3(64), 0, c->stream, (const unsigned long long *)pp.counters, c->d_rank_cnt, world, c->opt.rank);
            HB_HIP(hipGetLastError());
            HB_COLL(coll_group_start(c));
            HB_COLL(coll_all_gather(c, pp.bits_wr + r * (S / 32), pp.bits_wr, S / 32, ncclUint32, c->stream));
            HB_COLL(coll_all_reduce(c, pp.counters, hbk::kCounterWords, ncclUint64, ncclSum, c->stream));
            HB_COLL(coll_all_reduce(c, c->d_rank_cnt, (uint64_t)world, ncclUint64, ncclSum, c->stream));
            HB_COLL(coll_group_end(c));
            HB_HIP(hipMemcpyAsync(c->h_counters, pp.counters, hbk::kCounterWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
            HB_HIP(hipMemcpyAsync(c->h_rank_cnt, c->d_rank_cnt, (size_t)world * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
            HB_HIP(hipStreamSynchronize(c->stream));
            counters_read = true;
            std::vector<uint64_t> off((size_t)world + 1, 0);
            for (int k = 0; k < world; k++) off[(size_t)k + 1] = off[(size_t)k] + c->h_rank_cnt[k];
            int rc = exchange_pack(c, off.data());
            if (rc) return rc;
            HB_COLL(coll_group_start(c));
            for (int k = 0; k < world; k++) {
                const uint64_t cnt = c->ex_off[k + 1] - c->ex_off[k];
                if (cnt) HB_COLL(coll_broadcast(c, (uint8_t *)c->d_pack + c->ex_off[k] * packed_row_bytes(c), cnt * packed_row_bytes(c), ncclUint8, k, c->stream));
            }
            HB_COLL(coll_group_end(c));
            if ((rc = exchange_unpack(c))) return rc;
        } else if (packed_wire(c)) {
            int rc = wire6_pack_own_slice(c);
            if (rc) return rc;
            HB_COLL(coll_group_start(c));
            HB_COLL(coll_all_gather(c, c->d_w6[0] + r * S * 12, c->d_w6[0], S * 48, ncclUint8, c->stream));
            HB_COLL(coll_all_gather(c, pp.bits_wr + r * (S / 32), pp.bits_wr, S / 32, ncclUint32, c->stream));
            HB_COLL(coll_all_reduce(c, pp.counters, hbk::kCounterWords, ncclUint64, ncclSum, c->stream));
            HB_COLL(coll_group_end(c));
            if ((rc = wire6_unpack_foreign_slices(c))) return rc;
        } else {
            HB_COLL(coll_group_start(c));
            HB_COLL(coll_all_gather(c, pp.wr + r * S * 4, pp.wr, S * 64, ncclUint8, c->stream));
            HB_COLL(coll_all_gather(c, pp.bits_wr + r * (S / 32), pp.bits_wr, S / 32, ncclUint32, c->stream));
            HB_COLL(coll_all_reduce(c, pp.counters, hbk::kCounterWords, ncclUint64, ncclSum, c->stream));
            HB_COLL(coll_group_end(c));
            c->wire_bytes += (p.n_pad - std::min<uint64_t>(S, p.n_pad)) * 64 + (p.n_pad - std::min<uint64_t>(S, p.n_pad)) / 8;
        }
        HB_HIP(hipEventRecord(E[kEvCollective], c->stream));
    }
    PassEvent ev_end = (dest_mode(c) && linked(c)) ? kEvCollective : kEvMerge;
    if (unfused(c)) {
        HB_HIP(hipEventRecord(E[kEvEpilogue], c->stream));
        ev_end = kEvEpilogue;
    }
    if (!counters_read) {
        HB_HIP(hipMemcpyAsync(c->h_counters, c->d_counters + (size_t)hbk::kCounterWords * c->t,
                              hbk::kCounterWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HB_HIP(hipStreamSynchronize(c->stream));
    }
    sum_stripes(c->h_counters, c->h_counters);
    if (c->cur_mode == kModeDense && skips_saturated_rows(c)) c->sat_out_sum += c->h_counters[1]; // (the rows this pass found saturated: early_exit_rule)
    hb_pass_stats ps{};
    ps.active_edges = (c->opt.flags & HB_FLAG_PASS_STATS) ? c->h_counters[1] : c->last_active; // A_t
    ps.mode = c->cur_mode;
    if (counters_read) { // the end of this pass is still in flight: its events are read by resolve_pass_times
        c->pending_times.push_back(c->pstats.size());
    } else {
        const int rc = read_pass_times(c, E, ev_end, &ps);
        if (rc) return rc;
        if (linked(c) && (unfused(c) || dest_mode(c))) HB_HIP(hipEventElapsedTime(&ps.ms_collective, E[kEvMerge], E[kEvCollective]));
    }
    if (ref_tail(c)) {
        const int rc = reference_changed_state(c, (const uint32_t *)c->d_bits[c->cur ^ 1], c->h_counters[0]);
        if (rc) return rc;
    }
    book_pass(c, c->h_counters, ps);
    c->pending_local = false;
    if (has_changes) *has_changes = c->has_changes ? 1 : 0;
    return results_stage_policy(c, c->last_changed);
}

// ---- the far tail as one workgroup (hb_tail.hip.h) [r5] -------------------------------------------------------------------------
// EXPERIMENTS build only [r6]: built as round 4's design asked, exact, and measured no faster than the launches it replaces (DESIGN.md
// §3) - the product library carries neither the kernel nor its lists.
#ifndef HB_EXPERIMENTS
bool tail_kernel_ready(const hb_ctx *) { return false; }
int tail_kernel_run(hb_ctx *, uint32_t, uint32_t *ran)
{
    *ran = 0;
    return HB_OK;
}
#else
bool tail_kernel_ready(const hb_ctx *c)
{
    // (last_active = A_{t+1} = the out-degree sum of the changed nodes = the entries of their reader lists: every edge sits in one work row)
    return c->run_open && c->has_changes && c->t > 0 && c->last_changed <= hbk::kTailSeeds && c->last_active <= hbk::kTailReaders &&
           c->sparse_ok && !c->tl_declined &&
           c->d_tl_count && !multi_rank(c) && !linked(c) && !unfused(c) && !ref_tail(c) && !(c->opt.flags & (HB_FLAG_PASS_STATS | HB_FLAG_NO_FRONTIER)) &&
           xbit(c, HB_X_TAIL_KERNEL | HB_X_TAIL_KERNEL_ANY) && // OFF by default (measured: no faster than the launches it replaces, DESIGN.md §3)
           c->plan.level_begin.size() >= 1 && c->plan.level_begin.size() - 1 <= (size_t)hbk::kTailLevels && c->t < c->max_passes &&
           (c->cur_mode == 2 || c->cur_mode == 4 || xbit(c, HB_X_TAIL_KERNEL_ANY)); // after a sweep / tail-kernel pass
}

// up to `budget` passes in one launch; *ran = passes completed (0: the kernel declined - the next pass does not fit its lists)
int tail_kernel_run(hb_ctx *c, uint32_t budget, uint32_t *ran)
{
    *ran = 0;
    const Plan &p = c->plan;
    hbk::TailParams P{};
    P.row_ptr = c->d_row_ptr;
    P.src = c->d_src;
    P.regs[0] = c->d_regs[0];
    P.regs[1] = c->d_regs[1];
    P.part = c->d_part;
    P.bits[0] = c->d_bits[0];
    P.bits[1] = c->d_bits[1];
    P.kdirty = c->d_kdirty;
    P.ksum = c->d_ksum;
    P.kerr = c->d_kerr;
    P.size = c->d_size;
    P.outdeg = c->d_outdeg;
    P.counters = c->d_counters;
    P.raw = c->d_raw;
    P.bias = c->d_bias;
    P.lc = c->d_lc;
    P.out_ptr = c->d_out_ptr;
    P.out_rows = c->d_out_rows;
    P.touch = c->d_touch;
    P.n_pad = p.n_pad;
    P.rows_total = p.n_pad + p.nv;
    P.levels = (int)p.level_begin.size() - 1;
    if (P.levels < 0) P.levels = 0;
    for (int l = 0; l <= P.levels; l++) P.level_begin[l] = p.level_begin[(size_t)l];
    for (int k = 0; k < 2; k++) {
        P.changed[k] = c->d_tl_changed[k];
        P.vchanged[k] = c->d_tl_vchanged[k];
        P.dirty[k] = c->d_tl_dirty[k];
    }
    P.work = c->d_tl_work;
    P.count = c->d_tl_count;
    P.t0 = c->t;
    P.cur0 = c->cur;
    P.max_passes = (uint32_t)std::min<uint64_t>(budget, c->max_passes - c->t);
    if (!c->tl_valid) { // the five lists from the bitmaps as they are (one grid-wide scan per entry)
        HB_HIP(hipMemsetAsync(c->d_tl_count, 0, hbk::kTcWords * sizeof(uint32_t), c->stream));
        const uint64_t words = (P.rows_total + 31) / 32;
        hipLaunchKernelGGL(hbk::tail_collect_kernel, dim3(grid_blocks(c, (words + 255) / 256, 4, 1)), dim3(256), 0, c->stream, P);
        HB_HIP(hipGetLastError());
    }
    HB_HIP(hipEventRecord(c->tl_ev[kEvStart], c->stream));
    hipLaunchKernelGGL(hbk::tail_loop_kernel, dim3(1), dim3(1024), 0, c->stream, P);
    HB_HIP(hipGetLastError());
    HB_HIP(hipEventRecord(c->tl_ev[kEvEnd], c->stream));
    HB_HIP(hipMemcpyAsync(c->h_tl_count, c->d_tl_count, hbk::kTcWords * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HB_HIP(hipStreamSynchronize(c->stream));
    const uint32_t done = c->h_tl_count[hbk::kTcPasses], reason = c->h_tl_count[hbk::kTcReason];
    c->tl_valid = true; // the lists follow the bitmaps from now on (until another kernel runs a pass)
    if (!done) {
        c->tl_declined = true;
        return HB_OK;
    }
    std::vector<unsigned long long> cnt((size_t)done * hbk::kCounterWords);
    HB_HIP(hipMemcpyAsync(cnt.data(), c->d_counters + (size_t)hbk::kCounterWords * c->t, cnt.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HB_HIP(hipStreamSynchronize(c->stream));
    float ms = 0.f;
    HB_HIP(hipEventElapsedTime(&ms, c->tl_ev[kEvStart], c->tl_ev[kEvEnd]));
    for (uint32_t k = 0; k < done; k++) {
        hb_pass_stats ps{};
        ps.active_edges = c->last_active;
        ps.mode = 4; // one workgroup, work lists (hb_tail.hip.h)
        ps.ms_gpu = ms / (float)done;
        ps.ms_main = ps.ms_gpu;
        book_pass(c, &cnt[(size_t)k * hbk::kCounterWords], ps); // (one workgroup: stripe 0 holds the whole counters)
        c->cur_mode = 4;
        const int rc = results_stage_policy(c, c->last_changed);
        if (rc) return rc;
    }
    c->tail_kernel_passes += done;
    if (reason == 2) c->tl_declined = true; // the next pass does not fit: an ordinary pass first
    *ran = done;
    return HB_OK;
}
#endif // HB_EXPERIMENTS

// ---- hb_run's tail pipeline [r5] ---------------------------------------------------------------------------------------------
// In the convergence tail a pass is a handful of 5-10 us launches, and the host round trip that ends it (counters to the host,
// hipStreamSynchronize, the next pass' launches) left the GPU idle about as long again.  Once a sweep pass has changed <= 4096
// nodes, hb_run keeps ONE pass queued ahead: pass q + 1 goes into the stream - guarded on the device by pass q's changed count, see
// SweepParams::guard - before pass q's counters are read.  The loop still ends on the first pass that changes nothing
// (harmonic.rs:237-240): the pass queued behind it finds its guard closed and does nothing at all.  Mode, launch shapes and the
// `last_changed <= 4096` kernel choice of the queued pass come from pass q - 1; every choice gives the same bits (SURVEY App. C-1).
bool tail_pipeline_ready(const hb_ctx *c)
{
    return c->run_open && c->has_changes && c->t > 0 && c->cur_mode == 2 && c->last_changed <= 4096 && c->sparse_ok && !multi_rank(c) &&
           !linked(c) && !unfused(c) && !ref_tail(c) && !(c->opt.flags & HB_FLAG_PASS_STATS) && !xbit(c, HB_X_NO_TAIL_PIPELINE) &&
           c->t + 2 < c->max_passes;
}

// queue pass c->t (all its launches), then its counters' way to the host; nothing is waited for
int tail_queue(hb_ctx *c, bool guarded_by_previous)
{
    c->pipelined = true;
    c->spec_guard = guarded_by_previous ? c->d_counters + (size_t)hbk::kCounterWords * (c->t - 1) : nullptr;
    const int rc = step_local(c);
    c->spec_guard = nullptr;
    c->pipelined = false;
    if (rc) return rc;
    c->pending_local = false;
    const int slot = (int)(c->t & 1);
    HB_HIP(hipMemcpyAsync(c->h_slot + (size_t)slot * hbk::kCounterWords, c->d_counters + (size_t)hbk::kCounterWords * c->t,
                          hbk::kCounterWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HB_HIP(hipEventRecord(c->slot_done[slot], c->stream));
    return HB_OK;
}

// wait for pass c->t (queued by tail_queue), book it like step_finish does, advance the loop state
int tail_complete(hb_ctx *c)
{
    const int slot = (int)(c->t & 1);
    HB_HIP(hipEventSynchronize(c->slot_done[slot]));
    unsigned long long sum[4];
    sum_stripes(c->h_slot + (size_t)slot * hbk::kCounterWords, sum);
    hb_pass_stats ps{};
    ps.active_edges = c->last_active;
    ps.mode = c->cur_mode;
    const int rc = read_pass_times(c, c->ev_ring[c->t & 3].e, kEvMerge, &ps);
    if (rc) return rc;
    book_pass(c, sum, ps);
    return HB_OK;
}

int tail_pipeline(hb_ctx *c, int *has_changes)
{
    int rc = tail_queue(c, false); // pass q = c->t: the previous pass is known to have changed something
    if (rc) return rc;
    for (;;) {
        // pass q + 1 behind it, as if pass q had changed something (if it has not, the device guard keeps it from running)
        const bool ahead = c->t + 2 < c->max_passes;
        if (ahead) {
            c->t += 1;
            c->cur ^= 1;
            rc = tail_queue(c, true);
            c->t -= 1;
            c->cur ^= 1;
            if (rc) return rc;
        }
        if ((rc = tail_complete(c))) return rc; // pass q is booked; c->t = q + 1 now
        if (ahead && c->has_changes) c->pipelined_passes++; // (the pass behind it really runs)
        if ((rc = results_stage_policy(c, c->last_changed))) return rc;
        if (!c->has_changes) break;             // the loop's last pass; the pass queued behind it did nothing
        if (!ahead) {                           // (max_passes is near: back to the one-pass-at-a-time loop, which reports the limit)
            if (has_changes) *has_changes = 1;
            return HB_OK;
        }
        if (c->last_changed > 4096 || c->cur_mode != 2 || tail_kernel_ready(c)) {
            // the changed set grew again - or shrank enough for the single-workgroup kernel to take the rest of the tail: the pass
            // already queued is a real one - take it, then leave the pipeline
            if ((rc = tail_complete(c))) return rc;
            if ((rc = results_stage_policy(c, c->last_changed))) return rc;
            break;
        }
    }
    if (has_changes) *has_changes = c->has_changes ? 1 : 0;
    return HB_OK;
}

// ---- first dispatches at load time (declared in hb_api_load.inc) ---------------------------------------------------------------------
int warm_kernels(hb_ctx *c)
{
    if (!c->plan.n_pad || (c->opt.flags & HB_FLAG_PASS_STATS)) return HB_OK;
    hbk::PassParams pp = make_params(c);
    pp.row_lo = pp.row_hi = 0; // no tile anywhere below
    pp.xcd_map = 0;
    pp.n_pad = 0;              // (the sweep kernels size their bitmap scans by it; make_params' other fields stay valid pointers)
    pp.counters = c->d_counters + (size_t)c->max_passes * hbk::kCounterWords; // the spare slot (every kernel adds zero to it)
    hipStream_t s = c->stream;
    const dim3 one(1), blk(256);
    // the instances launch_pass will pick for this context's dense and bitmap passes (no HB_FLAG_PASS_STATS here), hub chunks and node rows
    const bool fused = !unfused(c), epi4 = !xbit(c, HB_X_TILE_EPILOGUE), compact = !xbit(c, HB_X_BITMAP_SLOTWISE);
    const int hub_unroll = pass_unroll(c, false), node_unroll = pass_unroll(c, true);
    auto warm = [&](PassKernel k) { hipLaunchKernelGGL(k, one, blk, 0, s, pp); };
    warm(dense_kernel(false, false, false, hub_unroll, false, false, false));
    warm(dense_kernel(true, fused, false, node_unroll, false, epi4, false));
    if (c->d_sat && fused && !(c->opt.flags & HB_FLAG_NO_EARLY_EXIT)) { // the EARLY instances of a context that may leave rows early
        warm(dense_kernel(false, false, false, hub_unroll, false, false, true));
        warm(dense_kernel(true, true, false, node_unroll, false, epi4, true));
    }
    if (fused && pass0_streams_initial_registers(c)) { // pass 0 as the INIT launch
        warm(dense_kernel(false, false, false, hub_unroll, true, false, false));
        warm(hbk::init_level1_kernel);
        warm(dense_kernel(true, true, false, node_unroll, true, epi4, false));
    }
    warm(bitmap_kernel(false, false, false, compact));
    warm(bitmap_kernel(true, fused, false, compact));
    if (!fused) warm(hbk::epilogue_kernel);
    if (c->d_sat) hipLaunchKernelGGL(hbk::sat_down_kernel, one, blk, 0, s, (const uint64_t *)c->d_row_ptr, (const uint32_t *)c->d_src, 0ull, 0ull, 0ull, c->d_sat);
    if (c->sparse_ok) {
        const hbk::SweepParams sp = make_sweep_params(c, pp, 0, nullptr); // (the counters: zeroed here, and again by every hb_begin)
        HB_HIP(hipMemsetAsync(c->d_sparse_counts, 0, 64 * sizeof(unsigned int), s));
        hipLaunchKernelGGL(hbk::sweep_collect_kernel, one, blk, 0, s, sp);
        hipLaunchKernelGGL(hbk::sweep_expand_kernel, one, blk, 0, s, sp);
        hipLaunchKernelGGL(hbk::sweep_expand_heavy_kernel, one, blk, 0, s, sp);
        hipLaunchKernelGGL(hbk::sweep_seed_small_kernel, one, blk, 0, s, sp);
        const bool by_rounds = xbit(c, HB_X_SWEEP_ROUNDS);
        hipLaunchKernelGGL(sweep_rows_kernel_for(false, by_rounds), one, blk, 0, s, sp);
        hipLaunchKernelGGL(sweep_rows_kernel_for(true, by_rounds), one, blk, 0, s, sp);
    }
    if (c->rs.on) {
        hipLaunchKernelGGL(hbk::results_sync_kernel, one, blk, 0, s, (const double *)c->d_ksum, c->rs.d_sent, (const uint32_t *)c->d_cid_of, (uint64_t)0, 1.0, 0,
                           c->d_out, (uint32_t *)nullptr, (double *)nullptr, 0ull, c->rs.d_count, pp.counters);
    }
    hipLaunchKernelGGL(hbk::finish_kernel, one, blk, 0, s, (const double *)c->d_ksum, (const uint32_t *)c->d_dev_of, (uint64_t)0, 1.0, c->d_out, pp.counters);
    HB_HIP(hipGetLastError());
    return HB_OK;
}
