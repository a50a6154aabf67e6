// hb_ampc_finish.inc - part of hb_ampc.hip: the finish of a job - values, ranks, top nodes, store
namespace {
// a temporary of one finish call (the caching allocator's: it goes back to it when its holder is reset or the call returns); never below 256 bytes
template <class T>
hipError_t alloc_temp(DevPtr<T> &p, uint64_t count)
{
    return p.alloc(std::max<size_t>((size_t)count, (256 + sizeof(T) - 1) / sizeof(T)));
}
// the entries of a centrality table in ascending-NodeID order, on the device: ids, quotients, the rank order and (if asked for) the ranks
struct Finished {
    DevPtr<hb_u128> d_ids;
    DevPtr<double> d_vals;
    DevPtr<uint64_t> d_order; // d_order[i] = the entry at position i of (value descending under total_cmp, NodeID ascending)
    DevPtr<uint64_t> d_rank;
};

int finish_refusal(hbu_table *t)
{
    if (!t) return fail(t, HB_ERR_INVALID, "NULL table");
    if (t->kind != HBU_KIND_KAHAN && t->kind != HBU_KIND_F64) return fail(t, HB_ERR_INVALID, "a centrality table is a KahanSum or an f64 table");
    if (t->broken) return fail(t, HB_ERR_INVALID, kBrokenMsg);
    return HB_OK;
}
int sort_error(hbu_table *t, const std::string &e)
{
    (void)hipGetLastError();
    return fail(t, e.find("memory") != std::string::npos ? HB_ERR_NOMEM : HB_ERR_HIP, e);
}

// keys by entry number -> one 128-bit sort carrying the entry number -> quotient and sort key of every entry in that order -> a stable
// 64-bit sort of the sort keys -> the scatter of the ranks.  The table is only read.  n = t->committed > 0.
// The reset()s in the middle bound the peak device memory of the finish: each sits in front of the next allocation.
int finish_on_device(hbu_table *t, double divisor, bool want_ranks, Finished *f)
{
    const uint64_t n = t->committed;
    const hipStream_t stream = t->stream;
    DevPtr<hb_u128> d_raw;
    DevPtr<uint32_t> d_entry;
    DevPtr<uint64_t> d_key;
    HBU_HIP(alloc_temp(d_raw, n));
    HBU_HIP(alloc_temp(f->d_ids, n));
    HBU_HIP(alloc_temp(d_entry, n));
    hipLaunchKernelGGL(hbr::set_export_kernel, dim3(grid_for(t->slots)), dim3(256), 0, stream, (const u128 *)t->d_keys.get(), (const uint32_t *)t->d_pids.get(), t->slots,
                       (uint32_t)n, d_raw.get());
    HBU_HIP(hipGetLastError());
    std::string e = hb::gpu_sort_ids_device((void *)stream, d_raw.get(), n, f->d_ids.get(), d_entry.get());
    if (!e.empty()) return sort_error(t, e);
    d_raw.reset();
    HBU_HIP(alloc_temp(f->d_vals, n));
    HBU_HIP(alloc_temp(d_key, n));
    if (t->kind == HBU_KIND_KAHAN)
        hipLaunchKernelGGL(hbn::finish_values_kernel<2>, dim3(grid_for(n)), dim3(256), 0, stream, (const double *)t->d_table.get(), (const uint32_t *)d_entry.get(), n, divisor,
                           f->d_vals.get(), d_key.get());
    else
        hipLaunchKernelGGL(hbn::finish_values_kernel<1>, dim3(grid_for(n)), dim3(256), 0, stream, (const double *)t->d_table.get(), (const uint32_t *)d_entry.get(), n, divisor,
                           f->d_vals.get(), d_key.get());
    HBU_HIP(hipGetLastError());
    HBU_HIP(alloc_temp(f->d_order, n));
    if (want_ranks) HBU_HIP(alloc_temp(f->d_rank, n));
    e = hb::gpu_rank_keys_device((void *)stream, d_key.get(), n, f->d_order.get(), f->d_rank.get());
    if (!e.empty()) return sort_error(t, e);
    return HB_OK; // (d_key and d_entry go here)
}
} // namespace

extern "C" {

int hbu_finish_centralities(hbu_table *centrality, double divisor, hb_u128 *ids_out, double *vals_out, uint64_t *ranks_out, uint64_t capacity, uint64_t *written)
{
    hbu_table *t = centrality;
    return guarded(t, [&]() -> int {
        if (written) *written = 0;
        int rc = finish_refusal(t);
        if (rc) return rc;
        const uint64_t n = t->committed;
        const bool any = ids_out || vals_out || ranks_out;
        if (any && capacity < n) return fail(t, HB_ERR_INVALID, "capacity below the number of keys");
        if (written) *written = n;
        if (!n || !any) return HB_OK;
        HBU_HIP(hipSetDevice(t->device));
        Finished f;
        if ((rc = finish_on_device(t, divisor, ranks_out != nullptr, &f))) {
            if (written) *written = 0;
            return rc;
        }
        if (ids_out) HBU_HIP(hipMemcpyAsync(ids_out, f.d_ids.get(), n * sizeof(hb_u128), hipMemcpyDeviceToHost, t->stream));
        if (vals_out) HBU_HIP(hipMemcpyAsync(vals_out, f.d_vals.get(), n * sizeof(double), hipMemcpyDeviceToHost, t->stream));
        if (ranks_out) HBU_HIP(hipMemcpyAsync(ranks_out, f.d_rank.get(), n * sizeof(uint64_t), hipMemcpyDeviceToHost, t->stream));
        HBU_HIP(hipStreamSynchronize(t->stream));
        return HB_OK;
    });
}

int hbu_top_centralities(hbu_table *centrality, double divisor, uint64_t k, hb_u128 *ids_out, double *vals_out, uint64_t *written)
{
    hbu_table *t = centrality;
    return guarded(t, [&]() -> int {
        if (written) *written = 0;
        int rc = finish_refusal(t);
        if (rc) return rc;
        const uint64_t top = std::min<uint64_t>(k, t->committed);
        if (written) *written = top;
        if (!top || (!ids_out && !vals_out)) return HB_OK;
        HBU_HIP(hipSetDevice(t->device));
        Finished f;
        if ((rc = finish_on_device(t, divisor, false, &f))) {
            if (written) *written = 0;
            return rc;
        }
        DevPtr<hb_u128> d_top_ids;
        DevPtr<double> d_top_vals;
        if (ids_out) HBU_HIP(alloc_temp(d_top_ids, top));
        if (vals_out) HBU_HIP(alloc_temp(d_top_vals, top));
        hipLaunchKernelGGL(hbn::top_gather_kernel, dim3(grid_for(top)), dim3(256), 0, t->stream, (const uint64_t *)f.d_order.get(), top, (const hb_u128 *)f.d_ids.get(),
                           (const double *)f.d_vals.get(), d_top_ids.get(), d_top_vals.get());
        HBU_HIP(hipGetLastError());
        if (ids_out) HBU_HIP(hipMemcpyAsync(ids_out, d_top_ids.get(), top * sizeof(hb_u128), hipMemcpyDeviceToHost, t->stream));
        if (vals_out) HBU_HIP(hipMemcpyAsync(vals_out, d_top_vals.get(), top * sizeof(double), hipMemcpyDeviceToHost, t->stream));
        HBU_HIP(hipStreamSynchronize(t->stream));
        return HB_OK;
    });
}

int hbu_store_centralities(hbu_table *centrality, double divisor, const char *output, char *err, uint64_t err_len)
{
    hbu_table *t = centrality;
    if (err && err_len) err[0] = 0;
    const int rc = guarded(t, [&]() -> int {
        int rc2 = finish_refusal(t);
        if (rc2) return rc2;
        if (!output || !*output) return fail(t, HB_ERR_INVALID, "hbu_store_centralities: output is empty");
        const uint64_t n = t->committed;
        // what crosses the link: the values, the ranks and the key order of the two databases - the ids stay where they are
        hb::RawVec<double> vals(n);
        hb::RawVec<uint64_t> ranks(n);
        hb::StoreKeyVec sorted(n);
        if (n) {
            HBU_HIP(hipSetDevice(t->device));
            Finished f;
            if ((rc2 = finish_on_device(t, divisor, true, &f))) return rc2;
            HBU_HIP(hipMemcpyAsync(vals.data(), f.d_vals.get(), n * sizeof(double), hipMemcpyDeviceToHost, t->stream));
            HBU_HIP(hipMemcpyAsync(ranks.data(), f.d_rank.get(), n * sizeof(uint64_t), hipMemcpyDeviceToHost, t->stream));
            HBU_HIP(hipStreamSynchronize(t->stream));
            f.d_vals.reset();
            f.d_rank.reset();
            f.d_order.reset();
            const std::string e = hb::gpu_store_keys_device((void *)t->stream.get(), f.d_ids.get(), n, sorted.data());
            if (!e.empty()) return sort_error(t, "hbu_store_centralities: " + e);
        }
        char msg[512] = {0};
        const int rc3 = hb::store_harmonic_presorted(output, &sorted, vals.data(), ranks.data(), msg, sizeof(msg));
        if (rc3) return fail(t, rc3, msg);
        return HB_OK;
    });
    if (rc && err && err_len) std::snprintf(err, (size_t)err_len, "%s", hbu_last_error(t));
    return rc;
}

} // extern "C"
