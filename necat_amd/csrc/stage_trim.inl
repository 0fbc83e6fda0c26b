// stage_trim.inl - the read trimming stage on records (oc2pm4 + oc2lcr): records grouped by read, one clip range per read.
// One of the stage files of libnecat_hip.so's single translation unit (see stage_pcan.inl).  Kernels: trim_kernels.h.

// ------------------------------------------------------------------------------------------ records by read (oc2pm4)

// scratch[SC_TRIM_OFF]: read_off[nids + 1], the count of reads handed back, the clip ranges[nids]
static size_t trim_off_bytes(int nids) { return (size_t)(nids + 2) * 8 + (size_t)nids * sizeof(necat_clip_range); }

int necat_trim_partition(necat_ctx* ctx, const necat_m4* recs, uint64_t n, int num_reads, double min_ident_perc,
                         necat_m4** grouped, uint64_t** read_off, uint64_t* n_grouped)
{
    KnobScope knob_scope_(ctx);
    if (!ctx || (n && !recs) || num_reads < 0 || num_reads > (1 << 30) || n > (1ULL << 40)) return NECAT_ERR_ARG;
    if (grouped) *grouped = nullptr;
    if (read_off) *read_off = nullptr;
    if (n_grouped) *n_grouped = 0;
    ctx->trim_nids = 0; ctx->trim_total = 0;
    const int nids = num_reads + 2;                      // ids 0 .. num_reads + 1: what the reference's calloc(num_reads + 2) holds
    NECAT_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    int rc;
    if ((rc = buf_ensure(ctx, ctx->scratch[SC_TRIM_IN], (size_t)n * sizeof(necat_m4) + (size_t)(nids + 1) * 8 + 256))) return rc;
    if ((rc = buf_ensure(ctx, ctx->scratch[SC_TRIM_OFF], trim_off_bytes(nids)))) return rc;
    necat_m4* d_in = (necat_m4*)ctx->scratch[SC_TRIM_IN].p;
    unsigned long long* d_cur = (unsigned long long*)((char*)d_in + (size_t)n * sizeof(necat_m4));      // 96 n: 8-byte aligned
    unsigned long long* d_off = (unsigned long long*)ctx->scratch[SC_TRIM_OFF].p;
    if (n) NECAT_HIP(ctx, hipMemcpyAsync(d_in, recs, (size_t)n * sizeof(necat_m4), hipMemcpyHostToDevice, s));
    NECAT_HIP(ctx, hipMemsetAsync(d_off, 0, (size_t)(nids + 1) * 8, s));
    const unsigned grid = (unsigned)((n + 255) / 256);
    if (n) {
        hipLaunchKernelGGL(k_trim_part<0>, dim3(grid), dim3(256), 0, s, (const necat_m4*)d_in, n, nids, min_ident_perc, d_off, (necat_m4*)nullptr);
        NECAT_CHECK_LAUNCH(ctx, "k_trim_part<count>");
    }
    hipLaunchKernelGGL(k_trim_scan, dim3(1), dim3(1024), 0, s, d_off, nids);
    NECAT_CHECK_LAUNCH(ctx, "k_trim_scan");
    unsigned long long total = 0;
    NECAT_HIP(ctx, hipMemcpyAsync(&total, d_off + nids, 8, hipMemcpyDeviceToHost, s));
    NECAT_HIP(ctx, hipStreamSynchronize(s));
    if (total > 2 * n) return set_err(ctx, NECAT_ERR_INTERNAL, "trim partition: %llu records out of %llu", total, (unsigned long long)n);
    if ((rc = buf_ensure(ctx, ctx->scratch[SC_TRIM_RECS], (size_t)total * sizeof(necat_m4) + 256))) return rc;
    necat_m4* d_out = (necat_m4*)ctx->scratch[SC_TRIM_RECS].p;
    if (n) {
        NECAT_HIP(ctx, hipMemcpyAsync(d_cur, d_off, (size_t)nids * 8, hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL(k_trim_part<1>, dim3(grid), dim3(256), 0, s, (const necat_m4*)d_in, n, nids, min_ident_perc, d_cur, d_out);
        NECAT_CHECK_LAUNCH(ctx, "k_trim_part<scatter>");
    }
    if (read_off) {
        uint64_t* off = (uint64_t*)result_alloc((size_t)(nids + 1) * 8);
        if (!off) return set_err(ctx, NECAT_ERR_MEMORY, "host allocation");
        *read_off = off;
        NECAT_HIP(ctx, hipMemcpyAsync(off, d_off, (size_t)(nids + 1) * 8, hipMemcpyDeviceToHost, s));
    }
    if (grouped) {
        necat_m4* g = (necat_m4*)result_alloc((size_t)total * sizeof(necat_m4) + sizeof(necat_m4));
        if (!g) return set_err(ctx, NECAT_ERR_MEMORY, "host allocation");
        *grouped = g;
        if (total) NECAT_HIP(ctx, hipMemcpyAsync(g, d_out, (size_t)total * sizeof(necat_m4), hipMemcpyDeviceToHost, s));
    }
    NECAT_HIP(ctx, hipStreamSynchronize(s));
    if (n_grouped) *n_grouped = total;
    ctx->trim_nids = nids; ctx->trim_total = total;
    return NECAT_OK;
}

// ------------------------------------------------------------------------------------------ one clip range per read (oc2lcr)

int necat_trim_ranges(necat_ctx* ctx, const necat_m4* grouped, const uint64_t* read_off, int num_reads, double min_ident_perc,
                      int min_ovlp_size, int min_cov, int min_size, necat_clip_range* out, uint64_t* n_host)
{
    KnobScope knob_scope_(ctx);
    if (!ctx || !out || num_reads < 0 || num_reads > (1 << 30) || ((grouped == nullptr) != (read_off == nullptr))) return NECAT_ERR_ARG;
    const int nids = num_reads + 2;
    NECAT_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    int rc;
    if (grouped) {
        // the caller's groups: offsets ascending and inside the array, or no kernel runs
        for (int i = 0; i < nids; ++i) if (read_off[i] > read_off[i + 1]) return set_err(ctx, NECAT_ERR_ARG, "read_off[%d] > read_off[%d]", i, i + 1);
        if (read_off[0] != 0 || read_off[nids] > (1ULL << 40)) return set_err(ctx, NECAT_ERR_ARG, "read_off does not start at 0 or ends beyond 2^40 records");
        const uint64_t total = read_off[nids];
        if ((rc = buf_ensure(ctx, ctx->scratch[SC_TRIM_RECS], (size_t)total * sizeof(necat_m4) + 256))) return rc;
        if ((rc = buf_ensure(ctx, ctx->scratch[SC_TRIM_OFF], trim_off_bytes(nids)))) return rc;
        ctx->trim_nids = 0;
        if (total) NECAT_HIP(ctx, hipMemcpyAsync(ctx->scratch[SC_TRIM_RECS].p, grouped, (size_t)total * sizeof(necat_m4), hipMemcpyHostToDevice, s));
        NECAT_HIP(ctx, hipMemcpyAsync(ctx->scratch[SC_TRIM_OFF].p, read_off, (size_t)(nids + 1) * 8, hipMemcpyHostToDevice, s));
        ctx->trim_nids = nids; ctx->trim_total = total;
    } else if (ctx->trim_nids != nids) {
        return set_err(ctx, NECAT_ERR_ARG, "necat_trim_ranges without records: the context holds no groups of %d reads (necat_trim_partition first)", num_reads);
    }
    unsigned long long* d_nhost = (unsigned long long*)ctx->scratch[SC_TRIM_OFF].p + (nids + 1);
    necat_clip_range* d_clip = (necat_clip_range*)(d_nhost + 1);
    NECAT_HIP(ctx, hipMemsetAsync(d_nhost, 0, 8, s));
    hipLaunchKernelGGL(k_trim_ranges, dim3((unsigned)nids), dim3(64), 0, s, (const necat_m4*)ctx->scratch[SC_TRIM_RECS].p,
                       (const unsigned long long*)ctx->scratch[SC_TRIM_OFF].p, nids, min_ident_perc, min_ovlp_size, min_cov, min_size, d_clip, d_nhost);
    NECAT_CHECK_LAUNCH(ctx, "k_trim_ranges");
    unsigned long long nh = 0;
    NECAT_HIP(ctx, hipMemcpyAsync(out, d_clip, (size_t)nids * sizeof(necat_clip_range), hipMemcpyDeviceToHost, s));
    NECAT_HIP(ctx, hipMemcpyAsync(&nh, d_nhost, 8, hipMemcpyDeviceToHost, s));
    NECAT_HIP(ctx, hipStreamSynchronize(s));
    if (n_host) *n_host = nh;
    return NECAT_OK;
}
