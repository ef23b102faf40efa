// vnd_hooks.hpp - measurement, tuning and diagnosis hooks (include/vnd_amd_internal.h): timing loops, the streaming-copy ceiling, the generated kernel sources, the variant override, phase stamps.
// (one translation unit: included by vnd_amd.hip after vnd_objects.hpp; everything static here is private to the library)
#pragma once

extern "C" {

vnd_status vnd_time_convolve_f32_dev(vnd_ctx *ctx, const vnd_taps *t, const float *x, float *y, int64_t batch,
                                     int64_t n, int32_t C, int32_t mode, int32_t n_buffers, int64_t stride,
                                     int32_t iters, void *stream_, float *avg_ms)
{
    vnd_status st = check_shape(ctx, t, batch, n, C, mode);
    if (st != VND_OK) return st;
    if (!avg_ms || iters <= 0 || n_buffers <= 0) return fail(VND_ERR_INVALID, "bad timing arguments");
    DeviceScope on(ctx->device);
    hipStream_t stream = (hipStream_t)stream_;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t he = hipEventCreate(&e0);
    if (he == hipSuccess) he = hipEventCreate(&e1);
    if (he == hipSuccess) he = hipEventRecord(e0, stream);
    for (int i = 0; he == hipSuccess && st == VND_OK && i < iters; ++i) {
        const int64_t off = (int64_t)(i % n_buffers) * stride;
        st = launch(ctx, t, x + off, y + off, batch, n, C, mode, stream);
    }
    float ms = 0.f;
    if (he == hipSuccess) he = hipEventRecord(e1, stream);
    if (he == hipSuccess) he = hipEventSynchronize(e1);
    if (he == hipSuccess) he = hipEventElapsedTime(&ms, e0, e1);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (st != VND_OK) return st;
    if (he != hipSuccess) return fail(VND_ERR_HIP, "timing: %s", hipGetErrorString(he));
    *avg_ms = ms / iters;
    return VND_OK;
}

// The streaming ceiling of the box, for bench.py: a plain copy with the per-table kernels' access shape (16 bytes per
// lane, non-temporal loads and stores) - the best of the shapes tools/micro/copy_ceiling.hip tries (5.9 TB/s on 7.9 GB
// each way, where hipMemcpyAsync reaches 5.1).  Not on the data path.
typedef float copy_v4f __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void stream_copy_kernel(const copy_v4f *x, copy_v4f *y, long long quads)
{
    const long long stride = (long long)gridDim.x * 256 * 4;
    for (long long base = (long long)blockIdx.x * 256 * 4 + threadIdx.x; base < quads; base += stride) {
        copy_v4f a[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) if (base + k * 256 < quads) a[k] = __builtin_nontemporal_load(x + base + k * 256);
#pragma unroll
        for (int k = 0; k < 4; ++k) if (base + k * 256 < quads) __builtin_nontemporal_store(a[k], y + base + k * 256);
    }
}

vnd_status vnd_time_copy_f32_dev(vnd_ctx *ctx, const float *x, float *y, int64_t elems, int32_t iters, void *stream_, float *avg_ms)
{
    if (!ctx || !x || !y || !avg_ms || iters <= 0 || elems <= 0 || (elems & 3)) return fail(VND_ERR_INVALID, "bad copy timing arguments");
    if (((uintptr_t)x | (uintptr_t)y) & 15) return fail(VND_ERR_INVALID, "the copy wants 16-byte aligned buffers");
    DeviceScope on(ctx->device);
    hipStream_t stream = (hipStream_t)stream_;
    const long long quads = elems / 4;
    const unsigned grid = (unsigned)std::min<long long>(65536, (quads + 1023) / 1024);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t he = hipEventCreate(&e0);
    if (he == hipSuccess) he = hipEventCreate(&e1);
    if (he == hipSuccess) he = hipEventRecord(e0, stream);
    for (int i = 0; he == hipSuccess && i < iters; ++i)
        hipLaunchKernelGGL(stream_copy_kernel, dim3(grid), dim3(256), 0, stream, (const copy_v4f *)x, (copy_v4f *)y, quads);
    float ms = 0.f;
    if (he == hipSuccess) he = hipEventRecord(e1, stream);
    if (he == hipSuccess) he = hipEventSynchronize(e1);
    if (he == hipSuccess) he = hipEventElapsedTime(&ms, e0, e1);
    if (he == hipSuccess) he = hipGetLastError();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (he != hipSuccess) return fail(VND_ERR_HIP, "copy timing: %s", hipGetErrorString(he));
    *avg_ms = ms / iters;
    return VND_OK;
}

// the SpecTable of a CSR tap table as the source hooks take it (seg_offsets NULL: the function path): whole channel pairs, offsets
// under 2^24, finite weights, segments that cover their channel's taps without an empty one
static vnd_status spec_table_from_csr(int32_t C, const int32_t *tap_offsets, const int32_t *tap_index, const float *tap_weight,
                                      const int32_t *seg_offsets, const int32_t *seg_end, const float *seg_gain, int32_t apply_gain,
                                      SpecTable *t)
{
    if (C < 2 || (C & 1) || C > 64 || !tap_offsets || tap_offsets[0] != 0)
        return fail(VND_ERR_INVALID, "the per-table kernels take a CSR tap table of whole channel pairs (2..64 channels)");
    t->C = C;
    t->tap_off.assign(tap_offsets, tap_offsets + C + 1);
    const int32_t total = tap_offsets[C];
    if (total <= 0 || !tap_index || !tap_weight) return fail(VND_ERR_INVALID, "empty tap table");
    for (int32_t k = 0; k < total; ++k) {
        if (tap_index[k] < 0 || tap_index[k] >= (1 << 24) || !std::isfinite(tap_weight[k]))
            return fail(VND_ERR_UNSUPPORTED, "tap %d is outside the specialised kernel's scope", k);
        t->max_index = std::max(t->max_index, tap_index[k]);
    }
    t->idx.assign(tap_index, tap_index + total);
    t->w.assign(tap_weight, tap_weight + total);
    t->w_raw = t->w;
    if (!seg_offsets) return VND_OK;
    if (!seg_end || !seg_gain || seg_offsets[0] != 0) return fail(VND_ERR_INVALID, "segment arrays incomplete");
    t->has_seg = true;
    t->apply_gain = apply_gain != 0;
    t->seg_off.assign(seg_offsets, seg_offsets + C + 1);
    t->seg_end.assign(seg_end, seg_end + seg_offsets[C]);
    t->seg_gain.assign(seg_gain, seg_gain + seg_offsets[C]);
    for (int c = 0; c < C; ++c) {
        int32_t prev = tap_offsets[c];
        for (int32_t sg = seg_offsets[c]; sg < seg_offsets[c + 1]; ++sg) {
            if (seg_end[sg] <= prev || seg_end[sg] > tap_offsets[c + 1]) return fail(VND_ERR_UNSUPPORTED, "empty or misplaced segment");
            prev = seg_end[sg];
            if (apply_gain)
                for (int32_t k = (sg == seg_offsets[c] ? tap_offsets[c] : seg_end[sg - 1]); k < seg_end[sg]; ++k) t->w[k] = tap_weight[k] * seg_gain[sg];
        }
        if (prev != tap_offsets[c + 1]) return fail(VND_ERR_UNSUPPORTED, "segments do not cover the channel's taps");
    }
    return VND_OK;
}

static vnd_status source_out(const std::string &src, char *text, int64_t capacity, int64_t *bytes)
{
    *bytes = (int64_t)src.size() + 1;
    if (!text) return VND_OK;                    // size query
    if (capacity < *bytes) return fail(VND_ERR_INVALID, "buffer too small: need %lld bytes", (long long)*bytes);
    memcpy(text, src.c_str(), src.size() + 1);
    return VND_OK;
}

vnd_status vnd_spec_kernel_source(int32_t C, const int32_t *tap_offsets, const int32_t *tap_index,
                                  const float *tap_weight, int32_t mode, char *text, int64_t capacity, int64_t *bytes)
{
    if (mode != VND_MODE_FAST && mode != VND_MODE_EXACT)
        return fail(VND_ERR_INVALID, "the specialised kernel exists for VND_MODE_FAST and VND_MODE_EXACT");
    if (!bytes) return fail(VND_ERR_INVALID, "null bytes pointer");
    const Tuning tun = tuning_snapshot();
    SpecTable t;
    if (vnd_status st = spec_table_from_csr(C, tap_offsets, tap_index, tap_weight, nullptr, nullptr, nullptr, 0, &t); st != VND_OK) return st;
    SpecConfig cfg;
    if (!spec_pick_config(t, tun, 160 * 1024, 0, 0, &cfg, false, false, mode == VND_MODE_EXACT)) return fail(VND_ERR_UNSUPPORTED, "halo does not fit the LDS ring");
    cfg.exact = mode == VND_MODE_EXACT ? 1 : 0;
    return source_out(spec_prologue(t, cfg) + kSpecKernelSource, text, capacity, bytes);
}

vnd_status vnd_window_kernel_source(int32_t C, const int32_t *tap_offsets, const int32_t *tap_index,
                                    const float *tap_weight, const int32_t *seg_offsets, const int32_t *seg_end,
                                    const float *seg_gain, int32_t apply_gain, int32_t mode, int32_t frames_per_lane,
                                    int32_t threads, char *text, int64_t capacity, int64_t *bytes,
                                    int64_t *lds_bytes_per_tile, int64_t *fmas_per_tile)
{
    if (mode != VND_MODE_FAST && mode != VND_MODE_EXACT)
        return fail(VND_ERR_INVALID, "the specialised kernel exists for VND_MODE_FAST and VND_MODE_EXACT");
    if (!bytes) return fail(VND_ERR_INVALID, "null bytes pointer");
    const Tuning tun = tuning_snapshot();
    SpecTable t;
    if (vnd_status st = spec_table_from_csr(C, tap_offsets, tap_index, tap_weight, seg_offsets, seg_end, seg_gain, apply_gain, &t); st != VND_OK)
        return st;
    const int M = frames_per_lane, G = tun.win_g > 0 ? tun.win_g : 8;
    WinGeom g;
    // (tables of 4k channels: the quad / octet form, as the launches take it - VND_WIN_QUAD=0: channel pairs)
    bool quad = C % 8 == 0 && tun.win_quad != 0 && tun.win_octet != 0 && win_geometry(t, M, threads, G, false, 160 * 1024, &g, 2);
    quad = quad || ((C % 4 == 0 || (C % 4 == 2 && C >= 6)) && tun.win_quad != 0 && win_geometry(t, M, threads, G, false, 160 * 1024, &g, 1));
    // (VND_WIN_SPLIT=1: the split form of a stereo table)
    const bool split = !quad && C == 2 && tun.win_split > 0 && win_geometry(t, M, threads, G, false, 160 * 1024, &g, 0, true);
    // (VND_WIN_SOURCE_FANOUT=1: the source of a mono input's fan-out launch through a stereo table - VW_BC)
    const bool bc = C == 2 && tun.win_source_fanout != 0;
    if (bc && !win_geometry(t, M, threads, G, true, 160 * 1024, &g, 0, split))
        return fail(VND_ERR_UNSUPPORTED, "this window geometry does not fit the LDS");
    if (!bc && !quad && !split && !win_geometry(t, M, threads, G, false, 160 * 1024, &g))
        return fail(VND_ERR_UNSUPPORTED, "this window geometry does not fit the LDS");
    SpecConfig cfg = win_config(t, g, tun, mode == VND_MODE_EXACT, bc);
    // (VND_WIN_SOURCE_EPI=1: with the decorrelate stage's steps in the store phase - stereo: pointwise steps and block sums; quads /
    //  octets, fast mode: the normaliser's sums)
    cfg.epi = (tun.win_source_epi != 0 && !bc && !split && (C == 2 || quad)) ? 1 : 0;
    if (lds_bytes_per_tile || fmas_per_tile) {
        size_t lb = 0, fm = 0;
        if (cfg.exact) win_traffic_exact(t, M, &lb, &fm);
        else win_traffic(t, M, &lb, &fm);
        if (lds_bytes_per_tile) *lds_bytes_per_tile = (int64_t)lb;
        if (fmas_per_tile) *fmas_per_tile = (int64_t)fm;
    }
    return source_out(win_source(t, g, cfg), text, capacity, bytes);
}

vnd_status vnd_code_object_private_bytes(const void *code, int64_t bytes, const char *kernel, int64_t *private_bytes)
{
    if (!code || bytes <= 0 || !kernel || !private_bytes) return fail(VND_ERR_INVALID, "bad arguments");
    const std::vector<char> image((const char *)code, (const char *)code + bytes);
    *private_bytes = spec_private_bytes(image, kernel);
    return VND_OK;
}

vnd_status vnd_tuning_read(const char *name, int32_t fallback, int32_t *value)
{
    if (!name || !value) return fail(VND_ERR_INVALID, "null name or value pointer");
    for (const TuningName &v : kTuningNames)
        if (strcmp(v.name, name) == 0) { *value = tuning_value(v, fallback); return VND_OK; }
    *value = fallback;
    return fail(VND_ERR_INVALID, "'%.64s' is not a registered tuning variable (kTuningNames, csrc/vnd_spec.hpp)", name);
}

vnd_status vnd_set_variant(vnd_ctx *ctx, int32_t variant)
{
    if (!ctx) return fail(VND_ERR_INVALID, "null context");
    ctx->variant = decode_variant(variant);
    return VND_OK;
}

vnd_status vnd_debug_read_stamps(vnd_ctx *ctx, const vnd_taps *t, int64_t batch, int64_t n, int32_t in_channels, int32_t mode,
                                 uint64_t *stamps, int64_t capacity, int64_t *count)
{
    if (!ctx || !t || !count || capacity < 0 || (capacity > 0 && !stamps)) return fail(VND_ERR_INVALID, "bad arguments");
    *count = 0;
    vnd_status st = check_shape(ctx, t, batch, n, t->C, mode, in_channels);
    if (st != VND_OK) return st;
    DeviceScope on(ctx->device);
    const SpecPlan sp = make_spec_plan(ctx, t, nullptr, nullptr, batch, n, t->C, in_channels, mode, nullptr);
    if (!sp.use || !sp.cfg.win) return VND_OK;
    SpecModule *m = spec_module(ctx, t, sp.cfg, true);
    if (!m || m->failed || !m->module) return VND_OK;
    hipDeviceptr_t at = nullptr;
    size_t bytes = 0;
    if (hipModuleGetGlobal(&at, &bytes, m->module, "vw_stamps") != hipSuccess) { (void)hipGetLastError(); return VND_OK; }
    *count = (int64_t)(bytes / sizeof(uint64_t));
    const size_t take = std::min<size_t>(bytes, (size_t)capacity * sizeof(uint64_t));
    HIP_TRY(hipDeviceSynchronize());
    if (take) HIP_TRY(hipMemcpy(stamps, at, take, hipMemcpyDeviceToHost));
    return VND_OK;
}

// The StreamPlan a vnd_stream_f32_dev call of this shape takes: the same make_stream_plan, on the call's output frames.
vnd_status vnd_describe_stream_launch(vnd_ctx *ctx, const vnd_taps *t, int64_t batch, int64_t n_out, int32_t in_channels,
                                      int32_t mode, int32_t epilogue, char *text, int32_t len)
{
    if (!ctx || !t) return fail(VND_ERR_INVALID, "null context or tap table");
    if (!text || len <= 0) return fail(VND_ERR_INVALID, "null text buffer");
    if (batch < 0 || batch > VND_MAX_STREAMS) return fail(VND_ERR_INVALID, "batch %lld outside 0..%d", (long long)batch, VND_MAX_STREAMS);
    if (n_out < 0) return fail(VND_ERR_INVALID, "negative frame count");
    if (in_channels <= 0 || t->C % in_channels != 0)
        return fail(VND_ERR_INVALID, "%d input channels do not divide the tap table's %d channels", in_channels, t->C);
    if (mode != VND_MODE_EXACT && mode != VND_MODE_FMA && mode != VND_MODE_FAST) return fail(VND_ERR_INVALID, "unknown mode %d", mode);
    if (epilogue && t->C != 2)
        return fail(VND_ERR_INVALID, "the side-channel encode and the width need 2 output channels, the table has %d", t->C);
    const StreamPlan p = make_stream_plan(ctx, t, batch, n_out, t->C, in_channels, mode, epilogue != 0);
    snprintf(text, (size_t)len,
             "%s direct=%d r=%d cg=%d bc=%d W=%d lds_bytes=%zu tiles=%d groups=%d nblocks=%u mode=%d epilogue=%d threads=%d",
             p.direct ? "conv_stream_direct" : "conv_stream", p.direct ? 1 : 0, p.r, p.cg, p.bc ? 1 : 0, p.W, p.lds_bytes,
             p.tiles, p.groups, p.nblocks, mode, epilogue ? 1 : 0, p.direct ? kDirectThreads : kStreamThreads);
    return VND_OK;
}

// The route a vnd_scan_bank_f32_host call of this shape takes: the call's own scalar checks and scan_route, the call's own
// decision.  No pointers, no device work (make_spec_plan only plans: nothing is built or looked up).
vnd_status vnd_describe_scan(vnd_ctx *ctx, const vnd_taps *t, int64_t n, int32_t in_channels, int32_t mode, char *text,
                             int32_t len)
{
    vnd_status st = scan_check(ctx, t, n, in_channels, mode);
    if (st != VND_OK) return st;
    if (!text || len <= 0) return fail(VND_ERR_INVALID, "null text buffer");
    const ScanRoute s = scan_route(ctx, t, n, in_channels, mode);
    const Plan &p = s.p;
    const int pairs = t->C / 2;
    char conv[64];
    if (n == 0) snprintf(conv, sizeof conv, "conv_none");
    else if (p.direct) snprintf(conv, sizeof conv, "conv_direct");
    else snprintf(conv, sizeof conv, "%s%s", mode == VND_MODE_FAST ? "conv_fast" : "conv_ordered", p.bc ? "_fanout" : "");
    // the unfused launch carries no epilogue, so a large enough one may go to the per-table kernel where that builds
    const bool spec = n > 0 && !s.fused && make_spec_plan(ctx, t, nullptr, nullptr, 1, n, t->C, in_channels, mode, nullptr).use;
    snprintf(text, (size_t)len, "%s%s %s%s cg=%d r=%d nt=%d bc=%d tiles=%d direct=%d halo=%d lds=%zuB workgroups=%u mode=%d pairs=%d",
             s.fused ? "fused" : "unfused", s.fused ? "" : (pairs >= kMomByCandidatePairs ? " by_candidate" : " by_frame"), conv,
             spec ? " (or the per-table kernel)" : "", p.cg, p.r, p.direct ? kDirectThreads : p.nt, p.bc ? 1 : 0, p.tiles,
             p.direct ? 1 : 0, p.direct || n == 0 ? 0 : p.W - 2 * p.nt * p.r, p.lds_bytes, p.nblocks, mode, pairs);
    return VND_OK;
}

// The EachStreamPlan a vnd_each_stream_f32_dev call with these arguments takes: the same checks and planner, no pointers.
vnd_status vnd_describe_each_stream_launch(vnd_ctx *ctx, const vnd_taps *t, int64_t max_frames_per_call, int64_t batch,
                                           int64_t pos, int64_t n_in, int32_t in_channels, int32_t final_, int32_t mode,
                                           int32_t epilogue, char *text, int32_t len)
{
    if (!text || len <= 0) return fail(VND_ERR_INVALID, "null text buffer");
    int64_t nout = 0;
    vnd_status st = each_stream_scalars(ctx, t, max_frames_per_call, batch, pos, n_in, in_channels, final_, mode, &nout);
    if (st != VND_OK) return st;
    const EachStreamPlan p = make_each_stream_plan(ctx, t, batch, nout, in_channels, epilogue != 0);
    snprintf(text, (size_t)len, "each_stream r=%d W=%d lds_bytes=%zu tiles=%d nblocks=%u n_out=%lld fma=%d epilogue=%d threads=%d",
             p.r, p.W, p.lds_bytes, p.tiles, p.nblocks, (long long)nout, p.fma ? 1 : 0, p.epi ? 1 : 0, kVpThreads);
    return VND_OK;
}

// The plan of a vnd_voice_stream_f32_dev call on a pool with these arguments: the pool's scalar checks and
// make_voice_stream_plan, the launch's own; advance_groups = the grid of voice_advance_kernel.  No pointers, no device work.
vnd_status vnd_describe_voice_stream_launch(vnd_ctx *ctx, const vnd_taps *t, int64_t max_frames_per_call, int64_t slots,
                                            int32_t in_channels, int32_t mode, int32_t epilogue, char *text, int32_t len)
{
    if (!text || len <= 0) return fail(VND_ERR_INVALID, "null text buffer");
    int64_t need = 0;
    vnd_status st = voice_stream_scalars(ctx, t, max_frames_per_call, slots, in_channels, mode, &need);
    if (st != VND_OK) return st;
    if ((st = voice_stream_rows(t, max_frames_per_call, slots)) != VND_OK) return st;
    const EachStreamPlan p = make_voice_stream_plan(ctx, t, slots, max_frames_per_call, in_channels, epilogue != 0);
    snprintf(text, (size_t)len, "voice_stream r=%d W=%d lds_bytes=%zu tiles=%d nblocks=%u fma=%d epilogue=%d threads=%d advance_groups=%lld",
             p.r, p.W, p.lds_bytes, p.tiles, p.nblocks, p.fma ? 1 : 0, p.epi ? 1 : 0, kVpThreads,
             (long long)voice_advance_groups(slots));
    return VND_OK;
}

// The plan of a vnd_voice_fade_stream_f32_dev call on a pool with these arguments: vnd_describe_voice_stream_launch's
// sibling - the crossfading pool's scalar checks, the same planner - with fade_frames behind its fields.
vnd_status vnd_describe_voice_fade_stream_launch(vnd_ctx *ctx, const vnd_taps *t, int64_t max_frames_per_call,
                                                 int64_t fade_frames, int64_t slots, int32_t in_channels, int32_t mode,
                                                 int32_t epilogue, char *text, int32_t len)
{
    if (!text || len <= 0) return fail(VND_ERR_INVALID, "null text buffer");
    int64_t need = 0;
    vnd_status st = voice_fade_scalars(ctx, t, max_frames_per_call, fade_frames, slots, in_channels, mode, &need);
    if (st != VND_OK) return st;
    if ((st = voice_stream_rows(t, max_frames_per_call, slots)) != VND_OK) return st;
    const EachStreamPlan p = make_voice_stream_plan(ctx, t, slots, max_frames_per_call, in_channels, epilogue != 0);
    snprintf(text, (size_t)len, "voice_fade_stream r=%d W=%d lds_bytes=%zu tiles=%d nblocks=%u fma=%d epilogue=%d threads=%d advance_groups=%lld fade_frames=%lld",
             p.r, p.W, p.lds_bytes, p.tiles, p.nblocks, p.fma ? 1 : 0, p.epi ? 1 : 0, kVpThreads,
             (long long)voice_advance_groups(slots), (long long)fade_frames);
    return VND_OK;
}

// The fixed launch of every vnd_correlogram_voice_stream_*_dev call on a pool with these sizes: the pool's own scalar checks
// and cg_voice_plan, the launch's own.  No pointers, no device work.
vnd_status vnd_describe_correlogram_voice_stream_launch(int64_t slots, int32_t window, int32_t hop, int32_t num_lags,
                                                        int64_t max_frames_per_call, char *text, int32_t len)
{
    if (!text || len <= 0) return fail(VND_ERR_INVALID, "null text buffer");
    CgVoicePlan p{};
    vnd_status st = cg_voice_plan(slots, window, hop, num_lags, max_frames_per_call, &p);
    if (st != VND_OK) return st;
    snprintf(text, (size_t)len, "correlogram_voice_stream rows_per_call=%lld groups=%lld tiles=%lld nblocks=%lld threads=%d advance_groups=%lld",
             (long long)p.rc, (long long)p.groups, (long long)p.tiles, (long long)p.workgroups, kCgThreads,
             (long long)p.advance_groups);
    return VND_OK;
}

// The fixed launch of every vnd_polar_voice_stream_*_dev call on a pool with these sizes: the pool's own scalar checks and
// polar_voice_plan, the launch's own.  No pointers, no device work.
vnd_status vnd_describe_polar_voice_stream_launch(int64_t slots, int64_t max_frames_per_call, int32_t sample_bytes, char *text,
                                                  int32_t len)
{
    if (!text || len <= 0) return fail(VND_ERR_INVALID, "null text buffer");
    PolarVoicePlan p{};
    vnd_status st = polar_voice_plan(slots, max_frames_per_call, sample_bytes, &p);
    if (st != VND_OK) return st;
    snprintf(text, (size_t)len, "polar_voice_stream groups=%lld nblocks=%lld finish_groups=%lld threads=%d state_bytes=%lld",
             (long long)p.G, (long long)p.workgroups, (long long)p.finish_groups, kPolarVoiceLanes, (long long)p.need);
    return VND_OK;
}

// The fixed launch of every vnd_spectrum_voice_stream_*_dev call on a pool with these sizes: the pool's own scalar checks and
// sv_plan, the launch's own.  No pointers, no device work.
vnd_status vnd_describe_spectrum_voice_stream_launch(int64_t slots, int32_t channels, int32_t nperseg, int32_t hop, int32_t nfft,
                                                     int64_t max_frames_per_call, int32_t is_float64, char *text, int32_t len)
{
    if (!text || len <= 0) return fail(VND_ERR_INVALID, "null text buffer");
    SvPlan p{};
    vnd_status st = sv_plan(slots, channels, nperseg, hop, nfft, max_frames_per_call, is_float64 ? 8 : 4, &p);
    if (st != VND_OK) return st;
    snprintf(text, (size_t)len, "spectrum_voice_stream rows_per_call=%lld run=%d groups=%lld nblocks=%lld threads=%d advance_groups=%lld state_bytes=%lld",
             (long long)p.rc, p.run, (long long)p.groups, (long long)p.workgroups, kSpectrumThreads, (long long)p.finish_groups,
             (long long)p.need);
    return VND_OK;
}

}  // extern "C"
