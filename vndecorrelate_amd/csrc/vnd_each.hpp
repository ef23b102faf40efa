// vnd_each.hpp - a pool through one filter or one delay PER SIGNAL (include/vnd_each.h): the application side of the
// batched optimisers, which return one kappa or one delay for every signal of a pool.
//
// Velvet noise: each_kernel is the sibling of velvet_pairs_kernel (vnd_velvet_pairs.hpp) that WRITES the frames.  A
// workgroup owns one tile of kVpTile frames of one signal b and the candidate tables[b] of a bank (candidate t owns
// channels 2t, 2t + 1).  It stages the signal's window (tile + the bank's largest tap index, CX planes) in LDS once,
// forms its frames with vp_channel - conv_ordered_kernel<MODE 0>'s bits: the same helpers in the same order - applies
// the decorrelate stage's pointwise steps in registers (EPI: epi_pointwise on the input frames still staged, as the
// ordered kernel's store phase does) and stores them.  The normaliser follows as decorrelate_dev runs it behind a
// launch that left no block sums (stage_setup ... stage_sums).
//
// Store: lane tid holds the frame pairs q = tid + kVpThreads * j, j < kVpR, each as (L_f, R_f, L_f+1, R_f+1), f = 2q:
// 16 bytes, consecutive lanes on consecutive 16 bytes.  It leaves through store_result's raw buffer descriptor over
// the rest of the signal's row: one 16-byte store where the tile starts 16-byte aligned (always, unless n is odd and so
// is b, or the caller's pointer is not), two 8-byte stores otherwise; the descriptor's range check is per dword, so of
// the last frame of an odd n the 8 bytes in range are written, and frames at or past n are dropped.
//
// HaasEffect: haas_each_kernel is haas_kernel (vnd_haas.hpp) with the delay read per signal, over a padded block of
// n + max_delay rows per signal; the rows past a signal's own n + d are zeros.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vnd_haas.hpp"
#include "vnd_velvet_pairs.hpp"
#include "../../include/vnd_each.h"

namespace vnd {

struct EachArgs {
    KArgs k;                                            // the bank's tables (table_args), pool (k.x, k.n, k.Cx), k.y, k.W, k.epi_*
    const int32_t *__restrict__ tables;                 // [batch]
    int32_t T;                                          // candidates in the bank
};

// One tile of a stream or signal through candidate `cand` of the bank - what each_kernel and each_stream_kernel
// (vnd_each_stream.hpp) share.  stage() fills the CX planes of W floats at `lds` with the tile's window; store(q, v) takes
// frame pair q = tid + kVpThreads * j, j < R, as (L_f, R_f, L_f+1, R_f+1), f = 2q.  cand is workgroup-uniform; outside
// [0, T) - outside the contract - the tile's row is NaN and nothing is staged.
template <int CX, int MODE, int R, bool EPI, typename Stage, typename Store>
__device__ __forceinline__ void each_tile(const KArgs &k, const float *lds, int32_t cand, int32_t T, Stage stage, Store store)
{
    const int tid = threadIdx.x;
    if (cand < 0 || cand >= T) {
        const float nan = __builtin_nanf("");
        const float v[4] = {nan, nan, nan, nan};
#pragma unroll
        for (int j = 0; j < R; ++j) store(tid + kVpThreads * j, v);
        return;
    }
    stage();
    __syncthreads();
    const float *right = lds + (CX == 2 ? k.W : 0);
    v2f out[2][R];
    vp_channel<MODE, R>(k, 2 * cand, lds + 2 * tid, out[0]);
    vp_channel<MODE, R>(k, 2 * cand + 1, right + 2 * tid, out[1]);
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int q = tid + kVpThreads * j;
        float v[4] = {out[0][j].x, out[1][j].x, out[0][j].y, out[1][j].y};
        if constexpr (EPI) {
            const float2 x0 = *(const float2 *)(lds + 2 * q), x1 = *(const float2 *)(right + 2 * q);
            const float xin[4] = {x0.x, x1.x, x0.y, x1.y};
            epi_pointwise(k, v, xin);
        }
        store(q, v);
    }
}

// grid = (ceil(n / kVpTile), batch); dynamic LDS = CX planes of k.W floats
template <int CX, int MODE, bool EPI>
__global__ __launch_bounds__(kVpThreads) void each_kernel(const EachArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float each_lds[];
    const KArgs &k = a.k;
    const int64_t b = blockIdx.y;
    const int64_t t0 = (int64_t)blockIdx.x * kVpTile;
    const float *__restrict__ xs = k.x + b * k.n * CX;
    float *dst = k.y + (b * k.n + t0) * 2;
    const v4i rdst = make_rsrc(dst, (k.n - t0) * 2 * 4);           // the rest of this signal's row: nothing past it is written
    const int shape = access_shape<2>(dst, 2);                     // workgroup-uniform
    each_tile<CX, MODE, kVpR, EPI>(
        k, each_lds, __builtin_amdgcn_readfirstlane(a.tables[b]), a.T,
        [&] { stage_window<kVpThreads, CX>(each_lds, xs + t0 * CX, (k.n - t0) * CX * 4, CX, k.W, (int)threadIdx.x); },
        [&](int q, const float (&v)[4]) { store_result_aux<2, kStoreAux>(rdst, shape, q, 1, 2, v); });
}

struct HeArgs {
    HArgs h;                                            // h.delay is not read: the delay is the signal's own
    const int32_t *__restrict__ delays;                 // [batch]
    int32_t max_delay;
};

// grid = (ceil((n + max_delay) / kHaasThreads), batch): one lane per frame of the padded block
__global__ __launch_bounds__(kHaasThreads) void haas_each_kernel(const HeArgs a)
{
    const HArgs &h = a.h;
    const int64_t rows = h.n + a.max_delay;
    const int64_t k = (int64_t)blockIdx.x * kHaasThreads + threadIdx.x;
    if (k >= rows) return;
    const int32_t d = a.delays[blockIdx.y];
    const float *__restrict__ xs = h.x + (int64_t)blockIdx.y * h.n * h.Cx;
    double *__restrict__ ys = h.y + (int64_t)blockIdx.y * rows * 2;
    double v[2];
    if (d < 0 || d > a.max_delay) {                     // outside the contract: the signal's rows are NaN
        v[0] = v[1] = __builtin_nan("");
    } else if (k >= h.n + d) {                          // past this signal's own n + d frames: padding
        v[0] = v[1] = 0.0;
    } else {
        double c[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) c[j] = haas_column(h, xs, j, j == h.delayed_channel ? k - d : k);   // np.roll: zeros wrap in
        haas_frame(h, c[0], c[1], v);
    }
    *(double2 *)(ys + 2 * k) = make_double2(v[0], v[1]);
}

}  // namespace vnd

extern "C" {

// The bank of a filter per signal or per stream, in two halves: a stream entry reports its position and frame count between
// them.  `one` / `many`: "signal" / "signals" or "stream" / "streams"; `instead`: what to do with a bank that is refused.
static vnd_status each_bank_pairs(const vnd_ctx *ctx, const vnd_taps *t)
{
    if (t->C % 2 != 0) return fail(VND_ERR_INVALID, "a bank holds stereo pairs: this one has %d channels", t->C);
    if (t->ctx != ctx && t->ctx->device != ctx->device)
        return fail(VND_ERR_INVALID, "the tap table lives on device %d, the context on device %d", t->ctx->device, ctx->device);
    return VND_OK;
}

static vnd_status each_bank_limits(const vnd_taps *t, int64_t batch, int32_t mode, const char *one, const char *many,
                                   const char *instead)
{
    if (mode != VND_MODE_EXACT) return fail(VND_ERR_UNSUPPORTED, "a filter per %s runs in VND_MODE_EXACT only, got mode %d", one, mode);
    if (batch > VND_MAX_STREAMS) return fail(VND_ERR_UNSUPPORTED, "more than %d %s per call: split the pool", VND_MAX_STREAMS, many);
    if (t->max_index > VND_VELVET_PAIRS_MAX_TAP_INDEX || !t->lds_images)
        return fail(VND_ERR_UNSUPPORTED, "the bank's largest tap index %d is above %d: %s", t->max_index,
                    VND_VELVET_PAIRS_MAX_TAP_INDEX, instead);
    if (t->nonfinite) return fail(VND_ERR_UNSUPPORTED, "the bank has a weight that is not finite: %s", instead);
    return VND_OK;
}

// What every velvet entry checks before anything else: scalars and the bank, no index array (after velvet_pairs_check).
static vnd_status each_check(const vnd_ctx *ctx, const vnd_taps *t, int32_t batch, int64_t n_frames, int32_t in_channels,
                             int32_t mode)
{
    if (!ctx || !t) return fail(VND_ERR_INVALID, "null context or tap table");
    if (batch < 0 || n_frames < 0) return fail(VND_ERR_INVALID, "negative batch or frame count");
    if (in_channels != 1 && in_channels != 2)
        return fail(VND_ERR_INVALID, "a pool of mono or stereo signals is taken, got %d channels", in_channels);
    vnd_status st = each_bank_pairs(ctx, t);
    if (st == VND_OK) st = each_bank_limits(t, batch, mode, "signal", "signals", "convolve it signal by signal");
    if (st != VND_OK) return st;
    if (n_frames > 0 && (int64_t)batch > INT64_MAX / 8 / n_frames)
        return fail(VND_ERR_UNSUPPORTED, "pool of %d x %lld frames too large", batch, (long long)n_frames);
    if (velvet_tiles(n_frames) > INT32_MAX) return fail(VND_ERR_UNSUPPORTED, "signal above %lld frames", (long long)kVpTile * INT32_MAX);
    return VND_OK;
}

// the pointer checks of a non-empty call
static vnd_status each_pointers(const float *x, const int32_t *tables, const float *y, int32_t batch, int64_t n, int32_t Cx)
{
    if (!x || !y || !tables) return fail(VND_ERR_INVALID, "null signal or table index pointer");
    if (overlaps(x, (int64_t)batch * n * Cx, y, (int64_t)batch * n * 2)) return fail(VND_ERR_INVALID, "x and y overlap");
    return VND_OK;
}

// The kernel enqueued on the caller's stream, after the checks; e: the stage's pointwise steps, or null.
static vnd_status each_launch(vnd_ctx *ctx, const vnd_taps *t, const float *x, const int32_t *tables, float *y, int32_t batch,
                              int64_t n, int32_t Cx, const EArgs *e, hipStream_t stream)
{
    EachArgs a{};
    table_args(a.k, t);
    a.k.x = x; a.k.y = y; a.k.n = n; a.k.C = t->C; a.k.Cx = Cx;
    a.k.W = kVpTile + halo_of(t->max_index);
    a.tables = tables; a.T = t->C / 2;
    const bool epi = e && (e->ms_encode || e->use_width);
    if (epi) { a.k.epi_ms_encode = e->ms_encode; a.k.epi_use_width = e->use_width; a.k.epi_w_mid = e->w_mid; a.k.epi_w_side = e->w_side; }
    const bool fma = arithmetic_of(t, VND_MODE_EXACT) != VND_MODE_EXACT;          // +-1 weights: the same bits
    void (*kern)(const EachArgs) =
        Cx == 2 ? (epi ? (fma ? each_kernel<2, 1, true> : each_kernel<2, 0, true>) : (fma ? each_kernel<2, 1, false> : each_kernel<2, 0, false>))
                : (epi ? (fma ? each_kernel<1, 1, true> : each_kernel<1, 0, true>) : (fma ? each_kernel<1, 1, false> : each_kernel<1, 0, false>));
    const size_t lds = (size_t)Cx * a.k.W * sizeof(float);
    hipLaunchKernelGGL(kern, dim3((unsigned)velvet_tiles(n), (unsigned)batch), dim3(kVpThreads), lds, stream, a);
    HIP_TRY(hipGetLastError());
    return VND_OK;
}

vnd_status vnd_convolve_each_f32_dev(vnd_ctx *ctx, const vnd_taps *t, const float *x, const int32_t *tables, float *y,
                                     int32_t batch, int64_t n, int32_t in_channels, int32_t mode, void *stream)
{
    vnd_status st = each_check(ctx, t, batch, n, in_channels, mode);
    if (st != VND_OK) return st;
    if (batch == 0 || n == 0) return VND_OK;
    if ((st = each_pointers(x, tables, y, batch, n, in_channels)) != VND_OK) return st;
    DeviceScope on(ctx->device);
    return each_launch(ctx, t, x, tables, y, batch, n, in_channels, nullptr, (hipStream_t)stream);
}

vnd_status vnd_decorrelate_each_f32_dev(vnd_ctx *ctx, const vnd_taps *t, const float *x, const int32_t *tables, float *y,
                                        int32_t batch, int64_t n, int32_t in_channels, int32_t mode, int32_t ms_encode,
                                        int32_t use_width, double width, int32_t normalize, float eps, void *workspace,
                                        int64_t workspace_bytes, void *stream_)
{
    vnd_status st = each_check(ctx, t, batch, n, in_channels, mode);
    if (st != VND_OK) return st;
    if (workspace_bytes < 0) return fail(VND_ERR_INVALID, "negative workspace size");
    if (batch == 0 || n == 0) return VND_OK;
    if ((st = each_pointers(x, tables, y, batch, n, in_channels)) != VND_OK) return st;
    int64_t need = 0;
    vnd_decorrelate_workspace_bytes(batch, n, 2, &need);
    if (normalize && (!workspace || workspace_bytes < need))
        return fail(VND_ERR_INVALID, "workspace too small: need %lld bytes", (long long)need);
    DeviceScope on(ctx->device);
    hipStream_t stream = (hipStream_t)stream_;
    // decorrelate_dev's table-order branch with the pointwise steps in the convolution's store phase and no block sums left
    StageSetup s = stage_setup(ctx, x, y, batch, n, in_channels, 2, VND_MODE_EXACT, ms_encode, use_width, width, normalize, eps,
                               workspace);
    EArgs &e = s.e;
    if ((st = each_launch(ctx, t, x, tables, y, batch, n, in_channels, &e, stream)) != VND_OK) return st;
    e.ms_encode = e.use_width = 0;                         // done
    if (!normalize) return VND_OK;
    const bool seq = s.want_seq;                           // the sums in NumPy's order: always here (exact mode, two channels)
    e.rows = seq ? 1 : (int32_t)epi_chunks(n);
    if (seq) e.normalize = 0;
    else hipLaunchKernelGGL(epilogue_pointwise_kernel, s.grid, dim3(kEpiThreads), 0, stream, e);
    return stage_sums(ctx, s, x, y, batch, n, in_channels, 2, normalize, seq, false, stream);
}

static vnd_status each_host(vnd_ctx *ctx, const vnd_taps *t, const float *x, const int32_t *tables, float *y, int32_t batch,
                            int64_t n, int32_t Cx, int32_t mode, bool stage, int32_t ms_encode, int32_t use_width, double width,
                            int32_t normalize, float eps, const char *name)
{
    vnd_status st = each_check(ctx, t, batch, n, Cx, mode);
    if (st != VND_OK) return st;
    if (batch == 0 || n == 0) return VND_OK;
    if ((st = each_pointers(x, tables, y, batch, n, Cx)) != VND_OK) return st;
    int64_t ws = 0;
    if (stage && normalize) vnd_decorrelate_workspace_bytes(batch, n, 2, &ws);
    const HostIndex ix{tables, t->C / 2, false, "table", "tables", "signal"};
    HostCall call(ctx);
    call.staged(x, (size_t)batch * n * Cx * sizeof(float), "x", y, (size_t)batch * n * 2 * sizeof(float), &ix, batch, (size_t)ws,
                nullptr, [&](void *x_dev, void *y_dev, int32_t *t_dev, void *ws_dev, hipStream_t s) {
        if (!stage) return vnd_convolve_each_f32_dev(ctx, t, (const float *)x_dev, t_dev, (float *)y_dev, batch, n, Cx, mode, s);
        return vnd_decorrelate_each_f32_dev(ctx, t, (const float *)x_dev, t_dev, (float *)y_dev, batch, n, Cx, mode, ms_encode,
                                            use_width, width, normalize, eps, ws_dev, ws, s);
    });
    return call.finish(name);
}

vnd_status vnd_convolve_each_f32_host(vnd_ctx *ctx, const vnd_taps *t, const float *x, const int32_t *tables, float *y,
                                      int32_t batch, int64_t n, int32_t in_channels, int32_t mode)
{
    return each_host(ctx, t, x, tables, y, batch, n, in_channels, mode, false, 0, 0, 0.0, 0, 0.0f, "vnd_convolve_each_f32_host");
}

vnd_status vnd_decorrelate_each_f32_host(vnd_ctx *ctx, const vnd_taps *t, const float *x, const int32_t *tables, float *y,
                                         int32_t batch, int64_t n, int32_t in_channels, int32_t mode, int32_t ms_encode,
                                         int32_t use_width, double width, int32_t normalize, float eps)
{
    return each_host(ctx, t, x, tables, y, batch, n, in_channels, mode, true, ms_encode, use_width, width, normalize, eps,
                     "vnd_decorrelate_each_f32_host");
}

// ---- HaasEffect with a delay per signal -------------------------------------------------------------------------------
static vnd_status haas_each_check(const vnd_ctx *ctx, int64_t batch, int64_t n, int32_t in_channels, int32_t max_delay,
                                  int32_t delayed_channel)
{
    vnd_status st = haas_check(ctx, batch, n, in_channels, max_delay, delayed_channel);
    if (st != VND_OK) return st;
    const int64_t rows = n + max_delay;
    if (rows > 0 && batch > INT64_MAX / 16 / rows)
        return fail(VND_ERR_UNSUPPORTED, "pool of %lld x %lld frames too large", (long long)batch, (long long)rows);
    if ((rows + kHaasThreads - 1) / kHaasThreads > INT32_MAX)
        return fail(VND_ERR_UNSUPPORTED, "signal above %lld frames", (long long)kHaasThreads * INT32_MAX);
    return VND_OK;
}

vnd_status vnd_haas_each_f64_dev(vnd_ctx *ctx, const float *x, double *y, int64_t batch, int64_t n, int32_t in_channels,
                                 const int32_t *delays, int32_t max_delay, int32_t delayed_channel, int32_t ms_mode,
                                 int32_t use_width, double width, void *stream)
{
    vnd_status st = haas_each_check(ctx, batch, n, in_channels, max_delay, delayed_channel);
    if (st != VND_OK) return st;
    const int64_t rows = n + max_delay;
    if (batch == 0 || rows == 0) return VND_OK;
    if (!y || !delays || (n > 0 && !x)) return fail(VND_ERR_INVALID, "null signal or delay pointer");
    DeviceScope on(ctx->device);
    HeArgs a{};
    a.h.x = x; a.h.y = y; a.h.n = n; a.h.Cx = in_channels; a.h.delayed_channel = delayed_channel;
    a.h.ms = ms_mode ? 1 : 0; a.h.use_width = use_width ? 1 : 0; a.h.w_mid = 1.0 - width; a.h.w_side = width;
    a.delays = delays; a.max_delay = max_delay;
    const dim3 grid((unsigned)((rows + kHaasThreads - 1) / kHaasThreads), (unsigned)batch);
    hipLaunchKernelGGL(haas_each_kernel, grid, dim3(kHaasThreads), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return VND_OK;
}

vnd_status vnd_haas_each_f64_host(vnd_ctx *ctx, const float *x, double *y, int64_t batch, int64_t n, int32_t in_channels,
                                  const int32_t *delays, int32_t max_delay, int32_t delayed_channel, int32_t ms_mode,
                                  int32_t use_width, double width)
{
    vnd_status st = haas_each_check(ctx, batch, n, in_channels, max_delay, delayed_channel);
    if (st != VND_OK) return st;
    const int64_t rows = n + max_delay;
    if (batch == 0 || rows == 0) return VND_OK;
    if (!y || !delays || (n > 0 && !x)) return fail(VND_ERR_INVALID, "null signal or delay pointer");
    const HostIndex ix{delays, max_delay, true, "delay", "delays", "signal"};
    HostCall call(ctx);
    call.staged(x, (size_t)batch * n * in_channels * sizeof(float), "x", y, (size_t)batch * rows * 2 * sizeof(double), &ix, batch, 0,
                nullptr, [&](void *x_dev, void *y_dev, int32_t *d_dev, void *, hipStream_t s) {
        return vnd_haas_each_f64_dev(ctx, (const float *)x_dev, (double *)y_dev, batch, n, in_channels, d_dev, max_delay,
                                     delayed_channel, ms_mode, use_width, width, s);
    });
    return call.finish("vnd_haas_each_f64_host");
}

}  // extern "C"
