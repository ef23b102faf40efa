// vnd_velvet_pairs.hpp - the velvet-noise optimiser's scan over a pool (include/vnd_velvet_search.h): the eight polar
// moments (vnd_polar.hpp's quantities, vnd_scan_bank_f32_host's order) of candidate c_p of a bank convolved with signal
// s_p of a pool x[batch][n][Cx], for P pairs (s_p, c_p), without writing any convolved signal.
//
// Frames: candidate t owns channels 2t, 2t + 1 of the bank.  Each frame is what conv_ordered_kernel<MODE 0> gives for
// those channels - the same helpers (stage_window, load_taps16, ordered_tap) in the same order: per segment seg += x*w
// in table order, seg *= gain, out += seg; samples past the end of the signal are staged as zeros, so their terms add
// +-0 and drop out; a pass-through channel is the staged input.  A table of +-1 weights runs the fma instantiation as
// every exact-mode launch does (arithmetic_of, vnd_plan.hpp: the product is exact, so the bits are the same).
//
// Shape, after haas_scan_kernel: a workgroup owns one tile of kVpTile frames and a block of kVpBlock consecutive pairs,
// which it walks as runs of one signal.  The signal's window (tile + the bank's largest tap index, Cx planes) is staged
// in LDS once per run; for every pair of the run each lane forms its 2 * kVpR frames (L, R) from LDS and feeds
// polar_add.  The window always fits: a bank whose largest tap index is above VND_VELVET_PAIRS_MAX_TAP_INDEX is refused
// before the launch (VND_ERR_UNSUPPORTED; the caller scores such a bank signal by signal with vnd_scan_bank_f32_host).
//
// Sums are float64 in a fixed order: per lane over its frames (pair j = 0 .. kVpR - 1, first frame then second), the
// fixed shuffle tree and wave order of hs_block_reduce per (pair, tile) partial, then a fixed-order reduction of the
// pair's ceil(n / kVpTile) partials.  The order depends on n alone: neither the other pairs of a launch, nor their
// order, nor the candidate's place in the bank, nor the signal's index enter it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vnd_haas_scan.hpp"
#include "vnd_kernels.hpp"
#include "vnd_polar.hpp"
#include "../../include/vnd_velvet_search.h"

namespace vnd {

constexpr int kVpThreads = kHsThreads;                  // hs_block_reduce's workgroup
constexpr int kVpR = 4;                                 // frame pairs per lane and tile
constexpr int kVpTile = 2 * kVpThreads * kVpR;          // 2048 frames per workgroup
constexpr int kVpBlock = 16;                            // pairs per workgroup
constexpr int kVpMaxHalo = 4096;                        // staged frames past the tile: 2 planes of 6144 floats, 48 KB

struct VpArgs {
    KArgs k;                                            // the bank's tables (table_args), pool (k.x, k.n, k.Cx), k.W
    const int32_t *__restrict__ signals;                // [P]
    const int32_t *__restrict__ candidates;             // [P]
    double *__restrict__ partials;                      // [P][tiles][8]
    double *__restrict__ moments;                       // [P][8]
    int32_t P, batch, T, tiles;                         // pairs, signals in the pool, candidates in the bank
};

__device__ __forceinline__ bool vp_valid(const VpArgs &a, int32_t s, int32_t c)
{
    return s >= 0 && s < a.batch && c >= 0 && c < a.T;
}

// Channel `ch` of the bank over this lane's frames, from the staged plane `pa` (the lane's first pair): the tap loop of
// conv_ordered_kernel.  R: the lane's frame pairs (the block stream of vnd_each_stream.hpp picks its tile per call).
template <int MODE, int R = kVpR>
__device__ __forceinline__ void vp_channel(const KArgs &a, int ch, const float *pa, v2f (&out)[R])
{
    constexpr int NT = kVpThreads;
    if (a.chan_flags != nullptr && (a.chan_flags[ch] & 1)) {          // unfiltered: copy through
#pragma unroll
        for (int j = 0; j < R; ++j) out[j] = *(const v2f *)(pa + 2 * NT * j);
        return;
    }
#pragma unroll
    for (int j = 0; j < R; ++j) out[j] = v2f{0.0f, 0.0f};
    const bool has_seg = a.seg_off != nullptr;
    const unsigned lane_addr = lds_addr(pa);
    int k = __builtin_amdgcn_readfirstlane(a.tap_off[ch]);
    const int k_last = __builtin_amdgcn_readfirstlane(a.tap_off[ch + 1]);
    const int s_begin = has_seg ? __builtin_amdgcn_readfirstlane(a.seg_off[ch]) : 0;
    const int nseg = has_seg ? __builtin_amdgcn_readfirstlane(a.seg_off[ch + 1]) - s_begin : 1;
    for (int s = 0; s < nseg; ++s) {
        const int kend = has_seg ? __builtin_amdgcn_readfirstlane(a.seg_end[s_begin + s]) : k_last;
        v2f sb[R];
#pragma unroll
        for (int j = 0; j < R; ++j) sb[j] = v2f{0.0f, 0.0f};
        while (k < kend) {
            FastTap t[16];
            load_taps16(a.taps_ord + k, t);              // zero-padded by 16 records
            const int m = kend - k;
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (i < m) ordered_tap<NT, R, MODE>(t[i], lane_addr, sb);
            k += m < 16 ? m : 16;
        }
        if (has_seg) {              // class path: seg *= envelope (unless identity); out += seg
            if (a.apply_gain) {
                const float gain = a.seg_gain[s_begin + s];
                const v2f gg = {gain, gain};
#pragma unroll
                for (int j = 0; j < R; ++j) sb[j] = sb[j] * gg;
            }
#pragma unroll
            for (int j = 0; j < R; ++j) out[j] = out[j] + sb[j];
        } else {
#pragma unroll
            for (int j = 0; j < R; ++j) out[j] = sb[j];
        }
    }
}

// grid = (tiles, ceil(P / kVpBlock)); dynamic LDS = CX planes of k.W floats
template <int CX, int MODE>
__global__ __launch_bounds__(kVpThreads) void velvet_pairs_kernel(const VpArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float vp_lds[];
    __shared__ double red[kVpThreads / 64][kMoments];
    __shared__ int32_t sl[kVpBlock], cl[kVpBlock];      // signal and candidate of each pair (candidate -1: outside the contract)
    __shared__ int32_t run_end[kVpBlock];               // at a run's first pair: its end
    const int tid = threadIdx.x;
    const int f0 = blockIdx.y * kVpBlock;
    const int nb = min(kVpBlock, a.P - f0);
    if (tid < nb) {
        const int32_t s = a.signals[f0 + tid], c = a.candidates[f0 + tid];
        sl[tid] = s;
        cl[tid] = vp_valid(a, s, c) ? c : -1;
    }
    __syncthreads();
    if (tid < nb && (tid == 0 || sl[tid - 1] != sl[tid])) {
        int c = tid;
        while (c < nb && sl[c] == sl[tid]) ++c;
        run_end[tid] = c;
    }
    __syncthreads();
    const KArgs &k = a.k;
    const int W = k.W;
    const int64_t t0 = (int64_t)blockIdx.x * kVpTile;
    // runs of consecutive pairs of one signal (wave-uniform: every bound comes from LDS)
    for (int r0 = 0, r1; r0 < nb; r0 = r1) {
        r1 = run_end[r0];
        const int32_t s = __builtin_amdgcn_readfirstlane(sl[r0]);
        if (s < 0 || s >= a.batch) continue;            // no pair of the run is inside the contract
        const float *__restrict__ xs = k.x + (int64_t)s * k.n * CX;
        __syncthreads();                                // the previous run's readers are done with the window
        stage_window<kVpThreads, CX>(vp_lds, xs + t0 * CX, (k.n - t0) * CX * 4, CX, W, tid);
        __syncthreads();
        for (int c = r0; c < r1; ++c) {
            const int32_t cand = __builtin_amdgcn_readfirstlane(cl[c]);
            if (cand < 0) continue;
            v2f out[2][kVpR];
            vp_channel<MODE>(k, 2 * cand, vp_lds + 2 * tid, out[0]);
            vp_channel<MODE>(k, 2 * cand + 1, vp_lds + (CX == 2 ? W : 0) + 2 * tid, out[1]);
            PolarAcc acc;
#pragma unroll
            for (int j = 0; j < kVpR; ++j) {
                const int64_t f = t0 + 2 * tid + 2 * kVpThreads * j;
                if (f < k.n) polar_add(acc, out[0][j].x, out[1][j].x);
                if (f + 1 < k.n) polar_add(acc, out[0][j].y, out[1][j].y);
            }
            double v[kMoments];
            polar_store(v, acc);
            hs_block_reduce(v, red);
            if (tid == 0) {
                double *p = a.partials + ((int64_t)(f0 + c) * a.tiles + blockIdx.x) * kMoments;
#pragma unroll
                for (int q = 0; q < kMoments; ++q) p[q] = v[q];
            }
        }
    }
}

// One workgroup per pair: lanes stride over its tiles' partials, then the fixed tree.  A pair outside the contract
// gets NaN moments.
__global__ __launch_bounds__(kVpThreads) void velvet_pairs_reduce_kernel(const VpArgs a)
{
    __shared__ double red[kVpThreads / 64][kMoments];
    const int f = blockIdx.x;
    const bool ok = vp_valid(a, a.signals[f], a.candidates[f]);
    const int tiles = ok ? a.tiles : 0;
    double v[kMoments];
#pragma unroll
    for (int q = 0; q < kMoments; ++q) v[q] = 0.0;
    for (int c = threadIdx.x; c < tiles; c += kVpThreads) {
        const double *p = a.partials + ((int64_t)f * a.tiles + c) * kMoments;
#pragma unroll
        for (int q = 0; q < kMoments; ++q) v[q] = q == 4 ? fmax(v[q], p[q]) : v[q] + p[q];
    }
    hs_block_reduce(v, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < kMoments; ++q) a.moments[(int64_t)f * kMoments + q] = ok ? v[q] : __builtin_nan("");
    }
}

}  // namespace vnd

static_assert(VND_VELVET_PAIRS_MAX == 65535 * vnd::kVpBlock, "the grid's y extent bounds the pairs per call");
static_assert(((VND_VELVET_PAIRS_MAX_TAP_INDEX + 2 + 15) & ~15) == vnd::kVpMaxHalo, "the largest halo the staged window holds");
static_assert(2 * (vnd::kVpTile + vnd::kVpMaxHalo) * sizeof(float) + 1024 <= 65536, "the window fits the default LDS limit");

extern "C" {

static int64_t velvet_tiles(int64_t n_frames) { return (n_frames + kVpTile - 1) / kVpTile; }

vnd_status vnd_velvet_pairs_workspace_bytes(int64_t n_frames, int32_t n_pairs, int64_t *bytes)
{
    if (!bytes) return fail(VND_ERR_INVALID, "null bytes");
    *bytes = 0;
    if (n_frames < 0 || n_pairs < 0) return fail(VND_ERR_INVALID, "negative frame or pair count");
    if (velvet_tiles(n_frames) > (1 << 23))
        return fail(VND_ERR_UNSUPPORTED, "signal above %lld frames", (long long)kVpTile << 23);
    *bytes = velvet_tiles(n_frames) * n_pairs * kMoments * (int64_t)sizeof(double);
    return VND_OK;
}

// What both entries check before anything else: scalars and the bank, no index array.
static vnd_status velvet_pairs_check(const vnd_ctx *ctx, const vnd_taps *t, int32_t batch, int64_t n_frames,
                                     int32_t in_channels, int32_t n_pairs, int32_t mode)
{
    if (!ctx || !t) return fail(VND_ERR_INVALID, "null context or tap table");
    if (batch < 0 || n_frames < 0 || n_pairs < 0) return fail(VND_ERR_INVALID, "negative batch, frame or pair count");
    if (in_channels != 1 && in_channels != 2)
        return fail(VND_ERR_INVALID, "a velvet-noise scan takes mono or stereo signals, got %d channels", in_channels);
    if (t->C % 2 != 0) return fail(VND_ERR_INVALID, "a scan needs stereo pairs: the bank has %d channels", t->C);
    if (t->ctx != ctx && t->ctx->device != ctx->device)
        return fail(VND_ERR_INVALID, "the tap table lives on device %d, the context on device %d", t->ctx->device, ctx->device);
    if (mode != VND_MODE_EXACT) return fail(VND_ERR_UNSUPPORTED, "the pairs scan runs in VND_MODE_EXACT only, got mode %d", mode);
    if (n_pairs > VND_VELVET_PAIRS_MAX)
        return fail(VND_ERR_UNSUPPORTED, "more than %d pairs per call: split them", VND_VELVET_PAIRS_MAX);
    if (t->max_index > VND_VELVET_PAIRS_MAX_TAP_INDEX || !t->lds_images)
        return fail(VND_ERR_UNSUPPORTED, "the bank's largest tap index %d is above %d: scan it signal by signal", t->max_index,
                    VND_VELVET_PAIRS_MAX_TAP_INDEX);
    if (t->nonfinite) return fail(VND_ERR_UNSUPPORTED, "the bank has a weight that is not finite: scan it signal by signal");
    if (n_frames > 0 && (int64_t)batch > INT64_MAX / 2 / n_frames)
        return fail(VND_ERR_UNSUPPORTED, "pool of %d x %lld frames too large", batch, (long long)n_frames);
    int64_t ws = 0;
    return vnd_velvet_pairs_workspace_bytes(n_frames, n_pairs, &ws);
}

// Both entries after velvet_pairs_check, device pointers in: the two kernels enqueued on the caller's stream.
static vnd_status velvet_pairs_launch(vnd_ctx *ctx, const vnd_taps *t, const float *x, int32_t batch, int64_t n_frames,
                                      int32_t in_channels, const int32_t *signals, const int32_t *candidates,
                                      int32_t n_pairs, double *moments, void *workspace, int64_t workspace_bytes,
                                      void *stream_)
{
    if (n_pairs == 0) return VND_OK;
    if (!signals || !candidates || !moments || (n_frames > 0 && batch > 0 && !x))
        return fail(VND_ERR_INVALID, "null signal, index or moments pointer");
    int64_t need = 0;
    vnd_velvet_pairs_workspace_bytes(n_frames, n_pairs, &need);
    if (workspace_bytes < need || (need > 0 && !workspace))
        return fail(VND_ERR_INVALID, "workspace too small: need %lld bytes", (long long)need);
    DeviceScope on(ctx->device);
    hipStream_t stream = (hipStream_t)stream_;
    VpArgs a{};
    table_args(a.k, t);
    a.k.x = x; a.k.n = n_frames; a.k.C = t->C; a.k.Cx = in_channels;
    a.k.W = kVpTile + halo_of(t->max_index);
    a.signals = signals; a.candidates = candidates; a.partials = (double *)workspace; a.moments = moments;
    a.P = n_pairs; a.batch = batch; a.T = t->C / 2; a.tiles = (int32_t)velvet_tiles(n_frames);
    if (a.tiles > 0) {
        const bool fma = arithmetic_of(t, VND_MODE_EXACT) != VND_MODE_EXACT;      // +-1 weights: the same bits
        void (*kern)(const VpArgs) = in_channels == 2 ? (fma ? velvet_pairs_kernel<2, 1> : velvet_pairs_kernel<2, 0>)
                                                      : (fma ? velvet_pairs_kernel<1, 1> : velvet_pairs_kernel<1, 0>);
        const size_t lds = (size_t)in_channels * a.k.W * sizeof(float);
        hipLaunchKernelGGL(kern, dim3((unsigned)a.tiles, (unsigned)((n_pairs + kVpBlock - 1) / kVpBlock)),
                           dim3(kVpThreads), lds, stream, a);
    }
    hipLaunchKernelGGL(velvet_pairs_reduce_kernel, dim3((unsigned)n_pairs), dim3(kVpThreads), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return VND_OK;
}

vnd_status vnd_velvet_pairs_f32_dev(vnd_ctx *ctx, const vnd_taps *t, const float *x, int32_t batch, int64_t n_frames,
                                    int32_t in_channels, const int32_t *signals, const int32_t *candidates,
                                    int32_t n_pairs, int32_t mode, double *moments, void *workspace,
                                    int64_t workspace_bytes, void *stream_)
{
    vnd_status st = velvet_pairs_check(ctx, t, batch, n_frames, in_channels, n_pairs, mode);
    if (st != VND_OK) return st;
    if (workspace_bytes < 0) return fail(VND_ERR_INVALID, "negative workspace size");
    return velvet_pairs_launch(ctx, t, x, batch, n_frames, in_channels, signals, candidates, n_pairs, moments, workspace,
                               workspace_bytes, stream_);
}

vnd_status vnd_velvet_pairs_f32_host(vnd_ctx *ctx, const vnd_taps *t, const float *x, int32_t batch, int64_t n_frames,
                                     int32_t in_channels, const int32_t *signals, const int32_t *candidates,
                                     int32_t n_pairs, int32_t mode, double *moments)
{
    vnd_status st = velvet_pairs_check(ctx, t, batch, n_frames, in_channels, n_pairs, mode);
    if (st != VND_OK) return st;
    if (n_pairs == 0) return VND_OK;
    if (!signals || !candidates || !moments || (n_frames > 0 && batch > 0 && !x))
        return fail(VND_ERR_INVALID, "null signal, index or moments pointer");
    for (int32_t p = 0; p < n_pairs; ++p) {
        if (signals[p] < 0 || signals[p] >= batch)
            return fail(VND_ERR_INVALID, "signal %d of pair %d is outside [0, %d)", signals[p], p, batch);
        if (candidates[p] < 0 || candidates[p] >= t->C / 2)
            return fail(VND_ERR_INVALID, "candidate %d of pair %d is outside [0, %d)", candidates[p], p, t->C / 2);
    }
    int64_t ws = 0;
    vnd_velvet_pairs_workspace_bytes(n_frames, n_pairs, &ws);
    HostCall call(ctx);
    const size_t x_bytes = (size_t)batch * n_frames * in_channels * sizeof(float);
    const size_t i_bytes = (size_t)n_pairs * sizeof(int32_t);
    const size_t m_bytes = (size_t)n_pairs * kMoments * sizeof(double);
    call.carve({(size_t)ws, m_bytes, i_bytes, i_bytes, x_bytes});
    double *m_dev = call.piece<double>(1);
    int32_t *s_dev = call.piece<int32_t>(2), *c_dev = call.piece<int32_t>(3);
    float *x_dev = call.piece<float>(4);
    call.up(x_dev, x, x_bytes, "x");
    call.up(s_dev, signals, i_bytes, "signals");
    call.up(c_dev, candidates, i_bytes, "candidates");
    call.run([&] { return velvet_pairs_launch(ctx, t, x_dev, batch, n_frames, in_channels, s_dev, c_dev, n_pairs, m_dev,
                                              call.piece<char>(0), ws, call.stream()); });
    call.down(moments, m_dev, m_bytes, "moments");
    return call.finish("vnd_velvet_pairs_f32_host");
}

}  // extern "C"
