// vnd_haas_scan_voice_stream.hpp - the Haas-delay scan of a voice pool (include/vnd_haas_scan_voice_stream.h): the eight polar
// moments of vnd_haas_scan.hpp for (slot, delay) pairs, scored against the last W frames of every voice, the signal arriving
// block by block, the position per slot in the device state and a count and start / end flags per slot and call.
// (one translation unit: included by vnd_amd.hip after vnd_haas_scan.hpp, vnd_voice_core.hpp and vnd_voice_window.hpp)
//
// The state keeps the window itself: per slot a ring of input frames, entry g mod W the voice's frame g, as the caller pushed
// it (float32, Cx values a frame).  A delay cares about order, so beside fill - how many entries are the voice's - the state
// keeps head = (p + n) mod W of the slot's last answered push, the entry the NEXT frame would take: the window in time order
// is the entries (head - fill + k) mod W, k in [0, fill).  Both survive an END, which zeroes the position only.
//
// PUSH, two launches on the caller's stream, grids fixed by (slots, M):
//   haas_scan_voice_copy_kernel, the walk of vnd_voice_window.hpp: idle slots, bad slots and workgroups past n leave at once.
//     Frame j of the chunk is the voice's frame g = p + j; the lane copies it to entry g mod W.  It reads nothing of the rings.
//   voice_advance_kernel<HaasScanVoiceArgs> (vnd_voice_core.hpp) writes valid[b] and pos[b]; the slot's advance() also writes
//     fill[b] = min(p + n, W) and head[b] = (p + n) mod W, by the same lane, for a slot that answers 1.
// The slot rule is scope_voice_span's (vnd_voice_window.hpp) as it stands; its `clear` is not used: nothing is cleared.
//
// PAIRS, a pure function of the state: hs_scan_body and hs_reduce_body of vnd_haas_scan.hpp over HsRingArgs - the one-shot's
// body, instantiated with the loader HsRingFrames, whose column(c, k) reads entry (first + k) mod W, first = (head - fill)
// mod W, where the one-shot's reads x[k].  Everything else - the tile, the runs, the staged delayed column, the unstaged route,
// the shuffle tree, the partials and their reduction - is the same text, so the same order of the same float64 operations.
//
// Every index that is built from device data:
//   - the push: vnd_voice_window.hpp's list;
//   - slots_of_pair[p] outside [0, slots), delays[p] outside [0, max_delay], fill[slot] outside [0, W] or head[slot] outside
//     [0, W): valid() is false, the pair gets dl = -1 in the scan and a row of NaN from the reduction; fill and head of a slot
//     are read only after its index passed, and open() only for a slot whose fill and head passed;
//   - ring entries: first in [0, W) and k in [0, fill), fill <= W: one wrap;
//   - partials: ceil((fill + d) / kHsTile) <= ceil((W + max_delay) / kHsTile) = cap, the launch's x extent.
#pragma once
#include "../../include/vnd_haas_scan_voice_stream.h"

// The window of one slot in time order: frame k is ring entry (first + k) mod W.
struct HsRingFrames {
    const float *__restrict__ ring;     // [W][Cx]
    int64_t n;                          // fill
    int32_t first, W;                   // first in [0, W)
    __device__ __forceinline__ double column(const vnd::HArgs &h, int c, int64_t k) const
    {
        if (k < 0 || k >= n) return 0.0;
        int64_t e = first + k;                                    // k < n <= W: one wrap
        if (e >= W) e -= W;
        if (h.Cx == 1) return vnd::haas_column_of(h, c, (double)ring[e], 0.0);
        return vnd::haas_column_of(h, c, (double)ring[2 * e], (double)ring[2 * e + 1]);
    }
};

// vnd_haas_scan.hpp's Args over the rings of a pool: h carries the configuration only (h.x and h.n are not used).
struct HsRingArgs {
    vnd::HArgs h;
    const float *__restrict__ ring;                     // [slots][W][Cx]
    const int32_t *__restrict__ fill;                   // [slots]
    const int32_t *__restrict__ head;                   // [slots]
    const int32_t *__restrict__ signals;                // [F] slot of each pair
    const int32_t *__restrict__ delays;                 // [F]
    double *__restrict__ partials;                      // [F][cap][8]
    double *__restrict__ moments;                       // [F][8]
    int32_t F;                                          // pairs
    int32_t slots, W, max_delay;
    int64_t cap;                                        // ceil((W + max_delay) / kHsTile)
    __device__ __forceinline__ int32_t signal(int f) const { return signals[f]; }
    __device__ __forceinline__ bool valid(int32_t s, int32_t d) const
    {
        if (s < 0 || s >= slots || d < 0 || d > max_delay) return false;
        const int32_t n = fill[s], hd = head[s];
        return n >= 0 && n <= W && hd >= 0 && hd < W;
    }
    __device__ __forceinline__ HsRingFrames open(int32_t s) const
    {
        const int32_t n = __builtin_amdgcn_readfirstlane(fill[s]), hd = __builtin_amdgcn_readfirstlane(head[s]);
        int32_t first = hd - n;                                   // in [-W, W)
        if (first < 0) first += W;
        return {ring + (int64_t)s * W * h.Cx, n, first, W};
    }
};

// grid = (cap, ceil(F / kHsBlock)) and (F): the one-shot's two kernels over the rings
__global__ __launch_bounds__(vnd::kHsThreads) void haas_scan_voice_kernel(const HsRingArgs a) { vnd::hs_scan_body(a); }
__global__ __launch_bounds__(vnd::kHsThreads) void haas_scan_voice_reduce_kernel(const HsRingArgs a) { vnd::hs_reduce_body(a); }

struct HaasScanVoiceArgs {
    const float *__restrict__ x;        // [slots][M][Cx]
    float *__restrict__ ring;           // [slots][W][Cx]: frame g at g mod W
    int64_t *__restrict__ pos;          // [slots]
    int32_t *__restrict__ fill;         // [slots]: how many ring entries are the voice's
    int32_t *__restrict__ head;         // [slots]: the entry the voice's next frame takes
    const int32_t *__restrict__ counts;
    const int32_t *__restrict__ flags;
    int32_t *__restrict__ out_counts;   // valid [slots]
    int64_t slots, M, W;
    int32_t Cx;
    __device__ vnd::VoiceAnswer advance(int64_t b) const
    {
        const ScopeVoiceSpan v = scope_voice_span(pos[b], counts[b], flags[b], M);
        if (v.valid == 1) {                                       // (the lane that moves pos[b] on)
            const int64_t q = v.p + v.n;
            fill[b] = (int32_t)(q < W ? q : W);
            head[b] = (int32_t)(q % W);
        }
        return {v.valid, v.valid == 1, v.next};
    }
};

// grid = (ceil(M / kScopeVoiceSpan), slots)
__global__ __launch_bounds__(kScopeVoiceThreads) void haas_scan_voice_copy_kernel(const HaasScanVoiceArgs a)
{
    const int64_t b = blockIdx.y;
    VoiceWindowWalk w;
    if (!w.open(a.pos, a.counts, a.flags, a.M, b, blockIdx.x)) return;
    w.enter(a.W);
    if (a.Cx == 2) {
        const float2 *__restrict__ src = (const float2 *)a.x + b * a.M;           // (x is 16-byte aligned, rows 8 M bytes)
        float2 *__restrict__ dst = (float2 *)a.ring + b * a.W;
        for (int64_t j = w.j0 + threadIdx.x; j < w.j1; j += kScopeVoiceThreads) dst[w.entry(j)] = src[j];
    } else {
        const float *__restrict__ src = a.x + b * a.M;
        float *__restrict__ dst = a.ring + b * a.W;
        for (int64_t j = w.j0 + threadIdx.x; j < w.j1; j += kScopeVoiceThreads) dst[w.entry(j)] = src[j];
    }
}

// ---- the host side ---------------------------------------------------------------------------------------------------------
// The fixed launch of a push, and where the parts of the state begin.
struct HaasScanVoicePlan {
    int64_t copy_groups, fill_at, head_at, ring_at, need;
};

static int64_t haas_scan_voice_pad16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// voice_window_plan's checks (there is no whole-voice form), then the state: the positions, the fills, the heads, the ring.
static vnd_status haas_scan_voice_plan(int64_t slots, int64_t max_frames_per_call, int64_t window_frames, int32_t in_channels,
                                       HaasScanVoicePlan *plan)
{
    HaasScanVoicePlan p{};
    const vnd_status st = voice_window_plan(slots, max_frames_per_call, window_frames, false, &p.copy_groups);
    if (st != VND_OK) return st;
    if (in_channels != 1 && in_channels != 2)
        return fail(VND_ERR_INVALID, "a Haas scan takes mono or stereo voices, got %d channels", in_channels);
    p.fill_at = voice_position_bytes(slots);
    p.head_at = p.fill_at + haas_scan_voice_pad16(slots * (int64_t)sizeof(int32_t));
    p.ring_at = p.head_at + haas_scan_voice_pad16(slots * (int64_t)sizeof(int32_t));
    p.need = p.ring_at + haas_scan_voice_pad16(slots * window_frames * in_channels * (int64_t)sizeof(float));
    *plan = p;
    return VND_OK;
}

// The partials a pair can have: ceil((W + max_delay) / kHsTile), the scan's x extent.
static vnd_status haas_scan_voice_cap(int64_t window_frames, int32_t n_pairs, int32_t max_delay, int64_t *cap)
{
    if (window_frames < 1) return fail(VND_ERR_INVALID, "window_frames must be >= 1");
    if (n_pairs < 0 || max_delay < 0) return fail(VND_ERR_INVALID, "negative pair count or delay");
    if (window_frames > INT32_MAX) return fail(VND_ERR_UNSUPPORTED, "window_frames %lld above INT32_MAX", (long long)window_frames);
    if (n_pairs > VND_HAAS_PAIRS_MAX)
        return fail(VND_ERR_UNSUPPORTED, "more than %d pairs per call: split them", VND_HAAS_PAIRS_MAX);
    *cap = vnd::hs_chunks(window_frames + max_delay);             // at most 2^21
    return VND_OK;
}

extern "C" {

vnd_status vnd_haas_scan_voice_stream_state_bytes(int64_t slots, int64_t max_frames_per_call, int64_t window_frames,
                                                  int32_t in_channels, int64_t *bytes)
{
    if (!bytes) return fail(VND_ERR_INVALID, "null bytes");
    *bytes = 0;
    HaasScanVoicePlan p{};
    const vnd_status st = haas_scan_voice_plan(slots, max_frames_per_call, window_frames, in_channels, &p);
    if (st != VND_OK) return st;
    *bytes = p.need;
    return VND_OK;
}

vnd_status vnd_haas_scan_voice_stream_reset_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t slots,
                                                int64_t max_frames_per_call, int64_t window_frames, int32_t in_channels,
                                                void *stream_)
{
    HaasScanVoicePlan p{};
    vnd_status st = haas_scan_voice_plan(slots, max_frames_per_call, window_frames, in_channels, &p);
    if (st != VND_OK) return st;
    if ((st = voice_state_check("Haas scan voice pool", state, state_bytes, p.need, slots)) != VND_OK) return st;
    if (!ctx) return fail(VND_ERR_INVALID, "null context");
    DeviceScope on(ctx->device);
    if (!on.ok) return fail(VND_ERR_HIP, "cannot select device %d", ctx->device);
    HIP_TRY(hipMemsetAsync(state, 0, (size_t)p.ring_at, (hipStream_t)stream_));       // the positions, the fills, the heads
    return VND_OK;
}

vnd_status vnd_haas_scan_voice_stream_push_f32_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t max_frames_per_call,
                                                   int64_t window_frames, const float *x, int32_t in_channels,
                                                   const int32_t *counts, const int32_t *flags, int32_t *valid, int64_t slots,
                                                   void *stream_)
{
    if (!state || !x || !counts || !flags || !valid)
        return fail(VND_ERR_INVALID, "null state, chunk, counts, flags or valid pointer");
    HaasScanVoicePlan p{};
    vnd_status st = haas_scan_voice_plan(slots, max_frames_per_call, window_frames, in_channels, &p);
    if (st != VND_OK) return st;
    if ((st = voice_state_check("Haas scan voice pool", state, state_bytes, p.need, slots)) != VND_OK) return st;
    if ((uintptr_t)x % (in_channels * sizeof(float)) != 0) return fail(VND_ERR_INVALID, "the chunk is not aligned to a frame");
    const int64_t xb = slots * max_frames_per_call * in_channels * (int64_t)sizeof(float);    // (< 2^16 * 2^31 * 8)
    const ScopeRegion outs[] = {{valid, slots * 4}, {state, p.need}};
    const ScopeRegion ins[] = {{x, xb}, {counts, slots * 4}, {flags, slots * 4}};
    if (const int hit = scope_clash(outs, 2, ins, 3, false))
        return fail(VND_ERR_INVALID, "valid and the state must not overlap %s", hit == 1 ? "the chunk, counts or flags" : "one another");
    if (!ctx) return fail(VND_ERR_INVALID, "null context");
    DeviceScope on(ctx->device);
    if (!on.ok) return fail(VND_ERR_HIP, "cannot select device %d", ctx->device);
    hipStream_t stream = (hipStream_t)stream_;

    HaasScanVoiceArgs a{};
    char *base = (char *)state;
    a.x = x; a.ring = (float *)(base + p.ring_at);
    a.pos = (int64_t *)base; a.fill = (int32_t *)(base + p.fill_at); a.head = (int32_t *)(base + p.head_at);
    a.counts = counts; a.flags = flags; a.out_counts = valid;
    a.slots = slots; a.M = max_frames_per_call; a.W = window_frames; a.Cx = in_channels;
    hipLaunchKernelGGL(haas_scan_voice_copy_kernel, dim3((unsigned)p.copy_groups, (unsigned)slots), dim3(kScopeVoiceThreads), 0,
                       stream, a);
    HIP_TRY(hipGetLastError());
    launch_voice_advance(a, slots, stream);
    HIP_TRY(hipGetLastError());
    return VND_OK;
}

vnd_status vnd_haas_scan_voice_stream_workspace_bytes(int64_t window_frames, int32_t n_pairs, int32_t max_delay, int64_t *bytes)
{
    if (!bytes) return fail(VND_ERR_INVALID, "null bytes");
    *bytes = 0;
    int64_t cap = 0;
    const vnd_status st = haas_scan_voice_cap(window_frames, n_pairs, max_delay, &cap);
    if (st != VND_OK) return st;
    *bytes = cap * n_pairs * kMoments * (int64_t)sizeof(double);
    return VND_OK;
}

vnd_status vnd_haas_scan_voice_stream_pairs_f64_dev(vnd_ctx *ctx, const void *state, int64_t state_bytes,
                                                    int64_t max_frames_per_call, int64_t window_frames, int32_t in_channels,
                                                    int64_t slots, const int32_t *slots_of_pair, const int32_t *delays,
                                                    int32_t n_pairs, int32_t max_delay, int32_t delayed_channel, int32_t ms_mode,
                                                    int32_t use_width, double width, double *moments, void *workspace,
                                                    int64_t workspace_bytes, void *stream_)
{
    if (!state || !slots_of_pair || !delays || !moments || !workspace)
        return fail(VND_ERR_INVALID, "null state, slot index, delay, moments or workspace pointer");
    if (n_pairs < 1) return fail(VND_ERR_INVALID, "n_pairs must be >= 1");
    if (delayed_channel != 0 && delayed_channel != 1)
        return fail(VND_ERR_INVALID, "delayed_channel must be 0 or 1, got %d", delayed_channel);
    HaasScanVoicePlan p{};
    vnd_status st = haas_scan_voice_plan(slots, max_frames_per_call, window_frames, in_channels, &p);
    if (st != VND_OK) return st;
    if ((st = voice_state_check("Haas scan voice pool", state, state_bytes, p.need, slots)) != VND_OK) return st;
    int64_t cap = 0;
    if ((st = haas_scan_voice_cap(window_frames, n_pairs, max_delay, &cap)) != VND_OK) return st;
    const int64_t ws = cap * n_pairs * kMoments * (int64_t)sizeof(double), mb = (int64_t)n_pairs * kMoments * (int64_t)sizeof(double);
    if (workspace_bytes < ws)
        return fail(VND_ERR_INVALID, "workspace of %lld bytes, the call needs %lld", (long long)workspace_bytes, (long long)ws);
    if ((uintptr_t)workspace % 8 != 0 || (uintptr_t)moments % 8 != 0)
        return fail(VND_ERR_INVALID, "moments or the workspace is not 8-byte aligned");
    const ScopeRegion outs[] = {{moments, mb}, {workspace, ws}};
    const ScopeRegion ins[] = {{state, p.need}, {slots_of_pair, (int64_t)n_pairs * 4}, {delays, (int64_t)n_pairs * 4}};
    if (const int hit = scope_clash(outs, 2, ins, 3, false))
        return fail(VND_ERR_INVALID, "moments and the workspace must not overlap %s",
                    hit == 1 ? "the state, the slot indices or the delays" : "one another");
    if (!ctx) return fail(VND_ERR_INVALID, "null context");
    DeviceScope on(ctx->device);
    if (!on.ok) return fail(VND_ERR_HIP, "cannot select device %d", ctx->device);
    hipStream_t stream = (hipStream_t)stream_;

    const char *base = (const char *)state;
    HsRingArgs a{};
    a.h.Cx = in_channels; a.h.delayed_channel = delayed_channel;
    a.h.ms = ms_mode ? 1 : 0; a.h.use_width = use_width ? 1 : 0; a.h.w_mid = 1.0 - width; a.h.w_side = width;
    a.ring = (const float *)(base + p.ring_at);
    a.fill = (const int32_t *)(base + p.fill_at); a.head = (const int32_t *)(base + p.head_at);
    a.signals = slots_of_pair; a.delays = delays; a.partials = (double *)workspace; a.moments = moments; a.F = n_pairs;
    a.slots = (int32_t)slots; a.W = (int32_t)window_frames; a.max_delay = max_delay; a.cap = cap;
    hipLaunchKernelGGL(haas_scan_voice_kernel, dim3((unsigned)cap, (unsigned)((n_pairs + kHsBlock - 1) / kHsBlock)),
                       dim3(kHsThreads), 0, stream, a);
    hipLaunchKernelGGL(haas_scan_voice_reduce_kernel, dim3((unsigned)n_pairs), dim3(kHsThreads), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return VND_OK;
}

}  // extern "C"
