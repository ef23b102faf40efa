// vnd_correlogram_voice_stream.hpp - the cross-correlogram of a voice pool (include/vnd_correlogram_voice_stream.h): the
// block stream of vnd_correlogram_stream.hpp with the stream position moved from the caller into the device state, one per
// slot, and a frame count and start / end flags per slot and call - what vnd_voice_stream.hpp is to vnd_each_stream.hpp.
// (one translation unit: included by vnd_amd.hip after vnd_correlogram_stream.hpp and vnd_voice_stream.hpp)
//
// The compute is correlogram_kernel's (vnd_correlogram.hpp), instantiated with a third sample source, CgVoice<T>.  Its view
// is built per workgroup: the workgroup reads pos[b], counts[b] and flags[b] of its slot once, workgroup-uniform, forms
// p, w0 and its row count with cg_voice_span - the host's own function - and offsets the chunk, ring and output pointers to
// slot b, so the body runs as on stream 0 of a one-stream CgRing call whose position, row count and ring plan are the
// slot's.  Block ranges, staging, cg_load / cg_block, the energy chains and butterfly and the float32 normaliser are the
// one-shot kernel's: every row is the same operation sequence on the same values, bit for bit the one-shot call's row,
// whatever the schedule and the neighbours.  T is the chunk's sample type: a float64 sample is cast to float32 where it is
// read (v_cvt_f32_f64 under the default rounding mode: round to nearest even), into the energies, the staging and the ring
// alike, so the rows are the one-shot call's on the cast signal.
//
// The grid is fixed by the pool - (slots, ceil(RC / kCgG) * tiles), RC = ceil(M / H) the rows a call can complete (the
// header proves the bound) - and not by the call.  The SLOT is the fast dimension, as in voice_stream_kernel: workgroups
// are dealt round-robin over the XCDs by their linear index, and in steady state only the first groups of a slot have rows.
// A workgroup whose group holds no row of this call leaves right after its share of the ring copy, before any barrier.
//
// Ring (vnd_correlogram_stream.hpp's argument, per slot with the slot's own p and n).  cap = W - 1 + M.  Frames read from
// the ring lie in [p - W + 1, p): window wc(p) was not complete at p.  Frames written lie in [p + n - min(n, W - 1), p + n).
// A written frame g and a read frame f satisfy 0 < g - f <= W - 2 + n < cap: different ring slots, so no ring slot is both
// read and written in one call although the slot's workgroups are not ordered.  A frame f in [p - W + 1, p) was written by
// the call that pushed it, and is overwritten only by a frame >= f + cap > p.  A call with END writes nothing: the next
// voice of the slot starts at 0 and reads no frame below its own 0, so the ring is never cleared and a reused slot shows
// nothing of the voice before it.  START puts p to 0: every frame of the call's windows then comes from the chunk.
//
// Every index that is built from device data:
//   - counts[b] outside [0, M], or pos[b] outside [0, 2^60] without START: the view is not ok and the workgroup leaves
//     before anything is addressed with it - so 0 <= p <= 2^60 and 0 <= n <= M below;
//   - chunk frames: a window of this call ends at or below p + n, so the chunk is read at [0, n) only; the ring copy reads
//     [n - min(n, W - 1), n);
//   - ring slots: wr_slot0 = wr_first % cap and slot0 = (w H) % cap lie in [0, cap), each walked forward by less than cap
//     with one wrap;
//   - rows: r < rows <= RC, so row r of slot b lies inside out[b][RC][num_lags].
//
// voice_advance_kernel<CgVoiceArgs<T>>, one lane per slot, follows on the same stream and writes pos[b] and out_counts[b]
// (vnd_voice_core.hpp).
#pragma once
#include "../../include/vnd_correlogram_voice_stream.h"

// One slot's side of a call, from the stored position, counts[b] and flags[b] alone.
struct CgVoiceSpan : vnd::VoiceHead {
    int64_t w0, rows;              // window of row 0, wc(p + n) - wc(p); !ok: the slot is left alone, out_counts = rows = -1
};

__host__ __device__ inline int64_t cg_voice_complete(int64_t q, int64_t W, int64_t H) { return q >= W ? (q - W) / H + 1 : 0; }

__host__ __device__ inline CgVoiceSpan cg_voice_span(int64_t stored, int32_t count, int32_t flags, int64_t M, int64_t W,
                                                     int64_t H)
{
    CgVoiceSpan v{vnd::voice_head(stored, count, flags, M)};
    if (!v.ok) { v.rows = -1; return v; }
    v.w0 = cg_voice_complete(v.p, W, H);
    v.rows = cg_voice_complete(v.p + v.n, W, H) - v.w0;
    return v;
}

template <class T>
struct CgVoiceArgs {
    CgArgs cg;                        // W, hop, num_lags, jmax, tiles, eps, stream_stride, frame_stride; out: the pool's;
                                      // x, y, windows and group0 are not read
    const T *__restrict__ x;          // the chunk: frame t of slot b at b * stream_stride + t * frame_stride
    const T *__restrict__ y;
    float2 *__restrict__ ring;        // [slots][cap] (x, y)
    int64_t *__restrict__ pos;        // [slots]
    const int32_t *__restrict__ counts;
    const int32_t *__restrict__ flags;
    int32_t *__restrict__ out_counts;
    int64_t M, cap, rc;               // max_frames_per_call, W - 1 + M, ceil(M / H)
    int32_t slots;
    __device__ vnd::VoiceAnswer advance(int64_t b) const
    {
        const CgVoiceSpan v = cg_voice_span(pos[b], counts[b], flags[b], M, cg.W, cg.hop);
        return {(int32_t)v.rows, v.ok, v.next};
    }
};

// grid = (slots, ceil(rc / kCgG) * tiles)
template <class T>
struct CgVoice {
    using Args = CgVoiceArgs<T>;
    static constexpr bool kRing = true;
    struct View {                     // workgroup-uniform, of slot b = blockIdx.x
        CgArgs cg;                    // windows: the rows of this call; out: row 0 of the slot
        const T *x, *y;               // the slot's chunk
        float2 *ring;                 // the slot's ring
        int64_t pos, cap, w0;
        int64_t wr_first, wr_count, wr_slot0;       // chunk frames [wr_first, wr_first + wr_count) (absolute) go to the ring
        int64_t group;
        int32_t tile;
        bool ok;
    };
    struct Run {
        const T *px, *py;
        const float2 *ring;
        int64_t rel, slot0, cap;      // rel: the window's first frame - pos
        int32_t fs;
        __device__ __forceinline__ int64_t slot(int i) const
        {
            const int64_t s = slot0 + i;
            return s >= cap ? s - cap : s;
        }
        __device__ __forceinline__ float x(int i) const
        {
            const int64_t r = rel + i;
            return r >= 0 ? (float)px[r * fs] : ring[slot(i)].x;
        }
        __device__ __forceinline__ float y(int i) const
        {
            const int64_t r = rel + i;
            return r >= 0 ? (float)py[r * fs] : ring[slot(i)].y;
        }
    };
    __device__ static __forceinline__ View view(const Args &a)
    {
        View v;
        const int64_t b = blockIdx.x;
        const CgVoiceSpan s = cg_voice_span(vnd::uniform_i64(a.pos[b]), __builtin_amdgcn_readfirstlane(a.counts[b]),
                                            __builtin_amdgcn_readfirstlane(a.flags[b]), a.M, a.cg.W, a.cg.hop);
        v.cg = a.cg;
        v.ok = s.ok;
        v.cg.windows = s.ok ? s.rows : 0;
        v.cg.out = a.cg.out + b * a.rc * (int64_t)a.cg.num_lags;
        v.x = a.x + b * a.cg.stream_stride; v.y = a.y + b * a.cg.stream_stride;
        v.ring = a.ring + b * a.cap;
        v.pos = s.p; v.cap = a.cap; v.w0 = s.w0;
        v.wr_count = !s.ok || s.end ? 0 : (s.n < a.cg.W - 1 ? s.n : a.cg.W - 1);
        v.wr_first = s.p + s.n - v.wr_count;
        v.wr_slot0 = v.wr_count > 0 ? v.wr_first % a.cap : 0;
        v.group = blockIdx.y / (unsigned)a.cg.tiles;
        v.tile = (int32_t)(blockIdx.y % (unsigned)a.cg.tiles);
        return v;
    }
    __device__ static __forceinline__ const CgArgs &cg(const View &v) { return v.cg; }
    __device__ static __forceinline__ int64_t stream(const View &) { return 0; }       // the view's pointers are the slot's
    __device__ static __forceinline__ int64_t group(const View &v) { return v.group; }
    __device__ static __forceinline__ int tile(const View &v) { return v.tile; }
    __device__ static __forceinline__ int64_t first_frame(const View &v, int64_t ww) { return (v.w0 + ww) * v.cg.hop; }
    __device__ static __forceinline__ int64_t slot0_of(const View &v, int64_t ww) { return first_frame(v, ww) % v.cap; }
    __device__ static __forceinline__ Run run(const View &v, int64_t, int64_t ww, int64_t slot0)
    {
        return Run{v.x, v.y, v.ring, first_frame(v, ww) - v.pos, slot0, v.cap, v.cg.frame_stride};
    }
    // The chunk frames later calls read, into the ring: the slot's workgroups share them in grid-stride order.  A
    // workgroup whose group has no row of this call only does this.
    __device__ static __forceinline__ bool prologue(const View &v, int64_t)
    {
        if (!v.ok) return false;
        const int64_t rel0 = v.wr_first - v.pos;
        for (int64_t k = (int64_t)blockIdx.y * kCgThreads + threadIdx.x; k < v.wr_count;
             k += (int64_t)gridDim.y * kCgThreads) {
            int64_t s = v.wr_slot0 + k;
            if (s >= v.cap) s -= v.cap;
            const int64_t r = (rel0 + k) * v.cg.frame_stride;
            v.ring[s] = make_float2((float)v.x[r], (float)v.y[r]);
        }
        return v.group * kCgG < v.cg.windows;
    }
};

// The fixed launch of a pool.
struct CgVoicePlan {
    int64_t rc, groups, tiles, workgroups, advance_groups, cap, need;
};

// The scalar side of the pool's checks, in the order the entries report them.
static vnd_status cg_voice_plan(int64_t slots, int32_t window, int32_t hop, int32_t num_lags, int64_t max_frames_per_call,
                                CgVoicePlan *plan)
{
    if (slots < 1 || window < 1 || hop < 1 || num_lags < 1 || max_frames_per_call < 1)
        return fail(VND_ERR_INVALID, "slots, window, hop, num_lags and max_frames_per_call must be >= 1");
    if (max_frames_per_call > INT32_MAX)
        return fail(VND_ERR_INVALID, "max_frames_per_call %lld above INT32_MAX: counts are int32", (long long)max_frames_per_call);
    CgVoicePlan p{};
    vnd_status st = vnd_correlogram_voice_stream_state_bytes(slots, window, max_frames_per_call, &p.need);
    if (st != VND_OK) return st;
    p.cap = max_frames_per_call + window - 1;
    p.rc = (max_frames_per_call + hop - 1) / hop;
    p.groups = (p.rc + kCgG - 1) / kCgG;
    p.tiles = ((int64_t)num_lags + kCgTile - 1) / kCgTile;
    p.workgroups = slots * p.groups * p.tiles;
    p.advance_groups = vnd::voice_advance_groups(slots);          // what launch_voice_advance launches
    if (slots * p.rc * (int64_t)num_lags > ((int64_t)1 << 40))
        return fail(VND_ERR_UNSUPPORTED, "an out of %lld x %lld x %d values, above 2^40", (long long)slots, (long long)p.rc, num_lags);
    if (p.groups * p.tiles > 65535)
        return fail(VND_ERR_UNSUPPORTED, "%lld window groups x %lld column tiles per slot, above the 65535 of a grid dimension",
                    (long long)p.groups, (long long)p.tiles);
    if (p.workgroups > ((int64_t)1 << 23))
        return fail(VND_ERR_UNSUPPORTED, "%lld workgroups in one launch, above 2^23", (long long)p.workgroups);
    *plan = p;
    return VND_OK;
}

template <class T>
static vnd_status cg_voice_stream_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t max_frames_per_call, const T *x,
                                      const T *y, int64_t stream_stride, int32_t frame_stride, const int32_t *counts,
                                      const int32_t *flags, float *out, int32_t *out_counts, int64_t slots, int32_t window,
                                      int32_t hop, int32_t num_lags, float eps, void *stream_)
{
    if (!ctx) return fail(VND_ERR_INVALID, "null context");
    if (stream_stride < 1 || frame_stride < 1) return fail(VND_ERR_INVALID, "strides must be >= 1");
    CgVoicePlan p{};
    vnd_status st = cg_voice_plan(slots, window, hop, num_lags, max_frames_per_call, &p);
    if (st != VND_OK) return st;
    if ((st = voice_state_check("voice pool", state, state_bytes, p.need, slots)) != VND_OK) return st;
    if (!x || !y || !counts || !flags || !out || !out_counts)
        return fail(VND_ERR_INVALID, "null chunk, counts, flags, output or out_counts pointer");
    int64_t xb = 0;
    if ((st = voice_chunk_bytes(slots, stream_stride, max_frames_per_call, frame_stride, sizeof(T), &xb)) != VND_OK) return st;
    const int64_t ob = slots * p.rc * (int64_t)num_lags * (int64_t)sizeof(float);
    for (const T *c : {x, y})
        if (voice_overlap(c, xb, out, ob) || voice_overlap(c, xb, state, p.need))
            return fail(VND_ERR_INVALID, "out and the state must not overlap the chunk");
    if (voice_overlap(out, ob, state, p.need)) return fail(VND_ERR_INVALID, "out must not overlap the state");
    DeviceScope on(ctx->device);
    if (!on.ok) return fail(VND_ERR_HIP, "cannot select device %d", ctx->device);
    hipStream_t stream = (hipStream_t)stream_;

    CgVoiceArgs<T> a{};
    a.cg.out = out; a.cg.stream_stride = stream_stride; a.cg.frame_stride = frame_stride;
    a.cg.W = window; a.cg.hop = hop; a.cg.num_lags = num_lags;
    a.cg.jmax = (int32_t)std::min<int64_t>(num_lags, 2 * (int64_t)window - 1);
    a.cg.tiles = (int32_t)p.tiles;
    a.cg.eps = eps;
    a.x = x; a.y = y; a.counts = counts; a.flags = flags; a.out_counts = out_counts;
    a.pos = (int64_t *)state;
    a.ring = (float2 *)((char *)state + voice_position_bytes(slots));
    a.M = max_frames_per_call; a.cap = p.cap; a.rc = p.rc; a.slots = (int32_t)slots;
    hipLaunchKernelGGL(correlogram_kernel<CgVoice<T>>, dim3((unsigned)slots, (unsigned)(p.groups * p.tiles)), dim3(kCgThreads),
                       0, stream, a);
    HIP_TRY(hipGetLastError());
    launch_voice_advance(a, slots, stream);
    HIP_TRY(hipGetLastError());
    return VND_OK;
}

extern "C" {

vnd_status vnd_correlogram_voice_stream_state_bytes(int64_t slots, int32_t window, int64_t max_frames_per_call, int64_t *bytes)
{
    if (!bytes) return fail(VND_ERR_INVALID, "null bytes");
    *bytes = 0;
    if (slots < 1) return fail(VND_ERR_INVALID, "slots, window and max_frames_per_call must be >= 1");
    if (slots > VND_MAX_STREAMS) return fail(VND_ERR_UNSUPPORTED, "slots %lld above %d: split the pool", (long long)slots, VND_MAX_STREAMS);
    int64_t ring = 0;
    vnd_status st = vnd_correlogram_stream_state_bytes(slots, window, max_frames_per_call, &ring);
    if (st != VND_OK) return st;
    *bytes = voice_position_bytes(slots) + ring;
    return VND_OK;
}

vnd_status vnd_correlogram_voice_stream_reset_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t slots,
                                                  int32_t window, int64_t max_frames_per_call, void *stream_)
{
    if (!ctx) return fail(VND_ERR_INVALID, "null context");
    int64_t need = 0;
    vnd_status st = vnd_correlogram_voice_stream_state_bytes(slots, window, max_frames_per_call, &need);
    if (st != VND_OK) return st;
    if ((st = voice_state_check("voice pool", state, state_bytes, need, slots)) != VND_OK) return st;
    return voice_reset_positions(ctx, state, slots, stream_);
}

vnd_status vnd_correlogram_voice_stream_f32_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t max_frames_per_call,
                                                const float *x, const float *y, int64_t stream_stride, int32_t frame_stride,
                                                const int32_t *counts, const int32_t *flags, float *out, int32_t *out_counts,
                                                int64_t slots, int32_t window, int32_t hop, int32_t num_lags, float eps,
                                                void *stream)
{
    return cg_voice_stream_dev<float>(ctx, state, state_bytes, max_frames_per_call, x, y, stream_stride, frame_stride, counts,
                                      flags, out, out_counts, slots, window, hop, num_lags, eps, stream);
}

vnd_status vnd_correlogram_voice_stream_f64_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t max_frames_per_call,
                                                const double *x, const double *y, int64_t stream_stride, int32_t frame_stride,
                                                const int32_t *counts, const int32_t *flags, float *out, int32_t *out_counts,
                                                int64_t slots, int32_t window, int32_t hop, int32_t num_lags, float eps,
                                                void *stream)
{
    return cg_voice_stream_dev<double>(ctx, state, state_bytes, max_frames_per_call, x, y, stream_stride, frame_stride, counts,
                                       flags, out, out_counts, slots, window, hop, num_lags, eps, stream);
}

}  // extern "C"
