// vnd_polar_voice_stream.hpp - the eight polar moments of a voice pool (include/vnd_polar_voice_stream.h): the one-shot
// reducer of vnd_moments.hpp (moments_by_frame_kernel + moments_reduce_kernel, n_pairs = 1) as a stream whose position
// lives in the device state, one per slot, with a frame count and start / end flags per slot and call - what
// vnd_correlogram_voice_stream.hpp is to the correlogram.
// (one translation unit: included by vnd_amd.hip after vnd_stage.hpp and vnd_voice_stream.hpp)
//
// The one-shot call sums in an order fixed by absolute frame positions: chunk c = frames [512 c, 512 c + 512); lane t adds
// frames 512 c + t and 512 c + 256 + t; shuffle tree 32..1; the four waves in order; reduce lane t adds the partials of the
// chunks c = t (mod 256) in ascending c from +0.0; the tree again.  A stream reproduces it exactly by carrying
//   - the 256 x 8 reduce-lane sums over the COMPLETED chunks (sums), and
//   - the frames of the chunk still incomplete (ring),
// and by forming, per call, the partial of every chunk the call touches from the ring (frames below p) and the block.
// vnd_moments.hpp is not touched and shares nothing with this file but polar_add / polar_store of vnd_polar.hpp, which both
// only call: polar_tree below is the tree of those kernels written out again, so their generated code cannot change.
//
// polar_voice_chunk_kernel, grid (slots, G = ceil(M / 512) + 1), the SLOT the fast dimension as in voice_stream_kernel:
// workgroup j of slot b takes chunk c = floor(p / 512) + j.  It reads count, flags and position once, workgroup-uniform,
// leaves before any barrier if the slot is idle or bad or its chunk has no frame below p + n, forms the chunk's partial
// in the one-shot order and writes it to partials[b][j].  The workgroup of the chunk that stays incomplete also keeps that
// chunk's frames of this call in the ring (those below p are there already); a call with END keeps nothing.
// j <= floor((p + n - 1) / 512) - floor(p / 512) <= floor((510 + M) / 512) = G - 1: every chunk a call can touch has a
// workgroup (p mod 512 = 511 with n = M touches G of them).
//
// polar_voice_finish_kernel, grid (slots), follows on the same stream; the kernel boundary is the ordering between every
// workgroup's read of pos[b] and its update, and between the partials' writes and reads (vnd_voice_core.hpp).  Lane t
// starts from sums[b][t] if t < floor(p / 512) - the lane has a completed chunk of THIS voice - and from +0.0 otherwise,
// which is why the sums need no clearing at START; adds this call's completed chunks c = t (mod 256) in ascending c (with
// M > 131072 a lane gets two in one call); stores the sums back unless END; adds the incomplete chunk's partial to its
// lane - the largest c of that lane; runs the tree and writes moments[b], valid[b] and pos[b].
//
// Ring.  cap = 511 + M, ring slot = absolute frame mod cap.  Frames read lie in [p - 511, p) (the incomplete chunk's
// frames before this call), frames written in [p, p + n): a written g and a read f have 0 < g - f <= 510 + n < cap, so they
// never share a slot although the slot's workgroups are unordered.  A frame f of the incomplete chunk is overwritten only
// by frame f + cap, which lies past that chunk's end.  512 slots would not do: a call that completes chunk c0 and starts
// c0 + 1 writes frame 512 (c0 + 1) + i over frame 512 c0 + i, which the workgroup of chunk c0 may still be reading.
//
// Every index that is built from device data:
//   - counts[b] outside [0, M], or pos[b] outside [0, 2^60] without START: the span is not ok and both kernels leave
//     before anything is addressed with it (the finish kernel writes valid[b] = -1 only) - so 0 <= p <= 2^60, 0 <= n <= M;
//   - block frames: f - p with p <= f < p + n, so [0, n) of row b;
//   - ring slots: (512 c) mod cap in [0, cap) plus a lane offset <= 511 < cap, one wrap;
//   - partials: j < G in the chunk kernel (the grid), and in the finish kernel j <= G - 1 by the bound above.
#pragma once
#include "../../include/vnd_polar_voice_stream.h"

constexpr int kPolarVoiceLanes = 256;                 // reduce lanes = threads of both kernels = kMomThreads
constexpr int64_t kPolarVoiceChunk = 512;             // kMomFrames
static_assert(kPolarVoiceLanes == vnd::kMomThreads && kPolarVoiceChunk == vnd::kMomFrames, "the one-shot order");

// One slot's side of a call, from the stored position, counts[b] and flags[b] alone.
struct PolarVoiceSpan : vnd::VoiceHead {
    int64_t q;                     // p + n
    int32_t valid;                 // 1 answered, 0 idle (p = q = 0, the position stays), -1 a bad count or position
};

__host__ __device__ inline PolarVoiceSpan polar_voice_span(int64_t stored, int32_t count, int32_t flags, int64_t M)
{
    PolarVoiceSpan v{vnd::voice_head(stored, count, flags, M)};
    if (!v.ok) { v.valid = -1; return v; }
    v.q = v.p + v.n;
    if (count == 0 && !(flags & (VND_VOICE_START | VND_VOICE_END))) { v.p = v.q = 0; return v; }      // idle: next is stored
    v.valid = 1;
    return v;
}

// Whether frames [0, q) end in a chunk that is not complete - the one-shot call's last chunk when it is short; q = 0 is
// its one chunk of zeros.
__host__ __device__ inline bool polar_voice_open_chunk(int64_t q) { return (q & (kPolarVoiceChunk - 1)) != 0 || q == 0; }

template <class T> struct PolarVoiceKind;
template <> struct PolarVoiceKind<float> {
    using Acc = vnd::PolarAcc;
    using Pair = float2;
    __device__ static __forceinline__ void add(Acc &a, float l, float r) { vnd::polar_add(a, l, r); }
    __device__ static __forceinline__ void values(double *v, const Acc &a) { vnd::polar_store(v, a); }
    __device__ static __forceinline__ Pair pair(float l, float r) { return make_float2(l, r); }
};
template <> struct PolarVoiceKind<double> {
    using Acc = vnd::PolarAcc64;
    using Pair = double2;
    __device__ static __forceinline__ void add(Acc &a, double l, double r) { vnd::polar_add64(a, l, r); }
    __device__ static __forceinline__ void values(double *v, const Acc &a) { vnd::polar_values64(v, a); }
    __device__ static __forceinline__ Pair pair(double l, double r) { return make_double2(l, r); }
};

template <class T>
struct PolarVoiceArgs {
    const T *__restrict__ l;          // the chunk: frame t of slot b at b * stream_stride + t * frame_stride
    const T *__restrict__ r;
    typename PolarVoiceKind<T>::Pair *__restrict__ ring;      // [slots][cap]
    double *__restrict__ sums;        // [slots][256][8]
    double *__restrict__ partials;    // [slots][G][8]
    int64_t *__restrict__ pos;        // [slots]
    const int32_t *__restrict__ counts;
    const int32_t *__restrict__ flags;
    double *__restrict__ moments;     // [slots][8]
    int32_t *__restrict__ valid;      // [slots]
    int64_t M, cap, G, stream_stride;
    int32_t frame_stride;
};

// The tree of moments_by_frame_kernel and moments_reduce_kernel: 32..1 per wave, then the four waves in order; lanes 0..7
// of the workgroup return moment k = threadIdx.x in t.  Every lane of the workgroup calls it.
__device__ __forceinline__ bool polar_tree(double (&v)[vnd::kMoments], double (*red)[vnd::kMoments], double &t)
{
#pragma unroll
    for (int k = 0; k < vnd::kMoments; ++k) {
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1) {
            const double o = __shfl_xor(v[k], sh);
            v[k] = k == 4 ? fmax(v[k], o) : v[k] + o;
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < vnd::kMoments; ++k) red[threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x >= vnd::kMoments) return false;
    const int k = threadIdx.x;
    t = red[0][k];
    for (int w = 1; w < kPolarVoiceLanes / 64; ++w) t = k == 4 ? fmax(t, red[w][k]) : t + red[w][k];   // fixed order
    return true;
}

// grid = (slots, G)
template <class T>
__global__ __launch_bounds__(kPolarVoiceLanes) void polar_voice_chunk_kernel(const PolarVoiceArgs<T> a)
{
    using K = PolarVoiceKind<T>;
    __shared__ double red[kPolarVoiceLanes / 64][vnd::kMoments];
    const int64_t b = blockIdx.x, j = blockIdx.y;
    const PolarVoiceSpan s = polar_voice_span(vnd::uniform_i64(a.pos[b]), __builtin_amdgcn_readfirstlane(a.counts[b]),
                                              __builtin_amdgcn_readfirstlane(a.flags[b]), a.M);
    if (s.valid != 1) return;                                     // idle or bad: nothing is addressed with the values
    const int64_t c = s.p / kPolarVoiceChunk + j, f0 = c * kPolarVoiceChunk;
    if (f0 >= s.q && !(s.q == 0 && j == 0)) return;               // no frame of the voice in this chunk (workgroup-uniform)
    // the chunk stays incomplete and the voice goes on: its frames of this call are kept
    const bool keep = !s.end && f0 + kPolarVoiceChunk > s.q;
    const T *__restrict__ pl = a.l + b * a.stream_stride;
    const T *__restrict__ pr = a.r + b * a.stream_stride;
    typename K::Pair *__restrict__ ring = a.ring + b * a.cap;
    const int64_t slot0 = f0 % a.cap;                             // uniform
    typename K::Acc acc;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int off = h * kPolarVoiceLanes + (int)threadIdx.x;
        const int64_t f = f0 + off;
        if (f >= s.q) continue;
        int64_t slot = slot0 + off;
        if (slot >= a.cap) slot -= a.cap;
        if (f >= s.p) {
            const int64_t i = (f - s.p) * a.frame_stride;
            const T l = pl[i], r = pr[i];
            if (keep) ring[slot] = K::pair(l, r);
            K::add(acc, l, r);
        } else {
            const typename K::Pair v = ring[slot];
            K::add(acc, v.x, v.y);
        }
    }
    double v[vnd::kMoments], t;
    K::values(v, acc);
    if (polar_tree(v, red, t)) a.partials[(b * a.G + j) * vnd::kMoments + threadIdx.x] = t;
}

// grid = slots: behind polar_voice_chunk_kernel on the same stream
template <class T>
__global__ __launch_bounds__(kPolarVoiceLanes) void polar_voice_finish_kernel(const PolarVoiceArgs<T> a)
{
    __shared__ double red[kPolarVoiceLanes / 64][vnd::kMoments];
    const int64_t b = blockIdx.x;
    const int lane = threadIdx.x;
    const PolarVoiceSpan s = polar_voice_span(vnd::uniform_i64(a.pos[b]), __builtin_amdgcn_readfirstlane(a.counts[b]),
                                              __builtin_amdgcn_readfirstlane(a.flags[b]), a.M);
    if (s.valid != 1) {                                           // (workgroup-uniform, before any barrier)
        if (lane == 0) a.valid[b] = s.valid;
        return;
    }
    const int64_t c0 = s.p / kPolarVoiceChunk, cq = s.q / kPolarVoiceChunk, done = cq - c0;     // done <= G - 1
    double *__restrict__ sum = a.sums + (b * kPolarVoiceLanes + lane) * vnd::kMoments;
    const double *__restrict__ part = a.partials + b * a.G * vnd::kMoments;
    double v[vnd::kMoments];
#pragma unroll
    for (int k = 0; k < vnd::kMoments; ++k) v[k] = lane < c0 ? sum[k] : 0.0;
    const int64_t j0 = (lane - (int)(c0 & (kPolarVoiceLanes - 1))) & (kPolarVoiceLanes - 1);      // c0 + j0 = lane (mod 256)
    for (int64_t j = j0; j < done; j += kPolarVoiceLanes) {
        const double *p = part + j * vnd::kMoments;
#pragma unroll
        for (int k = 0; k < vnd::kMoments; ++k) v[k] = k == 4 ? fmax(v[k], p[k]) : v[k] + p[k];
    }
    if (!s.end && j0 < done) {
#pragma unroll
        for (int k = 0; k < vnd::kMoments; ++k) sum[k] = v[k];
    }
    if (polar_voice_open_chunk(s.q) && lane == (int)(cq & (kPolarVoiceLanes - 1))) {
        const double *p = part + done * vnd::kMoments;
#pragma unroll
        for (int k = 0; k < vnd::kMoments; ++k) v[k] = k == 4 ? fmax(v[k], p[k]) : v[k] + p[k];
    }
    double t;
    if (polar_tree(v, red, t)) a.moments[b * vnd::kMoments + lane] = t;
    if (lane == 0) {
        a.valid[b] = 1;
        a.pos[b] = s.next;
    }
}

// The fixed launch of a pool, and where the parts of its state begin.
struct PolarVoicePlan {
    int64_t G, workgroups, finish_groups, cap, need;
    int64_t sums_at, partials_at, ring_at;
};

// The scalar side of the pool's checks, in the order the entries report them.
static vnd_status polar_voice_plan(int64_t slots, int64_t max_frames_per_call, int32_t sample_bytes, PolarVoicePlan *plan)
{
    if (slots < 1 || max_frames_per_call < 1) return fail(VND_ERR_INVALID, "slots and max_frames_per_call must be >= 1");
    if (max_frames_per_call > INT32_MAX)
        return fail(VND_ERR_INVALID, "max_frames_per_call %lld above INT32_MAX: counts are int32", (long long)max_frames_per_call);
    if (sample_bytes != 4 && sample_bytes != 8)
        return fail(VND_ERR_INVALID, "sample_bytes %d: 4 (float32) or 8 (float64)", sample_bytes);
    if (slots > VND_MAX_STREAMS) return fail(VND_ERR_UNSUPPORTED, "slots %lld above %d: split the pool", (long long)slots, VND_MAX_STREAMS);
    PolarVoicePlan p{};
    p.G = (max_frames_per_call + kPolarVoiceChunk - 1) / kPolarVoiceChunk + 1;
    p.cap = max_frames_per_call + kPolarVoiceChunk - 1;
    p.workgroups = slots * p.G;
    p.finish_groups = slots;
    if (p.G > 65535)
        return fail(VND_ERR_UNSUPPORTED, "%lld chunk workgroups per slot, above the 65535 of a grid dimension", (long long)p.G);
    if (p.workgroups > ((int64_t)1 << 23))
        return fail(VND_ERR_UNSUPPORTED, "%lld workgroups in one launch, above 2^23", (long long)p.workgroups);
    // slots <= 65535, G < 2^16, cap < 2^32: every product below fits int64
    p.sums_at = voice_position_bytes(slots);
    p.partials_at = p.sums_at + slots * kPolarVoiceLanes * vnd::kMoments * (int64_t)sizeof(double);
    p.ring_at = p.partials_at + slots * p.G * vnd::kMoments * (int64_t)sizeof(double);
    p.need = p.ring_at + slots * p.cap * 2 * (int64_t)sample_bytes;
    *plan = p;
    return VND_OK;
}

template <class T>
static vnd_status polar_voice_stream_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t max_frames_per_call, const T *l,
                                         const T *r, int64_t stream_stride, int32_t frame_stride, const int32_t *counts,
                                         const int32_t *flags, double *moments, int32_t *valid, int64_t slots, void *stream_)
{
    if (!ctx) return fail(VND_ERR_INVALID, "null context");
    if (stream_stride < 1 || frame_stride < 1) return fail(VND_ERR_INVALID, "strides must be >= 1");
    PolarVoicePlan p{};
    vnd_status st = polar_voice_plan(slots, max_frames_per_call, (int32_t)sizeof(T), &p);
    if (st != VND_OK) return st;
    if ((st = voice_state_check("voice pool", state, state_bytes, p.need, slots)) != VND_OK) return st;
    if (!l || !r || !counts || !flags || !moments || !valid)
        return fail(VND_ERR_INVALID, "null chunk, counts, flags, moments or valid pointer");
    int64_t xb = 0;
    if ((st = voice_chunk_bytes(slots, stream_stride, max_frames_per_call, frame_stride, sizeof(T), &xb)) != VND_OK) return st;
    const int64_t mb = slots * vnd::kMoments * (int64_t)sizeof(double), vb = slots * (int64_t)sizeof(int32_t);
    for (const T *c : {l, r})
        if (voice_overlap(c, xb, moments, mb) || voice_overlap(c, xb, valid, vb) || voice_overlap(c, xb, state, p.need))
            return fail(VND_ERR_INVALID, "moments, valid and the state must not overlap the chunk");
    if (voice_overlap(moments, mb, state, p.need) || voice_overlap(valid, vb, state, p.need) ||
        voice_overlap(moments, mb, valid, vb))
        return fail(VND_ERR_INVALID, "moments, valid and the state must not overlap one another");
    DeviceScope on(ctx->device);
    if (!on.ok) return fail(VND_ERR_HIP, "cannot select device %d", ctx->device);
    hipStream_t stream = (hipStream_t)stream_;

    PolarVoiceArgs<T> a{};
    a.l = l; a.r = r; a.counts = counts; a.flags = flags; a.moments = moments; a.valid = valid;
    a.pos = (int64_t *)state;
    a.sums = (double *)((char *)state + p.sums_at);
    a.partials = (double *)((char *)state + p.partials_at);
    a.ring = (typename PolarVoiceKind<T>::Pair *)((char *)state + p.ring_at);
    a.M = max_frames_per_call; a.cap = p.cap; a.G = p.G; a.stream_stride = stream_stride;
    a.frame_stride = frame_stride;
    hipLaunchKernelGGL(polar_voice_chunk_kernel<T>, dim3((unsigned)slots, (unsigned)p.G), dim3(kPolarVoiceLanes), 0, stream, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(polar_voice_finish_kernel<T>, dim3((unsigned)slots), dim3(kPolarVoiceLanes), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return VND_OK;
}

extern "C" {

vnd_status vnd_polar_voice_stream_state_bytes(int64_t slots, int64_t max_frames_per_call, int32_t sample_bytes, int64_t *bytes)
{
    if (!bytes) return fail(VND_ERR_INVALID, "null bytes");
    *bytes = 0;
    PolarVoicePlan p{};
    vnd_status st = polar_voice_plan(slots, max_frames_per_call, sample_bytes, &p);
    if (st != VND_OK) return st;
    *bytes = p.need;
    return VND_OK;
}

vnd_status vnd_polar_voice_stream_reset_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t slots,
                                            int64_t max_frames_per_call, int32_t sample_bytes, void *stream_)
{
    if (!ctx) return fail(VND_ERR_INVALID, "null context");
    PolarVoicePlan p{};
    vnd_status st = polar_voice_plan(slots, max_frames_per_call, sample_bytes, &p);
    if (st != VND_OK) return st;
    if ((st = voice_state_check("voice pool", state, state_bytes, p.need, slots)) != VND_OK) return st;
    return voice_reset_positions(ctx, state, slots, stream_);
}

vnd_status vnd_polar_voice_stream_f32_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t max_frames_per_call,
                                          const float *l, const float *r, int64_t stream_stride, int32_t frame_stride,
                                          const int32_t *counts, const int32_t *flags, double *moments, int32_t *valid,
                                          int64_t slots, void *stream)
{
    return polar_voice_stream_dev<float>(ctx, state, state_bytes, max_frames_per_call, l, r, stream_stride, frame_stride, counts,
                                         flags, moments, valid, slots, stream);
}

vnd_status vnd_polar_voice_stream_f64_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t max_frames_per_call,
                                          const double *l, const double *r, int64_t stream_stride, int32_t frame_stride,
                                          const int32_t *counts, const int32_t *flags, double *moments, int32_t *valid,
                                          int64_t slots, void *stream)
{
    return polar_voice_stream_dev<double>(ctx, state, state_bytes, max_frames_per_call, l, r, stream_stride, frame_stride, counts,
                                          flags, moments, valid, slots, stream);
}

}  // extern "C"
