// vnd_voice_core.hpp - what the ten voice pools share (vnd_voice_stream.hpp, vnd_voice_fade_stream.hpp, vnd_haas_voice_stream.hpp,
// vnd_haas_voice_fade_stream.hpp, vnd_correlogram_voice_stream.hpp, vnd_polar_voice_stream.hpp, vnd_spectrum_voice_stream.hpp, vnd_scope_voice_stream.hpp,
// vnd_level_voice_stream.hpp, vnd_haas_scan_voice_stream.hpp): the slot rule, the head of the state, the checks of the state and
// of strided chunks, the reset, and the kernel that moves the positions on.  (vnd_voice_window.hpp: what the last three share beyond it.)
// (one translation unit: included by vnd_voice_stream.hpp, after vnd_objects.hpp's fail / DeviceScope / HIP_TRY)
//
// THE SLOT RULE.  A pool's state begins with one int64 position per slot; a call brings a count and START / END flags per
// slot and is a pure function of device memory.  voice_head forms p = START ? 0 : stored.  A count outside [0, M], or a p
// outside [0, 2^60] (a state that was never reset), makes the slot BAD: nothing is addressed with its values, its position
// stays as stored and it answers -1.  Otherwise the call pushes n = count frames at p and the position becomes END ? 0 :
// p + n.  2^60 leaves every sum of a position, a count and a pool size far inside int64.  Each pool adds its own part -
// what comes out, its own bad and idle cases - in its span function, which host and device both call.  cg_voice_span and
// polar_voice_span start from voice_head; voice_span, and haas_voice_span and haas_voice_fade_span on top of it, write the
// same rule out in their own text (vnd_voice_stream.hpp says why).
//
// ORDERING.  Every workgroup of the compute kernel reads pos[b]; within one kernel the workgroups of a slot are not ordered,
// and the last one out would have to be found with an atomic.  So a second, small kernel follows on the same stream and
// writes pos[b] and the slot's answer: the kernel boundary is the ordering between every read of pos[b] and its update.
#pragma once
#include "../../include/vnd_voice_stream.h"

namespace vnd {

constexpr int64_t kVoiceMaxPosition = (int64_t)1 << 60;
constexpr int kVoiceAdvanceThreads = 256;

struct VoiceHead {
    int64_t p, n;                  // position the call starts at, frames pushed
    int64_t next;                  // the position after the call
    bool start, end, ok;           // !ok: a bad count or position - p = n = 0 and next is the stored position
};

__host__ __device__ inline VoiceHead voice_head(int64_t stored, int32_t count, int32_t flags, int64_t M)
{
    VoiceHead h{};
    h.start = (flags & VND_VOICE_START) != 0;
    h.end = (flags & VND_VOICE_END) != 0;
    h.p = h.start ? 0 : stored;
    h.ok = count >= 0 && count <= M && h.p >= 0 && h.p <= kVoiceMaxPosition;
    if (!h.ok) { h.p = 0; h.next = stored; return h; }
    h.n = count;
    h.next = h.end ? 0 : h.p + h.n;
    return h;
}

__device__ __forceinline__ int64_t uniform_i64(int64_t v)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

struct VoiceAnswer {
    int32_t answer;                // what out_counts[b] gets
    bool ok;                       // the position moves
    int64_t next;
};

// grid = ceil(slots / kVoiceAdvanceThreads), one lane per slot: behind the pool's compute kernel on the same stream.
// Args has pos, out_counts, slots and advance(b), the slot's span as a VoiceAnswer.
template <class Args>
__global__ __launch_bounds__(kVoiceAdvanceThreads) void voice_advance_kernel(const Args a)
{
    const int64_t b = (int64_t)blockIdx.x * kVoiceAdvanceThreads + threadIdx.x;
    if (b >= a.slots) return;
    const VoiceAnswer v = a.advance(b);
    a.out_counts[b] = v.answer;
    if (v.ok) a.pos[b] = v.next;
}

// The grid of voice_advance_kernel: the launch's, and what the describe_* entries report.
static int64_t voice_advance_groups(int64_t slots) { return (slots + kVoiceAdvanceThreads - 1) / kVoiceAdvanceThreads; }

template <class Args>
static void launch_voice_advance(const Args &a, int64_t slots, hipStream_t stream)
{
    const unsigned groups = (unsigned)voice_advance_groups(slots);
    hipLaunchKernelGGL(voice_advance_kernel<Args>, dim3(groups), dim3(kVoiceAdvanceThreads), 0, stream, a);
}

}  // namespace vnd

// The positions come first in the state, padded to 16 bytes; the pool's own part follows.
static int64_t voice_position_bytes(int64_t slots) { return (slots * (int64_t)sizeof(int64_t) + 15) & ~(int64_t)15; }

// The caller's state against the bytes the pool needs; `pool` is the pool's name in the first message.
static vnd_status voice_state_check(const char *pool, const void *state, int64_t state_bytes, int64_t need, int64_t slots)
{
    if (state_bytes < need)
        return fail(VND_ERR_INVALID, "state of %lld bytes, the %s needs %lld", (long long)state_bytes, pool, (long long)need);
    if (slots > 0 && !state) return fail(VND_ERR_INVALID, "null state pointer");
    if ((uintptr_t)state % 16 != 0) return fail(VND_ERR_INVALID, "the state is not 16-byte aligned");
    return VND_OK;
}

// What a reset does once the pool is checked: the positions to 0, nothing else of the state.
static vnd_status voice_reset_positions(const vnd_ctx *ctx, void *state, int64_t slots, void *stream_)
{
    DeviceScope on(ctx->device);
    if (!on.ok) return fail(VND_ERR_HIP, "cannot select device %d", ctx->device);
    HIP_TRY(hipMemsetAsync(state, 0, (size_t)voice_position_bytes(slots), (hipStream_t)stream_));
    return VND_OK;
}

// *bytes: from a strided chunk's first sample to the end of the last sample of the last slot's longest chunk.
static vnd_status voice_chunk_bytes(int64_t slots, int64_t stream_stride, int64_t max_frames_per_call, int32_t frame_stride,
                                    int64_t sample_bytes, int64_t *bytes)
{
    int64_t span, last;
    if (__builtin_mul_overflow(slots - 1, stream_stride, &span) ||
        __builtin_mul_overflow(max_frames_per_call - 1, (int64_t)frame_stride, &last) ||
        __builtin_add_overflow(span, last, &span) || span > INT64_MAX / 16)
        return fail(VND_ERR_INVALID, "buffer extents overflow");
    *bytes = (span + 1) * sample_bytes;
    return VND_OK;
}

static bool voice_overlap(const void *u, int64_t ub, const void *v, int64_t vb)
{
    const char *u0 = (const char *)u, *v0 = (const char *)v;
    return u0 < v0 + vb && v0 < u0 + ub;
}
