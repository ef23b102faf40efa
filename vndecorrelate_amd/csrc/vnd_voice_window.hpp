// vnd_voice_window.hpp - what the window pools share (vnd_scope_voice_stream.hpp, vnd_level_voice_stream.hpp,
// vnd_haas_scan_voice_stream.hpp): the slot rule, the walk of a workgroup over its frames and their ring entries, the scalar
// side of the plan and the radius_scale check.
// (one translation unit: included by vnd_amd.hip after vnd_scope.hpp and vnd_voice_core.hpp, before the pools' files)
//
// A window pool keeps, per slot, a ring of W entries behind the positions: entry g mod W belongs to the voice's frame g.  A
// call brings the frames [p, p + n) of each slot, n <= M, and a launch of grid (ceil(M / kScopeVoiceSpan), slots) with
// kScopeVoiceThreads threads walks them: workgroup x of slot b takes the chunk frames [j0, j1) = [x span, min(x span + span, n)),
// frame j of the chunk being the voice's frame g = p + j.
//
// Ring.  M <= W, so the frames [p, p + n) of one call have n <= W distinct residues mod W: every ring entry a call touches is
// read and written by the one lane that owns its frame, and no lane races another although the workgroups of a slot are
// unordered.  The ring is never cleared: each pool says in its own file which entries it may read (the scope pool entry
// g mod W only for g >= W, when frame g - W of THIS voice wrote it; the level pool the prefix its fill names; the Haas scan
// pool the fill entries that end before its head).
//
// Every index that is built from device data:
//   - counts[b] outside [0, M], or pos[b] outside [0, 2^60] without START: the span is not ok and every kernel leaves before
//     anything is addressed with it (the advance kernel writes valid[b] = -1 only) - so 0 <= p <= 2^60, 0 <= n <= M;
//   - chunk frames: j < n, so [0, n) of row b;
//   - ring entries: (p + j0) mod W in [0, W) plus a lane offset j - j0 < n <= W, one wrap.
#pragma once

constexpr int kScopeVoiceThreads = 256;
constexpr int64_t kScopeVoiceSpan = 1024;             // frames of one slot per workgroup of the walk

// One slot's side of a call, from the stored position, counts[b] and flags[b] alone.
struct ScopeVoiceSpan : vnd::VoiceHead {
    int32_t valid;                 // 1 answered, 0 idle (nothing is touched), -1 a bad count or position
    bool clear;                    // answered from position 0: a pool that keeps sums clears them first
};

__host__ __device__ inline ScopeVoiceSpan scope_voice_span(int64_t stored, int32_t count, int32_t flags, int64_t M)
{
    ScopeVoiceSpan v{vnd::voice_head(stored, count, flags, M)};
    if (!v.ok) { v.valid = -1; return v; }
    if (count == 0 && !v.start && !v.end) return v;               // idle: next is the stored position
    v.valid = 1;
    v.clear = v.p == 0;
    return v;
}

// The span of slot b as every lane of a workgroup sees it (workgroup-uniform).
__device__ __forceinline__ ScopeVoiceSpan scope_voice_view(const int64_t *pos, const int32_t *counts, const int32_t *flags, int64_t M,
                                                           int64_t b)
{
    return scope_voice_span(vnd::uniform_i64(pos[b]), __builtin_amdgcn_readfirstlane(counts[b]),
                            __builtin_amdgcn_readfirstlane(flags[b]), M);
}

// The walk of workgroup x of slot b.  open() is false for an idle slot, a bad slot and a workgroup past n: the workgroup leaves
// (workgroup-uniform, before any barrier), nothing is addressed with the values.  enter(W) finds where the chunk enters a ring
// of W > 0 entries; entry(j) is then the ring entry of chunk frame j in [j0, j1).
struct VoiceWindowWalk {
    ScopeVoiceSpan s;
    int64_t j0, j1, slot0, W;
    __device__ __forceinline__ bool open(const int64_t *pos, const int32_t *counts, const int32_t *flags, int64_t M, int64_t b,
                                         unsigned x)
    {
        s = scope_voice_view(pos, counts, flags, M, b);
        if (s.valid != 1) return false;
        j0 = (int64_t)x * kScopeVoiceSpan;
        j1 = j0 + kScopeVoiceSpan < s.n ? j0 + kScopeVoiceSpan : s.n;
        return j0 < s.n;
    }
    __device__ __forceinline__ void enter(int64_t window) { W = window; slot0 = (s.p + j0) % W; }       // uniform
    __device__ __forceinline__ int64_t entry(int64_t j) const
    {
        int64_t slot = slot0 + (j - j0);                          // j - j0 < n <= M <= W: one wrap
        if (slot >= W) slot -= W;
        return slot;
    }
};

// ---- the host side ---------------------------------------------------------------------------------------------------------
// The scalar side of a window pool's checks, in the order the entries report them; *groups: the workgroups of a slot's walk.
// whole_ok: window_frames = 0 is the pool's whole-voice form and not a refusal.
static vnd_status voice_window_plan(int64_t slots, int64_t max_frames_per_call, int64_t window_frames, bool whole_ok, int64_t *groups)
{
    if (slots < 1 || max_frames_per_call < 1) return fail(VND_ERR_INVALID, "slots and max_frames_per_call must be >= 1");
    if (max_frames_per_call > INT32_MAX)
        return fail(VND_ERR_INVALID, "max_frames_per_call %lld above INT32_MAX: counts are int32", (long long)max_frames_per_call);
    if (whole_ok && window_frames < 0) return fail(VND_ERR_INVALID, "window_frames %lld below 0", (long long)window_frames);
    if (!(whole_ok && window_frames == 0) && window_frames < max_frames_per_call)
        return fail(VND_ERR_INVALID, "window_frames %lld below max_frames_per_call %lld: two frames of one call would share a ring entry",
                    (long long)window_frames, (long long)max_frames_per_call);
    if (slots > VND_MAX_STREAMS) return fail(VND_ERR_UNSUPPORTED, "slots %lld above %d: split the pool", (long long)slots, VND_MAX_STREAMS);
    if (window_frames > INT32_MAX)
        return fail(VND_ERR_UNSUPPORTED, "window_frames %lld above INT32_MAX", (long long)window_frames);
    *groups = (max_frames_per_call + kScopeVoiceSpan - 1) / kScopeVoiceSpan;
    if (*groups * slots > kScopeMaxGroups)
        return fail(VND_ERR_UNSUPPORTED, "%lld workgroups in one launch, above 2^23: split the pool", (long long)(*groups * slots));
    return VND_OK;                 // slots < 2^16, W < 2^31: slots * W * (an entry of up to 8 bytes) fits int64
}

// A voice pool's radius_scale: fixed, positive, and neither zero nor infinite as a T.
template <class T>
static vnd_status voice_window_scale(double radius_scale)
{
    if (radius_scale != radius_scale) return fail(VND_ERR_INVALID, "radius_scale is NaN");
    if (!(radius_scale > 0.0))
        return fail(VND_ERR_INVALID, "radius_scale %g: a voice pool needs a fixed positive scale, the per-voice maximum of a "
                                     "later block would rescale the earlier frames", radius_scale);
    if (!(radius_scale <= (double)std::numeric_limits<T>::max() && (T)radius_scale > (T)0))
        return fail(VND_ERR_INVALID, "radius_scale %g is zero or infinite in the sample type", radius_scale);
    return VND_OK;
}
