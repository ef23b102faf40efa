// vnd_stream.hpp - chunked streaming of the velvet-noise tap sum (include/vnd_stream.h), and the ring every block stream
// of float32 frames keeps its history in (RingArgs, ring_plan, ring_write: the velvet streams here and in
// vnd_each_stream.hpp, the Haas streams in vnd_haas_stream.hpp).
//
// The tap sum is anti-causal, y[n] = sum_k w[c,k] * x[n + i[c,k]], so output frame n is final once input frame n + H has
// arrived (H = the table's largest tap index).  A pool of streams advances in lockstep; a call pushes n_in frames per stream
// at absolute position pos and writes outputs [E, E') of every stream:
//     E  = max(0, pos - H)
//     E' = final ? pos + n_in : max(0, pos + n_in - H)
// It reads the virtual input x[E .. E' + H) clipped to [0, pos + n_in): frames below pos from the stream's ring, frames
// from pos on from the caller's chunk, frames past the end as 0 - what the one-shot kernels' range-checked loads read
// there.  The same launch copies the chunk's last min(n_in, H) frames into the ring (the ring contract: RingArgs below).
//
// Compute and store are the one-shot kernels' (vnd_kernels.hpp), called unchanged: ordered_tap / ordered_consume for the exact
// and fma modes, run_tap_array (even / odd chains) for the fast mode, epi_pointwise for the side-channel encode and the width,
// store_result, the pass-through of chan_flags.  Only the staging is new.  Per output the exact and fma modes do the same
// operations in the same order as the one-shot call, so the concatenated outputs are bit-identical to it; the fast mode's
// even / odd chains follow the tile's parity, which here starts at E, so it is within the fast mode's tolerance instead.
#pragma once
#include "../../include/vnd_stream.h"

namespace vnd {

// THE RING.  A stream's history lives in a per-stream ring in device memory, owned by the caller: `cap` frames of Cx
// float32 samples, slot = absolute frame mod cap.  `reach` is how far below pos a call may read: the table's largest tap
// index H (velvet), the delay d (Haas) or the pool's max_delay (a delay per stream).  The contract, for every user:
//   - capacity: cap >= reach + max_frames_per_call (and n_in <= max_frames_per_call is checked before every launch);
//   - a call reads ring frames in [pos - reach, pos) only, never a frame below 0 (so the ring needs no clearing);
//   - the same launch writes the chunk's last min(n_in, reach) frames [wr_first, pos + n_in) - none after the final
//     call, none with reach = 0 - each stream's workgroups sharing them in grid-stride order (ring_write);
//   - so a frame f read and a frame g written in one call have 0 < g - f <= reach + n_in - 1 < cap: they never share a
//     slot, NO SLOT IS BOTH READ AND WRITTEN IN ONE CALL, no ordering between a call's workgroups is needed, and every
//     frame is written exactly once.
// The host computes the slots (ring_plan): no lane divides.
struct RingArgs {
    const float *__restrict__ chunk;   // [batch][n_in][Cx]
    float *__restrict__ ring;          // [batch][cap][Cx]
    int64_t pos, n_in;
    int64_t cap;                       // ring capacity, frames
    int64_t wr_first, wr_count, wr_slot0;   // chunk frames [wr_first, wr_first + wr_count) (absolute) go to the ring, from slot wr_slot0
    int32_t Cx;
};

// The chunk frames later calls need, into the ring; `worker` of a stream's `workers` workgroups of NT lanes.
template <int NT>
__device__ __forceinline__ void ring_write(const RingArgs &r, int64_t stream, int64_t worker, int64_t workers, int tid)
{
    const int Cx = r.Cx;
    const int64_t total = r.wr_count * Cx;
    if (total <= 0) return;
    const int64_t capf = r.cap * Cx;
    const float *__restrict__ src = r.chunk + (stream * r.n_in + (r.wr_first - r.pos)) * Cx;
    float *__restrict__ dst = r.ring + stream * capf;
    const int64_t s0 = r.wr_slot0 * Cx;
    for (int64_t e = worker * NT + tid; e < total; e += workers * NT) {
        int64_t s = s0 + e;
        if (s >= capf) s -= capf;
        dst[s] = src[e];
    }
}

struct StreamArgs {
    KArgs k;                       // k.n = output frames per stream of this call, k.Cx = r.Cx
    RingArgs r;
    int64_t first_out;             // E
    int32_t direct_epi;            // direct variant: one lane per frame, both channels, pointwise epilogue
};

// One source frame of the virtual input: the ring below pos, the chunk up to pos + n_in, 0 past it.
__device__ __forceinline__ float stream_sample(const RingArgs &a, int64_t stream, int64_t f, int64_t ring_slot, int ch)
{
    const int Cx = a.Cx;
    if (f < a.pos) return a.ring[(stream * a.cap + ring_slot) * Cx + ch];
    if (f < a.pos + a.n_in) return a.chunk[(stream * a.n_in + (f - a.pos)) * Cx + ch];
    return 0.0f;
}

// The window [base, base + W) of PG input channels from cx0 on, into per-channel LDS planes.  Consecutive lanes take
// consecutive (frame, channel) samples, so both sources are read on consecutive addresses; kStageDepth loads in flight.
template <int NT, int PG>
__device__ __forceinline__ void stream_stage(const RingArgs &a, float *plane, int64_t stream, int64_t base, int cx0,
                                             int W, int tid)
{
    const int64_t slot0 = base % a.cap;            // only frames below pos are read from the ring: they lie within H of base
    const int total = W * PG;
    for (int e0 = tid; e0 < total; e0 += NT * kStageDepth) {
        float v[kStageDepth];
        int e[kStageDepth];
#pragma unroll
        for (int u = 0; u < kStageDepth; ++u) {
            e[u] = e0 + u * NT;
            v[u] = 0.0f;
            if (e[u] < total) {
                const int f = e[u] / PG, c = e[u] - (e[u] / PG) * PG;
                int64_t slot = slot0 + f;
                if (slot >= a.cap) slot -= a.cap;
                v[u] = stream_sample(a, stream, base + f, slot, cx0 + c);
            }
        }
#pragma unroll
        for (int u = 0; u < kStageDepth; ++u) {
            if (e[u] < total) {
                const int f = e[u] / PG, c = e[u] - (e[u] / PG) * PG;
                plane[c * W + f] = v[u];
            }
        }
    }
}

// MODE 0 / 1: the ordered kernel's tap loop (VND_MODE_EXACT / VND_MODE_FMA arithmetic); MODE 2: the fast kernel's even / odd
// chains.  BC: a mono chunk fanned out (one plane for both output channels).  The pointwise epilogue is a runtime switch
// (k.epi_ms_encode / k.epi_use_width, stereo outputs only).  LDS: PG planes of W floats, then (MODE 2) the exchange buffer.
template <int NT, int CG, int R, int MODE, bool BC>
__global__ __launch_bounds__(NT) void conv_stream_kernel(const StreamArgs sa)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const KArgs &a = sa.k;
    constexpr int T = 2 * NT * R;
    constexpr int PG = BC ? 1 : CG;
    const int tid = threadIdx.x;
    const int W = a.W;
    const BlockCoord bc = decode_block(a);
    const int C = a.C, Cx = a.Cx;
    ring_write<NT>(sa.r, bc.stream, (int64_t)bc.tile * a.groups + bc.group, (int64_t)a.tiles * a.groups, tid);
    if (a.n == 0) return;                          // (a call that only fills the ring: one workgroup per stream)

    const int c0 = bc.group * CG;
    const int cx0 = BC ? 0 : (Cx == C ? c0 : c0 % Cx);
    const int64_t t0 = (int64_t)bc.tile * T;
    float *__restrict__ ys = a.y + bc.stream * a.n * C;
    const int64_t bytes_left = ((a.n - t0) * C - c0) * 4;
    stream_stage<NT, PG>(sa.r, lds, bc.stream, sa.first_out + t0, cx0, W, tid);
    __syncthreads();

    float v_out[R][2 * CG];                        // per j: frames 2q, 2q+1 of the CG channels
    if constexpr (MODE == 2) {
        float2 accE[CG][R], accO[CG][R];
        float edge[CG];
        const int lane = tid & 63;
#pragma unroll
        for (int c = 0; c < CG; ++c) {
            const int ch = c0 + c;
            const float *pc = lds + (BC ? 0 : c * W);
            const float *pa = pc + 2 * tid;
            edge[c] = 0.0f;
#pragma unroll
            for (int j = 0; j < R; ++j) { accE[c][j] = make_float2(0.0f, 0.0f); accO[c][j] = make_float2(0.0f, 0.0f); }
            if (a.chan_flags != nullptr && (a.chan_flags[ch] & 1)) {
#pragma unroll
                for (int j = 0; j < R; ++j) accE[c][j] = *(const float2 *)(pa + 2 * NT * j);
                continue;
            }
            const int first = __builtin_amdgcn_readfirstlane(a.fast_off[ch]);
            const FastTap *__restrict__ tp = a.taps_fast + first;
            const int n_all = __builtin_amdgcn_readfirstlane(a.fast_off[ch + 1]) - first;
            const int n_even = __builtin_amdgcn_readfirstlane(a.fast_even[ch]);
            const int n_odd = n_all - n_even;
            run_tap_array<NT, R>(tp, n_even, lds_addr(pa), accE[c]);
            run_tap_array<NT, R>(tp + n_even, n_odd, lds_addr(pa), accO[c]);
            if (tid >= NT - 64) {
                float part = 0.0f;
                for (int k = lane; k < n_odd; k += 64) {
                    const FastTap t = tp[n_even + k];
                    part = __builtin_fmaf(pc[T + (t.off >> 2)], t.w, part);
                }
#pragma unroll
                for (int sh = 32; sh > 0; sh >>= 1) part += __shfl_xor(part, sh);
                edge[c] = part;
            }
        }
        // exchange buffer behind the planes: the input stays readable for the epilogue
        float *xo = lds + PG * W;
        constexpr int XS = T / 2 + 1;
#pragma unroll
        for (int c = 0; c < CG; ++c) {
#pragma unroll
            for (int j = 0; j < R; ++j) xo[c * XS + tid + NT * j] = accO[c][j].x;
            if (tid == NT - 1) xo[c * XS + T / 2] = edge[c];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const int q = tid + NT * j;
#pragma unroll
            for (int c = 0; c < CG; ++c) {
                v_out[j][c] = accE[c][j].x + accO[c][j].y;
                v_out[j][CG + c] = accE[c][j].y + xo[c * XS + q + 1];
            }
        }
    } else {
        const bool has_seg = a.seg_off != nullptr;
#pragma unroll
        for (int c = 0; c < CG; ++c) {
            const int ch = c0 + c;
            const float *pa = lds + (BC ? 0 : c * W) + 2 * tid;
            v2f out[R];
            if (a.chan_flags != nullptr && (a.chan_flags[ch] & 1)) {
#pragma unroll
                for (int j = 0; j < R; ++j) out[j] = *(const v2f *)(pa + 2 * NT * j);
            } else {
#pragma unroll
                for (int j = 0; j < R; ++j) out[j] = v2f{0.0f, 0.0f};
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
                        load_taps16(a.taps_ord + k, t);
                        const int m = kend - k;
#pragma unroll
                        for (int i = 0; i < 16; ++i)
                            if (i < m) ordered_tap<NT, R, MODE>(t[i], lane_addr, sb);
                        k += m < 16 ? m : 16;
                    }
                    if (has_seg) {
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
#pragma unroll
            for (int j = 0; j < R; ++j) { v_out[j][c] = out[j].x; v_out[j][CG + c] = out[j].y; }
        }
    }

    float *dst = ys + t0 * C + c0;
    const v4i rdst = make_rsrc(dst, bytes_left);
    const int shape = access_shape<CG>(dst, C);
    const int strideG = C / CG;
    const bool epi = a.epi_ms_encode || a.epi_use_width;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int q = tid + NT * j;
        if constexpr (CG == 2) {
            if (epi) {
                const float2 x0 = *(const float2 *)(lds + 2 * q), x1 = *(const float2 *)(lds + (BC ? 0 : W) + 2 * q);
                const float xin[4] = {x0.x, x1.x, x0.y, x1.y};
                epi_pointwise(a, v_out[j], xin);
            }
        }
        store_result<CG>(rdst, shape, a.stream_out, q, strideG, C, v_out[j]);
    }
}

// Tables whose window does not fit a workgroup's LDS (or with non-finite weights, or indices past the LDS images): one lane per
// output (frame, channel) - or, with the pointwise epilogue, per frame and both channels - taps gathered from the two sources,
// table order and association as conv_direct_kernel, a term past the end of the signal dropped.
template <int MODE>
__device__ __forceinline__ float stream_direct_channel(const StreamArgs &sa, int64_t b, int64_t fo, int ch)
{
    const KArgs &a = sa.k;
    const int cx = ch % a.Cx;
    const int64_t end = sa.r.pos + sa.r.n_in;
    auto slot_of = [&](int64_t f) { return f % sa.r.cap; };
    if (a.chan_flags != nullptr && (a.chan_flags[ch] & 1)) return stream_sample(sa.r, b, fo, slot_of(fo), cx);
    const bool has_seg = a.seg_off != nullptr;
    int k = a.tap_off[ch];
    const int k_last = a.tap_off[ch + 1];
    const int s_begin = has_seg ? a.seg_off[ch] : 0;
    const int nseg = has_seg ? a.seg_off[ch + 1] - s_begin : 1;
    float out = 0.0f;
    for (int s = 0; s < nseg; ++s) {
        const int kend = has_seg ? a.seg_end[s_begin + s] : k_last;
        float sb = 0.0f;
        for (; k < kend; ++k) {
            const Tap tp = a.taps[k];
            const int64_t m = fo + tp.idx;
            if (m >= end) continue;                 // the term DROPS, as in the one-shot direct kernel
            sb = tap_op<MODE>(sb, stream_sample(sa.r, b, m, slot_of(m), cx), tp.w);
        }
        if (has_seg) {
            if (a.apply_gain) sb = sb * a.seg_gain[s_begin + s];
            out = out + sb;
        } else {
            out = sb;
        }
    }
    return out;
}

template <int MODE>
__global__ __launch_bounds__(kDirectThreads) void conv_stream_direct_kernel(const StreamArgs sa)
{
    const KArgs &a = sa.k;
    const int64_t batch = a.tiles;                 // tiles carries the batch here, as in conv_direct_kernel
    const int64_t per_block = (int64_t)gridDim.x / batch;     // the grid is a whole number of blocks per stream
    const int64_t b_ring = blockIdx.x / per_block;
    ring_write<kDirectThreads>(sa.r, b_ring, blockIdx.x - b_ring * per_block, per_block, threadIdx.x);
    const int lanes_per_frame = sa.direct_epi ? 1 : a.C;
    const int64_t per_stream = a.n * lanes_per_frame;
    const int64_t total = per_stream * batch;
    for (int64_t e = (int64_t)blockIdx.x * kDirectThreads + threadIdx.x; e < total;
         e += (int64_t)gridDim.x * kDirectThreads) {
        const int64_t b = e / per_stream;
        const int64_t r = e - b * per_stream;
        const int64_t n0 = r / lanes_per_frame;
        const int64_t fo = sa.first_out + n0;
        float *yf = a.y + (b * a.n + n0) * a.C;
        if (sa.direct_epi) {                       // stereo output, pointwise epilogue on the frame
            float v[4], xin[4];
            v[0] = v[2] = stream_direct_channel<MODE>(sa, b, fo, 0);
            v[1] = v[3] = stream_direct_channel<MODE>(sa, b, fo, 1);
            xin[0] = xin[2] = stream_sample(sa.r, b, fo, fo % sa.r.cap, 0);
            xin[1] = xin[3] = stream_sample(sa.r, b, fo, fo % sa.r.cap, a.Cx == 1 ? 0 : 1);
            epi_pointwise(a, v, xin);
            yf[0] = v[0]; yf[1] = v[1];
        } else {
            const int ch = (int)(r - n0 * a.C);
            yf[ch] = stream_direct_channel<MODE>(sa, b, fo, ch);
        }
    }
}

}  // namespace vnd

// ------------------------------------------------------------------------------
// C ABI (include/vnd_stream.h)
// ------------------------------------------------------------------------------
struct StreamPlan {
    bool direct = false;
    bool bc = false;                // a mono chunk fanned out: one staged plane per workgroup
    int cg = 1, r = 1;              // channels per workgroup, frame pairs per lane (tile = 2 * 256 * r frames)
    int W = 0;
    size_t lds_bytes = 0;
    int tiles = 1, groups = 1;
    uint32_t nblocks = 0;
};

typedef void (*stream_kern_t)(const StreamArgs);
constexpr int kStreamThreads = 256;

template <int CG, int MODE, bool BC>
static stream_kern_t stream_by_r(int r)
{
    switch (r) {
    case 1: return conv_stream_kernel<kStreamThreads, CG, 1, MODE, BC>;
    case 2: return conv_stream_kernel<kStreamThreads, CG, 2, MODE, BC>;
    case 4: return conv_stream_kernel<kStreamThreads, CG, 4, MODE, BC>;
    default: return nullptr;
    }
}

template <int MODE>
static stream_kern_t stream_by_cg(const StreamPlan &p)
{
    if (p.bc) return stream_by_r<2, MODE, true>(p.r);
    switch (p.cg) {
    case 1: return stream_by_r<1, MODE, false>(p.r);
    case 2: return stream_by_r<2, MODE, false>(p.r);
    default: return stream_by_r<4, MODE, false>(p.r);
    }
}

static stream_kern_t stream_kernel(const StreamPlan &p, int arithmetic)
{
    return arithmetic == VND_MODE_EXACT ? stream_by_cg<0>(p) : arithmetic == VND_MODE_FMA ? stream_by_cg<1>(p) : stream_by_cg<2>(p);
}

// planes of the window, then (fast mode) the exchange buffer [cg][T/2 + 1] behind them
static size_t stream_lds_need(int cg, int r, int max_index, bool bc, bool fast)
{
    const size_t T = (size_t)2 * kStreamThreads * r;
    const size_t planes = (size_t)(bc ? 1 : cg) * (T + halo_of(max_index));
    return (planes + (fast ? (((size_t)cg * (T / 2 + 1) + 3) & ~(size_t)3) : 0)) * sizeof(float);
}

static StreamPlan make_stream_plan(const vnd_ctx *ctx, const vnd_taps *t, int64_t batch, int64_t n_out, int C, int Cx,
                                   int mode, bool epi)
{
    StreamPlan p;
    const bool fast = mode == VND_MODE_FAST;
    const int cus = ctx->prop.multiProcessorCount > 0 ? ctx->prop.multiProcessorCount : 256;
    int cg = C % 2 == 0 ? 2 : 1;
    bool bc = false;
    if (Cx != C) {
        if (Cx == 1 && C % 2 == 0) bc = true;
        else if (Cx % cg != 0) cg = 1;
    }
    const size_t limit = (size_t)ctx->lds_limit - 1024;
    auto fits = [&](int r_) { return stream_lds_need(cg, r_, t->max_index, bc, fast) <= limit; };
    // the largest tile that still leaves every CU six workgroups (as make_plan), else the smallest
    int r = 1;
    for (int cand : {4, 2}) {
        const int64_t T = (int64_t)2 * kStreamThreads * cand;
        const int64_t blocks = batch * ((n_out + T - 1) / T) * (C / cg);
        if (blocks >= (int64_t)cus * 6 && stream_lds_need(cg, cand, t->max_index, bc, fast) <= limit / 4) { r = cand; break; }
    }
    bool direct = t->nonfinite || !t->lds_images;
    while (!direct && !fits(r)) {
        if (r > 1) { r /= 2; continue; }
        if (epi) { direct = true; break; }             // the pointwise epilogue needs both channels in one workgroup
        if (bc) { bc = false; cg = 1; continue; }
        if (cg > 1) { cg /= 2; continue; }
        direct = true;
    }
    if (direct) {
        p.direct = true;
        const int64_t lanes = std::max<int64_t>(1, n_out * (epi ? 1 : C));
        const int64_t per_stream = std::min<int64_t>((lanes + kDirectThreads - 1) / kDirectThreads,
                                                     std::max<int64_t>(1, (int64_t)cus * 32 / std::max<int64_t>(batch, 1)));
        p.nblocks = (uint32_t)(batch * std::max<int64_t>(per_stream, 1));
        return p;
    }
    const int64_t T = (int64_t)2 * kStreamThreads * r;
    p.bc = bc; p.cg = cg; p.r = r;
    p.W = (int)T + halo_of(t->max_index);
    p.lds_bytes = stream_lds_need(cg, r, t->max_index, bc, fast);
    p.tiles = (int)std::max<int64_t>(1, (n_out + T - 1) / T);          // (a call that only fills the ring: one tile)
    p.groups = C / cg;
    p.nblocks = (uint32_t)(batch * p.tiles * p.groups);
    return p;
}

// The ring side of a call (RingArgs above): which chunk frames go to the ring, and from which slot.  reach = 0 keeps nothing.
// On the host for the streams whose position the caller holds, on the device for the voice pool (vnd_voice_stream.hpp),
// whose positions live in the state: one 64-bit modulo per workgroup there.
static __host__ __device__ inline RingArgs ring_plan(int64_t pos, int64_t n_in, int64_t reach, bool final_, int64_t cap)
{
    RingArgs r{};
    r.pos = pos; r.n_in = n_in; r.cap = cap;
    // the last `reach` frames of the chunk are what later calls read (none after the final call)
    const int64_t kept = pos + n_in - reach;
    r.wr_first = (final_ || reach == 0) ? pos + n_in : (kept > pos ? kept : pos);
    r.wr_count = pos + n_in - r.wr_first;
    r.wr_slot0 = cap > 0 ? r.wr_first % cap : 0;
    return r;
}

// nothing to compute and nothing to keep: the call launches nothing
static bool ring_idle(const RingArgs &r, int64_t batch, int64_t n_out) { return batch == 0 || (n_out == 0 && r.wr_count == 0); }

// What every block stream checks of its position, frame count and state, in this order.
static vnd_status block_stream_check(int64_t pos, int64_t n_in, int64_t max_frames_per_call, int64_t state_bytes, int64_t need)
{
    if (pos < 0 || pos > ((int64_t)1 << 60)) return fail(VND_ERR_INVALID, "position %lld out of range", (long long)pos);
    if (n_in < 0) return fail(VND_ERR_INVALID, "negative frame count");
    if (n_in > max_frames_per_call)
        return fail(VND_ERR_INVALID, "%lld frames in one call, above max_frames_per_call %lld", (long long)n_in,
                    (long long)max_frames_per_call);
    if (state_bytes < need)
        return fail(VND_ERR_INVALID, "state of %lld bytes, the stream needs %lld", (long long)state_bytes, (long long)need);
    return VND_OK;
}

static int64_t stream_capacity(const vnd_taps *t, int64_t max_frames_per_call)
{
    return std::max<int64_t>(1, (int64_t)t->max_index + max_frames_per_call);
}

extern "C" {

vnd_status vnd_stream_state_bytes(const vnd_taps *t, int64_t batch, int32_t in_channels, int64_t max_frames_per_call,
                                  int64_t *bytes)
{
    if (!t || !bytes) return fail(VND_ERR_INVALID, "null tap table or bytes");
    *bytes = 0;
    if (batch < 0 || batch > VND_MAX_STREAMS) return fail(VND_ERR_INVALID, "batch %lld outside 0..%d", (long long)batch, VND_MAX_STREAMS);
    if (in_channels <= 0 || t->C % in_channels != 0)
        return fail(VND_ERR_INVALID, "%d input channels do not divide the tap table's %d channels", in_channels, t->C);
    if (max_frames_per_call < 0 || max_frames_per_call > ((int64_t)1 << 40))
        return fail(VND_ERR_INVALID, "max_frames_per_call %lld out of range", (long long)max_frames_per_call);
    *bytes = batch * stream_capacity(t, max_frames_per_call) * in_channels * (int64_t)sizeof(float);
    return VND_OK;
}

// Every argument check, before anything is enqueued; *n_out from position, n_in, H and final alone.
static vnd_status stream_check(vnd_ctx *ctx, const vnd_taps *t, const void *state, int64_t state_bytes,
                               int64_t max_frames_per_call, const float *x, const float *y, int64_t batch, int64_t pos,
                               int64_t n_in, int32_t Cx, int32_t final_, int32_t mode, int32_t ms_encode, int32_t use_width,
                               int64_t *n_out)
{
    if (!ctx || !t) return fail(VND_ERR_INVALID, "null context or tap table");
    if (!n_out) return fail(VND_ERR_INVALID, "null n_out");
    *n_out = 0;
    if (t->ctx != ctx && t->ctx->device != ctx->device)
        return fail(VND_ERR_INVALID, "the tap table lives on device %d, the context on device %d", t->ctx->device, ctx->device);
    int64_t need = 0;
    vnd_status st = vnd_stream_state_bytes(t, batch, Cx, max_frames_per_call, &need);
    if (st != VND_OK) return st;
    if (mode != VND_MODE_EXACT && mode != VND_MODE_FMA && mode != VND_MODE_FAST) return fail(VND_ERR_INVALID, "unknown mode %d", mode);
    if ((st = block_stream_check(pos, n_in, max_frames_per_call, state_bytes, need)) != VND_OK) return st;
    if ((ms_encode || use_width) && t->C != 2)
        return fail(VND_ERR_INVALID, "the side-channel encode and the width need 2 output channels, the table has %d", t->C);
    const int64_t H = t->max_index;
    const int64_t e0 = std::max<int64_t>(0, pos - H);
    const int64_t e1 = final_ ? pos + n_in : std::max<int64_t>(0, pos + n_in - H);
    if (batch > 0 && ((need > 0 && !state) || (n_in > 0 && !x) || (e1 > e0 && !y)))
        return fail(VND_ERR_INVALID, "null state, chunk or output pointer");
    if (batch * (e1 - e0) * t->C > ((int64_t)1 << 40)) return fail(VND_ERR_UNSUPPORTED, "problem too large");
    *n_out = e1 - e0;
    return VND_OK;
}

vnd_status vnd_stream_f32_dev(vnd_ctx *ctx, const vnd_taps *t, void *state, int64_t state_bytes, int64_t max_frames_per_call,
                              const float *x, float *y, int64_t batch, int64_t pos, int64_t n_in, int32_t Cx, int32_t final_,
                              int32_t mode, int32_t ms_encode, int32_t use_width, double width, int64_t *n_out,
                              void *stream_)
{
    vnd_status st = stream_check(ctx, t, state, state_bytes, max_frames_per_call, x, y, batch, pos, n_in, Cx, final_, mode,
                                 ms_encode, use_width, n_out);
    if (st != VND_OK) return st;
    const int64_t H = t->max_index, C = t->C, nout = *n_out;
    StreamArgs sa{};
    sa.r = ring_plan(pos, n_in, H, final_, stream_capacity(t, max_frames_per_call));
    sa.r.chunk = x; sa.r.ring = (float *)state; sa.r.Cx = Cx;
    sa.first_out = std::max<int64_t>(0, pos - H);
    if (ring_idle(sa.r, batch, nout)) return VND_OK;
    const bool epi = ms_encode || use_width;
    const StreamPlan p = make_stream_plan(ctx, t, batch, nout, (int)C, Cx, mode, epi);
    KArgs &a = sa.k;
    a.y = y; a.n = nout; a.C = (int32_t)C; a.Cx = Cx;
    table_args(a, t);
    a.epi_ms_encode = ms_encode ? 1 : 0; a.epi_use_width = use_width ? 1 : 0;
    a.epi_w_mid = (float)(1.0 - width); a.epi_w_side = (float)width;       // as the decorrelate stage passes the width
    a.nblocks = p.nblocks;
    DeviceScope on(ctx->device);
    if (!on.ok) return fail(VND_ERR_HIP, "cannot select device %d", ctx->device);
    hipStream_t stream = (hipStream_t)stream_;
    if (p.direct) {
        a.tiles = (int32_t)batch; a.groups = 1; a.W = 0;
        sa.direct_epi = epi ? 1 : 0;
        const int arith = arithmetic_of(t, mode);
        hipLaunchKernelGGL(arith == VND_MODE_EXACT ? conv_stream_direct_kernel<0> : conv_stream_direct_kernel<1>,
                           dim3(p.nblocks), dim3(kDirectThreads), 0, stream, sa);
    } else {
        if ((int64_t)batch * p.tiles * p.groups > 0x7fffffffLL) return fail(VND_ERR_UNSUPPORTED, "grid too large; split the batch");
        a.tiles = p.tiles; a.groups = p.groups; a.W = p.W;
        stream_kern_t k = stream_kernel(p, arithmetic_of(t, mode));
        if (!k) return fail(VND_ERR_UNSUPPORTED, "no stream kernel for this tile shape");
        if (st = allow_lds(ctx, (const void *)k, p.lds_bytes); st != VND_OK) return st;
        hipLaunchKernelGGL(k, dim3(p.nblocks), dim3(kStreamThreads), p.lds_bytes, stream, sa);
    }
    HIP_TRY(hipGetLastError());
    return VND_OK;
}

vnd_status vnd_stream_f32_host(vnd_ctx *ctx, const vnd_taps *t, void *state, int64_t state_bytes, int64_t max_frames_per_call,
                               const float *x, float *y, int64_t batch, int64_t pos, int64_t n_in, int32_t Cx, int32_t final_,
                               int32_t mode, int32_t ms_encode, int32_t use_width, double width, int64_t *n_out)
{
    vnd_status st = stream_check(ctx, t, state, state_bytes, max_frames_per_call, x, y, batch, pos, n_in, Cx, final_, mode,
                                 ms_encode, use_width, n_out);
    if (st != VND_OK) return st;
    const int64_t nout = *n_out;
    if (batch == 0 || (n_in == 0 && nout == 0)) return VND_OK;
    HostCall call(ctx);
    call.staged(x, (size_t)(batch * n_in * Cx) * sizeof(float), "the chunk", y, (size_t)(batch * nout * t->C) * sizeof(float),
                nullptr, 0, 0, n_out, [&](void *x_dev, void *y_dev, int32_t *, void *, hipStream_t s) {
        int64_t got = 0;
        return vnd_stream_f32_dev(ctx, t, state, state_bytes, max_frames_per_call, (const float *)x_dev, (float *)y_dev, batch, pos,
                                  n_in, Cx, final_, mode, ms_encode, use_width, width, &got, s);
    });
    return call.finish("vnd_stream_f32_host");
}

}  // extern "C"
