R"VNDSPEC(
// vnd_spec_kernel - the fast-mode tap sum SPECIALISED for one tap table (gfx950, wave64).
//
// Compiled at run time with hipRTC (vnd_spec.hpp) behind a generated prologue that defines
//   VS_NT  threads per workgroup (256)      VS_RR  frame pairs per lane and tile (tile T = 2*NT*RR frames)
//   VS_PP  ring slots of T frames           VS_DD  tiles prefetched ahead into registers (1 or 2)
//   VS_C   interleaved channels             VS_LA  LDS reads kept in flight ahead of the FMAs
//   VS_NT_STORES  1: non-temporal output stores (outputs too large to be re-read from cache)
//   VS_BC  1: fan-out of a MONO input (stereo table): one input plane, read by both channels' taps
//   VS_GROUPS = VS_C / 2 channel pairs, and per pair g the read schedule as constexpr arrays:
//   VS_RD_N[g] unique LDS reads with VS_RD_PLANE / VS_RD_OFF[g][k] (frames: (i & ~1) + 2*NT*row) and
//   VS_RD_FIRST[g][k] (prefix of consumer counts); consumers VS_CS_SET (accumulator set: channel-in-
//   pair * 2 + parity of i), VS_CS_ROW, VS_CS_W (weight * segment gain); VS_NODD[g][c],
//   VS_ODD_OFF / VS_ODD_W (the odd taps in the order row 0 accumulates them, for the one output per
//   span that has no lane).
//
// VS_EXACT 1 selects the bit-exact arithmetic instead (VND_MODE_EXACT, see the section "exact mode"
// below); the prologue then carries the step program VS_EX_* in place of the read schedule.
//
// Same arithmetic as conv_fast_kernel (vnd_kernels.hpp: every tap one aligned ds_read_b64 + one
// v_pk_fma_f32; even taps feed outputs (2q, 2q+1), odd taps outputs (2q-1, 2q); the two sets are
// merged once per tile), i.e. the reference's tap sum (decorrelation.py:649-658, :402-414) in free
// summation order.  What the specialisation changes is everything around the FMAs:
//   * tap offsets are ds_read immediates and weights literals: no address VALU, no scalar loads;
//   * a workgroup is PERSISTENT over a span of consecutive tiles of one stream and keeps the
//     window in an LDS RING of PP slots: a frame is staged exactly once (the generic kernel
//     re-stages the halo, 1.6x at cfg2), and the next tile's frames are already in flight in
//     registers while this tile's taps run - HBM requests never pause for the compute phase;
//   * the ring wraps at slot granularity: a read's offset falls into one of a few classes
//     (offset / T), and per tile each class gets a base register pointing at the slot it lands in,
//     so every ring address is still a base + immediate with ONE code body for all slot phases
//     (unrolled over the phases instead, a 128-tap table was 90 KB of code against a 64 KB
//     instruction cache); the first 2*NT frames are mirrored behind the ring so that no read
//     straddles the wrap;
//   * one s_barrier per tile: the odd-set neighbour comes from the next lane by DPP, only the
//     wave-boundary values cross through LDS.
typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef int v4i __attribute__((ext_vector_type(4)));
// LDS pointers carry their address space in the type: through a generic pointer hipcc emits flat loads
#define VS_LDS __attribute__((address_space(3)))
typedef VS_LDS char vs_lchar;
typedef VS_LDS float vs_lfloat;
typedef VS_LDS v2f vs_lv2f;

__device__ v2f vs_load2(v4i rsrc, int voff, int soff, int aux) __asm("llvm.amdgcn.raw.buffer.load.v2f32");
__device__ v4f vs_load4(v4i rsrc, int voff, int soff, int aux) __asm("llvm.amdgcn.raw.buffer.load.v4f32");
__device__ void vs_store2(v2f d, v4i rsrc, int voff, int soff, int aux) __asm("llvm.amdgcn.raw.buffer.store.v2f32");
__device__ void vs_store4(v4f d, v4i rsrc, int voff, int soff, int aux) __asm("llvm.amdgcn.raw.buffer.store.v4f32");

struct VSArgs {
    const float *x;
    float *y;
    long long n;             // frames per stream
    int tiles_total;         // ceil(n / T)
    int tiles_per_span;
    int spans;               // spans per stream
    unsigned nblocks;        // workgroups launched
    unsigned units;          // (stream, channel pair, span) units: workgroup w takes units w, w + nblocks, ...
    int epi_ms_encode;       // VS_EPI: the decorrelate stage's pointwise steps in the store phase (exact mode, stereo)
    int epi_use_width;
    float epi_w_mid, epi_w_side;
};

constexpr int VS_T = 2 * VS_NT * VS_RR;         // frames per tile
constexpr int VS_PT = VS_PP * VS_T;             // frames in the ring
constexpr int VS_PL = VS_PT + 2 * VS_NT + (VS_SHIFT ? 2 : 0);        // frames per LDS plane: ring + mirror of its first 2*NT frames (+ a pad)
constexpr int VS_NW = VS_NT / 64;
constexpr int VS_XO = VS_NW * VS_RR * 2;        // floats of one exchange buffer: [wave][row][channel]
constexpr int VS_NPL0 = VS_BC ? 1 : 2;          // input planes in LDS (a mono input is staged once for both outputs)
constexpr int VS_NPL = VS_SHIFT ? 2 * VS_NPL0 : VS_NPL0;      // exact mode, VS_SHIFT: plus a copy of each, one frame ahead, for the odd offsets
constexpr int VS_CX = VS_BC ? 1 : VS_C;         // interleaved INPUT channels
static_assert(!VS_BC || VS_C == 2, "fan-out: a mono input through a stereo table");
static_assert(VS_DD >= 1 && VS_DD <= 3, "prefetch depth 1..3");
static_assert((VS_NPL * VS_PL * 4 + 2 * VS_XO * 4) <= 160 * 1024, "LDS");
static_assert(2 * VS_PL * 4 < 65536, "ds offset field is 16 bits");
static_assert(!VS_SHIFT || (VS_EXACT && VS_RR >= 2), "the shifted copies serve the exact mode's odd offsets (their mirror's last frame comes from row 1)");

// Raw buffer descriptor (stride 0): num_records = bytes left in the stream, so loads past the end of
// the stream return 0 (the reference's dropped terms, decorrelation.py:656-658) and stores past it
// are discarded.  Built from kernel arguments, blockIdx and the tile counter only: lives in SGPRs.
__device__ __forceinline__ v4i vs_rsrc(const void *base, long long bytes)
{
    const long long cap = 0x7fffffff;
    const unsigned long long addr = (unsigned long long)base;
    v4i r;
    r.x = (int)(unsigned)addr;
    r.y = (int)((unsigned)(addr >> 32) & 0xffffu);
    r.z = (int)(bytes < 0 ? 0 : (bytes > cap ? cap : bytes));
    r.w = 0x00020000;
    return r;
}

// blocks b and b + 8 share an XCD (and its L2): give one XCD consecutive logical ids, so the channel
// pairs of one span (which read the same cache lines when C > 2) and neighbouring spans share an L2
__device__ __forceinline__ unsigned vs_xcd_remap(unsigned b, unsigned nwg)
{
    const unsigned q = nwg >> 3, r = nwg & 7u, xcd = b & 7u;
    const unsigned start = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return start + (b >> 3);
}

// one frame pair of channel pair g: {f0.c0, f0.c1, f1.c0, f1.c1}
__device__ __forceinline__ v4f vs_load_pair(v4i rsrc, int voff)
{
    if constexpr (VS_BC) {                          // two mono frames: kept in the slots of channel 0
        const v2f a = vs_load2(rsrc, voff, 0, VS_LOAD_AUX);
        return v4f{a.x, 0.0f, a.y, 0.0f};
    } else if constexpr (VS_C == 2) {
        return vs_load4(rsrc, voff, 0, VS_LOAD_AUX);
    } else {
        const v2f a = vs_load2(rsrc, voff, 0, 0), b = vs_load2(rsrc, voff + VS_C * 4, 0, 0);
        return v4f{a.x, a.y, b.x, b.y};
    }
}

// aux bit 1 = nt: a large output is not read again before it has left the caches
constexpr int VS_STORE_AUX = VS_NT_STORES ? VS_NT_STORE_AUX : 0;
static_assert(VS_QUAD_STORES == 1, "a wider signal's frame pairs are stored through the lane-quad exchange (vs_store_pair): the only form");

// a value of another lane of the quad (DPP quad_perm; every lane of the quad must be executing)
template <int CTRL>
__device__ __forceinline__ float vs_quad(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}

// The lane's frame pair (frames 2p, 2p+1 at byte offset voff) goes to memory; second = false keeps frame 2p+1 back
// (the fast kernel's last lane: that frame is completed a tile later).
// In a wider signal a frame pair is two 8-byte pieces VS_C*4 bytes apart, and a store instruction of such pairs touches
// every other frame: 64 pieces in 32 lines.  There the four lanes of a quad - frames 8k .. 8k+7 - first exchange
// frames, so that one instruction writes frames 8k .. 8k+3 (lane i: frame 8k+i, from lane i/2) and the next
// 8k+4 .. 8k+7: four pieces per line, which the memory pipeline takes 1.7x faster (tools/micro/piece_stores.hip).
// Called by every lane of a wave (the exchange reads the neighbours' registers).
__device__ __forceinline__ void vs_store_pair(v4f v, v4i rsrc, int voff, bool second = true)
{
    if constexpr (VS_C == 2) {
        if (second) vs_store4(v, rsrc, voff, 0, VS_STORE_AUX);
        else vs_store2(v2f{v.x, v.y}, rsrc, voff, 0, VS_STORE_AUX);
    } else {
        const int i = (int)threadIdx.x & 3;
        const bool odd = (i & 1) != 0;
        // quad_perm [0,0,1,1] = 0x50: lane i reads lane i/2;  [2,2,3,3] = 0xfa: lane 2 + i/2
        const float a0 = vs_quad<0x50>(v.x), a1 = vs_quad<0x50>(v.y), a2 = vs_quad<0x50>(v.z), a3 = vs_quad<0x50>(v.w);
        const float b0 = vs_quad<0xfa>(v.x), b1 = vs_quad<0xfa>(v.y), b2 = vs_quad<0xfa>(v.z), b3 = vs_quad<0xfa>(v.w);
        const v2f A = {odd ? a2 : a0, odd ? a3 : a1};
        const v2f B = {odd ? b2 : b0, odd ? b3 : b1};
        const int va = voff - i * (VS_C * 4);                  // frame 8k + i: the quad's first frame is 2 * (p - i)
        vs_store2(A, rsrc, va, 0, VS_STORE_AUX);
        if (second) vs_store2(B, rsrc, va + 4 * VS_C * 4, 0, VS_STORE_AUX);      // (frame 8k+7 is lane 3's own second frame)
        __builtin_amdgcn_sched_barrier(0);         // (one pair's exchange at a time: hoisted together they cost 8 registers per pair)
    }
}

// de-interleave one staged pair into the two channel planes; `at` = byte offset of the frame pair
// inside a plane (immediate after inlining)
__device__ __forceinline__ void vs_write_pair(vs_lchar *lane_lds, int at, v4f v)
{
    *(vs_lv2f *)(lane_lds + at) = v2f{v.x, v.z};
    if constexpr (!VS_BC) *(vs_lv2f *)(lane_lds + VS_PL * 4 + at) = v2f{v.y, v.w};
    if constexpr (VS_SHIFT) {
        // the copy one frame ahead: S[k] = x[k + 1] along the ring, so that an odd offset is an ALIGNED pair of S.
        // This pair's frames 2q, 2q+1 are S's frames 2q-1, 2q: two dword writes.  The ring's first pair (q = 0)
        // belongs at S[PT-1]: its mirrored write (at + PT) puts it there, the plain one falls into the pad that
        // ends the plane before.  S[kT-1], inside the slot before the one being refilled, is the new tile's first
        // frame - what follows that slot's last frame once the refill is complete, and outside every window until then.
        *(vs_lfloat *)(lane_lds + VS_NPL0 * VS_PL * 4 + at - 4) = v.x;
        *(vs_lfloat *)(lane_lds + VS_NPL0 * VS_PL * 4 + at) = v.z;
        if constexpr (!VS_BC) {
            *(vs_lfloat *)(lane_lds + (VS_NPL0 + 1) * VS_PL * 4 + at - 4) = v.y;
            *(vs_lfloat *)(lane_lds + (VS_NPL0 + 1) * VS_PL * 4 + at) = v.w;
        }
    }
}

// the last frame of the shifted copies' mirror, S[PT + 2*NT - 1] = x[2*NT]: the ring's frame 2*NT is row 1's first
// (lane 0 of slot 0 calls this with row 1's `at`)
__device__ __forceinline__ void vs_write_shift_tail(vs_lchar *lane_lds, int at, v4f v)
{
    *(vs_lfloat *)(lane_lds + VS_NPL0 * VS_PL * 4 + at + VS_PT * 4 - 4) = v.x;
    if constexpr (!VS_BC) *(vs_lfloat *)(lane_lds + (VS_NPL0 + 1) * VS_PL * 4 + at + VS_PT * 4 - 4) = v.y;
}

// row j of the slot whose plane byte offset is slot_bytes; the ring's first 2*NT frames (slot 0, row 0)
// are written once more behind the ring
template <int J = 0>
__device__ __forceinline__ void vs_fill_rows(vs_lchar *slot_lds, bool slot0, bool lane0, const v4f (&v)[VS_RR])
{
    if constexpr (J < VS_RR) {
        constexpr int at = 2 * VS_NT * J * 4;
        vs_write_pair(slot_lds, at, v[J]);
        if constexpr (J == 0) { if (slot0) vs_write_pair(slot_lds, at + VS_PT * 4, v[J]); }
        if constexpr (VS_SHIFT && J == 1) { if (slot0 && lane0) vs_write_shift_tail(slot_lds, at, v[J]); }
        vs_fill_rows<J + 1>(slot_lds, slot0, lane0, v);
    }
}

#if VS_EPI
static_assert(VS_C == 2, "the fused pointwise steps need a stereo output");
// VelvetNoise.decorrelate's pointwise steps on one stereo frame pair, in the reference's float32 operation order
// (utils/dsp.py:59-63 side-channel encode, :34-37 stereo width; as epi_pointwise in vnd_kernels.hpp; built with
// -ffp-contract=off).  v = {L0, R0, L1, R1} of the convolution, xin the same of the input.
__device__ __forceinline__ v2f vs_pointwise1(const VSArgs &a, v2f y, v2f x)          // one frame: {L, R}
{
    float y0 = y.x, y1 = y.y;
    if (a.epi_ms_encode) {
        const float mid = x.x + x.y;
        const float side = (y0 - y1) * 0.5f;
        y0 = (mid + side) * 0.5f;
        y1 = (mid - side) * 0.5f;
    }
    if (a.epi_use_width) {
        float m = (y0 + y1) * 0.5f, sd = (y0 - y1) * 0.5f;
        m = m * a.epi_w_mid;
        sd = sd * a.epi_w_side;
        y0 = m + sd;
        y1 = m - sd;
    }
    return v2f{y0, y1};
}

__device__ __forceinline__ v4f vs_pointwise(const VSArgs &a, v4f v, v4f xin)            // a frame pair
{
    const v2f f0 = vs_pointwise1(a, v2f{v.x, v.y}, v2f{xin.x, xin.y}), f1 = vs_pointwise1(a, v2f{v.z, v.w}, v2f{xin.z, xin.w});
    return v4f{f0.x, f0.y, f1.x, f1.y};
}
#endif

struct VSState {
#if VS_EXACT
    v2f out[2][VS_RR];          // [channel-in-pair][row]: the output pair (2q, 2q+1)
    v2f sb[2][VS_RR];           // the running segment (function-path tables: the one and only)
#else
    v2f acc[4][VS_RR];          // [channel-in-pair * 2 + parity][row]
#endif
    v4f pre[VS_DD][VS_RR];      // frames in flight for the slots ahead
    float carry[2];             // even part of the previous tile's last output (last wave, lane 63)
#if VS_EPI
    float carry_x[2];           // and that frame's input (the pointwise steps run when the output is complete)
#endif
};

#if VS_EXACT
// ---- exact mode: the reference's own association, bit for bit ------------------------------------
// Step k of the program adds ONE tap to its channel's running segment, in TABLE order:
//     sb = f32(sb + f32(x * w))                  (NumPy's  out[:N-i] += x[i:] * w,  decorrelation.py:656-658;
//                                                 a weight of +-1 is the class path's  sb += / -= x,  :405-410)
// and, when VS_EX_END says the tap closes a segment,  sb *= gain  (unless the envelope is the identity,
// :411-412) and  out += sb  (:413);  a function-path table is one segment whose sum IS the output.
// One accumulator per output (no even/odd sets, nothing crosses lanes): an even offset is one aligned
// ds_read_b64, an odd one two ds_read_b32 straight into the halves of the operand pair.  Products and
// sums are separate, individually rounded instructions (-ffp-contract=off).  Channels alternate step
// by step; reads run VS_LA steps ahead of the arithmetic.
constexpr int VS_NCLS = VS_MAX_OFF / VS_T + 1;     // classes of read offsets: offset / T
constexpr int VS_NCLSX = VS_SHIFT ? 2 * VS_NCLS : VS_NCLS;      // ... and the same bases into the shifted copies (immediates stay 16 bits)

template <int G, int K, int J = 0>
__device__ __forceinline__ void vs_ex_issue(vs_lchar *const (&cls)[VS_NCLSX], v2f (&buf)[VS_RR])
{
    if constexpr (K < VS_EX_N[G] && J < VS_RR) {
        constexpr int plane = (VS_BC ? 0 : VS_EX_CH[G][K]) * VS_PL * 4;
        constexpr int off = VS_EX_OFF[G][K] + 2 * VS_NT * J;
        if constexpr ((off & 1) == 0) {
            buf[J] = *(const volatile vs_lv2f *)(cls[off / VS_T] + plane + (off % VS_T) * 4);
        } else if constexpr (VS_SHIFT) {
            constexpr int so = off - 1;                    // even: (x[off], x[off + 1]) = (S[off - 1], S[off])
            buf[J] = *(const volatile vs_lv2f *)(cls[VS_NCLS + so / VS_T] + plane + (so % VS_T) * 4);
        } else {
            const float lo = *(const volatile vs_lfloat *)(cls[off / VS_T] + plane + (off % VS_T) * 4);
            const float hi = *(const volatile vs_lfloat *)(cls[(off + 1) / VS_T] + plane + ((off + 1) % VS_T) * 4);
            buf[J] = v2f{lo, hi};
        }
        vs_ex_issue<G, K, J + 1>(cls, buf);
    }
}

template <int G, int K>
__device__ __forceinline__ void vs_ex_consume(VSState &st, const v2f (&buf)[VS_RR])
{
    constexpr int c = VS_EX_CH[G][K];
    constexpr float w = VS_EX_W[G][K];
#pragma unroll
    for (int j = VS_RR - 1; j >= 0; --j) {              // last-issued row first: one wait covers them all
        if constexpr (w == 1.0f) st.sb[c][j] = st.sb[c][j] + buf[j];
        else if constexpr (w == -1.0f) st.sb[c][j] = st.sb[c][j] - buf[j];
        else { const v2f p = buf[j] * v2f{w, w}; st.sb[c][j] = st.sb[c][j] + p; }
    }
    if constexpr (VS_EX_END[G][K] != 0) {
        constexpr float gain = VS_EX_GAIN[G][K];
#pragma unroll
        for (int j = 0; j < VS_RR; ++j) {
            if constexpr (VS_EX_END[G][K] == 1) {                 // function path: the sum is the output
                st.out[c][j] = st.sb[c][j];
            } else {
                if constexpr (VS_EX_END[G][K] == 3) st.sb[c][j] = st.sb[c][j] * v2f{gain, gain};
                st.out[c][j] = st.out[c][j] + st.sb[c][j];
                st.sb[c][j] = v2f{0.0f, 0.0f};
            }
        }
    }
}

template <int G, int LO, int HI>
struct VSExact {
    static __device__ __forceinline__ void run(vs_lchar *const (&cls)[VS_NCLSX], VSState &st, v2f (&buf)[VS_LA + 1][VS_RR])
    {
        if constexpr (HI - LO == 1) {
            constexpr int K = LO;
            vs_ex_issue<G, K + VS_LA>(cls, buf[(K + VS_LA) % (VS_LA + 1)]);
            vs_ex_consume<G, K>(st, buf[K % (VS_LA + 1)]);
            __builtin_amdgcn_sched_barrier(0);                    // pin the software pipeline (see VSTaps)
        } else if constexpr (HI - LO > 1) {
            constexpr int MID = LO + (HI - LO) / 2;
            VSExact<G, LO, MID>::run(cls, st, buf);
            VSExact<G, MID, HI>::run(cls, st, buf);
        }
    }
};

template <int G, int K>
struct VSExactPrime {
    static __device__ __forceinline__ void run(vs_lchar *const (&cls)[VS_NCLSX], v2f (&buf)[VS_LA + 1][VS_RR])
    {
        if constexpr (K < VS_LA) {
            vs_ex_issue<G, K>(cls, buf[K % (VS_LA + 1)]);
            VSExactPrime<G, K + 1>::run(cls, buf);
        }
    }
};
#else
// ---- the tap loops of one tile: slot phase S, channel pair G ---------------------------------
// The generated schedule is a list of UNIQUE LDS reads: read k fetches the aligned pair at frame
// offset VS_RD_OFF[G][k] (= (i & ~1) + 2*NT*row) of plane VS_RD_PLANE[G][k] and feeds the FMAs
// VS_CS_*[G][VS_RD_FIRST[G][k] .. VS_RD_FIRST[G][k+1]): one per (tap, row) that needs exactly that
// pair.  Rows are 2*NT frames apart, so two taps whose offsets differ by a multiple of 2*NT share
// reads between rows - 3 % of the reads at cfg2, 19 % with 128 taps per channel.
// volatile LDS loads: hipcc must keep each read a plain ds_read_b64 with an immediate offset
// (fused into ds_read2st64_b64 they run at half the LDS rate) and in source order, which is the
// software pipeline: read k + LA is issued before read k is consumed.  Waits are hipcc's own
// counted lgkmcnt(N).
constexpr int VS_NCLS = VS_MAX_OFF / VS_T + 1;     // classes of read offsets: offset / T

template <int G, int K>
__device__ __forceinline__ void vs_issue(vs_lchar *const (&cls)[VS_NCLS], v2f &buf)
{
    if constexpr (K < VS_RD_N[G]) {
        constexpr int c = VS_RD_OFF[G][K] / VS_T, rem = VS_RD_OFF[G][K] % VS_T;
        buf = *(const volatile vs_lv2f *)(cls[c] + VS_RD_PLANE[G][K] * VS_PL * 4 + rem * 4);
    }
}

template <int G, int M, int END>
__device__ __forceinline__ void vs_consume(VSState &st, const v2f &buf)
{
    if constexpr (M < END) {
        constexpr float w = VS_CS_W[G][M];
        st.acc[VS_CS_SET[G][M]][VS_CS_ROW[G][M]] =
            __builtin_elementwise_fma(buf, v2f{w, w}, st.acc[VS_CS_SET[G][M]][VS_CS_ROW[G][M]]);
        vs_consume<G, M + 1, END>(st, buf);
    }
}

// reads [LO, HI) of the schedule, split in halves: the template depth stays logarithmic in the table size
template <int G, int LO, int HI>
struct VSTaps {
    // buf is a ring of LA + 1 read buffers, indexed statically
    static __device__ __forceinline__ void run(vs_lchar *const (&cls)[VS_NCLS], VSState &st, v2f (&buf)[VS_LA + 1])
    {
        if constexpr (HI - LO == 1) {
            constexpr int K = LO;
            vs_issue<G, K + VS_LA>(cls, buf[(K + VS_LA) % (VS_LA + 1)]);
            vs_consume<G, VS_RD_FIRST[G][K], VS_RD_FIRST[G][K + 1]>(st, buf[K % (VS_LA + 1)]);
            // pin the software pipeline: left alone, hipcc's scheduler lets the reads run far ahead of
            // the FMAs (168 VGPRs, a drained LDS queue before every batch of FMAs)
            __builtin_amdgcn_sched_barrier(0);
        } else if constexpr (HI - LO > 1) {
            constexpr int MID = LO + (HI - LO) / 2;
            VSTaps<G, LO, MID>::run(cls, st, buf);
            VSTaps<G, MID, HI>::run(cls, st, buf);
        }
    }
};

template <int G, int K>
struct VSPrime {
    static __device__ __forceinline__ void run(vs_lchar *const (&cls)[VS_NCLS], v2f (&buf)[VS_LA + 1])
    {
        if constexpr (K < VS_LA) {
            vs_issue<G, K>(cls, buf[K % (VS_LA + 1)]);
            VSPrime<G, K + 1>::run(cls, buf);
        }
    }
};

#endif   // VS_EXACT

#if !VS_EXACT
// lane l takes lane l+1's value; lane 63 takes `last` (DPP wave_shl:1, no LDS traffic)
__device__ __forceinline__ float vs_from_next_lane(float v, float last)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, last), __builtin_bit_cast(int, v),
                                                                 0x130, 0xf, 0xf, false));
}

// The odd-tap part of a span's LAST output frame f (no pair to its right is computed by this
// workgroup): sum over odd i of w * x[f + i], x[f + i] = ring[(ring_frame0 + (i - 1)) mod PT].
// The same fma chain, in the same order, as the odd accumulator of the pair that would follow, so
// the result does not depend on where the span seams fall (batch == loop, bit for bit).  Every lane
// of the calling wave runs the chain on broadcast reads; once per span.
template <int G>
__device__ __forceinline__ float vs_edge(const vs_lfloat *lds, int c, int ring_frame0)
{
    float acc = 0.0f;
    for (int k = 0; k < VS_NODD[G][c]; ++k) {
        int fr = ring_frame0 + VS_ODD_OFF[G][c][k];          // (i - 1), even
        fr = fr >= VS_PT ? fr - VS_PT : fr;
        acc = __builtin_fmaf(lds[(VS_BC ? 0 : c) * VS_PL + fr], VS_ODD_W[G][c][k], acc);
    }
    return acc;
}

#endif

// ---- one tile: slot phase s = t % PP (run time), prefetch buffer PB = t % DD (static) --------------
template <int PB, int G>
__device__ __forceinline__ void vs_tile(const VSArgs &a, vs_lfloat *lds, VSState &st, int t, int s, long long bytes_need,
                                        const float *xs, float *ys, long long bytes_left, int tid)
{
    constexpr int T = VS_T;
    vs_lchar *lane_lds = (vs_lchar *)lds + tid * 8;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    vs_lfloat *xo = lds + VS_NPL * VS_PL + (t & 1) * VS_XO;      // exchange buffer, alternating per tile

    // 1. the frames loaded DD tiles ago land in the slot that tile t-1 has just stopped reading
    constexpr int pb = PB;
    const int fill_slot = s == 0 ? VS_PP - 1 : s - 1;
    vs_fill_rows(lane_lds + fill_slot * (T * 4), fill_slot == 0, tid == 0, st.pre[pb]);

    // 2. ... and the loads for slot t + PP - 1 + DD start now, to be consumed DD tiles from here
    {
        const long long f = (long long)(t + VS_PP - 1 + VS_DD) * T;
        // bytes_need ends where the span's last window ends: the slots prefetched past it are never
        // read, and an out-of-range buffer load moves no data
        const v4i rx = vs_rsrc(xs + f * VS_CX, bytes_need - f * VS_CX * 4);
#pragma unroll
        for (int j = 0; j < VS_RR; ++j) st.pre[pb][j] = vs_load_pair(rx, (tid + VS_NT * j) * (2 * VS_CX * 4));
    }

#if VS_EXACT
    // 3. the step program
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int j = 0; j < VS_RR; ++j) { st.out[c][j] = v2f{0.0f, 0.0f}; st.sb[c][j] = v2f{0.0f, 0.0f}; }
    {
        vs_lchar *cls[VS_NCLSX];
#pragma unroll
        for (int c = 0; c < VS_NCLS; ++c) {
            int sc = s + c;
            sc = sc >= VS_PP ? sc - VS_PP : sc;
            cls[c] = lane_lds + sc * (T * 4);
            if constexpr (VS_SHIFT) cls[VS_NCLS + c] = cls[c] + VS_NPL0 * VS_PL * 4;
        }
        v2f buf[VS_LA + 1][VS_RR];
        VSExactPrime<G, 0>::run(cls, buf);
        VSExact<G, 0, VS_EX_N[G]>::run(cls, st, buf);
    }
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int j = 0; j < VS_RR; ++j) asm volatile("" : "+v"(st.out[c][j]));
#if VS_EPI
    // the tile's own input frames are still in the ring (this tile's slot, offset 0): fetched before the barrier,
    // because the next tile refills that slot
    v2f xin[2][VS_RR];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int j = 0; j < VS_RR; ++j)
            xin[c][j] = *(const volatile vs_lv2f *)(lane_lds + s * (T * 4) + (VS_BC ? 0 : c) * VS_PL * 4 + 2 * VS_NT * j * 4);
#endif
    // 4. every wave is done reading this tile's window before the next tile refills a slot
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    // 5. store: every lane owns its outputs outright
    (void)lane; (void)wave; (void)xo;
    const long long fo = (long long)t * T;
    const v4i ry = vs_rsrc(ys + fo * VS_C, bytes_left - fo * VS_C * 4);
#pragma unroll
    for (int j = 0; j < VS_RR; ++j) {
        v4f v = {st.out[0][j].x, st.out[1][j].x, st.out[0][j].y, st.out[1][j].y};
#if VS_EPI
        v = vs_pointwise(a, v, v4f{xin[0][j].x, xin[1][j].x, xin[0][j].y, xin[1][j].y});
#endif
        vs_store_pair(v, ry, (tid + VS_NT * j) * (2 * VS_C * 4));
    }
}
#else
    // 3. tap loops
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int j = 0; j < VS_RR; ++j) st.acc[s][j] = v2f{0.0f, 0.0f};
    {
        // class c of read offsets lands in slot (s + c) mod PP this tile
        vs_lchar *cls[VS_NCLS];
#pragma unroll
        for (int c = 0; c < VS_NCLS; ++c) {
            int sc = s + c;
            sc = sc >= VS_PP ? sc - VS_PP : sc;
            cls[c] = lane_lds + sc * (T * 4);                     // the immediates carry offset % T
        }
        v2f buf[VS_LA + 1];
        VSPrime<G, 0>::run(cls, buf);
        VSTaps<G, 0, VS_RD_N[G]>::run(cls, st, buf);
    }
    // the sums are complete HERE: without this use hipcc sinks the even sets' FMA chains (first read
    // after the barrier) below it, with every LDS value they consume kept live until then
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int j = 0; j < VS_RR; ++j) asm volatile("" : "+v"(st.acc[s][j]));

#if VS_EPI
    // the tile's own input frames are still in the ring (this tile's slot, offset 0): fetched before the barrier,
    // because the next tile refills that slot
    v2f xin[2][VS_RR];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int j = 0; j < VS_RR; ++j)
            xin[c][j] = *(const volatile vs_lv2f *)(lane_lds + s * (T * 4) + (VS_BC ? 0 : c) * VS_PL * 4 + 2 * VS_NT * j * 4);
#endif
    // 4. wave-boundary values of the odd sets: lane 0 of every wave publishes accO.x per row and channel
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < VS_RR; ++j) {
            xo[(wave * VS_RR + j) * 2 + 0] = st.acc[1][j].x;
            xo[(wave * VS_RR + j) * 2 + 1] = st.acc[3][j].x;
        }
    }
    // LDS only: the prefetch loads and the previous tile's stores stay in flight across the barrier
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

    // 5. merge the two sets and store.  Output pair q = tid + NT*j needs accO.x of pair q + 1: the next
    // lane, the next wave's lane 0 (same row), or - last wave - wave 0's lane 0 of the next row; the
    // tile's very last frame waits for the next tile's pair 0 (carry).
    const long long fo = (long long)t * T;
    const v4i ry = vs_rsrc(ys + fo * VS_C, bytes_left - fo * VS_C * 4);
    const int nbase = wave < VS_NW - 1 ? (wave + 1) * VS_RR * 2 : 2;
    const bool last_lane = tid == VS_NT - 1;
    if (wave == VS_NW - 1 && t > 0) {
        // complete and store the previous tile's last frame: its odd part is this tile's pair 0
        const float o0 = xo[0], o1 = xo[1];
        if (last_lane) {
            v2f fix = {st.carry[0] + o0, st.carry[1] + o1};
#if VS_EPI
            fix = vs_pointwise1(a, fix, v2f{st.carry_x[0], st.carry_x[1]});
#endif
            const v4i rf = vs_rsrc(ys + (fo - 1) * VS_C, bytes_left - (fo - 1) * VS_C * 4);     // offsets are unsigned
            vs_store2(fix, rf, 0, 0, 0);
        }
    }
#pragma unroll
    for (int j = 0; j < VS_RR; ++j) {
        const float b0 = xo[nbase + j * 2 + 0], b1 = xo[nbase + j * 2 + 1];
        const float n0 = vs_from_next_lane(st.acc[1][j].x, b0);
        const float n1 = vs_from_next_lane(st.acc[3][j].x, b1);
        v4f v;
        v.x = st.acc[0][j].x + st.acc[1][j].y;      // frame 2q,   channel 0
        v.y = st.acc[2][j].x + st.acc[3][j].y;      // frame 2q,   channel 1
        v.z = st.acc[0][j].y + n0;                  // frame 2q+1, channel 0
        v.w = st.acc[2][j].y + n1;                  // frame 2q+1, channel 1
#if VS_EPI
        // (the last lane's frame 2q+1 is not complete yet: what the steps make of it here is never stored)
        v = vs_pointwise(a, v, v4f{xin[0][j].x, xin[1][j].x, xin[0][j].y, xin[1][j].y});
#endif
        const int voff = (tid + VS_NT * j) * (2 * VS_C * 4);
        bool whole = true;
        if (j == VS_RR - 1 && wave == VS_NW - 1) {
            // the tile's last frame is completed by the next tile (or by vs_span at the span's end)
            if (last_lane) {
                st.carry[0] = st.acc[0][j].y;
                st.carry[1] = st.acc[2][j].y;
#if VS_EPI
                st.carry_x[0] = xin[0][j].y;
                st.carry_x[1] = xin[1][j].y;
#endif
                whole = false;
            }
        }
        vs_store_pair(v, ry, voff, whole);
    }
}
#endif   // VS_EXACT

template <int G>
__device__ __forceinline__ void vs_span(const VSArgs &a, vs_lfloat *lds, long long stream, int span)
{
    constexpr int T = VS_T;
    const int tid = threadIdx.x;
    vs_lchar *lane_lds = (vs_lchar *)lds + tid * 8;
    const int t_first = span * a.tiles_per_span;
    const int left = a.tiles_total - t_first;
    const int ntiles = left < a.tiles_per_span ? left : a.tiles_per_span;
    const long long f0 = (long long)t_first * T;
    const float *xs = a.x + (stream * a.n + f0) * VS_CX + (VS_BC ? 0 : 2 * G);
    float *ys = a.y + (stream * a.n + f0) * VS_C + 2 * G;
    const long long bytes_left = ((a.n - f0) * VS_C - 2 * G) * 4;
    const long long bytes_left_x = VS_BC ? (a.n - f0) * 4 : bytes_left;
    // what this span reads: its tiles plus the last tile's halo, i.e. slots 0 .. ntiles + PP - 3
    const long long need = ((long long)(ntiles + VS_PP - 2) * T * VS_CX - (VS_BC ? 0 : 2 * G)) * 4;
    const long long bytes_need = need < bytes_left_x ? need : bytes_left_x;

    VSState st;
    st.carry[0] = st.carry[1] = 0.0f;
#if VS_EPI
    st.carry_x[0] = st.carry_x[1] = 0.0f;
#endif

    // prologue: slots 0 .. PP-2 hold the first tile's window; the loads for the next DD slots start
    {
        const v4i rx = vs_rsrc(xs, bytes_need);
        v4f w[VS_PP - 1][VS_RR];
#pragma unroll
        for (int s = 0; s < VS_PP - 1; ++s)
#pragma unroll
            for (int j = 0; j < VS_RR; ++j) w[s][j] = vs_load_pair(rx, (s * (T / 2) + tid + VS_NT * j) * (2 * VS_CX * 4));
#pragma unroll
        for (int d = 0; d < VS_DD; ++d)
#pragma unroll
            for (int j = 0; j < VS_RR; ++j)
                st.pre[d][j] = vs_load_pair(rx, ((VS_PP - 1 + d) * (T / 2) + tid + VS_NT * j) * (2 * VS_CX * 4));
#pragma unroll
        for (int s = 0; s < VS_PP - 1; ++s)
#pragma unroll
            for (int j = 0; j < VS_RR; ++j) {
                const int at = (s * T + 2 * VS_NT * j) * 4;
                vs_write_pair(lane_lds, at, w[s][j]);
                if (s == 0 && j == 0) vs_write_pair(lane_lds, at + VS_PT * 4, w[s][j]);
                if constexpr (VS_SHIFT) { if (s == 0 && j == 1 && tid == 0) vs_write_shift_tail(lane_lds, at, w[s][j]); }
            }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

    for (int t = 0, slot = 0; t < ntiles;) {
        vs_tile<0, G>(a, lds, st, t, slot, bytes_need, xs, ys, bytes_left, tid);
        slot = slot + 1 == VS_PP ? 0 : slot + 1;
        if (++t >= ntiles) break;
        if constexpr (VS_DD > 1) {
            vs_tile<1, G>(a, lds, st, t, slot, bytes_need, xs, ys, bytes_left, tid);
            slot = slot + 1 == VS_PP ? 0 : slot + 1;
            if (++t >= ntiles) break;
        }
        if constexpr (VS_DD > 2) {
            vs_tile<2, G>(a, lds, st, t, slot, bytes_need, xs, ys, bytes_left, tid);
            slot = slot + 1 == VS_PP ? 0 : slot + 1;
            if (++t >= ntiles) break;
        }
    }

#if !VS_EXACT
    // the span's last output frame has no pair to its right: its odd taps are reduced from the ring,
    // x[f + i] = ring[(ntiles * T + (i - 1)) mod PT], by the last wave.  The ring slots it reads were
    // written at least one barrier ago.
    if (tid >= VS_NT - 64) {
        const int ring0 = (int)(((long long)ntiles * T) % VS_PT);
        const float e0 = vs_edge<G>(lds, 0, ring0), e1 = vs_edge<G>(lds, 1, ring0);
        if (tid == VS_NT - 1) {
            const long long fl = (long long)ntiles * T - 1;
            const v4i rf = vs_rsrc(ys + fl * VS_C, bytes_left - fl * VS_C * 4);
            v2f last = {st.carry[0] + e0, st.carry[1] + e1};
#if VS_EPI
            last = vs_pointwise1(a, last, v2f{st.carry_x[0], st.carry_x[1]});
#endif
            vs_store2(last, rf, 0, 0, 0);
        }
    }
#endif
}

// VS_WAVES_PER_EU: the waves per SIMD that the LDS footprint lets a CU hold; without the bound hipcc
// spreads an 84-register loop body over 250 registers (the prologue's loads) and halves the residency
extern "C" __global__ __launch_bounds__(VS_NT) __attribute__((amdgpu_waves_per_eu(VS_WAVES_PER_EU, 8)))
void vnd_spec_kernel(const VSArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds_generic[];
    vs_lfloat *lds = (vs_lfloat *)lds_generic;
    // One round of workgroups: more units than resident slots are walked inside the kernel (a second
    // round of dispatches measured 9 % slower than the same work in one round of twice-as-long workgroups).
    for (unsigned unit = vs_xcd_remap(blockIdx.x, a.nblocks); unit < a.units; unit += a.nblocks) {
        unsigned id = unit;
        const int g = (int)(id % (unsigned)VS_GROUPS);
        id /= (unsigned)VS_GROUPS;
        const int span = (int)(id % (unsigned)a.spans);
        const long long stream = id / (unsigned)a.spans;
        VS_DISPATCH(g)
        // the next unit refills the ring: every wave must be done with this one's (the span-end chain reads it)
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
}
)VNDSPEC"
