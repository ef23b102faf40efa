R"VNDWIN(
// vnd_spec_kernel, WINDOW form - the per-table tap sum with a register window (gfx950, wave64).
//
// Compiled at run time with hipRTC (vnd_win.hpp) behind a generated prologue that defines
//   VW_NT   threads per workgroup                 VW_M   consecutive output frames a lane owns per tile (16 | 32 | 64)
//   VW_R    ring entries (one entry = the M frames of one lane's run): NT of the tile + VW_DE of halo
//   VW_G    entries mirrored behind the ring, = the reach of one base register
//   VW_NB   base registers per channel (VW_DE / VW_G + 1)
//   VW_PLANE  bytes between the LDS planes of consecutive 16-byte chunks of an entry
//   VW_LA   LDS reads kept in flight ahead of the FMAs
//   VW_C    interleaved channels of the signal (even): a workgroup takes ONE channel pair of a span, 8 bytes of
//           every VW_C*4-byte frame (VW_C = 2: the whole frame, 16-byte accesses)
//   VW_Q    1: the QUAD form for signals of 4k channels - a workgroup takes a channel QUAD of a span (16 bytes of every
//           frame), a wave computes ONE channel of it (tap functions vw_taps_<pair>c<channel>) and stages and stores whole
//           16-byte pieces for all four (vw_span_qc below)
//           2: the OCTET form for signals of 8k channels - two neighbouring quads (32 bytes of every frame: with 8 channels,
//           whole frames and whole cache lines) per workgroup, an eighth of its lanes per channel
//   VW_S    1: the SPLIT form of a stereo signal - half the workgroup's waves compute channel 0, the others channel 1 (the tap
//           functions vw_taps_c0 / vw_taps_c1): a lane carries one channel's accumulators, so three waves fit a SIMD's registers
//           where the plain form holds two (vw_span_s below)
// and the functions vw_taps(), vw_taps_1(), ... (at the marker below): the tap sum of ONE lane for each channel
// pair, fully unrolled, with vw_taps_of<PG>() to pick one and VW_DISPATCH(pg): the span loop vw_span<pg> of a run-time pair number.
//
// The reference's tap sum (decorrelation.py:649-658, :402-414) asks, per output sample, for one input sample
// per tap.  vnd_spec_kernel.inc reads each of them from LDS (one aligned ds_read_b64 per tap and output
// pair: 4 B per FMA); here a lane owns M CONSECUTIVE outputs of both channels, so the windows
// x[n+i .. n+i+M) of taps whose offsets are closer than M overlap in its registers: the lane reads the
// UNION of its taps' windows once, in ascending 16-byte chunks (ds_read_b128), and every chunk feeds all
// the (tap, output) pairs it covers - 2.6 B per FMA on a 30-tap log-distributed table with M = 32,
// 1.4 B on a uniform 128-tap one.  Tap offsets are compile-time constants, so which register a tap reads
// for which output is static: no address arithmetic, no shuffles.
//   * LDS layout: chunk r of ring entry p lives at r * PLANE + p * 16 (per channel).  Lanes own
//     consecutive entries, so every window read is 64 consecutive 16-byte pieces: conflict-free, and
//     its address is a per-lane base register + an immediate.  The ring wraps at entry granularity:
//     base k holds entry (own + k*G) mod R, the immediate reaches at most G-1 entries further, into
//     the mirror of the ring's first G entries.
//   * arithmetic as in the other fast kernels: v_pk_fma_f32 on aligned pairs.  Even taps accumulate
//     output pairs (0,1), (2,3), ...; odd taps pairs (1,2), (3,4), ... plus outputs 0 and M-1 as single
//     FMAs - everything stays inside the lane, nothing is exchanged between lanes or tiles.  Every
//     output is fl(E + O), E / O = the fma chains over its even / odd taps in ascending offset: the
//     result does not depend on geometry, tile or span position (batch == loop, bit for bit).
//   * no refill region: a tile's own entries die at the barrier that ends its tap phase, and the wave
//     that owned them (a) transposes its outputs through them (planar runs -> interleaved frame
//     pairs: every global store instruction writes 1 KB of consecutive frames), (b) refills them with
//     the frames it prefetched into registers a tile ago - all wave-private, in LDS program order -
//     then a second barrier publishes the refill.  The ring is one tile + halo: twice the occupancy
//     of a ring with a slot in flight.
typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef int v4i __attribute__((ext_vector_type(4)));
#define VW_LDS __attribute__((address_space(3)))
typedef VW_LDS char vw_lchar;
typedef VW_LDS float vw_lfloat;
typedef VW_LDS v2f vw_lv2f;
typedef VW_LDS v4f vw_lv4f;

__device__ v2f vw_load2(v4i rsrc, int voff, int soff, int aux) __asm("llvm.amdgcn.raw.buffer.load.v2f32");
__device__ v4f vw_load4(v4i rsrc, int voff, int soff, int aux) __asm("llvm.amdgcn.raw.buffer.load.v4f32");
__device__ void vw_store4(v4f d, v4i rsrc, int voff, int soff, int aux) __asm("llvm.amdgcn.raw.buffer.store.v4f32");
__device__ void vw_store2(v2f d, v4i rsrc, int voff, int soff, int aux) __asm("llvm.amdgcn.raw.buffer.store.v2f32");

struct VWArgs {                 // = SpecArgs (vnd_spec.hpp)
    const float *x;
    float *y;
    long long n;             // frames per stream
    int tiles_total;         // ceil(n / T)
    int tiles_per_span;
    int spans;               // spans per stream
    unsigned nblocks;        // workgroups launched
    unsigned units;          // (stream, span, channel pair) units: workgroup w takes units w, w + nblocks, ...
    int epi_ms_encode;       // VW_EPI: the decorrelate stage's pointwise steps in the store phase
    int epi_use_width;
    float epi_w_mid, epi_w_side;
    // One round of workgroups over a small launch (units == nblocks == CUs x chunk_rounds): a CU's co-resident workgroups share a
    // CHUNK of chunk_tiles consecutive tiles of one stream; the one dispatched first takes chunk_len0 of them, the next the rest
    // (chunk_tiles == 0: uniform spans, units walked as above)
    int chunk_tiles, chunk_len0, chunks_per_stream, cus_per_xcd;
    int stagger_ticks;       // a CU's second workgroup starts its prologue this many 100 MHz ticks after it enters the kernel
    int chunk_prio;          // 1: a CU's first-dispatched workgroup (the longer piece: the launch's critical path) runs at raised wave priority
    // BALANCED cut (stereo, uniform spans that would fill the resident workgroups unevenly): bal_total = streams x tiles_total > 0 - logical
    // workgroup L of nblocks walks the pool's tiles [L * bal_total / nblocks, (L + 1) * bal_total / nblocks), stream by stream: every
    // workgroup the same number of tiles (+- 1), a range that crosses into the next stream pays one more ring fill
    int bal_total;
    // VW_EPI, 32-frame runs: a wave's 64 runs are one 2048-frame block of the exact RMS sums (vnd_epilogue.hpp, rms_par_*): its sums of
    // squares of x and of the finished y, [stream][x0 x1 y0 y1][block] - the float64 PREDICTIONS the block-parallel sums start from
    // (every step of those is verified against the running sum: the values need not be the reference's, only close)
    double *epi_blk_sum;
    int epi_nblocks;
    int epi_rows_major;      // 1: [stream][block][x0 x1 y0 y1] instead - the rows epilogue_reduce_kernel adds up (the fused fast stage)
    // PACING of a CU's two co-resident workgroups (one round of persistent workgroups): the SIMDs issue the OLDER wave first, so the
    // workgroup a CU received first runs at nearly full speed and the second in what that leaves - cfg3: tile periods 17.9 against 30 us,
    // the first workgroups done at 300 us of a 440 us launch, half the SIMD slots idle behind them (profiles/r04_pacing.txt).  Each
    // workgroup publishes its count of finished tiles in its CU's slot pair and reads its partner's: the one BEHIND runs its next tile at
    // raised wave priority.  pace: [CU index][2] counters in device memory (never reset: a stale count only costs the first tile its bias)
    unsigned *pace;
};

struct VWPace { unsigned *mine; const unsigned *other; unsigned done; };

constexpr int VW_NW = VW_NT / 64;
constexpr int VW_QC = VW_M / 4;                 // 16-byte chunks per entry and channel
constexpr int VW_NH = VW_S ? VW_NT / 2 : VW_Q ? VW_NT / (4 * VW_Q) : VW_NT;  // lanes - and ring entries of a tile - per channel pair
constexpr int VW_T = VW_NH * VW_M;              // frames per tile
constexpr int VW_LPE = VW_Q ? VW_M * VW_Q : VW_M / 2;  // lanes of a 1 KB global access that fall into one entry (a lane moves a frame pair; VW_Q: one frame of four channels)
constexpr int VW_EPI_N = 64 / VW_LPE;           // entries per 1 KB global access
constexpr int VW_NI = VW_M / 2;                 // 1 KB global accesses per wave and tile
constexpr int VW_NPL = 2;                       // plane sets in LDS: one per output channel (the store phase transposes both channels' runs through them)
constexpr int VW_NXP = (VW_BC && !VW_S) ? 1 : 2; // ... of them holding INPUT: a mono input is staged once for both outputs (in the split form into both sets)
constexpr int VW_CH = VW_QC * VW_PLANE;         // byte offset of channel 1's planes
constexpr int VW_CX = VW_BC ? 1 : VW_C;         // interleaved INPUT channels
// channel pairs (VW_Q: quads or octets): one per workgroup and span.  4k + 2 channels (6, 10, ...) as QUADS: k full quads and one more that
// starts at channel C - 4 - it overlaps its neighbour in one channel pair, which both workgroups compute and write with the same bits
// (a frame's 16 bytes per access instead of the pair form's 8, for (k + 1) / (k + 1/2) of the arithmetic)
constexpr int VW_PAIRS = VW_Q ? (VW_C + 4 * VW_Q - 1) / (4 * VW_Q) : VW_C / 2;
constexpr int VW_PAIRB = 2 * VW_CH;             // VW_Q: byte offset of the second pair's plane sets
constexpr int VW_QUADB = 2 * VW_PAIRB + VW_QUADPAD; // octets: ... of the second QUAD's (shifted by 16 bytes: the two quads of a frame - neighbouring lanes of the 4-byte staging accesses - in different banks)
static_assert(VW_C >= 2 && VW_C % 2 == 0 && (VW_C == 2 || !VW_BC) && (VW_C == 2 || VW_Q || !VW_EPI), "whole channel pairs; fan-out and fused pointwise steps are stereo (quads / octets: the normaliser's sums only)");
static_assert(VW_Q == 0 || VW_Q == 1 || VW_Q == 2, "pairs, quads or octets");
static_assert(!VW_S || (VW_C == 2 && !VW_Q && !VW_EPI && VW_NT % 128 == 0 && VW_M >= 16), "split form: a stereo table, whole waves per channel");
static_assert(!VW_Q || ((VW_C % (4 * VW_Q) == 0 || (VW_Q == 1 && VW_C % 4 == 2 && VW_C >= 6)) && VW_NT % (256 * VW_Q) == 0 && VW_M * VW_Q <= 64 && VW_M <= 32), "quad / octet form: whole channel quads (4k + 2 channels: the last quad overlaps), whole waves per channel");
static_assert(VW_M == 16 || VW_M == 32 || VW_M == 64, "run length");
constexpr int VW_NBT = VW_NB + VW_TAIL;          // base registers per channel: the ring's, then one per entry offset that reaches into the tail
static_assert(VW_NT % 64 == 0 && VW_R >= VW_NH && VW_R + VW_TAIL == VW_NH + VW_DE && (VW_TAIL == 0 || (VW_Q && VW_R % 16 == 0)), "ring (+ tail) = tile + halo");
static_assert(VW_NB * VW_G > VW_DE, "bases cover the halo");
static_assert((VW_PLANE / 16) >= VW_R + VW_G + VW_TAIL, "plane stride: room for ring + mirror (+ tail)");
static_assert((VW_QC - 1) * VW_PLANE + VW_G * 16 < 65536 && VW_CH < 65536, "ds offset field is 16 bits");
static_assert((VW_Q ? 2 * VW_Q : 1) * VW_NPL * VW_QC * VW_PLANE + VW_QUADPAD <= 160 * 1024 && VW_QUADPAD % 16 == 0, "LDS");

// Raw buffer descriptor (stride 0): num_records = bytes left in the stream, so loads past the end of
// the stream return 0 (the reference's dropped terms, decorrelation.py:656-658) and stores past it
// are discarded.  Built from kernel arguments, blockIdx and the tile counter only: lives in SGPRs.
__device__ __forceinline__ v4i vw_rsrc(const void *base, long long bytes)
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

// blocks b and b + 8 share an XCD (and its L2): give one XCD consecutive logical ids, so that neighbouring
// spans (whose halos overlap) share an L2
__device__ __forceinline__ unsigned vw_xcd_remap(unsigned b, unsigned nwg)
{
    const unsigned q = nwg >> 3, r = nwg & 7u, xcd = b & 7u;
    const unsigned start = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return start + (b >> 3);
}

// (a mod R) for a < 2R, without a comparison: a - R wraps past 2^32 when a < R
__device__ __forceinline__ unsigned vw_wrap(unsigned a)
{
    const unsigned b = a - (unsigned)VW_R;
    return a < b ? a : b;
}

// one frame pair as {f0.c0, f0.c1, f1.c0, f1.c1}; a mono input fills the slots of channel 0.  In a wider signal the
// descriptor starts at the workgroup's channel pair: its 8 bytes of frames 2*pair and 2*pair + 1
__device__ __forceinline__ v4f vw_load_pair(v4i rsrc, int pair)
{
    if constexpr (VW_BC) {
        const v2f a = vw_load2(rsrc, pair * 8, 0, VW_LOAD_AUX);
        return v4f{a.x, 0.0f, a.y, 0.0f};
    } else if constexpr (VW_C == 2) {
        return vw_load4(rsrc, pair * 16, 0, VW_LOAD_AUX);
    } else {
        const v2f a = vw_load2(rsrc, pair * (VW_C * 8), 0, VW_LOAD_AUX), b = vw_load2(rsrc, pair * (VW_C * 8) + VW_C * 4, 0, VW_LOAD_AUX);
        return v4f{a.x, a.y, b.x, b.y};
    }
}

__device__ __forceinline__ void vw_store_pair(v4f v, v4i rsrc, int pair, int aux)
{
    if constexpr (VW_C == 2) {
        vw_store4(v, rsrc, pair * 16, 0, aux);
    } else {
        vw_store2(v2f{v.x, v.y}, rsrc, pair * (VW_C * 8), 0, aux);
        vw_store2(v2f{v.z, v.w}, rsrc, pair * (VW_C * 8) + VW_C * 4, 0, aux);
    }
}

// the staged pair goes to the channel planes (de-interleaved): 8 bytes each at `at` (chunk plane + entry + half)
__device__ __forceinline__ void vw_write_pair(vw_lchar *at, v4f v)
{
    *(vw_lv2f *)at = v2f{v.x, v.z};
    if constexpr (!VW_BC) *(vw_lv2f *)(at + VW_CH) = v2f{v.y, v.w};
}

#define VW_RD(base, imm) (*(const volatile vw_lv4f *)((base) + (imm)))
#define VW_FMA(x, w, a) __builtin_elementwise_fma((x), v2f{(w), (w)}, (a))
#define VW_MUL(x, w) ((x) * v2f{(w), (w)})
#define VW_SB __builtin_amdgcn_sched_barrier(0)
// One-element sums of the exact mode as opaque single instructions (2 cycles each): written in C, hipcc re-vectorises two
// of them into a v_pk_mov_b32 + v_pk_add_f32 (8 cycles, and a register file full of shuffled temporaries)
__device__ __forceinline__ float vw_add1(float a, float b)
{
    float r;
    asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float vw_sub1(float a, float b)
{
    float r;
    asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// (a.y, b.x) in ONE instruction: the exact mode's input pairs that start at an odd element (hipcc often takes two v_mov_b32)
__device__ __forceinline__ v2f vw_pair(v2f a, v2f b)
{
    v2f r;
    asm("v_pk_mov_b32 %0, %1, %2 op_sel:[1,0]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

//@@VW_TAPS@@

#if VW_STAMPS
// diagnosis (VND_WIN_STAMPS under VND_TUNING; tools/win_stamps.py): wave 0 of the first VW_STAMPS workgroups leaves the 100 MHz
// wall clock at its phase boundaries (first unit only) - [0] start, [1] ring filled, then for each of the first two tiles: taps done,
// (window dead: not kept), outputs exchanged, refill published; [14] the wave's stores acknowledged; [15] = HW_ID | XCC_ID << 32.  The stamps wait in SGPRs until the span is done
// (the kernel lives within a few VGPRs of its budget: a store per stamp made hipRTC's build spill).
__device__ unsigned long long vw_stamps[VW_STAMPS * 16];
#if VW_STAMP_PHASES
#define VW_STAMP_DECL unsigned vw_st[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}
#define VW_STAMP(k) do { vw_st[k] = (unsigned)__builtin_amdgcn_s_memrealtime(); } while (0)
// ([12] = the workgroup's entry into the kernel, [13] = its exit (stores acknowledged), both written by the kernel function:
//  with VW_STAMP_PHASES 0 these two are all there is, and nothing is held in registers across the span)
#define VW_STAMP_FLUSH(on) do { if (on) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); const unsigned long long end_ = __builtin_amdgcn_s_memrealtime(); if (threadIdx.x == VW_STAMP_WAVE * 64) { _Pragma("unroll") for (int q_ = 0; q_ < 12; ++q_) vw_stamps[blockIdx.x * 16 + q_] = vw_st[q_] ? (end_ - (unsigned long long)((unsigned)end_ - vw_st[q_])) : 0ull; vw_stamps[blockIdx.x * 16 + 14] = end_; } } } while (0)
#define VW_STAMP_TILE(t, k) do { if ((k) != 1 || VW_Q) { const unsigned now_ = (unsigned)__builtin_amdgcn_s_memrealtime(); _Pragma("unroll") for (int q_ = 0; q_ < 2; ++q_) if ((t) == q_) vw_st[2 + 4 * q_ + (k)] = now_; } } while (0)
#endif
#endif
#if !VW_STAMPS || !VW_STAMP_PHASES
#define VW_STAMP_DECL
#define VW_STAMP(k)
#define VW_STAMP_TILE(t, k)
#define VW_STAMP_FLUSH(on)
#endif

#if VW_EPI
// VelvetNoise.decorrelate's pointwise steps on one stereo frame, in the reference's float32 operation order
// (utils/dsp.py:59-63 side-channel encode, :34-37 stereo width; built with -ffp-contract=off)
__device__ __forceinline__ v2f vw_pointwise1(const VWArgs &a, v2f y, v2f x)          // one frame: {L, R}
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
#endif

template <int PG>
__device__ __forceinline__ void vw_span(const VWArgs &a, vw_lchar *lds, long long stream, int t_first, int ntiles, int flags, VWPace &pace)
{
    const int tid = threadIdx.x;
    const int ln = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long f0 = (long long)t_first * VW_T;
    // (the descriptors start at the channel pair: PGX / PG * 8 bytes into the first frame, and end as much before
    //  the end of the stream's last frame - inside the pair's last 8 bytes' frame, never in the next stream)
    constexpr int PGX = VW_BC ? 0 : PG;
    const float *xs = a.x + (stream * a.n + f0) * VW_CX + 2 * PGX;
    float *ys = a.y + (stream * a.n + f0) * VW_C + 2 * PG;
    const long long bytes_left_y = (a.n - f0) * (VW_C * 4) - 8 * PG;
    const long long bytes_left_x = (a.n - f0) * (VW_CX * 4) - 8 * PGX;
    // what this span reads: its tiles plus the last tile's halo (the entries prefetched past it are never
    // read, and an out-of-range buffer load moves no data)
    const long long need = ((long long)ntiles * VW_T + (long long)VW_DE * VW_M) * (VW_CX * 4) - 8 * PGX;
    const long long bytes_need = need < bytes_left_x ? need : bytes_left_x;

    // a lane's part in a 1 KB global access (frame pair 64*m + lq of the wave's 64*M frames): entry m*EPI_N + lane_e,
    // chunk plane and half in lane_at.
    // WHICH pair of the 64 a lane moves is a matter of LDS banks: its 8-byte staging writes go 16 lanes at a time into 32
    // banks, its read-backs 32 lanes at a time into 64.  With 32-frame runs (a pair index is entry : chunk : half = 2 : 3 : 1
    // bits) and planes 2 mod 4 slots apart, lanes 0-15 must hold chunks 0-3 of two entries and lanes 16-31 chunks 4-7: the
    // pair index with bits 3 and 4 exchanged.  Both kinds of access then touch every bank once (SQ_LDS_BANK_CONFLICT,
    // profiles/r03_lds_conflicts.txt); the global access is the same 1 KB, its 128-byte lines taken by other lane octets.
#if VW_LANE_SWIZZLE
    const int lq = (ln & ~24) | ((ln & 8) << 1) | ((ln & 16) >> 1);
#else
    const int lq = ln;
#endif
    const int lane_e = lq / VW_LPE;
    const int lane_at = ((lq % VW_LPE) >> 1) * VW_PLANE + (lq & 1) * 8;
    const int lane_slot = (lq % VW_LPE) * VW_PLANE;                    // (VW_XPOSE_PAIRS: the pair's 16-byte slot of its entry)
    // ... and in a 1 KB LOAD.  Stereo: as above.  A mono input (VW_BC): 4 frames = one whole 16-byte chunk of an entry per lane (8-byte
    // loads cost the memory pipeline 1.4-1.8x per byte), 256 frames = 256 / M entries per access, half as many accesses; plane set 0 only
    constexpr int NIN = VW_BC ? VW_NI / 2 : VW_NI;                       // loads per wave and tile (its 64 entries: M/2 KB of stereo, M/4 KB of mono frames)
    constexpr int EIN = VW_BC ? 256 / VW_M : VW_EPI_N;                   // ring entries per load
    const int in_e = VW_BC ? ln / (VW_M / 4) : lane_e;
    const int in_at = VW_BC ? (ln % (VW_M / 4)) * VW_PLANE : lane_at;
    auto load_in = [&](v4i rsrc, int m, int lq_now) -> v4f {
        if constexpr (VW_BC) return vw_load4(rsrc, m * 1024 + ln * 16, 0, VW_LOAD_AUX);
        else return vw_load_pair(rsrc, 64 * m + lq_now);
    };
    auto stage = [&](vw_lchar *at, v4f v) {
        if constexpr (VW_BC) *(vw_lv4f *)at = v;
        else vw_write_pair(at, v);
    };

    // ---- prologue: entries 0 .. R-1 (the first tile's window) into ring positions 0 .. R-1 ----------------
    {
        const v4i rx = vw_rsrc(xs, bytes_need);
        constexpr int NFILL = (VW_R + EIN - 1) / EIN;                    // 1 KB accesses that cover R entries
        constexpr int PER = (NFILL + VW_NW - 1) / VW_NW;                 // per wave
        constexpr int BATCH = 8;
        for (int k0 = 0; k0 < PER; k0 += BATCH) {
            v4f w[BATCH];
#pragma unroll
            for (int kk = 0; kk < BATCH; ++kk) {
                const int i = wv + VW_NW * (k0 + kk);
                w[kk] = load_in(rx, i, lq);                              // accesses past NFILL are masked at the write
            }
#pragma unroll
            for (int kk = 0; kk < BATCH; ++kk) {
                const int i = wv + VW_NW * (k0 + kk);
                const int e = i * EIN + in_e;
                if (k0 + kk < PER && e < VW_R) {
                    stage(lds + in_at + e * 16, w[kk]);
                    if (e < VW_G) stage(lds + in_at + (e + VW_R) * 16, w[kk]);
                }
            }
        }
    }
    // the frames that will replace this wave's own entries after the first tile: entries R + 64*wv ...
    v4f pre[NIN];
    {
        const long long f = ((long long)VW_R + 64 * wv) * VW_M;
        const v4i rx = vw_rsrc(xs + f * VW_CX, bytes_need - f * (VW_CX * 4));
#pragma unroll
        for (int m = 0; m < NIN; ++m) pre[m] = load_in(rx, m, lq);
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

    bool hi = (flags & 2) != 0;                                          // (wave-uniform) raised priority: a chunk's first workgroup - or, paced, the one behind
    if (hi) __builtin_amdgcn_s_setprio(2);
    unsigned p0 = 0;                                                     // ring position of the tile's first entry
    for (int t = 0; t < ntiles; ++t) {
        const unsigned pw = vw_wrap(p0 + 64u * (unsigned)wv);            // ... of this wave's first entry
        const unsigned pl = vw_wrap(p0 + (unsigned)tid);                 // ... of this lane's own entry
        // (a lane's pair number in a 1 KB access and its entry in it: opaque per tile, so that hipcc does not hoist
        //  their sums with every access number out of the tile loop - 2 x M/2 registers held through the tap phase, vw_span_s)
        int lqo = lq;
        unsigned pwl = pw + (unsigned)lane_e, pwi = pw + (unsigned)in_e;
        asm volatile("" : "+v"(lqo), "+v"(pwl));
        if constexpr (VW_BC) asm volatile("" : "+v"(pwi));
        float o0[VW_M], o1[VW_M];
        {
            // base k = the entry k*G past the lane's own, wrapped; the immediates reach G-1 entries further (mirror)
            vw_lchar *b[2][VW_NBT];
#pragma unroll
            for (int k = 0; k < VW_NB; ++k) {
                b[0][k] = lds + vw_wrap(pl + (unsigned)(k * VW_G)) * 16u;
                b[1][k] = b[0][k] + (VW_BC ? 0 : VW_CH);
            }
            vw_taps_of<PG>(b, o0, o1);
        }
#pragma unroll
        for (int j = 0; j < VW_M; ++j) { asm volatile("" : "+v"(o0[j])); asm volatile("" : "+v"(o1[j])); }
#if VW_EPI
        // the run's own input frames are still in the lane's entry: fetched before the barrier
        v4f xin[VW_NXP][VW_QC];
#pragma unroll
        for (int c = 0; c < VW_NXP; ++c)
#pragma unroll
            for (int r = 0; r < VW_QC; ++r) xin[c][r] = VW_RD(lds + pl * 16u, c * VW_CH + r * VW_PLANE);
#pragma unroll
        for (int j = 0; j < VW_M; ++j) {
            const v2f xf = {xin[0][j / 4][j % 4], xin[VW_NXP - 1][j / 4][j % 4]};
            const v2f yf = vw_pointwise1(a, v2f{o0[j], o1[j]}, xf);
            o0[j] = yf.x; o1[j] = yf.y;
        }
        if constexpr (VW_M == 32) {
            if (a.epi_blk_sum != nullptr) {                              // (wave-uniform)
                float sq[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int j = 0; j < VW_M; ++j) {
                    const float x0 = xin[0][j / 4][j % 4], x1 = xin[VW_NXP - 1][j / 4][j % 4];
                    sq[0] += x0 * x0; sq[1] += x1 * x1; sq[2] += o0[j] * o0[j]; sq[3] += o1[j] * o1[j];
                }
                // a lane's 32 squares add up in float32 (relative error <= 32 * 2^-24, independent between lanes); from there on - across
                // the wave here, across blocks in epilogue_reduce_kernel - the sums are float64: in the fully fused FAST stage these
                // are the normaliser's actual sums (rows_major), in the exact stage predictions that the tally verifies
                double tot[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    double v = (double)sq[c];
#pragma unroll
                    for (int sh = 32; sh > 0; sh >>= 1) {
                        const unsigned long long bits = __builtin_bit_cast(unsigned long long, v);
                        const unsigned lo = (unsigned)__builtin_amdgcn_ds_bpermute((ln ^ sh) << 2, (int)(unsigned)bits);
                        const unsigned up = (unsigned)__builtin_amdgcn_ds_bpermute((ln ^ sh) << 2, (int)(unsigned)(bits >> 32));
                        v += __builtin_bit_cast(double, ((unsigned long long)up << 32) | lo);
                    }
                    tot[c] = v;
                }
                const int blk = (t_first + t) * (VW_T / 2048) + wv;
                if (ln == 0 && blk < a.epi_nblocks) {
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        a.epi_blk_sum[a.epi_rows_major ? (stream * a.epi_nblocks + blk) * 4 + c : (stream * 4 + c) * a.epi_nblocks + blk] = tot[c];
                }
            }
        }
#endif
        // X. every wave is done reading this tile's window: the tile's own entries are dead
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        // the store / refill phase is a chain of round trips with a handful of instructions between them: ahead of the other
        // workgroup's tap phase in the SIMD's arbitration, it ends sooner and costs that tap phase next to nothing
        // (priority 1 against none: cfg2 +1.0 % fast, +0.5 % exact; cfg3 unchanged - tools/closed/win_phase_try.py)
        if (hi) __builtin_amdgcn_s_setprio(3);
        else __builtin_amdgcn_s_setprio(1);
        unsigned seen = 0;                                               // (pacing: the partner's count, in flight through the store phase)
        if (pace.other != nullptr) seen = __hip_atomic_load(pace.other, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

        // transposition through the lane's own (dead) entry: planar runs in, interleaved frame pairs out.
        // (A mono input's ring uses plane set 0 only; set 1 is there for channel 1's runs to cross: one pass, as for a stereo input.)
        const long long fo = (long long)t * VW_T + 64 * wv * VW_M;       // the wave's first output frame
        const v4i ry = vw_rsrc(ys + fo * VW_C, bytes_left_y - fo * (VW_C * 4));
        const long long fi = ((long long)(t + 1) * VW_NT + VW_R + 64 * wv) * VW_M;     // the refill after the NEXT tile
        const v4i rx = vw_rsrc(xs + fi * VW_CX, bytes_need - fi * (VW_CX * 4));
        constexpr int ST_AUX = VW_NT_STORES ? VW_NT_STORE_AUX : 0;
        // (read-back and store go one 1 KB access at a time: issuing all the read-backs first was measured - no faster,
        //  the other workgroup of the CU covers the round trips - and costs 80 more registers in this phase)
        if constexpr (VW_XPOSE_PAIRS) {
            // the dead entry's 2*QC slots of 16 bytes (the planes of both channels, CH = QC planes on) take the lane's run as
            // interleaved FRAME PAIRS - slot k = frames 2k, 2k+1 of both channels - so that the read-back is one 16-byte read
            // per global store, already in memory order
#pragma unroll
            for (int k = 0; k < 2 * VW_QC; ++k)
                *(vw_lv4f *)(lds + pl * 16u + k * VW_PLANE) = v4f{o0[2 * k], o1[2 * k], o0[2 * k + 1], o1[2 * k + 1]};
#pragma unroll
            for (int m = 0; m < VW_NI; ++m) {
                const v4f v = *(const volatile vw_lv4f *)(lds + lane_slot + vw_wrap(pwl + (unsigned)(m * VW_EPI_N)) * 16u);
                vw_store_pair(v, ry, 64 * m + lqo, ST_AUX);
            }
        } else {
#pragma unroll
            for (int r = 0; r < VW_QC; ++r) {
                *(vw_lv4f *)(lds + pl * 16u + r * VW_PLANE) = v4f{o0[4 * r], o0[4 * r + 1], o0[4 * r + 2], o0[4 * r + 3]};
                *(vw_lv4f *)(lds + pl * 16u + VW_CH + r * VW_PLANE) = v4f{o1[4 * r], o1[4 * r + 1], o1[4 * r + 2], o1[4 * r + 3]};
            }
#pragma unroll
            for (int m = 0; m < VW_NI; ++m) {
                vw_lchar *at = lds + lane_at + vw_wrap(pwl + (unsigned)(m * VW_EPI_N)) * 16u;
                const v2f r0 = *(const volatile vw_lv2f *)at, r1 = *(const volatile vw_lv2f *)(at + VW_CH);
                vw_store_pair(v4f{r0.x, r1.x, r0.y, r1.y}, ry, 64 * m + lqo, ST_AUX);
            }
        }
        // refill: the frames prefetched a tile ago take the place of the wave's own entries (LDS operations of
        // one wave execute in order: the read-back above is ahead of these writes), and the next prefetch starts.
        // The mirror of the ring's first G entries is rewritten only by the wave whose entries include them.
        // (the last tile of the workgroup's last unit refills nothing and waits for nobody: its stores are the wave's last work)
        const bool fin = (flags & 1) != 0 && t == ntiles - 1;
        if (!fin) {
            const bool mirror = pw < (unsigned)VW_G || pw + 64u > (unsigned)VW_R;            // wave-uniform
#pragma unroll
            for (int m = 0; m < NIN; ++m) {
                const unsigned e = vw_wrap((VW_BC ? pwi : pwl) + (unsigned)(m * EIN));
                vw_lchar *at = lds + in_at + e * 16u;
                stage(at, pre[m]);
                if (mirror) { if (e < (unsigned)VW_G) stage(at + VW_R * 16, pre[m]); }
                pre[m] = load_in(rx, m, lqo);
            }
        }
        p0 = p0 + VW_NT >= VW_R ? p0 + VW_NT - VW_R : p0 + VW_NT;
        pace.done += 1;
        if (pace.other != nullptr) {
            if (threadIdx.x == 0) __hip_atomic_store(pace.mine, pace.done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            hi = (unsigned)__builtin_amdgcn_readfirstlane((int)seen) > pace.done;       // the partner is ahead: this workgroup's next tile goes first
        }
        if (hi) __builtin_amdgcn_s_setprio(2);
        else __builtin_amdgcn_s_setprio(0);
        // Y. the refill is in place for every wave's window (and, after the last tile, the ring is free for the next unit)
        if (!fin) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
    if (hi) __builtin_amdgcn_s_setprio(0);
}

#if VW_Q
// ---- QUADS and OCTETS: 16 / 32 bytes of every frame ---------------------------------------------------------
// A signal of 4k interleaved channels is 16k bytes per frame; a workgroup that owns one channel PAIR moves 8 of them, and
// 8-byte pieces cost the memory pipeline 1.7x (loads) to 3.8x (stores) what whole 16-byte accesses cost
// (profiles/r03_cfg5_request_floor.txt).  Here a workgroup owns a channel QUAD (VW_Q 1) or OCTET (VW_Q 2: two neighbouring
// quads - with 8 channels whole frames, whole cache lines) of a span, and every global access is 64 lanes x 16 bytes: a lane
// moves one frame's quad.  Its waves are split over the CHANNELS (NT / 4Q lanes = ring entries of a tile per channel, tap
// functions vw_taps_<pair>c<channel>): one channel's accumulators per lane, 32-frame runs.  The 64 ring entries that the 4Q
// partner waves (same wave index, one per channel) compute are staged and stored by those same waves, 64 / 4Q entries of ALL
// channels each; outputs cross the partner waves as planar runs through the tile's dead entries (one barrier more than the
// stereo form), the refill stays wave-private, in LDS program order.
// (Round 3 also had a wave per channel PAIR - 16-frame runs, 3.4 B of LDS per FMA against 2.6: cfg5 0.333-0.348 against 0.318 ms,
//  profiles/r03_cfg5_octets.txt - and partner quads placed on one CU, which changed nothing: both removed in round 4.)
__device__ __forceinline__ void vw_write_quad(vw_lchar *at, v4f v)
{
    *(vw_lfloat *)at = v.x;
    *(vw_lfloat *)(at + VW_CH) = v.y;
    *(vw_lfloat *)(at + VW_PAIRB) = v.z;
    *(vw_lfloat *)(at + VW_PAIRB + VW_CH) = v.w;
}

#endif

#if VW_Q
template <int QD>
__device__ __forceinline__ void vw_span_qc(const VWArgs &a, vw_lchar *lds, long long stream, int t_first, int ntiles, int flags, VWPace &pace)
{
    constexpr int Q = VW_Q, NCH = 4 * Q;                                 // quads and channels of the workgroup
    constexpr int NWH = VW_NW / NCH;                                     // waves per channel
    constexpr int FB = VW_C * 4;                                         // bytes per frame
    constexpr int WE = 64 / NCH;                                         // entries (of every channel) a wave stages and stores per tile
    constexpr int FPA = 64 / Q;                                          // frames per 64-lane access
    constexpr int NI = VW_M / 4;                                         // accesses per wave and tile
    static_assert(NWH >= 1 && WE % VW_EPI_N == 0 && WE / VW_EPI_N == NI, "a wave's share of a tile in whole accesses");
    const int tid = threadIdx.x;
    const int ln = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pc = wv / NWH;                                             // the wave's channel of the workgroup's NCH
    const int wl = wv - pc * NWH;
    const int tl = wl * 64 + ln;                                         // the entry of a tile this LANE computes (in its channel)
    const int we = wl * 64 + pc * WE;                                    // the first of the WE entries this WAVE stages and stores (all channels)
    const long long f0 = (long long)t_first * VW_T;
    constexpr int CH0 = (VW_C % (4 * Q) != 0 && QD == VW_PAIRS - 1) ? VW_C - 4 * Q : 4 * Q * QD;      // the workgroup's first channel of the frame
    const float *xs = a.x + (stream * a.n + f0) * VW_C + CH0;
    float *ys = a.y + (stream * a.n + f0) * VW_C + CH0;
    const long long bytes_left = (a.n - f0) * FB - 4 * CH0;
    const long long need = ((long long)ntiles * VW_T + (long long)VW_DE * VW_M) * FB - 4 * CH0;
    const long long bytes_need = need < bytes_left ? need : bytes_left;
    const int lane_f = ln / Q, lane_q = ln % Q;
    const int lane_e = lane_f / VW_M, lane_j = lane_f % VW_M;
    const int lane_g = lane_f * FB + lane_q * 16;                        // byte offset in the access
    const int lane_at = lane_q * VW_QUADB + (lane_j >> 2) * VW_PLANE + (lane_j & 3) * 4;     // one float per channel plane
#if VW_STAMPS && VW_STAMP_PHASES
    const bool vw_stamp_on = blockIdx.x < VW_STAMPS && (unsigned)((stream * a.spans + t_first / a.tiles_per_span) * VW_PAIRS + QD) == vw_xcd_remap(blockIdx.x, a.nblocks);
    if (vw_stamp_on && threadIdx.x == 0) {
        unsigned hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        vw_stamps[blockIdx.x * 16 + 15] = (unsigned long long)hw | ((unsigned long long)xcc << 32);
    }
#endif
    VW_STAMP_DECL;
    VW_STAMP(0);

    {
        const v4i rx = vw_rsrc(xs, bytes_need);
        constexpr int NFILL = (VW_R + VW_TAIL + VW_EPI_N - 1) / VW_EPI_N;      // (the tail's entries follow the ring's in the stream)
        constexpr int PER = (NFILL + VW_NW - 1) / VW_NW;
        constexpr int BATCH = 8;
        for (int k0 = 0; k0 < PER; k0 += BATCH) {
            v4f w[BATCH];
#pragma unroll
            for (int kk = 0; kk < BATCH; ++kk) {
                const int i = wv + VW_NW * (k0 + kk);
                w[kk] = vw_load4(rx, i * (FPA * FB) + lane_g, 0, VW_LOAD_AUX);
            }
#pragma unroll
            for (int kk = 0; kk < BATCH; ++kk) {
                const int i = wv + VW_NW * (k0 + kk);
                const int e = i * VW_EPI_N + lane_e;
                if (k0 + kk < PER && e < VW_R + VW_TAIL) {
                    vw_write_quad(lds + lane_at + (e < VW_R ? e : e + VW_G) * 16, w[kk]);      // ring slot e, or tail slot behind the mirror
                    if (e < VW_G) vw_write_quad(lds + lane_at + (e + VW_R) * 16, w[kk]);
                }
            }
        }
    }
    v4f pre[NI];
    {
        const long long f = ((long long)VW_R + we) * VW_M;
        const v4i rx = vw_rsrc(xs + f * VW_C, bytes_need - f * FB);
#pragma unroll
        for (int m = 0; m < NI; ++m) pre[m] = vw_load4(rx, m * (FPA * FB) + lane_g, 0, VW_LOAD_AUX);
    }
#if VW_TAIL
    // the TAIL: the window's last VW_TAIL entries, past the ring's 16-aligned length.  Tile t + 1's are the first entries of the refill
    // that follows tile t + 1 - needed a tile before the ring gets them: the first waves carry one access of them each, a tile ahead
    // of the ring's prefetch, and write it behind the mirror in tile t's store phase.
    constexpr int NTA = (VW_TAIL + VW_EPI_N - 1) / VW_EPI_N;
    static_assert(NTA <= VW_NW, "one tail access per wave");
    v4f tailreg = {0.0f, 0.0f, 0.0f, 0.0f};
    if (wv < NTA) {
        const long long f = ((long long)VW_NH + VW_R + wv * VW_EPI_N) * VW_M;            // tile 1's tail
        tailreg = vw_load4(vw_rsrc(xs + f * VW_C, bytes_need - f * FB), lane_g, 0, VW_LOAD_AUX);
    }
#endif
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    VW_STAMP(1);

    vw_lchar *const lp = lds + (pc >> 1) * VW_PAIRB + (pc >> 2) * VW_QUADPAD;   // the channel's pair: its plane sets
    unsigned p0 = 0;
    for (int t = 0; t < ntiles; ++t) {
        const unsigned pw = vw_wrap(p0 + (unsigned)we);
        const unsigned pl = vw_wrap(p0 + (unsigned)tl);
        // (per-access constants opaque per tile: not hoisted into the tap phase's registers, as in vw_span_s)
        int lg = lane_g;
        unsigned pwl = pw + (unsigned)lane_e;
        asm volatile("" : "+v"(lg), "+v"(pwl));
        float o[VW_M];
        {
            vw_lchar *b[2][VW_NBT];
#pragma unroll
            for (int k = 0; k < VW_NB; ++k) {
                b[0][k] = lp + vw_wrap(pl + (unsigned)(k * VW_G)) * 16u;
                b[1][k] = b[0][k] + VW_CH;
            }
#if VW_TAIL
            // entry offsets VW_R - VW_NH + 1 ... VW_DE: in the ring for the tile's first lanes, in the tail for its last ones
#pragma unroll
            for (int j = 0; j < VW_TAIL; ++j) {
                const unsigned d = (unsigned)(VW_R - VW_NH + 1 + j);
                const unsigned e = (unsigned)tl + d;                                         // entry of the tile's window
                b[0][VW_NB + j] = lp + (e < (unsigned)VW_R ? vw_wrap(pl + d) : e + (unsigned)VW_G) * 16u;
                b[1][VW_NB + j] = b[0][VW_NB + j] + VW_CH;
            }
#endif
            VW_TAPS_OF_CHANNEL(pc)
        }
#pragma unroll
        for (int j = 0; j < VW_M; ++j) asm volatile("" : "+v"(o[j]));
        VW_STAMP_TILE(t, 0);
#if VW_EPI
        // The normaliser's sums of squares (utils/dsp.py:107-109, LR mode on 4k channels: no pointwise step, a scale per channel) leave
        // here: the lane's run of INPUT frames is still in its entry of the channel's planes (the outputs overwrite it below), the finished
        // outputs are in registers.  A lane's 32 squares add up in float32, the wave and everything after in float64; one row of 2 C
        // sums per (tile, wave of the channel): rows for epilogue_reduce_kernel.  Frames past the stream's end were loaded as zeros.
        if (a.epi_blk_sum != nullptr) {                                  // (wave-uniform)
            vw_lchar *const own = lp + (pc & 1) * VW_CH + pl * 16u;
            float sx = 0.0f, sy = 0.0f;
#pragma unroll
            for (int r = 0; r < VW_QC; ++r) {
                const v4f xin = VW_RD(own, r * VW_PLANE);
                sx += xin.x * xin.x; sx += xin.y * xin.y; sx += xin.z * xin.z; sx += xin.w * xin.w;
            }
#pragma unroll
            for (int j = 0; j < VW_M; ++j) sy += o[j] * o[j];
            double tot[2] = {(double)sx, (double)sy};
#pragma unroll
            for (int c = 0; c < 2; ++c) {
#pragma unroll
                for (int sh = 32; sh > 0; sh >>= 1) {
                    const unsigned long long bits = __builtin_bit_cast(unsigned long long, tot[c]);
                    const unsigned lo = (unsigned)__builtin_amdgcn_ds_bpermute((ln ^ sh) << 2, (int)(unsigned)bits);
                    const unsigned up = (unsigned)__builtin_amdgcn_ds_bpermute((ln ^ sh) << 2, (int)(unsigned)(bits >> 32));
                    tot[c] += __builtin_bit_cast(double, ((unsigned long long)up << 32) | lo);
                }
            }
            const int row = (t_first + t) * NWH + wl;
            if (ln == 0 && row < a.epi_nblocks) {
                const int cg = CH0 + pc;                                 // the wave's channel of the frame
                if (a.epi_rows_major) {                                  // the fused fast stage's rows: [stream][row][x_0 .. x_C-1, y_0 .. y_C-1]
                    double *const at = a.epi_blk_sum + (stream * a.epi_nblocks + row) * (2 * VW_C) + cg;
                    at[0] = tot[0];
                    at[VW_C] = tot[1];
                } else {
                    // the exact stage's block-parallel sums (rms_par_*): [stream * C/2 + pair][x ch0, x ch1, y ch0, y ch1][block] - a wave's
                    // 2048-frame tile IS one of their blocks (VW_T == 2048, one wave per channel: checked where the plan attaches them)
                    double *const at = a.epi_blk_sum + ((stream * (VW_C / 2) + (cg >> 1)) * 4 + (cg & 1)) * (long long)a.epi_nblocks + row;
                    at[0] = tot[0];
                    at[2 * (long long)a.epi_nblocks] = tot[1];
                }
            }
        }
#endif
        // X. every wave is done reading this tile's window: the tile's own entries are dead (all channels).
        // With ONE wave per channel (NWH == 1: octets of 512 lanes, quads of 256) nobody else reads the channel's planes: the wave that
        // read the window is the one that overwrites it, in LDS program order - no barrier here, two per tile instead of three.
        if constexpr (NWH > 1) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        __builtin_amdgcn_s_setprio(1);
        vw_lchar *const mine = lp + (pc & 1) * VW_CH + pl * 16u;
#pragma unroll
        for (int r = 0; r < VW_QC; ++r)
            *(vw_lv4f *)(mine + r * VW_PLANE) = v4f{o[4 * r], o[4 * r + 1], o[4 * r + 2], o[4 * r + 3]};
        // X2. ... and the partner waves' (the other channels of the same 64 entries)
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        VW_STAMP_TILE(t, 2);
        const long long fo = (long long)t * VW_T + (long long)we * VW_M;
        const v4i ry = vw_rsrc(ys + fo * VW_C, bytes_left - fo * FB);
        const long long fi = ((long long)(t + 1) * VW_NH + VW_R + we) * VW_M;
        const v4i rx = vw_rsrc(xs + fi * VW_C, bytes_need - fi * FB);
        constexpr int ST_AUX = VW_NT_STORES ? VW_NT_STORE_AUX : 0;
#pragma unroll
        for (int m = 0; m < NI; ++m) {
            vw_lchar *at = lds + lane_at + vw_wrap(pwl + (unsigned)(m * VW_EPI_N)) * 16u;
            const float c0 = *(const volatile vw_lfloat *)at, c1 = *(const volatile vw_lfloat *)(at + VW_CH);
            const float c2 = *(const volatile vw_lfloat *)(at + VW_PAIRB), c3 = *(const volatile vw_lfloat *)(at + VW_PAIRB + VW_CH);
            vw_store4(v4f{c0, c1, c2, c3}, ry, lg + m * (FPA * FB), 0, ST_AUX);
        }
        VW_STAMP_TILE(t, 1);                                                          // (quads / octets: read-backs and stores issued)
        const bool fin = (flags & 1) != 0 && t == ntiles - 1;          // (as vw_span: nothing to refill, nobody to wait for)
        if (!fin) {
            const bool mirror = pw < (unsigned)VW_G || pw + (unsigned)WE > (unsigned)VW_R;    // wave-uniform
#pragma unroll
            for (int m = 0; m < NI; ++m) {
                const unsigned e = vw_wrap(pwl + (unsigned)(m * VW_EPI_N));
                vw_lchar *at = lds + lane_at + e * 16u;
                vw_write_quad(at, pre[m]);
                if (mirror) { if (e < (unsigned)VW_G) vw_write_quad(at + VW_R * 16, pre[m]); }
                pre[m] = vw_load4(rx, lg + m * (FPA * FB), 0, VW_LOAD_AUX);
            }
#if VW_TAIL
            if (wv < NTA) {                                                              // wave-uniform
                const unsigned e = (unsigned)(wv * VW_EPI_N) + (unsigned)lane_e;
                if (e < (unsigned)VW_TAIL) vw_write_quad(lds + lane_at + ((unsigned)(VW_R + VW_G) + e) * 16u, tailreg);      // tile t + 1's
                const long long ft = ((long long)(t + 2) * VW_NH + VW_R + wv * VW_EPI_N) * VW_M;                               // tile t + 2's
                tailreg = vw_load4(vw_rsrc(xs + ft * VW_C, bytes_need - ft * FB), lg, 0, VW_LOAD_AUX);
            }
#endif
        }
        p0 = p0 + VW_NH >= VW_R ? p0 + VW_NH - VW_R : p0 + VW_NH;
        __builtin_amdgcn_s_setprio(0);
        if (!fin) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        VW_STAMP_TILE(t, 3);
    }
    VW_STAMP_FLUSH(vw_stamp_on);
}
#endif

#if VW_S
// ---- the SPLIT form of a stereo signal: a wave computes ONE channel ---------------------------------------
// The plain form's lane carries both channels' work one after the other: E / P accumulators, the first channel's finished
// outputs and a tile of prefetched frames - ~240 registers, two waves per SIMD.  Here waves 0 .. NW/2-1 run channel 0's tap
// function (vw_taps_c0) on the tile's NT/2 entries and the other half channel 1's: per lane one channel's accumulators, half
// the prefetch - three waves per SIMD fit (two workgroups of 384 lanes per CU: 12 waves), on the same ring and the same
// 1 KB global accesses.  A frame's two channels now sit in two waves: outputs go as planar runs into the tile's dead
// entries, one barrier more, then each wave reads back and stores the 32 entries it also refills (as vw_span_qc).
template <int CH>
__device__ __forceinline__ void vw_taps_ch(vw_lchar *const (&b)[2][VW_NBT], float (&o)[VW_M])
{
    if constexpr (CH == 0) vw_taps_c0(b, o, o);
    else vw_taps_c1(b, o, o);
}

__device__ __forceinline__ void vw_span_s(const VWArgs &a, vw_lchar *lds, long long stream, int t_first, int ntiles, int flags, VWPace &pace)
{
    constexpr int NWH = VW_NW / 2;                                       // waves per channel
    constexpr int NI = VW_M / 4;                                         // 1 KB global STORES per wave and tile (64 frame pairs each)
    // VW_BC - a mono input fanned out: the one input channel is staged into BOTH plane sets (each output channel's waves read their own
    // copy with the tap functions of the stereo form unchanged), 16 bytes = 4 frames per lane and access: half as many input accesses,
    // each 256 frames = 256 / M ring entries (stereo: 128 frames)
    constexpr int NIN = VW_BC ? VW_M / 8 : VW_M / 4;                     // 1 KB global LOADS per wave and tile
    constexpr int EIN = VW_BC ? 256 / VW_M : VW_EPI_N;                   // ring entries per load
    constexpr int XB = VW_BC ? 4 : 8;                                    // input bytes per frame
    // the refill's frames: NE accesses are prefetched a tile ahead and held in registers through the tap phase, the other
    // LATE are loaded at the start of the store phase that consumes them (64-frame runs: the accumulators need the room)
    constexpr int LATE = VW_LATE < NIN ? VW_LATE : NIN - 1;
    constexpr int NE = NIN - LATE;
    static_assert(VW_LATE >= 0 && LATE < NIN, "late refill accesses");
    const int tid = threadIdx.x;
    const int ln = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pc = wv >= NWH ? 1 : 0;                                    // the wave's channel
    const int wl = wv - pc * NWH;
    const int tl = wl * 64 + ln;                                         // the entry of a tile this LANE computes (in its channel)
    const int we = wl * 64 + pc * 32;                                    // the first of the 32 entries this WAVE stages and stores (both channels)
    const long long f0 = (long long)t_first * VW_T;
    const float *xs = a.x + (stream * a.n + f0) * (XB / 4);
    float *ys = a.y + (stream * a.n + f0) * 2;
    const long long bytes_left = (a.n - f0) * 8;                         // (of the output)
    const long long need = ((long long)ntiles * VW_T + (long long)VW_DE * VW_M) * XB;
    const long long bytes_need = need < (a.n - f0) * XB ? need : (a.n - f0) * XB;
#if VW_LANE_SWIZZLE
    const int lq = (ln & ~24) | ((ln & 8) << 1) | ((ln & 16) >> 1);      // (as vw_span: the 8-byte staging writes and read-backs touch every bank once)
#else
    const int lq = ln;
#endif
    const int lane_e = lq / VW_LPE;
    const int lane_at = ((lq % VW_LPE) >> 1) * VW_PLANE + (lq & 1) * 8;
    // ... and in a 1 KB LOAD: stereo as above; mono - 4 frames = one 16-byte chunk of entry ln / (M / 4), written to both plane sets
    const int in_e = VW_BC ? ln / (VW_M / 4) : lane_e;
    const int in_at = VW_BC ? (ln % (VW_M / 4)) * VW_PLANE : lane_at;
    const int in16 = VW_BC ? ln * 16 : lq * 16;                          // the lane's byte offset in a load
    auto stage = [&](vw_lchar *at, v4f v) {
        if constexpr (VW_BC) { *(vw_lv4f *)at = v; *(vw_lv4f *)(at + VW_CH) = v; }
        else vw_write_pair(at, v);
    };
#if VW_STAMPS && VW_STAMP_PHASES
    const bool vw_stamp_on = blockIdx.x < VW_STAMPS && (a.chunk_tiles > 0 || a.bal_total > 0 || (unsigned)(stream * a.spans + t_first / a.tiles_per_span) == vw_xcd_remap(blockIdx.x, a.nblocks));
    if (vw_stamp_on && threadIdx.x == 0) {
        unsigned hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        vw_stamps[blockIdx.x * 16 + 15] = (unsigned long long)hw | ((unsigned long long)xcc << 32);
    }
#endif
    VW_STAMP_DECL;
    VW_STAMP(0);

    {
        const v4i rx = vw_rsrc(xs, bytes_need);
        constexpr int NFILL = (VW_R + EIN - 1) / EIN;
        constexpr int PER = (NFILL + VW_NW - 1) / VW_NW;
        constexpr int BATCH = 8;                                     // loads in flight per wave before the first staging write (all of them: no faster, run_r4c.sh)
        for (int k0 = 0; k0 < PER; k0 += BATCH) {
            v4f w[BATCH];
#pragma unroll
            for (int kk = 0; kk < BATCH; ++kk) {
                const int i = wv + VW_NW * (k0 + kk);
                w[kk] = vw_load4(rx, i * 1024 + in16, 0, VW_LOAD_AUX);
            }
#pragma unroll
            for (int kk = 0; kk < BATCH; ++kk) {
                const int i = wv + VW_NW * (k0 + kk);
                const int e = i * EIN + in_e;
                if (k0 + kk < PER && e < VW_R) {
                    stage(lds + in_at + e * 16, w[kk]);
                    if (e < VW_G) stage(lds + in_at + (e + VW_R) * 16, w[kk]);
                }
            }
        }
    }
    v4f pre[NE];
    {
        const long long f = ((long long)VW_R + we) * VW_M;
        const v4i rx = vw_rsrc(xs + f * (XB / 4), bytes_need - f * XB);
#pragma unroll
        for (int m = 0; m < NE; ++m) pre[m] = vw_load4(rx, 1024 * m + in16, 0, VW_LOAD_AUX);
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    VW_STAMP(1);
    bool hi = (flags & 2) != 0;                                          // (wave-uniform) raised priority: a chunk's first workgroup - or, paced, the one behind
    if (hi) __builtin_amdgcn_s_setprio(2);

    unsigned p0 = 0;
    for (int t = 0; t < ntiles; ++t) {
        // the last tile of the workgroup's last unit refills nothing: no loads, no staging writes, no barrier behind its stores
        const bool fin = (flags & 1) != 0 && t == ntiles - 1;
        const unsigned pw = vw_wrap(p0 + (unsigned)we);
        const unsigned pl = vw_wrap(p0 + (unsigned)tl);
        // (a lane's byte offset in a 1 KB access and its entry in it, made opaque per tile: hipcc otherwise hoists the sums with
        //  every access number out of the tile loop - 2 x M/4 registers of constants held through the tap phase, which with
        //  64-frame runs is what spilled)
        int lq16 = lq * 16, in16o = in16;
        unsigned pwl = pw + (unsigned)lane_e, pwi = pw + (unsigned)in_e;
        asm volatile("" : "+v"(lq16), "+v"(pwl));
        if constexpr (VW_BC) asm volatile("" : "+v"(in16o), "+v"(pwi));
        float o[VW_M];
        {
            vw_lchar *b[2][VW_NBT];
#pragma unroll
            for (int k = 0; k < VW_NB; ++k) {
                b[0][k] = lds + vw_wrap(pl + (unsigned)(k * VW_G)) * 16u;
                b[1][k] = b[0][k] + VW_CH;
            }
            if (pc == 0) vw_taps_ch<0>(b, o);
            else vw_taps_ch<1>(b, o);
        }
#pragma unroll
        for (int j = 0; j < VW_M; ++j) asm volatile("" : "+v"(o[j]));
        VW_STAMP_TILE(t, 0);
        // X. every wave is done reading this tile's window: the tile's own entries are dead (both channels)
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        VW_STAMP_TILE(t, 1);
        if (hi) __builtin_amdgcn_s_setprio(3);
        else __builtin_amdgcn_s_setprio(1);
        // (pacing: the partner's count, in flight through the store phase)
        unsigned seen = 0;
        if (pace.other != nullptr) seen = __hip_atomic_load(pace.other, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // (the late part of THIS tile's refill: in flight through the transposition and the stores)
        v4f late[LATE > 0 ? LATE : 1];
        if constexpr (LATE > 0) {                                        // (also on a final tile: out of range there, no data moves)
            const long long fl = ((long long)t * VW_NH + VW_R + we) * VW_M;
            const v4i rl = vw_rsrc(xs + fl * (XB / 4), bytes_need - fl * XB);
#pragma unroll
            for (int m = 0; m < LATE; ++m) late[m] = vw_load4(rl, (VW_BC ? in16o : lq16) + 1024 * (NE + m), 0, VW_LOAD_AUX);
        }
        // the lane's run into its own dead entry, planar (its channel's planes)
        vw_lchar *const mine = lds + pc * VW_CH + pl * 16u;
#pragma unroll
        for (int r = 0; r < VW_QC; ++r)
            *(vw_lv4f *)(mine + r * VW_PLANE) = v4f{o[4 * r], o[4 * r + 1], o[4 * r + 2], o[4 * r + 3]};
        // X2. ... and the partner wave's (the other channel of the same 64 entries)
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        VW_STAMP_TILE(t, 2);
        const long long fo = (long long)t * VW_T + (long long)we * VW_M;
        const v4i ry = vw_rsrc(ys + fo * 2, bytes_left - fo * 8);
        const long long fi = ((long long)(t + 1) * VW_NH + VW_R + we) * VW_M;
        const v4i rx = vw_rsrc(xs + fi * (XB / 4), bytes_need - fi * XB);
        constexpr int ST_AUX = VW_NT_STORES ? VW_NT_STORE_AUX : 0;
        // (one access at a time; batches of 4 or 8 read-backs ahead of their stores measured no faster - the CU's other workgroup, or in a
        //  short launch nothing much, covers these round trips: tools/ablate/RUNS.md: run_r4c, run_r4g.sh)
#pragma unroll
        for (int m = 0; m < NI; ++m) {
            vw_lchar *at = lds + lane_at + vw_wrap(pwl + (unsigned)(m * VW_EPI_N)) * 16u;
            const v2f r0 = *(const volatile vw_lv2f *)at, r1 = *(const volatile vw_lv2f *)(at + VW_CH);
            vw_store4(v4f{r0.x, r1.x, r0.y, r1.y}, ry, lq16 + 1024 * m, 0, ST_AUX);
        }
        if (!fin) {
            const bool mirror = pw < (unsigned)VW_G || pw + 32u > (unsigned)VW_R;             // wave-uniform
#pragma unroll
            for (int m = 0; m < NIN; ++m) {
                const unsigned e = vw_wrap((VW_BC ? pwi : pwl) + (unsigned)(m * EIN));
                vw_lchar *at = lds + in_at + e * 16u;
                const v4f v = m < NE ? pre[m < NE ? m : 0] : late[m >= NE ? m - NE : 0];
                stage(at, v);
                if (mirror) { if (e < (unsigned)VW_G) stage(at + VW_R * 16, v); }
                if (m < NE) pre[m < NE ? m : 0] = vw_load4(rx, (VW_BC ? in16o : lq16) + 1024 * m, 0, VW_LOAD_AUX);
            }
        }
        p0 = p0 + VW_NH >= VW_R ? p0 + VW_NH - VW_R : p0 + VW_NH;
        pace.done += 1;
        if (pace.other != nullptr) {
            if (threadIdx.x == 0) __hip_atomic_store(pace.mine, pace.done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            hi = (unsigned)__builtin_amdgcn_readfirstlane((int)seen) > pace.done;       // the partner is ahead: this workgroup's next tile goes first
        }
        if (hi) __builtin_amdgcn_s_setprio(2);
        else __builtin_amdgcn_s_setprio(0);
        // Y. the refill is in place for every wave's window
        if (!fin) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        VW_STAMP_TILE(t, 3);
    }
    if (hi) __builtin_amdgcn_s_setprio(0);
    VW_STAMP_FLUSH(vw_stamp_on);
}
#endif

// VW_WAVES_PER_EU: the waves per SIMD that the LDS footprint and the registers let a CU hold - as minimum AND maximum:
// the scheduler must not trade registers for an occupancy the LDS will not grant
extern "C" __global__ __launch_bounds__(VW_NT) __attribute__((amdgpu_waves_per_eu(VW_WAVES_PER_EU, VW_WAVES_PER_EU)))
void vnd_spec_kernel(const VWArgs a)
{
#if VW_STAMPS
    { const unsigned long long entry_ = __builtin_amdgcn_s_memrealtime(); if (threadIdx.x == 0 && blockIdx.x < VW_STAMPS) vw_stamps[blockIdx.x * 16 + 12] = entry_; }
#endif
    extern __shared__ __attribute__((aligned(16))) float lds_generic[];
    vw_lchar *lds = (vw_lchar *)(vw_lfloat *)lds_generic;
    // One round of workgroups: more units than resident slots are walked inside the kernel
    // (the channel pairs of a span are neighbouring units: their workgroups touch the same lines at about the same time)
    const unsigned first = vw_xcd_remap(blockIdx.x, a.nblocks);
    // (ONE call site of the span loop - it is the whole tap sum, inlined - for both ways of cutting the work)
    const bool chunked = VW_PAIRS == 1 && a.chunk_tiles > 0;
    VWPace pace = {nullptr, nullptr, 0u};
    if (a.pace != nullptr && !chunked) {
        // the CU this workgroup runs on (HW_ID: cu 11:8, sh 12, se 15:13; XCC_ID) and its dispatch round there
        unsigned hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        const unsigned cu = (((xcc & 7u) * 8u + ((hw >> 13) & 7u)) * 2u + ((hw >> 12) & 1u)) * 16u + ((hw >> 8) & 15u);
        const unsigned round = ((blockIdx.x >> 3) / (unsigned)a.cus_per_xcd) & 1u;
        pace.mine = a.pace + cu * 2u + round;
        pace.other = a.pace + cu * 2u + (round ^ 1u);
        if (threadIdx.x == 0) __hip_atomic_store(pace.mine, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const bool balanced = VW_PAIRS == 1 && !chunked && a.bal_total > 0;
    long long g = 0, g_end = 0;                                          // balanced: this workgroup's range of the pool's tiles
    if (balanced) {
        g = (long long)first * a.bal_total / (long long)a.nblocks;
        g_end = (long long)(first + 1u) * a.bal_total / (long long)a.nblocks;
    }
    for (unsigned unit = first; chunked || (balanced ? g < g_end : unit < a.units); unit += a.nblocks) {
        int pg = 0, t_first, ntiles;
        long long stream;
        if (balanced) {
            stream = g / a.tiles_total;
            t_first = (int)(g - stream * a.tiles_total);
            const long long left_s = a.tiles_total - t_first, left_w = g_end - g;
            ntiles = (int)(left_s < left_w ? left_s : left_w);
            g += ntiles;
        } else if (chunked) {
            // An XCD hands its workgroups to its CUs in turn, a CU's second workgroup a whole round after its first (measured: stamps of
            // HW_ID, tools/win_stamps.py): workgroup j of XCD x runs on CU j mod cus_per_xcd as that CU's (j / cus_per_xcd)-th.  Were the
            // dispatch ever different, every piece would still be computed exactly once - only the balance would suffer.
            const unsigned xcd = blockIdx.x & 7u, j = blockIdx.x >> 3;
            const unsigned cu = j % (unsigned)a.cus_per_xcd, round = j / (unsigned)a.cus_per_xcd;
            const unsigned g = xcd * (unsigned)a.cus_per_xcd + cu;                           // the CU's chunk
            stream = g / (unsigned)a.chunks_per_stream;
            const int chunk = (int)(g % (unsigned)a.chunks_per_stream);
            const int len = round == 0 ? a.chunk_len0 : (round == 1 ? a.chunk_tiles - a.chunk_len0 : 0);
            t_first = chunk * a.chunk_tiles + (round == 0 ? 0 : a.chunk_len0);
            const int left = a.tiles_total - t_first;
            ntiles = left < len ? left : len;
            if (ntiles <= 0) break;
            if (round != 0 && a.stagger_ticks > 0) {
                const unsigned long long until = __builtin_amdgcn_s_memrealtime() + (unsigned long long)a.stagger_ticks;
                while (__builtin_amdgcn_s_memrealtime() < until) __builtin_amdgcn_s_sleep(8);
            }
        } else {
            unsigned id = unit;
            pg = (int)(id % (unsigned)VW_PAIRS);
            id /= (unsigned)VW_PAIRS;
            const int span = (int)(id % (unsigned)a.spans);
            stream = id / (unsigned)a.spans;
            t_first = span * a.tiles_per_span;
            const int left = a.tiles_total - t_first;
            ntiles = left < a.tiles_per_span ? left : a.tiles_per_span;
        }
        // flags: 1 = the workgroup's last unit (its last tile refills nothing), 2 = raised wave priority throughout
        const int flags = ((chunked || (balanced ? g >= g_end : unit + a.nblocks >= a.units)) ? 1 : 0) | ((chunked && a.chunk_prio && (blockIdx.x >> 3) < (unsigned)a.cus_per_xcd) ? 2 : 0);
        VW_DISPATCH(pg)
        if (chunked) break;
    }
#if VW_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    { const unsigned long long exit_ = __builtin_amdgcn_s_memrealtime(); if (threadIdx.x == 0 && blockIdx.x < VW_STAMPS) vw_stamps[blockIdx.x * 16 + 13] = exit_; }
#endif
}
)VNDWIN"
