// vnd_dense.hpp - WhiteNoise on the device: the dense float64 FIR of WhiteNoise.decorrelate (np.convolve(x[:, c], h[:, c],
// mode='same') per channel, decorrelation.py:684-699) and the stage around it (width, rms_normalize: the epilogue of vnd_stage.hpp).
// (one translation unit: included by vnd_amd.hip after vnd_stage.hpp; everything static here is private to the library)
#pragma once

// Numerics.  NumPy promotes the float32 signal to float64 exactly, forms each output as a float64 dot product and rounds it once
// to float32.  Here: y[n] = f32(fma chain over k = 0 .. M-1 ascending of h[k] * f64(x[n + o - k])), o = (M-1)/2, with x = 0
// outside [0, n) - adding 0 * h to the chain changes no bit while h is finite.  The order of the chain is fixed per output, so
// the result does not depend on batch, tiling or stream position.  NumPy's own float64 order depends on the BLAS kernel the host
// picks; the two agree to within one float32 ulp of the output plus 2^-40 * sum |h x| (vnd_amd.h).
//
// Form (FP64-bound: 1323 FMAs per output against 8 bytes of HBM traffic).  A workgroup of 4 waves owns kDenseTile consecutive
// output frames of ONE channel of one stream; each lane owns kDenseR = 16 consecutive outputs in 16 float64 accumulators.  The
// input window of a chunk of kDenseTaps taps is staged into LDS as float32 (zeros outside the signal).  Taps go in blocks of 16:
// a block needs x[s .. s+30] of the lane's window, held as two 16-value float64 register arrays (lo / hi) that swap roles from
// block to block, so each block costs 16 new values (four ds_read_b128 + 16 conversions) for 256 v_fma_f64.  h[k][c] is
// wave-uniform: scalar loads, an SGPR-pair operand of every FMA.
// One channel per workgroup (rather than every channel of a frame range) keeps h uniform per wave and the LDS window at
// kDenseTile + kDenseTaps floats whatever the channel count; the strided staging reads cost nothing next to the FMAs.
constexpr int kDenseThreads = 256;
constexpr int kDenseR = 16;                                   // outputs per lane (and taps per block)
constexpr int kDenseTile = kDenseThreads * kDenseR;           // 4096 output frames per workgroup
constexpr int kDenseTaps = 1024;                              // taps per staged chunk: a multiple of kDenseR

struct DArgs {
    const float *__restrict__ x;      // [batch][n][Cx]
    const double *__restrict__ h;     // [M][C], the reference's layout
    float *__restrict__ y;            // [batch][n][C]
    int64_t n;
    int32_t M, C, Cx, o;              // o = (M - 1) / 2: NumPy's 'same' window
    int32_t tiles;                    // workgroups per channel of a stream
};

// 16 consecutive floats of the staged window (16-byte aligned) as float64
__device__ __forceinline__ void dense_load(double (&v)[kDenseR], const float *p)
{
#pragma unroll
    for (int q = 0; q < kDenseR / 4; ++q) {
        const float4 f = reinterpret_cast<const float4 *>(p)[q];
        v[4 * q + 0] = (double)f.x; v[4 * q + 1] = (double)f.y; v[4 * q + 2] = (double)f.z; v[4 * q + 3] = (double)f.w;
    }
}

// One block of 16 taps, k = k0 + i ascending (i = 0 .. 15): output j of the lane takes x at window offset 15 - i + j, which is
// lo[15 - i + j] below 16 and hi[-1 - i + j] from there.  Guard: taps i < first are not part of the filter (the top block of a
// chunk whose length is not a multiple of 16).
template <bool Guard>
__device__ __forceinline__ void dense_block(double (&acc)[kDenseR], const double (&lo)[kDenseR], const double (&hi)[kDenseR],
                                            const double *__restrict__ hc, int k0, int C, int first)
{
#pragma unroll
    for (int i = 0; i < kDenseR; ++i) {
        if (Guard && i < first) continue;
        const double hk = hc[(int64_t)(k0 + i) * C];
#pragma unroll
        for (int j = 0; j < kDenseR; ++j) {
            const int m = kDenseR - 1 - i + j;
            acc[j] = fma(hk, m < kDenseR ? lo[m] : hi[m - kDenseR], acc[j]);
        }
    }
}

__global__ __launch_bounds__(kDenseThreads) void dense_fir_kernel(DArgs a)
{
    __shared__ __align__(16) float xs[kDenseTile + kDenseTaps];
    const int tile = (int)(blockIdx.x % (unsigned)a.tiles);
    const int c = (int)(blockIdx.x / (unsigned)a.tiles);
    const int64_t b = blockIdx.y;
    const int64_t n0 = (int64_t)tile * kDenseTile;
    const float *__restrict__ xc = a.x + b * a.n * a.Cx + (a.Cx == 1 ? 0 : c);
    const double *__restrict__ hc = a.h + c;
    const int t0 = threadIdx.x * kDenseR;                       // the lane's first output, relative to n0

    double acc[kDenseR];
#pragma unroll
    for (int j = 0; j < kDenseR; ++j) acc[j] = 0.0;

    for (int kc0 = 0; kc0 < a.M; kc0 += kDenseTaps) {
        const int kc_end = min(kc0 + kDenseTaps, a.M);
        const int L = kc_end - kc0;
        const int Lr = (L + kDenseR - 1) & ~(kDenseR - 1);
        // the chunk's window: xs[s] = x[gbase + s], s < kDenseTile + Lr.  Tap k of output t reads s = t + (kc_end - 1 - k)
        // (at most kDenseTile - 1 + Lr - 1; the top block's guarded taps and the unused tail reach kDenseTile + Lr - 1).
        const int64_t gbase = n0 + a.o - (kc_end - 1);
        __syncthreads();                                        // the previous chunk's reads are done
        for (int s = threadIdx.x; s < kDenseTile + Lr; s += kDenseThreads) {
            const int64_t g = gbase + s;
            xs[s] = (g >= 0 && g < a.n) ? xc[g * a.Cx] : 0.0f;
        }
        __syncthreads();
        // blocks from the top of the window down (u = kc_end - 1 - k descending = k ascending); block U covers u in
        // [U, U + 16): k0 = kc_end - 16 - U, its window x[t0 + U .. t0 + U + 31]
        double A[kDenseR], B[kDenseR];
        int U = Lr - kDenseR;
        dense_load(A, xs + t0 + U);
        dense_load(B, xs + t0 + U + kDenseR);
        dense_block<true>(acc, A, B, hc, kc_end - kDenseR - U, a.C, Lr - L);
        int left = U / kDenseR;                                 // blocks below the top one
        for (; left >= 2; left -= 2) {
            U -= kDenseR;
            dense_load(B, xs + t0 + U);
            dense_block<false>(acc, B, A, hc, kc_end - kDenseR - U, a.C, 0);
            U -= kDenseR;
            dense_load(A, xs + t0 + U);
            dense_block<false>(acc, A, B, hc, kc_end - kDenseR - U, a.C, 0);
        }
        if (left) {
            U -= kDenseR;
            dense_load(B, xs + t0 + U);
            dense_block<false>(acc, B, A, hc, kc_end - kDenseR - U, a.C, 0);
        }
    }
    float *__restrict__ yc = a.y + b * a.n * a.C + c;
#pragma unroll
    for (int j = 0; j < kDenseR; ++j) {
        const int64_t nn = n0 + t0 + j;
        if (nn < a.n) yc[nn * a.C] = (float)acc[j];
    }
}

extern "C" {

static bool bytes_overlap(const void *p, int64_t pb, const void *q, int64_t qb)
{
    const char *a = (const char *)p, *b = (const char *)q;
    return pb > 0 && qb > 0 && a < b + qb && b < a + pb;
}

vnd_status vnd_white_noise_f32_dev(vnd_ctx *ctx, const float *x, const double *h, float *y, int64_t batch, int64_t n,
                                   int32_t Cx, int32_t C, int32_t M, int32_t use_width, double width, int32_t normalize,
                                   float eps, void *workspace, int64_t workspace_bytes, void *stream_)
{
    if (!ctx) return fail(VND_ERR_INVALID, "null context");
    if (batch < 0) return fail(VND_ERR_INVALID, "negative batch");
    if (C <= 0 || C > 65535) return fail(VND_ERR_INVALID, "n_channels %d out of range", C);
    if (!(Cx == C || (Cx == 1 && C == 2)))
        return fail(VND_ERR_INVALID, "in_channels must equal n_channels, or be 1 with 2 output channels: got %d and %d", Cx, C);
    if (M < 1) return fail(VND_ERR_INVALID, "fir_length must be >= 1, got %d", M);
    if (n < M) return fail(VND_ERR_INVALID, "n_frames (%lld) must be >= fir_length (%d)", (long long)n, M);
    if (use_width && C != 2) return fail(VND_ERR_INVALID, "stereo width needs 2 channels, got %d", C);
    if (normalize != VND_NORMALIZE_OFF && normalize != VND_NORMALIZE_RMS && normalize != VND_NORMALIZE_RMS_REFERENCE_ORDER)
        return fail(VND_ERR_INVALID, "unknown normalize %d", normalize);
    // (a dispatch counts its work-items in 32 bits: tiles x channels x 256 threads)
    if (n > (int64_t)1 << 40 || (n + kDenseTile - 1) / kDenseTile * C > (int64_t)(UINT32_MAX / kDenseThreads))
        return fail(VND_ERR_UNSUPPORTED, "problem too large: split the signal's channels");
    if (batch == 0) return VND_OK;
    if (!x || !h || !y) return fail(VND_ERR_INVALID, "null signal or filter pointer");
    const int64_t xb = batch * n * Cx * (int64_t)sizeof(float), yb = batch * n * C * (int64_t)sizeof(float);
    const int64_t hb = (int64_t)M * C * (int64_t)sizeof(double);
    int64_t need = 0;
    vnd_decorrelate_workspace_bytes(batch, n, C, &need);
    if (normalize && (!workspace || workspace_bytes < need))
        return fail(VND_ERR_INVALID, "workspace too small: need %lld bytes", (long long)need);
    const int64_t wb = normalize ? need : 0;
    if (bytes_overlap(x, xb, y, yb) || bytes_overlap(h, hb, y, yb) || bytes_overlap(workspace, wb, x, xb) ||
        bytes_overlap(workspace, wb, y, yb) || bytes_overlap(workspace, wb, h, hb))
        return fail(VND_ERR_INVALID, "x, h, y and the workspace must not overlap");
    if (batch > VND_MAX_STREAMS) return fail(VND_ERR_UNSUPPORTED, "more than %d streams per call: split the batch", VND_MAX_STREAMS);
    DeviceScope on(ctx->device);
    hipStream_t stream = (hipStream_t)stream_;

    DArgs d{};
    d.x = x; d.h = h; d.y = y; d.n = n; d.M = M; d.C = C; d.Cx = Cx; d.o = (M - 1) / 2;
    d.tiles = (int32_t)((n + kDenseTile - 1) / kDenseTile);
    hipLaunchKernelGGL(dense_fir_kernel, dim3((unsigned)(d.tiles * C), (unsigned)batch), dim3(kDenseThreads), 0, stream, d);
    if (!(use_width || normalize)) {
        HIP_TRY(hipGetLastError());
        return VND_OK;
    }
    // the epilogue of the exact velvet-noise stage (decorrelate_dev's table-order branch): the float64 FIR rounds once per output,
    // so both normalize values take NumPy's order of the sums of squares
    StageSetup s = stage_setup(ctx, x, y, batch, n, Cx, C, VND_MODE_EXACT, 0, use_width, width, normalize, eps, workspace);
    EArgs &e = s.e;
    e.rows = s.want_seq ? 1 : (int32_t)epi_chunks(n);
    if (s.want_seq) e.normalize = 0;                   // pointwise pass without its partial sums
    if (e.use_width || (normalize && !s.want_seq))
        hipLaunchKernelGGL(epilogue_pointwise_kernel, s.grid, dim3(kEpiThreads), 0, stream, e);
    return stage_sums(ctx, s, x, y, batch, n, Cx, C, normalize, s.want_seq, false, stream);
}

}  // extern "C"
