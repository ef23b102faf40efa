// vnd_polar.hpp - the polar sample of one stereo frame and its moments, shared by the
// stand-alone moments kernels (vnd_moments.hpp) and the convolution kernels' moments sink (vnd_kernels.hpp).
// Element maths in float32 like NumPy's (utils/dsp.py:374-422), sums in float64.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vnd {

constexpr int kMoments = 8;

struct PolarAcc {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, lr = 0.0, ll = 0.0, rr = 0.0;
    float tmax = 0.0f;
};

__device__ __forceinline__ void polar_add(PolarAcc &a, float l, float r)
{
    const float kHalfPi = 1.57079632679489661923f, kPi = 3.14159265358979323846f;   // float32(np.pi / 2), float32(np.pi)
    float th = atan2f(l - r, l + r);
    if (th < -kHalfPi) th = th + kPi;                  // np.where(t < -pi/2, t + pi, np.where(t > pi/2, t - pi, t))
    else if (th > kHalfPi) th = th - kPi;
    const float rad = sqrtf(l * l + r * r);
    const float t2 = th * th;
    a.s0 += (double)rad;
    a.s1 += (double)(rad * th);
    a.s2 += (double)(rad * t2);
    a.s3 += (double)(rad * (t2 * th));
    a.tmax = fmaxf(a.tmax, fabsf(th));
    a.lr += (double)(l * r);
    a.ll += (double)(l * l);
    a.rr += (double)(r * r);
}

// The sample alone, for the vectorscope (vnd_scope.hpp): polar_add's theta and radius with polar_coordinates' two options
// open - `ms` false is LayoutMode.LR, atan2f(l, r); `fold` false keeps the whole circle.  The coordinates kernel and the
// histogram kernels all take their sample from here, so a count grid is the grid of the thetas and radii written out.
__device__ __forceinline__ void polar_sample(float l, float r, bool ms, bool fold, float &th, float &rad)
{
    const float kHalfPi = 1.57079632679489661923f, kPi = 3.14159265358979323846f;   // float32(np.pi / 2), float32(np.pi)
    th = ms ? atan2f(l - r, l + r) : atan2f(l, r);
    if (fold) {
        if (th < -kHalfPi) th = th + kPi;
        else if (th > kHalfPi) th = th - kPi;
    }
    rad = sqrtf(l * l + r * r);
}

__device__ __forceinline__ void polar_store(double *out, const PolarAcc &a)
{
    out[0] = a.s0; out[1] = a.s1; out[2] = a.s2; out[3] = a.s3;
    out[4] = (double)a.tmax; out[5] = a.lr; out[6] = a.ll; out[7] = a.rr;
}


// The float64 sibling, for float64 signals (HaasEffect's output, vnd_haas_scan.hpp): theta, r and every product in
// float64 as NumPy does them on float64 arrays - np.arctan2, the fold with float64 pi, np.sqrt(l**2 + r**2) (two
// roundings, then a correctly rounded sqrt; the build keeps mul and add apart).  atan2 follows C99 on signed zeros,
// as NumPy's does: a silent frame folds to theta = +0 (from +-pi) or keeps its sign (+-0), so |theta| = 0.
struct PolarAcc64 {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, tmax = 0.0, lr = 0.0, ll = 0.0, rr = 0.0;
};

__device__ __forceinline__ void polar_add64(PolarAcc64 &a, double l, double r)
{
    const double kHalfPi = 1.5707963267948966, kPi = 3.141592653589793;          // np.pi / 2, np.pi
    double th = atan2(l - r, l + r);
    if (th < -kHalfPi) th = th + kPi;
    else if (th > kHalfPi) th = th - kPi;
    const double rad = sqrt(l * l + r * r);
    const double t2 = th * th;
    a.s0 += rad;
    a.s1 += rad * th;
    a.s2 += rad * t2;
    a.s3 += rad * (t2 * th);
    a.tmax = fmax(a.tmax, fabs(th));
    a.lr += l * r;
    a.ll += l * l;
    a.rr += r * r;
}

// polar_sample for float64 frames
__device__ __forceinline__ void polar_sample64(double l, double r, bool ms, bool fold, double &th, double &rad)
{
    const double kHalfPi = 1.5707963267948966, kPi = 3.141592653589793;          // np.pi / 2, np.pi
    th = ms ? atan2(l - r, l + r) : atan2(l, r);
    if (fold) {
        if (th < -kHalfPi) th = th + kPi;
        else if (th > kHalfPi) th = th - kPi;
    }
    rad = sqrt(l * l + r * r);
}

__device__ __forceinline__ void polar_values64(double v[kMoments], const PolarAcc64 &a)
{
    v[0] = a.s0; v[1] = a.s1; v[2] = a.s2; v[3] = a.s3; v[4] = a.tmax; v[5] = a.lr; v[6] = a.ll; v[7] = a.rr;
}


}  // namespace vnd
