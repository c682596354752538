// Sample-rate conversion: torchaudio's sinc_interp_hann resampling written per output sample - the second half of
// pitch_shift, which is time_stretch followed by this.  With o : n the reduced ratio orig : new, base = min(o, n) * rolloff,
// W = lowpass_filter_width and x read as zero outside 0 ... L - 1, output m of ceil(n L / o) is
//     y[m] = (base / o) * sum over s with |tau| < W of  sinc(tau) * cos^2(pi tau / (2 W)) * x[s],
//     tau = base * d / (o n),   d = s n - m o   (an exact 64-bit integer),   sinc(t) = sin(pi t) / (pi t).
// Weights and sum are float64 for both dtypes and y is rounded once (k_phase_vocoder's rule).
// One lane per output sample, 256 consecutive outputs of one row per workgroup.  The lane's taps are s = c + j, |j| <= J,
// c = round(m o / n) and J = ceil(W o / base): tau_j = tau_0 + j * delta with delta = base / o and |tau_0| <= delta / 2.  No table:
// the lane takes sin and cos of pi tau_0 and of pi tau_0 / W once, and the pair of taps c + j, c - j follows from the pair before
// it by the fixed rotations by pi delta and pi delta / W (one uniform sine / cosine pair each, computed on the host), walking
// outwards from the centre so that a tap j steps away carries j rotations' rounding on a sinc whose 1 / (pi tau_j) has shrunk by
// the same j.  The centre tap, where pi tau goes down to 1e-4 and below, takes its sinc from its own sine, not from a recurrence.
// A workgroup's taps are one contiguous span of its row, c(first) - J ... c(last) + J: it is staged through LDS, zeros where the
// row ends, when it fits kResampleLdsBytes, and the loop then runs without bounds; a ratio that lowers the rate further reads
// global memory directly (STAGE = false: the same arithmetic in the same order, the same bits).
#pragma once
#include <cmath>

#include "common.h"

namespace specinv {

constexpr int kResampleTile = 256;           // outputs per workgroup, one per lane
constexpr int kResampleLdsBytes = 16384;     // the staged span's budget: ten workgroups share a CU's 160 KiB

struct ResampleArgs {
  int64_t o, n;            // the reduced ratio orig : new
  int64_t n_in, n_out;     // L and ceil(n L / o)
  int64_t tiles;           // workgroups per row, ceil(n_out / kResampleTile)
  int J;                   // taps reach c - J ... c + J
  double scale;            // base / (o n): tau = scale * d
  double delta;            // base / o: tau's step from one input sample to the next, and the gain of the sum
  double width;            // W
  double sin_d, cos_d;     // sin, cos of pi delta
  double sin_w, cos_w;     // sin, cos of pi delta / W
};

// c = round(m o / n) and r = m o - c n, |r| <= n / 2 (m o < 2^62: the entry point checks it)
__device__ __forceinline__ int64_t resample_centre(int64_t m, int64_t o, int64_t n, int64_t* r_out) {
  const int64_t mo = m * o;
  int64_t c = mo / n;
  int64_t r = mo - c * n;
  if (r > n - r) {
    ++c;
    r -= n;
  }
  *r_out = r;
  return c;
}

template <typename T, bool STAGE>
__global__ void __launch_bounds__(kResampleTile) k_resample(const T* __restrict__ x, T* __restrict__ y, int64_t block0,
                                                            ResampleArgs a) {
#pragma clang fp contract(off)
  __shared__ T span[STAGE ? kResampleLdsBytes / sizeof(T) : 1];
  const int64_t blk = block0 + blockIdx.x;
  const int64_t row = blk / a.tiles;
  const int64_t m0 = (blk - row * a.tiles) * kResampleTile;
  const int64_t m = m0 + threadIdx.x;
  const T* xrow = x + row * a.n_in;
  int64_t r;
  const int64_t c = resample_centre(m < a.n_out ? m : a.n_out - 1, a.o, a.n, &r);
  int64_t first = 0;       // the sample span[0] holds
  if constexpr (STAGE) {
    int64_t r_unused;
    const int64_t m1 = m0 + kResampleTile - 1 < a.n_out ? m0 + kResampleTile - 1 : a.n_out - 1;
    first = resample_centre(m0, a.o, a.n, &r_unused) - a.J;
    const int len = (int)(resample_centre(m1, a.o, a.n, &r_unused) + a.J - first) + 1;   // (the host chose STAGE: it fits)
    for (int i = threadIdx.x; i < len; i += kResampleTile) {
      const int64_t s = first + i;
      span[i] = s >= 0 && s < a.n_in ? xrow[s] : T(0);
    }
    __syncthreads();
  }
  if (m >= a.n_out) return;
  auto tap = [&](int64_t s) -> double {
    if constexpr (STAGE) {
      return (double)span[(int)(s - first)];
    } else {
      return s >= 0 && s < a.n_in ? (double)xrow[s] : 0.0;
    }
  };
  const double pi = 3.14159265358979323846;
  const double tau0 = a.scale * (double)(-r);
  double sp, cp, swp, cwp;                   // sin, cos of pi tau and of pi tau / W at tap c + j ...
  sincospi(tau0, &sp, &cp);
  sincospi(tau0 / a.width, &swp, &cwp);
  double sm = sp, cm = cp, swm = swp, cwm = cwp;   // ... and at tap c - j
  // the centre: its own sine over its own argument (tau0 = 0 is r = 0), |tau0| <= delta / 2 < W
  const double w0 = (r == 0 ? 1.0 : sp / (pi * tau0)) * fma(0.5, cwp, 0.5);
  double acc = w0 * tap(c);
  for (int j = 1; j <= a.J; ++j) {
    double t;
    t = fma(sp, a.cos_d, cp * a.sin_d);      // rotate by +pi delta
    cp = fma(cp, a.cos_d, -(sp * a.sin_d));
    sp = t;
    t = fma(swp, a.cos_w, cwp * a.sin_w);
    cwp = fma(cwp, a.cos_w, -(swp * a.sin_w));
    swp = t;
    t = fma(sm, a.cos_d, -(cm * a.sin_d));   // rotate by -pi delta
    cm = fma(cm, a.cos_d, sm * a.sin_d);
    sm = t;
    t = fma(swm, a.cos_w, -(cwm * a.sin_w));
    cwm = fma(cwm, a.cos_w, swm * a.sin_w);
    swm = t;
    const double tp = fma((double)j, a.delta, tau0);     // > 0
    const double tm = fma(-(double)j, a.delta, tau0);    // < 0
    const double inv = 1.0 / (pi * (tp * tm));           // one division for the pair: 1 / tp = tm * inv, 1 / tm = tp * inv
    const double wp = tp < a.width ? sp * (tm * inv) * fma(0.5, cwp, 0.5) : 0.0;
    const double wm = -tm < a.width ? sm * (tp * inv) * fma(0.5, cwm, 0.5) : 0.0;
    acc = fma(wp, tap(c + j), acc);
    acc = fma(wm, tap(c - j), acc);
  }
  y[row * a.n_out + m] = (T)(a.delta * acc);
}

}  // namespace specinv
