// The phase vocoder: a complex spectrogram (B, F, T) resampled along time at `rate` to T_out frames - the
// time-scale modification of Griffin & Lim 1984 / librosa.phase_vocoder / torchaudio.functional.phase_vocoder, whose result
// time_stretch hands to the iterative methods as their start.  With t_j = j * rate, i = floor(t_j), a = t_j - i and frames at
// and beyond T read as +0 + 0i, output frame j of bin k is
//     m_j = a |S[i+1]| + (1 - a) |S[i]| ;   P[j] = m_j exp(i phi_j) ;   phi_0 = arg S[0] ,  phi_{j+1} = phi_j + d_j ,
//     d_j = wrap(arg S[i+1] - arg S[i] - adv) + adv ,   adv = 2 pi k_s hop / n_fft ,   wrap(x) = x - 2 pi round(x / 2 pi),
// k_s the signed bin (k, or k - n_fft above n_fft / 2: two-sided spectra).  The angles are taken in the input dtype; everything
// after them is float64 for both dtypes, the running sum included, and P is rounded once.  (phase_init rounds every partial sum to
// float32 because the reference does; here the expected advance reaches pi * hop rad per frame, a float32 chain loses 1e-3 of the
// result to it and there is no reference to reproduce.)
// One wave per (b, k) row as k_phase_init: the 64 lanes take 64 consecutive output frames, gather their two source frames along
// the contiguous time axis, and the sum is a prefix over the lanes with a carry from one step of 64 to the next.  The loads of the
// next 64 frames are issued before the scan of the current ones.
#pragma once
#include <cmath>
#include <type_traits>

#include "common.h"

namespace specinv {

// T_out: the smallest n >= 1 with (double)n * rate >= n_in, the product a float64 product - the host layer's
// timescale.stretched_frames is the same statement.  0: no such n fits an int32 (or the arguments are not valid).
inline int64_t pvoc_stretched_frames(int64_t n_in, double rate) {
  if (n_in < 1 || !(rate > 0) || !std::isfinite(rate)) return 0;
  const double q = std::ceil((double)n_in / rate);
  if (!(q < 2147483000.0)) return 0;
  int64_t n = q < 1 ? 1 : (int64_t)q;
  while (n > 1 && (double)(n - 1) * rate >= (double)n_in) --n;
  while ((double)n * rate < (double)n_in) ++n;
  return n;
}

__device__ inline float pvoc_angle(float re, float im) { return atan2f(im, re); }
__device__ inline double pvoc_angle(double re, double im) { return atan2(im, re); }
// |z| in float64: a float's squares and their sum's root are exact but for two roundings, no overflow to guard
__device__ inline double pvoc_abs(float re, float im) {
  const double x = (double)re, y = (double)im;
  return sqrt(fma(x, x, y * y));
}
__device__ inline double pvoc_abs(double re, double im) { return hypot(re, im); }

template <typename T>
__global__ void __launch_bounds__(256) k_phase_vocoder(const cplx<T>* __restrict__ in, cplx<T>* __restrict__ out, int rows, int F,
                                                       int Tin, int Tout, double rate, int n_fft, int hop) {
#pragma clang fp contract(off)
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;                                 // (a whole wave: the scans below run with every lane)
  const int k = row % F;
  const cplx<T>* irow = in + (int64_t)row * Tin;
  cplx<T>* orow = out + (int64_t)row * Tout;
  const double two_pi = 6.283185307179586476925286766559;
  const int ks = k <= n_fft / 2 ? k : k - n_fft;
  const double adv = two_pi * (double)ks * (double)hop / (double)n_fft;
  // the two source frames of output frame j and the weight of the second; j < Tout keeps i = floor(j * rate) below Tin
  auto fetch = [&](int j, cplx<T>& s0, cplx<T>& s1, double& a) {
    s0 = mk<T>(T(0), T(0));
    s1 = s0;
    a = 0;
    if (j < Tout) {
      const double t = (double)j * rate;
      const double fl = floor(t);
      const int64_t i = (int64_t)fl;
      a = t - fl;
      if (i < Tin) s0 = irow[i];
      if (i + 1 < Tin) s1 = irow[i + 1];
    }
  };
  cplx<T> c0, c1, n0, n1;
  double ca, na;
  fetch(lane, c0, c1, ca);
  double carry = 0;        // phi of the previous step's last frame
  double d_prev = 0;       // ... and its increment d
  for (int j0 = 0; j0 < Tout; j0 += 64) {
    const int j = j0 + lane;
    fetch(j + 64, n0, n1, na);
    const double th0 = (double)pvoc_angle(c0.x, c0.y);
    const double th1 = (double)pvoc_angle(c1.x, c1.y);
    double d = th1 - th0 - adv;
    d = d - two_pi * rint(d / two_pi);
    d = d + adv;
    // lane l adds d_{j-1}: its neighbour's increment, across a step the previous step's last; frame 0 starts at arg S[0]
    double v = __shfl_up(d, 1, 64);
    if (lane == 0) v = j0 == 0 ? th0 : d_prev;
    d_prev = __shfl(d, 63, 64);
    if constexpr (std::is_same<T, double>::value) {
      v = wave_scan_in_order(v, carry, lane);              // one addition after the other, as a cumulative sum on the host
    } else {
      v = wave_scan_inclusive(v);
      v += carry;
      carry = __shfl(v, 63, 64);
    }
    if (j < Tout) {
      const double m = ca * pvoc_abs(c1.x, c1.y) + (1.0 - ca) * pvoc_abs(c0.x, c0.y);
      double sn, cs;
      sincos_phase(v, &sn, &cs);                           // the float64 phase, not a rounded one
      orow[j] = mk<T>((T)(m * cs), (T)(m * sn));
    }
    c0 = n0;
    c1 = n1;
    ca = na;
  }
}

// Host side (tu_pvoc.hip): four rows per workgroup of 256.  in (rows, n_in), out (rows, n_out), rows = batch * n_freq.
template <typename T>
int pvoc_launch(const cplx<T>* in, cplx<T>* out, int batch, int n_freq, int n_in, int n_out, double rate, int n_fft, int hop,
                hipStream_t stream);

}  // namespace specinv
