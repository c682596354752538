// The phase vocoder with identity phase locking (Laroche & Dolson 1999): the vocoder of kernels_pvoc.h whose phase is
// kept coherent around every spectral peak.  With S0 = S[i], theta = arg S0, m and the running phase phi of DESIGN 3.19:
//     q[k] = re^2 + im^2 of S0[k] in float64 (two products and a sum, no contraction);
//     k is a peak of frame j when q[k] > q[k'] for k' = k +- 1, k +- 2 - taken modulo n_fft on a two-sided spectrum, dropped outside
//       0 .. F - 1 on a one-sided one, dropped where k' is the bin's own mirror image (k' + k = 0 mod n_fft);
//     the owner p(k) is the nearest peak of the frame (|k - p|, circular on two-sided spectra; a tie goes to the smaller |k_s|,
//       then to the lower index);
//     psi[k] = (phi[p] - theta[p]) + theta[k] ,  P[j][k] = m (cos psi + i sin psi) ;  a frame without a peak keeps psi = phi.
// Two launches.  k_pvoc_lock_scan is k_phase_vocoder's scan (a wave per (b, k) row, 64 output frames per step, the float64 prefix
// with its carry) and writes phi as float64 into the plan's scratch (B, F, T_out) instead of P.  It is phi and not phi - theta
// that is kept: a frame without a peak then gets the bits of the unlocked vocoder, and theta[p] is taken again, from the same bits
// by the same function, only at the peaks.
// k_pvoc_lock_apply: a wave takes 64 consecutive output frames of one item, one frame per lane, and a band of kPvocLockBand bins.
// A lane walks its band upward with a five-bin window of q in registers and keeps the band's peaks as a bit mask; where the band's
// first / last peak leaves bins without a nearer owner it searches downward from the band's lower edge / upward from its upper one
// (over the wrap-around on two-sided spectra) for the next peak, no further than that peak could still win.  Then it walks the band
// once more, carries the peak below (index, phi - theta) and the peak above, and resolves every bin: S0[k], S1[k] again (cache
// hits), m, sincos_phase((phi_p - theta_p) + theta_k), one store.  The loads and stores of a wave are contiguous along time.
// Every loop is bounded by F; no wave waits for another and nothing is atomic.
#pragma once
#include "kernels_pvoc.h"

namespace specinv {

constexpr int kPvocLockBand = 32;        // bins per wave of k_pvoc_lock_apply, at most 64 (the peak mask); tools/log/EXPERIMENTS.md
static_assert(kPvocLockBand >= 1 && kPvocLockBand <= 64, "the band's peaks are one 64-bit mask");

template <typename T>
__global__ void __launch_bounds__(256) k_pvoc_lock_scan(const cplx<T>* __restrict__ in, double* __restrict__ phi, int rows, int F,
                                                        int Tin, int Tout, double rate, int n_fft, int hop) {
#pragma clang fp contract(off)
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;                                 // (a whole wave: the scans below run with every lane)
  const int k = row % F;
  const cplx<T>* irow = in + (int64_t)row * Tin;
  double* prow = phi + (int64_t)row * Tout;
  const double two_pi = 6.283185307179586476925286766559;
  const int ks = k <= n_fft / 2 ? k : k - n_fft;
  const double adv = two_pi * (double)ks * (double)hop / (double)n_fft;
  auto fetch = [&](int j, cplx<T>& s0, cplx<T>& s1) {
    s0 = mk<T>(T(0), T(0));
    s1 = s0;
    if (j < Tout) {
      const int64_t i = (int64_t)floor((double)j * rate);
      if (i < Tin) s0 = irow[i];
      if (i + 1 < Tin) s1 = irow[i + 1];
    }
  };
  cplx<T> c0, c1, n0, n1;
  fetch(lane, c0, c1);
  double carry = 0;        // phi of the previous step's last frame
  double d_prev = 0;       // ... and its increment d
  for (int j0 = 0; j0 < Tout; j0 += 64) {
    const int j = j0 + lane;
    fetch(j + 64, n0, n1);
    const double th0 = (double)pvoc_angle(c0.x, c0.y);
    const double th1 = (double)pvoc_angle(c1.x, c1.y);
    double d = th1 - th0 - adv;
    d = d - two_pi * rint(d / two_pi);
    d = d + adv;
    double v = __shfl_up(d, 1, 64);
    if (lane == 0) v = j0 == 0 ? th0 : d_prev;
    d_prev = __shfl(d, 63, 64);
    if constexpr (std::is_same<T, double>::value) {
      v = wave_scan_in_order(v, carry, lane);
    } else {
      v = wave_scan_inclusive(v);
      v += carry;
      carry = __shfl(v, 63, 64);
    }
    if (j < Tout) prow[j] = v;
    c0 = n0;
    c1 = n1;
  }
}

// One lane's view of its output frame: the two source frames of every bin, the scratch column and the output column.
template <typename T>
struct PvocLockFrame {
  const cplx<T>* s0;       // S0[k] = s0[k * Tin]
  const double* phi;       // phi[k] = phi[k * Tout]
  int F, Tin, Tout;
  bool two_sided, has1;    // has1: frame i + 1 exists (else S1 = +0 + 0i)

  // q of bin kk, which may lie outside 0 .. F - 1: wrapped on a two-sided spectrum, -1 (below every q) on a one-sided one
  __device__ __forceinline__ double q(int kk) const {
#pragma clang fp contract(off)
    if (two_sided) {
      kk %= F;
      if (kk < 0) kk += F;
    } else if (kk < 0 || kk >= F) {
      return -1.0;
    }
    const cplx<T> s = s0[(int64_t)kk * Tin];
    const double x = (double)s.x, y = (double)s.y;
    return x * x + y * y;
  }
  // is bin k (0 .. F - 1, the same in every lane) a peak, given q at k - 2 .. k + 2
  __device__ __forceinline__ bool peak(int k, double m2, double m1, double c, double p1, double p2) const {
    if (two_sided) {                                       // a neighbour that is the bin's mirror image does not count
      if ((2 * k + F - 2) % F == 0) m2 = -1.0;
      if ((2 * k + F - 1) % F == 0) m1 = -1.0;
      if ((2 * k + 1) % F == 0) p1 = -1.0;
      if ((2 * k + 2) % F == 0) p2 = -1.0;
    }
    return c > m2 && c > m1 && c > p1 && c > p2;
  }
  __device__ __forceinline__ int wrapped(int kk) const { return kk < 0 ? kk + F : (kk >= F ? kk - F : kk); }
  __device__ __forceinline__ int abs_ks(int p) const { return two_sided && p > F / 2 ? F - p : p; }
  // phi - theta of the peak at bin p
  __device__ __forceinline__ double rot(int p) const {
#pragma clang fp contract(off)
    const cplx<T> s = s0[(int64_t)p * Tin];
    return phi[(int64_t)p * Tout] - (double)pvoc_angle(s.x, s.y);
  }
};

template <typename T>
__global__ void __launch_bounds__(256) k_pvoc_lock_apply(const cplx<T>* __restrict__ in, const double* __restrict__ phi,
                                                         cplx<T>* __restrict__ out, int B, int F, int Tin, int Tout, double rate,
                                                         int two_sided, int chunks, int bands) {
#pragma clang fp contract(off)
  const int64_t w = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int band = (int)(w % bands);
  const int chunk = (int)((w / bands) % chunks);
  const int64_t b = w / ((int64_t)bands * chunks);
  const int j = chunk * 64 + (threadIdx.x & 63);
  if (b >= B || j >= Tout) return;                         // (no lane below talks to another)
  const double t = (double)j * rate;
  const double fl = floor(t);
  const int64_t i = (int64_t)fl;                           // j < Tout keeps i below Tin (pvoc_lock_launch checks Tout)
  if (i >= Tin) return;
  const double a = t - fl;
  PvocLockFrame<T> f;
  f.s0 = in + b * F * Tin + i;
  f.phi = phi + b * F * Tout + j;
  f.F = F;
  f.Tin = Tin;
  f.Tout = Tout;
  f.two_sided = two_sided != 0;
  f.has1 = i + 1 < Tin;
  cplx<T>* ocol = out + b * F * Tout + j;
  const int k0 = band * kPvocLockBand;
  const int k1 = min(F, k0 + kPvocLockBand);

  // the band's peaks: bit k - k0
  unsigned long long mask = 0;
  {
    double m2 = f.q(k0 - 2), m1 = f.q(k0 - 1), c = f.q(k0), p1 = f.q(k0 + 1);
    for (int k = k0; k < k1; ++k) {
      const double p2 = f.q(k + 2);
      if (f.peak(k, m2, m1, c, p1, p2)) mask |= 1ull << (k - k0);
      m2 = m1;
      m1 = c;
      c = p1;
      p1 = p2;
    }
  }
  // The nearest peak below the band and the nearest above it, as indices that run on past 0 and F - 1 on a two-sided spectrum
  // (the distance to a bin of the band is then the plain difference).  With a peak in the band, one further from the band's edge
  // than the band's own first / last peak owns no bin of the band; without one the search ends at the spectrum's end, or after
  // one turn.
  const int first = mask ? k0 + __builtin_ctzll(mask) : 0;
  const int last = mask ? k0 + 63 - __builtin_clzll(mask) : 0;
  int lo = 0, hi = 0;
  bool has_lo = false, has_hi = mask != 0;
  {
    const int reach = f.two_sided ? F - 1 : k0;
    const int steps = mask ? min(first - k0, reach) : reach;
    double m1 = f.q(k0 - 2), c = f.q(k0 - 1), p1 = f.q(k0), p2 = f.q(k0 + 1);
    for (int s = 1; s <= steps && !has_lo; ++s) {
      const double m2 = f.q(k0 - s - 2);
      if (f.peak(f.wrapped(k0 - s), m2, m1, c, p1, p2)) {
        has_lo = true;
        lo = k0 - s;
      }
      p2 = p1;
      p1 = c;
      c = m1;
      m1 = m2;
    }
  }
  if (mask) {
    hi = first;
  }
  int up = 0;
  bool has_up = false;
  {
    const int reach = f.two_sided ? F - 1 : F - k1;
    const int steps = mask ? min(k1 - 1 - last, reach) : reach;
    double m2 = f.q(k1 - 2), m1 = f.q(k1 - 1), c = f.q(k1), p1 = f.q(k1 + 1);
    for (int s = 1; s <= steps && !has_up; ++s) {
      const double p2 = f.q(k1 + s + 1);
      if (f.peak(f.wrapped(k1 - 1 + s), m2, m1, c, p1, p2)) {
        has_up = true;
        up = k1 - 1 + s;
      }
      m2 = m1;
      m1 = c;
      c = p1;
      p1 = p2;
    }
  }
  if (!mask) {
    has_hi = has_up;
    hi = up;
  }
  const bool any = has_lo || has_hi;
  double r_lo = 0, r_hi = 0;
  if (has_lo) r_lo = f.rot(f.wrapped(lo));
  if (has_hi) r_hi = f.rot(f.wrapped(hi));

  for (int k = k0; k < k1; ++k) {
    const cplx<T> s0 = f.s0[(int64_t)k * Tin];
    cplx<T> s1 = mk<T>(T(0), T(0));
    if (f.has1) s1 = f.s0[(int64_t)k * Tin + 1];
    double psi;
    if (any) {
      bool take_lo = has_lo;
      if (has_lo && has_hi) {
        const int dl = k - lo, dh = hi - k;
        const int pl = f.wrapped(lo), ph = f.wrapped(hi);
        const int al = f.abs_ks(pl), ah = f.abs_ks(ph);
        take_lo = dl < dh || (dl == dh && (al < ah || (al == ah && pl <= ph)));
      }
      psi = (take_lo ? r_lo : r_hi) + (double)pvoc_angle(s0.x, s0.y);
    } else {
      psi = f.phi[(int64_t)k * Tout];
    }
    const double m = a * pvoc_abs(s1.x, s1.y) + (1.0 - a) * pvoc_abs(s0.x, s0.y);
    double sn, cs;
    sincos_phase(psi, &sn, &cs);
    ocol[(int64_t)k * Tout] = mk<T>((T)(m * cs), (T)(m * sn));
    if (has_hi && k == hi) {                               // past a peak of the band: it is the peak below from here on
      lo = hi;
      r_lo = r_hi;
      has_lo = true;
      const unsigned long long rest = k - k0 + 1 < 64 ? mask >> (k - k0 + 1) : 0;
      if (rest) {
        hi = k + 1 + __builtin_ctzll(rest);
        r_hi = f.rot(hi);
      } else {
        has_hi = has_up;
        hi = up;
        if (has_up) r_hi = f.rot(f.wrapped(up));
      }
    }
  }
}

// Host side (tu_pvoc_lock.hip): the two launches.  in (batch, n_freq, n_in), out (batch, n_freq, n_out), phi batch * n_freq * n_out
// doubles of scratch.
template <typename T>
int pvoc_lock_launch(const cplx<T>* in, cplx<T>* out, double* phi, int batch, int n_freq, int n_in, int n_out, double rate,
                     int n_fft, int hop, bool two_sided, hipStream_t stream);

}  // namespace specinv
