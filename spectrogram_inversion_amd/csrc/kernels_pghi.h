// Phase gradient heap integration, real-time form with one look-ahead frame (Prusa, Balazs & Sondergaard 2017, Prusa &
// Sondergaard 2016): a phase for magnitudes alone.  s (B, F, T) real, N = n_fft even, a = hop, F = N/2 + 1, g = gamma.  All
// arithmetic is float64 for both dtypes (contraction off: the sums are the definition's, operation by operation).
//   floor = tol * max(0, max s) per item ; (m,n) live iff s > 0 and s >= floor ; l = log(max(s, floor)), l[-1] = l[1], l[F] = l[F-2]
//   wt[m,n] = (2 pi / N) ((a m) mod N) + (a N / g) ((l[m+1,n] - l[m-1,n]) / 2)
//   wf[m,n] = pi - (g / (a N)) D[m,n],  D = (l[m,n+1] - l[m,n-1]) / 2, one-sided at n = 0 and n = T-1, 0 for T = 1
//   Frame n:  c[m] = s[m,n] if live else -inf ; p[m] = s[m,n-1] if live else -inf (n = 0: -inf but for the lowest-index maximum of
//     frame 0, +inf if live) ;  Lf[0] = -inf, Lf[m] = min(c[m-1], max(p[m-1], Lf[m-1])) ;  Rg[F-1] = -inf,
//     Rg[m] = min(c[m+1], max(p[m+1], Rg[m+1])) ;  b = max(p, Lf, Rg) ;  code 0 if p >= b, else 1 if Lf >= b, else 2 ; not live: 3
//   phi:  0: phi[m,n-1] + (wt[m,n-1] + wt[m,n]) / 2 (frame 0: 0) ;  1: phi[m-1,n] + (wf[m-1,n] + wf[m,n]) / 2 ;
//         2: phi[m+1,n] - (wf[m+1,n] + wf[m,n]) / 2 ;  3: 0
//   out = (s cos phi, s sin phi), rounded once.
//
// k_pghi<T, NT, K>: a workgroup of NT lanes (four waves as shipped; one wave was measured and dropped) owns an item and walks its
// frames; items beyond the grid are looped over.  The frame chain never leaves the compute unit.
//   Pre-pass.  The workgroup reduces the item's maximum (one coalesced sweep), loads frames 0 and 1 and finds frame 0's seed.
//   Layout.  Lane t owns the K consecutive bins [t K, t K + K), K = ceil(F / NT) made odd (a template parameter: 1, 3 ... 13): K
//     doubles per lane is then an odd number of bank pairs and the lanes of an LDS lane group fall on different banks.  Serial
//     inside the chunk, a shuffle ladder across the 64 lanes, the waves' totals through LDS.
//   State in LDS, a rolling window of three frames (n-1, n, n+1): l with its two mirror bins, and s.  phi of frame n-1, overwritten
//     in place by frame n's.  wt of frame n-1 is evaluated again from l[., n-1]: the same operations give the same bits.  A frame's
//     own values - c, p, Lf, the codes, the phase steps - are K registers each: every loop over the chunk is unrolled, a slot
//     past the item's last bin holds the identity clamp (c = +inf, p = -inf).
//   Prefetch.  The magnitudes of frame n+2 are requested into K registers at the top of frame n and written over frame n-1's
//     slot, with their logarithms, at its end.
//   Per frame.  (1) each lane folds its chunk's clamps x -> min(c, max(p, x)) into one (lo, hi) pair in both directions ; an
//     exclusive prefix scan and an exclusive suffix scan of the pairs (a clamp after a clamp is a clamp: (f2 . f1) = (f2(lo1),
//     f2(hi1))) give Lf at the chunk's first bin and Rg at its last ; (2) the lane runs both recurrences through its chunk and
//     selects the parents ; (3) per bin the value the phase is made of - the finished phase for codes 0 and 3, the step -(wf + wf)/2
//     or +(wf + wf)/2 for codes 2 and 1 ; (4) a segmented suffix sum (chains of code 2 end in a code-0 root on their right), then a
//     segmented prefix sum (chains of code 1 start from a code-0 or code-2 root on their left) ; (5) sincos and the stores.
//   Barriers per frame: 2 around the window's rotation, and with four waves 3 more for the scans' totals.
//   LDS: 8 (4 F + 6) + 3 sizeof(T) F + 512 bytes (l x 3, phi ; s x 3 ; totals): 56 F + 560 in float64, 163 800 of the 163 840 at
//     F = 2915.  Dynamic, raised by attribute.
#pragma once
#include "common.h"

namespace specinv {

constexpr int kPghiMaxFreq = 2915;                   // 56 F + 560 bytes <= 160 KiB
constexpr int kPghiMaxFft = 2 * (kPghiMaxFreq - 1);  // 5828
constexpr int kPghiScratch = 512;                    // bytes of totals in front of the arrays
constexpr int kPghiThreads = 256;                    // four waves: one wave per item took 1.8 - 2.6 x as long (tools/log/EXPERIMENTS.md)
constexpr int kPghiMaxChunk = 13;                    // bins per lane: 256 x 13 = 3328
static_assert(56 * kPghiMaxFreq + 48 + kPghiScratch <= 160 * 1024, "k_pghi: the state of a frame must fit a compute unit's LDS");
static_assert(kPghiMaxChunk % 2 == 1 && kPghiThreads * kPghiMaxChunk >= kPghiMaxFreq,
              "k_pghi: ceil(F / lanes) made odd must not exceed the largest chunk");

struct PghiArgs {
  int64_t batch;
  int n_freq, n_frames, n_fft;
  unsigned hop_mod;    // a mod N: (a m) mod N = ((a mod N) m) mod N stays below 2^32
  double kt, kf;       // a N / gamma, gamma / (a N)
  double w0;           // 2 pi / N
  double tol;
};

inline size_t pghi_lds_bytes(int n_freq, size_t elem) {
  return kPghiScratch + 8 * (4 * (size_t)n_freq + 6) + 3 * elem * (size_t)n_freq;
}

// x -> min(hi, max(lo, x)), lo <= hi
struct PghiClamp {
  double lo, hi;
};
__device__ __forceinline__ double pghi_apply(double c, double p, double x) { return fmin(c, fmax(p, x)); }
// `later` after `earlier`
__device__ __forceinline__ PghiClamp pghi_after(PghiClamp later, PghiClamp earlier) {
  PghiClamp r;
  r.lo = fmin(later.hi, fmax(later.lo, earlier.lo));
  r.hi = fmin(later.hi, fmax(later.lo, earlier.hi));
  return r;
}
// a segmented sum's state: the sum back to the nearest root, and whether there is one
struct PghiSeg {
  double sum;
  int root;
};
__device__ __forceinline__ PghiSeg pghi_after(PghiSeg later, PghiSeg earlier) {
#pragma clang fp contract(off)
  PghiSeg r;
  r.sum = later.root ? later.sum : earlier.sum + later.sum;
  r.root = later.root | earlier.root;
  return r;
}
template <bool UP>
__device__ __forceinline__ PghiClamp pghi_shfl(PghiClamp v, int off) {
  PghiClamp r;
  r.lo = UP ? __shfl_up(v.lo, off, 64) : __shfl_down(v.lo, off, 64);
  r.hi = UP ? __shfl_up(v.hi, off, 64) : __shfl_down(v.hi, off, 64);
  return r;
}
template <bool UP>
__device__ __forceinline__ PghiSeg pghi_shfl(PghiSeg v, int off) {
  PghiSeg r;
  r.sum = UP ? __shfl_up(v.sum, off, 64) : __shfl_down(v.sum, off, 64);
  r.root = UP ? __shfl_up(v.root, off, 64) : __shfl_down(v.root, off, 64);
  return r;
}
// inclusive scan over the wave: UP folds the lanes below into each lane (a prefix), else the lanes above (a suffix)
template <bool UP, typename V>
__device__ __forceinline__ V pghi_wave_scan(V v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const V o = pghi_shfl<UP>(v, off);
    if (UP ? lane >= off : lane + off < 64) v = pghi_after(v, o);
  }
  return v;
}
// from the wave's inclusive scan to the workgroup's exclusive one: `totals` holds every wave's fold (written before the barrier the
// caller placed); `ident` is what the first lane gets
template <bool UP, int NW, typename V>
__device__ __forceinline__ V pghi_exclusive(V incl, const V* totals, V ident, int lane, int wave) {
  V e = pghi_shfl<UP>(incl, 1);
  if (UP ? lane == 0 : lane == 63) e = ident;
  if (NW > 1) {
    V before = ident;
    if (UP) {
      for (int w = 0; w < wave; ++w) before = pghi_after(totals[w], before);
    } else {
      for (int w = NW - 1; w > wave; --w) before = pghi_after(totals[w], before);
    }
    e = pghi_after(e, before);
  }
  return e;
}

template <typename T, int NT, int K>
__global__ void __launch_bounds__(NT) k_pghi(const T* __restrict__ mag, cplx<T>* __restrict__ out, double* __restrict__ phase_out,
                                             int8_t* __restrict__ parents_out, PghiArgs a) {
#pragma clang fp contract(off)
  constexpr int NW = NT / 64;
  constexpr double kInf = __builtin_inf();
  constexpr double kPi = 3.14159265358979323846;
  extern __shared__ double pghi_lds[];
  const int F = a.n_freq, T_ = a.n_frames;
  // scratch: [0, 128) clamp totals up, [128, 256) clamp totals down, [256, 384) sums, [384, 512) the reductions
  PghiClamp* tot_up = reinterpret_cast<PghiClamp*>(pghi_lds);
  PghiClamp* tot_dn = tot_up + 8;
  PghiSeg* tot_seg = reinterpret_cast<PghiSeg*>(pghi_lds + 32);
  double* red_v = pghi_lds + 48;
  int* red_i = reinterpret_cast<int*>(pghi_lds + 56);
  double* ell = pghi_lds + kPghiScratch / 8;                 // [3][F + 2], bin m at m + 1
  double* phi = ell + 3 * (size_t)(F + 2);                   // [F]
  T* sv = reinterpret_cast<T*>(phi + F);                     // [3][F]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = tid * K < F ? tid * K : F;
  const int m1 = m0 + K < F ? m0 + K : F;

  for (int64_t item = blockIdx.x; item < a.batch; item += gridDim.x) {
    const T* row = mag + item * F * T_;
    const int64_t total = (int64_t)F * T_;
    // the item's maximum
    double mx = 0.0;
#pragma unroll 8
    for (int64_t i = tid; i < total; i += NT) {        // (unrolled: eight independent loads in flight, not one)
      const double v = (double)row[i];
      if (v > mx) mx = v;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
    if (NW > 1) {
      if (lane == 0) red_v[wave] = mx;
      __syncthreads();
      mx = red_v[0];
      for (int w = 1; w < NW; ++w) mx = fmax(mx, red_v[w]);
    }
    const double floor_ = a.tol * mx;
    auto is_live = [&](T s) { return s > T(0) && (double)s >= floor_; };
    auto put_frame = [&](int slot, int m, T s) {
      sv[slot * (size_t)F + m] = s;
      const double dv = (double)s;
      const double l = log(dv > floor_ ? dv : floor_);
      double* e = ell + slot * (size_t)(F + 2);
      e[m + 1] = l;
      if (m == 1) e[0] = l;
      if (m == F - 2) e[F + 1] = l;
    };
    // frames 0 and 1, and frame 0's seed: its lowest-index maximum, if live
    double best = -kInf;
    int seed = 0;
    for (int m = m0; m < m1; ++m) {
      const T s0 = row[(int64_t)m * T_];
      put_frame(0, m, s0);
      if (T_ > 1) put_frame(1, m, row[(int64_t)m * T_ + 1]);
      phi[m] = 0.0;
      if ((double)s0 > best) {
        best = (double)s0;
        seed = m;
      }
    }
    if (m0 >= m1) seed = F;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double ov = __shfl_xor(best, off, 64);
      const int oi = __shfl_xor(seed, off, 64);
      if (ov > best || (ov == best && oi < seed)) {
        best = ov;
        seed = oi;
      }
    }
    if (NW > 1) {
      if (lane == 0) {
        red_v[4 + wave] = best;
        red_i[wave] = seed;
      }
    }
    __syncthreads();
    if (NW > 1) {
      best = red_v[4];
      seed = red_i[0];
      for (int w = 1; w < NW; ++w)
        if (red_v[4 + w] > best || (red_v[4 + w] == best && red_i[w] < seed)) {
          best = red_v[4 + w];
          seed = red_i[w];
        }
    }
    if (!(best > 0.0 && best >= floor_)) seed = -1;

    for (int n = 0; n < T_; ++n) {
      const int ic = n % 3, ip = (n + 2) % 3, in = (n + 1) % 3;
      const double* eP = ell + ip * (size_t)(F + 2);
      const double* eC = ell + ic * (size_t)(F + 2);
      const double* eN = ell + in * (size_t)(F + 2);
      const T* sC = sv + ic * (size_t)F;
      const T* sP = sv + ip * (size_t)F;
      const bool has_p = n > 0, has_n = n + 1 < T_, more = n + 2 < T_;
      // frame n + 2, in flight during the frame
      T pre[K];
      if (more) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
          const int m = m0 + j;
          pre[j] = m < m1 ? row[(int64_t)m * T_ + n + 2] : T(0);
        }
      }
      // the chunk in registers; a slot past the chunk's end holds the identity clamp
      double c[K], p[K], v[K];
      T sc[K];
      int cd[K];
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const int m = m0 + j;
        sc[j] = T(0);
        c[j] = kInf;
        p[j] = -kInf;
        if (m < m1) {
          sc[j] = sC[m];
          c[j] = is_live(sc[j]) ? (double)sc[j] : -kInf;
          if (has_p) {
            const T q = sP[m];
            p[j] = is_live(q) ? (double)q : -kInf;
          } else {
            p[j] = m == seed ? kInf : -kInf;
          }
        }
      }
      // (1) the chunk's clamps folded upwards and downwards, scanned
      const PghiClamp ident = {-kInf, kInf};
      PghiClamp up = ident, dn = ident;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        up.lo = pghi_apply(c[j], p[j], up.lo);
        up.hi = pghi_apply(c[j], p[j], up.hi);
      }
#pragma unroll
      for (int j = K - 1; j >= 0; --j) {
        dn.lo = pghi_apply(c[j], p[j], dn.lo);
        dn.hi = pghi_apply(c[j], p[j], dn.hi);
      }
      up = pghi_wave_scan<true>(up, lane);
      dn = pghi_wave_scan<false>(dn, lane);
      if (NW > 1) {
        if (lane == 63) tot_up[wave] = up;
        if (lane == 0) tot_dn[wave] = dn;
        __syncthreads();
      }
      double x = pghi_exclusive<true, NW>(up, tot_up, ident, lane, wave).lo;      // Lf[m0]: the fold applied to -inf is its lo
      double y = pghi_exclusive<false, NW>(dn, tot_dn, ident, lane, wave).lo;     // Rg[m1 - 1]
      // (2) the recurrences through the chunk, the parents
#pragma unroll
      for (int j = 0; j < K; ++j) {
        v[j] = x;                        // Lf, until (3)
        x = pghi_apply(c[j], p[j], x);
      }
#pragma unroll
      for (int j = K - 1; j >= 0; --j) {
        cd[j] = 3;
        if (m0 + j < m1 && c[j] > -kInf) {
          const double b = fmax(p[j], fmax(v[j], y));
          cd[j] = p[j] >= b ? 0 : v[j] >= b ? 1 : 2;
        }
        y = pghi_apply(c[j], p[j], y);
      }
      // (3) what each bin's phase is made of
      auto wf = [&](int m) {             // bin m at index m + 1
        const double d = has_p && has_n ? (eN[m + 1] - eP[m + 1]) / 2.0
                         : has_n        ? eN[m + 1] - eC[m + 1]
                         : has_p        ? eC[m + 1] - eP[m + 1]
                                        : 0.0;
        return kPi - a.kf * d;
      };
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const int m = m0 + j;
        v[j] = 0.0;
        if (cd[j] == 0) {
          if (has_p) {
            const double base = a.w0 * (double)((a.hop_mod * (unsigned)m) % (unsigned)a.n_fft);
            const double wp = base + a.kt * ((eP[m + 2] - eP[m]) / 2.0);
            const double wc = base + a.kt * ((eC[m + 2] - eC[m]) / 2.0);
            v[j] = phi[m] + (wp + wc) / 2.0;
          }
        } else if (cd[j] == 1) {
          v[j] = (wf(m - 1) + wf(m)) / 2.0;
        } else if (cd[j] == 2) {
          v[j] = -((wf(m + 1) + wf(m)) / 2.0);
        }
      }
      // (4) chains of code 2 from their root on the right, then chains of code 1 from their root on the left
      const PghiSeg none = {0.0, 0};
      PghiSeg seg = none;
#pragma unroll
      for (int j = K - 1; j >= 0; --j) {
        if (m0 + j < m1) {
          PghiSeg e;
          e.sum = cd[j] == 1 ? 0.0 : v[j];
          e.root = cd[j] != 2;
          seg = pghi_after(e, seg);
        }
      }
      seg = pghi_wave_scan<false>(seg, lane);
      if (NW > 1) {
        if (lane == 0) tot_seg[wave] = seg;
        __syncthreads();
      }
      double run = pghi_exclusive<false, NW>(seg, tot_seg, none, lane, wave).sum;
#pragma unroll
      for (int j = K - 1; j >= 0; --j) {
        if (m0 + j < m1) {
          if (cd[j] == 2) {
            run = run + v[j];
            v[j] = run;
          } else {
            run = cd[j] == 1 ? 0.0 : v[j];
          }
        }
      }
      seg = none;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        if (m0 + j < m1) {
          PghiSeg e;
          e.sum = v[j];
          e.root = cd[j] != 1;
          seg = pghi_after(e, seg);
        }
      }
      seg = pghi_wave_scan<true>(seg, lane);
      if (NW > 1) {
        if (lane == 63) tot_seg[4 + wave] = seg;
        __syncthreads();
      }
      run = pghi_exclusive<true, NW>(seg, tot_seg + 4, none, lane, wave).sum;
      // (5) the outputs
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const int m = m0 + j;
        if (m < m1) {
          run = cd[j] == 1 ? run + v[j] : v[j];
          phi[m] = run;
          double sn, cs;
          sincos_moderate(run, &sn, &cs);
          const double s = (double)sc[j];
          const int64_t at = (item * F + m) * T_ + n;
          out[at] = mk<T>((T)(s * cs), (T)(s * sn));
          if (phase_out) phase_out[at] = run;
          if (parents_out) parents_out[at] = (int8_t)cd[j];
        }
      }
      // the window moves on: frame n + 2 over frame n - 1
      __syncthreads();
      if (more) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
          const int m = m0 + j;
          if (m < m1) put_frame(ip, m, pre[j]);
        }
      }
      __syncthreads();
    }
  }
}

}  // namespace specinv
