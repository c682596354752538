// Time-domain time-scale modification: waveform-similarity overlap-add (WSOLA, Verhelst & Roelands 1993) and, with
// a tolerance of 0, plain overlap-add (OLA).  x is (B, L) real, N = frame even in 2 ... 2048, Hs = hop in 1 ... N the synthesis
// hop, D = tol in 0 ... 1024, w a real window of N entries, xz(i) = x[i] for 0 <= i < L and 0 elsewhere.
//   Frames.  M = (n_out - 1 + N/2) / Hs + 1: exactly the frames whose support [m Hs - N/2, m Hs + N/2) meets [0, n_out).
//   Analysis centres.  a_m, m < M: non-decreasing int64, an input (the host makes floor(m Hs rate + 0.5) once in float64; the
//     kernels never evaluate that expression, which hipcc would contract into an fma).
//   Lag chain.  del_0 = 0; for m = 0 ... M - 2, with u_m = a_m + del_m - N/2:
//       p[n]      = xz(u_m + Hs + n), n < N                            (the natural continuation of frame m)
//       c[d]      = sum_n xz(a_{m+1} - N/2 + d + n) p[n], |d| <= D     (float64 products and sums for both dtypes)
//       del_{m+1} = the d with the largest c[d]; among equals the smallest |d|; of +-d the negative one
//   Overlap-add.  For 0 <= j < n_out, over the frames m in [0, M) with 0 <= n = j - m Hs + N/2 < N, in ascending m, in float64:
//       acc[j] = sum_m w[n] xz(u_m + n)      ow[j] = sum_m w[n]
//       y[j]   = acc[j] / (ow[j] >= 1e-3 ? ow[j] : 1), rounded once to T
//   D = 0 is plain OLA: all lags are 0 and the chain is not run.  ow does not depend on the data.  NaN input is unspecified.
//
// k_wsola_lags, the serial part: one workgroup of 512 lanes per item walks m = 0 ... M - 2; the only dependence between steps is
// the integer del_m, so a device-wide barrier per frame would cost more than a step and the chain stays inside one workgroup.
//   Regions.  E_m[i] = xz(a_m - N/2 - D + i), i < len = N + 2 D + Hs + 16, lives in LDS: it holds the search region of the step
//     that ends in frame m (offset d + D + n) and every possible p of the step that starts from it (offset D + del_m + Hs + n),
//     and 16 more samples so that a lane may run a few lags and a few n past the end without a bounds test (a product past the
//     end is taken with p = 0, a lag past D never enters the arg-max).  Two buffers: step m reads E_m and E_{m+1}.  The loads of
//     E_{m+2} depend on no lag: every lane issues its share (13 values at most) into registers before the step's sums and
//     writes them over E_m after them.  A centre is clamped to [-8192, L + 8192] first - beyond either end every read of that
//     frame is outside the row and zero, with or without the clamp - so no centre, however large, can overflow an index, and
//     every global read is guarded against [0, L).
//   Sums.  A lane owns 9 consecutive lags as a sliding window of 9 registers: per n one broadcast read of p[n], one new region
//     element and 9 float64 fmas; the loop is unrolled by 9 so that the window rotates by renaming.  The lane stride is 9
//     elements because it is odd: 9 dwords (float) or 18 (double) per lane put the 32 lanes of an LDS lane group on 32
//     different banks, where a stride of 8 would put them on 4 (an 8-way conflict).  With G = ceil((2 D + 1) / 9) lag groups
//     the 512 lanes are G x S: the n axis is cut into S = min(512 / G, ...) slices, and the S partial sums of a lag go
//     through LDS and are added in slice order (the result does not depend on timing).
//   Arg-max.  The key is lexicographic, (c, -|d|, -d): lane-local over the lags tid, tid + 512, ..., then a 64-lane butterfly,
//     then the 8 wave results through LDS, which every lane reduces itself.  Two barriers per step.
//   LDS: 2 len sizeof(T) + 8 * 9 * 512 (partials) + 128 bytes, 135 552 at the limits in float64 (dynamic, raised by attribute).
//
// k_wsola_ola, the parallel part: one lane per output sample, 256 consecutive samples of one item per workgroup; a sample sums
// its at most ceil(N / Hs) + 1 frames in ascending m with ow beside it, divides, rounds once.  Neighbouring lanes read
// neighbouring samples of the same frames.
#pragma once
#include "common.h"

namespace specinv {

constexpr int kWsolaMaxFrame = 2048;
constexpr int kWsolaMaxTol = 1024;
constexpr int kWsolaThreads = 512;         // k_wsola_lags
constexpr int kWsolaRun = 9;               // consecutive lags per lane (odd: see above)
constexpr int kWsolaPad = 16;              // region samples past N + 2 D + Hs
constexpr int kWsolaPrefetch = 13;         // ceil((2048 + 2048 + 2048 + 16) / 512) region values per lane
constexpr int kWsolaTile = 256;            // k_wsola_ola: outputs per workgroup
constexpr int64_t kWsolaClamp = 8192;      // > N/2 + D + N + Hs + pad at the limits

struct WsolaArgs {
  int64_t n_in, n_out;
  int64_t tiles;       // k_wsola_ola: workgroups per item
  int n_frames;        // M
  int frame, hop, tol; // N, Hs, D
  int len;             // region length, N + 2 D + Hs + kWsolaPad
  int groups;          // G: lag groups of kWsolaRun
  int slices;          // S: cuts of the n axis
  int slice_len;       // n per slice, a multiple of kWsolaRun
};

__device__ __forceinline__ int64_t wsola_centre(const int64_t* __restrict__ centres, int m, int64_t n_in) {
  const int64_t a = centres[m];
  return a < -kWsolaClamp ? -kWsolaClamp : a > n_in + kWsolaClamp ? n_in + kWsolaClamp : a;
}

// (c1, d1) comes before (c2, d2) under the key (c, -|d|, -d)
__device__ __forceinline__ bool wsola_better(double c1, int d1, double c2, int d2) {
  if (c1 != c2) return c1 > c2;
  const int a1 = d1 < 0 ? -d1 : d1, a2 = d2 < 0 ? -d2 : d2;
  return a1 != a2 ? a1 < a2 : d1 < d2;
}

// x (B, L), centres (M), lags (B, M) int32; item block0 + blockIdx.x
template <typename T>
__global__ void __launch_bounds__(kWsolaThreads) k_wsola_lags(const T* __restrict__ x, const int64_t* __restrict__ centres,
                                                              int32_t* __restrict__ lags, int64_t block0, WsolaArgs a) {
  extern __shared__ double wsola_lds[];
  double* part = wsola_lds;                                         // [slices][groups * kWsolaRun]
  double* wbest_c = part + (size_t)kWsolaRun * kWsolaThreads;       // [8]
  int* wbest_d = reinterpret_cast<int*>(wbest_c + 8);               // [8]
  T* buf0 = reinterpret_cast<T*>(wbest_c + 16);
  T* buf1 = buf0 + a.len;

  const int tid = threadIdx.x;
  const int64_t item = block0 + blockIdx.x;
  const T* xrow = x + item * a.n_in;
  int32_t* lrow = lags + item * a.n_frames;
  const int half = a.frame >> 1;
  const int n_lags = 2 * a.tol + 1;
  const int row = a.groups * kWsolaRun;                             // partial sums per slice (>= n_lags)

  auto region_value = [&](int64_t first, int i) -> T {
    const int64_t s = first + i;
    return i < a.len && s >= 0 && s < a.n_in ? xrow[s] : T(0);
  };
  // E_0 and E_1
  for (int e = 0; e < 2; ++e) {
    const int64_t first = wsola_centre(centres, e, a.n_in) - half - a.tol;
    T* buf = e ? buf1 : buf0;
    for (int i = tid; i < a.len; i += kWsolaThreads) buf[i] = region_value(first, i);
  }
  if (tid == 0) lrow[0] = 0;
  __syncthreads();

  const int g = tid % a.groups, s = tid / a.groups;
  const bool active = s < a.slices;
  const int nb = s * a.slice_len;
  const int ne = nb + a.slice_len < a.frame ? nb + a.slice_len : a.frame;
  int del = 0;
  for (int m = 0; m + 1 < a.n_frames; ++m) {
    T* cur = (m & 1) ? buf1 : buf0;                // E_m: p
    const T* nxt = (m & 1) ? buf0 : buf1;          // E_{m+1}: the search region
    // the loads of E_{m+2}, in flight during the sums
    T pre[kWsolaPrefetch];
    const bool more = m + 2 < a.n_frames;
    if (more) {
      const int64_t first = wsola_centre(centres, m + 2, a.n_in) - half - a.tol;
#pragma unroll
      for (int q = 0; q < kWsolaPrefetch; ++q) pre[q] = region_value(first, tid + q * kWsolaThreads);
    }
    if (active) {
      const T* pp = cur + a.tol + del + a.hop;     // p[n] = pp[n]
      const T* rr = nxt + g * kWsolaRun;           // lag index l = g * 9 + j reads rr[j + n]
      double c[kWsolaRun], w[kWsolaRun];
#pragma unroll
      for (int j = 0; j < kWsolaRun; ++j) c[j] = 0.0;
#pragma unroll
      for (int j = 0; j < kWsolaRun - 1; ++j) w[j] = (double)rr[nb + j];
      for (int n = nb; n < ne; n += kWsolaRun) {
#pragma unroll
        for (int u = 0; u < kWsolaRun; ++u) {
          // the window holds rr[n + u + j], j < 8, in slots (u + j) % 9; the ninth comes in
          w[(u + kWsolaRun - 1) % kWsolaRun] = (double)rr[n + u + kWsolaRun - 1];
          const double pv = n + u < ne ? (double)pp[n + u] : 0.0;
#pragma unroll
          for (int j = 0; j < kWsolaRun; ++j) c[j] = fma(w[(u + j) % kWsolaRun], pv, c[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < kWsolaRun; ++j) part[s * row + g * kWsolaRun + j] = c[j];
    }
    __syncthreads();
    // a lag's slices in order, the lane's lags, the wave
    double best_c = -__builtin_inf();
    int best_d = 0;
    for (int l = tid; l < n_lags; l += kWsolaThreads) {
      double sum = part[l];
      for (int q = 1; q < a.slices; ++q) sum += part[q * row + l];
      const int d = l - a.tol;
      if (wsola_better(sum, d, best_c, best_d)) {
        best_c = sum;
        best_d = d;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double oc = __shfl_xor(best_c, off, 64);
      const int od = __shfl_xor(best_d, off, 64);
      if (wsola_better(oc, od, best_c, best_d)) {
        best_c = oc;
        best_d = od;
      }
    }
    if ((tid & 63) == 0) {
      wbest_c[tid >> 6] = best_c;
      wbest_d[tid >> 6] = best_d;
    }
    if (more) {
#pragma unroll
      for (int q = 0; q < kWsolaPrefetch; ++q) {
        const int i = tid + q * kWsolaThreads;
        if (i < a.len) cur[i] = pre[q];
      }
    }
    __syncthreads();
    best_c = wbest_c[0];
    best_d = wbest_d[0];
#pragma unroll
    for (int q = 1; q < kWsolaThreads / 64; ++q) {
      const double oc = wbest_c[q];
      const int od = wbest_d[q];
      if (wsola_better(oc, od, best_c, best_d)) {
        best_c = oc;
        best_d = od;
      }
    }
    del = best_d;                                  // |del| <= D: every candidate is a lag of the search, or the initial 0
    if (tid == 0) lrow[m + 1] = del;
  }
}

// x (B, L), centres (M), window (N), lags (B, M) -> y (B, n_out); workgroup block0 + blockIdx.x of B * tiles
template <typename T>
__global__ void __launch_bounds__(kWsolaTile) k_wsola_ola(const T* __restrict__ x, const int64_t* __restrict__ centres,
                                                          const T* __restrict__ window, const int32_t* __restrict__ lags,
                                                          T* __restrict__ y, int64_t block0, WsolaArgs a) {
#pragma clang fp contract(off)
  const int64_t blk = block0 + blockIdx.x;
  const int64_t item = blk / a.tiles;
  const int64_t j = (blk - item * a.tiles) * kWsolaTile + threadIdx.x;
  if (j >= a.n_out) return;
  const T* xrow = x + item * a.n_in;
  const int32_t* lrow = lags + item * a.n_frames;
  const int half = a.frame >> 1;
  // 0 <= j - m Hs + N/2 < N  <=>  j - N/2 < m Hs <= j + N/2
  const int64_t below = j - half;
  int64_t m_lo = below < 0 ? 0 : below / a.hop + 1;
  int64_t m_hi = (j + half) / a.hop;
  if (m_hi > a.n_frames - 1) m_hi = a.n_frames - 1;
  double acc = 0.0, ow = 0.0;
  for (int64_t m = m_lo; m <= m_hi; ++m) {
    const int n = (int)(j - m * a.hop + half);
    const int64_t i = wsola_centre(centres, (int)m, a.n_in) + lrow[m] - half + n;
    const double wv = (double)window[n];
    const double v = i >= 0 && i < a.n_in ? (double)xrow[i] : 0.0;
    acc += wv * v;
    ow += wv;
  }
  y[item * a.n_out + j] = (T)(acc / (ow >= 1e-3 ? ow : 1.0));
}

}  // namespace specinv
