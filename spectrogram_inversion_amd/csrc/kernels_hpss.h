// Harmonic-percussive separation: two median filters over the magnitude of a spectrogram (B, F, T), one along time
// and one along frequency, and librosa's soft masks from the pair - librosa.decompose.hpss, in one launch.
//   A = S for a real input, sqrt(re^2 + im^2) in float64 for a complex one (for complex64 both squares are exact in float64).
//   refl(i, n) = j if j < n else 2 n - 1 - j, j = i mod 2 n (Python's mod): scipy's 'reflect', continued periodically.
//   harm[f, t] = median{ A[f, refl(t + d, T)] : |d| <= k_h / 2 },  perc[f, t] = median{ A[refl(f + d, F), t] : |d| <= k_p / 2 },
//   k_h, k_p odd in 1 ... 127: a median is an element of its window.
//   soft(X, R): Z = max(X, R); p = inf: X > R ? 1 : 0; else Z < tiny: (split ? 0.5 : 0); else a = (X / Z)^p, r = (R / Z)^p, a / (a + r);
//   M_h = soft(harm, m_h perc), M_p = soft(perc, m_p harm), split = (m_h == 1 and m_p == 1), tiny the smallest normal number of T.
//   From Z on everything is float64 for both dtypes and the result is rounded once; p = 1 and p = 2 are products, not pow.
//   Outputs: the components S M_h, S M_p (of S's kind), the masks, or the medians (real).
//
// Tile.  A workgroup of 256 lanes owns TF x 32 outputs (f, t) of one item.  TF = 32 where the 32-row tile takes no more than 32 KiB
// of LDS, else 16 (the host picks: hpss_tile_rows): float staging has 32 rows up to k_h + k_p = 129, double staging always 16,
// and the largest tile, (127, 127) in double, is 65024 bytes.  The selection waits for LDS, so the workgroups resident on a CU
// count for more than the halo a flatter tile re-reads: 48 KiB -> 28 KiB at (31, 31) in double is 0.44 -> 0.31 ms.  The halo is a
// cross, k_p - 1 rows above and below the tile's columns and k_h - 1 columns left and right of its rows; the corners belong to no
// window.  It is staged as two images with the reflection resolved and the magnitude taken once per staged element:
//   hs[TF][32 + k_h - 1]      the tile's rows, time along the row,
//   ps[32][(TF + k_p - 1) | 1]   the tile's columns, frequency along the row: the transposed image, so that the frequency-direction
//     filter walks its window at stride 1 like the time-direction one, with an odd row length so that the 32 lanes of a staging
//     write, one column each, fall on 32 banks.
// Staged values are T for a real input and double for a complex one of either width: the masks take the float64 magnitude.
//
// Selection, one path for every size: rank counting with a sliding rank.  A lane owns one staged element e = line[i], not one
// output.  Under the strict total order (value, then position) its rank in the window [s, s + k) is the count of elements below it;
// the lane counts it once for the first window that holds i (k reads), and from one window to the next it drops line[s] and takes
// in line[s + k] (2 reads), over the at most min(k, 32) windows of the tile that hold i.  Where the rank is k / 2 it writes e as
// window s's median: exactly one element of a window has that rank, so every output is written once, by one lane, with no atomics.
// A line of L = 32 + k - 1 elements and 32 windows costs L k reads for the first ranks and 2 (32 k - L) for the steps - 118 per
// output at k = 31 and 871 at k = 127, where counting every window on its own takes up to k^2 = 961 and 16129 (measured at B 16,
// 513 x 512 complex64, both on 32-row tiles: 0.44 against 2.85 ms and 3.1 against 63 ms; tools/log/EXPERIMENTS.md).  Lanes next to each other own
// neighbours of one line and read neighbours: stride 1, no bank conflict.  k = 1 is the same code (rank 0).
// The two medians go to two TF x 32 images in LDS; after a barrier lane (r, c) evaluates the masks of its outputs and writes rows
// of 32 consecutive t.  The components read S a second time there (an L2 hit: the workgroup staged it a moment ago).
// All loops are bounded by TF, 32 and k.  Offsets into global memory are 64-bit.
#pragma once
#include <cmath>

#include "common.h"

namespace specinv {

constexpr int kHpssThreads = 256;
constexpr int kHpssTileT = 32;               // outputs along time per workgroup
constexpr int kHpssMaxWin = 127;
constexpr int kHpssLdsBytes = 65536;         // what a workgroup may take: two and more share a CU's 160 KiB
constexpr int kHpssTileBytes = 32768;        // what a 32-row tile may take: five workgroups and more per CU, else 16 rows

struct HpssArgs {
  int64_t tiles_f, tiles_t;   // workgroups per item along each axis
  int n_freq, n_frames;
  int k_h, k_p;
  int tile_f;                 // TF: 32 or 16
  int mode;                   // SPECINV_HPSS_*
  int power_kind;             // 0: pow, 1: p = 1, 2: p = 2, 3: p = inf
  int split;                  // both margins are 1
  double power, m_h, m_p;
};

// rows per tile: 32 where the staged images of `elem` bytes per value fit kHpssTileBytes, else 16 (65024 bytes at most: it fits
// kHpssLdsBytes at every size)
inline int hpss_tile_rows(int k_h, int k_p, size_t elem, size_t* bytes_out) {
  for (int tf = 32;; tf = 16) {
    const size_t n = (size_t)tf * (kHpssTileT + k_h - 1) + (size_t)kHpssTileT * ((tf + k_p - 1) | 1) + 2 * (size_t)tf * kHpssTileT;
    if (n * elem <= (size_t)kHpssTileBytes || tf == 16) {
      *bytes_out = n * elem;
      return tf;
    }
  }
}

// refl(i, n) for any i of magnitude below 2^31 and 1 <= n < 2^31
__device__ __forceinline__ int hpss_refl(int64_t i, int n) {
  if (i >= 0 && i < n) return (int)i;
  const unsigned m = 2u * (unsigned)n;
  const unsigned j = i >= 0 ? (unsigned)i % m : m - 1u - (unsigned)(-i - 1) % m;
  return (int)(j < (unsigned)n ? j : m - 1u - j);
}

template <typename T, bool CPLX>
__device__ __forceinline__ auto hpss_mag(const T* __restrict__ spec, int64_t at) {
  if constexpr (CPLX) {
    const double re = (double)spec[2 * at], im = (double)spec[2 * at + 1];
    return sqrt(re * re + im * im);
  } else {
    return spec[at];
  }
}

// the medians of the windows [s, s + k), s = 0 ... n_out - 1, of n_lines lines of n_out + k - 1 staged elements (line l at
// src + l * src_stride), written to dst[l * dst_line + s * dst_elem]
template <typename ST>
__device__ __forceinline__ void hpss_select(const ST* __restrict__ src, int n_lines, int src_stride, int k, int n_out,
                                            ST* __restrict__ dst, int dst_line, int dst_elem) {
  const unsigned len = (unsigned)(n_out + k - 1);
  const int half = k >> 1;
  for (unsigned idx = threadIdx.x; idx < (unsigned)n_lines * len; idx += kHpssThreads) {
    const unsigned l = idx / len;
    const int i = (int)(idx - l * len);
    const ST* line = src + l * src_stride;
    const ST e = line[i];
    int s = i - k + 1 > 0 ? i - k + 1 : 0;              // the windows that hold i: s ... s_last
    const int s_last = i < n_out - 1 ? i : n_out - 1;
    int rank = 0;
#pragma unroll 4
    for (int j = s; j < s + k; ++j) {
      const ST v = line[j];
      rank += (v < e || (v == e && j < i)) ? 1 : 0;
    }
    ST* out = dst + l * dst_line;
    if (rank == half) out[s * dst_elem] = e;
    // window s -> s + 1 drops line[s], which lies before i (s < s_last <= i: a tie counted), and takes in line[s + k], which
    // lies behind it (s >= i - k + 1: a tie does not count); s + k <= s_last - 1 + k <= len - 1
    const int steps = s_last - s;
#pragma unroll 4
    for (int n = 0; n < steps; ++n) {
      rank += (line[s + k] < e ? 1 : 0) - (line[s] <= e ? 1 : 0);
      ++s;
      if (rank == half) out[s * dst_elem] = e;
    }
  }
}

__device__ __forceinline__ double hpss_soft(double x, double r, const HpssArgs& a, double tiny) {
  if (a.power_kind == 3) return x > r ? 1.0 : 0.0;
  const double z = x > r ? x : r;
  if (z < tiny) return a.split ? 0.5 : 0.0;
  double qa = x / z, qr = r / z;
  if (a.power_kind == 2) {
    qa = qa * qa;
    qr = qr * qr;
  } else if (a.power_kind == 0) {
    qa = pow(qa, a.power);
    qr = pow(qr, a.power);
  }
  return qa / (qa + qr);
}

// spec (B, F, T) of T, or of (re, im) pairs of T; out_a, out_b likewise for the components of a complex input, else real
template <typename T, bool CPLX>
__global__ void __launch_bounds__(kHpssThreads) k_hpss(const T* __restrict__ spec, T* __restrict__ out_a, T* __restrict__ out_b,
                                                       int64_t block0, HpssArgs a) {
#pragma clang fp contract(off)
  using ST = decltype(hpss_mag<T, CPLX>(spec, 0));
  extern __shared__ double hpss_lds[];
  const int tf = a.tile_f, tt = kHpssTileT;
  const int len_h = tt + a.k_h - 1, len_p = tf + a.k_p - 1, stride_p = len_p | 1;
  ST* hs = reinterpret_cast<ST*>(hpss_lds);
  ST* ps = hs + tf * len_h;
  ST* med_h = ps + tt * stride_p;
  ST* med_p = med_h + tf * tt;

  const int64_t blk = block0 + blockIdx.x;
  const int64_t per_item = a.tiles_f * a.tiles_t;
  const int64_t item = blk / per_item;
  const int64_t rest = blk - item * per_item;
  const int64_t tile_row = rest / a.tiles_t;
  const int64_t f0 = tile_row * tf, t0 = (rest - tile_row * a.tiles_t) * tt;
  const int64_t base = item * a.n_freq * (int64_t)a.n_frames;
  const int tid = threadIdx.x;

  // hs: wave w takes rows w, w + 4, ...; its lanes run along time.  A row beyond F is zeros: its medians are not written out.
  for (int r = tid >> 6; r < tf; r += kHpssThreads / 64) {
    const int64_t f = f0 + r;
    for (int i = tid & 63; i < len_h; i += 64) {
      ST v = ST(0);
      if (f < a.n_freq) v = hpss_mag<T, CPLX>(spec, base + f * a.n_frames + hpss_refl(t0 + i - (a.k_h >> 1), a.n_frames));
      hs[r * len_h + i] = v;
    }
  }
  // ps: 32 lanes run along time (one global row segment), the 8 groups of 32 take the staged rows g, g + 8, ...
  {
    const int c = tid & 31;
    const int64_t t = t0 + c;
    for (int i = tid >> 5; i < len_p; i += kHpssThreads / 32) {
      ST v = ST(0);
      if (t < a.n_frames) v = hpss_mag<T, CPLX>(spec, base + (int64_t)hpss_refl(f0 + i - (a.k_p >> 1), a.n_freq) * a.n_frames + t);
      ps[c * stride_p + i] = v;
    }
  }
  __syncthreads();
  hpss_select<ST>(hs, tf, len_h, a.k_h, tt, med_h, tt, 1);
  hpss_select<ST>(ps, tt, stride_p, a.k_p, tf, med_p, 1, tt);
  __syncthreads();

  const double tiny = sizeof(T) == 4 ? 1.17549435082228750797e-38 : 2.22507385850720138309e-308;
  for (int idx = tid; idx < tf * tt; idx += kHpssThreads) {
    const int r = idx >> 5, c = idx & 31;
    const int64_t f = f0 + r, t = t0 + c;
    if (f >= a.n_freq || t >= a.n_frames) continue;
    const int64_t at = base + f * a.n_frames + t;
    const ST xh = med_h[idx], xp = med_p[idx];
    if (a.mode == SPECINV_HPSS_MEDIANS) {
      out_a[at] = (T)xh;
      out_b[at] = (T)xp;
      continue;
    }
    const double mh = hpss_soft((double)xh, a.m_h * (double)xp, a, tiny);
    const double mp = hpss_soft((double)xp, a.m_p * (double)xh, a, tiny);
    if (a.mode == SPECINV_HPSS_MASKS) {
      out_a[at] = (T)mh;
      out_b[at] = (T)mp;
    } else if constexpr (CPLX) {
      const double re = (double)spec[2 * at], im = (double)spec[2 * at + 1];
      out_a[2 * at] = (T)(re * mh);
      out_a[2 * at + 1] = (T)(im * mh);
      out_b[2 * at] = (T)(re * mp);
      out_b[2 * at + 1] = (T)(im * mp);
    } else {
      const double s = (double)spec[at];
      out_a[at] = (T)(s * mh);
      out_b[at] = (T)(s * mp);
    }
  }
}

}  // namespace specinv
