// k_mel_nnls: the magnitude behind a mel spectrogram, min_s 1/2 |M s - y|^2 subject to s >= 0, per frame, by FISTA from s = 0
// (accelerated projected gradient, step 1 / L, L = lambda_max(M M^T); include/specinv.h: specinv_mel_nnls).
//
// A wave owns a frame for the whole run: its z, s (F each), residual and mel column (n_mels each) sit in a wave-private slice of
// LDS, so the n_iter iterations touch HBM twice per frame (y in, s out) and synchronise nothing beyond the wave.  The filterbank
// is held in band form (mel_nnls_build), staged once per workgroup when it fits beside the waves' slices:
//   rows:    M z as segments - a contiguous run of bins of one mel row, at most `piece` long, with its weights - so that the lanes
//            of a wave share the row products evenly whatever the bands' lengths; a row's residual is the sum of its segments;
//   columns: per bin the contiguous range of rows that touch it and their weights (<= 2 rows for a triangular bank), so that a
//            lane forms M^T r for its bins with a handful of multiply-adds.
// A band spans a row's (a column's) first to last non-zero entry; zeros inside it are stored, so any matrix - a dense one is a
// band of length F - gives the same result through the same kernel.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"

namespace specinv {
struct PlanBase;

namespace fast {

constexpr int kNnlsMaxWaves = 8;

template <typename T>
struct MelNnlsArgs {
  const T* y;                 // (B, n_mels, T)
  T* out;                     // (B, F, T)
  const double* beta;         // momentum of iteration k: (t_k - 1) / t_{k+1}
  const T* wr;                // row-segment weights
  const T* wc;                // column weights
  const int4* seg;            // segment: first bin, length, offset in wr, -
  const int* rowseg;          // row m: segments [rowseg[m], rowseg[m + 1])
  const int2* col;            // bin f: first row | row count << 16, offset in wc
  int F, n_mels, nseg, nwr, nwc;
  int frames, tgroups, n_groups, n_iter;
  int per_wave;               // elements of T in a wave's LDS slice
  int stage_bytes;            // bytes of the staged band form (0: read from global memory)
  T step;                     // 1 / L
  int root;                   // 1: s, 2: sqrt(s), 0: pow(s, inv_power)
  T inv_power;
};

__host__ __device__ constexpr int nnls_align16(int bytes) { return (bytes + 15) & ~15; }

template <typename T, bool STAGED>
__global__ __launch_bounds__(64 * kNnlsMaxWaves) void k_mel_nnls(MelNnlsArgs<T> a);

#if defined(__HIPCC__)
template <typename T, bool STAGED>
__global__ __launch_bounds__(64 * kNnlsMaxWaves) void k_mel_nnls(MelNnlsArgs<T> a) {
  extern __shared__ __align__(16) unsigned char nnls_lds[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, W = blockDim.x >> 6;
  const T* wr = a.wr;
  const T* wc = a.wc;
  const int4* seg = a.seg;
  const int* rowseg = a.rowseg;
  const int2* col = a.col;
  if constexpr (STAGED) {
    // layout of the stage: wr | wc | seg | col | rowseg, each 16-byte aligned (tu_mel_nnls.hip: stage_bytes)
    unsigned char* p = nnls_lds;
    T* swr = reinterpret_cast<T*>(p);
    p += nnls_align16(a.nwr * (int)sizeof(T));
    T* swc = reinterpret_cast<T*>(p);
    p += nnls_align16(a.nwc * (int)sizeof(T));
    int4* sseg = reinterpret_cast<int4*>(p);
    p += 16 * a.nseg;
    int2* scol = reinterpret_cast<int2*>(p);
    p += nnls_align16(8 * a.F);
    int* srow = reinterpret_cast<int*>(p);
    for (int i = threadIdx.x; i < a.nwr; i += blockDim.x) swr[i] = a.wr[i];
    for (int i = threadIdx.x; i < a.nwc; i += blockDim.x) swc[i] = a.wc[i];
    for (int i = threadIdx.x; i < a.nseg; i += blockDim.x) sseg[i] = a.seg[i];
    for (int i = threadIdx.x; i < a.F; i += blockDim.x) scol[i] = a.col[i];
    for (int i = threadIdx.x; i <= a.n_mels; i += blockDim.x) srow[i] = a.rowseg[i];
    wr = swr;
    wc = swc;
    seg = sseg;
    col = scol;
    rowseg = srow;
    __syncthreads();
  }
  // a wave's slice: z[F] | s[F] | r[n_mels] | y[n_mels] | part[nseg]
  T* const slices = reinterpret_cast<T*>(nnls_lds + a.stage_bytes);
  T* const z = slices + (size_t)w * a.per_wave;
  T* const s = z + a.F;
  T* const r = s + a.F;
  T* const yv = r + a.n_mels;
  T* const part = yv + a.n_mels;
  const int F = a.F, NM = a.n_mels;
  const T step = a.step;
  for (int grp = blockIdx.x; grp < a.n_groups; grp += gridDim.x) {
    const int b = grp / a.tgroups, t0 = (grp - b * a.tgroups) * W, t = t0 + w;
    if (t < a.frames) {
      for (int f = lane; f < F; f += 64) {
        z[f] = T(0);
        s[f] = T(0);
      }
      const T* yp = a.y + (size_t)b * NM * a.frames + t;
      for (int m = lane; m < NM; m += 64) yv[m] = yp[(size_t)m * a.frames];
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      for (int k = 0; k < a.n_iter; ++k) {
        // M z, one segment per lane at a time
        for (int q = lane; q < a.nseg; q += 64) {
          const int4 sg = seg[q];
          const T* wp = wr + sg.z;
          const T* zp = z + sg.x;
          T acc0 = T(0), acc1 = T(0);
          int i = 0;
          for (; i + 1 < sg.y; i += 2) {
            acc0 = fma(wp[i], zp[i], acc0);
            acc1 = fma(wp[i + 1], zp[i + 1], acc1);
          }
          if (i < sg.y) acc0 = fma(wp[i], zp[i], acc0);
          part[q] = acc0 + acc1;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        // r = M z - y
        for (int m = lane; m < NM; m += 64) {
          T acc = T(0);
          for (int q = rowseg[m]; q < rowseg[m + 1]; ++q) acc += part[q];
          r[m] = acc - yv[m];
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        // g = M^T r; s' = max(0, z - g / L); z = s' + beta_k (s' - s)
        const T beta = (T)a.beta[k];
        for (int f = lane; f < F; f += 64) {
          const int2 c = col[f];
          const int m0 = c.x & 0xffff, nc = c.x >> 16;
          const T* wp = wc + c.y;
          const T* rp = r + m0;
          T g = T(0);
          for (int j = 0; j < nc; ++j) g = fma(wp[j], rp[j], g);
          const T sn = fmax(T(0), z[f] - g * step);
          z[f] = sn + beta * (sn - s[f]);
          s[f] = sn;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      }
    }
    __syncthreads();
    // the workgroup's frames are consecutive: lanes run along t, so that W neighbouring samples of a bin leave together
    const int nt = min(W, a.frames - t0);
    T* op = a.out + (size_t)b * F * a.frames + t0;
    for (int i = threadIdx.x; i < F * W; i += blockDim.x) {
      const int f = i / W, tt = i - f * W;
      if (tt < nt) {
        const T v = slices[(size_t)tt * a.per_wave + F + f];
        op[(size_t)f * a.frames + tt] = a.root == 1 ? v : a.root == 2 ? sqrt(v) : (v > T(0) ? pow(v, a.inv_power) : T(0));
      }
    }
    __syncthreads();
  }
}
#endif

// ---- host side ------------------------------------------------------------------------------------------------------------------

// The band form of a (n_mels, F) matrix: what k_mel_nnls reads.  `piece` bounds a segment's length (chosen here so that a wave's
// lanes carry about equal shares of M z: the largest segment count a lane takes times the piece, plus the segments a row sums).
struct MelNnlsBands {
  std::vector<double> wr, wc;
  std::vector<int> seg;      // 4 ints per segment
  std::vector<int> rowseg;   // n_mels + 1
  std::vector<int> col;      // 2 ints per bin
  int nseg = 0, piece = 0;
};

inline void mel_nnls_build(const std::vector<double>& M, int n_mels, int F, MelNnlsBands& bd) {
  std::vector<int> lo(n_mels, 0), len(n_mels, 0);
  int longest = 1;
  for (int m = 0; m < n_mels; ++m) {
    int a = -1, e = -1;
    for (int f = 0; f < F; ++f)
      if (M[(size_t)m * F + f] != 0.0) {
        if (a < 0) a = f;
        e = f;
      }
    if (a >= 0) {
      lo[m] = a;
      len[m] = e - a + 1;
      longest = std::max(longest, len[m]);
    }
  }
  // piece: least estimated cost of M z and the row sums for a wave of 64 lanes
  long long best = -1;
  for (int P = 1; P <= longest; ++P) {
    long long nseg = 0, most = 0;
    for (int m = 0; m < n_mels; ++m) {
      const long long c = (len[m] + P - 1) / P;
      nseg += c;
      most = std::max(most, c);
    }
    const long long cost = (nseg + 63) / 64 * (P + 4) + (n_mels + 63) / 64 * most;
    if (best < 0 || cost < best) {
      best = cost;
      bd.piece = P;
    }
  }
  const int P = bd.piece;
  bd.wr.clear();
  bd.seg.clear();
  bd.rowseg.assign(n_mels + 1, 0);
  for (int m = 0; m < n_mels; ++m) {
    bd.rowseg[m] = (int)(bd.seg.size() / 4);
    for (int f0 = lo[m]; f0 < lo[m] + len[m]; f0 += P) {
      const int n = std::min(P, lo[m] + len[m] - f0);
      bd.seg.insert(bd.seg.end(), {f0, n, (int)bd.wr.size(), 0});
      for (int i = 0; i < n; ++i) bd.wr.push_back(M[(size_t)m * F + f0 + i]);
    }
  }
  bd.nseg = (int)(bd.seg.size() / 4);
  bd.rowseg[n_mels] = bd.nseg;
  bd.wc.clear();
  bd.col.assign((size_t)2 * F, 0);
  for (int f = 0; f < F; ++f) {
    int a = -1, e = -1;
    for (int m = 0; m < n_mels; ++m)
      if (M[(size_t)m * F + f] != 0.0) {
        if (a < 0) a = m;
        e = m;
      }
    const int n = a >= 0 ? e - a + 1 : 0;
    bd.col[2 * f] = (a >= 0 ? a : 0) | (n << 16);
    bd.col[2 * f + 1] = (int)bd.wc.size();
    for (int j = 0; j < n; ++j) bd.wc.push_back(M[(size_t)(a + j) * F + f]);
  }
}

}  // namespace fast

// libspecinv's side of specinv_mel_nnls_setup / specinv_mel_nnls (tu_mel_nnls.hip); the state hangs off the plan (plan.h)
int mel_nnls_setup(PlanBase& pl, const void* mel_fb, int n_mels, double lipschitz);
int mel_nnls_run(PlanBase& pl, const void* mel, int n_iter, double power, void* mag_out);

}  // namespace specinv
