// Weighted prediction error dereverberation (Nakatani et al. 2010, the offline form): per item and bin, a linear
// filter over the frames at least `delay` back, fitted by least squares weighted with the reciprocal of the result's own power,
// re-estimated n_iter times.  One launch for all iterations; one workgroup owns an (item, bin) and the grid is looped.
//   X is (B, C, F, T); per (item, f), with D = C K, x_t = X[:, f, t] and the stacked past xs_t, entry (c', k) at row c' K + k =
//   X[c', f, t - delay - k] (zero before the first frame):
//     q_t    = mean_c |Y[c, f, t]|^2          Y the previous iteration's result, X itself in the first - or power[f, t] there
//     p_t    = the mean of q over the frames t - ctx ... t + ctx that exist
//     lam_t  = max(p_t, eps max_t p_t, tiny)                                     tiny = the smallest normal double
//     R      = sum_t xs_t xs_t^H / lam_t ,  P = sum_t xs_t x_t^H / lam_t ,  R += (diag_load tr(R) / D + tiny) I
//     G      = R^-1 P  (D x C) ,  Y[:, f, t] = x_t - G^H xs_t
//   Everything is float64 for complex64 input as well; Y is rounded once, when the last pass stores it.
//
// The passes of an iteration, each a walk over tiles of `tile` frames (kWpeTile; kWpeTileWide beyond kWpeWideChannels channels,
// where the staged rows would not fit beside R and P):
//   Stage.   X[c, f, tile] goes to LDS as complex double twice: the `past` window, frames tb - delay - (K - 1) ... tb - delay +
//            tile - 1 (tile + K - 1 of them: the K lags of every frame of the tile, whatever the delay, so LDS does not grow with
//            it), and the `now` window, the tile itself.  Loads run along T.
//   Power.   The first iteration reads q from X or `power`.  A later one recomputes Y = x - G^H xs in float64 from the G in LDS
//            instead of reading a rounded Y back, so that a complex64 call takes the same lam as the float64 definition.  q goes
//            to `lam` (to `qbuf` when ctx > 0), global arrays this workgroup alone reads back after a workgroup barrier; then the
//            context mean, the maximum over all frames and the floor.
//   Sums.    The lower triangle of R and all of P are cut into 4 x 4 blocks of entries; a thread owns up to NB blocks and keeps
//            them in registers over the whole walk (32 doubles a block).  With fewer than 129 blocks the threads split into
//            nsl = 2, 4 or 8 slices that take every nsl-th frame of a tile, and the slices are summed through LDS in slice order
//            at the end.  The mapping depends on C and K alone: item b of a batch and the same item alone give the same bits.
//   Solve.   R = U D U^H in place on the packed triangle (the square-root-free Cholesky; pivots floored at tiny), U y = P,
//            z = D^-1 y, U^H G = z, one workgroup barrier a column; G replaces P.
//   Filter.  The walk once more: Y = x - G^H xs, a thread per (channel, frame), the d sum in row order with explicit fma: the
//            same instructions whether G was just solved or handed in (specinv_wpe's filter-only mode), hence the same bits.
// LDS (doubles): R 2 tri(D) | P / G 2 D C | 1 / pivot D || past 2 C (tile + K - 1) | now 2 C tile | 1 / lam tile | |y|^2 C tile | 8;
// the slices' partial sums (nsl nblocks 32) overlay the part after ||.  At most 140 KB (C 64, K 1); 19 KB at C 1, K 10.
// No atomics, no communication between workgroups.  All global offsets are 64-bit.
#pragma once
#include "common.h"

namespace specinv {

constexpr int kWpeThreads = 256;
constexpr int kWpeTile = 32;            // frames a tile holds (dereverb.py: TILE_FRAMES)
constexpr int kWpeTileWide = 16;        // ... with more than kWpeWideChannels channels
constexpr int kWpeWideChannels = 32;
constexpr int kWpeMaxD = 64;            // C K, the unknowns a channel's filter has
constexpr int kWpeMaxContext = 64;      // psd_context: the context mean is 2 ctx + 1 reads a frame (dereverb.py: MAX_CONTEXT)
constexpr int kWpeMaxIter = 100;        // n_iter: the launch's length is bounded (dereverb.py: MAX_ITER)
constexpr int kWpeBlk = 4;             // a register block is kWpeBlk x kWpeBlk entries
#ifndef SPECINV_WPE_SLICES
#define SPECINV_WPE_SLICES 8            // the most slices the frames of a tile are dealt to (measured, tools/log/EXPERIMENTS.md)
#endif
constexpr int kWpeMaxSlices = SPECINV_WPE_SLICES;
constexpr int kWpeMaxGrid = 8192;       // workgroups of a launch; the problems beyond are looped over
constexpr double kWpeTiny = 2.2250738585072014e-308;
static_assert(kWpeMaxSlices == 1 || kWpeMaxSlices == 2 || kWpeMaxSlices == 4 || kWpeMaxSlices == 8, "slices are a power of two");

struct WpeArgs {
  const void* spec;        // (B, C, F, T) cplx<T>
  const double* power;     // (B, F, T) or nullptr
  const void* filt_in;     // (B, F, D, C) complex double or nullptr; given: the filter-only mode
  void* out;               // (B, C, F, T) cplx<T>
  void* filt_out;          // (B, F, D, C) complex double or nullptr
  double* lam;             // (B, F, T); nullptr in the filter-only mode
  double* qbuf;            // (B, F, T) when ctx > 0
  int64_t batch, n_freq, n_frames;
  int64_t delay, ctx;
  int channels, taps, n_iter;
  double eps, diag_load;
};

// what C and K fix: the blocks, the slices and the LDS layout (offsets in doubles)
struct WpeGeom {
  int D, tile, W, nrb, npb, ntri, nblocks, nsl, nbt;
  int oP, oInv, oPast, oNow, oW, oQ, oRed, oPart, total;
};

__host__ __device__ inline WpeGeom wpe_geom(int C, int K) {
  WpeGeom g;
  g.D = C * K;
  g.tile = C > kWpeWideChannels ? kWpeTileWide : kWpeTile;
  g.W = g.tile + K - 1;
  g.nrb = (g.D + kWpeBlk - 1) / kWpeBlk;
  g.npb = (C + kWpeBlk - 1) / kWpeBlk;
  g.ntri = g.nrb * (g.nrb + 1) / 2;
  g.nblocks = g.ntri + g.nrb * g.npb;
  g.nsl = 1;
  while (g.nsl < kWpeMaxSlices && g.nblocks * g.nsl * 2 <= kWpeThreads) g.nsl *= 2;
  g.nbt = kWpeThreads / g.nsl;
  g.oP = g.D * (g.D + 1);
  g.oInv = g.oP + 2 * g.D * C;
  g.oPast = (g.oInv + g.D + 1) & ~1;
  g.oNow = g.oPast + 2 * C * g.W;
  g.oW = g.oNow + 2 * C * g.tile;
  g.oQ = g.oW + g.tile;
  g.oRed = g.oQ + C * g.tile;
  g.oPart = g.oPast;
  const int end_walk = g.oRed + 8;
  const int end_part = g.nsl > 1 ? g.oPart + g.nsl * g.nblocks * 2 * kWpeBlk * kWpeBlk : 0;
  g.total = end_walk > end_part ? end_walk : end_part;
  return g;
}

// block `blk` of the list: rows 4 rb ..., and columns 4 cb ... of R (is_p false: cb <= rb) or of P
__device__ __forceinline__ void wpe_block(const WpeGeom& g, int blk, int& rb, int& cb, bool& is_p) {
  if (blk < g.ntri) {
    rb = 0;
    while ((rb + 1) * (rb + 2) / 2 <= blk) ++rb;
    cb = blk - rb * (rb + 1) / 2;
    is_p = false;
  } else {
    const int pb = blk - g.ntri;
    rb = pb / g.npb;
    cb = pb - rb * g.npb;
    is_p = true;
  }
}

__device__ __forceinline__ double wpe_wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}

// the two windows of the tile at frame tb; x is the (item, bin)'s row of channel 0, channels `cs` elements apart
template <typename T>
__device__ __forceinline__ void wpe_stage(const WpeArgs& a, const WpeGeom& g, double* lds, const cplx<T>* x, int64_t cs, int64_t tb) {
  cplx<double>* const past = (cplx<double>*)(lds + g.oPast);
  cplx<double>* const now = (cplx<double>*)(lds + g.oNow);
  const int64_t nT = a.n_frames;
  const int64_t t0 = tb - a.delay - (a.taps - 1);
  const int n_past = a.channels * g.W, n_now = a.channels * g.tile;
  for (int idx = threadIdx.x; idx < n_past; idx += kWpeThreads) {
    const int c = idx / g.W, u = idx - c * g.W;
    const int64_t t = t0 + u;
    cplx<double> v = mk<double>(0.0, 0.0);
    if (t >= 0 && t < nT) {
      const cplx<T> e = x[c * cs + t];
      v = mk<double>((double)e.x, (double)e.y);
    }
    past[idx] = v;
  }
  for (int idx = threadIdx.x; idx < n_now; idx += kWpeThreads) {
    const int c = idx / g.tile, u = idx - c * g.tile;
    const int64_t t = tb + u;
    cplx<double> v = mk<double>(0.0, 0.0);
    if (t < nT) {
      const cplx<T> e = x[c * cs + t];
      v = mk<double>((double)e.x, (double)e.y);
    }
    now[idx] = v;
  }
}

// Y[c, tb + tl] = x - G^H xs from the staged windows
__device__ __forceinline__ cplx<double> wpe_filtered(const WpeArgs& a, const WpeGeom& g, const double* lds, int c, int tl) {
#pragma clang fp contract(off)
  const cplx<double>* const sG = (const cplx<double>*)(lds + g.oP);
  const cplx<double>* const past = (const cplx<double>*)(lds + g.oPast);
  const cplx<double>* const now = (const cplx<double>*)(lds + g.oNow);
  const int C = a.channels, K = a.taps;
  double re = 0.0, im = 0.0;
  for (int cp = 0; cp < C; ++cp) {
    const cplx<double>* const row = past + cp * g.W + tl + (K - 1);
    const cplx<double>* const gp = sG + (cp * K) * C + c;
    for (int k = 0; k < K; ++k) {
      const cplx<double> xs = row[-k], gg = gp[k * C];
      re = fma(gg.x, xs.x, re);
      re = fma(gg.y, xs.y, re);
      im = fma(gg.x, xs.y, im);
      im = fma(-gg.y, xs.x, im);
    }
  }
  const cplx<double> x = now[c * g.tile + tl];
  return mk<double>(x.x - re, x.y - im);
}

// lam for every frame of the (item, bin); `first`: from X or `power`, else from the filter in LDS
template <typename T>
__device__ __forceinline__ void wpe_lambda(const WpeArgs& a, const WpeGeom& g, double* lds, const cplx<T>* x, int64_t cs, int64_t prob,
                                           bool first) {
#pragma clang fp contract(off)
  const int64_t nT = a.n_frames;
  const int C = a.channels, tid = threadIdx.x;
  double* const lam = a.lam + prob * nT;
  double* const q = a.ctx > 0 ? a.qbuf + prob * nT : lam;
  if (first) {
    for (int64_t t = tid; t < nT; t += kWpeThreads) {
      double s = 0.0;
      if (a.power != nullptr) {
        s = a.power[prob * nT + t];
      } else {
        for (int c = 0; c < C; ++c) {
          const cplx<T> e = x[c * cs + t];
          const double re = (double)e.x, im = (double)e.y;
          s = s + (re * re + im * im);
        }
        s = s / (double)C;
      }
      q[t] = s;
    }
  } else {
    double* const ysq = lds + g.oQ;
    for (int64_t tb = 0; tb < nT; tb += g.tile) {
      wpe_stage<T>(a, g, lds, x, cs, tb);
      __syncthreads();
      for (int idx = tid; idx < C * g.tile; idx += kWpeThreads) {
        const int c = idx / g.tile, tl = idx - c * g.tile;
        double v = 0.0;
        if (tb + tl < nT) {
          const cplx<double> y = wpe_filtered(a, g, lds, c, tl);
          v = y.x * y.x + y.y * y.y;
        }
        ysq[idx] = v;
      }
      __syncthreads();
      if (tid < g.tile && tb + tid < nT) {
        double s = 0.0;
        for (int c = 0; c < C; ++c) s = s + ysq[c * g.tile + tid];
        q[tb + tid] = s / (double)C;
      }
    }
  }
  __syncthreads();      // q was written by other threads of this workgroup
  double m = 0.0;
  for (int64_t t = tid; t < nT; t += kWpeThreads) {
    double p;
    if (a.ctx > 0) {
      const int64_t lo = t - a.ctx > 0 ? t - a.ctx : 0, hi = t + a.ctx < nT - 1 ? t + a.ctx : nT - 1;
      double s = 0.0;
      for (int64_t u = lo; u <= hi; ++u) s = s + q[u];
      p = s / (double)(hi - lo + 1);
      lam[t] = p;
    } else {
      p = q[t];
    }
    m = fmax(m, p);
  }
  double* const red = lds + g.oRed;
  m = wpe_wave_max(m);
  if ((tid & 63) == 0) red[tid >> 6] = m;
  __syncthreads();
  const double pmax = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  const double floor_ = fmax(a.eps * pmax, kWpeTiny);
  for (int64_t t = tid; t < nT; t += kWpeThreads) lam[t] = fmax(lam[t], floor_);   // (the thread's own frames)
  __syncthreads();
}

// R (packed lower triangle) and P from the walk over all frames, weighted by 1 / lam
template <typename T, int NB>
__device__ __forceinline__ void wpe_accumulate(const WpeArgs& a, const WpeGeom& g, double* lds, const cplx<T>* x, int64_t cs,
                                               int64_t prob) {
  const int64_t nT = a.n_frames;
  const int C = a.channels, K = a.taps, D = g.D, tid = threadIdx.x;
  const int slice = tid / g.nbt, e = tid - slice * g.nbt;
  const cplx<double>* const win = (const cplx<double>*)(lds + g.oPast);     // past, then now: one base for both
  double* const winv = lds + g.oW;
  const double* const lam = a.lam + prob * nT;
  double ar[NB][kWpeBlk][kWpeBlk], ai[NB][kWpeBlk][kWpeBlk];
  int off_a[NB][kWpeBlk], off_b[NB][kWpeBlk], rbs[NB], cbs[NB];
  bool has[NB], isp[NB];
#pragma unroll
  for (int n = 0; n < NB; ++n) {
    const int blk = e + n * g.nbt;
    has[n] = slice < g.nsl && blk < g.nblocks;
    rbs[n] = cbs[n] = 0;
    isp[n] = false;
    if (has[n]) wpe_block(g, blk, rbs[n], cbs[n], isp[n]);
#pragma unroll
    for (int r = 0; r < kWpeBlk; ++r) {
      int i = kWpeBlk * rbs[n] + r;
      i = i < D ? i : D - 1;                         // (a row or column beyond the matrix: computed on the last one, never stored)
      off_a[n][r] = (i / K) * g.W + (K - 1) - (i % K);
      int j = kWpeBlk * cbs[n] + r;
      if (isp[n]) {
        j = j < C ? j : C - 1;
        off_b[n][r] = C * g.W + j * g.tile;
      } else {
        j = j < D ? j : D - 1;
        off_b[n][r] = (j / K) * g.W + (K - 1) - (j % K);
      }
#pragma unroll
      for (int s = 0; s < kWpeBlk; ++s) ar[n][r][s] = ai[n][r][s] = 0.0;
    }
  }
  for (int64_t tb = 0; tb < nT; tb += g.tile) {
    __syncthreads();                                 // the previous tile's reads are over
    wpe_stage<T>(a, g, lds, x, cs, tb);
    if (tid < g.tile) winv[tid] = tb + tid < nT ? 1.0 / lam[tb + tid] : 0.0;
    __syncthreads();
    const int len = nT - tb < g.tile ? (int)(nT - tb) : g.tile;
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      if (!has[n]) continue;
      for (int tl = slice; tl < len; tl += g.nsl) {
        const double w = winv[tl];
        cplx<double> u[kWpeBlk], v[kWpeBlk];
#pragma unroll
        for (int r = 0; r < kWpeBlk; ++r) {
          const cplx<double> xa = win[off_a[n][r] + tl];
          u[r] = mk<double>(xa.x * w, xa.y * w);
          v[r] = win[off_b[n][r] + tl];
        }
#pragma unroll
        for (int r = 0; r < kWpeBlk; ++r)
#pragma unroll
          for (int s = 0; s < kWpeBlk; ++s) {       // u conj(v)
            ar[n][r][s] = fma(u[r].x, v[s].x, ar[n][r][s]);
            ar[n][r][s] = fma(u[r].y, v[s].y, ar[n][r][s]);
            ai[n][r][s] = fma(u[r].y, v[s].x, ai[n][r][s]);
            ai[n][r][s] = fma(-u[r].x, v[s].y, ai[n][r][s]);
          }
      }
    }
  }
  __syncthreads();                                   // the windows are dead: the partial sums may overlay them
  cplx<double>* const sR = (cplx<double>*)lds;
  cplx<double>* const sP = (cplx<double>*)(lds + g.oP);
  constexpr int kEnt = kWpeBlk * kWpeBlk;
  if (g.nsl == 1) {
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      if (!has[n]) continue;
#pragma unroll
      for (int r = 0; r < kWpeBlk; ++r)
#pragma unroll
        for (int s = 0; s < kWpeBlk; ++s) {
          const int i = kWpeBlk * rbs[n] + r, j = kWpeBlk * cbs[n] + s;
          if (i >= D) continue;
          if (isp[n]) {
            if (j < C) sP[i * C + j] = mk<double>(ar[n][r][s], ai[n][r][s]);
          } else if (j <= i) {
            sR[i * (i + 1) / 2 + j] = mk<double>(ar[n][r][s], ai[n][r][s]);
          }
        }
    }
  } else {
    cplx<double>* const part = (cplx<double>*)(lds + g.oPart);
    if (has[0]) {                                    // (with slices a thread owns one block)
#pragma unroll
      for (int r = 0; r < kWpeBlk; ++r)
#pragma unroll
        for (int s = 0; s < kWpeBlk; ++s) part[(slice * g.nblocks + e) * kEnt + r * kWpeBlk + s] = mk<double>(ar[0][r][s], ai[0][r][s]);
    }
    __syncthreads();
    for (int idx = tid; idx < g.nblocks * kEnt; idx += kWpeThreads) {
      const int blk = idx / kEnt, rs = idx - blk * kEnt, r = rs / kWpeBlk, s = rs - r * kWpeBlk;
      int rb, cb;
      bool is_p;
      wpe_block(g, blk, rb, cb, is_p);
      const int i = kWpeBlk * rb + r, j = kWpeBlk * cb + s;
      if (i >= D || (is_p ? j >= C : j > i)) continue;
      double sr = 0.0, si = 0.0;
      for (int sl = 0; sl < g.nsl; ++sl) {
        const cplx<double> p = part[(sl * g.nblocks + blk) * kEnt + rs];
        sr += p.x;
        si += p.y;
      }
      if (is_p)
        sP[i * C + j] = mk<double>(sr, si);
      else
        sR[i * (i + 1) / 2 + j] = mk<double>(sr, si);
    }
  }
  __syncthreads();
}

// G = (R + load I)^-1 P in LDS; G replaces P
__device__ __forceinline__ void wpe_solve(const WpeArgs& a, const WpeGeom& g, double* lds) {
#pragma clang fp contract(off)
  const int C = a.channels, D = g.D, tid = threadIdx.x;
  cplx<double>* const sR = (cplx<double>*)lds;
  cplx<double>* const sP = (cplx<double>*)(lds + g.oP);
  double* const invd = lds + g.oInv;
  double* const red = lds + g.oRed;
  if (tid < 64) {
    double tr = 0.0;
    for (int i = tid; i < D; i += 64) tr += sR[i * (i + 1) / 2 + i].x;
    tr = wave_sum(tr);
    if (tid == 0) red[4] = tr;
  }
  __syncthreads();
  const double load = a.diag_load * red[4] / (double)D + kWpeTiny;
  if (tid < D) sR[tid * (tid + 1) / 2 + tid] = mk<double>(sR[tid * (tid + 1) / 2 + tid].x + load, 0.0);
  __syncthreads();
  // R = U D U^H: column j keeps M[i][j] = U[i][j] D[j], the diagonal D[j]
  for (int j = 0; j < D; ++j) {
    const double inv = 1.0 / fmax(sR[j * (j + 1) / 2 + j].x, kWpeTiny);
    if (tid == 0) invd[j] = inv;
    for (int i = j + 1 + (tid >> 4); i < D; i += kWpeThreads / 16) {
      const cplx<double> m = sR[i * (i + 1) / 2 + j];
      const double lx = m.x * inv, ly = m.y * inv;
      for (int k = j + 1 + (tid & 15); k <= i; k += 16) {
        const cplx<double> mk_ = sR[k * (k + 1) / 2 + j];
        cplx<double> r = sR[i * (i + 1) / 2 + k];
        r.x = fma(-lx, mk_.x, r.x);
        r.x = fma(-ly, mk_.y, r.x);
        r.y = fma(-ly, mk_.x, r.y);
        r.y = fma(lx, mk_.y, r.y);
        sR[i * (i + 1) / 2 + k] = r;
      }
    }
    __syncthreads();
  }
  // U y = P
  for (int j = 0; j + 1 < D; ++j) {
    const double inv = invd[j];
    for (int idx = tid; idx < (D - 1 - j) * C; idx += kWpeThreads) {
      const int i = j + 1 + idx / C, c = idx % C;
      const cplx<double> m = sR[i * (i + 1) / 2 + j], y = sP[j * C + c];
      const double ux = m.x * inv, uy = m.y * inv;
      cplx<double> p = sP[i * C + c];
      p.x = fma(-ux, y.x, p.x);
      p.x = fma(uy, y.y, p.x);
      p.y = fma(-ux, y.y, p.y);
      p.y = fma(-uy, y.x, p.y);
      sP[i * C + c] = p;
    }
    __syncthreads();
  }
  // z = D^-1 y
  for (int idx = tid; idx < D * C; idx += kWpeThreads) {
    const double inv = invd[idx / C];
    const cplx<double> p = sP[idx];
    sP[idx] = mk<double>(p.x * inv, p.y * inv);
  }
  __syncthreads();
  // U^H G = z
  for (int i = D - 1; i >= 1; --i) {
    for (int idx = tid; idx < i * C; idx += kWpeThreads) {
      const int j = idx / C, c = idx % C;
      const cplx<double> m = sR[i * (i + 1) / 2 + j], gi = sP[i * C + c];
      const double inv = invd[j];
      const double ux = m.x * inv, uy = m.y * inv;      // conj(u) gi
      cplx<double> p = sP[j * C + c];
      p.x = fma(-ux, gi.x, p.x);
      p.x = fma(-uy, gi.y, p.x);
      p.y = fma(-ux, gi.y, p.y);
      p.y = fma(uy, gi.x, p.y);
      sP[j * C + c] = p;
    }
    __syncthreads();
  }
}

template <typename T, int NB>
__global__ __launch_bounds__(kWpeThreads) void k_wpe(const WpeArgs a) {
  extern __shared__ __attribute__((aligned(16))) double wpe_lds[];
  double* const lds = wpe_lds;
  const WpeGeom g = wpe_geom(a.channels, a.taps);
  const int64_t nT = a.n_frames, F = a.n_freq;
  const int C = a.channels, tid = threadIdx.x;
  const int64_t cs = F * nT;
  cplx<double>* const sG = (cplx<double>*)(lds + g.oP);
  for (int64_t prob = blockIdx.x; prob < a.batch * F; prob += gridDim.x) {
    const int64_t item = prob / F, f = prob - item * F;
    const int64_t base = (item * C * F + f) * nT;
    const cplx<T>* const x = (const cplx<T>*)a.spec + base;
    if (a.filt_in != nullptr) {
      const cplx<double>* const gin = (const cplx<double>*)a.filt_in + prob * g.D * C;
      for (int idx = tid; idx < g.D * C; idx += kWpeThreads) sG[idx] = gin[idx];
    } else {
      if (a.n_iter == 0) {
        for (int idx = tid; idx < g.D * C; idx += kWpeThreads) sG[idx] = mk<double>(0.0, 0.0);
        wpe_lambda<T>(a, g, lds, x, cs, prob, true);
      }
      for (int it = 0; it < a.n_iter; ++it) {
        wpe_lambda<T>(a, g, lds, x, cs, prob, it == 0);
        wpe_accumulate<T, NB>(a, g, lds, x, cs, prob);
        wpe_solve(a, g, lds);
      }
      if (a.filt_out != nullptr) {
        cplx<double>* const gout = (cplx<double>*)a.filt_out + prob * g.D * C;
        for (int idx = tid; idx < g.D * C; idx += kWpeThreads) gout[idx] = sG[idx];
      }
    }
    cplx<T>* const y = (cplx<T>*)a.out + base;
    for (int64_t tb = 0; tb < nT; tb += g.tile) {
      __syncthreads();                               // G is in place; the previous tile's reads are over
      wpe_stage<T>(a, g, lds, x, cs, tb);
      __syncthreads();
      for (int idx = tid; idx < C * g.tile; idx += kWpeThreads) {
        const int c = idx / g.tile, tl = idx - c * g.tile;
        if (tb + tl < nT) {
          const cplx<double> v = wpe_filtered(a, g, lds, c, tl);
          y[c * cs + tb + tl] = mk<T>((T)v.x, (T)v.y);
        }
      }
    }
    __syncthreads();                                 // before the next problem's writes to LDS
  }
}

}  // namespace specinv
