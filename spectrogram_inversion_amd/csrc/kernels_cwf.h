// Consistent Wiener filtering (Le Roux & Vincent 2013; not in the reference): the element-wise kernels of a
// preconditioned conjugate-gradient loop on  A S = X / v_n ,  A P = Lam P + g (u - G' u),  u = P - G P,  whose four transforms per
// iteration are the plan's own (specinv_istft, specinv_stft, specinv_stft_adjoint, specinv_istft_adjoint).  The definition is
// include/specinv.h's (specinv_cwf_run).
//
// Layout: every array is (batch, n_freq, n_frames) as specinv_stft writes it, complex ones interleaved (re, im); an item is ft =
// n_freq * n_frames bins.  Launch: grid (nblk, batch), 256 lanes; a lane takes groups of four consecutive bins of its item - 32
// bytes of a complex float32 array, 64 of a float64 one, as 16-byte loads and stores - at a stride of nblk * 256 groups, and lane 0
// of workgroup 0 takes the item's last ft % 4 bins.  The groups are cut by the index within the item, never by the address: an
// item's sums are added in one order wherever it sits in a batch, and an item that starts off a 16-byte boundary (ft % 4 != 0)
// takes the same groups with element loads.
//
// Sums: all float64.  A workgroup adds its lanes' sums (the wave's exchange ladder, then the four waves in order) and stores one
// partial per (item, workgroup); every workgroup of the NEXT launch adds the item's nblk <= 256 partials the same way, one per lane.
// The kernel boundary is the only synchronisation: no atomics, no flags, and every workgroup of an item arrives at the same bits.
// The partial sets (cwf_part) and the item's scalars (cwf_scal) are laid out below.
#pragma once
#include <type_traits>

#include "common.h"

// No contraction of a * b + c below: the aligned and the unaligned form of a loop must round alike, whatever the compiler would
// choose for each (an item's bits do not depend on its place in a batch).
#pragma clang fp contract(off)

namespace specinv {

constexpr int kCwfThreads = 256;
constexpr int kCwfGroup = 4;          // bins per lane and step
constexpr int kCwfMaxBlocks = 256;    // workgroups per item = partials per set and item: one per lane of the workgroup that adds them

// partial sets, (batch, nblk) doubles each
enum { kCwfPartMax = 0, kCwfPartMean, kCwfPartPq, kCwfPartRz0, kCwfPartRzA, kCwfPartRzB, kCwfPartSets };
// an item's scalars: m, g, and whether it is finished as of an even / odd iteration count (written by one launch, read by the next)
enum { kCwfScalM = 0, kCwfScalG, kCwfScalFin0, kCwfScalFin1, kCwfScalStride };

// which partial set holds <r, z> after `k` iterations
__host__ __device__ inline int cwf_rz_set(int k) { return k == 0 ? kCwfPartRz0 : (k & 1) ? kCwfPartRzB : kCwfPartRzA; }

inline int cwf_blocks(int64_t ft) {
  const int64_t want = ceil_div(ft / kCwfGroup, kCwfThreads);
  return (int)(want < 1 ? 1 : want > kCwfMaxBlocks ? kCwfMaxBlocks : want);
}

template <typename T>
struct CwfArgs {
  const T* mix;      // X
  const T* vs;       // v_s, v_n as given
  const T* vn;
  T* S;              // the iterate (S_out)
  T* R;              // r
  T* P;              // p
  T* U;              // u = p - G p
  T* Q;              // G p, then G' u, then q (N_out until the end)
  T* lam;            // Lam, real
  double* part;
  double* scal;
  int64_t ft;
  int nblk, batch;
  double gamma, floor, shrink;   // shrink = 1 - hop / n_fft
  int relative;
};

template <typename T>
struct CwfVec;
template <>
struct CwfVec<float> {
  using type = float4;
};
template <>
struct CwfVec<double> {
  using type = double2;
};

// N values of T from / to p: 16-byte accesses where VEC (p is then 16-byte aligned and N * sizeof(T) a multiple of 16)
template <typename T, int N, bool VEC>
__device__ __forceinline__ void cwf_load(const T* p, T (&v)[N]) {
  constexpr int W = 16 / (int)sizeof(T);
  using V = typename CwfVec<T>::type;
  if constexpr (VEC) {
#pragma unroll
    for (int i = 0; i < N / W; ++i) {
      const V t = reinterpret_cast<const V*>(p)[i];
      v[W * i] = t.x;
      v[W * i + 1] = t.y;
      if constexpr (W == 4) {
        v[W * i + 2] = t.z;
        v[W * i + 3] = t.w;
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = p[i];
  }
}
template <typename T, int N, bool VEC>
__device__ __forceinline__ void cwf_store(T* p, const T (&v)[N]) {
  constexpr int W = 16 / (int)sizeof(T);
  using V = typename CwfVec<T>::type;
  if constexpr (VEC) {
#pragma unroll
    for (int i = 0; i < N / W; ++i) {
      V t;
      t.x = v[W * i];
      t.y = v[W * i + 1];
      if constexpr (W == 4) {
        t.z = v[W * i + 2];
        t.w = v[W * i + 3];
      }
      reinterpret_cast<V*>(p)[i] = t;
    }
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) p[i] = v[i];
  }
}

// The workgroup's sum (MAX: maximum) in a fixed order, in every lane.  The exchange ladder leaves the same bits in all 64 lanes
// (each step adds the same two numbers on both sides), the four waves are then added in order.
template <bool MAX>
__device__ inline double cwf_block_reduce(double v, double* lds4) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double o = __shfl_xor(v, off, 64);
    v = MAX ? fmax(v, o) : v + o;
  }
  __syncthreads();                    // (lds4 may still be read from the call before)
  if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = lds4[0];
#pragma unroll
  for (int w = 1; w < kCwfThreads / 64; ++w) r = MAX ? fmax(r, lds4[w]) : r + lds4[w];
  return r;
}

// finish what the launch before left: the item's nblk partials of `set`, one per lane
template <bool MAX = false>
__device__ inline double cwf_finish(const double* part, int set, int batch, int nblk, double* lds4) {
  const double* p = part + ((size_t)set * batch + blockIdx.y) * nblk;
  return cwf_block_reduce<MAX>((int)threadIdx.x < nblk ? p[threadIdx.x] : 0.0, lds4);
}
__device__ inline void cwf_put(double* part, int set, int batch, int nblk, double v) {
  if (threadIdx.x == 0) part[((size_t)set * batch + blockIdx.y) * nblk + blockIdx.x] = v;
}

using cwf_four = std::integral_constant<int, kCwfGroup>;
using cwf_one = std::integral_constant<int, 1>;

// body(e, count, vec): the bins [e, e + count) of item blockIdx.y, e counted within the item, with 16-byte accesses where vec.
// The aligned and the unaligned item have a loop each: as one loop with a branch around every access the compiler merges the two
// forms of a store into the element form.
template <typename Body>
__device__ __forceinline__ void cwf_for_bins(int64_t ft, bool aligned, Body&& body) {
  const int64_t ng = ft / kCwfGroup;
  const int64_t j0 = (int64_t)blockIdx.x * kCwfThreads + threadIdx.x, dj = (int64_t)gridDim.x * kCwfThreads;
  if (aligned)
    for (int64_t j = j0; j < ng; j += dj) body(j * kCwfGroup, cwf_four{}, std::true_type{});
  else
    for (int64_t j = j0; j < ng; j += dj) body(j * kCwfGroup, cwf_four{}, std::false_type{});
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int64_t e = ng * kCwfGroup; e < ft; ++e) body(e, cwf_one{}, std::false_type{});
}

// whether item b's groups sit on 16-byte boundaries (the arrays' bases do: the host checks)
__device__ __forceinline__ bool cwf_item_aligned(int64_t ft) { return ((int64_t)blockIdx.y * ft) % kCwfGroup == 0; }

// ---- setup 1: the partial maxima of v_s + v_n -----------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kCwfThreads) void k_cwf_max(CwfArgs<T> a) {
  __shared__ double lds4[kCwfThreads / 64];
  const int64_t base = (int64_t)blockIdx.y * a.ft;
  const bool al = cwf_item_aligned(a.ft);
  double m = 0.0;
  cwf_for_bins(a.ft, al, [&](int64_t e, auto cnt, auto vec) {
    constexpr int NB = decltype(cnt)::value;
    constexpr bool V = decltype(vec)::value;
    T vs[NB], vn[NB];
    cwf_load<T, NB, V>(a.vs + base + e, vs);
    cwf_load<T, NB, V>(a.vn + base + e, vn);
#pragma unroll
    for (int k = 0; k < NB; ++k) m = fmax(m, (double)vs[k] + (double)vn[k]);
  });
  m = cwf_block_reduce<true>(m, lds4);
  cwf_put(a.part, kCwfPartMax, a.batch, a.nblk, m);
}

// ---- setup 2: m, the floored variances, Lam, S_0 = v_s / (v_s + v_n) X, the right-hand side X / v_n (into R) and the partial sums
// of v_s v_n / (v_s + v_n).  An item with m = 0 (not > 0) is dead: S = R = Lam = 0, and it is finished from the start. -------------
template <typename T>
__global__ __launch_bounds__(kCwfThreads) void k_cwf_init(CwfArgs<T> a) {
  __shared__ double lds4[kCwfThreads / 64];
  const int64_t base = (int64_t)blockIdx.y * a.ft;
  const bool al = cwf_item_aligned(a.ft);
  const double m = a.floor * cwf_finish<true>(a.part, kCwfPartMax, a.batch, a.nblk, lds4);
  const bool live = m > 0.0;
  const T mt = (T)m;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double* sc = a.scal + (size_t)blockIdx.y * kCwfScalStride;
    sc[kCwfScalM] = live ? m : 0.0;
    sc[kCwfScalFin0] = live ? 0.0 : 1.0;
  }
  double sum = 0.0;
  cwf_for_bins(a.ft, al, [&](int64_t e, auto cnt, auto vec) {
    constexpr int NB = decltype(cnt)::value;
    constexpr bool V = decltype(vec)::value;
    T vs[NB], vn[NB], x[2 * NB], s[2 * NB], b[2 * NB], lam[NB];
    cwf_load<T, NB, V>(a.vs + base + e, vs);
    cwf_load<T, NB, V>(a.vn + base + e, vn);
    cwf_load<T, 2 * NB, V>(a.mix + 2 * (base + e), x);
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      if (live) {
        const T ps = vs[k] > mt ? vs[k] : mt, pn = vn[k] > mt ? vn[k] : mt;
        lam[k] = T(1) / ps + T(1) / pn;
        const T gain = ps / (ps + pn);
        s[2 * k] = gain * x[2 * k];
        s[2 * k + 1] = gain * x[2 * k + 1];
        b[2 * k] = x[2 * k] / pn;
        b[2 * k + 1] = x[2 * k + 1] / pn;
        sum += (double)ps * (double)pn / ((double)ps + (double)pn);
      } else {
        lam[k] = T(0);
        s[2 * k] = s[2 * k + 1] = b[2 * k] = b[2 * k + 1] = T(0);
      }
    }
    cwf_store<T, NB, V>(a.lam + base + e, lam);
    cwf_store<T, 2 * NB, V>(a.S + 2 * (base + e), s);
    cwf_store<T, 2 * NB, V>(a.R + 2 * (base + e), b);
  });
  sum = cwf_block_reduce<false>(sum, lds4);
  cwf_put(a.part, kCwfPartMean, a.batch, a.nblk, sum);
}

// ---- u = p - G p: src is p (S_0 during the setup), Q holds G p, U receives u ------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kCwfThreads) void k_cwf_u(CwfArgs<T> a, const T* src) {
  const int64_t base = (int64_t)blockIdx.y * a.ft;
  const bool al = cwf_item_aligned(a.ft);
  cwf_for_bins(a.ft, al, [&](int64_t e, auto cnt, auto vec) {
    constexpr int NB = decltype(cnt)::value;
    constexpr bool V = decltype(vec)::value;
    T p[2 * NB], gp[2 * NB];
    cwf_load<T, 2 * NB, V>(src + 2 * (base + e), p);
    cwf_load<T, 2 * NB, V>(a.Q + 2 * (base + e), gp);
#pragma unroll
    for (int k = 0; k < 2 * NB; ++k) gp[k] = p[k] - gp[k];
    cwf_store<T, 2 * NB, V>(a.U + 2 * (base + e), gp);
  });
}

// ---- q = Lam p + g (u - G' u): Q holds G' u and receives q, with the partials of <p, q>.
// FIRST (the setup, p is S_0 and R holds X / v_n): g from the mean's partials, r = X / v_n - q into R, p = z = r / M into P, the
// partials of <r, z>; q itself is not kept. -----------------------------------------------------------------------------------------
template <typename T, bool FIRST>
__global__ __launch_bounds__(kCwfThreads) void k_cwf_q(CwfArgs<T> a) {
  __shared__ double lds4[kCwfThreads / 64];
  const int64_t base = (int64_t)blockIdx.y * a.ft;
  const bool al = cwf_item_aligned(a.ft);
  double* sc = a.scal + (size_t)blockIdx.y * kCwfScalStride;
  double g;
  if constexpr (FIRST) {
    const bool live = sc[kCwfScalM] > 0.0;
    const double mean = cwf_finish(a.part, kCwfPartMean, a.batch, a.nblk, lds4) / (double)a.ft;
    g = !live ? 0.0 : a.relative ? a.gamma / mean : a.gamma;
    if (blockIdx.x == 0 && threadIdx.x == 0) sc[kCwfScalG] = g;
  } else {
    g = sc[kCwfScalG];
  }
  const T gt = (T)g, gm = (T)(g * a.shrink);
  const T* src = FIRST ? a.S : a.P;
  double sum = 0.0;
  cwf_for_bins(a.ft, al, [&](int64_t e, auto cnt, auto vec) {
    constexpr int NB = decltype(cnt)::value;
    constexpr bool V = decltype(vec)::value;
    T p[2 * NB], u[2 * NB], q[2 * NB], lam[NB];
    cwf_load<T, 2 * NB, V>(src + 2 * (base + e), p);
    cwf_load<T, 2 * NB, V>(a.U + 2 * (base + e), u);
    cwf_load<T, 2 * NB, V>(a.Q + 2 * (base + e), q);
    cwf_load<T, NB, V>(a.lam + base + e, lam);
#pragma unroll
    for (int k = 0; k < 2 * NB; ++k) q[k] = lam[k >> 1] * p[k] + gt * (u[k] - q[k]);
    if constexpr (FIRST) {
      T r[2 * NB];
      cwf_load<T, 2 * NB, V>(a.R + 2 * (base + e), r);
#pragma unroll
      for (int k = 0; k < 2 * NB; ++k) {
        const T mk = lam[k >> 1] + gm;
        r[k] = r[k] - q[k];
        p[k] = mk > T(0) ? r[k] / mk : T(0);
        sum += (double)r[k] * (double)p[k];
      }
      cwf_store<T, 2 * NB, V>(a.R + 2 * (base + e), r);
      cwf_store<T, 2 * NB, V>(a.P + 2 * (base + e), p);
    } else {
#pragma unroll
      for (int k = 0; k < 2 * NB; ++k) sum += (double)p[k] * (double)q[k];
      cwf_store<T, 2 * NB, V>(a.Q + 2 * (base + e), q);
    }
  });
  sum = cwf_block_reduce<false>(sum, lds4);
  cwf_put(a.part, FIRST ? kCwfPartRz0 : kCwfPartPq, a.batch, a.nblk, sum);
}

// ---- iteration k: alpha = rz / <p, q> from the partials (0 for a finished item, and an item whose rz is 0 or whose <p, q> is not
// > 0 is finished from here on), S += alpha p, r -= alpha q, and the partials of <r, z> with z = r / M formed on the fly ------------
template <typename T>
__global__ __launch_bounds__(kCwfThreads) void k_cwf_update(CwfArgs<T> a, int k) {
  __shared__ double lds4[kCwfThreads / 64];
  const int64_t base = (int64_t)blockIdx.y * a.ft;
  const bool al = cwf_item_aligned(a.ft);
  double* sc = a.scal + (size_t)blockIdx.y * kCwfScalStride;
  const double pq = cwf_finish(a.part, kCwfPartPq, a.batch, a.nblk, lds4);
  const double rz = cwf_finish(a.part, cwf_rz_set(k - 1), a.batch, a.nblk, lds4);
  const bool fin = sc[kCwfScalFin0 + ((k - 1) & 1)] != 0.0 || rz == 0.0 || !(pq > 0.0);
  if (blockIdx.x == 0 && threadIdx.x == 0) sc[kCwfScalFin0 + (k & 1)] = fin ? 1.0 : 0.0;
  const T alpha = fin ? T(0) : (T)(rz / pq);
  const T gm = (T)(sc[kCwfScalG] * a.shrink);
  double sum = 0.0;
  cwf_for_bins(a.ft, al, [&](int64_t e, auto cnt, auto vec) {
    constexpr int NB = decltype(cnt)::value;
    constexpr bool V = decltype(vec)::value;
    T s[2 * NB], r[2 * NB], p[2 * NB], q[2 * NB], lam[NB];
    cwf_load<T, 2 * NB, V>(a.S + 2 * (base + e), s);
    cwf_load<T, 2 * NB, V>(a.R + 2 * (base + e), r);
    cwf_load<T, 2 * NB, V>(a.P + 2 * (base + e), p);
    cwf_load<T, 2 * NB, V>(a.Q + 2 * (base + e), q);
    cwf_load<T, NB, V>(a.lam + base + e, lam);
#pragma unroll
    for (int i = 0; i < 2 * NB; ++i) {
      const T mk = lam[i >> 1] + gm;
      s[i] = s[i] + alpha * p[i];
      r[i] = r[i] - alpha * q[i];
      const T z = mk > T(0) ? r[i] / mk : T(0);
      sum += (double)r[i] * (double)z;
    }
    cwf_store<T, 2 * NB, V>(a.S + 2 * (base + e), s);
    cwf_store<T, 2 * NB, V>(a.R + 2 * (base + e), r);
  });
  sum = cwf_block_reduce<false>(sum, lds4);
  cwf_put(a.part, cwf_rz_set(k), a.batch, a.nblk, sum);
}

// ---- after iteration k: beta = rz' / rz from the two sets of partials (0 for a finished item), p = z + beta p ---------------------
template <typename T>
__global__ __launch_bounds__(kCwfThreads) void k_cwf_dir(CwfArgs<T> a, int k) {
  __shared__ double lds4[kCwfThreads / 64];
  const int64_t base = (int64_t)blockIdx.y * a.ft;
  const bool al = cwf_item_aligned(a.ft);
  const double* sc = a.scal + (size_t)blockIdx.y * kCwfScalStride;
  const double rz_old = cwf_finish(a.part, cwf_rz_set(k - 1), a.batch, a.nblk, lds4);
  const double rz_new = cwf_finish(a.part, cwf_rz_set(k), a.batch, a.nblk, lds4);
  const T beta = sc[kCwfScalFin0 + (k & 1)] != 0.0 ? T(0) : (T)(rz_new / rz_old);
  const T gm = (T)(sc[kCwfScalG] * a.shrink);
  cwf_for_bins(a.ft, al, [&](int64_t e, auto cnt, auto vec) {
    constexpr int NB = decltype(cnt)::value;
    constexpr bool V = decltype(vec)::value;
    T r[2 * NB], p[2 * NB], lam[NB];
    cwf_load<T, 2 * NB, V>(a.R + 2 * (base + e), r);
    cwf_load<T, 2 * NB, V>(a.P + 2 * (base + e), p);
    cwf_load<T, NB, V>(a.lam + base + e, lam);
#pragma unroll
    for (int i = 0; i < 2 * NB; ++i) {
      const T mk = lam[i >> 1] + gm;
      p[i] = (mk > T(0) ? r[i] / mk : T(0)) + beta * p[i];
    }
    cwf_store<T, 2 * NB, V>(a.P + 2 * (base + e), p);
  });
}

// ---- the residuals after k iterations, sqrt(rz / rz0), 0 for a finished item: grid (1, batch) ------------------------------------
__global__ __launch_bounds__(kCwfThreads) void k_cwf_residual(const double* part, const double* scal, int batch, int nblk, int k,
                                                               double* res) {
  __shared__ double lds4[kCwfThreads / 64];
  const double rz0 = cwf_finish(part, kCwfPartRz0, batch, nblk, lds4);
  const double rz = cwf_finish(part, cwf_rz_set(k), batch, nblk, lds4);
  const bool fin = scal[(size_t)blockIdx.y * kCwfScalStride + kCwfScalFin0 + (k & 1)] != 0.0 || rz == 0.0 || !(rz0 > 0.0);
  if (threadIdx.x == 0) res[blockIdx.y] = fin ? 0.0 : sqrt(rz / rz0);
}

// ---- N = X - S, once at the end (Q, the scratch of the loop, is N_out) -----------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kCwfThreads) void k_cwf_noise(CwfArgs<T> a) {
  const int64_t base = (int64_t)blockIdx.y * a.ft;
  const bool al = cwf_item_aligned(a.ft);
  cwf_for_bins(a.ft, al, [&](int64_t e, auto cnt, auto vec) {
    constexpr int NB = decltype(cnt)::value;
    constexpr bool V = decltype(vec)::value;
    T x[2 * NB], s[2 * NB];
    cwf_load<T, 2 * NB, V>(a.mix + 2 * (base + e), x);
    cwf_load<T, 2 * NB, V>(a.S + 2 * (base + e), s);
#pragma unroll
    for (int i = 0; i < 2 * NB; ++i) x[i] = x[i] - s[i];
    cwf_store<T, 2 * NB, V>(a.Q + 2 * (base + e), x);
  });
}

// the launches (tu_cwf.hip)
enum { kCwfMax = 0, kCwfInit, kCwfU0, kCwfQ0, kCwfU, kCwfQ, kCwfUpdate, kCwfDir, kCwfNoise };
template <typename T>
int cwf_launch(int which, const CwfArgs<T>& a, int k, hipStream_t stream);
int cwf_residual_launch(const double* part, const double* scal, int batch, int nblk, int k, double* res, hipStream_t stream);

}  // namespace specinv
