// Flat and multi-vector kernels of L_BFGS (reference: torch.optim.LBFGS) and their lb_* launchers: reductions and updates of
// the two-loop recursion over parameter-sized vectors, accumulated in float64.
#pragma once
#include "common.h"
#include "kernels_generic.h"

namespace specinv {

// ---- flat vector kernels ------------------------------------------------------------------------------
template <typename T>
__global__ void k_dot_partials(const T* __restrict__ a, const T* __restrict__ b, int64_t n, double* __restrict__ part) {
  __shared__ double red[16];
  double s = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    s += (double)a[i] * (double)b[i];
  const double t = block_sum(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

template <typename T>
__global__ void k_abs_partials(const T* __restrict__ a, int64_t n, double* __restrict__ part) {
  __shared__ double red[16];
  double s = 0, m = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double v = fabs((double)a[i]);
    s += v;
    m = v > m ? v : m;
  }
  // max over the block
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double o = __shfl_xor(m, off, 64);
    m = o > m ? o : m;
  }
  __shared__ double mx[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) mx[wave] = m;
  const double t = block_sum(s, red);
  if (threadIdx.x == 0) {
    double mm = 0;
    for (int w = 0; w < (int)((blockDim.x + 63) >> 6); ++w) mm = mx[w] > mm ? mx[w] : mm;
    part[2 * blockIdx.x] = mm;
    part[2 * blockIdx.x + 1] = t;
  }
}

// out[0] = max_i part[2i], out[1] = sum_i part[2i+1]
static __global__ void k_finish_absmax(const double* __restrict__ part, int n, double* __restrict__ out) {
  __shared__ double red[16];
  double s = 0, m = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    m = part[2 * i] > m ? part[2 * i] : m;
    s += part[2 * i + 1];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double o = __shfl_xor(m, off, 64);
    m = o > m ? o : m;
  }
  __shared__ double mx[16];
  if ((threadIdx.x & 63) == 0) mx[threadIdx.x >> 6] = m;
  const double t = block_sum(s, red);
  if (threadIdx.x == 0) {
    double mm = 0;
    for (int w = 0; w < (int)((blockDim.x + 63) >> 6); ++w) mm = mx[w] > mm ? mx[w] : mm;
    out[0] = mm;
    out[1] = t;
  }
}

template <typename T>
__global__ void k_axpy(T alpha, const T* __restrict__ x, T* __restrict__ y, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = y[i] + alpha * x[i];
}

template <typename T>
__global__ void k_scale(T alpha, const T* __restrict__ x, T* __restrict__ y, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = alpha * x[i];
}

// One pass for the curvature pair of an L-BFGS iteration: y = g - g_prev, s = t * d, partial sums of y.s, y.y, g.g and
// g.g_prev (the last two give the new pair's products with g by linearity: y.g = g.g - g_prev.g)
template <typename T>
__global__ void k_lbfgs_pair(const T* __restrict__ g, const T* __restrict__ gp, const T* __restrict__ d, T t,
                             T* __restrict__ y, T* __restrict__ sv, int64_t n, double* __restrict__ part) {
  __shared__ double red[16];
  double ys = 0, yy = 0, gg = 0, ggp = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const T gi = g[i], pi = gp[i];
    const T yi = gi - pi;
    const T si = t * d[i];
    y[i] = yi;
    sv[i] = si;
    ys += (double)yi * (double)si;
    yy += (double)yi * (double)yi;
    gg += (double)gi * (double)gi;
    ggp += (double)gi * (double)pi;
  }
  const double a = block_sum(ys, red), b = block_sum(yy, red), c = block_sum(gg, red), e = block_sum(ggp, red);
  if (threadIdx.x == 0) {
    part[4 * blockIdx.x] = a;
    part[4 * blockIdx.x + 1] = b;
    part[4 * blockIdx.x + 2] = c;
    part[4 * blockIdx.x + 3] = e;
  }
}

// One pass for what a step needs to know about g and d: g.d, max|g|, sum|g|, max|d|
template <typename T>
__global__ void k_lbfgs_stats(const T* __restrict__ g, const T* __restrict__ d, int64_t n, double* __restrict__ part) {
  __shared__ double red[16];
  __shared__ double mx[2][16];
  double gd = 0, sg = 0, mg = 0, md = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double gi = (double)g[i], di = (double)d[i];
    gd += gi * di;
    const double ag = fabs(gi), ad = fabs(di);
    sg += ag;
    mg = ag > mg ? ag : mg;
    md = ad > md ? ad : md;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double o1 = __shfl_xor(mg, off, 64), o2 = __shfl_xor(md, off, 64);
    mg = o1 > mg ? o1 : mg;
    md = o2 > md ? o2 : md;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    mx[0][wave] = mg;
    mx[1][wave] = md;
  }
  const double a = block_sum(gd, red), b = block_sum(sg, red);
  if (threadIdx.x == 0) {
    double m0 = 0, m1 = 0;
    for (int w = 0; w < (int)((blockDim.x + 63) >> 6); ++w) {
      m0 = mx[0][w] > m0 ? mx[0][w] : m0;
      m1 = mx[1][w] > m1 ? mx[1][w] : m1;
    }
    part[4 * blockIdx.x] = a;
    part[4 * blockIdx.x + 1] = b;
    part[4 * blockIdx.x + 2] = m0;
    part[4 * blockIdx.x + 3] = m1;
  }
}

// out[0..1] = sums of part[4i], part[4i+1]; out[2..3] = maxima of part[4i+2], part[4i+3]   (one workgroup, fixed order)
static __global__ void k_finish_stats(const double* __restrict__ part, int n, double* __restrict__ out) {
  __shared__ double red[16];
  __shared__ double mx[2][16];
  double a = 0, b = 0, m0 = 0, m1 = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    a += part[4 * i];
    b += part[4 * i + 1];
    m0 = part[4 * i + 2] > m0 ? part[4 * i + 2] : m0;
    m1 = part[4 * i + 3] > m1 ? part[4 * i + 3] : m1;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double o0 = __shfl_xor(m0, off, 64), o1 = __shfl_xor(m1, off, 64);
    m0 = o0 > m0 ? o0 : m0;
    m1 = o1 > m1 ? o1 : m1;
  }
  if ((threadIdx.x & 63) == 0) {
    mx[0][threadIdx.x >> 6] = m0;
    mx[1][threadIdx.x >> 6] = m1;
  }
  const double ta = block_sum(a, red), tb = block_sum(b, red);
  if (threadIdx.x == 0) {
    double r0 = 0, r1 = 0;
    for (int w = 0; w < (int)((blockDim.x + 63) >> 6); ++w) {
      r0 = mx[0][w] > r0 ? mx[0][w] : r0;
      r1 = mx[1][w] > r1 ? mx[1][w] : r1;
    }
    out[0] = ta;
    out[1] = tb;
    out[2] = r0;
    out[3] = r1;
  }
}

// The curvature pair and the step statistics in ONE pass over g, g_prev, d (what an L-BFGS iteration needs to know about
// the new gradient): partials per block = {g.d, sum|g|, y.s, y.y, g.g, g.g_prev, max|g|, max|d|}
template <typename T>
__global__ void k_lbfgs_pair_stats(const T* __restrict__ g, const T* __restrict__ gp, const T* __restrict__ d, T t,
                                   T* __restrict__ y, T* __restrict__ sv, int64_t n, double* __restrict__ part) {
  __shared__ double red[16];
  __shared__ double mx[2][16];
  double s[6] = {0, 0, 0, 0, 0, 0}, mg = 0, md = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const T gi = g[i], pi = gp[i], di = d[i];
    const T yi = gi - pi;
    const T si = t * di;
    y[i] = yi;
    sv[i] = si;
    const double g64 = (double)gi, d64 = (double)di, ag = fabs(g64), ad = fabs(d64);
    s[0] += g64 * d64;
    s[1] += ag;
    s[2] += (double)yi * (double)si;
    s[3] += (double)yi * (double)yi;
    s[4] += g64 * g64;
    s[5] += g64 * (double)pi;
    mg = ag > mg ? ag : mg;
    md = ad > md ? ad : md;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double o1 = __shfl_xor(mg, off, 64), o2 = __shfl_xor(md, off, 64);
    mg = o1 > mg ? o1 : mg;
    md = o2 > md ? o2 : md;
  }
  if ((threadIdx.x & 63) == 0) {
    mx[0][threadIdx.x >> 6] = mg;
    mx[1][threadIdx.x >> 6] = md;
  }
  double tot[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) tot[c] = block_sum(s[c], red);
  if (threadIdx.x == 0) {
    double m0 = 0, m1 = 0;
    for (int w = 0; w < (int)((blockDim.x + 63) >> 6); ++w) {
      m0 = mx[0][w] > m0 ? mx[0][w] : m0;
      m1 = mx[1][w] > m1 ? mx[1][w] : m1;
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) part[8 * blockIdx.x + c] = tot[c];
    part[8 * blockIdx.x + 6] = m0;
    part[8 * blockIdx.x + 7] = m1;
  }
}

// out = {g.d, sum|g|, max|g|, max|d|, y.s, y.y, g.g, g.g_prev}   (one workgroup, fixed order)
static __global__ void k_finish_pair_stats(const double* __restrict__ part, int n, double* __restrict__ out) {
  __shared__ double red[16];
  __shared__ double mx[2][16];
  double s[6] = {0, 0, 0, 0, 0, 0}, m0 = 0, m1 = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
#pragma unroll
    for (int c = 0; c < 6; ++c) s[c] += part[8 * i + c];
    m0 = part[8 * i + 6] > m0 ? part[8 * i + 6] : m0;
    m1 = part[8 * i + 7] > m1 ? part[8 * i + 7] : m1;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double o0 = __shfl_xor(m0, off, 64), o1 = __shfl_xor(m1, off, 64);
    m0 = o0 > m0 ? o0 : m0;
    m1 = o1 > m1 ? o1 : m1;
  }
  if ((threadIdx.x & 63) == 0) {
    mx[0][threadIdx.x >> 6] = m0;
    mx[1][threadIdx.x >> 6] = m1;
  }
  double tot[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) tot[c] = block_sum(s[c], red);
  if (threadIdx.x == 0) {
    double r0 = 0, r1 = 0;
    for (int w = 0; w < (int)((blockDim.x + 63) >> 6); ++w) {
      r0 = mx[0][w] > r0 ? mx[0][w] : r0;
      r1 = mx[1][w] > r1 ? mx[1][w] : r1;
    }
    out[0] = tot[0];
    out[1] = tot[1];
    out[2] = r0;
    out[3] = r1;
    out[4] = tot[2];
    out[5] = tot[3];
    out[6] = tot[4];
    out[7] = tot[5];
  }
}

template <typename P, typename T>
int lb_pair_stats(P& pl, const T* g, const T* gp, const T* d, double t, T* y, T* sv, int64_t n, double* out8_dev) {
  SI_CHECK(g && gp && d && y && sv && out8_dev && n > 0, SPECINV_EINVAL, "bad arguments");
  const int nb = (int)std::min<int64_t>(1024, std::max<int64_t>(1, ceil_div(n, 256 * 8)));
  SI_TRY(pl.lb_part.reserve((size_t)4 * 4 * 1024 * sizeof(double)));
  double* part = pl.lb_part.template as<double>() + 2 * 4 * 1024;       // slots 2-3 of 4
  hipLaunchKernelGGL((k_lbfgs_pair_stats<T>), dim3(nb), dim3(256), 0, pl.stream, g, gp, d, (T)t, y, sv, n, part);
  SI_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_finish_pair_stats, dim3(1), dim3(256), 0, pl.stream, part, nb, out8_dev);
  SI_HIP(hipGetLastError());
  return SPECINV_OK;
}

// Results go to the host (`out_host`: the call synchronises) or to device memory (`out_dev`: nothing waits; the partial
// sums then live in a scratch of their own, `pl.lb_part`, slot `part_slot`, so that back-to-back passes do not share one).
template <typename P, typename T>
int lb_pair(P& pl, const T* g, const T* gp, const T* d, double t, T* y, T* sv, int64_t n, double* out2_host,
            double* out4_dev = nullptr) {
  SI_CHECK(g && gp && d && y && sv && (out2_host || out4_dev) && n > 0, SPECINV_EINVAL, "bad arguments");
  const int nb = (int)std::min<int64_t>(1024, std::max<int64_t>(1, ceil_div(n, 256 * 8)));
  SI_TRY(pl.lb_part.reserve((size_t)4 * 4 * 1024 * sizeof(double)));
  double* part = pl.lb_part.template as<double>();                      // slot 0 of 4
  hipLaunchKernelGGL((k_lbfgs_pair<T>), dim3(nb), dim3(256), 0, pl.stream, g, gp, d, (T)t, y, sv, n, part);
  SI_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_finish_partials, dim3(1), dim3(256), 0, pl.stream, part, (int64_t)nb, 4,
                     out4_dev ? out4_dev : pl.sums.template as<double>());
  SI_HIP(hipGetLastError());
  if (out4_dev) return SPECINV_OK;
  SI_HIP(hipMemcpyAsync(out2_host, pl.sums.p, 2 * sizeof(double), hipMemcpyDeviceToHost, pl.stream));
  SI_HIP(si_stream_wait_short(pl.stream));
  return SPECINV_OK;
}

template <typename P, typename T>
int lb_stats(P& pl, const T* g, const T* d, int64_t n, double* out4_host, double* out4_dev = nullptr) {
  SI_CHECK(g && d && (out4_host || out4_dev) && n > 0, SPECINV_EINVAL, "bad arguments");
  const int nb = (int)std::min<int64_t>(1024, std::max<int64_t>(1, ceil_div(n, 256 * 8)));
  SI_TRY(pl.lb_part.reserve((size_t)4 * 4 * 1024 * sizeof(double)));
  double* part = pl.lb_part.template as<double>() + 4 * 1024;           // slot 1 of 4
  hipLaunchKernelGGL((k_lbfgs_stats<T>), dim3(nb), dim3(256), 0, pl.stream, g, d, n, part);
  SI_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_finish_stats, dim3(1), dim3(256), 0, pl.stream, part, nb, out4_dev ? out4_dev : pl.sums.template as<double>());
  SI_HIP(hipGetLastError());
  if (out4_dev) return SPECINV_OK;
  SI_HIP(hipMemcpyAsync(out4_host, pl.sums.p, 4 * sizeof(double), hipMemcpyDeviceToHost, pl.stream));
  SI_HIP(si_stream_wait_short(pl.stream));
  return SPECINV_OK;
}

template <typename P, typename T>
int lb_dot(P& pl, const T* a, const T* b, int64_t n, double* out) {
  SI_CHECK(a && b && out && n > 0, SPECINV_EINVAL, "bad arguments");
  const int nb = (int)std::min<int64_t>(1024, std::max<int64_t>(1, ceil_div(n, 256 * 8)));
  SI_TRY(pl.partials.reserve(std::max<size_t>((size_t)nb, 3 * 1024) * sizeof(double)));
  hipLaunchKernelGGL((k_dot_partials<T>), dim3(nb), dim3(256), 0, pl.stream, a, b, n, pl.partials.template as<double>());
  SI_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_finish_partials, dim3(1), dim3(256), 0, pl.stream, pl.partials.template as<double>(), (int64_t)nb, 1,
                     pl.sums.template as<double>());
  SI_HIP(hipGetLastError());
  SI_HIP(hipMemcpyAsync(out, pl.sums.p, sizeof(double), hipMemcpyDeviceToHost, pl.stream));
  SI_HIP(si_stream_wait_short(pl.stream));
  return SPECINV_OK;
}

template <typename P, typename T>
int lb_axpy(P& pl, T alpha, const T* x, T* y, int64_t n) {
  SI_CHECK(x && y && n > 0, SPECINV_EINVAL, "bad arguments");
  hipLaunchKernelGGL((k_axpy<T>), dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, pl.stream, alpha, x, y, n);
  SI_HIP(hipGetLastError());
  return SPECINV_OK;
}

template <typename P, typename T>
int lb_scale(P& pl, T alpha, const T* x, T* y, int64_t n) {
  SI_CHECK(x && y && n > 0, SPECINV_EINVAL, "bad arguments");
  hipLaunchKernelGGL((k_scale<T>), dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, pl.stream, alpha, x, y, n);
  SI_HIP(hipGetLastError());
  return SPECINV_OK;
}

template <typename P, typename T>
int lb_absmax_abssum(P& pl, const T* x, int64_t n, double* out) {
  SI_CHECK(x && out && n > 0, SPECINV_EINVAL, "bad arguments");
  const int nb = (int)std::min<int64_t>(1024, std::max<int64_t>(1, ceil_div(n, 256 * 8)));
  SI_TRY(pl.partials.reserve(std::max<size_t>((size_t)nb * 2, 3 * 1024) * sizeof(double)));
  hipLaunchKernelGGL((k_abs_partials<T>), dim3(nb), dim3(256), 0, pl.stream, x, n, pl.partials.template as<double>());
  SI_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_finish_absmax, dim3(1), dim3(256), 0, pl.stream, pl.partials.template as<double>(), nb,
                     pl.sums.template as<double>());
  SI_HIP(hipGetLastError());
  SI_HIP(hipMemcpyAsync(out, pl.sums.p, 2 * sizeof(double), hipMemcpyDeviceToHost, pl.stream));
  SI_HIP(si_stream_wait_short(pl.stream));
  return SPECINV_OK;
}

// ---- many vectors in one pass (the L-BFGS recursion written on Gram matrices needs g . v_j for the whole memory and one
// linear combination of it: two passes over the 2 m vectors instead of four dependent ones per pair) ----------------
constexpr int kMultiVec = 64;   // vectors per launch (their addresses travel as kernel arguments)
template <typename T>
struct MultiVecArgs {
  const T* v[kMultiVec];
  double c[kMultiVec];
  int k;
};

// part[j * gridDim.x + block] = sum over the block's elements of g[e] * v_j[e]  (float64 accumulation, fixed order).
// A block keeps kSlab elements per thread of g in registers and streams the k vectors past them, 16 bytes per lane and
// load; one wave reduction per (block pass, j).
template <typename T>
__global__ __launch_bounds__(256) void k_multi_dot(const T* __restrict__ g, MultiVecArgs<T> a, int64_t n,
                                                   double* __restrict__ part) {
  constexpr int W = 16 / sizeof(T);                 // elements per 16-byte load
  constexpr int Q = 8;                              // 16-byte pieces per thread and pass
  typedef T VT __attribute__((ext_vector_type(W)));
  __shared__ double acc[4][kMultiVec];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int j = lane; j < a.k; j += 64) acc[wv][j] = 0.0;
  const int64_t nv = n / W;                         // whole 16-byte pieces; the tail is handled by block 0 below
  const int64_t pass = (int64_t)blockDim.x * Q;
  for (int64_t base = (int64_t)blockIdx.x * pass; base < nv; base += (int64_t)gridDim.x * pass) {
    VT gv[Q];
#pragma unroll
    for (int e = 0; e < Q; ++e) {
      const int64_t i = base + (int64_t)e * blockDim.x + threadIdx.x;
      if (i < nv) gv[e] = reinterpret_cast<const VT*>(g)[i];
      else
        for (int c = 0; c < W; ++c) gv[e][c] = T(0);
    }
    for (int j = 0; j < a.k; ++j) {
      const VT* __restrict__ v = reinterpret_cast<const VT*>(a.v[j]);
      VT vv[Q];
#pragma unroll
      for (int e = 0; e < Q; ++e) {
        const int64_t i = base + (int64_t)e * blockDim.x + threadIdx.x;
        if (i < nv) vv[e] = v[i];
        else
          for (int c = 0; c < W; ++c) vv[e][c] = T(0);
      }
      double s = 0.0;
#pragma unroll
      for (int e = 0; e < Q; ++e)
#pragma unroll
        for (int c = 0; c < W; ++c) s += (double)gv[e][c] * (double)vv[e][c];
      s = wave_sum(s);
      if (lane == 0) acc[wv][j] += s;               // wave-private slot: no atomics, fixed order
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {        // the n % W trailing elements
    for (int j = 0; j < a.k; ++j) {
      double s = 0.0;
      for (int64_t i = nv * W; i < n; ++i) s += (double)g[i] * (double)a.v[j][i];
      acc[0][j] += s;
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < a.k; j += blockDim.x)
    part[(int64_t)j * gridDim.x + blockIdx.x] = ((acc[0][j] + acc[1][j]) + acc[2][j]) + acc[3][j];
}

// out[j] = sum_b part[j * nb + b]
static __global__ void k_multi_finish(const double* __restrict__ part, int nb, double* __restrict__ out) {
  __shared__ double red[16];
  const int j = blockIdx.x;
  double s = 0;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) s += part[(int64_t)j * nb + i];
  const double t = block_sum(s, red);
  if (threadIdx.x == 0) out[j] = t;
}

// out[e] = (accumulate ? out[e] : 0) + sum_j c_j * v_j[e], summed in float64 in the order of j, rounded once; one
// 16-byte piece per thread (the trailing n % W elements by the last thread)
// With `xs` given the same pass also takes the step xs += t * out (the rounded direction: what k_axpy would read back).
template <typename T>
__global__ __launch_bounds__(256) void k_lincomb(MultiVecArgs<T> a, int accumulate, T* __restrict__ out, int64_t n,
                                                 T t = T(0), T* __restrict__ xs = nullptr) {
  constexpr int W = 16 / sizeof(T);
  typedef T VT __attribute__((ext_vector_type(W)));
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nv = n / W;
  if (i < nv) {
    double s[W];
    const VT o = accumulate ? reinterpret_cast<const VT*>(out)[i] : VT(0);
#pragma unroll
    for (int c = 0; c < W; ++c) s[c] = (double)o[c];
#pragma unroll 4
    for (int j = 0; j < a.k; ++j) {
      const VT v = reinterpret_cast<const VT*>(a.v[j])[i];
#pragma unroll
      for (int c = 0; c < W; ++c) s[c] += a.c[j] * (double)v[c];
    }
    VT r;
#pragma unroll
    for (int c = 0; c < W; ++c) r[c] = (T)s[c];
    reinterpret_cast<VT*>(out)[i] = r;
    if (xs != nullptr) {
      VT xv = reinterpret_cast<const VT*>(xs)[i];
#pragma unroll
      for (int c = 0; c < W; ++c) xv[c] = fma(t, r[c], xv[c]);
      reinterpret_cast<VT*>(xs)[i] = xv;
    }
  } else if (i == nv) {
    for (int64_t e = nv * W; e < n; ++e) {
      double s = accumulate ? (double)out[e] : 0.0;
      for (int j = 0; j < a.k; ++j) s += a.c[j] * (double)a.v[j][e];
      out[e] = (T)s;
      if (xs != nullptr) xs[e] = fma(t, (T)s, xs[e]);
    }
  }
}

template <typename P, typename T>
int lb_multi_dot(P& pl, const T* g, const void* const* vecs, int k, int64_t n, double* out, double* out_dev = nullptr) {
  SI_CHECK(g && vecs && (out || out_dev) && k > 0 && n > 0, SPECINV_EINVAL, "bad arguments");
  SI_CHECK(((uintptr_t)g & 15) == 0, SPECINV_EINVAL, "g is not 16-byte aligned");
  const int nb = (int)std::min<int64_t>(1024, std::max<int64_t>(1, ceil_div(n, 256 * 8 * 4)));
  SI_TRY(pl.partials.reserve(std::max<size_t>((size_t)nb * kMultiVec, 3 * 1024) * sizeof(double)));
  SI_TRY(pl.lb_scal.reserve((size_t)std::max(k, 4) * sizeof(double)));
  double* dots = out_dev ? out_dev : pl.lb_scal.template as<double>();
  for (int j0 = 0; j0 < k; j0 += kMultiVec) {
    MultiVecArgs<T> a{};
    a.k = std::min(kMultiVec, k - j0);
    for (int j = 0; j < a.k; ++j) {
      SI_CHECK(vecs[j0 + j] != nullptr && ((uintptr_t)vecs[j0 + j] & 15) == 0, SPECINV_EINVAL,
               "vector %d is NULL or not 16-byte aligned", j0 + j);
      a.v[j] = static_cast<const T*>(vecs[j0 + j]);
    }
    hipLaunchKernelGGL((k_multi_dot<T>), dim3(nb), dim3(256), 0, pl.stream, g, a, n, pl.partials.template as<double>());
    hipLaunchKernelGGL(k_multi_finish, dim3(a.k), dim3(256), 0, pl.stream, pl.partials.template as<double>(), nb, dots + j0);
    SI_HIP(hipGetLastError());
  }
  if (out_dev) return SPECINV_OK;
  SI_HIP(hipMemcpyAsync(out, dots, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, pl.stream));
  SI_HIP(si_stream_wait_short(pl.stream));
  return SPECINV_OK;
}

template <typename P, typename T>
int lb_lincomb(P& pl, const void* const* vecs, const double* coef, int k, int64_t n, T* out, double t = 0.0, T* xs = nullptr) {
  SI_CHECK(vecs && coef && out && k > 0 && n > 0, SPECINV_EINVAL, "bad arguments");
  SI_CHECK(((uintptr_t)out & 15) == 0, SPECINV_EINVAL, "out is not 16-byte aligned");
  SI_CHECK(xs == nullptr || ((uintptr_t)xs & 15) == 0, SPECINV_EINVAL, "x is not 16-byte aligned");
  for (int j0 = 0; j0 < k; j0 += kMultiVec) {
    MultiVecArgs<T> a{};
    a.k = std::min(kMultiVec, k - j0);
    for (int j = 0; j < a.k; ++j) {
      SI_CHECK(vecs[j0 + j] != nullptr && ((uintptr_t)vecs[j0 + j] & 15) == 0, SPECINV_EINVAL,
               "vector %d is NULL or not 16-byte aligned", j0 + j);
      a.v[j] = static_cast<const T*>(vecs[j0 + j]);
      a.c[j] = coef[j0 + j];
    }
    const int64_t pieces = n / (16 / (int64_t)sizeof(T)) + 1;      // + the thread that takes the trailing elements
    const bool last = j0 + kMultiVec >= k;                         // the step rides on the launch that completes the sum
    hipLaunchKernelGGL((k_lincomb<T>), dim3((unsigned)ceil_div(pieces, 256)), dim3(256), 0, pl.stream, a, j0 > 0 ? 1 : 0, out, n,
                       (T)t, last ? xs : nullptr);
    SI_HIP(hipGetLastError());
  }
  return SPECINV_OK;
}

// ---- two-loop recursion with device-resident scalars -----------------------------------------------------
// slot = scale * sum(partials)      (al_i = rho_i * (s_i . q))
static __global__ void k_finish_scaled(const double* __restrict__ part, int n, double scale, double* __restrict__ slot) {
  __shared__ double red[16];
  double s = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) s += part[i];
  const double t = block_sum(s, red);
  if (threadIdx.x == 0) *slot = scale * t;
}

// y += (sa * a[0] + sb * (b ? b[0] : 0)) * x    with the coefficient read from device memory
template <typename T>
__global__ void k_axpy_dev(const double* __restrict__ a, double sa, const double* __restrict__ b, double sb,
                           const T* __restrict__ x, T* __restrict__ y, int64_t n) {
  const T c = (T)(sa * a[0] + (b ? sb * b[0] : 0.0));
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = y[i] + c * x[i];
}

template <typename P, typename T>
int lb_direction(P& pl, const T* g, const void* const* s_list, const void* const* y_list, const double* rho, int m,
                 double h_diag, T* d, int64_t n) {
  SI_CHECK(g && d && n > 0 && m >= 0, SPECINV_EINVAL, "bad arguments");
  SI_CHECK(m == 0 || (s_list && y_list && rho), SPECINV_EINVAL, "history arrays are NULL");
  const int nb = (int)std::min<int64_t>(1024, std::max<int64_t>(1, ceil_div(n, 256 * 8)));
  SI_TRY(pl.partials.reserve(std::max<size_t>((size_t)nb, 3 * 1024) * sizeof(double)));
  SI_TRY(pl.lb_scal.reserve((size_t)(m + 2) * sizeof(double)));
  double* al = pl.lb_scal.template as<double>();      // al[0..m-1], be at al[m]
  double* part = pl.partials.template as<double>();
  const dim3 ge((unsigned)ceil_div(n, 256)), blk(256);
  hipLaunchKernelGGL((k_scale<T>), ge, blk, 0, pl.stream, T(-1), g, d, n);                       // q = -g
  for (int i = m - 1; i >= 0; --i) {
    const T* si = static_cast<const T*>(s_list[i]);
    const T* yi = static_cast<const T*>(y_list[i]);
    hipLaunchKernelGGL((k_dot_partials<T>), dim3(nb), blk, 0, pl.stream, si, static_cast<const T*>(d), n, part);
    hipLaunchKernelGGL(k_finish_scaled, dim3(1), blk, 0, pl.stream, part, nb, rho[i], al + i);   // al_i
    hipLaunchKernelGGL((k_axpy_dev<T>), ge, blk, 0, pl.stream, al + i, -1.0, (const double*)nullptr, 0.0, yi, d, n);
  }
  hipLaunchKernelGGL((k_scale<T>), ge, blk, 0, pl.stream, (T)h_diag, static_cast<const T*>(d), d, n);   // r = H0 q
  for (int i = 0; i < m; ++i) {
    const T* si = static_cast<const T*>(s_list[i]);
    const T* yi = static_cast<const T*>(y_list[i]);
    hipLaunchKernelGGL((k_dot_partials<T>), dim3(nb), blk, 0, pl.stream, yi, static_cast<const T*>(d), n, part);
    hipLaunchKernelGGL(k_finish_scaled, dim3(1), blk, 0, pl.stream, part, nb, rho[i], al + m);   // be_i
    hipLaunchKernelGGL((k_axpy_dev<T>), ge, blk, 0, pl.stream, al + i, 1.0, al + m, -1.0, si, d, n);
  }
  SI_HIP(hipGetLastError());
  return SPECINV_OK;
}

}  // namespace specinv
