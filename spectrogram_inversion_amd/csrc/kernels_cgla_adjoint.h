// The element-wise kernel of constrained AGLA's backward sweep (constrained_unfolded): k_agla_step_adjoint
// (kernels_agla_adjoint.h) with the select of the known samples and the constant signal of the known bins.  Iteration n >= 2 is
//     u = P(c_{n-1}) + off ;  t_n = where(W, off, (1 - gamma_n) d_{n-1} + gamma_n u) ;  c_n, d_n as in AGLA
// (kernels_cgla.h), off = where(W, xk, k) the one constant signal of the run.  The sweep carries a, gc, gd as AGLA's does and goff,
// the cotangent of off, which it accumulates.  One step, with delta = t_n - t_{n-1}:
//     s  = a + (1 + alpha_n) gc + (1 + beta_n) gd                                  the whole cotangent of t_n
//     s' = W ? 0 : s                                                               what passes the select
//     alpha_bar_n = <gc, delta> ;  beta_bar_n = <gd, delta> ;  gamma_bar_n = <s', t_n - d_{n-1}> / gamma_n
//     goff += W ? s : gamma_n s'
//     a <- -alpha_n gc - beta_n gd ;  gd <- (1 - gamma_n) s' ;  gc <- gamma_n s' / env ;  c_prev <- c_{n-1}
// Off W, t_n - d_{n-1} = gamma_n (u - d_{n-1}); on W, s' is 0: no u has to be recorded.  gc then goes through the projection adjoint
// at c_prev against m' = where(M, 0, m) (plan_impl.h: proj_adjoint_stages).  FIRST is the closing step, t_1 = c_1 = d_1 =
// where(W, off, P(c_0) + off):  s = a + gc + gd ;  goff += s ;  gc <- s' / env, nothing else read or written.
// Memory-bound on plain rows (the recorded signals are whole waveforms): k_agla_step_adjoint's ten transfers of sizeof(T) per
// sample, eight with every gamma = 1, plus goff read and written and one mask byte.
#pragma once
#include "kernels_agla_adjoint.h"
#include "kernels_cgla.h"

namespace specinv {

template <typename T>
struct CglaAdjArgs {
  T* a;              // (B, L): AglaAdjArgs::a
  T* gc;             // (B, L): cotangent of c_n in, gamma_n s' / env out
  T* gd;             // (B, L): cotangent of d_n in, (1 - gamma_n) s' out; the GENERAL kernel alone (nullptr: every gamma is 1)
  T* goff;           // (B, L): the cotangent of off, accumulated
  const T* tn;       // (B, L): t_n
  const T* tp;       // (B, L): t_{n-1}
  const T* tpp;      // (B, L): t_{n-2}; nullptr for n = 2, where c_1 = d_1 = t_1
  const T* env;      // (L): the window-square envelope
  const uint8_t* mask;   // (B, L): non-zero where the sample is known; nullptr: no sample is
  T* c_prev;         // (B, L): c_{n-1}, what the projection of iteration n read, to rounding
  double* partials;  // (gridDim.x, 3): one triple of partial inner products per workgroup
  T alpha, beta, gamma, one_minus_gamma;   // of iteration n, each rounded to T once
  T alpha_p, beta_p;                       // of iteration n - 1
  int64_t L;
  int64_t upr;       // work items per row: L / V
  int64_t n_units;   // B * upr
  int first;         // the closing step
};

// V, GENERAL, the walk and the inner products are k_agla_step_adjoint's; the V mask bytes of a thread are one load, the mask pointer
// is uniform: one scalar branch per work item.  Every element of a, gc, gd, goff and c_prev is written by the thread that read it.
template <typename T, int V, bool GENERAL>
__global__ void __launch_bounds__(256) k_cgla_step_adjoint(CglaAdjArgs<T> p) {
  using Vec = MisiVec<T, V>;
  __shared__ double red[3][4];
  const T one_a = T(1) + p.alpha, one_b = T(1) + p.beta;
  const double beta_p = (double)p.beta_p;
  double s_al = 0, s_be = 0, s_ga = 0;
  for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < p.n_units; u += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = u / p.upr;
    const int64_t n = (u - b * p.upr) * V;
    const int64_t at = b * p.L + n;
    const Vec e = *reinterpret_cast<const Vec*>(p.env + n);
    const Vec a = *reinterpret_cast<const Vec*>(p.a + at);
    Vec gc = *reinterpret_cast<const Vec*>(p.gc + at);
    Vec go = *reinterpret_cast<const Vec*>(p.goff + at);
    Vec gd{};
    if constexpr (GENERAL) gd = *reinterpret_cast<const Vec*>(p.gd + at);
    CglaMask<V> w{};
    if (p.mask != nullptr) w = *reinterpret_cast<const CglaMask<V>*>(p.mask + at);
    if (p.first) {
#pragma unroll
      for (int i = 0; i < V; ++i) {
        T s = a.v[i] + gc.v[i];
        if constexpr (GENERAL) s += gd.v[i];
        go.v[i] += s;
        gc.v[i] = w.v[i] ? T(0) : s / e.v[i];
      }
      *reinterpret_cast<Vec*>(p.gc + at) = gc;
      *reinterpret_cast<Vec*>(p.goff + at) = go;
      continue;
    }
    const Vec tn = *reinterpret_cast<const Vec*>(p.tn + at);
    const Vec tp = *reinterpret_cast<const Vec*>(p.tp + at);
    Vec cp = tp, an, gdn{};
    double dprev[V];
#pragma unroll
    for (int i = 0; i < V; ++i) dprev[i] = (double)tp.v[i];
    if (p.tpp != nullptr) {
      const Vec tpp = *reinterpret_cast<const Vec*>(p.tpp + at);
#pragma unroll
      for (int i = 0; i < V; ++i) {
        cp.v[i] = tp.v[i] + p.alpha_p * (tp.v[i] - tpp.v[i]);
        dprev[i] = (double)tp.v[i] + beta_p * ((double)tp.v[i] - (double)tpp.v[i]);
      }
    }
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const double delta = (double)tn.v[i] - (double)tp.v[i];
      T s = a.v[i] + one_a * gc.v[i];
      an.v[i] = -p.alpha * gc.v[i];
      s_al += (double)gc.v[i] * delta;
      if constexpr (GENERAL) {
        s += one_b * gd.v[i];
        an.v[i] -= p.beta * gd.v[i];
        s_be += (double)gd.v[i] * delta;
      }
      const T sp = w.v[i] ? T(0) : s;                              // s'
      if constexpr (GENERAL) gdn.v[i] = p.one_minus_gamma * sp;
      s_ga += (double)sp * ((double)tn.v[i] - dprev[i]);
      const T through = GENERAL ? p.gamma * sp : sp;               // to u: to the projection and, off W, to off
      go.v[i] += w.v[i] ? s : through;
      gc.v[i] = through / e.v[i];
    }
    *reinterpret_cast<Vec*>(p.a + at) = an;
    *reinterpret_cast<Vec*>(p.gc + at) = gc;
    if constexpr (GENERAL) *reinterpret_cast<Vec*>(p.gd + at) = gdn;
    *reinterpret_cast<Vec*>(p.goff + at) = go;
    *reinterpret_cast<Vec*>(p.c_prev + at) = cp;
  }
  if (p.first) return;
  // (every lane is back from the loop: the moves below read all 64)
  s_al = wave_scan_inclusive(s_al);
  s_be = wave_scan_inclusive(s_be);
  s_ga = wave_scan_inclusive(s_ga);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 63) {
    red[0][wave] = s_al;
    red[1][wave] = s_be;
    red[2][wave] = s_ga;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const double* r = red[threadIdx.x];
    p.partials[(int64_t)blockIdx.x * 3 + threadIdx.x] = ((r[0] + r[1]) + r[2]) + r[3];
  }
}

// Host side (tu_cgla_adjoint.hip): picks V (the widest of 16 / 8 / 4 bytes - float64: 16 / 8 - that divides L and the pointers'
// alignment) and GENERAL (p.gd != nullptr), launches at most kAglaAdjMaxGrid workgroups of 256 and, unless p.first, the finishing
// launch of AGLA's sweep (agla_dots_finish_launch) that leaves {alpha_bar, beta_bar, gamma_bar} in dots_dev.  p.upr and p.n_units
// are filled in here; p.partials holds 3 * kAglaAdjMaxGrid doubles.
template <typename T>
int cgla_step_adjoint_launch(CglaAdjArgs<T> p, int batch, double* dots_dev, hipStream_t stream);

}  // namespace specinv
