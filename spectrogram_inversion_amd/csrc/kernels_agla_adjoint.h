// The element-wise kernel of AGLA's backward sweep (agla_unfolded).  Iteration n >= 2 of the unfolded method is
//     y = P(c_{n-1}) ;  t_n = (1 - gamma_n) d_{n-1} + gamma_n y ;  c_n = t_n + alpha_n (t_n - t_{n-1}) ;  d_n = t_n + beta_n (t_n - t_{n-1})
// (kernels_agla.h), P = B proj A the momentum-free projection.  The sweep carries a, gc, gd - the cotangents of t_n (complete), c_n
// and d_n - and only the t's were recorded.  One step, with delta = t_n - t_{n-1}:
//     s = a + (1 + alpha_n) gc + (1 + beta_n) gd                                   the whole cotangent of t_n
//     alpha_bar_n = <gc, delta> ;  beta_bar_n = <gd, delta> ;  gamma_bar_n = <s, t_n - d_{n-1}> / gamma_n      (= <s, y - d_{n-1}>)
//     a <- -alpha_n gc - beta_n gd ;  gd <- (1 - gamma_n) s ;  gc <- gamma_n s / env                            (B^T's division)
//     c_prev <- c_{n-1} = t_{n-1} + alpha_{n-1} (t_{n-1} - t_{n-2})   (n = 2: t_1) ;  d_{n-1} likewise with beta_{n-1}
// after which gc goes through the projection adjoint at c_prev (plan_impl.h: proj_adjoint_stages, the stages MISI's sweep runs).
// FIRST is the closing step, t_1 = c_1 = d_1 = P(c_0):  gc <- (a + gc + gd) / env, nothing else read or written.
// Memory-bound on plain rows: ten transfers of sizeof(T) per sample (a, gc, gd, t_n, t_{n-1}, t_{n-2} read; a, gc, gd, c_prev
// written), eight with every gamma = 1, where gd is identically 0 and neither allocated nor touched; the envelope's L values stay in
// the caches.
//
// Under a constraint (constrained_unfolded) iteration n >= 2 is
//     u = P(c_{n-1}) + off ;  t_n = where(W, off, (1 - gamma_n) d_{n-1} + gamma_n u) ;  c_n, d_n as above,
// off = where(W, xk, k) the one constant signal of the run, and the sweep also carries goff, the cotangent of off, which it
// accumulates.  With s' = W ? 0 : s, what passes the select:
//     gamma_bar_n = <s', t_n - d_{n-1}> / gamma_n ;  goff += W ? s : gamma_n s' ;  gd <- (1 - gamma_n) s' ;  gc <- gamma_n s' / env
// and alpha_bar_n, beta_bar_n, a and c_prev as above.  Off W, t_n - d_{n-1} = gamma_n (u - d_{n-1}); on W, s' is 0: no u has to be
// recorded.  gc then goes through the projection adjoint at c_prev against m' = where(M, 0, m).  FIRST, t_1 = c_1 = d_1 =
// where(W, off, P(c_0) + off):  s = a + gc + gd ;  goff += s ;  gc <- s' / env.  goff read and written and one mask byte per sample
// beside the transfers above.
#pragma once
#include "common.h"
#include "kernels_agla.h"

namespace specinv {

constexpr int kAglaAdjMaxGrid = 256 * 8;   // workgroups of one launch: as many partial triples at the most

template <typename T>
struct AglaAdjArgs {
  T* a;              // (B, L): cotangent of t_n in, the part of t_{n-1}'s that does not pass through c_{n-1}, d_{n-1} out
  T* gc;             // (B, L): cotangent of c_n in, gamma_n s / env out
  T* gd;             // (B, L): cotangent of d_n in, of d_{n-1} out; the GENERAL kernel alone (nullptr: every gamma is 1)
  const T* tn;       // (B, L): t_n
  const T* tp;       // (B, L): t_{n-1}
  const T* tpp;      // (B, L): t_{n-2}; nullptr for n = 2, where c_1 = d_1 = t_1
  const T* env;      // (L): the window-square envelope
  T* c_prev;         // (B, L): c_{n-1}, what the projection of iteration n read, to rounding
  double* partials;  // (gridDim.x, 3): one triple of partial inner products per workgroup
  T alpha, beta, gamma, one_minus_gamma;   // of iteration n, each rounded to T once
  T alpha_p, beta_p;                       // of iteration n - 1
  int64_t L;
  int64_t upr;       // work items per row: L / V
  int64_t n_units;   // B * upr
  int first;         // the closing step
  // the constraint, read by the CONSTRAINED kernel alone (last: the other kernels see the fields above where they were)
  T* goff;               // (B, L): the cotangent of off, accumulated; nullptr: no constraint
  const uint8_t* mask;   // (B, L): non-zero where the sample is known; nullptr: no sample is
};

// V: consecutive samples per thread, one load / store of V * sizeof(T) bytes each (rows start at multiples of L elements, L % V == 0
// aligns every row).  Grid-stride over (row, V samples); every element of a, gc, gd and c_prev is written by the thread that read
// it.  The inner products: every factor converted to double (delta and t_n - d_{n-1} are formed there from the recorded values),
// multiplied and accumulated in double per thread, summed over the wave by data-parallel-primitive moves (wave_scan_inclusive: lane
// 63 holds the total), over the four waves through LDS in a fixed order - no atomics, one triple per workgroup.
// CONSTRAINED: goff and the mask are read beside the cotangents, the V mask bytes of a thread in one load; the mask pointer is
// uniform, one scalar branch per work item.  Every element of goff is written by the thread that read it.
template <typename T, int V, bool GENERAL, bool CONSTRAINED>
__global__ void __launch_bounds__(256) k_agla_step_adjoint(AglaAdjArgs<T> p) {
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
    Vec go{};
    if constexpr (CONSTRAINED) go = *reinterpret_cast<const Vec*>(p.goff + at);
    Vec gd{};
    if constexpr (GENERAL) gd = *reinterpret_cast<const Vec*>(p.gd + at);
    CglaMask<V> w{};
    if constexpr (CONSTRAINED) {
      if (p.mask != nullptr) w = *reinterpret_cast<const CglaMask<V>*>(p.mask + at);
    }
    if (p.first) {
#pragma unroll
      for (int i = 0; i < V; ++i) {
        T s = a.v[i] + gc.v[i];
        if constexpr (GENERAL) s += gd.v[i];
        if constexpr (CONSTRAINED) {
          go.v[i] += s;
          gc.v[i] = w.v[i] ? T(0) : s / e.v[i];
        } else {
          gc.v[i] = s / e.v[i];
        }
      }
      *reinterpret_cast<Vec*>(p.gc + at) = gc;
      if constexpr (CONSTRAINED) *reinterpret_cast<Vec*>(p.goff + at) = go;
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
      if constexpr (CONSTRAINED) {
        const T sp = w.v[i] ? T(0) : s;                              // s'
        if constexpr (GENERAL) gdn.v[i] = p.one_minus_gamma * sp;
        s_ga += (double)sp * ((double)tn.v[i] - dprev[i]);
        const T through = GENERAL ? p.gamma * sp : sp;               // to u: to the projection and, off W, to off
        go.v[i] += w.v[i] ? s : through;
        gc.v[i] = through / e.v[i];
      } else {
        if constexpr (GENERAL) gdn.v[i] = p.one_minus_gamma * s;
        s_ga += (double)s * ((double)tn.v[i] - dprev[i]);
        gc.v[i] = GENERAL ? p.gamma * s / e.v[i] : s / e.v[i];
      }
    }
    *reinterpret_cast<Vec*>(p.a + at) = an;
    *reinterpret_cast<Vec*>(p.gc + at) = gc;
    if constexpr (GENERAL) *reinterpret_cast<Vec*>(p.gd + at) = gdn;
    if constexpr (CONSTRAINED) *reinterpret_cast<Vec*>(p.goff + at) = go;
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

// Host side (tu_agla_adjoint.hip): picks V (the widest of 16 / 8 / 4 bytes - float64: 16 / 8 - that divides L and the pointers'
// alignment), GENERAL (p.gd != nullptr) and CONSTRAINED (p.goff != nullptr), launches at most kAglaAdjMaxGrid workgroups of 256
// and, unless p.first, the finishing launch (k_agla_dots_finish, one workgroup that sums the partial triples in a fixed order) that
// leaves {alpha_bar, beta_bar, gamma_bar} in dots_dev (3 doubles on the device; beta_bar = 0 without gd).  p.upr and p.n_units are
// filled in here; p.partials holds 3 * kAglaAdjMaxGrid doubles.
template <typename T>
int agla_step_adjoint_launch(AglaAdjArgs<T> p, int batch, double* dots_dev, hipStream_t stream);

}  // namespace specinv
