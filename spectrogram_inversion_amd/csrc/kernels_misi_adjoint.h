// The two element-wise kernels of MISI's backward sweep (misi_unfolded).  One unfolded iteration is
//     x_n = M(B(m * A x_{n-1} / (|A x_{n-1}| + 1e-16))) ,   M(y)_k = y_k + (mix - sum_j y_j) / K ,
// A the STFT, B the ISTFT.  Its adjoint, on the cotangent g of x_n:
//     c = (1/K) sum_k g_k ;  gmix += c ;  u_k = (g_k - c) / env                      k_misi_mix_adjoint  (M^T, B^T's division)
//     Y = unscaled forward DFT of the zero-padded frames of u                        stft_internal
//     R = A x_{n-1}                                                                  stft_internal (recomputed, never stored)
//     gQ = inv_scale (interior ? 2 Y : Re Y) ;  d = |R| + 1e-16 ;  dot = Re(conj(gQ) R)
//     gm += dot / d ;  gR = gQ m/d - R (|R| > 0 ? dot m/(d^2 |R|) : 0) ;  halve the interior bins
//                                                                                    k_misi_proj_adjoint (three passes in one)
//     g = A^T gR                                                                     grad_from_spec
// Both kernels are memory-bound and work on plain rows: no LDS, no chunk tails (backward buffers are whole waveforms).
#pragma once
#include "common.h"
#include "kernels_misi.h"

namespace specinv {

template <typename T>
struct MisiMixAdjArgs {
  T* g;             // (n_mix * K, L): the cotangents of the K sources of every mixture; g_k - c (/ env) in place
  T* gmix;          // (n_mix, L): c is added - element (b, n) has exactly one writer
  const T* env;     // (L): the window-square envelope (DIV_ENV only)
  int64_t L;
  int64_t upr;      // work items per row: L / V
  int64_t n_units;  // n_mix * upr
  int K;
};

// The adjoint of k_misi_mix's x_k += (mix - sum_j x_j) / K with respect to x and mix, the envelope division of the ISTFT's adjoint
// folded in where DIV_ENV.  KT, V: k_misi_mix's scheme (K = 2, 3, 4 in registers, 0: a run-time loop that reads g twice; V samples
// per thread in one load / store, L % V == 0).  (2 K + 2) sizeof(T) bytes per mixture sample, 3 K + 2 in the loop form; the
// envelope's L values stay in the caches.  Grid-stride over (mixture, V samples).
template <typename T, int KT, int V, bool DIV_ENV>
__global__ void __launch_bounds__(256) k_misi_mix_adjoint(MisiMixAdjArgs<T> a) {
  using Vec = MisiVec<T, V>;
  const int K = KT > 0 ? KT : a.K;
  const T kf = (T)K;
  for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < a.n_units; u += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = u / a.upr;
    const int64_t n = (u - b * a.upr) * V;
    const int64_t row0 = b * K;
    Vec e{};
    if constexpr (DIV_ENV) e = *reinterpret_cast<const Vec*>(a.env + n);
    Vec c = *reinterpret_cast<const Vec*>(a.gmix + b * a.L + n);
    Vec s{};
    if constexpr (KT > 0) {
      Vec g[KT];
#pragma unroll
      for (int k = 0; k < KT; ++k) g[k] = *reinterpret_cast<const Vec*>(a.g + (row0 + k) * a.L + n);
#pragma unroll
      for (int k = 0; k < KT; ++k) {
#pragma unroll
        for (int i = 0; i < V; ++i) s.v[i] = k == 0 ? g[k].v[i] : s.v[i] + g[k].v[i];
      }
#pragma unroll
      for (int i = 0; i < V; ++i) {
        s.v[i] /= kf;
        c.v[i] += s.v[i];
      }
#pragma unroll
      for (int k = 0; k < KT; ++k) {
#pragma unroll
        for (int i = 0; i < V; ++i) {
          g[k].v[i] -= s.v[i];
          if constexpr (DIV_ENV) g[k].v[i] /= e.v[i];
        }
        *reinterpret_cast<Vec*>(a.g + (row0 + k) * a.L + n) = g[k];
      }
    } else {
      for (int k = 0; k < K; ++k) {
        const Vec g = *reinterpret_cast<const Vec*>(a.g + (row0 + k) * a.L + n);
#pragma unroll
        for (int i = 0; i < V; ++i) s.v[i] = k == 0 ? g.v[i] : s.v[i] + g.v[i];
      }
#pragma unroll
      for (int i = 0; i < V; ++i) {
        s.v[i] /= kf;
        c.v[i] += s.v[i];
      }
      for (int k = 0; k < K; ++k) {
        Vec g = *reinterpret_cast<const Vec*>(a.g + (row0 + k) * a.L + n);
#pragma unroll
        for (int i = 0; i < V; ++i) {
          g.v[i] -= s.v[i];
          if constexpr (DIV_ENV) g.v[i] /= e.v[i];
        }
        *reinterpret_cast<Vec*>(a.g + (row0 + k) * a.L + n) = g;
      }
    }
    *reinterpret_cast<Vec*>(a.gmix + b * a.L + n) = c;
  }
}

template <typename T>
struct MisiProjAdjArgs {
  cplx<T>* y;           // (B T, F) frame-major: Y in, the halved gR out
  const cplx<T>* r;     // (B T, F): R = A x_{n-1}
  const T* m;           // (B T, F): the target magnitude, frame-major
  T* gm;                // (B T, F): its cotangent, accumulated
  int64_t total;        // B T F
  int F, n_fft, onesided;
  T inv_scale;
};

// k_istft_adjoint_scale, k_gla_update_adjoint at lr = 0 and k_halve_interior (kernels_adjoint.h) in one pass over the frame-major
// arrays, the same operations in the same order: reads Y, R, m and gm, writes gR over Y and gm - 3 complex + 3 real values per bin
// (36 bytes in float32) where the three kernels and their two layout transposes move 12 complex + 3 real (108).
template <typename T>
__global__ void __launch_bounds__(256) k_misi_proj_adjoint(MisiProjAdjArgs<T> a) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.total; i += (int64_t)gridDim.x * blockDim.x) {
    const int f = (int)(i % a.F);
    const bool interior = a.onesided && f != 0 && 2 * f != a.n_fft;
    cplx<T> g = a.y[i];
    if (!a.onesided) g = mk<T>(g.x * a.inv_scale, g.y * a.inv_scale);
    else if (interior) g = mk<T>(g.x * (2 * a.inv_scale), g.y * (2 * a.inv_scale));
    else g = mk<T>(g.x * a.inv_scale, T(0));
    const cplx<T> s = a.r[i];
    const T m = a.m[i];
    const T mag = si_hypot(s.x, s.y);
    const T d = mag + eps16<T>::value;
    const T dot = g.x * s.x + g.y * s.y;                     // Re(conj(gQ) R)
    const T c1 = m / d;
    const T c2 = mag > T(0) ? dot * m / (d * d * mag) : T(0);
    cplx<T> gr = mk<T>(g.x * c1 - s.x * c2, g.y * c1 - s.y * c2);
    if (interior) gr = mk<T>(gr.x * T(0.5), gr.y * T(0.5));
    a.y[i] = gr;
    a.gm[i] += dot / d;
  }
}

// Host side (tu_misi_adjoint.hip).  The mix adjoint picks KT and V like misi_mix_launch (the widest of 16 / 8 / 4 bytes - float64:
// 16 / 8 - that divides L and the pointers' alignment) and DIV_ENV from a.env; both launch at most 2048 workgroups of 256.
template <typename T>
int misi_mix_adjoint_launch(MisiMixAdjArgs<T> a, int n_mix, hipStream_t stream);
template <typename T>
int misi_proj_adjoint_launch(MisiProjAdjArgs<T> a, hipStream_t stream);

}  // namespace specinv
