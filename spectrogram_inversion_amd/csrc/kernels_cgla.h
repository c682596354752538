// The extrapolation step of Accelerated Griffin-Lim under constraints (constrained_griffin_lim): known bins of the
// spectrogram and known samples of the signal.  The STFT is linear, so the amplitude projection with the known bins K under the
// mask M put in, ISTFT(where(M, K, S m / (|S| + 1e-16))), is the projection launch with zeros in its magnitude operand under M
// plus the constant signal k = ISTFT(where(M, K, 0)); a known sample is one more select on the same signal.  After every
// projection launch has left y = P_m'(c_{n-1}) on the signal state, with offset = where(W, xk, k) made once by the host layer,
//     u = y + offset ;   t_n = where(W, offset, (1 - gamma) d_{n-1} + gamma u) ;
//     c_n = t_n + alpha (t_n - t_{n-1}) ;   d_n = t_n + beta (t_n - t_{n-1}),
// c_n written back to the state the next projection launch reads.  The select acts on t_n: from t_1 on the difference is exactly 0
// at a known sample, so t, c and d hold xk there bit for bit.  Memory-bound: 5 transfers of sizeof(T) per sample with gamma = 1
// (x and t read and written, offset read), 7 in general, plus one mask byte and the read of a chunk tail where there is one.
#pragma once
#include "kernels_agla.h"

namespace specinv {

template <typename T>
struct CglaStepArgs {
  T* x;             // (B, L): y (less the tail) on entry, c_n (less the tail) on return - AglaStepArgs::x
  T* t;             // (B, L): t_{n-1} on entry, t_n on return - the method's result
  T* d;             // (B, L): d_{n-1} / d_n; the GENERAL kernel alone (nullptr with gamma = 1)
  const T* offset;  // (B, L): the known sample under the mask, the known bins' signal k elsewhere
  const uint8_t* mask;   // (B, L): non-zero where the sample is known; nullptr: no sample is
  const T* tail;    // the chunk tails of the float32 fused kernels (AglaStepArgs::tail), nullptr: x is the whole waveform
  T alpha, beta, gamma, one_minus_gamma;   // each rounded to T once
  int64_t L;
  int64_t upr;      // work items per row: L / V
  int64_t n_units;  // B * upr
  int first;        // n = 1, no history yet: t = d = c_1 = where(W, offset, y + offset)
  int n_frames, nchunks, skew, hop, nb, pb;   // the tails' geometry, the fields misi_tail_offset reads
};

template <int V>
struct alignas(V) CglaMask {
  uint8_t v[V];
};

// V, GENERAL and the walk are k_agla_step's; the V mask bytes of a thread are one load.  The mask pointer is uniform: one scalar
// branch per work item.  With tails y = x + tail on entry and x = c_n - tail on return on both arms (t_n is no longer x + tail
// where an offset was added or a sample selected); the first iteration writes x as well, c_1 = t_1 differs from y.
template <typename T, int V, bool GENERAL>
__global__ void __launch_bounds__(256) k_cgla_step(CglaStepArgs<T> a) {
  using Vec = MisiVec<T, V>;
  const int64_t tail_row = (int64_t)a.nchunks * a.nb * a.hop;
  for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < a.n_units; u += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = u / a.upr;
    const int64_t n = (u - b * a.upr) * V;
    const int64_t at = b * a.L + n;
    const int64_t toff = a.tail != nullptr ? misi_tail_offset(a, n) : -1;
    Vec y = *reinterpret_cast<const Vec*>(a.x + at), tl{};
    const Vec off = *reinterpret_cast<const Vec*>(a.offset + at);
    CglaMask<V> w{};
    if (a.mask != nullptr) w = *reinterpret_cast<const CglaMask<V>*>(a.mask + at);
    if (toff >= 0) {
      tl = *reinterpret_cast<const Vec*>(a.tail + b * tail_row + toff);
#pragma unroll
      for (int i = 0; i < V; ++i) y.v[i] += tl.v[i];
    }
    Vec tn, c, dn;
#pragma unroll
    for (int i = 0; i < V; ++i) tn.v[i] = y.v[i] + off.v[i];         // u, rounded before the relaxation
    if (a.first) {
#pragma unroll
      for (int i = 0; i < V; ++i) {
        tn.v[i] = w.v[i] ? off.v[i] : tn.v[i];
        c.v[i] = tn.v[i] - tl.v[i];
      }
      *reinterpret_cast<Vec*>(a.t + at) = tn;
      if constexpr (GENERAL) *reinterpret_cast<Vec*>(a.d + at) = tn;
      *reinterpret_cast<Vec*>(a.x + at) = c;
      continue;
    }
    const Vec tp = *reinterpret_cast<const Vec*>(a.t + at);
    if constexpr (GENERAL) {
      const Vec dp = *reinterpret_cast<const Vec*>(a.d + at);
#pragma unroll
      for (int i = 0; i < V; ++i) tn.v[i] = a.one_minus_gamma * dp.v[i] + a.gamma * tn.v[i];
    }
#pragma unroll
    for (int i = 0; i < V; ++i) {
      tn.v[i] = w.v[i] ? off.v[i] : tn.v[i];
      const T diff = tn.v[i] - tp.v[i];
      c.v[i] = tn.v[i] + a.alpha * diff - tl.v[i];
      if constexpr (GENERAL) dn.v[i] = tn.v[i] + a.beta * diff;
    }
    *reinterpret_cast<Vec*>(a.t + at) = tn;
    if constexpr (GENERAL) *reinterpret_cast<Vec*>(a.d + at) = dn;
    *reinterpret_cast<Vec*>(a.x + at) = c;
  }
}

// Host side (tu_cgla.hip): picks V (the widest of 16 / 8 / 4 bytes - float64: 16 / 8 - that divides L; with tails also the hop)
// and GENERAL (a.d != nullptr), launches at most 2048 workgroups of 256.  a.upr and a.n_units are filled in here.
template <typename T>
int cgla_step_launch(CglaStepArgs<T> a, int batch, hipStream_t stream);

}  // namespace specinv
