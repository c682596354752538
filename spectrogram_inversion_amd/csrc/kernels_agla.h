// The extrapolation step of Accelerated Griffin-Lim (AGLA; Peer, Welker & Gerkmann 2022 - with gamma = 1 the Fast Griffin-Lim of
// Perraudin, Balazs & Soendergaard 2013).  All three of its sequences are consistent spectrograms once the first projection has
// run and the STFT is linear, so they are carried as signals of L samples: after every projection launch has left y = P(c_{n-1})
// on the signal state,
//     t_n = (1 - gamma) d_{n-1} + gamma y ;   c_n = t_n + alpha (t_n - t_{n-1}) ;   d_n = t_n + beta (t_n - t_{n-1}),
// c_n written back to the state the next projection launch reads (plan_impl.h: launch_agla).  Memory-bound: 4 transfers of
// sizeof(T) per sample with gamma = 1 (x and t read and written; d is neither allocated nor touched), 6 in general, plus the
// read of a chunk tail where there is one.
//
// Under constraints (constrained_griffin_lim) - known bins of the spectrogram and known samples of the signal - the
// amplitude projection with the known bins K under the mask M put in, ISTFT(where(M, K, S m / (|S| + 1e-16))), is the projection
// launch with zeros in its magnitude operand under M plus the constant signal k = ISTFT(where(M, K, 0)); a known sample is one more
// select on the same signal.  With offset = where(W, xk, k) made once by the host layer,
//     u = y + offset ;   t_n = where(W, offset, (1 - gamma) d_{n-1} + gamma u) ;   c_n, d_n as above.
// The select acts on t_n: from t_1 on the difference is exactly 0 at a known sample, so t, c and d hold xk there bit for bit.  One
// more transfer per sample (offset read) and one mask byte.
#pragma once
#include "common.h"
#include "fast_core.h"
#include "kernels_misi.h"

namespace specinv {

template <typename T>
struct AglaStepArgs {
  T* x;             // (B, L): the rows the next projection launch reads, y on entry, c_n (less the tail) on return
  T* t;             // (B, L): t_{n-1} on entry, t_n on return - the method's result
  T* d;             // (B, L): d_{n-1} / d_n; read and written by the GENERAL kernel alone (nullptr with gamma = 1)
  // The float32 fused kernels keep a signal as x plus chunk tails (kernels_misi.h: MisiMixArgs::tail): y = x + tail, and
  // x = c_n - tail (with gamma = 1: x + alpha (t_n - t_{n-1}), the tail never subtracted) makes x + tail again what the next
  // launch loads.  nullptr: x is the whole waveform.
  const T* tail;
  T alpha, beta, gamma, one_minus_gamma;   // each rounded to T once
  int64_t L;
  int64_t upr;      // work items per row: L / V
  int64_t n_units;  // B * upr
  int first;        // n = 1, no history yet: t = d = y, x stays (c_1 = y); CONSTRAINED: t = d = c_1 = where(W, offset, y + offset)
  int n_frames, nchunks, skew, hop, nb, pb;   // the tails' geometry, the fields misi_tail_offset reads
  // the constraint, read by the CONSTRAINED kernel alone (last: the other kernels see the fields above where they were)
  const T* offset;       // (B, L): the known sample under the mask, the known bins' signal k elsewhere; nullptr: no constraint
  const uint8_t* mask;   // (B, L): non-zero where the sample is known; nullptr: no sample is
};

template <int V>
struct alignas(V) CglaMask {
  uint8_t v[V];
};

// V: consecutive samples per thread, one load / store of V * sizeof(T) bytes each (kernels_misi.h: rows start at multiples of L
// elements, L % V == 0 aligns every row; with tails hop % V == 0 keeps the V samples in one hop-block).  GENERAL: gamma != 1.
// Grid-stride over (row, V samples); t and d are updated in place by the thread that read them.
// CONSTRAINED: offset and the mask are read beside x, the V mask bytes of a thread in one load; the mask pointer is uniform, one
// scalar branch per work item.  The two schemes round differently and stay apart: with a constraint t_n is no longer x + tail, so
// c_n - tail is formed from t_n on both arms and the first iteration writes x as well (c_1 = t_1 differs from y).
template <typename T, int V, bool GENERAL, bool CONSTRAINED>
__global__ void __launch_bounds__(256) k_agla_step(AglaStepArgs<T> a) {
  using Vec = MisiVec<T, V>;
  const int64_t tail_row = (int64_t)a.nchunks * a.nb * a.hop;
  for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < a.n_units; u += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = u / a.upr;
    const int64_t n = (u - b * a.upr) * V;
    const int64_t at = b * a.L + n;
    const int64_t toff = a.tail != nullptr ? misi_tail_offset(a, n) : -1;
    const Vec xv = *reinterpret_cast<const Vec*>(a.x + at);
    Vec y = xv, tl{}, off{};
    CglaMask<V> w{};
    if constexpr (CONSTRAINED) {
      off = *reinterpret_cast<const Vec*>(a.offset + at);
      if (a.mask != nullptr) w = *reinterpret_cast<const CglaMask<V>*>(a.mask + at);
    }
    if (toff >= 0) {
      tl = *reinterpret_cast<const Vec*>(a.tail + b * tail_row + toff);
#pragma unroll
      for (int i = 0; i < V; ++i) y.v[i] += tl.v[i];
    }
    if constexpr (CONSTRAINED) {
#pragma unroll
      for (int i = 0; i < V; ++i) y.v[i] += off.v[i];                // u, rounded before the relaxation
    }
    if (a.first) {
      if constexpr (CONSTRAINED) {
        Vec c;
#pragma unroll
        for (int i = 0; i < V; ++i) {
          y.v[i] = w.v[i] ? off.v[i] : y.v[i];
          c.v[i] = y.v[i] - tl.v[i];
        }
        *reinterpret_cast<Vec*>(a.x + at) = c;
      }
      *reinterpret_cast<Vec*>(a.t + at) = y;
      if constexpr (GENERAL) *reinterpret_cast<Vec*>(a.d + at) = y;
      continue;
    }
    const Vec tp = *reinterpret_cast<const Vec*>(a.t + at);
    Vec tn = y, c, dn;
    if constexpr (GENERAL) {
      const Vec dp = *reinterpret_cast<const Vec*>(a.d + at);
      // (tn holds y here, one value under two names: which one is read decides which of the two products the compiler rounds
      // when it contracts the sum at V = 1, and each scheme keeps the choice of the kernel it came from -
      // tests/test_gpu_agla_step_bits.py)
#pragma unroll
      for (int i = 0; i < V; ++i) tn.v[i] = a.one_minus_gamma * dp.v[i] + a.gamma * (CONSTRAINED ? tn.v[i] : y.v[i]);
    }
#pragma unroll
    for (int i = 0; i < V; ++i) {
      if constexpr (CONSTRAINED) tn.v[i] = w.v[i] ? off.v[i] : tn.v[i];
      const T diff = tn.v[i] - tp.v[i];
      if constexpr (CONSTRAINED) {
        c.v[i] = tn.v[i] + a.alpha * diff - tl.v[i];
      } else if constexpr (GENERAL) {
        c.v[i] = tn.v[i] + a.alpha * diff;
      } else {
        // t_n = y = x + tail: c_n - tail is x + alpha (t_n - t_{n-1}) - no cancellation against the tail, alpha = 0 leaves x's bits
        c.v[i] = xv.v[i] + a.alpha * diff;
      }
      if constexpr (GENERAL) dn.v[i] = tn.v[i] + a.beta * diff;
      if constexpr (GENERAL && !CONSTRAINED) {
        if (toff >= 0) c.v[i] -= tl.v[i];                            // (after d_n, where it stood: the float32 V = 4 schedule)
      }
    }
    *reinterpret_cast<Vec*>(a.t + at) = tn;
    if constexpr (GENERAL) *reinterpret_cast<Vec*>(a.d + at) = dn;
    *reinterpret_cast<Vec*>(a.x + at) = c;
  }
}

// Host side (tu_agla.hip): picks V (the widest of 16 / 8 / 4 bytes - float64: 16 / 8 - that divides L; with tails also the hop)
// and the pointers' alignment, GENERAL (a.d != nullptr) and CONSTRAINED (a.offset != nullptr), launches at most 2048 workgroups of
// 256.  a.upr and a.n_units are filled in here.
template <typename T>
int agla_step_launch(AglaStepArgs<T> a, int batch, hipStream_t stream);

}  // namespace specinv
