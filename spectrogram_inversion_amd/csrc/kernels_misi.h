// MISI's coupling step (Multiple Input Spectrogram Inversion, Gunawan & Sen 2010): after every inverse transform the K source
// estimates of a mixture share out what their sum misses of the mixture,
//     e = (mix - sum_k x_k) / K ;   x_k += e,
// on the signal state the next projection launch reads (plan_impl.h: launch_mix) - no round trip through the host layer.
// Memory-bound: (2 K + 1) sizeof(T) bytes per mixture sample (K = 2, 3, 4 keep the K values in registers: one read, one write per
// source; larger K reads the sources twice, 3 K + 1).
#pragma once
#include <initializer_list>

#include "common.h"
#include "fast_core.h"

namespace specinv {

template <typename T>
struct MisiMixArgs {
  T* x;             // (n_mix * K, L): item b * K + k is source k of mixture b; updated in place
  const T* mix;     // (n_mix, L)
  // The float32 fused kernels keep a signal as x plus chunk tails: the first nb hop-blocks of every chunk but the first are two
  // partial sums, the chunk's own frames in x and the previous chunk's last frames in tail[row][c][q][hop] (fast_core.h:
  // load_block adds them on load, kernels_layout.h: k_wave_out for get_wave).  The sum over the sources is that of the whole
  // waveforms, the correction goes to x alone: x + e + tail is what the next launch loads.  nullptr: x is the whole waveform.
  const T* tail;
  int64_t L;
  int64_t upr;      // work items per row: L / V
  int64_t n_units;  // n_mix * upr
  int K;
  int n_frames, nchunks, skew, hop, nb, pb;   // the tails' geometry (fast::chunk_begin, fast::Ovl: HOP, NB, PB)
};

template <typename T, int V>
struct alignas(sizeof(T) * V) MisiVec {
  T v[V];
};

// Host side, the V a launcher takes: the widest of 16 / 8 / 4 bytes (float64: 16 / 8) in samples that divides L, the hop where the
// rows have chunk tails (hop = 0: none) and the address of every pointer in `rows` - every row starts at a multiple of L (hop)
// elements from its base.  `bytes` is an array of one byte per sample (a mask): V bytes per thread.  nullptr is aligned.
template <typename T>
inline int misi_vec_width(int64_t L, int hop, std::initializer_list<const void*> rows, const void* bytes = nullptr) {
  for (int v = sizeof(T) == 4 ? 4 : 2; v > 1; v /= 2) {
    bool ok = L % v == 0 && hop % v == 0 && reinterpret_cast<uintptr_t>(bytes) % v == 0;
    for (const void* p : rows) ok = ok && reinterpret_cast<uintptr_t>(p) % (v * sizeof(T)) == 0;
    if (ok) return v;
  }
  return 1;
}

// Offset of the tail samples that belong to samples n ... n + V - 1 of a row (hop % V == 0, n % V == 0: one hop-block) inside the
// row's nchunks * nb * hop tail entries, -1 where the row's x is the whole value
// (Args: MisiMixArgs, or another kernel's arguments with the same geometry fields - kernels_agla.h)
template <typename Args>
__device__ __forceinline__ int64_t misi_tail_offset(const Args& a, int64_t n) {
  const int blk = (int)(n / a.hop) + a.pb;                          // padded-signal hop-block
  const int smp = (int)(n % a.hop);
  // the chunk c whose frames begin at or before this block (chunks are skewed by a few frames around the even split)
  int c = (int)(((int64_t)blk * a.nchunks) / a.n_frames);
  c = c < a.nchunks - 1 ? c : a.nchunks - 1;
  while (c + 1 < a.nchunks && fast::chunk_begin(c + 1, a.n_frames, a.nchunks, a.skew) <= blk) ++c;
  while (c > 0 && fast::chunk_begin(c, a.n_frames, a.nchunks, a.skew) > blk) --c;
  const int q = blk - fast::chunk_begin(c, a.n_frames, a.nchunks, a.skew);
  if (c < 1 || q >= a.nb) return -1;
  return ((int64_t)(c - 1) * a.nb + q) * a.hop + smp;
}

// KT: K at compile time (2, 3, 4), 0: a run-time loop that reads the sources twice.  V: consecutive samples per thread, one load /
// store of V * sizeof(T) bytes each (16 bytes where L allows: rows start at multiples of L elements, so L % V == 0 is what aligns
// every row; V = 1 takes any L).  Grid-stride over (mixture, V samples).
template <typename T, int KT, int V>
__global__ void __launch_bounds__(256) k_misi_mix(MisiMixArgs<T> a) {
  using Vec = MisiVec<T, V>;
  const int K = KT > 0 ? KT : a.K;
  const T kf = (T)K;
  const int64_t tail_row = (int64_t)a.nchunks * a.nb * a.hop;
  for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < a.n_units; u += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = u / a.upr;
    const int64_t n = (u - b * a.upr) * V;
    const int64_t row0 = b * K;
    const int64_t toff = a.tail != nullptr ? misi_tail_offset(a, n) : -1;
    const Vec m = *reinterpret_cast<const Vec*>(a.mix + b * a.L + n);
    auto whole = [&](int k, Vec w) {                                // source k's waveform at these samples: x (+ tail)
      if (toff >= 0) {
        const Vec t = *reinterpret_cast<const Vec*>(a.tail + (row0 + k) * tail_row + toff);
#pragma unroll
        for (int i = 0; i < V; ++i) w.v[i] += t.v[i];
      }
      return w;
    };
    Vec s{};
    if constexpr (KT > 0) {
      Vec x[KT];
#pragma unroll
      for (int k = 0; k < KT; ++k) x[k] = *reinterpret_cast<const Vec*>(a.x + (row0 + k) * a.L + n);
#pragma unroll
      for (int k = 0; k < KT; ++k) {
        const Vec w = whole(k, x[k]);
#pragma unroll
        for (int i = 0; i < V; ++i) s.v[i] = k == 0 ? w.v[i] : s.v[i] + w.v[i];
      }
#pragma unroll
      for (int k = 0; k < KT; ++k) {
#pragma unroll
        for (int i = 0; i < V; ++i) x[k].v[i] += (m.v[i] - s.v[i]) / kf;
        *reinterpret_cast<Vec*>(a.x + (row0 + k) * a.L + n) = x[k];
      }
    } else {
      for (int k = 0; k < K; ++k) {
        const Vec w = whole(k, *reinterpret_cast<const Vec*>(a.x + (row0 + k) * a.L + n));
#pragma unroll
        for (int i = 0; i < V; ++i) s.v[i] = k == 0 ? w.v[i] : s.v[i] + w.v[i];
      }
      Vec e;
#pragma unroll
      for (int i = 0; i < V; ++i) e.v[i] = (m.v[i] - s.v[i]) / kf;
      for (int k = 0; k < K; ++k) {
        Vec x = *reinterpret_cast<const Vec*>(a.x + (row0 + k) * a.L + n);
#pragma unroll
        for (int i = 0; i < V; ++i) x.v[i] += e.v[i];
        *reinterpret_cast<Vec*>(a.x + (row0 + k) * a.L + n) = x;
      }
    }
  }
}

// Host side (tu_misi.hip): picks KT and V (the widest of 16 / 8 / 4 bytes - float64: 16 / 8 - that divides L; with tails also the
// hop) and launches at most 2048 workgroups of 256.  a.upr and a.n_units are filled in here.
template <typename T>
int misi_mix_launch(MisiMixArgs<T> a, int n_mix, hipStream_t stream);

}  // namespace specinv
