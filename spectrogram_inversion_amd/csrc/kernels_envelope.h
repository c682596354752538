// Spectral envelope: the true-envelope estimator of Roebel & Rodet 2005 over a one-sided spectrogram, one launch.
//   Per item and frame, N = n_fft, F = N / 2 + 1 bins:
//     a0[k] = log(max(|S[k]|, amin))                       amin = floor * max |S| over the item (the caller's (B,) array);
//                                                          amin <= 0 (an all-zero item): a0 = 0, so V = 0 and E = 1
//     C(a)  = Re rfft(irfft(a, N) * l),  l[q] = 1 if min(q, N - q) <= order else 0
//     V_0 = C(a0),  V_i = C(max(a0, V_{i-1})), i = 1 ... n_iter,   E = exp(V_{n_iter})
//   n_iter is a count, not a stop rule.  float32 throughout; a complex input's magnitude is hypotf.
//
// Transform.  a is real and read as an even sequence of length N, so its cepstrum is real and even and so is C(a).  A complex
// N-point transform of a_A + i a_B therefore carries two frames, one in the real and one in the imaginary parts, in both
// directions, with no untangling pass: a wave owns a PAIR of frames and runs fast_core.h's wave-level FFT with M = N complex
// points, R = N / 64 per lane (N = 256, 512, 1024, 2048 <-> R = 4, 8, 16, 32).  Lane l, register u holds point 64 u + l on both
// sides of either transform, so the lifter is a predicate on that index and the 1 / N goes with it (a power of two: exact).
// The odd last frame of a tile pairs with a row of zeros.
//
// Layout.  The public layout is (B, F, T): a frame is a strided column.  A workgroup of four waves takes a tile of TT consecutive
// frames of one item (TT = 32 up to n_fft 512, 16 at 1024, 8 at 2048: about 32 KiB of float32 either way) and stages it as
// tile[t][f] in LDS, log-magnitude taken on the way in.  The global loads run along T, TT lanes to a row; the row stride of the
// image is N / 2 + 32 / TT, which puts the TT x (32 / TT) elements a 32-lane write group stores on 32 banks.  frame_major
// ((B, T, F)) loads rows along F instead and needs no transpose.  The tile IS the resident a0: a wave reads its two rows for the
// first transform and for every max (stride 1 along the lanes, mirrored above N / 2: no bank conflict), and overwrites them with
// V at the end - no other wave reads those rows.  After a barrier the tile goes out the way it came in, exp taken on the way.
// Nothing touches global memory between the load and the store.
//
// LDS: pass-1 twiddles (R - 1) x 64, four transpose scratches of Geo<R>::TR, the tile - 31 / 56 / 75 / 116 KiB for R = 4 ... 32,
// so five / two / two / one workgroup per CU.  All loops are bounded by TT, F and n_iter; offsets into global memory are 64-bit.
#pragma once
#include "fast_core.h"

namespace specinv {

constexpr int kEnvWaves = 4;
constexpr int kEnvThreads = 64 * kEnvWaves;
constexpr int kEnvMaxIter = 256;

struct EnvArgs {
  const float* spec;   // (B, F, T) or (B, T, F); (re, im) pairs for a complex input
  float* out;          // the same layout, real
  const float* amin;   // (B,)
  int64_t tiles_t;     // workgroups per item
  int n_frames;
  int order, n_iter;
  int out_log;         // 1: V, 0: E = exp(V)
  int frame_major;
};

template <int R>
struct EnvGeo {
  static constexpr int N = 64 * R;                 // n_fft = the transform's complex points
  static constexpr int F = N / 2 + 1;
  static constexpr int TT = R <= 8 ? 32 : R == 16 ? 16 : 8;   // frames per workgroup (even: whole pairs)
  static constexpr int STRIDE = N / 2 + 32 / TT;   // floats per staged frame (>= F)
  static constexpr int TABLES = (R - 1) * 64 + kEnvWaves * fast::Geo<R>::TR;   // v2f elements ahead of the tile
  static constexpr size_t lds_bytes() { return sizeof(fast::v2f) * (size_t)TABLES + sizeof(float) * (size_t)TT * STRIDE; }
  static_assert(STRIDE >= F && TT % 2 == 0 && kEnvThreads % TT == 0, "tile geometry");
};

template <bool CPLX>
__device__ __forceinline__ float env_log_mag(const float* __restrict__ spec, int64_t at, float amin) {
  float m;
  if constexpr (CPLX) m = hypotf(spec[2 * at], spec[2 * at + 1]);
  else m = spec[at];
  return amin > 0.0f ? logf(fmaxf(m, amin)) : 0.0f;
}

template <int R, bool CPLX>
__global__ void __launch_bounds__(kEnvThreads) k_spectral_envelope(EnvArgs a, int64_t block0) {
  using namespace fast;
  using G = Geo<R>;
  using E = EnvGeo<R>;
  constexpr int N = E::N, F = E::F, TT = E::TT, STRIDE = E::STRIDE;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  v2f* lds_tw1 = reinterpret_cast<v2f*>(smem);
  const int tid = threadIdx.x;
  const int wib = __builtin_amdgcn_readfirstlane(tid >> 6);
  v2f* tr = lds_tw1 + (R - 1) * 64 + wib * G::TR;
  float* tile = reinterpret_cast<float*>(lds_tw1 + E::TABLES);

  for (int i = tid; i < (R - 1) * 64; i += kEnvThreads) {
    const int k1 = i / 64 + 1, l = i & 63;
    lds_tw1[i] = unit(2.0f * (float)((l * k1) % N) / (float)N);
  }

  const int64_t blk = block0 + blockIdx.x;
  const int64_t item = blk / a.tiles_t;
  const int t0 = (int)(blk - item * a.tiles_t) * TT;
  const int nt = a.n_frames - t0 < TT ? a.n_frames - t0 : TT;      // frames of this tile, >= 1
  const float amin = a.amin[item];
  const int64_t base = item * F * (int64_t)a.n_frames;

  // ---- stage the tile: tile[t * STRIDE + f] = a0 of frame t0 + t, zeros for the frames beyond T
  if (a.frame_major) {
    for (int t = wib; t < TT; t += kEnvWaves)
      for (int f = tid & 63; f < F; f += 64)
        tile[t * STRIDE + f] = t < nt ? env_log_mag<CPLX>(a.spec, base + (int64_t)(t0 + t) * F + f, amin) : 0.0f;
  } else {
    const int t = tid % TT;
    for (int f = tid / TT; f < F; f += kEnvThreads / TT)
      tile[t * STRIDE + f] = t < nt ? env_log_mag<CPLX>(a.spec, base + (int64_t)f * a.n_frames + t0 + t, amin) : 0.0f;
  }
  __syncthreads();

  // ---- a pair of frames per wave: every iteration in registers, a0 read from the tile
  const LaneConst<R> k = lane_consts<R>();
  const int lane = k.lane;
  const float inv_n = 1.0f / (float)N;
  for (int p = wib; 2 * p < nt; p += kEnvWaves) {
    float* rowa = tile + 2 * p * STRIDE;
    float* rowb = rowa + STRIDE;
    v2f z[R];
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const int n = 64 * u + lane, f = n <= N / 2 ? n : N - n;
      z[u] = v2f{rowa[f], rowb[f]};
    }
    for (int it = 0;; ++it) {
      fft_inverse<R>(z, k, lds_tw1, tr);
#pragma unroll
      for (int u = 0; u < R; ++u) {
        const int q = 64 * u + lane, qs = q <= N / 2 ? q : N - q;
        const float l = qs <= a.order ? inv_n : 0.0f;
        z[u] = z[u] * l;
      }
      fft_forward<R>(z, k, lds_tw1, tr);
      if (it == a.n_iter) break;
#pragma unroll
      for (int u = 0; u < R; ++u) {
        const int n = 64 * u + lane, f = n <= N / 2 ? n : N - n;
        z[u] = v2f{fmaxf(rowa[f], z[u].x), fmaxf(rowb[f], z[u].y)};
      }
    }
    // V over a0: bins 0 ... N / 2 are registers 0 ... R / 2 - 1 of every lane and register R / 2 of lane 0
#pragma unroll
    for (int u = 0; u <= R / 2; ++u) {
      const int n = 64 * u + lane;
      if (n <= N / 2) {
        rowa[n] = z[u].x;
        rowb[n] = z[u].y;
      }
    }
  }
  __syncthreads();

  // ---- the tile goes out the way it came in
  if (a.frame_major) {
    for (int t = wib; t < nt; t += kEnvWaves)
      for (int f = tid & 63; f < F; f += 64) {
        const float v = tile[t * STRIDE + f];
        a.out[base + (int64_t)(t0 + t) * F + f] = a.out_log ? v : expf(v);
      }
  } else {
    const int t = tid % TT;
    if (t < nt)
      for (int f = tid / TT; f < F; f += kEnvThreads / TT) {
        const float v = tile[t * STRIDE + f];
        a.out[base + (int64_t)f * a.n_frames + t0 + t] = a.out_log ? v : expf(v);
      }
  }
}

}  // namespace specinv
