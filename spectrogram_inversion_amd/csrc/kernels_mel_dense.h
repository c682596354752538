// The kernel chain of the L_BFGS objective (reference: torch_specinv/methods.py:509-569): what runs where the one-launch
// kernels (kernels_objective.h, kernels_objective_walk.h) do not cover a configuration.
//
//   * transform forward  V = |STFT(x)|  or  V = log1p(Mel @ |STFT(x)|)
//   * loss = mean((V - target)^2) and its analytic gradient w.r.t. x (verified against
//     autograd): dV = 2(V-T)/numel ; dMel = dV/(1 + Mel|S|) ; dA = Mel^T dMel ; G = dA * S/|S|
//     (0 where |S| = 0) ; frame gradient = Re sum_k G[k] e^{+2 pi i k n/N} (onesided: interior bins
//     halved, then Hermitian inverse) * window ; overlap-add without envelope ; padded margins folded
//     back according to the pad mode.
//   * the two mel contractions are dense GEMMs and run on the matrix cores with the exact-float32 MFMA
//     (v_mfma_f32_32x32x2_f32, bitwise an fmaf chain) - the only MFMA use in the library.
#pragma once
#include "common.h"
#include "kernels_generic.h"

namespace specinv {

// ---- mel contractions on the matrix cores ----------------------------------------------------------------
// One wave owns a 32 x 32 output tile and feeds v_mfma_f32_32x32x2_f32 (A: lane l holds A[l&31][l>>5],
// B: lane l holds B[l>>5][l&31]; C/D: col = l&31, row = (r&3) + 8*(r>>2) + 4*(l>>5)).  Operands are staged
// through LDS in 32 x 32 tiles with a one-dword row pad (conflict-free column reads).
using f32x16 = float __attribute__((ext_vector_type(16)));

__device__ inline f32x16 mfma_32x32x2(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

// mm[bt, m] = sum_f Mel[m, f] * |S[bt, f]|  ->  V = log1p(mm).   S: (BT, F) complex, Mel: (n_mels, F).
// grid (ceil(BT/32), ceil(n_mels/32)), one wave per block.  Float32 only.
static __global__ __launch_bounds__(64) void k_mel_forward_mfma(const cplx<float>* __restrict__ spec, const float* __restrict__ mel,
                                                         float* __restrict__ mm_out, int64_t BT, int F, int n_mels) {
  __shared__ float sa[32][33];   // Mel tile  [m][k]
  __shared__ float sb[32][33];   // |S| tile  [bt][k]
  const int lane = threadIdx.x;
  const int64_t bt0 = (int64_t)blockIdx.x * 32;
  const int m0 = blockIdx.y * 32;
  f32x16 acc = {0};
  for (int k0 = 0; k0 < F; k0 += 32) {
    // 32 x 32 tiles, 16 elements per lane, rows contiguous in k (coalesced 128-byte rows)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int r = i * 2 + (lane >> 5), c = lane & 31;
      const int k = k0 + c;
      float va = 0.f, vb = 0.f;
      if (k < F) {
        if (m0 + r < n_mels) va = mel[(int64_t)(m0 + r) * F + k];
        if (bt0 + r < BT) {
          const cplx<float> s = spec[(bt0 + r) * F + k];
          vb = hypotf(s.x, s.y);
        }
      }
      sa[r][c] = va;
      sb[r][c] = vb;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 32; kk += 2) {
      const float a = sa[lane & 31][kk + (lane >> 5)];
      const float b = sb[lane & 31][kk + (lane >> 5)];
      acc = mfma_32x32x2(a, b, acc);
    }
    __syncthreads();
  }
  // D[row = m][col = bt]
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    const int col = lane & 31;
    if (m0 + row < n_mels && bt0 + col < BT) mm_out[(bt0 + col) * n_mels + m0 + row] = acc[r];
  }
}

// Same contraction, one workgroup per 32 frames and ALL mel rows (MT tiles of 32): the spectrum - the large operand -
// is read once.  The four waves split K (wave w takes the k-steps w, w+4, ...), each with wave-private LDS tiles
// (no workgroup barrier inside the K loop: the LDS queue of a wave is in order), and add their accumulators through
// LDS at the end.  The filterbank is read from a copy tiled per k-step as [k][m] (zero padded to 32 k x MT*32 m,
// k_mel_tile): one k-step is MT*4 KB of contiguous, 16-byte aligned data - 16-byte loads, 16-byte LDS stores, and
// conflict-free operand reads (consecutive m in consecutive lanes).  The |S| tile is kept [k][bt] with a padded row
// for the same reason.  The next k-step's spectrum values are fetched before the MFMA block of the current one.
template <int MT>
__global__ __launch_bounds__(256) void k_mel_forward_splitk(const cplx<float>* __restrict__ spec,
                                                            const float* __restrict__ mel_tiled, float* __restrict__ mm_out,
                                                            int64_t BT, int F, int n_mels) {
  using f4 = float __attribute__((ext_vector_type(4)));
  constexpr int MW = MT * 32;                      // mel rows per k
  extern __shared__ __attribute__((aligned(16))) float mel_smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* sa = mel_smem + (size_t)wave * (32 * MW + 32 * 33);   // Mel tile [k][m]
  float* sb = sa + 32 * MW;                                    // |S| tile [k][bt], row stride 33
  const int64_t bt0 = (int64_t)blockIdx.x * 32;
  f32x16 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = f32x16{0};
  const int ksteps = (F + 31) / 32;
  const int c = lane & 31, rh = lane >> 5;

  cplx<float> sv[16];
  auto fetch = [&](int ks) {
    const int k = ks * 32 + c;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int r = i * 2 + rh;
      sv[i] = (k < F && bt0 + r < BT) ? spec[(bt0 + r) * F + k] : mk<float>(0.f, 0.f);
    }
  };
  if (wave < ksteps) fetch(wave);
  for (int ks = wave; ks < ksteps; ks += 4) {
    const f4* mg = reinterpret_cast<const f4*>(mel_tiled + (size_t)ks * 32 * MW);
    f4 mv[MT * 4];
#pragma unroll
    for (int i = 0; i < MT * 4; ++i) mv[i] = mg[i * 64 + lane];
#pragma unroll
    for (int i = 0; i < 16; ++i) sb[c * 33 + i * 2 + rh] = __builtin_amdgcn_sqrtf(fmaf(sv[i].x, sv[i].x, sv[i].y * sv[i].y));
#pragma unroll
    for (int i = 0; i < MT * 4; ++i) reinterpret_cast<f4*>(sa)[i * 64 + lane] = mv[i];
    if (ks + 4 < ksteps) fetch(ks + 4);                  // in flight during the MFMA block
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's tiles are in LDS (and the compiler keeps the order)
#pragma unroll
    for (int kk = 0; kk < 32; kk += 2) {
      const float b = sb[(kk + rh) * 33 + c];
#pragma unroll
      for (int t = 0; t < MT; ++t) acc[t] = mfma_32x32x2(sa[(kk + rh) * MW + t * 32 + c], b, acc[t]);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // tile reads done before the next k-step overwrites them
  }
  __syncthreads();
  float* red = mel_smem;                                 // [wave][MT][16][64]
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) red[((wave * MT + t) * 16 + r) * 64 + lane] = acc[t][r];
  __syncthreads();
  for (int idx = threadIdx.x; idx < MT * 16 * 64; idx += 256) {
    const int l = idx & 63, r = (idx >> 6) & 15, t = idx >> 10;
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) v += red[((w * MT + t) * 16 + r) * 64 + l];
    const int m = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
    const int64_t bt = bt0 + (l & 31);
    if (m < n_mels && bt < BT) mm_out[bt * n_mels + m] = v;
  }
}

// mel (n_mels, F) -> tiled[ks][k][m] with m padded to mw and k to 32 * ksteps (zeros)
static __global__ void k_mel_tile(const float* __restrict__ mel, float* __restrict__ tiled, int F, int n_mels, int mw, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int m = i % mw;
  const int64_t k = i / mw;
  tiled[i] = (m < n_mels && k < F) ? mel[(int64_t)m * F + k] : 0.f;
}

// dA[bt, f] = sum_m dM[bt, m] * Mel[m, f] ; G[bt, f] = dA * S/|S| * (interior ? 1/2 : 1)   (in place over S)
// grid (ceil(BT/32), ceil(F/32)), one wave per block.
static __global__ __launch_bounds__(64) void k_mel_backward_mfma(cplx<float>* __restrict__ spec, const float* __restrict__ mel,
                                                          const float* __restrict__ dM, int64_t BT, int F, int n_mels,
                                                          int n_fft, int onesided) {
  __shared__ float sa[32][33];   // dM tile  [bt][m]
  __shared__ float sb[32][33];   // Mel tile [m][f]
  const int lane = threadIdx.x;
  const int64_t bt0 = (int64_t)blockIdx.x * 32;
  const int f0 = blockIdx.y * 32;
  f32x16 acc = {0};
  for (int k0 = 0; k0 < n_mels; k0 += 32) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int r = i * 2 + (lane >> 5), c = lane & 31;
      float va = 0.f, vb = 0.f;
      if (bt0 + r < BT && k0 + c < n_mels) va = dM[(bt0 + r) * n_mels + k0 + c];
      if (k0 + r < n_mels && f0 + c < F) vb = mel[(int64_t)(k0 + r) * F + f0 + c];
      sa[r][c] = va;
      sb[r][c] = vb;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 32; kk += 2) {
      const float a = sa[lane & 31][kk + (lane >> 5)];   // A[i = bt][k = m]
      const float b = sb[kk + (lane >> 5)][lane & 31];   // B[k = m][j = f]
      acc = mfma_32x32x2(a, b, acc);
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);   // bt
    const int f = f0 + (lane & 31);
    if (bt0 + row < BT && f < F) {
      const int64_t idx = (bt0 + row) * F + f;
      const cplx<float> s = spec[idx];
      const float mag = hypotf(s.x, s.y);
      float g = mag > 0.f ? acc[r] / mag : 0.f;
      if (onesided && f != 0 && 2 * f != n_fft) g *= 0.5f;
      spec[idx] = mk<float>(s.x * g, s.y * g);
    }
  }
}

// Same contraction per workgroup of 32 frames: the dM tile (32 frames x all mel rows) is staged once as [m][bt]; each
// wave then walks frequency tiles (wave w takes tiles w, w+4, ...), reading the filterbank from a copy tiled per
// frequency tile as [m][f] (k_mel_tile_t) and the spectrum values of the tile before the MFMA block.
template <int MT>
__global__ __launch_bounds__(256) void k_mel_backward_tiles(cplx<float>* __restrict__ spec, const float* __restrict__ mel_tiled_t,
                                                            const float* __restrict__ dM, int64_t BT, int F, int n_mels,
                                                            int n_fft, int onesided) {
  using f4 = float __attribute__((ext_vector_type(4)));
  constexpr int MW = MT * 32;
  extern __shared__ __attribute__((aligned(16))) float mel_smem[];
  float* sd = mel_smem;                                   // dM tile [m][bt], row stride 33
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* sm = mel_smem + MW * 33 + (size_t)wave * MW * 32;   // this wave's Mel tile [m][f]
  const int64_t bt0 = (int64_t)blockIdx.x * 32;
  const int c = lane & 31, rh = lane >> 5;
  for (int e = threadIdx.x; e < 32 * MW; e += 256) {
    const int bt = e / MW, m = e - bt * MW;
    sd[m * 33 + bt] = (bt0 + bt < BT && m < n_mels) ? dM[(bt0 + bt) * n_mels + m] : 0.f;
  }
  __syncthreads();
  const int ftiles = (F + 31) / 32;
  cplx<float> sv[16], sn[16];
  f4 mv[MT * 4], mn[MT * 4];
  auto fetch = [&](int ft, cplx<float>(&svv)[16], f4(&mvv)[MT * 4]) {
    const int f = ft * 32 + c;
    const f4* mg = reinterpret_cast<const f4*>(mel_tiled_t + (size_t)ft * MW * 32);
#pragma unroll
    for (int i = 0; i < MT * 4; ++i) mvv[i] = mg[i * 64 + lane];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * rh;
      svv[r] = (bt0 + row < BT && f < F) ? spec[(bt0 + row) * F + f] : mk<float>(0.f, 0.f);
    }
  };
  if (wave < ftiles) fetch(wave, sv, mv);
  for (int ft = wave; ft < ftiles; ft += 4) {
    const int f = ft * 32 + c;
#pragma unroll
    for (int i = 0; i < MT * 4; ++i) reinterpret_cast<f4*>(sm)[i * 64 + lane] = mv[i];
    if (ft + 4 < ftiles) fetch(ft + 4, sn, mn);          // the next tile's operands fly during this tile's MFMA block
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    f32x16 acc = {0};
#pragma unroll
    for (int kk = 0; kk < MW; kk += 2) acc = mfma_32x32x2(sd[(kk + rh) * 33 + c], sm[(kk + rh) * 32 + c], acc);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * rh;
      if (bt0 + row < BT && f < F) {
        const float mag = __builtin_amdgcn_sqrtf(fmaf(sv[r].x, sv[r].x, sv[r].y * sv[r].y));
        float g = mag > 0.f ? acc[r] / mag : 0.f;
        if (onesided && f != 0 && 2 * f != n_fft) g *= 0.5f;
        spec[(bt0 + row) * F + f] = mk<float>(sv[r].x * g, sv[r].y * g);
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) sv[r] = sn[r];
#pragma unroll
    for (int i = 0; i < MT * 4; ++i) mv[i] = mn[i];
  }
}

// mel (n_mels, F) -> tiled_t[ft][m][f] with m padded to mw and f to 32 * ftiles (zeros)
static __global__ void k_mel_tile_t(const float* __restrict__ mel, float* __restrict__ tiled, int F, int n_mels, int mw, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int fl = i & 31;
  const int m = (i >> 5) % mw;
  const int64_t ft = i / ((int64_t)32 * mw);
  const int64_t f = ft * 32 + fl;
  tiled[i] = (m < n_mels && f < F) ? mel[(int64_t)m * F + f] : 0.f;
}

// ---- elementwise pieces -----------------------------------------------------------------------------------------
// V = |S| in user layout (B, F, T) from S (B, T, F)
template <typename T>
__global__ void k_mag_to_user(const cplx<T>* __restrict__ spec, T* __restrict__ v, int Bn, int Tn, int F) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // over (b, f, t)
  if (i >= (int64_t)Bn * F * Tn) return;
  const int t = i % Tn;
  const int f = (i / Tn) % F;
  const int64_t b = i / ((int64_t)Tn * F);
  const cplx<T> s = spec[(b * Tn + t) * F + f];
  v[i] = si_hypot(s.x, s.y);
}

// V = log1p(mm) in user layout (B, n_mels, T) from mm (B*T, n_mels)
template <typename T>
__global__ void k_log1p_to_user(const T* __restrict__ mm, T* __restrict__ v, int Bn, int Tn, int n_mels) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // over (b, m, t)
  if (i >= (int64_t)Bn * n_mels * Tn) return;
  const int t = i % Tn;
  const int m = (i / Tn) % n_mels;
  const int64_t b = i / ((int64_t)Tn * n_mels);
  v[i] = log1p(mm[(b * Tn + t) * n_mels + m]);
}

// MAG transform: loss partials and G = (2/numel) (|S| - T) S/|S| * (interior ? 1/2 : 1) in place over S
template <typename T>
__global__ void k_mag_loss_grad(cplx<T>* __restrict__ spec, const T* __restrict__ target, int target_btf, int Bn, int Tn, int F,
                                int n_fft, int onesided, double inv_numel, double* __restrict__ part) {
  __shared__ double red[16];
  double s2 = 0;
  const int64_t total = (int64_t)Bn * Tn * F;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int f = i % F;
    const int t = (i / F) % Tn;
    const int64_t b = i / ((int64_t)F * Tn);
    const cplx<T> s = spec[i];
    const T mag = si_hypot(s.x, s.y);
    const T d = mag - (target_btf ? target[i] : target[(b * F + f) * Tn + t]);
    s2 += (double)d * (double)d;
    T g = mag > T(0) ? (T)(2.0 * inv_numel) * d / mag : T(0);
    if (onesided && f != 0 && 2 * f != n_fft) g *= T(0.5);
    spec[i] = mk<T>(s.x * g, s.y * g);
  }
  const double t = block_sum(s2, red);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// LOGMEL: loss partials and dM = (2/numel) (log1p(mm) - T) / (1 + mm), in place over mm (BT, n_mels)
template <typename T>
__global__ void k_logmel_loss_dm(T* __restrict__ mm, const T* __restrict__ target, int Bn, int Tn, int n_mels,
                                 double inv_numel, double* __restrict__ part) {
  __shared__ double red[16];
  double s2 = 0;
  const int64_t total = (int64_t)Bn * Tn * n_mels;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int m = i % n_mels;
    const int t = (i / n_mels) % Tn;
    const int64_t b = i / ((int64_t)n_mels * Tn);
    const T v = mm[i];
    const T d = log1p(v) - target[(b * n_mels + m) * Tn + t];
    s2 += (double)d * (double)d;
    mm[i] = (T)(2.0 * inv_numel) * d / (T(1) + v);
  }
  const double t = block_sum(s2, red);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// float64 / generic mel contractions (VALU): thread per output
template <typename T>
__global__ void k_mel_forward_valu(const cplx<T>* __restrict__ spec, const T* __restrict__ mel, T* __restrict__ mm,
                                   int64_t BT, int F, int n_mels) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= BT * n_mels) return;
  const int m = i % n_mels;
  const int64_t bt = i / n_mels;
  T acc = 0;
  for (int f = 0; f < F; ++f) {
    const cplx<T> s = spec[bt * F + f];
    acc += mel[(int64_t)m * F + f] * si_hypot(s.x, s.y);
  }
  mm[i] = acc;
}

template <typename T>
__global__ void k_mel_backward_valu(cplx<T>* __restrict__ spec, const T* __restrict__ mel, const T* __restrict__ dM,
                                    int64_t BT, int F, int n_mels, int n_fft, int onesided) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= BT * F) return;
  const int f = i % F;
  const int64_t bt = i / F;
  T acc = 0;
  for (int m = 0; m < n_mels; ++m) acc += dM[bt * n_mels + m] * mel[(int64_t)m * F + f];
  const cplx<T> s = spec[i];
  const T mag = si_hypot(s.x, s.y);
  T g = mag > T(0) ? acc / mag : T(0);
  if (onesided && f != 0 && 2 * f != n_fft) g *= T(0.5);
  spec[i] = mk<T>(s.x * g, s.y * g);
}

// inverse frames (generic): windowed Hermitian inverse transform of a (B, T, F) spectrum, scale = c.inv_scale.
// Used by _istft (scale 1/N) and by the STFT adjoint of the L_BFGS gradient (scale = forward scale).
template <typename T, bool IP = false>
__global__ void k_grad_frames(FrameCfg<T> c, const cplx<T>* __restrict__ g, T* __restrict__ frames) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cplx<T>* a = reinterpret_cast<cplx<T>*>(smem);
  cplx<T>* b = IP ? a : a + c.n_fft;
  const int t = blockIdx.x, bi = blockIdx.y;
  const cplx<T>* in = g + ((int64_t)bi * c.n_frames + t) * c.n_freq;
  for (int f = threadIdx.x; f < c.n_freq; f += blockDim.x) a[f] = in[f];
  __syncthreads();
  spectrum_to_frame<T, IP>(c, a, b, frames + ((int64_t)bi * c.n_frames + t) * c.n_fft, c.window);
}

// Fold of the padded margins onto the signal: grad already holds the plain overlap-add of the gradient frames over
// the signal's own positions (k_ola / k_ola_f4 without the envelope); every sample within `pad` of an edge also
// receives what the padding copied from it (reflect / replicate / circular).  One thread per margin sample.  The
// gradient w.r.t. a padded sample is gathered from `frames`, or read from `margins` (B, 2, pad: the pad samples left and
// right of the signal, written by k_hop_inverse) when that is given.
template <typename T>
__global__ void k_grad_fold_margins(const T* __restrict__ frames, T* __restrict__ grad, int n_fft, int hop, int pad,
                                    int pad_mode, int n_frames, int64_t len, int64_t rows, const T* __restrict__ margins) {
  const int64_t per_row = 2 * ((int64_t)pad + 1);
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * per_row) return;
  const int64_t bi = i / per_row, j = i - bi * per_row;
  int64_t n;
  if (j <= pad) {
    n = j;                                            // left stretch 0 .. pad
    if (n >= len) return;
  } else {
    n = len - 1 - pad + (j - pad - 1);                // right stretch len-1-pad .. len-1
    if (n <= pad || n >= len) return;                 // (short signals: already covered by the left stretch)
  }
  const T* fr = frames + bi * n_frames * n_fft;
  const int64_t covered = (int64_t)(n_frames - 1) * hop + n_fft;   // padded positions that receive any frame
  auto at = [&](int64_t np) -> T {                                 // gradient w.r.t. padded sample np
    if (np < 0 || np >= covered) return T(0);
    if (margins != nullptr) {
      const T* mg = margins + bi * 2 * pad;
      if (np < pad) return mg[np];
      const int64_t r = np - pad - len;
      return (r >= 0 && r < pad) ? mg[pad + r] : T(0);
    }
    int64_t t_hi = np / hop;
    if (t_hi > n_frames - 1) t_hi = n_frames - 1;
    const int64_t t_lo = np - n_fft + 1 <= 0 ? 0 : (np - n_fft + hop) / hop;
    T acc = 0;
    for (int64_t t = t_lo; t <= t_hi; ++t) acc += fr[t * n_fft + (np - t * hop)];
    return acc;
  };
  T g = 0;
  switch (pad_mode) {
    case SPECINV_PAD_REFLECT:
      if (n >= 1 && n <= pad) g += at(pad - n);                               // left margin i = pad - n
      if (n <= len - 2 && n >= len - 1 - pad) g += at(pad + len + (len - 2 - n));
      break;
    case SPECINV_PAD_REPLICATE:
      if (n == 0)
        for (int64_t q = 0; q < pad; ++q) g += at(q);
      if (n == len - 1)
        for (int64_t q = 0; q < pad; ++q) g += at(pad + len + q);
      break;
    case SPECINV_PAD_CIRCULAR:
      if (n >= len - pad) g += at(n - (len - pad));
      if (n < pad) g += at(pad + len + n);
      break;
    default:
      break;
  }
  grad[bi * len + n] += g;
}

}  // namespace specinv
