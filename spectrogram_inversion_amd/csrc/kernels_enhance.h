// Single-channel speech enhancement: a noise-power tracker, the decision-directed a-priori SNR and a Wiener or
// log-spectral-amplitude gain over a batch of spectrograms, one launch.
//   Per item and bin, frames l = 0 ... T - 1.  P_l = |X_l|^2 (re^2 + im^2, or m^2 for real magnitudes).  All state and arithmetic
//   are float64 whatever the input dtype; tiny = 1e-300, and every quotient by max(sigma^2, tiny) is capped at 1e300 (nothing
//   overflows, so nothing is NaN); xi1 = the prior SNR, c = xi1 / (1 + xi1).
//   Tracker (Gerkmann & Hendriks 2012).  Without a state sigma^2_{-1} is the mean of P_l over the first min(init_frames, T) frames,
//   summed in frame order, and Pbar_{-1} = 0.
//       g'     = P_l / max(sigma^2_{l-1}, tiny)
//       p      = 1 / (1 + (1 + xi1) exp(-(g' c)))
//       Pbar_l = a_spp Pbar_{l-1} + (1 - a_spp) p ;   if Pbar_l > 0.99: p = min(p, 0.99)
//       sigma^2_l = a_pow sigma^2_{l-1} + (1 - a_pow) ((1 - p) P_l + p sigma^2_{l-1})
//   With a noise array the tracker is bypassed: sigma^2_l is that array's value, Pbar passes through.
//   Gain (decision-directed, Ephraim & Malah 1984 / 1985).
//       g    = P_l / max(sigma^2_l, tiny)
//       xi_l = max(alpha A^2_{l-1} / max(sigma^2_l, tiny) + (1 - alpha) max(g - 1, 0), xi_min)     (no state, l = 0: alpha)
//       w    = xi_l / (1 + xi_l) ;   Wiener: G = w ;   LSA: G = w exp(E1(max(w g, 1e-12)) / 2)
//       G_l  = min(max(G, g_min), 1) ;   A^2_l = G_l^2 P_l
//   The products and sums above are not contracted, so that a frame's values are a function of the chain's three numbers and P_l
//   alone: a walk cut in two and chained through the state gives the same bits, and so do the two layouts.
//
// E1.  v <= 1: -gamma - ln v + sum_{k=1}^{18} c_k v^k, c_k = (-1)^(k+1) / (k k!).  1 < v <= 700: exp(-v) / v R(v) with
// R(v) = v e^v E1(v) a Chebyshev sum of degree 15 in 1 / v on each of [1, 2), [2, 4), ... [64, 128), [128, 1024] (enhance_e1_table.h,
// written by tools/gen_e1_table.py from 50-digit values).  Beyond 700: 0.  The float64 evaluation of the scheme is within 4.9e-16
// of E1 on [1e-12, 700] with NumPy's exp and log; the bound stated for the device is 1e-13.  The table sits in constant memory and a
// lane reads its own interval's row: 16 loads a frame that hit the scalar or vector cache.
//
// Mapping.  A lane owns one (item, bin) chain and walks its frames with sigma^2, Pbar and A^2 in registers; a workgroup takes
// kEnhBins neighbouring chains, which one wave walks.  Output pointers are nullable and a null one skips its store.
//   Frame-major, (B, T, F): lanes on consecutive bins read and write consecutive addresses; a lane keeps the next kEnhAhead frames'
//   loads in flight.
//   Bin-major, (B, F, T): the rows of the (B F, T) matrix are the chains.  A tile is kEnhBins rows by kEnhTile frames; the four waves
//   of the workgroup load it along T (32 consecutive frames of two rows per wave instruction), turn it into P in float64 and lay
//   it into LDS with rows of kEnhTile + 1 doubles, so that the walk's lane b reads [b][t] without a bank conflict (66 dwords
//   between lanes, 32 lanes on 64 banks).  The results go back through LDS tiles of the same shape and are stored along T; the product G X reads X once
//   more (a cache hit).  Tile n + 1's loads are issued before tile n is walked and wait in registers, kEnhBins / 8 elements a thread;
//   waves 1 ... 3 then wait at the barrier while wave 0 walks.
//   LDS: seven tiles (P twice, sigma^2 twice - the noise array's tiles when it is given, the tracker's output otherwise - p, G, xi),
//   7 x kEnhBins x 33 x 8 bytes.
// The grid is looped: any number of chains.  No atomics, no plan, no scratch allocation.  All offsets are 64-bit.
#pragma once
#include "common.h"
#include "enhance_e1_table.h"

namespace specinv {

#ifndef SPECINV_ENHANCE_BINS
#define SPECINV_ENHANCE_BINS 64   // chains a wave walks (64, 32 or 16: measured, tools/log/EXPERIMENTS.md)
#endif
constexpr int kEnhBins = SPECINV_ENHANCE_BINS;
constexpr int kEnhTile = 32;            // frames a tile holds (enhance.py: _TILE_FRAMES)
constexpr int kEnhThreads = 256;        // the bin-major workgroup: wave 0 walks, all four load and store
constexpr int kEnhAhead = 4;            // frames a lane requests ahead in the frame-major walk
constexpr int kEnhMaxGrid = 4096;       // workgroups of a launch; the groups beyond are looped over
constexpr int kEnhLd = kEnhTile + 1;
static_assert(kEnhBins == 16 || kEnhBins == 32 || kEnhBins == 64, "a wave walks 16, 32 or 64 chains");
static_assert(kEnhTile == 32, "the tile's loads take 32 frames of two rows per wave instruction");

enum { kEnhWiener = 0, kEnhLsa = 1 };
enum { kEnhNoiseTracked = 0, kEnhNoiseFull = 1, kEnhNoiseProfile = 2 };

constexpr size_t enhance_lds_bytes() { return sizeof(double) * 7 * (size_t)kEnhBins * kEnhLd; }

struct EnhArgs {
  const void* spec;        // (B, F, T) or (B, T, F), T or cplx<T>
  const void* noise_in;    // nullptr, the same shape (real T), or (B, F)
  const double* state_in;  // (B, F, 3) or nullptr
  void* noise_out;         // real T, spec's shape, or nullptr (so are the next three)
  void* spp_out;
  void* gain_out;
  void* snr_out;
  void* enh_out;           // spec's type and shape, or nullptr
  double* state_out;       // (B, F, 3) or nullptr
  int64_t batch, n_freq, n_frames;
  int init_frames;
  int noise_mode;
  double a_pow, a_spp, xi1p, c, alpha, xi_min, g_min;   // xi1p = 1 + xi1
};

struct EnhChain {
  double sig, pbar, a2;
  bool first;
};

__device__ __forceinline__ double enh_e1(double v) {
  if (v <= 1.0) {
    double s = kE1SeriesCoef[kE1Series - 1];
#pragma unroll
    for (int k = kE1Series - 2; k >= 0; --k) s = fma(s, v, kE1SeriesCoef[k]);
    return (s * v - log(v)) - 0.57721566490153286061;
  }
  if (!(v <= 700.0)) return 0.0;
  int j = (int)((__double2hiint(v) >> 20) & 0x7ff) - 1023;      // floor(log2 v), 0 ... 9
  j = j < kE1Intervals - 1 ? j : kE1Intervals - 1;
  const double rv = 1.0 / v;
  const double t = (2.0 * rv - kE1Mid[j]) * kE1Scale[j];
  const double* cf = kE1Cheb[j];
  double b1 = 0.0, b2 = 0.0;
#pragma unroll
  for (int k = kE1Degree; k >= 1; --k) {
    const double b0 = cf[k] + fma(2.0 * t, b1, -b2);
    b2 = b1;
    b1 = b0;
  }
  const double r = cf[0] + fma(t, b1, -b2);
  return exp(-v) * rv * r;
}

template <typename T, bool CPLX>
struct EnhIn {
  using type = T;
  static __device__ __forceinline__ double power(T x) {
#pragma clang fp contract(off)
    const double m = (double)x;
    return m * m;
  }
  static __device__ __forceinline__ T scale(T x, double g) { return (T)(g * (double)x); }
  static __device__ __forceinline__ T zero() { return (T)0; }
};
template <typename T>
struct EnhIn<T, true> {
  using type = cplx<T>;
  static __device__ __forceinline__ double power(cplx<T> x) {
#pragma clang fp contract(off)
    const double re = (double)x.x, im = (double)x.y;
    const double a = re * re, b = im * im;
    return a + b;
  }
  static __device__ __forceinline__ cplx<T> scale(cplx<T> x, double g) { return mk<T>((T)(g * (double)x.x), (T)(g * (double)x.y)); }
  static __device__ __forceinline__ cplx<T> zero() { return mk<T>((T)0, (T)0); }
};

// one frame of one chain: `sig_in` is the noise array's value when the tracker is bypassed
template <int RULE>
__device__ __forceinline__ void enh_step(const EnhArgs& a, bool track, EnhChain& s, double P, double sig_in, double& p_out, double& g_out,
                                         double& xi_out) {
#pragma clang fp contract(off)
  constexpr double kTiny = 1e-300, kCap = 1e300;
  double p = 0.0;
  if (track) {
    const double gp = fmin(P / fmax(s.sig, kTiny), kCap);
    const double e = exp(-(gp * a.c));
    p = 1.0 / (1.0 + a.xi1p * e);
    const double q = (1.0 - a.a_spp) * p;
    s.pbar = a.a_spp * s.pbar + q;
    if (s.pbar > 0.99) p = fmin(p, 0.99);
    const double u = (1.0 - p) * P, v = p * s.sig;
    const double m = (1.0 - a.a_pow) * (u + v);
    s.sig = a.a_pow * s.sig + m;
  } else {
    s.sig = sig_in;
  }
  const double den = fmax(s.sig, kTiny);
  const double g = fmin(P / den, kCap);
  const double r = s.first ? 1.0 : fmin(s.a2 / den, kCap);
  const double dd = a.alpha * r, ml = (1.0 - a.alpha) * fmax(g - 1.0, 0.0);
  const double xi = fmax(dd + ml, a.xi_min);
  const double w = xi / (1.0 + xi);
  double G = w;
  if (RULE == kEnhLsa) {
    const double wg = w * g;
    const double h = 0.5 * enh_e1(fmax(wg, 1e-12));
    G = w * exp(h);
  }
  G = fmin(fmax(G, a.g_min), 1.0);
  const double gg = G * G;
  s.a2 = gg * P;
  s.first = false;
  p_out = p;
  g_out = G;
  xi_out = xi;
}

// the chain's start: the state, or the start rule over the first min(init_frames, T) frames, `stride` elements apart
template <typename T, bool CPLX>
__device__ __forceinline__ EnhChain enh_start(const EnhArgs& a, bool track, int64_t chain, const typename EnhIn<T, CPLX>::type* x,
                                              int64_t stride) {
#pragma clang fp contract(off)
  EnhChain s;
  if (a.state_in != nullptr) {
    s.sig = a.state_in[3 * chain];
    s.pbar = a.state_in[3 * chain + 1];
    s.a2 = a.state_in[3 * chain + 2];
    s.first = false;
    return s;
  }
  s.sig = 0.0;
  s.pbar = 0.0;
  s.a2 = 0.0;
  s.first = true;
  if (track) {
    const int64_t n0 = a.init_frames < a.n_frames ? (int64_t)a.init_frames : a.n_frames;
    double acc = 0.0;
    for (int64_t l = 0; l < n0; ++l) acc = acc + EnhIn<T, CPLX>::power(x[l * stride]);
    s.sig = acc / (double)n0;
  }
  return s;
}

__device__ __forceinline__ void enh_finish(const EnhArgs& a, int64_t chain, const EnhChain& s) {
  if (a.state_out != nullptr) {
    a.state_out[3 * chain] = s.sig;
    a.state_out[3 * chain + 1] = s.pbar;
    a.state_out[3 * chain + 2] = s.a2;
  }
}

template <typename T, bool CPLX, int RULE>
__device__ __forceinline__ void enh_walk_frame_major(const EnhArgs& a) {
  using In = EnhIn<T, CPLX>;
  using V = typename In::type;
  const bool track = a.noise_mode == kEnhNoiseTracked;
  const int64_t F = a.n_freq, nT = a.n_frames;
  const int64_t groups_f = (F + kEnhBins - 1) / kEnhBins;
  const int64_t n_groups = a.batch * groups_f;
  T* const noise_out = (T*)a.noise_out;
  T* const spp_out = (T*)a.spp_out;
  T* const gain_out = (T*)a.gain_out;
  T* const snr_out = (T*)a.snr_out;
  V* const enh_out = (V*)a.enh_out;
  for (int64_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
    const int64_t item = grp / groups_f;
    const int64_t f = (grp - item * groups_f) * kEnhBins + threadIdx.x;
    if ((int)threadIdx.x >= kEnhBins || f >= F) continue;
    const int64_t chain = item * F + f;
    const int64_t base = item * nT * F + f;
    const V* x = (const V*)a.spec + base;
    const T* nz = a.noise_mode == kEnhNoiseFull ? (const T*)a.noise_in + base : nullptr;
    const double profile = a.noise_mode == kEnhNoiseProfile ? (double)((const T*)a.noise_in)[chain] : 0.0;
    V xb[kEnhAhead];
    T nb[kEnhAhead];
#pragma unroll
    for (int i = 0; i < kEnhAhead; ++i) {
      xb[i] = In::zero();
      nb[i] = (T)0;
      if (i < nT) {
        xb[i] = x[(int64_t)i * F];
        if (nz != nullptr) nb[i] = nz[(int64_t)i * F];
      }
    }
    EnhChain s = enh_start<T, CPLX>(a, track, chain, x, F);
    for (int64_t t0 = 0; t0 < nT; t0 += kEnhAhead) {
#pragma unroll
      for (int i = 0; i < kEnhAhead; ++i) {
        const int64_t t = t0 + i;
        if (t < nT) {
          const V cur = xb[i];
          const double sig_in = nz != nullptr ? (double)nb[i] : profile;
          if (t + kEnhAhead < nT) {
            xb[i] = x[(t + kEnhAhead) * F];
            if (nz != nullptr) nb[i] = nz[(t + kEnhAhead) * F];
          }
          double p, G, xi;
          enh_step<RULE>(a, track, s, In::power(cur), sig_in, p, G, xi);
          const int64_t o = base + t * F;
          if (noise_out != nullptr) noise_out[o] = (T)s.sig;
          if (spp_out != nullptr) spp_out[o] = (T)p;
          if (gain_out != nullptr) gain_out[o] = (T)G;
          if (snr_out != nullptr) snr_out[o] = (T)xi;
          if (enh_out != nullptr) enh_out[o] = In::scale(cur, G);
        }
      }
    }
    enh_finish(a, chain, s);
  }
}

template <typename T, bool CPLX, int RULE>
__device__ __forceinline__ void enh_walk_bin_major(const EnhArgs& a, double* lds) {
  using In = EnhIn<T, CPLX>;
  using V = typename In::type;
  constexpr int kTileElems = kEnhBins * kEnhLd;
  constexpr int kPass = kEnhThreads / 32;       // rows the workgroup loads at once: row kPass i + tid / 32, frame tid % 32
  constexpr int kPer = kEnhBins / kPass;        // elements of a tile a thread loads
  double* const sP = lds;                        // two tiles
  double* const sN = lds + 2 * kTileElems;       // two tiles
  double* const sS = lds + 4 * kTileElems;
  double* const sG = lds + 5 * kTileElems;
  double* const sX = lds + 6 * kTileElems;
  const bool track = a.noise_mode == kEnhNoiseTracked;
  const bool full = a.noise_mode == kEnhNoiseFull;
  const int64_t rows = a.batch * a.n_freq, nT = a.n_frames;
  const int64_t n_groups = (rows + kEnhBins - 1) / kEnhBins;
  const int64_t n_tiles = (nT + kEnhTile - 1) / kEnhTile;
  const int lane = threadIdx.x, lt = lane & 31, lr = lane >> 5;      // (lane: the chain of the group, for wave 0)
  const V* const spec = (const V*)a.spec;
  const T* const noise_in = (const T*)a.noise_in;
  T* const noise_out = (T*)a.noise_out;
  T* const spp_out = (T*)a.spp_out;
  T* const gain_out = (T*)a.gain_out;
  T* const snr_out = (T*)a.snr_out;
  V* const enh_out = (V*)a.enh_out;
  for (int64_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
    const int64_t row0 = grp * kEnhBins;
    const int64_t chain = row0 + lane;
    const bool walks = lane < kEnhBins && chain < rows;
    V xr[kPer];
    T nr[kPer];
    // tile 0's loads first, so that the start rule's strided reads wait alongside them
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int64_t r = row0 + kPass * i + lr;
      xr[i] = In::zero();
      nr[i] = (T)0;
      if (r < rows && lt < nT) {
        xr[i] = spec[r * nT + lt];
        if (full) nr[i] = noise_in[r * nT + lt];
      }
    }
    EnhChain s;
    double profile = 0.0;
    if (walks) {
      s = enh_start<T, CPLX>(a, track, chain, spec + chain * nT, 1);
      if (a.noise_mode == kEnhNoiseProfile) profile = (double)noise_in[chain];
    }
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      sP[(kPass * i + lr) * kEnhLd + lt] = In::power(xr[i]);
      if (full) sN[(kPass * i + lr) * kEnhLd + lt] = (double)nr[i];
    }
    __syncthreads();
    for (int64_t n = 0; n < n_tiles; ++n) {
      const int cur = (int)(n & 1);
      const int64_t tb = n * kEnhTile;
      const bool more = n + 1 < n_tiles;
      if (more) {
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
          const int64_t r = row0 + kPass * i + lr, t = tb + kEnhTile + lt;
          xr[i] = In::zero();
          nr[i] = (T)0;
          if (r < rows && t < nT) {
            xr[i] = spec[r * nT + t];
            if (full) nr[i] = noise_in[r * nT + t];
          }
        }
      }
      if (walks) {
        const int len = nT - tb < kEnhTile ? (int)(nT - tb) : kEnhTile;
        const double* const pP = sP + cur * kTileElems + lane * kEnhLd;
        double* const pN = sN + cur * kTileElems + lane * kEnhLd;
        double* const pS = sS + lane * kEnhLd;
        double* const pG = sG + lane * kEnhLd;
        double* const pX = sX + lane * kEnhLd;
        for (int t = 0; t < len; ++t) {
          double p, G, xi;
          enh_step<RULE>(a, track, s, pP[t], full ? pN[t] : profile, p, G, xi);
          pN[t] = s.sig;
          pS[t] = p;
          pG[t] = G;
          pX[t] = xi;
        }
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < kPer; ++i) {
        const int64_t r = row0 + kPass * i + lr, t = tb + lt;
        if (r < rows && t < nT) {
          const int e = (kPass * i + lr) * kEnhLd + lt;
          const int64_t o = r * nT + t;
          if (noise_out != nullptr) noise_out[o] = (T)sN[cur * kTileElems + e];
          if (spp_out != nullptr) spp_out[o] = (T)sS[e];
          if (gain_out != nullptr) gain_out[o] = (T)sG[e];
          if (snr_out != nullptr) snr_out[o] = (T)sX[e];
          if (enh_out != nullptr) enh_out[o] = In::scale(spec[o], sG[e]);
        }
      }
      if (more) {
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
          sP[(cur ^ 1) * kTileElems + (kPass * i + lr) * kEnhLd + lt] = In::power(xr[i]);
          if (full) sN[(cur ^ 1) * kTileElems + (kPass * i + lr) * kEnhLd + lt] = (double)nr[i];
        }
      }
      __syncthreads();
    }
    if (walks) enh_finish(a, chain, s);
  }
}

template <typename T, bool CPLX, bool FRAME_MAJOR, int RULE>
__global__ __launch_bounds__(kEnhThreads) void k_enhance(const EnhArgs a) {
  extern __shared__ __attribute__((aligned(16))) double enh_lds[];
  if constexpr (FRAME_MAJOR)
    enh_walk_frame_major<T, CPLX, RULE>(a);
  else
    enh_walk_bin_major<T, CPLX, RULE>(a, enh_lds);
}

}  // namespace specinv
