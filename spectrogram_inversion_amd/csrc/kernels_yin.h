// YIN: the f0 tracker of de Cheveigne & Kawahara 2002 over a batch of waveforms, one launch.
//   x is (B, L), real.  N = frame_length (256, 512, 1024, 2048), W = N / 2, H = hop_length (1 ... N); xz(i) = x[i] for
//   0 <= i < L, else 0.
//   Frames.       center: T = 1 + L / H, s_m = m H - W;  otherwise L >= N, T = 1 + (L - N) / H, s_m = m H.  f_m[j] = xz(s_m + j), j < N.
//   Difference.   d(tau) = sum_{j<W} (f[j] - f[j+tau])^2 = E(0) + E(tau) - 2 r(tau), tau = 0 ... W, with
//                 E(tau) = sum_{j=tau}^{tau+W-1} f[j]^2 and r(tau) = sum_{j<W} f[j] f[j+tau]: the first W + 1 lags of the circular
//                 length-N correlation of the frame with its own first half zero-padded to N (nothing wraps for tau <= N - W).
//   Normalised.   d'(0) = 1;  c(tau) = sum_{k=1}^{tau} d(k);  d'(tau) = d(tau) tau / c(tau) where c(tau) > 0, else 1 (silence: d' = 1).
//   Pick over [tau_min, tau_max], 1 <= tau_min < tau_max <= W - 1:  tau0 = the smallest tau of the range with d'(tau) < threshold.
//                 If it exists, tau* = tau0 advanced while tau* + 1 <= tau_max and d'(tau* + 1) < d'(tau*); if not, tau* is the
//                 first arg-min of d' over the range.
//   Refinement.   a, b, c = d'(tau* - 1), d'(tau*), d'(tau* + 1), q = a - 2 b + c;  s = (a - c) / (2 q) if q > 0 and |a - c| < q,
//                 else 0;  period = tau* + s, aperiodicity = b (voiced: b < threshold, exactly the condition that tau0 existed).
//   Arithmetic.   r through the float32 wave-level FFT (lags 1 ... 8: d by the literal sum in float64); E, d and c in float64; d'
//                 rounded once to float32; the pick runs on those float32 values (the ones `cmnd` receives) against the float64
//                 threshold; the refinement in float64 from the three float32 values, rounded once.  NaN input is unspecified.
//
// Mapping.  A wave owns a frame; a workgroup of four waves takes four consecutive frames of one item, so that the frames in flight
// are neighbours and their overlap meets in L2.  A frame is N contiguous samples: lane l, register u holds point 64 u + l, a
// coalesced 256-byte row per load and fast_core.h's input layout with M = N complex points, R = N / 64 per lane (R = 4, 8, 16,
// 32).  No span of the signal is staged in LDS.
//
// Correlation: two complex transforms per frame.  z = f + i g with g = 2^sh f [j < W], sh = floor(log2(E_frame / E(0)) / 2), so
// that both halves of the packed transform carry about the same energy (a frame that leaves a silence would otherwise lose its
// quiet half in the rounding of the loud one); E(0) = 0 is r = 0.  Z = fft_forward(z) leaves bin k = 64 u + l in
// lane l, register u.  A[k] = (Z[k] + conj Z[N-k]) / 2 and G[k] = (Z[k] - conj Z[N-k]) / (2 i); the partner N - k is register
// R - 1 - u of lane 64 - l, and for lane 0 register (R - u) mod R of the lane itself.  With S = Z[k] + conj Z[N-k] and
// D = Z[k] - conj Z[N-k], conj(G) A = i conj(D) S / 4; fft_inverse of that is N r in the real parts, lag tau = 64 u + l in lane l,
// register u - the layout the frame came in.  2^-sh / (4 N) is a power of two.
//
// Short lags.  On a smooth signal d(1), d(2), ... are small differences of E(0), E(tau) and 2 r(tau), and c(tau) is a sum of a few
// of them: the float32 rounding of r, harmless relative to E, is then large relative to d and reaches every d' through c.  The
// lags 1 ... 8 therefore take d from the literal sum over j in float64, formed before the transforms from lane shifts of the
// frame: 8 (R / 2 + 1) shuffles and 8 wave sums.  With that the float32 restatement of the whole (tests/_yin_oracle.py, cmnd_f32)
// is within 2.2e-6 of float64 on the test signals instead of 7.1e-6, and nearly all of what remained was at lags 2 ... 7.
//
// Sums.  E(tau) = P(tau + W) - P(tau) with P the exclusive prefix sum of f^2: a 64-lane scan per register with a carry across
// registers, in float64, and tau + W is the same lane R / 2 registers up.  c is the same scan over d.  d' goes to the wave's
// transpose scratch as W + 1 floats, where the neighbours d'(tau + 1) of the descent and the three values of the refinement are
// read back; the pick itself is ballots over the R / 2 registers: the first lag below the threshold, the first lag at or after it
// that the descent does not leave, and - for an unvoiced frame - the first lag that equals the wave's minimum.  Both picks are
// computed and one is selected: no loop depends on the data.  Every lane computes the refinement; lane 0 stores.
//
// LDS: pass-1 twiddles (R - 1) x 64 and four transpose scratches of Geo<R>::TR complex elements - 13.9 / 23.0 / 41.5 / 81.5 KiB for
// R = 4 ... 32, which lets eleven / six / three / one workgroup share a CU's 160 KiB.  The registers allow fewer: 101 / 134 / 240 /
// 308 per lane with nothing spilled under __launch_bounds__(256) are four / three / two / one wave per SIMD, and a workgroup is one
// wave on each SIMD, so four / three / two / one workgroup per CU run.  All loops are bounded by R and W; offsets
// into global memory are 64-bit.
#pragma once
#include "fast_core.h"

namespace specinv {

constexpr int kYinWaves = 4;
constexpr int kYinThreads = 64 * kYinWaves;
constexpr int kYinDirect = 8;      // lags 1 ... 8 take d from the literal sum (below 64: they sit in register 0)

struct YinArgs {
  const float* x;        // (B, L)
  float* period;         // (B, T)
  float* aper;           // (B, T)
  int32_t* tau;          // (B, T) or nullptr
  float* cmnd;           // (B, T, W + 1) or nullptr
  int64_t length;        // L
  int64_t n_frames;      // T
  int64_t groups_t;      // workgroups per item, ceil(T / 4)
  int hop, center;
  int tau_min, tau_max;
  double threshold;
};

template <int R>
struct YinGeo {
  static constexpr int N = 64 * R;
  static constexpr int W = N / 2;
  static constexpr size_t lds_bytes() { return sizeof(fast::v2f) * (size_t)((R - 1) * 64 + kYinWaves * fast::Geo<R>::TR); }
  static_assert(sizeof(float) * (W + 1) <= sizeof(fast::v2f) * fast::Geo<R>::TR, "d' must fit the transpose scratch");
};

// inclusive sum over the lanes of a wave
__device__ __forceinline__ double yin_scan(double v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  return v;
}

// the smallest lag 64 u + l whose lane voted, over registers in rising order: `first` stays -1 while no lane has
__device__ __forceinline__ void yin_first(int& first, unsigned long long votes, int u) {
  if (first < 0 && votes != 0ull) first = 64 * u + __builtin_ctzll(votes);
}

template <int R>
__global__ void __launch_bounds__(kYinThreads) k_yin(YinArgs a, int64_t block0) {
  using namespace fast;
  using G = Geo<R>;
  constexpr int N = YinGeo<R>::N, W = YinGeo<R>::W, HR = R / 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  v2f* lds_tw1 = reinterpret_cast<v2f*>(smem);
  const int tid = threadIdx.x;
  const int wib = __builtin_amdgcn_readfirstlane(tid >> 6);
  v2f* tr = lds_tw1 + (R - 1) * 64 + wib * G::TR;
  float* dps = reinterpret_cast<float*>(tr);                 // d'(0 ... W) of the wave's frame, between its two uses as FFT scratch

  for (int i = tid; i < (R - 1) * 64; i += kYinThreads) {
    const int k1 = i / 64 + 1, l = i & 63;
    lds_tw1[i] = unit(2.0f * (float)((l * k1) % N) / (float)N);
  }
  __syncthreads();

  const LaneConst<R> k = lane_consts<R>();
  const int lane = k.lane;
  const int64_t blk = block0 + blockIdx.x;
  const int64_t item = blk / a.groups_t;
  const int64_t t = (blk - item * a.groups_t) * kYinWaves + wib;      // the wave's frame; the last workgroup of an item may not be full
  const float* __restrict__ xi = a.x + item * a.length;
  const double thr = a.threshold;
  const float scale = 1.0f / (float)(4 * N);

  if (t < a.n_frames) {
    // ---- the frame, and E from the prefix sums of its squares
    const int64_t s = t * (int64_t)a.hop - (a.center ? W : 0);
    v2f z[R];
    double e[HR], e0, ew;
    float back;                                              // r = Re z * back
    double dshort = 0.0;                                     // d(lane) for lane = 1 ... kYinDirect
    {
      double p[R], carry = 0.0;
#pragma unroll
      for (int u = 0; u < R; ++u) {
        const int64_t i = s + 64 * u + lane;
        const float f = (i >= 0 && i < a.length) ? xi[i] : 0.0f;
        z[u] = v2f{f, u < HR ? f : 0.0f};
        const double sq = (double)f * (double)f;
        const double inc = yin_scan(sq, lane) + carry;
        p[u] = inc - sq;                                     // P(64 u + l), exclusive
        carry = __shfl(inc, 63, 64);
      }
#pragma unroll
      for (int tau = 1; tau <= kYinDirect; ++tau) {
        // d(tau) by the literal sum: f[j + tau] is lane l + tau of the same register or lane l + tau - 64 of the next
        const int src = (lane + tau) & 63;
        const bool same = lane + tau < 64;
        float next = __shfl(z[0].x, src, 64);
        double acc = 0.0;
#pragma unroll
        for (int u = 0; u < HR; ++u) {
          const float here = next;
          next = __shfl(z[u + 1].x, src, 64);
          const double df = (double)z[u].x - (double)(same ? here : next);
          acc = fma(df, df, acc);
        }
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) acc += __shfl_xor(acc, m, 64);
        if (lane == tau) dshort = acc;
      }
#pragma unroll
      for (int u = 0; u < HR; ++u) e[u] = p[u + HR] - p[u];
      e0 = __shfl(p[HR], 0, 64);                             // P(W) = E(0)
      ew = carry - e0;                                       // E(W) = P(N) - P(W)
      // g enters as 2^sh g with about the frame's energy: G comes out of Z by a difference, so its error is relative to |A|
      const int sh = e0 > 0.0 ? min((ilogb(carry) - ilogb(e0)) / 2, 60) : 0;
      const float up = ldexpf(1.0f, sh);
      back = e0 > 0.0 ? ldexpf(scale, -sh) : 0.0f;          // a silent first half: r = 0, not the transform's rounding
#pragma unroll
      for (int u = 0; u < HR; ++u) z[u].y *= up;
    }

    // ---- r: forward, untangle into conj(G) A, inverse
    fft_forward<R>(z, k, lds_tw1, tr);
    {
      v2f x[R];
#pragma unroll
      for (int u = 0; u < R; ++u) {
        const v2f other = shfl2(z[R - 1 - u], k.partner);
        const v2f pz = lane == 0 ? z[(R - u) % R] : other;   // Z[N - k]
        x[u] = mul_i(cmulc_k(add_conj(z[u], pz), sub_conj(z[u], pz)));
      }
#pragma unroll
      for (int u = 0; u < R; ++u) z[u] = x[u];
    }
    fft_inverse<R>(z, k, lds_tw1, tr);

    // ---- d, c and d'
    float dp[HR + 1];
    {
      double carry = 0.0;
#pragma unroll
      for (int u = 0; u < HR; ++u) {
        const int tau = 64 * u + lane;
        const double d = tau == 0 ? 0.0 : (u == 0 && lane <= kYinDirect) ? dshort : e0 + e[u] - 2.0 * (double)(z[u].x * back);
        const double c = yin_scan(d, lane) + carry;
        carry = __shfl(c, 63, 64);
        dp[u] = (tau != 0 && c > 0.0) ? (float)(d * (double)tau / c) : 1.0f;
      }
      const double d = e0 + ew - 2.0 * (double)(z[HR].x * back);      // tau = W: lane 0's value is the one that counts
      const double c = carry + d;
      dp[HR] = c > 0.0 ? (float)(d * (double)W / c) : 1.0f;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
    for (int u = 0; u < HR; ++u) dps[64 * u + lane] = dp[u];
    if (lane == 0) dps[W] = dp[HR];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");

    const int64_t o = item * a.n_frames + t;
    if (a.cmnd != nullptr) {
      float* __restrict__ row = a.cmnd + o * (int64_t)(W + 1);
#pragma unroll
      for (int u = 0; u < HR; ++u) row[64 * u + lane] = dp[u];
      if (lane == 0) row[W] = dp[HR];
    }

    // ---- the pick: both branches, then one of them
    int tau0 = -1;
    float low = __builtin_inff();
#pragma unroll
    for (int u = 0; u < HR; ++u) {
      const int tau = 64 * u + lane;
      const bool in = tau >= a.tau_min && tau <= a.tau_max;
      yin_first(tau0, __ballot(in && (double)dp[u] < thr), u);
      if (in) low = fminf(low, dp[u]);
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) low = fminf(low, __shfl_xor(low, m, 64));
    int rest = -1, least = -1;
#pragma unroll
    for (int u = 0; u < HR; ++u) {
      const int tau = 64 * u + lane;
      const bool in = tau >= a.tau_min && tau <= a.tau_max;
      const float next = dps[tau + 1];                       // tau + 1 <= W
      const bool stop = tau >= a.tau_max || !(next < dp[u]);
      yin_first(rest, __ballot(in && tau >= tau0 && stop), u);
      yin_first(least, __ballot(in && dp[u] == low), u);
    }
    int pick = tau0 >= 0 ? rest : least;
    pick = pick < a.tau_min ? a.tau_min : pick > a.tau_max ? a.tau_max : pick;      // (NaN input: stay inside the scratch)

    // ---- the refinement
    const double ra = (double)dps[pick - 1], rb = (double)dps[pick], rc = (double)dps[pick + 1];
    const double q = ra - 2.0 * rb + rc, num = ra - rc;
    const double sh = (q > 0.0 && fabs(num) < q) ? num / (2.0 * q) : 0.0;
    if (lane == 0) {
      a.period[o] = (float)((double)pick + sh);
      a.aper[o] = dps[pick];
      if (a.tau != nullptr) a.tau[o] = pick;
    }
  }
}

}  // namespace specinv
