// pYIN: the probabilistic YIN of Mauch & Dixon 2014 on the d' that k_yin writes (kernels_yin.h), two launches.
//   d' is (F, W + 1) float32, F = B T frames, lag 0 ... W, W = 128, 256, 512 or 1024;  1 <= tau_min < tau_max <= W - 1.
//   Troughs.      tau in [tau_min, tau_max] with d'(tau) < d'(tau - 1) and d'(tau) <= d'(tau + 1), compared in float32.  Two
//                 neighbouring lags are never both troughs.
//   Candidates.   For threshold k = 1 ... K, s_k and its weight w_k: the troughs with d'(tau) < s_k (float64) ranked by rising lag,
//                 r = 0, 1, ..., n - 1;  p(tau) += (w_k inv[n]) boltz[r], in rising k, with the host's float64 tables
//                 boltz[r] = (1 - e^-lambda) e^(-lambda r) and inv[n] = 1 / (1 - e^(-lambda n)).  Then the first arg-min trough tau_g
//                 gets q cum[m], m the number of thresholds with d'(tau_g) >= s_k, cum[m] = w_1 + ... + w_m.
//   Observation.  A trough with p > 0: period = tau + shift (k_yin's refinement), bin = rint(scale log2(sample_rate / period / fmin)),
//                 scale = 12 bins_per_semitone, in float64;  a bin below 0 is bin 0, a bin above P - 1 is dropped;  of several
//                 candidates in one bin the largest lag stands.  obs[j] = (float) p or 0;  vprob = clip(sum of the standing p, 0, 1).
//   Decode.       2P states, j < P voiced bin j, P + j unvoiced bin j.  log B_v[j] = log(obs[j] + tiny), log B_u = log((1 - vprob) / P
//                 + tiny);  delta_0 = log(init + tiny) + log B_0 with init = 0 voiced, 1 / P unvoiced;  delta_t[j] = max_i(delta_{t-1}[i]
//                 + log A[i][j]) + log B_t[j], lowest i on ties;  A = [[1 - s, s], [s, 1 - s]] (x) tri(j - i) / Z_i inside
//                 |j - i| <= half, 0 outside, and a 0 enters as log tiny: a floor, not -inf.  The last frame's arg-max (lowest index)
//                 is walked back through the pointers.
//
// k_pyin_obs<C>: a wave owns a frame, four to a workgroup (as k_yin); lane l owns the C = W / 64 consecutive lags [l C, l C + C),
// read with their two neighbours from the wave's LDS copy of the row.  A rank in lag order is then the lane's own count plus an
// exclusive wave scan of the counts.  The K thresholds are a loop whose body is a mask, that scan and one multiply-add per owned
// trough into a float64 accumulator; contraction is off, so the sums are the definition's operation by operation.  tau_g is a wave
// minimum and a wave minimum of lags; m is counted by every lane on the broadcast value.  Collisions: an LDS atomic max of the lag per
// bin, then the lane whose lag stands writes the value; the row goes out in one coalesced sweep, zeros included.  No loop bound
// depends on the data.  LDS: four times (W + 2 + 2 P) words, 48 KiB at the caps.
//
// k_pyin_viterbi: a workgroup of ceil(P / 64) waves (up to 1024 lanes) owns an item and walks its frames; lane j owns bin j in both
// groups.  LDS holds a[i] = (delta_v[i] - log Z_i, delta_u[i] - log Z_i) as pairs, double-buffered, with `half` pairs of -inf on
// the left and half + 8 on the right, so that the band needs no bounds; log tri(kk - half) for the 2 half + 1 taps, padded with -inf
// to whole chunks of eight; -log Z_i; and the waves' arg-max totals.  Per frame a lane
//   (1) requests its observation obs[t][j] and vprob[t];
//   (2) runs the band: M_g[j] = max_{|i - j| <= half} a_g[i] + log tri(j - i) for both groups from one 16-byte read per tap, in
//       chunks of eight taps - inside a chunk only the maximum, between chunks a strict comparison (the earliest chunk stands), then
//       the standing chunk's taps added again for the first that equals the maximum: the same sum, the same bits, the lowest index.
//       (The plain loop that carries the arg-max tap by tap measured 16.7 / 10.6 us a frame against 13.7 / 9.3: EXPERIMENTS.md.)
//   (3) takes for the voiced and for the unvoiced target the best of: stay, switch, and the floor of either group - that group's
//       maximum of delta (lowest index) plus log tiny, which is what every state outside the band offers in the dense definition; an
//       in-band state always beats its own floor, so the floor's arg-max is right whenever it wins;
//   (4) adds log B (log tiny itself for a zero observation), stores the two int16 pointers, writes a for the next frame and folds
//       (delta, index) of both groups over the wave; one barrier; every lane then folds the waves' totals itself.
// After the last frame lane 0 walks the pointers back (a chain of T dependent loads) and writes T int32 states.  Offsets into
// global memory are 64-bit.  LDS: 32 (P + 2 half + 8) + 8 (2 half + 1 rounded up to eights) + 8 P + 768 bytes, 81 KiB at the caps;
// dynamic, raised by attribute.
#pragma once
#include "common.h"

namespace specinv {

constexpr int kPyinWaves = 4;
constexpr int kPyinThreads = 64 * kPyinWaves;
constexpr int kPyinMaxBins = 1024;          // P: 2 P <= 2048 states, int16 pointers, one lane per bin
constexpr int kPyinMaxHalf = 512;           // width = 2 half + 1 <= 1025
constexpr int kPyinMaxThresholds = 1024;
constexpr int kPyinVitMaxWaves = kPyinMaxBins / 64;
constexpr int kPyinChunk = 8;               // taps of the band between two comparisons of the running maximum
constexpr double kPyinTiny = 2.2250738585072014e-308;      // the smallest normal float64

struct PyinObsArgs {
  const float* cmnd;      // (F, W + 1)
  const double* thr;      // s_k, K entries
  const double* wk;       // w_k, K entries
  const double* cum;      // cum[0 ... K]
  const double* boltz;    // n_ranks entries
  const double* inv;      // n_ranks + 1 entries, inv[0] unused
  float* obs;             // (F, P)
  float* vprob;           // (F,)
  int64_t frames;         // F
  int n_thr, tau_min, tau_max, n_bins;
  double sample_rate, fmin, scale, no_trough;
};

constexpr size_t pyin_obs_lds_bytes(int w, int n_bins) { return (size_t)kPyinWaves * 4 * (size_t)(w + 2 + 2 * n_bins); }

template <int C>
__global__ void __launch_bounds__(kPyinThreads) k_pyin_obs(PyinObsArgs a, int64_t block0) {
#pragma clang fp contract(off)
  constexpr int W = 64 * C;
  extern __shared__ __attribute__((aligned(16))) char pyin_smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wib = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int P = a.n_bins;
  float* dps = reinterpret_cast<float*>(pyin_smem) + (size_t)wib * (size_t)(W + 2 + 2 * P);      // d'(0 ... W)
  int* owner = reinterpret_cast<int*>(dps + W + 2);                                                // [P] the lag that stands, 0: none
  float* val = reinterpret_cast<float*>(owner + P);                                                // [P]
  const int64_t fr = (block0 + blockIdx.x) * kPyinWaves + wib;       // the wave's frame; the last workgroup may not be full
  if (fr >= a.frames) return;                                         // (no workgroup barrier below: a wave is on its own)

  const float* __restrict__ row = a.cmnd + fr * (int64_t)(W + 1);
  for (int i = lane; i <= W; i += 64) dps[i] = row[i];
  for (int i = lane; i < P; i += 64) owner[i] = 0;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();

  // ---- the lane's lags with their neighbours, the troughs, tau_g
  float d[C + 2];
#pragma unroll
  for (int j = 0; j < C + 2; ++j) {
    const int i = lane * C - 1 + j;                                  // -1 only for lag 0, which is never in the range
    d[j] = dps[i < 0 ? 0 : i];
  }
  bool tr[C];
  double dd[C], acc[C];
  float low = __builtin_inff();
#pragma unroll
  for (int j = 0; j < C; ++j) {
    const int tau = lane * C + j;
    tr[j] = tau >= a.tau_min && tau <= a.tau_max && d[j + 1] < d[j] && d[j + 1] <= d[j + 2];
    dd[j] = (double)d[j + 1];
    acc[j] = 0.0;
    if (tr[j]) low = fminf(low, d[j + 1]);
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) low = fminf(low, __shfl_xor(low, m, 64));
  int tau_g = 0x7fffffff;
#pragma unroll
  for (int j = C - 1; j >= 0; --j)
    if (tr[j] && d[j + 1] == low) tau_g = lane * C + j;
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) tau_g = min(tau_g, __shfl_xor(tau_g, m, 64));
  const double dg = (double)low;                                     // +inf where the frame has no trough: m stays 0

  // ---- the thresholds
  int m_g = 0;
  for (int k = 0; k < a.n_thr; ++k) {
    const double s = a.thr[k];
    bool hit[C];
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < C; ++j) {
      hit[j] = tr[j] && dd[j] < s;
      cnt += hit[j] ? 1 : 0;
    }
    int incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    const int n = __shfl(incl, 63, 64);
    m_g += dg >= s ? 1 : 0;
    if (n > 0) {
      const double f = a.wk[k] * a.inv[n];
      int r = incl - cnt;
#pragma unroll
      for (int j = 0; j < C; ++j) {
        if (hit[j]) {
          acc[j] = acc[j] + f * a.boltz[r];
          ++r;
        }
      }
    }
  }
  if (tau_g != 0x7fffffff) {
    const double extra = a.no_trough * a.cum[m_g];
#pragma unroll
    for (int j = 0; j < C; ++j)
      if (lane * C + j == tau_g) acc[j] = acc[j] + extra;
  }

  // ---- bins: the largest lag of a bin stands
  int bin[C];
#pragma unroll
  for (int j = 0; j < C; ++j) {
    bin[j] = -1;
    if (tr[j] && acc[j] > 0.0) {
      const int tau = lane * C + j;
      const double ra = (double)d[j], rb = dd[j], rc = (double)d[j + 2];
      const double q = ra - 2.0 * rb + rc, num = ra - rc;
      const double sh = (q > 0.0 && fabs(num) < q) ? num / (2.0 * q) : 0.0;
      const double period = (double)tau + sh;
      double b = rint(a.scale * log2(a.sample_rate / period / a.fmin));
      if (b < 0.0) b = 0.0;
      if (b <= (double)(P - 1)) {                                    // (NaN: dropped)
        bin[j] = (int)b;
        atomicMax(&owner[bin[j]], tau);
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  double vsum = 0.0;
#pragma unroll
  for (int j = 0; j < C; ++j) {
    if (bin[j] >= 0 && owner[bin[j]] == lane * C + j) {
      val[bin[j]] = (float)acc[j];
      vsum = vsum + acc[j];
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) vsum = vsum + __shfl_xor(vsum, m, 64);
  float* __restrict__ out = a.obs + fr * (int64_t)P;
  for (int i = lane; i < P; i += 64) out[i] = owner[i] != 0 ? val[i] : 0.0f;
  if (lane == 0) a.vprob[fr] = (float)(vsum < 0.0 ? 0.0 : vsum > 1.0 ? 1.0 : vsum);
}

struct PyinVitArgs {
  const float* obs;       // (B, T, P)
  const float* vprob;     // (B, T)
  const double* ltri;     // log tri(0 ... half)
  const double* nlz;      // -log Z_i, P entries
  int16_t* backptr;       // (B, T, 2 P) scratch; frame 0's row is not used
  int32_t* states;        // (B, T)
  int64_t* ticks;         // (B, 3) wall-clock ticks at an item's start, before the walk back and at its end, or nullptr
  int64_t batch, n_frames;
  int n_bins, half;
  double l_stay, l_switch, l_tiny;       // log(1 - s), log s, log tiny
};

constexpr size_t pyin_vit_lds_bytes(int n_bins, int half) {
  return 32 * (size_t)(n_bins + 2 * half + kPyinChunk) + 8 * (size_t)((2 * half + kPyinChunk) / kPyinChunk * kPyinChunk) +
         8 * (size_t)n_bins + 768;
}

struct PyinBest {
  double v;
  int i;
};
// the larger value; among equals the lower index
__device__ __forceinline__ void pyin_take(PyinBest& b, double v, int i) {
  if (v > b.v || (v == b.v && i < b.i)) {
    b.v = v;
    b.i = i;
  }
}
__device__ __forceinline__ PyinBest pyin_wave_best(PyinBest b) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const double ov = __shfl_xor(b.v, m, 64);
    const int oi = __shfl_xor(b.i, m, 64);
    pyin_take(b, ov, oi);
  }
  return b;
}

// TICKS: the variant that also reads the wall clock into a.ticks (tools/bench_pyin.py)
template <bool TICKS>
__global__ void __launch_bounds__(kPyinMaxBins) k_pyin_viterbi(PyinVitArgs a) {
#pragma clang fp contract(off)
  constexpr double kInf = __builtin_inf();
  extern __shared__ __attribute__((aligned(16))) double pyin_lds[];
  const int P = a.n_bins, half = a.half;
  const int n_tap8 = (2 * half + kPyinChunk) / kPyinChunk * kPyinChunk;      // 2 half + 1 taps, rounded up to whole chunks
  const int stride = P + 2 * half + kPyinChunk;                            // the pad on the right also covers the last chunk
  const int NW = (int)(blockDim.x >> 6);
  double2* abuf = reinterpret_cast<double2*>(pyin_lds);                  // [2][stride], bin i at half + i
  double* tap = pyin_lds + 4 * (size_t)stride;                           // [n_tap8]: log tri(kk - half), -inf past the band
  double* nlz = tap + n_tap8;                                            // [P]
  double* tot_v = nlz + P;                                               // [2][16][2]: frame parity, wave, group
  int* tot_i = reinterpret_cast<int*>(tot_v + 4 * kPyinVitMaxWaves);     // [2][16][2]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool own = tid < P;
  const int j = own ? tid : 0;                                           // a lane past the last bin computes bin 0 and stores nothing
  const int64_t T_ = a.n_frames;
  const double unif = 1.0 / (double)P;

  for (int i = tid; i < n_tap8; i += blockDim.x) tap[i] = i <= 2 * half ? a.ltri[i < half ? half - i : i - half] : -kInf;
  for (int i = tid; i < P; i += blockDim.x) nlz[i] = a.nlz[i];
  for (int i = tid; i < 2 * half + kPyinChunk; i += blockDim.x) {
    const int at = i < half ? i : P + i;
    abuf[at] = make_double2(-kInf, -kInf);
    abuf[stride + at] = make_double2(-kInf, -kInf);
  }
  __syncthreads();
  const double my_nlz = nlz[j];

  // a for the next frame and this frame's maxima, into the buffers of parity `par`
  auto publish = [&](int par, double dv, double du) {
    if (own) abuf[par * stride + half + j] = make_double2(dv + my_nlz, du + my_nlz);
    PyinBest bv = {own ? dv : -kInf, own ? j : 0x7fffffff}, bu = {own ? du : -kInf, own ? j : 0x7fffffff};
    bv = pyin_wave_best(bv);
    bu = pyin_wave_best(bu);
    if (lane == 0) {
      const int at = (par * kPyinVitMaxWaves + wave) * 2;
      tot_v[at] = bv.v;
      tot_v[at + 1] = bu.v;
      tot_i[at] = bv.i;
      tot_i[at + 1] = bu.i;
    }
  };
  auto totals = [&](int par, PyinBest& gv, PyinBest& gu) {
    gv = PyinBest{-kInf, 0x7fffffff};
    gu = gv;
    for (int w = 0; w < NW; ++w) {
      const int at = (par * kPyinVitMaxWaves + w) * 2;
      pyin_take(gv, tot_v[at], tot_i[at]);
      pyin_take(gu, tot_v[at + 1], tot_i[at + 1]);
    }
  };

  for (int64_t item = blockIdx.x; item < a.batch; item += gridDim.x) {
    const float* __restrict__ obs = a.obs + item * T_ * P;
    const float* __restrict__ vp = a.vprob + item * T_;
    int16_t* __restrict__ bp = a.backptr + item * T_ * (2 * (int64_t)P);
    int32_t* __restrict__ st = a.states + item * T_;
    if (TICKS && tid == 0) a.ticks[item * 3] = (int64_t)wall_clock64();

    {  // frame 0: no voiced state to start from
      const double o = (double)obs[j];
      const double lbu = log((1.0 - (double)vp[0]) / (double)P + kPyinTiny);
      publish(0, a.l_tiny + (o == 0.0 ? a.l_tiny : log(o + kPyinTiny)), log(unif + kPyinTiny) + lbu);
    }
    __syncthreads();

    for (int64_t t = 1; t < T_; ++t) {
      const int cur = (int)((t - 1) & 1), nxt = (int)(t & 1);
      const float o_f = obs[t * P + j];                                // in flight during the band
      const float vp_f = vp[t];
      PyinBest gv, gu;
      totals(cur, gv, gu);
      const double2* __restrict__ base = abuf + cur * stride + j;      // base[kk]: bin j - half + kk
      // the band in chunks of eight taps: only maxima inside a chunk, a strict comparison between chunks (the earliest chunk
      // stands), then the first tap of the standing chunk that gives the maximum - the same sum, so the same bits
      double mv = -kInf, mu = -kInf;
      int iv = 0, iu = 0;
      for (int k0 = 0; k0 < n_tap8; k0 += kPyinChunk) {
        double cv = -kInf, cu = -kInf;
#pragma unroll
        for (int q = 0; q < kPyinChunk; ++q) {
          const double lt = tap[k0 + q];
          const double2 av = base[k0 + q];
          const double sv = av.x + lt, su = av.y + lt;
          cv = sv > cv ? sv : cv;
          cu = su > cu ? su : cu;
        }
        if (cv > mv) {
          mv = cv;
          iv = k0;
        }
        if (cu > mu) {
          mu = cu;
          iu = k0;
        }
      }
      {
        const int cv0 = iv, cu0 = iu;
#pragma unroll
        for (int q = kPyinChunk - 1; q >= 0; --q) {
          if (base[cv0 + q].x + tap[cv0 + q] == mv) iv = cv0 + q;
          if (base[cu0 + q].y + tap[cu0 + q] == mu) iu = cu0 + q;
        }
      }
      iv += j - half;
      iu += P + j - half;
      const double fv = gv.v + a.l_tiny, fu = gu.v + a.l_tiny;
      PyinBest tv = {mv + a.l_stay, iv}, tu = {mv + a.l_switch, iv};
      pyin_take(tv, mu + a.l_switch, iu);
      pyin_take(tu, mu + a.l_stay, iu);
      pyin_take(tv, fv, gv.i);
      pyin_take(tu, fv, gv.i);
      pyin_take(tv, fu, P + gu.i);
      pyin_take(tu, fu, P + gu.i);
      const double lbv = o_f == 0.0f ? a.l_tiny : log((double)o_f + kPyinTiny);      // (most bins of a frame observe nothing)
      const double lbu = log((1.0 - (double)vp_f) / (double)P + kPyinTiny);
      if (own) {
        bp[t * (2 * (int64_t)P) + j] = (int16_t)tv.i;
        bp[t * (2 * (int64_t)P) + P + j] = (int16_t)tu.i;
      }
      publish(nxt, tv.v + lbv, tu.v + lbu);
      __syncthreads();
    }

    // the last frame's arg-max, then the walk back
    PyinBest gv, gu;
    totals((int)((T_ - 1) & 1), gv, gu);
    __threadfence();
    __syncthreads();
    if (tid == 0) {
      if (TICKS) a.ticks[item * 3 + 1] = (int64_t)wall_clock64();
      const auto inside = [P](int s) { return s < 0 ? 0 : s > 2 * P - 1 ? 2 * P - 1 : s; };      // (NaN input: stay inside the row)
      int s = inside(gv.v >= gu.v ? gv.i : gu.i < P ? P + gu.i : 0);
      st[T_ - 1] = s;
      for (int64_t t = T_ - 1; t >= 1; --t) {
        s = inside(bp[t * (2 * (int64_t)P) + s]);
        st[t - 1] = s;
      }
      if (TICKS) a.ticks[item * 3 + 2] = (int64_t)wall_clock64();
    }
    __syncthreads();
  }
}

}  // namespace specinv
