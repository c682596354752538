// The backward pass of gla_projection: the adjoint of P(x; m) = ISTFT(m S / (|S| + 1e-16)), S = STFT(x), with no
// spectrum in device memory.  What proj_adjoint_stages (plan_impl.h) runs as stft_internal(u), stft_internal(x),
// k_misi_proj_adjoint and the inverse transform of grad_from_spec - Y, R and gR each written to and read from HBM - a lane
// group of one wave does here per frame, on kernels_wave.h's transform:
//   1. R: the frame of x, the plan's padding and forward scale                              (analyse<false> into the group's R buffer)
//   2. Y: the frame of u = g / env, divided on load, zero padding, scale 1                  (analyse<true> into its Y buffer)
//   3. the conjugate pairs (k, M - k): real-FFT split of both, k_misi_proj_adjoint's arithmetic per bin - gm written, gR halved
//      on the interior bins - and the inverse split of gR over Y
//   4. the inverse passes, the last one straight to the frames buffer with the forward scale and the window
// launch_grad_fold then overlap-adds the frames and folds the padded margins as it does for every other signal gradient.
// R survives the second transform in a second wave-private piece of LDS (registers would need the pair walk unrolled over all of
// a lane's pairs: DESIGN 3.16 has the numbers).  No atomics: a frame's gm row, gR and synthesis frame have one writer each.
#pragma once
#include <algorithm>
#include <mutex>

#include "kernels_wave.h"
#include "proj_adjoint_api.h"

namespace specinv {

template <typename T>
__global__ void __launch_bounds__(256) k_project(cplx<T>* __restrict__ spec, const T* __restrict__ m, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const cplx<T> s = spec[i];
    const T inv = T(1) / (si_hypot(s.x, s.y) + eps16<T>::value);      // (k_gla_update's operations, in its order)
    spec[i] = mk<T>((s.x * m[i]) * inv, (s.y * m[i]) * inv);
  }
}

namespace wave {

// One frame's M-point transform into `buf`: the first pass from the signal row `xr` (frame start `start`, which may reach into the
// padding), the others through LDS.  DIV: the samples are xr[n] / env[n] inside the signal and 0 outside (the ISTFT adjoint's
// zero-padded frames of g / env); else torch.stft's padding by `pad_mode`.  The window is applied in both.
template <typename T, int LOGM, bool DIV>
__device__ __forceinline__ void analyse(cplx<T>* buf, const cplx<T>* tab1, const cplx<T>* tab2, const cplx<T>* tab3,
                                        const T* __restrict__ xr, const T* __restrict__ env, int64_t start, int64_t length,
                                        int pad_mode, const T* __restrict__ win, int gl) {
  using G = Geo<T, LOGM>;
  using C = cplx<T>;
  constexpr int M = m_of<LOGM>(), N = 2 * M, LG = G::LG, PS = G::R0;
  constexpr int NS1 = G::R0, NS2 = G::R0 * G::R1, NS3 = G::R0 * G::R1 * G::R2;
  constexpr int R = G::R0, NB = M / R, PER = NB / LG;
  static_assert(PER >= 1, "a lane owns at least one butterfly of the first pass");
  const T* xp = xr + start;
  const T* ep = env + start;
  const bool interior = start >= 0 && start + N <= length;
  // (pairs of samples in one load: the frame's first sample - and the envelope's - on a pair boundary)
  const bool aligned = reinterpret_cast<uintptr_t>(xp) % sizeof(C) == 0 && (!DIV || reinterpret_cast<uintptr_t>(ep) % sizeof(C) == 0);
  C v[PER][R];
  if (interior && aligned) {
#pragma unroll
    for (int it = 0; it < PER; ++it)
#pragma unroll
      for (int q = 0; q < R; ++q) {
        const int p = gl + it * LG + q * NB;
        v[it][q] = *reinterpret_cast<const C*>(xp + 2 * p);
        if constexpr (DIV) {
          const C e = *reinterpret_cast<const C*>(ep + 2 * p);
          v[it][q] = mk<T>(v[it][q].x / e.x, v[it][q].y / e.y);
        }
      }
  } else if (interior) {
#pragma unroll
    for (int it = 0; it < PER; ++it)
#pragma unroll
      for (int q = 0; q < R; ++q) {
        const int p = gl + it * LG + q * NB;
        v[it][q] = DIV ? mk<T>(xp[2 * p] / ep[2 * p], xp[2 * p + 1] / ep[2 * p + 1]) : mk<T>(xp[2 * p], xp[2 * p + 1]);
      }
  } else {
    // a frame that reaches into the padding: per sample, in a rolled loop that parks the lane's points in the buffer (k_wave_iter)
    auto at = [&](int64_t n) -> T {
      if constexpr (DIV) return n >= 0 && n < length ? xr[n] / env[n] : T(0);
      else return load_padded(xr, length, n, pad_mode);
    };
#pragma unroll 1
    for (int m = 0; m < M / LG; ++m) {
      const int p = gl + m * LG;
      buf[phys<PS>(p)] = mk<T>(at(start + 2 * p), at(start + 2 * p + 1));
    }
#pragma unroll
    for (int it = 0; it < PER; ++it)
#pragma unroll
      for (int q = 0; q < R; ++q) v[it][q] = buf[phys<PS>(gl + it * LG + q * NB)];
    wave_sync<LG>();          // (a team: `interior` is the frame's, the same for every thread)
  }
#pragma unroll
  for (int it = 0; it < PER; ++it) {
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const C w2 = *reinterpret_cast<const C*>(win + 2 * (gl + it * LG + q * NB));
      v[it][q] = mk<T>(v[it][q].x * w2.x, v[it][q].y * w2.y);
    }
    bfly<T, R, false>(v[it]);
    const int j = gl + it * LG;
#pragma unroll
    for (int i = 0; i < R; ++i) buf[phys<PS>(j * R + i)] = v[it][i];
  }
  wave_sync<LG>();
  pass_lds<T, G::R1, NS1, false, LOGM, LG, PS>(buf, tab1, gl);
  if constexpr (G::NPASS >= 3) pass_lds<T, G::R2, NS2, false, LOGM, LG, PS>(buf, tab2, gl);
  if constexpr (G::NPASS == 4) pass_lds<T, G::R3, NS3, false, LOGM, LG, PS>(buf, tab3, gl);
}

// k_misi_proj_adjoint's arithmetic for one bin of a one-sided spectrum: y the unscaled transform of u, s = R, m the target
template <typename T>
__device__ __forceinline__ cplx<T> proj_adj_bin(cplx<T> y, cplx<T> s, T m, bool interior, T inv_scale, T& gm) {
  const cplx<T> g = interior ? mk<T>(y.x * (2 * inv_scale), y.y * (2 * inv_scale)) : mk<T>(y.x * inv_scale, T(0));
  const T mag = si_hypot(s.x, s.y);
  const T d = mag + eps16<T>::value;
  const T dot = g.x * s.x + g.y * s.y;                     // Re(conj(gQ) R)
  const T c1 = m / d;
  const T c2 = mag > T(0) ? dot * m / (d * d * mag) : T(0);
  cplx<T> gr = mk<T>(g.x * c1 - s.x * c2, g.y * c1 - s.y * c2);
  if (interior) gr = mk<T>(gr.x * T(0.5), gr.y * T(0.5));
  gm = dot / d;
  return gr;
}

// waves per SIMD the registers are held to: a float64 frame and a float32 frame of 16 points per lane take 256 registers
template <typename T, int LOGM>
constexpr int proj_adj_waves_per_simd() {
  return Geo<T, LOGM>::LG > 64 || sizeof(T) == 8 || m_of<LOGM>() / Geo<T, LOGM>::LG >= 16 ? 2 : 4;
}

template <typename T, int LOGM>
__global__ __attribute__((amdgpu_flat_work_group_size(64, 512), amdgpu_waves_per_eu((proj_adj_waves_per_simd<T, LOGM>()))))
void k_wave_proj_adjoint(ProjAdjArgs<T> a) {
  using G = Geo<T, LOGM>;
  using C = cplx<T>;
  constexpr int M = m_of<LOGM>(), N = 2 * M, LG = G::LG;
  constexpr int TEAM = LG > 64 ? LG / 64 : 1;            // waves per frame (a team is a whole workgroup)
  constexpr int FPW = LG > 64 ? 1 : 64 / LG;             // frames per wave
  constexpr int PS = G::R0;
  constexpr int MP = phys<PS>(M) + 1;                    // a frame's points in LDS
  constexpr int NS1 = G::R0, NS2 = G::R0 * G::R1, NS3 = G::R0 * G::R1 * G::R2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using TB = Tabs<T, LOGM>;
  C* tab1 = reinterpret_cast<C*>(smem);                  // pass tables, then W_N^(i LG): k_wave_iter's
  C* tab2 = tab1 + TB::N1;
  C* tab3 = tab2 + TB::N2;
  C* tabs = tab3 + TB::N3;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  const bool lane_on = TEAM > 1 || lane < FPW * LG;
  const int g = TEAM > 1 ? 0 : (lane_on ? lane / LG : 0), gl = TEAM > 1 ? (int)threadIdx.x : lane % LG;
  C* buf = tab1 + TB::TOTAL + (size_t)(TEAM > 1 ? 0 : wave * FPW + g) * (2 * MP);   // Y, then gR
  C* bufr = buf + MP;                                                               // R
  {
    constexpr int ST1 = N / (NS1 * G::R1);
    for (int i = threadIdx.x; i < TB::N1; i += blockDim.x) tab1[i] = a.c.tw[((i % NS1) * (i / NS1 + 1)) * ST1];
    if constexpr (G::NPASS >= 3) {
      constexpr int ST2 = N / (NS2 * G::R2);
      for (int i = threadIdx.x; i < TB::N2; i += blockDim.x) tab2[i] = a.c.tw[((i % NS2) * (i / NS2 + 1)) * ST2];
    }
    if constexpr (G::NPASS == 4) {
      constexpr int ST3 = N / (NS3 * G::R3);
      for (int i = threadIdx.x; i < TB::N3; i += blockDim.x) tab3[i] = a.c.tw[((i % NS3) * (i / NS3 + 1)) * ST3];
    }
    for (int i = threadIdx.x; i < TB::NPAIR; i += blockDim.x) tabs[i] = a.c.tw[i * LG];
  }
  const C wlane = a.c.tw[gl];                            // W_N^gl
  __syncthreads();
  const FrameCfg<T>& c = a.c;
  const int Tn = c.n_frames, F = c.n_freq;
  const int64_t total = (int64_t)a.batch * Tn;
  const int64_t w0 = TEAM > 1 ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
  const int64_t nw = TEAM > 1 ? (int64_t)gridDim.x : (int64_t)gridDim.x * (blockDim.x >> 6);
  const T hs = T(0.5) * c.fwd_scale, inv_scale = c.inv_scale;
  const T* __restrict__ win = c.window;
  // a group of FPW frames per wave and trip; the last group of the launch may be partly filled (a team: FPW = 1, every thread of
  // the workgroup takes the same trips and reaches every barrier)
  for (int64_t ur = w0; ur * FPW < total; ur += nw) {
    const int64_t u = ur * FPW + g;
    if (!(u < total && lane_on)) continue;
    const int fi = (int)u;                          // (host: fewer than 2^31 frames)
    const int bi = (int)((unsigned)fi / (unsigned)Tn);
    const int t = fi - bi * Tn;
    const int fi0 = __builtin_amdgcn_readfirstlane(fi);
    const T* magu = a.mag + (int64_t)fi0 * F;
    T* gmu = a.gmag + (int64_t)fi0 * F;
    const int so = (fi - fi0) * F;
    const int64_t start = (int64_t)t * c.hop - c.pad;
    analyse<T, LOGM, false>(bufr, tab1, tab2, tab3, a.x + (int64_t)bi * c.length, nullptr, start, c.length, c.pad_mode, win, gl);
    analyse<T, LOGM, true>(buf, tab1, tab2, tab3, a.g + (int64_t)bi * c.length, a.env, start, c.length, SPECINV_PAD_CONSTANT, win, gl);
    // ---- the conjugate pairs (k, M - k) of both spectra
    constexpr int NPAIR = (M / 2) / LG;             // k = gl + i LG < M / 2
    constexpr int CH = NPAIR % 2 == 0 ? 2 : 1;      // pairs whose target is requested together
    static_assert(NPAIR % CH == 0 && (M / 2) % LG == 0, "whole chunks of pairs");
#pragma unroll 1
    for (int i0 = 0; i0 < NPAIR; i0 += CH) {
      C ra[CH], rb[CH], ya[CH], yb[CH];
      T ma[CH], mb[CH];
#pragma unroll
      for (int uu = 0; uu < CH; ++uu) {
        const int k = gl + (i0 + uu) * LG;
        const int kb = k == 0 ? M : M - k;          // k = 0 pairs the real bins 0 and M
        ma[uu] = magu[so + k];
        mb[uu] = magu[so + kb];
        ra[uu] = bufr[phys<PS>(k)];
        rb[uu] = bufr[phys<PS>(k == 0 ? 0 : M - k)];
        ya[uu] = buf[phys<PS>(k)];
        yb[uu] = buf[phys<PS>(k == 0 ? 0 : M - k)];
      }
#pragma unroll
      for (int uu = 0; uu < CH; ++uu) {
        const int k = gl + (i0 + uu) * LG;
        const int kb = k == 0 ? M : M - k;
        const C w = (i0 + uu) == 0 ? wlane : cmul(wlane, tabs[i0 + uu]);   // W_N^k
        // the real-FFT split of a transform z with scale 2 h: bins k and kb
        auto split = [&](C za, C zb, T h, C& xk, C& xm) {
          if (k == 0) {
            xk = mk<T>((za.x + za.y) * (2 * h), T(0));
            xm = mk<T>((za.x - za.y) * (2 * h), T(0));
          } else {
            const C bc = conj(zb);
            const C e = mk<T>((za.x + bc.x) * h, (za.y + bc.y) * h);
            const C d = mk<T>((za.x - bc.x) * h, (za.y - bc.y) * h);
            const C wo = cmul(w, mk<T>(d.y, -d.x));   // W^k (-i d)
            xk = e + wo;
            xm = conj(e - wo);
          }
        };
        C rk, rm, yk, ym;
        split(ra[uu], rb[uu], hs, rk, rm);
        split(ya[uu], yb[uu], T(0.5), yk, ym);
        T gk, gmm;
        const C qk = proj_adj_bin<T>(yk, rk, ma[uu], k != 0, inv_scale, gk);
        const C qm = proj_adj_bin<T>(ym, rm, mb[uu], k != 0, inv_scale, gmm);
        gmu[so + k] = gk;
        gmu[so + kb] = gmm;
        if (k == 0) {                               // the Hermitian inverse: the imaginary parts of bins 0 and M do not count
          buf[phys<PS>(0)] = mk<T>(qk.x + qm.x, qk.x - qm.x);
        } else {
          const C p = mk<T>(qk.x + qm.x, qk.y - qm.y);                   // G_k + conj G_{M-k}
          const C q = cmul(mk<T>(qk.x - qm.x, qk.y + qm.y), conj(w));    // (G_k - conj G_{M-k}) conj W^k
          buf[phys<PS>(k)] = mk<T>(p.x - q.y, p.y + q.x);
          buf[phys<PS>(M - k)] = mk<T>(p.x + q.y, q.x - p.y);
        }
      }
    }
    if (gl == 0) {                                  // the one bin that is its own partner: M / 2 (interior)
      const C zr = bufr[phys<PS>(M / 2)], zy = buf[phys<PS>(M / 2)];
      T gmid;
      const C q = proj_adj_bin<T>(mk<T>(zy.x, -zy.y), mk<T>(zr.x * c.fwd_scale, -zr.y * c.fwd_scale), magu[so + M / 2], true, inv_scale, gmid);
      gmu[so + M / 2] = gmid;
      buf[phys<PS>(M / 2)] = mk<T>(T(2) * q.x, T(-2) * q.y);
    }
    // ---- A^T: the passes again with conjugated twiddles, the last one straight to the frames buffer
    wave_sync<LG>();
    pass_lds<T, G::R0, 1, true, LOGM, LG, PS>(buf, tab1, gl);
    if constexpr (G::NPASS >= 3) pass_lds<T, G::R1, NS1, true, LOGM, LG, PS>(buf, tab1, gl);
    if constexpr (G::NPASS == 4) pass_lds<T, G::R2, NS2, true, LOGM, LG, PS>(buf, tab2, gl);
    {
      constexpr int R = G::NPASS == 4 ? G::R3 : G::NPASS == 3 ? G::R2 : G::R1, NS = M / R, NB = M / R, PER = NB / LG;
      static_assert(PER >= 1 && NB % LG == 0, "a lane owns whole butterflies of the last pass");
      const C* tabl = G::NPASS == 4 ? tab3 : G::NPASS == 3 ? tab2 : tab1;
      C v[PER][R];
#pragma unroll
      for (int it = 0; it < PER; ++it) {
        const int j = gl + it * LG;
#pragma unroll
        for (int q = 0; q < R; ++q) v[it][q] = buf[phys<PS>(j + q * NB)];
      }
      T* fru = a.frames + (int64_t)fi0 * N;
      const int fo = (fi - fi0) * N;
#pragma unroll
      for (int it = 0; it < PER; ++it) {
        const int j = gl + it * LG;                 // k = j, blk = 0
#pragma unroll
        for (int q = 1; q < R; ++q) v[it][q] = cmul(v[it][q], tw_get<T, true>(tabl, (q - 1) * NS + j));
        bfly<T, R, true>(v[it]);
#pragma unroll
        for (int i = 0; i < R; ++i) {
          const int p = gl + it * LG + i * NS;      // samples 2 p, 2 p + 1 of the frame
          const C w2 = *reinterpret_cast<const C*>(win + 2 * p);
          *reinterpret_cast<C*>(fru + fo + 2 * p) = mk<T>((v[it][i].x * c.fwd_scale) * w2.x, (v[it][i].y * c.fwd_scale) * w2.y);
        }
      }
      wave_sync<LG>();        // (the next frame's first pass writes the buffers this one still read)
    }
  }
}

// Launch shape: workgroups of four or eight waves (a team: its own), whichever puts more waves on a CU by the runtime's count of
// resident workgroups; the launch fills the chip once and every wave walks its share of the frame groups.
template <typename T, int LOGM>
int proj_adjoint_launch_one(const ProjAdjArgs<T>& a, hipStream_t stream) {
  using G = Geo<T, LOGM>;
  constexpr int M = m_of<LOGM>(), TEAM = G::LG > 64 ? G::LG / 64 : 1, FPW = G::LG > 64 ? 1 : 64 / G::LG, MP = phys<G::R0>(M) + 1;
  const void* fn = (const void*)k_wave_proj_adjoint<T, LOGM>;
  auto lds_of = [](int w) {
    const size_t groups_wg = (size_t)(TEAM > 1 ? 1 : w) * FPW;
    return sizeof(cplx<T>) * ((size_t)Tabs<T, LOGM>::TOTAL + groups_wg * 2 * MP);
  };
  static int n_cu = 0, wpw_s = 0, per_cu_s = 0;
  static std::mutex mu;
  {
    std::lock_guard<std::mutex> lock(mu);
    if (wpw_s == 0) {
      int dev = 0;
      hipDeviceProp_t prop{};
      if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) n_cu = prop.multiProcessorCount;
      if (n_cu <= 0) n_cu = 256;
      (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)std::min<size_t>(lds_of(8), 160 * 1024));
      int best = 0;
      for (int w : {4, 8}) {
        int nb = 0;
        if (TEAM > 1) w = TEAM;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, 64 * w, lds_of(w)) != hipSuccess) nb = 0;
        if (nb * w > best) {
          best = nb * w;
          wpw_s = w;
          per_cu_s = nb;
        }
      }
      (void)hipGetLastError();
      if (wpw_s == 0) {
        wpw_s = TEAM > 1 ? TEAM : 4;
        per_cu_s = 1;
      }
    }
  }
  SI_CHECK(wave_iter_fits(a.c.n_fft, a.c.n_frames, a.batch, false), SPECINV_EUNSUPPORTED,
           "k_wave_proj_adjoint: too many frames for 32-bit frame offsets");
  const int64_t groups = ((int64_t)a.batch * a.c.n_frames + FPW - 1) / FPW;
  int wpw = wpw_s;
  int64_t wgs = std::min<int64_t>(TEAM > 1 ? groups : (groups + wpw - 1) / wpw, (int64_t)n_cu * per_cu_s);
  if (a.max_waves > 0) {                                 // (tests: a small problem makes every wave walk several groups)
    if (TEAM == 1) wpw = std::min(wpw, a.max_waves);
    wgs = std::min<int64_t>(wgs, std::max(1, a.max_waves / wpw));
  }
  wgs = std::max<int64_t>(1, wgs);
  ProjAdjArgs<T> args = a;
  void* kargs[] = {&args};
  SI_HIP(hipLaunchKernel(fn, dim3((unsigned)wgs), dim3(64 * wpw), kargs, lds_of(wpw), stream));
  return SPECINV_OK;
}

}  // namespace wave
}  // namespace specinv
