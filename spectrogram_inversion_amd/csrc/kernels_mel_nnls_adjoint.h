// k_mel_nnls_adjoint: the reverse sweep of k_mel_nnls (kernels_mel_nnls.h) - the gradient of a loss with respect to the mel
// columns, given its gradient with respect to the magnitudes (mel_to_stft_unfolded).
//
// Forward, per frame (step = 1 / L, beta_k the momentum table):   z_0 = s_0 = 0,
//     u_k = z_k - step M^T (M z_k - y),   s_{k+1} = max(0, u_k),   z_{k+1} = s_{k+1} + beta_k (s_{k+1} - s_k),   out = s_n^(1/power).
// The only data-dependent quantities the sweep needs are the active sets [s_{k+1} > 0] and s_n, so nothing is recorded by the
// forward launch: the same wave that owns the frame recomputes the iteration from y (phase 1, k_mel_nnls's arithmetic in
// k_mel_nnls's order, so that the sets are the forward launch's), keeps one ballot word per 64 bins and iteration behind its
// slice in LDS, and sweeps back (phase 2) with the cotangents in the slots the forward quantities leave:
//     sb = G (1/power) s_n^(1/power - 1) where s_n > 0, else 0;   zb = 0;   yb = 0
//     k = n-1 ... 0:   a = sb + (1 + beta_k) zb;   sb = -beta_k zb;   ub = a [s_{k+1} > 0];   q = M ub;   zb = ub - step M^T q;
//                      yb += step q
// (d max(0, u) / du = 0 at u = 0, the root's derivative 0 at s_n = 0: a silent frame and a bin no band touches get exact zeros).
// zb and ub live in z's slot, sb in s's, q in r's, yb in y's (free once phase 1 is done).  HBM is touched for y, G and the
// result alone; no atomics.
//
// A wave's slice: z[F] | s[F] | r[n_mels] | y[n_mels] | part[nseg] | (8-byte aligned) mask[n_iter * ceil(F / 64)] 64-bit words;
// word k * ceil(F / 64) + j holds [s_{k+1}[64 j + lane] > 0] at bit `lane`.
#pragma once
#include "kernels_mel_nnls.h"

namespace specinv {
namespace fast {

template <typename T>
struct MelNnlsAdjointArgs {
  MelNnlsArgs<T> f;           // the forward launch's arguments (y = the mel; out unused)
  const T* g;                 // (B, F, T) cotangent of the magnitudes
  T* gy;                      // (B, n_mels, T) cotangent of the mel
  int nwords;                 // ceil(F / 64)
  int slice_bytes;            // a wave's slice with its mask words
  int mask_off;               // bytes from a slice's start to its mask words
};

template <typename T, bool STAGED>
__global__ __launch_bounds__(64 * kNnlsMaxWaves) void k_mel_nnls_adjoint(MelNnlsAdjointArgs<T> aa);

#if defined(__HIPCC__)
template <typename T, bool STAGED>
__global__ __launch_bounds__(64 * kNnlsMaxWaves) void k_mel_nnls_adjoint(MelNnlsAdjointArgs<T> aa) {
  extern __shared__ __align__(16) unsigned char nnls_adj_lds[];
  const MelNnlsArgs<T>& a = aa.f;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, W = blockDim.x >> 6;
  const T* wr = a.wr;
  const T* wc = a.wc;
  const int4* seg = a.seg;
  const int* rowseg = a.rowseg;
  const int2* col = a.col;
  if constexpr (STAGED) {
    // layout of the stage: wr | wc | seg | col | rowseg, each 16-byte aligned (k_mel_nnls's)
    unsigned char* p = nnls_adj_lds;
    T* swr = reinterpret_cast<T*>(p);
    p += nnls_align16(a.nwr * (int)sizeof(T));
    T* swc = reinterpret_cast<T*>(p);
    p += nnls_align16(a.nwc * (int)sizeof(T));
    int4* sseg = reinterpret_cast<int4*>(p);
    p += 16 * a.nseg;
    int2* scol = reinterpret_cast<int2*>(p);
    p += nnls_align16(8 * a.F);
    int* srow = reinterpret_cast<int*>(p);
    for (int i = threadIdx.x; i < a.nwr; i += blockDim.x) swr[i] = a.wr[i];
    for (int i = threadIdx.x; i < a.nwc; i += blockDim.x) swc[i] = a.wc[i];
    for (int i = threadIdx.x; i < a.nseg; i += blockDim.x) sseg[i] = a.seg[i];
    for (int i = threadIdx.x; i < a.F; i += blockDim.x) scol[i] = a.col[i];
    for (int i = threadIdx.x; i <= a.n_mels; i += blockDim.x) srow[i] = a.rowseg[i];
    wr = swr;
    wc = swc;
    seg = sseg;
    col = scol;
    rowseg = srow;
    __syncthreads();
  }
  unsigned char* const slices = nnls_adj_lds + a.stage_bytes;
  T* const z = reinterpret_cast<T*>(slices + (size_t)w * aa.slice_bytes);
  T* const s = z + a.F;
  T* const r = s + a.F;
  T* const yv = r + a.n_mels;
  T* const part = yv + a.n_mels;
  unsigned long long* const mask = reinterpret_cast<unsigned long long*>(slices + (size_t)w * aa.slice_bytes + aa.mask_off);
  const int F = a.F, NM = a.n_mels, NW = aa.nwords;
  const T step = a.step;
  // part = the row segments' products with z's slot
  auto segments = [&]() {
    for (int q = lane; q < a.nseg; q += 64) {
      const int4 sg = seg[q];
      const T* wp = wr + sg.z;
      const T* zp = z + sg.x;
      T acc0 = T(0), acc1 = T(0);
      int i = 0;
      for (; i + 1 < sg.y; i += 2) {
        acc0 = fma(wp[i], zp[i], acc0);
        acc1 = fma(wp[i + 1], zp[i + 1], acc1);
      }
      if (i < sg.y) acc0 = fma(wp[i], zp[i], acc0);
      part[q] = acc0 + acc1;
    }
  };
  for (int grp = blockIdx.x; grp < a.n_groups; grp += gridDim.x) {
    const int b = grp / a.tgroups, t0 = (grp - b * a.tgroups) * W, t = t0 + w;
    const int nt = min(W, a.frames - t0);
    // ---- phase 1: the forward iteration again, the active sets kept ----
    if (t < a.frames) {
      for (int f = lane; f < F; f += 64) {
        z[f] = T(0);
        s[f] = T(0);
      }
      const T* yp = a.y + (size_t)b * NM * a.frames + t;
      for (int m = lane; m < NM; m += 64) yv[m] = yp[(size_t)m * a.frames];
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      for (int k = 0; k < a.n_iter; ++k) {
        segments();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        for (int m = lane; m < NM; m += 64) {
          T acc = T(0);
          for (int q = rowseg[m]; q < rowseg[m + 1]; ++q) acc += part[q];
          r[m] = acc - yv[m];
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const T beta = (T)a.beta[k];
        unsigned long long* const mk = mask + (size_t)k * NW;
        for (int f = lane; f < F; f += 64) {
          const int2 c = col[f];
          const int m0 = c.x & 0xffff, nc = c.x >> 16;
          const T* wp = wc + c.y;
          const T* rp = r + m0;
          T g = T(0);
          for (int j = 0; j < nc; ++j) g = fma(wp[j], rp[j], g);
          const T sn = fmax(T(0), z[f] - g * step);
          z[f] = sn + beta * (sn - s[f]);
          s[f] = sn;
          // (lanes past F are inactive in the last trip and give zero bits; lane 0 is in every trip)
          const unsigned long long active = __ballot(sn > T(0));
          if (lane == 0) mk[f >> 6] = active;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      }
    }
    __syncthreads();
    // ---- the cotangent in: sb = G d(root)/ds at s_n in s's slot, W neighbouring frames of a bin together (lanes along t) ----
    const T* gp = aa.g + (size_t)b * F * a.frames + t0;
    for (int i = threadIdx.x; i < F * W; i += blockDim.x) {
      const int f = i / W, tt = i - f * W;
      if (tt < nt) {
        T* const sl = reinterpret_cast<T*>(slices + (size_t)tt * aa.slice_bytes) + F + f;
        const T v = *sl, gv = gp[(size_t)f * a.frames + tt];
        *sl = a.root == 1 ? gv : v > T(0) ? (a.root == 2 ? gv * (T(0.5) / sqrt(v)) : gv * (a.inv_power * pow(v, a.inv_power - T(1)))) : T(0);
      }
    }
    __syncthreads();
    // ---- phase 2: the sweep ----
    if (t < a.frames) {
      for (int m = lane; m < NM; m += 64) yv[m] = T(0);
      if (a.n_iter > 0) {
        // k = n - 1 with zb = 0: ub = sb [s_n > 0], sb = 0
        const unsigned long long* const mk = mask + (size_t)(a.n_iter - 1) * NW;
        for (int f = lane; f < F; f += 64) {
          z[f] = (mk[f >> 6] >> lane) & 1ull ? s[f] : T(0);
          s[f] = T(0);
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      for (int k = a.n_iter - 1; k >= 0; --k) {
        // q = M ub; yb += step q
        segments();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        for (int m = lane; m < NM; m += 64) {
          T acc = T(0);
          for (int q = rowseg[m]; q < rowseg[m + 1]; ++q) acc += part[q];
          r[m] = acc;
          yv[m] = fma(step, acc, yv[m]);
        }
        if (k == 0) break;                                      // (z_0 = 0 is a constant: its cotangent goes nowhere)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        // zb = ub - step M^T q, then iteration k - 1's a = sb + (1 + beta) zb, sb = -beta zb, ub = a [s_k > 0]
        const T beta = (T)a.beta[k - 1];
        const unsigned long long* const mk = mask + (size_t)(k - 1) * NW;
        for (int f = lane; f < F; f += 64) {
          const int2 c = col[f];
          const int m0 = c.x & 0xffff, nc = c.x >> 16;
          const T* wp = wc + c.y;
          const T* rp = r + m0;
          T g = T(0);
          for (int j = 0; j < nc; ++j) g = fma(wp[j], rp[j], g);
          const T zb = z[f] - g * step;
          const T av = s[f] + (T(1) + beta) * zb;
          s[f] = -beta * zb;
          z[f] = (mk[f >> 6] >> lane) & 1ull ? av : T(0);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      }
    }
    __syncthreads();
    // ---- the result out: W neighbouring frames of a band together ----
    T* op = aa.gy + (size_t)b * NM * a.frames + t0;
    for (int i = threadIdx.x; i < NM * W; i += blockDim.x) {
      const int m = i / W, tt = i - m * W;
      if (tt < nt) op[(size_t)m * a.frames + tt] = reinterpret_cast<const T*>(slices + (size_t)tt * aa.slice_bytes)[2 * F + NM + m];
    }
    __syncthreads();
  }
}
#endif

}  // namespace fast

// libspecinv's side of specinv_mel_nnls_adjoint / specinv_mel_nnls_adjoint_max_iter (tu_mel_nnls_adjoint.hip)
int mel_nnls_adjoint_run(PlanBase& pl, const void* mel, int n_iter, double power, const void* gmag, void* gmel_out);
int mel_nnls_adjoint_max_iter(PlanBase& pl, int* out);

}  // namespace specinv
