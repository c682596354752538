// Mask-based beamforming (Souden et al. 2010 for the reference-channel MVDR, the eigenvector form after
// torchaudio's rtf_power, the multichannel Wiener filter): per item and bin two mask-weighted C x C covariance sums over all
// frames, a small Hermitian solve and an inner product per frame.  One launch; one WAVE owns an (item, bin) and is a workgroup of
// its own (kBfWaves = 1 ships; up to four independent waves a workgroup were measured: with more, the LDS of a 16-channel
// workgroup leaves a CU fewer waves), no workgroup barrier anywhere, the grid is looped.
//   X is (B, C, F, T); per (item, f), with x_t = X[:, f, t], m / n the target / noise mask (n = 1 - m when none is given):
//     Phi(m)  = sum_t m_t x_t x_t^H / max(sum_t m_t, tiny)                      tiny = the smallest normal double
//     load(A) = A + (diag_load Re tr(A) / C + tiny) I
//     souden:     A = load(Phi_n); N = A^-1 Phi_s; w = N[:, ref] / max(Re tr(N), tiny)
//     rtf_power:  A, N as above; v = N[:, ref]; (n_power_iter - 1) times v <- N (v / max(|Re v|_inf, |Im v|_inf, tiny));
//                 a = A v; w = v conj(a[ref]) / max(Re(a^H v), tiny)
//     mwf:        A = load(Phi_s + mu Phi_n); w = A^-1 Phi_s[:, ref]
//     Y[f, t] = w^H x_t
//   Everything is float64 for complex64 input as well; Y is rounded once.
//
// The passes of a wave:
//   Sums.    The frames are walked in tiles of kBfTile = 64.  For the loads the lane is the frame: every channel's row is one
//            coalesced read, held in registers and written to the wave's LDS tile (in the input's own type; rows kBfTile + 1
//            elements apart, so that the rows of one frame fall on different banks) while the next tile's loads are in flight.
//            For the sums the lane is an entry (row, col) of both matrices: with P the power of two >= C, P P entries and
//            64 / (P P) slices that take every (64 / (P P))-th frame of a tile (C <= 8: k_beamform<T, 1>); beyond 8 channels a
//            lane owns four neighbouring columns of one row and there is one slice (k_beamform<T, 4>).  x comes from LDS as
//            broadcasts, the masks too; Phi_s, Phi_n and the two mask sums stay in float64 registers over the whole walk, the
//            products by explicit fma in a fixed order.  The slices are summed by an xor butterfly.  The mapping depends on C
//            alone: item b of a batch, the item alone, and every mode give the same bits.
//   Store.   The lower triangle is kept, the upper is its conjugate and the diagonal real: Phi is exactly Hermitian.
//   Solve.   A = U D U^H in LDS (the square-root-free Cholesky, pivots floored at tiny), U y = B, z = D^-1 y, U^H N = z: the
//            steps of kernels_wpe.h's solve, on one wave with wave-level synchronisation.  The short serial sums (traces, the
//            power iteration's norm, a^H v) are run by every lane alike.
//   Apply.   The lane is the frame again: Y = sum_c conj(w_c) x_c in channel order by explicit fma - the same instructions
//            whether w was just solved or handed in (the filter-only mode), hence the same bits.  The second read of X follows
//            the first closely.
// Modes by NULL pointers (specinv_beamform): full; covariance only (no out, no w); filter only (w_in given, no masks).
// LDS of a wave (doubles): Phi_s 2 C C | Phi_n 2 C C | A 2 C C | B / N 2 C C | w 2 C | v 2 C | a 2 C | 1 / pivot C || m 64 | n 64 |
// tile C (64 + 1) elements of the input's type.  34.1 KiB a wave at C 16 in complex128, 9.5 KiB at C 8 in complex64.
// No atomics, no communication between waves.  All global offsets are 64-bit.
#pragma once
#include "common.h"

namespace specinv {

#ifndef SPECINV_BEAMFORM_WAVES
#define SPECINV_BEAMFORM_WAVES 1        // independent waves a workgroup (measured, tools/log/EXPERIMENTS.md)
#endif
constexpr int kBfWaves = SPECINV_BEAMFORM_WAVES;
constexpr int kBfThreads = 64 * kBfWaves;
static_assert(kBfWaves >= 1 && kBfWaves <= 4, "a wave's LDS is sized for up to four a workgroup at 16 channels");
constexpr int kBfTile = 64;             // frames a tile holds: the lane is the frame (beamform.py: TILE)
constexpr int kBfRow = kBfTile + 1;     // a channel's row in the LDS tile, in elements
constexpr int kBfMaxChannels = 16;      // (beamform.py: MAX_CHANNELS)
constexpr int kBfNarrowChannels = 8;    // up to here an entry a lane; beyond, four
constexpr int kBfMaxPowerIter = 64;     // (beamform.py: MAX_POWER_ITER)
constexpr int kBfMaxGrid = 8192;        // workgroups of a launch; the problems beyond are looped over
constexpr double kBfTiny = 2.2250738585072014e-308;

struct BfArgs {
  const void* spec;        // (B, C, F, T) cplx<T>
  const double* mask_t;    // (B, F, T) or nullptr: all ones
  const double* mask_n;    // (B, F, T) or nullptr: 1 - mask_t
  const void* w_in;        // (B, F, C) complex double or nullptr; given: the filter-only mode
  void* out;               // (B, F, T) cplx<T> or nullptr: the covariance-only mode
  void* w_out;             // (B, F, C) complex double or nullptr
  void* scm_t;             // (B, F, C, C) complex double or nullptr
  void* scm_n;             // (B, F, C, C) complex double or nullptr
  int64_t batch, n_freq, n_frames;
  int channels, solution, ref, n_power_iter;
  double diag_load, mu;
};

// the wave's LDS layout, offsets in doubles
struct BfGeom {
  int oS, oN, oA, oB, oW, oV, oU, oInv, oMt, oMn, oTile, wave_doubles;
};

__host__ __device__ inline BfGeom bf_geom(int C, int elem_bytes) {
  BfGeom g;
  const int cc = 2 * C * C;
  g.oS = 0;
  g.oN = cc;
  g.oA = 2 * cc;
  g.oB = 3 * cc;
  g.oW = 4 * cc;
  g.oV = g.oW + 2 * C;
  g.oU = g.oV + 2 * C;
  g.oInv = g.oU + 2 * C;
  g.oMt = g.oInv + ((C + 1) & ~1);
  g.oMn = g.oMt + kBfTile;
  g.oTile = g.oMn + kBfTile;
  const int tile_doubles = (C * kBfRow * 2 * elem_bytes + 7) / 8;
  g.wave_doubles = (g.oTile + tile_doubles + 1) & ~1;
  return g;
}

__device__ __forceinline__ void bf_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// N = A^-1 B in the wave's LDS: A (C x C, the lower triangle is read and destroyed), B (C x nr) is replaced
__device__ __forceinline__ void bf_solve(cplx<double>* sA, cplx<double>* sB, double* invd, int C, int nr, int lane) {
#pragma clang fp contract(off)
  // A = U D U^H: column j keeps M[i][j] = U[i][j] D[j], the diagonal D[j]
  for (int j = 0; j < C; ++j) {
    const double inv = 1.0 / fmax(sA[j * C + j].x, kBfTiny);
    if (lane == 0) invd[j] = inv;
    const int k = j + 1 + (lane & 15);
    for (int i = j + 1 + (lane >> 4); i < C; i += 4) {
      if (k <= i) {
        const cplx<double> m = sA[i * C + j], mk_ = sA[k * C + j];
        const double lx = m.x * inv, ly = m.y * inv;
        cplx<double> r = sA[i * C + k];
        r.x = fma(-lx, mk_.x, r.x);
        r.x = fma(-ly, mk_.y, r.x);
        r.y = fma(-ly, mk_.x, r.y);
        r.y = fma(lx, mk_.y, r.y);
        sA[i * C + k] = r;
      }
    }
    bf_sync();
  }
  // U y = B
  for (int j = 0; j + 1 < C; ++j) {
    const double inv = invd[j];
    for (int idx = lane; idx < (C - 1 - j) * nr; idx += 64) {
      const int i = j + 1 + idx / nr, c = idx % nr;
      const cplx<double> m = sA[i * C + j], y = sB[j * nr + c];
      const double ux = m.x * inv, uy = m.y * inv;
      cplx<double> p = sB[i * nr + c];
      p.x = fma(-ux, y.x, p.x);
      p.x = fma(uy, y.y, p.x);
      p.y = fma(-ux, y.y, p.y);
      p.y = fma(-uy, y.x, p.y);
      sB[i * nr + c] = p;
    }
    bf_sync();
  }
  // z = D^-1 y
  for (int idx = lane; idx < C * nr; idx += 64) {
    const double inv = invd[idx / nr];
    const cplx<double> p = sB[idx];
    sB[idx] = mk<double>(p.x * inv, p.y * inv);
  }
  bf_sync();
  // U^H N = z
  for (int i = C - 1; i >= 1; --i) {
    for (int idx = lane; idx < i * nr; idx += 64) {
      const int j = idx / nr, c = idx % nr;
      const cplx<double> m = sA[i * C + j], gi = sB[i * nr + c];
      const double inv = invd[j];
      const double ux = m.x * inv, uy = m.y * inv;      // conj(u) gi
      cplx<double> p = sB[j * nr + c];
      p.x = fma(-ux, gi.x, p.x);
      p.x = fma(-uy, gi.y, p.x);
      p.y = fma(-ux, gi.y, p.y);
      p.y = fma(uy, gi.x, p.y);
      sB[j * nr + c] = p;
    }
    bf_sync();
  }
}

// w (sW) from Phi_s (sS) and Phi_n (sN), all in the wave's LDS
__device__ __forceinline__ void bf_weights(const BfArgs& a, const BfGeom& g, double* lds, int lane) {
#pragma clang fp contract(off)
  const int C = a.channels, ref = a.ref;
  const cplx<double>* const sS = (const cplx<double>*)(lds + g.oS);
  const cplx<double>* const sN = (const cplx<double>*)(lds + g.oN);
  cplx<double>* const sA = (cplx<double>*)(lds + g.oA);
  cplx<double>* const sB = (cplx<double>*)(lds + g.oB);
  cplx<double>* const sW = (cplx<double>*)(lds + g.oW);
  cplx<double>* const sV = (cplx<double>*)(lds + g.oV);
  cplx<double>* const sU = (cplx<double>*)(lds + g.oU);
  double* const invd = lds + g.oInv;
  const bool mwf = a.solution == SPECINV_BEAMFORM_MWF;
  const int nr = mwf ? 1 : C;
  // A, its trace (every lane the same sum, in index order) and the loading
  double tr = 0.0;
  for (int i = 0; i < C; ++i) {
    const double s = sS[i * C + i].x, n = sN[i * C + i].x;
    tr = tr + (mwf ? s + a.mu * n : n);
  }
  const double load = a.diag_load * tr / (double)C + kBfTiny;
  for (int idx = lane; idx < C * C; idx += 64) {
    const int i = idx / C, j = idx - i * C;
    const cplx<double> s = sS[idx], n = sN[idx];
    cplx<double> v = mwf ? mk<double>(s.x + a.mu * n.x, s.y + a.mu * n.y) : n;
    if (i == j) v = mk<double>(v.x + load, 0.0);
    sA[idx] = v;
    if (!mwf) sB[idx] = s;
  }
  if (mwf && lane < C) sB[lane] = sS[lane * C + ref];
  bf_sync();
  bf_solve(sA, sB, invd, C, nr, lane);
  if (mwf) {
    if (lane < C) sW[lane] = sB[lane];
  } else if (a.solution == SPECINV_BEAMFORM_SOUDEN) {
    double trn = 0.0;
    for (int i = 0; i < C; ++i) trn = trn + sB[i * C + i].x;
    const double den = fmax(trn, kBfTiny);
    if (lane < C) {
      const cplx<double> v = sB[lane * C + ref];
      sW[lane] = mk<double>(v.x / den, v.y / den);
    }
  } else {
    if (lane < C) sV[lane] = sB[lane * C + ref];
    bf_sync();
    for (int it = 1; it < a.n_power_iter; ++it) {
      double s = kBfTiny;
      for (int j = 0; j < C; ++j) s = fmax(s, fmax(fabs(sV[j].x), fabs(sV[j].y)));
      cplx<double> acc = mk<double>(0.0, 0.0);
      if (lane < C) {
        for (int j = 0; j < C; ++j) {
          const cplx<double> v = sV[j], n = sB[lane * C + j];
          const double vx = v.x / s, vy = v.y / s;
          acc.x = fma(n.x, vx, acc.x);
          acc.x = fma(-n.y, vy, acc.x);
          acc.y = fma(n.x, vy, acc.y);
          acc.y = fma(n.y, vx, acc.y);
        }
      }
      bf_sync();                                         // every lane has read the old v
      if (lane < C) sV[lane] = acc;
      bf_sync();
    }
    // a = A v with the loaded Phi_n (A itself was factored in place)
    if (lane < C) {
      cplx<double> acc = mk<double>(0.0, 0.0);
      for (int j = 0; j < C; ++j) {
        const cplx<double> v = sV[j];
        cplx<double> n = sN[lane * C + j];
        if (j == lane) n = mk<double>(n.x + load, 0.0);
        acc.x = fma(n.x, v.x, acc.x);
        acc.x = fma(-n.y, v.y, acc.x);
        acc.y = fma(n.x, v.y, acc.y);
        acc.y = fma(n.y, v.x, acc.y);
      }
      sU[lane] = acc;
    }
    bf_sync();
    double d = 0.0;
    for (int i = 0; i < C; ++i) {
      const cplx<double> u = sU[i], v = sV[i];
      d = fma(u.x, v.x, d);
      d = fma(u.y, v.y, d);
    }
    const double den = fmax(d, kBfTiny);
    if (lane < C) {
      const cplx<double> v = sV[lane], ar = sU[ref];       // v conj(a[ref])
      const double px = fma(v.x, ar.x, v.y * ar.y), py = fma(v.y, ar.x, -(v.x * ar.y));
      sW[lane] = mk<double>(px / den, py / den);
    }
  }
  bf_sync();
}

// NE entries of Phi_s and Phi_n a lane: 1 up to kBfNarrowChannels channels, 4 beyond
template <typename T, int NE>
__global__ __launch_bounds__(kBfThreads) void k_beamform(const BfArgs a) {
#pragma clang fp contract(off)
  static_assert(NE == 1 || NE == 4, "an entry a lane, or four");
  constexpr int CMAX = NE == 1 ? kBfNarrowChannels : kBfMaxChannels;
  extern __shared__ __attribute__((aligned(16))) double bf_lds[];
  const int C = a.channels;
  const int lane = threadIdx.x & 63;
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const BfGeom g = bf_geom(C, (int)sizeof(T));
  double* const lds = bf_lds + (size_t)wib * g.wave_doubles;
  cplx<double>* const sS = (cplx<double>*)(lds + g.oS);
  cplx<double>* const sN = (cplx<double>*)(lds + g.oN);
  cplx<double>* const sW = (cplx<double>*)(lds + g.oW);
  double* const sMt = lds + g.oMt;
  double* const sMn = lds + g.oMn;
  cplx<T>* const tile = (cplx<T>*)(lds + g.oTile);
  const int64_t nT = a.n_frames, F = a.n_freq;
  const int64_t cs = F * nT, nprob = a.batch * F;

  // the lane's entries: (row, col0 ... col0 + NE - 1) of slice `slice` of nsl
  int row, col0, slice, nsl, pp;
  if (NE == 1) {
    int lg = 0;
    while ((1 << lg) < C) ++lg;
    pp = 1 << (2 * lg);
    const int e = lane & (pp - 1);
    slice = lane >> (2 * lg);
    nsl = 64 >> (2 * lg);
    row = e >> lg;
    col0 = e & ((1 << lg) - 1);
  } else {
    pp = 64;
    row = lane >> 2;
    col0 = (lane & 3) * NE;
    slice = 0;
    nsl = 1;
  }
  const int rr = row < C ? row : C - 1;                  // (an entry beyond the matrix: computed on the last one, never stored)
  int cc[NE];
#pragma unroll
  for (int k = 0; k < NE; ++k) cc[k] = col0 + k < C ? col0 + k : C - 1;

  for (int64_t prob = (int64_t)blockIdx.x * kBfWaves + wib; prob < nprob; prob += (int64_t)gridDim.x * kBfWaves) {
    const int64_t item = prob / F, f = prob - item * F;
    const cplx<T>* const x = (const cplx<T>*)a.spec + (item * C * F + f) * nT;
    if (a.w_in != nullptr) {
      if (lane < C) sW[lane] = ((const cplx<double>*)a.w_in)[prob * C + lane];
      bf_sync();
    } else {
      // ---- the sums
      const double* const mt = a.mask_t != nullptr ? a.mask_t + prob * nT : nullptr;
      const double* const mn = a.mask_n != nullptr ? a.mask_n + prob * nT : nullptr;
      double sr[NE], si[NE], nr_[NE], ni[NE], msum = 0.0, nsum = 0.0;
#pragma unroll
      for (int k = 0; k < NE; ++k) sr[k] = si[k] = nr_[k] = ni[k] = 0.0;
      cplx<T> nx[CMAX];
      double nm = 0.0, nn = 0.0;
      auto request = [&](int64_t tb) {
        const int64_t t = tb + lane;
        const bool in = t < nT;
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
          nx[c] = mk<T>((T)0, (T)0);
          if (c < C && in) nx[c] = x[c * cs + t];
        }
        nm = nn = 0.0;
        if (in) {
          nm = mt != nullptr ? mt[t] : 1.0;
          nn = mn != nullptr ? mn[t] : 1.0 - nm;
        }
      };
      request(0);
      for (int64_t tb = 0; tb < nT; tb += kBfTile) {
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
          if (c < C) tile[c * kBfRow + lane] = nx[c];
        sMt[lane] = nm;
        sMn[lane] = nn;
        bf_sync();
        if (tb + kBfTile < nT) request(tb + kBfTile);     // in flight during the sums
        const int len = nT - tb < kBfTile ? (int)(nT - tb) : kBfTile;
        for (int tl = slice; tl < len; tl += nsl) {
          const double m = sMt[tl], n = sMn[tl];
          const cplx<T> xr = tile[rr * kBfRow + tl];
          const double xx = (double)xr.x, xy = (double)xr.y;
          const double ux = m * xx, uy = m * xy, vx = n * xx, vy = n * xy;
#pragma unroll
          for (int k = 0; k < NE; ++k) {                  // u conj(x_col)
            const cplx<T> xc = tile[cc[k] * kBfRow + tl];
            const double cx = (double)xc.x, cy = (double)xc.y;
            sr[k] = fma(ux, cx, sr[k]);
            sr[k] = fma(uy, cy, sr[k]);
            si[k] = fma(uy, cx, si[k]);
            si[k] = fma(-ux, cy, si[k]);
            nr_[k] = fma(vx, cx, nr_[k]);
            nr_[k] = fma(vy, cy, nr_[k]);
            ni[k] = fma(vy, cx, ni[k]);
            ni[k] = fma(-vx, cy, ni[k]);
          }
          msum = msum + m;
          nsum = nsum + n;
        }
        bf_sync();                                        // the tile's reads are over
      }
      if (NE == 1) {
        for (int off = pp; off < 64; off <<= 1) {         // the slices
          sr[0] = sr[0] + __shfl_xor(sr[0], off, 64);
          si[0] = si[0] + __shfl_xor(si[0], off, 64);
          nr_[0] = nr_[0] + __shfl_xor(nr_[0], off, 64);
          ni[0] = ni[0] + __shfl_xor(ni[0], off, 64);
          msum = msum + __shfl_xor(msum, off, 64);
          nsum = nsum + __shfl_xor(nsum, off, 64);
        }
      }
      // ---- Phi: the lower triangle, its conjugate above, a real diagonal
      const double dm = fmax(msum, kBfTiny), dn = fmax(nsum, kBfTiny);
      cplx<double>* const gs = a.scm_t != nullptr ? (cplx<double>*)a.scm_t + prob * C * C : nullptr;
      cplx<double>* const gn = a.scm_n != nullptr ? (cplx<double>*)a.scm_n + prob * C * C : nullptr;
#pragma unroll
      for (int k = 0; k < NE; ++k) {
        const int col = col0 + k;
        if (slice == 0 && row < C && col <= row) {
          const bool diag = col == row;
          const cplx<double> ps = mk<double>(sr[k] / dm, diag ? 0.0 : si[k] / dm);
          const cplx<double> pn = mk<double>(nr_[k] / dn, diag ? 0.0 : ni[k] / dn);
          sS[row * C + col] = ps;
          sN[row * C + col] = pn;
          if (gs != nullptr) gs[row * C + col] = ps;
          if (gn != nullptr) gn[row * C + col] = pn;
          if (!diag) {
            sS[col * C + row] = conj(ps);
            sN[col * C + row] = conj(pn);
            if (gs != nullptr) gs[col * C + row] = conj(ps);
            if (gn != nullptr) gn[col * C + row] = conj(pn);
          }
        }
      }
      bf_sync();
      if (a.out == nullptr && a.w_out == nullptr) continue;      // the covariance-only mode
      bf_weights(a, g, lds, lane);
      if (a.w_out != nullptr && lane < C) ((cplx<double>*)a.w_out)[prob * C + lane] = sW[lane];
    }
    if (a.out == nullptr) continue;
    // ---- Y = w^H x
    double wx[CMAX], wy[CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
      const cplx<double> w = sW[c < C ? c : 0];
      wx[c] = w.x;
      wy[c] = w.y;
    }
    cplx<T>* const y = (cplx<T>*)a.out + prob * nT;
    for (int64_t t = lane; t < nT; t += kBfTile) {
      cplx<T> xv[CMAX];
#pragma unroll
      for (int c = 0; c < CMAX; ++c) {
        xv[c] = mk<T>((T)0, (T)0);
        if (c < C) xv[c] = x[c * cs + t];
      }
      double re = 0.0, im = 0.0;
#pragma unroll
      for (int c = 0; c < CMAX; ++c) {
        if (c < C) {
          const double cx = (double)xv[c].x, cy = (double)xv[c].y;
          re = fma(wx[c], cx, re);
          re = fma(wy[c], cy, re);
          im = fma(wx[c], cy, im);
          im = fma(-wy[c], cx, im);
        }
      }
      y[t] = mk<T>((T)re, (T)im);
    }
    bf_sync();                                            // before the next problem's writes to w
  }
}

}  // namespace specinv
