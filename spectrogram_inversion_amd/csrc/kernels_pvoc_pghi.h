// The phase vocoder with heap-integrated phase (Prusa & Holighaus 2017, "phase vocoder done right", in this package's
// frame-resampling vocoder): identity locking (kernels_pvoc_lock.h) in which a bin's owner is the root of its magnitude-ordered
// heap chain and a root's phase continues from the locked phase of the previous output frame.  One-sided S (B, F, T_in) complex,
// F = n_fft / 2 + 1, -> P (B, F, T_out).  t_j, i, a, S0 = S[i], S1 = S[i+1] (zeros at and beyond T_in), adv, wrap, d_j as in
// kernels_pvoc.h; theta0 = arg S0 and theta1 = arg S1 in the input's dtype, widened; everything after them float64 for both
// dtypes, contraction off (the comparisons are the definition's, operation by operation):
//   q(z) = re re + im im from the input's own bits ;  r(z) = sqrt(q(z)) ;  m_j[k] = fl(fl(a r(S1[k])) + fl(fl(1 - a) r(S0[k])))
//   floor = tol * sqrt(max q over the item's input) ;  (j,k) live iff m_j[k] > 0 and m_j[k] >= floor
//   Frame 0:  psi_0 = theta0 ;  code 0 where live, 3 elsewhere.
//   Frame j >= 1:  c[k] = m_j[k] if live else -inf ;  p[k] = m_{j-1}[k] if (j-1,k) is live else -inf ;
//     Lf[0] = -inf, Lf[k] = min(c[k-1], max(p[k-1], Lf[k-1])) ;  Rg[F-1] = -inf, Rg[k] = min(c[k+1], max(p[k+1], Rg[k+1])) ;
//     live bin, b = max(p, Lf, Rg):  code 0 if p >= b (time wins ties, and when all three are -inf), else 1 if Lf >= b, else 2 ;
//     not live: 3 ;  phi_j[k] = psi_{j-1}[k] + d_{j-1}[k] (every bin, one addition) ;
//     root(k) = k for codes 0 and 3, root(k+1) for code 2 (resolved first), root(k-1) for code 1 ;
//     psi_j[k] = phi_j[k] if root(k) = k, else (phi_j[root] - theta0_j[root]) + theta0_j[k].
//   P[j][k] = (m cos psi, m sin psi), rounded once.
//
// k_pvoc_pghi<T, NT, K> is k_pghi's form (kernels_pghi.h, whose clamp and segment scans it uses as they are): a workgroup of NT
// lanes owns an item and walks its output frames, items beyond the grid are looped over, lane t owns the K consecutive bins
// [t K, t K + K), K = ceil(F / NT) made odd, every loop over the chunk unrolled.
//   Pre-pass.  One coalesced sweep over the item's input for max q.
//   State, in registers across frames, K each: phi_j = psi_{j-1} + d_{j-1} (added at the end of frame j-1: d_{j-1} is kept in it),
//     p (m_{j-1} or -inf) ; theta and r of the two source frames.
//     There is no window in LDS: LDS holds the scans' totals and the pre-pass reduction, 512 bytes.
//   Sources.  theta and r are made once per source frame: when i advances by one, frame i+1's pair moves to frame i's registers
//     and only S[i+2] is read; when i stays, nothing is read; otherwise both frames are read.  The read for output frame j + 1
//     is requested at the top of frame j and converted (atan2, sqrt) at its end.  In float64 at K = 13 (F > 2816) the second read
//     of a frame that skips a source frame (rate > 1) is requested at the frame's end instead: held across the frame its 4 K
//     registers no longer fit the 512 and the kernel would spill.  The reads are strided by T_in along frequency.
//   Per frame.  (1) m_j of the lane's bins ; (2) the two clamp scans and the codes, as k_pghi ; (3) a segmented suffix pass,
//     then a segmented prefix pass that carry the root's offset phi[root] - theta0[root] instead of a sum: a root contributes its
//     offset, a chained bin 0.0, and adding 0.0 is exact ; (4) sincos_phase (the library's float64 sincos: psi grows by up to
//     pi hop per frame) and the stores.
//   Barriers per frame: 3, one before each read of the scans' totals (clamps up and down together, suffix, prefix).  Each of the
//     three total arrays is written before its own barrier and read before the next one, so no array is rewritten until two
//     further barriers have passed: k_pghi's two rotation barriers have no counterpart.  Frame 0 has none; one more per item
//     (the pre-pass reduction) and one at the item's end.
//   No atomics and nothing device-wide.  float64 inputs whose q overflows or underflows (|z| beyond about 1e150) are out of scope.
#pragma once
#include "kernels_pghi.h"
#include "kernels_pvoc.h"

namespace specinv {

struct PvocPghiArgs {
  int64_t batch;
  int n_freq, n_in, n_out, n_fft, hop;
  double rate, tol;
};

template <typename T, int NT, int K>
__global__ void __launch_bounds__(NT) k_pvoc_pghi(const cplx<T>* __restrict__ in, cplx<T>* __restrict__ out,
                                                  int8_t* __restrict__ parents_out, PvocPghiArgs a) {
#pragma clang fp contract(off)
  constexpr int NW = NT / 64;
  constexpr bool kLate = sizeof(T) == 8 && K >= 13;   // see "Sources"
  constexpr double kInf = __builtin_inf();
  constexpr double two_pi = 6.283185307179586476925286766559;
  // bytes [0, 64) clamp totals up, [64, 128) down, [128, 192) suffix offsets, [256, 320) prefix offsets, [384, 416) the reduction
  __shared__ double lds[64];
  PghiClamp* tot_up = reinterpret_cast<PghiClamp*>(lds);
  PghiClamp* tot_dn = tot_up + 4;
  PghiSeg* tot_sfx = reinterpret_cast<PghiSeg*>(lds + 16);
  PghiSeg* tot_pfx = reinterpret_cast<PghiSeg*>(lds + 32);
  double* red_v = lds + 48;
  static_assert(NW <= 4, "the totals are laid out for four waves");

  const int F = a.n_freq, Tin = a.n_in, Tout = a.n_out;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = tid * K < F ? tid * K : F;
  const int m1 = m0 + K < F ? m0 + K : F;

  for (int64_t item = blockIdx.x; item < a.batch; item += gridDim.x) {
    const cplx<T>* src = in + item * F * Tin;
    const int64_t total = (int64_t)F * Tin;
    double mq = 0.0;
#pragma unroll 8
    for (int64_t e = tid; e < total; e += NT) {
      const cplx<T> z = src[e];
      const double x = (double)z.x, y = (double)z.y;
      const double q = x * x + y * y;
      if (q > mq) mq = q;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mq = fmax(mq, __shfl_xor(mq, off, 64));
    if (NW > 1) {
      if (lane == 0) red_v[wave] = mq;
      __syncthreads();
      mq = red_v[0];
      for (int w = 1; w < NW; ++w) mq = fmax(mq, red_v[w]);
    }
    const double floor_ = a.tol * sqrt(mq);

    // theta and r of source frame `fr` for the lane's bins; a frame at or beyond T_in is +0 + 0i
    // (the lane's address moves with the frame and the bins' strides j T are uniform: K addresses held across the frame loop
    // would cost 2 K registers here and 4 K more at the stores)
    auto request = [&](int fr, cplx<T>(&z)[K]) {
      const cplx<T>* col = src + (int64_t)m0 * Tin + fr;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        z[j] = mk<T>(T(0), T(0));
        if (m0 + j < m1 && fr < Tin) z[j] = col[(int64_t)j * Tin];
      }
    };
    auto convert = [&](const cplx<T>(&z)[K], double(&th)[K], double(&r)[K]) {
#pragma clang fp contract(off)
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const double x = (double)z[j].x, y = (double)z[j].y;
        th[j] = (double)pvoc_angle(z[j].x, z[j].y);
        r[j] = sqrt(x * x + y * y);
      }
    };

    double th0[K], r0[K], th1[K], r1[K];
    double psi[K], p[K];                                // psi: phi_n at the top of frame n, psi_n from (3) on
    {
      cplx<T> z0[K], z1[K];
      request(0, z0);
      request(1, z1);
      convert(z0, th0, r0);
      convert(z1, th1, r1);
    }
    int i = 0;
    for (int n = 0; n < Tout; ++n) {
      const double t = (double)n * a.rate;
      const double w1 = t - floor(t), w0 = 1.0 - w1;
      // the sources of frame n + 1, in flight during the frame (n + 1 < Tout keeps its i below Tin)
      int step = 0;
      cplx<T> za[K], zb[K];
      if (n + 1 < Tout) {
        const int inext = (int)floor((double)(n + 1) * a.rate);
        step = inext - i;
        if (step >= 1) request(inext + 1, zb);
        if (step > 1 && !kLate) request(inext, za);
        i = inext;
      }
      // (1) the frame's magnitudes
      auto mag = [&](int j) {
#pragma clang fp contract(off)
        return w1 * r1[j] + w0 * r0[j];
      };
      unsigned live = 0;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const double mj = mag(j);
        if (m0 + j < m1 && mj > 0.0 && mj >= floor_) live |= 1u << j;
      }
      int cd[K];
      if (n == 0) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
          psi[j] = th0[j];
          cd[j] = (live >> j) & 1 ? 0 : 3;
        }
      } else {
        // the chunk's clamps; a slot past the item's last bin holds the identity clamp
        double c[K], v[K];
#pragma unroll
        for (int j = 0; j < K; ++j) {
          c[j] = (live >> j) & 1 ? mag(j) : -kInf;
          if (m0 + j >= m1) {
            c[j] = kInf;
            p[j] = -kInf;
          }
        }
        // (2) the clamps folded upwards and downwards, scanned; the recurrences through the chunk; the parents
        const PghiClamp ident = {-kInf, kInf};
        PghiClamp up = ident, dn = ident;
#pragma unroll
        for (int j = 0; j < K; ++j) {
          up.lo = pghi_apply(c[j], p[j], up.lo);
          up.hi = pghi_apply(c[j], p[j], up.hi);
        }
#pragma unroll
        for (int j = K - 1; j >= 0; --j) {
          dn.lo = pghi_apply(c[j], p[j], dn.lo);
          dn.hi = pghi_apply(c[j], p[j], dn.hi);
        }
        up = pghi_wave_scan<true>(up, lane);
        dn = pghi_wave_scan<false>(dn, lane);
        if (NW > 1) {
          if (lane == 63) tot_up[wave] = up;
          if (lane == 0) tot_dn[wave] = dn;
          __syncthreads();
        }
        double x = pghi_exclusive<true, NW>(up, tot_up, ident, lane, wave).lo;      // Lf[m0]
        double y = pghi_exclusive<false, NW>(dn, tot_dn, ident, lane, wave).lo;     // Rg[m1 - 1]
#pragma unroll
        for (int j = 0; j < K; ++j) {
          v[j] = x;                                     // Lf, until (3)
          x = pghi_apply(c[j], p[j], x);
        }
#pragma unroll
        for (int j = K - 1; j >= 0; --j) {
          cd[j] = 3;
          if ((live >> j) & 1) {
            const double b = fmax(p[j], fmax(v[j], y));
            cd[j] = p[j] >= b ? 0 : v[j] >= b ? 1 : 2;
          }
          y = pghi_apply(c[j], p[j], y);
        }
        // (3) the offset of every root (a dead bin's is never read), 0.0 in the chains; chains of code 2 take theirs from the
        // right, then chains of code 1 from the left
#pragma unroll
        for (int j = 0; j < K; ++j) v[j] = cd[j] == 1 || cd[j] == 2 ? 0.0 : psi[j] - th0[j];
        const PghiSeg none = {0.0, 0};
        PghiSeg seg = none;
#pragma unroll
        for (int j = K - 1; j >= 0; --j) {
          if (m0 + j < m1) {
            PghiSeg e;
            e.sum = v[j];
            e.root = cd[j] != 2;
            seg = pghi_after(e, seg);
          }
        }
        seg = pghi_wave_scan<false>(seg, lane);
        if (NW > 1) {
          if (lane == 0) tot_sfx[wave] = seg;
          __syncthreads();
        }
        double run = pghi_exclusive<false, NW>(seg, tot_sfx, none, lane, wave).sum;
#pragma unroll
        for (int j = K - 1; j >= 0; --j) {
          if (m0 + j < m1) {
            if (cd[j] == 2) {
              run = run + v[j];
              v[j] = run;
            } else {
              run = v[j];
            }
          }
        }
        seg = none;
#pragma unroll
        for (int j = 0; j < K; ++j) {
          if (m0 + j < m1) {
            PghiSeg e;
            e.sum = v[j];
            e.root = cd[j] != 1;
            seg = pghi_after(e, seg);
          }
        }
        seg = pghi_wave_scan<true>(seg, lane);
        if (NW > 1) {
          if (lane == 63) tot_pfx[wave] = seg;
          __syncthreads();
        }
        run = pghi_exclusive<true, NW>(seg, tot_pfx, none, lane, wave).sum;
#pragma unroll
        for (int j = 0; j < K; ++j) {
          if (m0 + j < m1) {
            run = cd[j] == 1 ? run + v[j] : v[j];
            if (cd[j] == 1 || cd[j] == 2) psi[j] = run + th0[j];
          }
        }
      }
      // (4) the outputs, and the state frame n + 1 reads: p, and phi_{n+1} from this frame's increment d_n
      unsigned codes = 0;                               // (two bits a bin: K registers fewer through the sincos)
#pragma unroll
      for (int j = 0; j < K; ++j) codes |= (unsigned)cd[j] << (2 * j);
      // (values the compiler would otherwise keep in 2 K registers each across the frame, or across the frame loop: the magnitudes
      // of (1), and adv, which does not depend on the frame.  Made again from an opaque copy, they are the same bits.)
      double w1b = w1;
      int mb = m0;
      asm volatile("" : "+v"(w1b), "+v"(mb));
      const double w0b = 1.0 - w1b;
      const int64_t at0 = (item * F + m0) * Tout + n;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const int m = m0 + j;
        const double mj = w1b * r1[j] + w0b * r0[j];
        if (m < m1) {
          double sn, cs;
          sincos_phase(psi[j], &sn, &cs);
          (out + at0)[(int64_t)j * Tout] = mk<T>((T)(mj * cs), (T)(mj * sn));
          if (parents_out) (parents_out + at0)[(int64_t)j * Tout] = (int8_t)((codes >> (2 * j)) & 3u);
        }
        p[j] = (live >> j) & 1 ? mj : -kInf;
        const double adv = two_pi * (double)(mb + j) * (double)a.hop / (double)a.n_fft;
        double d = th1[j] - th0[j] - adv;
        d = d - two_pi * rint(d / two_pi);
        d = d + adv;
        psi[j] = psi[j] + d;                            // phi_{n+1} = psi_n + d_n
      }
      if (step > 1 && kLate) request(i, za);
      if (step == 1) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
          th0[j] = th1[j];
          r0[j] = r1[j];
        }
        convert(zb, th1, r1);
      } else if (step > 1) {
        convert(za, th0, r0);
        convert(zb, th1, r1);
      }
    }
    __syncthreads();                                    // (the next item's reduction writes what a slower wave may still read)
  }
}

}  // namespace specinv
