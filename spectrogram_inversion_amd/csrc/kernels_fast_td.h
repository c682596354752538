// Griffin-Lim on the fused shapes with the momentum carried as a signal: fused_td_body and its two launch forms (k_fused4_td for the
// headline shapes, k_fused_td<R, OV> for every other overlap).  Built on fast_core.h (the wave-level FFT, the block loaders load_block /
// load_block4, FastArgs); compiled in tu_td_*.hip; the host side is FastState<float>::launch_td (fast_state.h).
#pragma once
#include "fast_core.h"

namespace specinv {
namespace fast {

// ---- Griffin-Lim with the momentum carried in the time domain (every fused shape: hop = n_fft/2, /4, /8) ---------------------
// methods.py:243-244 keep pre_t = STFT(x_t) - lr * pre_{t-1}, a (B, F, T) complex array read and written every iteration
// (16 F of the 8 hop + 20 F bytes a frame-iteration moves).  The STFT (padding included) is linear, so
//     pre_t = STFT(z_t) + (-lr)^t * c0,     z_t = x_t - lr * z_{t-1},  z_0 = 0,
// with c0 the starting spectrum: the recursion can run on the (B, L) signal z instead.  This kernel transforms z_t's
// frames (one forward FFT, as before), adds the geometrically vanishing c0 term while it is above 2^-30 (EARLY: c0 is read,
// never written), projects, synthesises x_{t+1} and writes z_{t+1} = x_{t+1} - lr * z_t next to it: the hop-block of z_t that
// an output block needs is the oldest block of the frame just analysed, still in registers.  Per frame-iteration: 4 hop (z in)
// + 4 F (target) + 8 hop (z, x out) instead of 8 hop + 20 F bytes; the same arithmetic up to the rounding of where the linear
// combination is taken (time domain here, frequency domain in the reference).  The evaluating variant transforms x_t's frames
// as well (|STFT(x_t)| is what the metric wants, methods.py:242).
//   a.x_in / a.x_out  : z_t / z_{t+1}          a.x2_in / a.x2_out : x_t (EVAL only) / x_{t+1} (nullptr: not wanted)
//   a.xtail_in / _out : chunk seams, shared by x and z (the - lr * z_t term goes to the block's owner)
//   a.P_in, a.Pmid_in : c0 pairs (EARLY)        a.tds : (-lr)^t

template <bool FIRST, typename A, typename B>
__device__ __forceinline__ const auto& td_pick(const A& a, const B& b) {
  if constexpr (FIRST) return a;
  else return b;
}


// one hop-block of the sample window (the tuned n_fft/4 copy of the loader where it applies)
template <int R, int OV, bool NT = false>
__device__ __forceinline__ void td_load_block(const float* __restrict__ xrow, const float* __restrict__ tailrow, long long L,
                                              int T, int c, int t_begin, int t_end, int j, int lane, int pad_mode,
                                              v2f (&q)[R / OV]) {
  if constexpr (OV == 4) load_block4<R, NT>(xrow, tailrow, L, T, c, t_begin, t_end, j, lane, pad_mode, q);
  else load_block<R, OV>(xrow, tailrow, L, T, c, t_begin, t_end, j, lane, pad_mode, q);
}

// ---- the n_fft 2048 transform as this file's kernels run it ----------------------------------------------------------------------
// The same butterflies on the same values as fft_forward_t / fft_inverse_t<16> (fast_core.h), bit for bit, written for a frame loop
// that is bound by the vector instructions it issues:
//   * the one +-i rotation of the radix-16 (W_16^4 on a[10]) rides on the source modifiers of the two packed adds that read it
//     instead of a v_xor + v_mov in front of them;
//   * the transpose scratch is addressed from two per-lane LDS pointers.  The strided side (the rows a 16-lane row owns, up to
//     8 KiB apart) goes through volatile accesses: one ds_read_b64 / ds_write_b64 each with the distance in the 16-bit offset
//     field - left to the compiler's pairing into ds_read2 / ds_write2, whose offsets hold 8 bits, every pair gets a v_add_u32 of
//     its own to re-base it.  The contiguous side pairs up within 8 bits of a pointer the compiler cannot fold the table's base
//     into (td_scratch).  16 vector instructions per transform pair for 16 more LDS instructions; same rows, same pads.  The
//     forward transform's single writes are free of bank conflicts like the pairs were; the inverse's 16 single reads are 2-way
//     conflicted (the two 16-lane rows of a 32-lane read group lie 34 elements apart; a ds_read2_b64 serves 16 lanes at a time
//     and never met that): SQ_LDS_BANK_CONFLICT 0 -> 32 cycles per frame, measured WITH the gain this form brings
//     (profiles/frame_loop_trim.json).  Written through `tr` these reads pair up again - but `tr` is __restrict__ and the
//     writes just before go through sc.b: every access of the n_fft 2048 path must stay on the two TdScratch pointers.
// The other sizes, and the kernels of the other translation units, keep the shared text.
using lds_v2f = __attribute__((address_space(3))) v2f;
struct TdScratch {
  volatile lds_v2f* q;     // tr + k.tr_q: the strided side
  lds_v2f* b;              // tr + k.tr_b: the contiguous side
};
template <int R>
__device__ __forceinline__ TdScratch td_scratch(v2f* tr, const LaneConst<R>& k) {
  TdScratch s;
  s.q = (volatile lds_v2f*)(tr + k.tr_q);
  s.b = (lds_v2f*)(tr + k.tr_b);
  asm volatile("" : "+v"(s.b));     // (opaque: the contiguous side's 16 offsets count from this register)
  return s;
}

// dft4 of (a0, a1, rot<INV>(a2), a3)
template <bool INV>
__device__ __forceinline__ void dft4_rot2(v2f& a0, v2f& a1, v2f& a2, v2f& a3) {
  const v2f t0 = INV ? add_i(a0, a2) : sub_i(a0, a2);
  const v2f t1 = INV ? sub_i(a0, a2) : add_i(a0, a2);
  const v2f t2 = a1 + a3, d = a1 - a3;
  a0 = t0 + t2;
  a2 = t0 - t2;
  a1 = INV ? add_i(t1, d) : sub_i(t1, d);
  a3 = INV ? sub_i(t1, d) : add_i(t1, d);
}
// Dft<16, INV, true>::run
template <bool INV>
__device__ __forceinline__ void td_dft16(v2f (&a)[16]) {
  constexpr float c1 = 0.92387953251128675613f, s1 = 0.38268343236508977173f, h = 0.70710678118654752440f;
#pragma unroll
  for (int n0 = 0; n0 < 4; ++n0) dft4<INV>(a[n0], a[n0 + 4], a[n0 + 8], a[n0 + 12]);
  dirmul_x4<INV, true>(a[5], a[6], a[7], a[9], v2f{c1, -s1}, v2f{h, -h}, v2f{s1, -c1}, v2f{h, -h});
  dirmul_x4<INV, true>(a[11], a[13], a[14], a[15], v2f{-h, -h}, v2f{s1, -c1}, v2f{-h, -h}, v2f{-c1, s1});
  dft4<INV>(a[0], a[1], a[2], a[3]);
  dft4<INV>(a[4], a[5], a[6], a[7]);
  dft4_rot2<INV>(a[8], a[9], a[10], a[11]);
  dft4<INV>(a[12], a[13], a[14], a[15]);
  v2f o[16];
#pragma unroll
  for (int k0 = 0; k0 < 4; ++k0)
#pragma unroll
    for (int k1 = 0; k1 < 4; ++k1) o[k1 + 4 * k0] = a[k0 + 4 * k1];
#pragma unroll
  for (int i = 0; i < 16; ++i) a[i] = o[i];
}

template <int R, typename TW>
__device__ __forceinline__ void td_fft_forward(v2f (&z)[R], const LaneConst<R>& k, const TW& tw, v2f* __restrict__ tr,
                                               const TdScratch& sc) {
  if constexpr (R == 16) {
    td_dft16<false>(z);
    cmul_all<R, true, false, 1>(z, tw);
#pragma unroll
    for (int g = 0; g < R; g += 4) xlane_dft4_in<false>(z[g], z[g + 1], z[g + 2], z[g + 3]);
#pragma unroll
    for (int g = 0; g < R; g += 4) {
      z[g + 2] = cmul(z[g + 2], k.postq[0]);
      z[g + 1] = cmul(z[g + 1], k.postq[1]);
      z[g + 3] = cmul(z[g + 3], k.postq[2]);
    }
#pragma unroll
    for (int g = 0; g < R; g += 4) {
      sc.q[(0 * R + g) * (R + 1)] = z[g];
      sc.q[(1 * R + g) * (R + 1)] = z[g + 2];
      sc.q[(2 * R + g) * (R + 1)] = z[g + 1];
      sc.q[(3 * R + g) * (R + 1)] = z[g + 3];
    }
#pragma unroll
    for (int i = 0; i < R; ++i) z[i] = sc.b[i];
    td_dft16<false>(z);
  } else {
    fft_forward_t<R>(z, k, tw, tr);
  }
}
template <int R, typename TW>
__device__ __forceinline__ void td_fft_inverse(v2f (&z)[R], const LaneConst<R>& k, const TW& tw, v2f* __restrict__ tr,
                                               const TdScratch& sc) {
  if constexpr (R == 16) {
    td_dft16<true>(z);
#pragma unroll
    for (int i = 0; i < R; ++i) sc.b[i] = z[i];
#pragma unroll
    for (int g = 0; g < R; g += 4) {
      z[g] = sc.q[(0 * R + g) * (R + 1)];
      z[g + 2] = sc.q[(1 * R + g) * (R + 1)];
      z[g + 1] = sc.q[(2 * R + g) * (R + 1)];
      z[g + 3] = sc.q[(3 * R + g) * (R + 1)];
    }
#pragma unroll
    for (int g = 0; g < R; g += 4) {
      z[g + 2] = cmulc(z[g + 2], k.postq[0]);
      z[g + 1] = cmulc(z[g + 1], k.postq[1]);
      z[g + 3] = cmulc(z[g + 3], k.postq[2]);
    }
#pragma unroll
    for (int g = 0; g < R; g += 4) xlane_dft4_out<true>(z[g], z[g + 1], z[g + 2], z[g + 3]);
    cmul_all<R, true, true, 1>(z, tw);
    td_dft16<true>(z);
  } else {
    fft_inverse_t<R>(z, k, tw, tr);
  }
}

// Lane 0 of the conjugate-partner exchange is its own partner: after the shuffle it takes eight values of its own.  Written as
// eight 64-bit moves under exec = 1 (saved and restored around them) instead of sixteen selects on a lane mask; the values are the
// same.  Only called in uniform control flow with all lanes active.
__device__ __forceinline__ void td_lane0_mov8(v2f& d0, v2f& d1, v2f& d2, v2f& d3, v2f& d4, v2f& d5, v2f& d6, v2f& d7, v2f s0, v2f s1,
                                              v2f s2, v2f s3, v2f s4, v2f s5, v2f s6, v2f s7) {
  unsigned long long saved;
  asm("s_mov_b64 %8, exec\n\t"
      "s_mov_b64 exec, 1\n\t"
      "v_mov_b64 %0, %9\n\t"
      "v_mov_b64 %1, %10\n\t"
      "v_mov_b64 %2, %11\n\t"
      "v_mov_b64 %3, %12\n\t"
      "v_mov_b64 %4, %13\n\t"
      "v_mov_b64 %5, %14\n\t"
      "v_mov_b64 %6, %15\n\t"
      "v_mov_b64 %7, %16\n\t"
      "s_mov_b64 exec, %8"
      : "+v"(d0), "+v"(d1), "+v"(d2), "+v"(d3), "+v"(d4), "+v"(d5), "+v"(d6), "+v"(d7), "=&s"(saved)
      : "v"(s0), "v"(s1), "v"(s2), "v"(s3), "v"(s4), "v"(s5), "v"(s6), "v"(s7));
}

template <int R, int OV, bool EARLY, bool EVAL>
__device__ __forceinline__ void fused_td_body(const FastArgs& a) {
  using G = Geo<R>;
  using O = Ovl<R, OV>;
  constexpr int H = G::H, M = G::M, QU = O::QU, HOP = O::HOP, NB = O::NB, PB = O::PB;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // The synthesis window carries the inverse transform's scale (a second table): one multiplication less per bin pair in the
  // projection; 1 / n_fft is a power of two, so nothing changes in the result (normalized=True never takes this kernel when the
  // reference's operation chain is asked for: FastState::begin_t).
  v2f* lds_win = reinterpret_cast<v2f*>(smem);
  v2f* lds_wins = lds_win + M;
  v2f* lds_tw1 = lds_win + 2 * M;      // (Geo::lds_bytes_td)
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  v2f* tr = lds_tw1 + (R - 1) * 64 + wib * G::TR;

  WinRegs<M> wreg;
  win_request<M>(a.window, wreg);      // (in flight while the twiddles are built)
  for (int i = threadIdx.x; i < (R - 1) * 64; i += blockDim.x) {
    const int k1 = i / 64 + 1, l = i & 63;
    lds_tw1[i] = unit(2.0f * (float)((l * k1) % M) / (float)M);   // W_M^(l*k1)
  }
  win_store<M>(wreg, lds_win, lds_wins, a.inv_scale);
  __syncthreads();

  int w = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + wib);   // (scalar: the frame loop and its padding tests branch on the scalar unit; left to the compiler the work-group size may arrive in a vector register and make all of it per-lane)
  if (a.skew == 0 && w >= a.n_waves) return;     // (skewed chunks: the test follows the mapping, which permutes inside a workgroup)
  const LaneConst<R> k = lane_consts<R>();
  const TdScratch tsc = td_scratch<R>(tr, k);
  const int lane = k.lane;
  const unsigned ulane = (unsigned)lane;
  // Even chunks: wave w walks chunk w mod nchunks of item w / nchunks.  Skewed chunks (a launch of exactly two waves per SIMD):
  // the older wave of a SIMD, which the arbiter serves first - it runs 1.7 x as fast as its neighbour while both are there -
  // takes the even (longer) chunk of a pair, the younger the odd one.  In 8-wave workgroups (the headline shape) the role is the
  // wave's index in the workgroup / 4.  In 4-wave workgroups (the other overlaps) it is inferred from the dispatch order: the
  // dispatcher hands every CU its first workgroup before any gets a second, so the first half of the waves are the older ones
  // (1024 of 1024 in every wave dump of DESIGN 3.2; a launch placed differently is merely less balanced).  (Drawing the chunk
  // by the slot actually occupied, with two atomic counters, balanced the waves to 4 % - and cost more in 1024 same-address
  // atomics per counter than it won.)
  int b = w / a.nchunks, c = w - b * a.nchunks;
  if (a.skew >= 0x10000) {       // three waves per SIMD, 12-wave workgroups: the chunk triples of k_fused4 (kernels_fused.h)
    const int cg = 3 * ((int)blockIdx.x * 4 + (wib & 3)) + (wib >> 2);
    b = cg / a.nchunks;
    c = cg - b * a.nchunks;
    w = cg;
  } else if (a.skew != 0 && (blockDim.x >> 6) == 8) {
    // 8-wave workgroups, one per CU: the two waves of a SIMD are waves i and i + 4 of one workgroup, dispatched in that order -
    // the hardware slot is the wave's index in the workgroup / 4 whatever else runs on the chip
    const int cg = 2 * ((int)blockIdx.x * 4 + (wib & 3)) + (wib >> 2);
    b = cg / a.nchunks;
    c = cg - b * a.nchunks;
    w = cg;
  } else if (a.skew != 0) {
    const int half = a.n_waves >> 1, second = w >= half ? 1 : 0, wl = w - second * half, pairs = a.nchunks >> 1;
    b = wl / pairs;
    c = 2 * (wl - b * pairs) + second;
    w = b * a.nchunks + c;      // (the index of the chunk walked: the partial sums go by it)
  }
  if (a.skew != 0 && w >= a.n_waves) return;
  const int t_begin = chunk_begin(c, a.T, a.nchunks, a.skew);
  const int t_end = chunk_begin(c + 1, a.T, a.nchunks, a.skew);
  const float* zrow = a.x_in + (long long)b * a.L;
  const float* tailrow = a.xtail_in + (long long)b * a.nchunks * NB * HOP;
  float* zorow = a.x_out + (long long)b * a.L;
  // x_{t+1} is only written when somebody will read it (a.x2_out given): the launch before an evaluating one and the last one of
  // a call; the recursion itself runs on z
  const bool write_x = a.x2_out != nullptr;
  float* xorow = a.x2_out + (long long)b * a.L;
  const float half_scale = 0.5f * a.fwd_scale;
  const float tds_raw = a.tds / half_scale;
  const float nlr = -a.coef;

  v2f acc[NB * QU];
#pragma unroll
  for (int i = 0; i < NB * QU; ++i) acc[i] = v2f{0.0f, 0.0f};
  double sd = 0.0, so = 0.0;
  // pass-1 twiddles in registers - except in the evaluating variants (one launch in ten), which have no room for them at
  // n_fft 2048 and read the LDS table instead (measured: the same step time, no spills in the late one)
  constexpr bool TWLDS = EVAL && R >= 16;
  TwRegs<TWLDS ? 2 : R> twr_regs;
  if (!TWLDS) {
#pragma unroll
    for (int k1 = 1; k1 < R; ++k1) twr_regs.w[(TWLDS ? 1 : k1) - 1] = lds_tw1[(k1 - 1) * 64 + lane];
  }
  const TwLds twr_lds{lds_tw1, lane};
  const auto& twr = td_pick<TWLDS>(twr_lds, twr_regs);

  // samples of z_t: three hop-blocks carried from frame to frame plus the new one, fetched one frame ahead
  v2f xq[NB][QU], xn[QU];
#pragma unroll
  for (int q = 0; q < NB; ++q)
    td_load_block<R, OV, true>(zrow, tailrow, a.L, a.T, c, t_begin, t_end, t_begin + q, lane, a.pad_mode, xq[q]);
  td_load_block<R, OV, true>(zrow, tailrow, a.L, a.T, c, t_begin, t_end, t_begin + NB, lane, a.pad_mode, xn);

  // The overlap-add envelope is periodic in the hop wherever all n_fft / hop frames that cover a sample exist (hop-blocks NB .. T-1:
  // the same summands in the same order, plan_impl.h): one block of its reciprocal is kept in registers instead of being loaded for
  // every frame (the evaluating variant has no registers to spare and keeps loading)
  constexpr bool ENVREG = !EVAL;
  v2f envc[QU], envr[QU];        // (the envelope block and its correctly rounded reciprocal)
  if (ENVREG) {
    const v2f* e0 = reinterpret_cast<const v2f*>(a.env + (long long)(NB - PB) * HOP);
#pragma unroll
    for (int i = 0; i < QU; ++i) {
      envc[i] = e0[64u * i + ulane];
      envr[i] = env_rcp(envc[i]);
    }
  }
  // the real-FFT twiddles of the pairs, W_N^(lane + 64 j): the plain launches have the registers to keep all of them (two waves
  // per SIMD leave 256 each), the others rebuild them from W_N^lane every frame
  constexpr bool WKREG = !EVAL;
  v2f wkr[WKREG ? H : 1];
  if (WKREG) {
#pragma unroll
    for (int j = 0; j < H; ++j) wkr[j] = pair_twiddle<R>(k.wn, j);
  }
  for (int t = t_begin; t < t_end; ++t) {
    asm volatile("" ::: "memory");     // (window / twiddle reads stay inside the loop: hoisted they pin ~80 VGPRs)
    v2f wn = k.wn;
    if (!WKREG) asm volatile("" : "+v"(wn));     // (only the launches that rebuild the pair twiddles read it)
    const long long fi = (long long)b * a.T + t;
    v4f mm[H / 2];
    v4f pp[EARLY ? H : 1];
    v2f pmid = v2f{0.0f, 0.0f};
    float mmid = 0.0f;
    __builtin_amdgcn_s_setprio(1);
    {
      const v4f* min_ = a.m_pairs + fi * (H / 2 * 64);
#pragma unroll
      for (int j = 0; j < H / 2; ++j) mm[j] = ld_stream(&min_[j * 64u + ulane]);
      if (lane == 0) {
        mmid = a.m_mid[fi];
        if (EARLY) pmid = a.Pmid_in[fi];
      }
    }
#define SPECINV_TD_C0_LOADS()                                                              \
    if (EARLY) {                                                                           \
      const v4f* pin_ = a.P_in + fi * (H * 64);                                            \
      _Pragma("unroll") for (int j = 0; j < H; ++j) pp[j] = ld_stream(&pin_[j * 64u + ulane]); \
    }
    if (!EVAL) SPECINV_TD_C0_LOADS();      // (in flight during the forward FFT; the evaluating variant has no registers for
                                           // them before its first transform is done)

    v2f z[R];
    if (EVAL) {
      // |STFT(x_t)| against the target (methods.py:242): x_t's frame, transformed and dropped
      const float* xrow = a.x2_in + (long long)b * a.L;
#pragma unroll
      for (int qq = 0; qq < OV; ++qq) {
        v2f q[QU];
        td_load_block<R, OV>(xrow, tailrow, a.L, a.T, c, t_begin, t_end, t + qq, lane, a.pad_mode, q);
#pragma unroll
        for (int i = 0; i < QU; ++i) z[qq * QU + i] = q[i] * lds_win[64 * (qq * QU + i) + lane];
      }
      td_fft_forward<R>(z, k, twr, tr, tsc);
      v2f rc[H];
#pragma unroll
      for (int m = H; m < R; ++m) {
        const v2f got = shfl2(z[m], k.partner);
        const v2f own = z[(m + 1) % R];
        rc[m - H] = v2f{lane == 0 ? own.x : got.x, lane == 0 ? own.y : got.y};
      }
      // a frame's 2 H + 1 terms per lane are summed in float32 (relative error 1e-7: the metric is compared to 1e-5), the
      // frames in float64 - this kernel is bound by its vector instructions, float64 ones cost several each
      float fd = 0.0f, fo = 0.0f;
#pragma unroll
      for (int j = 0; j < H; ++j) {
        const v2f wk = pair_twiddle<R>(wn, j);
        v2f xk, xm;
        td_split<R>(z[j], rc[R - 1 - j - H], wk, half_scale, xk, xm);
        const float mk = (j & 1) ? mm[j / 2].z : mm[j / 2].x;
        const float mq = (j & 1) ? mm[j / 2].w : mm[j / 2].y;
        const float ok = fast_abs(xk), om = fast_abs(xm);
        const float dk = ok - mk, dm = om - mq;
        fd = fmaf(dk, dk, fmaf(dm, dm, fd));
        fo = fmaf(ok, ok, fmaf(om, om, fo));
      }
      if (lane == 0) {
        const float o = fast_abs(z[H] * v2f{a.fwd_scale, -a.fwd_scale});
        const float d = o - mmid;
        fd = fmaf(d, d, fd);
        fo = fmaf(o, o, fo);
      }
      sd += (double)fd;
      so += (double)fo;
      asm volatile("" ::: "memory");       // (keeps the scheduler from hoisting the loads into the transform above)
      __builtin_amdgcn_sched_barrier(0);
      SPECINV_TD_C0_LOADS();
    }
#undef SPECINV_TD_C0_LOADS

    // ---- analysis of z_t's frame; its oldest hop-block is the one this frame's output block needs
    v2f zold[QU];
#pragma unroll
    for (int i = 0; i < QU; ++i) {
      zold[i] = xq[0][i];
#pragma unroll
      for (int q = 0; q < NB; ++q) z[q * QU + i] = xq[q][i] * lds_win[64 * (q * QU + i) + lane];
      z[NB * QU + i] = xn[i] * lds_win[64 * (NB * QU + i) + lane];
#pragma unroll
      for (int q = 0; q + 1 < NB; ++q) xq[q][i] = xq[q + 1][i];
      xq[NB - 1][i] = xn[i];
    }
    // (the block after a chunk's last frame has no reader: the empty asm defines xn there, so that the compiler does not carry
    // the old block round the loader's arms in a second set of registers)
    if (t + 1 < t_end) {
      td_load_block<R, OV, true>(zrow, tailrow, a.L, a.T, c, t_begin, t_end, t + OV, lane, a.pad_mode, xn);
    } else {
#pragma unroll
      for (int i = 0; i < QU; ++i) asm volatile("" : "=v"(xn[i]));
    }
    __builtin_amdgcn_s_setprio(0);

    td_fft_forward<R>(z, k, twr, tr, tsc);

    v2f rc[H];
    if constexpr (R == 16) {
#pragma unroll
      for (int m = H; m < R; ++m) rc[m - H] = shfl2(z[m], k.partner);
      // lane 0 is its own partner, shifted by one register
      td_lane0_mov8(rc[0], rc[1], rc[2], rc[3], rc[4], rc[5], rc[6], rc[7], z[9], z[10], z[11], z[12], z[13], z[14], z[15], z[0]);
    } else {
#pragma unroll
      for (int m = H; m < R; ++m) {
        const v2f got = shfl2(z[m], k.partner);
        const v2f own = z[(m + 1) % R];              // lane 0 is its own partner, shifted by one register
        rc[m - H] = v2f{lane == 0 ? own.x : got.x, lane == 0 ? own.y : got.y};
      }
    }

    // ---- per pair: split -> (+ c0 term) -> projection -> fold back
    v2f back[H];
    // The reference's operation order (ref_rcp_abs2, fast_core.h), written breadth-first over the frame's H pairs: every step of
    // the chain of dependent packed operations is issued for all pairs before the next one, so that no instruction waits on the
    // one just before it (the compiler pads such pairs with s_nop: 44 in the frame loop instead of 106).
    // Nothing but the projection reads the bins, and it divides by their magnitude: the 1/2 fwd_scale of the split is left out
    // (late launches) or moved onto the c0 term's factor (early launches: S / s = raw + (tds / s) c0, one packed multiply-add per
    // bin).  This is exact, not approximate: the kernel is only taken for fwd_scale = 1, the factor 2 scales every intermediate
    // result without a rounding, and the guard / floor constants are doubled / quadrupled with it.
    {
      v2f sk[H], sm[H], tt[H], yy[H], hh[H];
#pragma unroll
      for (int j = 0; j < H; ++j) {
        const v2f wk = WKREG ? wkr[WKREG ? j : 0] : pair_twiddle<R>(wn, j);
        td_split_raw<R>(z[j], rc[R - 1 - j - H], wk, sk[j], sm[j]);
        if (EARLY) {
          sk[j] = __builtin_elementwise_fma(v2f{pp[j].x, pp[j].y}, v2f{tds_raw, tds_raw}, sk[j]);
          sm[j] = __builtin_elementwise_fma(v2f{pp[j].z, pp[j].w}, v2f{tds_raw, tds_raw}, sm[j]);
        }
        tt[j] = v2f{ref_norm2(sk[j], 4.0f * kRefFloor), ref_norm2(sm[j], 4.0f * kRefFloor)};
      }
#pragma unroll
      for (int j = 0; j < H; ++j) yy[j] = v2f{__builtin_amdgcn_rsqf(tt[j].x), __builtin_amdgcn_rsqf(tt[j].y)};
      // one Newton step on y ~ t^-1/2: the correctly rounded 1 / |s| in all but ~1e-6 of the cases (ONE rounding of the exact
      // value where the reference rounds |s| and then its reciprocal); the guard 1e-16 only matters below |s| = 3e-9
#pragma unroll
      for (int j = 0; j < H; ++j) hh[j] = tt[j] * yy[j];
#pragma unroll
      for (int j = 0; j < H; ++j) tt[j] = __builtin_elementwise_fma(-hh[j], yy[j], v2f{1.0f, 1.0f});
#pragma unroll
      for (int j = 0; j < H; ++j) yy[j] = __builtin_elementwise_fma(yy[j] * 0.5f, tt[j], yy[j]);
#pragma unroll
      for (int j = 0; j < H; ++j) {
        const v2f mp = (j & 1) ? v2f{mm[j / 2].z, mm[j / 2].w} : v2f{mm[j / 2].x, mm[j / 2].y};
        sk[j] = scale_lo(sk[j], mp);
        sm[j] = scale_hi(sm[j], mp);
      }
#pragma unroll
      for (int j = 0; j < H; ++j) {
        const v2f wk = WKREG ? wkr[WKREG ? j : 0] : pair_twiddle<R>(wn, j);
        v2f ak = scale_lo(sk[j], yy[j]);
        v2f am = scale_hi(sm[j], yy[j]);
        if (j == 0 && lane == 0) {   // bins 0 and M: irfft ignores their imaginary parts
          ak.y = 0.0f;
          am.y = 0.0f;
        }
        const v2f e2i = add_conj(ak, am);
        const v2f o2i = cmulc(sub_conj(ak, am), wk);
        z[j] = add_i(e2i, o2i);
        back[j] = conj_sub_i(e2i, o2i);
      }
    }
    v2f zmid;
    {
      v2f smid = z[H] * v2f{a.fwd_scale, -a.fwd_scale};
      if (EARLY) smid = v2f{fmaf(a.tds, pmid.x, smid.x), fmaf(a.tds, pmid.y, smid.y)};
      const v2f am = (smid * mmid) * ref_rcp_abs(ref_norm2(smid));
      zmid = am * v2f{2.0f, -2.0f};
    }
    if constexpr (R == 16) {
#pragma unroll
      for (int m = H; m < R; ++m) z[m] = shfl2(back[R - 1 - m], k.partner);
      td_lane0_mov8(z[8], z[9], z[10], z[11], z[12], z[13], z[14], z[15], zmid, back[7], back[6], back[5], back[4], back[3], back[2],
                    back[1]);
    } else {
#pragma unroll
      for (int m = H; m < R; ++m) {
        const v2f got = shfl2(back[R - 1 - m], k.partner);
        const v2f l0 = (m == H) ? zmid : back[(R - m) % H];
        z[m] = v2f{lane == 0 ? l0.x : got.x, lane == 0 ? l0.y : got.y};
      }
    }

    td_fft_inverse<R>(z, k, twr, tr, tsc);

    // ---- synthesis window, register overlap-add, one finished hop-block of x_{t+1} and of z_{t+1} out
    // (the newest quarter is multiplied where it is stored, after the shift below has read its slot: the product lands in the
    // accumulator's registers instead of being moved there)
#pragma unroll
    for (int u = 0; u < NB * QU; ++u) z[u] = z[u] * lds_wins[64 * u + lane];
    if (t >= PB) {
      const long long o0 = (long long)(t - PB) * HOP;
      const v2f* envp = reinterpret_cast<const v2f*>(a.env + o0);   // uniform
      v2f* xo = reinterpret_cast<v2f*>(xorow + o0);
      v2f* zo = reinterpret_cast<v2f*>(zorow + o0);
      // The envelope block: the register copy wherever it is valid, read where it lies.  The first frames of an item load theirs
      // into it - in an arm of its own that also waits for it (the empty asm reads the registers): left to a select per value
      // the compiler puts each load behind a branch and an unconditional s_waitcnt vmcnt(0) after the join, which on gfx950 also
      // waits for the stores just issued - three store round trips per frame in the steady state.  Frame NB's block IS the
      // periodic one (envp = a.env + (NB - PB) HOP there): the arm's last pass leaves it in the registers for the rest of the chunk.
      if (!ENVREG) {
#pragma unroll
        for (int i = 0; i < QU; ++i) {
          envc[i] = envp[64u * i + ulane];
          envr[i] = env_rcp(envc[i]);
        }
      } else if (t <= NB) {
#pragma unroll
        for (int i = 0; i < QU; ++i) envc[i] = envp[64u * i + ulane];
#pragma unroll
        for (int i = 0; i < QU; ++i) asm volatile("" : "+v"(envc[i]));
#pragma unroll
        for (int i = 0; i < QU; ++i) envr[i] = env_rcp(envc[i]);
      }
#pragma unroll
      for (int i = 0; i < QU; ++i) {
        const v2f xv = env_apply_r(acc[i] + z[i], envc[i], envr[i]);
        const v2f zv = __builtin_elementwise_fma(v2f{nlr, nlr}, zold[i], xv);     // (one packed operation)
        if (write_x) xo[64u * i + ulane] = xv;
        zo[64u * i + ulane] = zv;
      }
    }
#pragma unroll
    for (int i = 0; i < QU; ++i) {
#pragma unroll
      for (int q = 0; q + 1 < NB; ++q) acc[q * QU + i] = acc[(q + 1) * QU + i] + z[(q + 1) * QU + i];
    }
#pragma unroll
    for (int i = 0; i < QU; ++i) acc[(NB - 1) * QU + i] = z[NB * QU + i] * lds_wins[64 * (NB * QU + i) + lane];
  }
  if (t_end == a.T) {
    // the chunk that holds the last frame also finishes hop-blocks T .. T + PB - 2 (the frames that reach them are done);
    // xq[q] is z_t's block T + q by now
#pragma unroll
    for (int q = 0; q < PB - 1; ++q) {
      const long long o0 = (long long)(a.T + q - PB) * HOP;
      const v2f* envp = reinterpret_cast<const v2f*>(a.env + o0);
      v2f* xo = reinterpret_cast<v2f*>(xorow + o0);
      v2f* zo = reinterpret_cast<v2f*>(zorow + o0);
#pragma unroll
      for (int i = 0; i < QU; ++i) {
        const v2f xv = env_apply(acc[q * QU + i], envp[64u * i + ulane]);
        if (write_x) xo[64u * i + ulane] = xv;
        zo[64u * i + ulane] = v2f{fmaf(nlr, xq[q][i].x, xv.x), fmaf(nlr, xq[q][i].y, xv.y)};
      }
    }
  } else {
    // what this chunk's last NB frames contribute to the next chunk's first NB hop-blocks (of x and of z alike)
    v2f* tl = reinterpret_cast<v2f*>(a.xtail_out + ((long long)b * a.nchunks + c) * NB * HOP);
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      const v2f* envp = reinterpret_cast<const v2f*>(a.env + (long long)(t_end + q - PB) * HOP);
#pragma unroll
      for (int i = 0; i < QU; ++i) tl[(q * QU + i) * 64u + ulane] = env_apply(acc[q * QU + i], envp[64u * i + ulane]);
    }
  }
  if (EVAL) {
    const double d = wave_sum(sd), o = wave_sum(so);
    if (lane == 0) {
      a.partials[2 * (long long)w] = d;
      a.partials[2 * (long long)w + 1] = o;
    }
  }
}

// the headline shapes (hop = n_fft/4 at n_fft 1024 / 2048) launch 8-wave workgroups, one per CU, like k_fused4
template <int R, bool EARLY, bool EVAL>
__global__ __launch_bounds__(R == 8 ? 768 : 64 * kFused4Waves, R == 8 ? kR8Waves : kMinWaves) void k_fused4_td(FastArgs a) {
  fused_td_body<R, 4, EARLY, EVAL>(a);
}
// every other fused shape: 4-wave workgroups like k_fused<R, OV>
template <int R, int OV, bool EARLY, bool EVAL>
__global__ __launch_bounds__(256, R >= 32 ? 1 : R == 8 ? kR8Waves : kMinWaves) void k_fused_td(FastArgs a) {
  fused_td_body<R, OV, EARLY, EVAL>(a);
}

// ---- the evaluation of x_t as a kernel of its own ----------------------------------------------------------------------------
// |STFT(x_t)| against the target (methods.py:180-182, 242) does not depend on iteration t's update, which reads z_t.  Inside
// the iteration kernel the second transform runs in a 256-register wave, two to a SIMD, its frame loaded block by block through
// the seam logic four times over: + 0.16 ms per launch at BASELINE C2.  On its own - launched behind the plain iteration kernel
// on the same stream - it is a forward transform and a sum with the sample window carried from frame to frame like the
// iteration's: 0.12 ms.  A wave walks one of kEvalSub pieces of a chunk of the iteration's chunking (whose seams the block
// loader resolves).  Same operations in the same order as the EVAL block of fused_td_body: the same sums, bit for bit.
constexpr int kEvalSub = kEvalPieces;
template <int R, int OV>
__global__ __launch_bounds__(256, kEvalWaves) void k_eval_td(FastArgs a) {
  using G = Geo<R>;
  using O = Ovl<R, OV>;
  constexpr int H = G::H, M = G::M, QU = O::QU, HOP = O::HOP, NB = O::NB;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  v2f* lds_win = reinterpret_cast<v2f*>(smem);
  v2f* lds_tw1 = lds_win + M;
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  v2f* tr = lds_tw1 + (R - 1) * 64 + wib * G::TR;
  WinRegs<M> wreg;
  win_request<M>(a.window, wreg);      // (in flight while the twiddles are built)
  for (int i = threadIdx.x; i < (R - 1) * 64; i += blockDim.x) {
    const int k1 = i / 64 + 1, l = i & 63;
    lds_tw1[i] = unit(2.0f * (float)((l * k1) % M) / (float)M);
  }
  win_store<M>(wreg, lds_win);
  __syncthreads();
  const int w = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wib);
  if (w >= a.n_waves * kEvalSub) return;
  const LaneConst<R> k = lane_consts<R>();
  const TdScratch tsc = td_scratch<R>(tr, k);
  const int lane = k.lane;
  const unsigned ulane = (unsigned)lane;
  const int cw = w / kEvalSub, sub = w - cw * kEvalSub;
  const int b = cw / a.nchunks, c = cw - b * a.nchunks;
  const int t_begin = chunk_begin(c, a.T, a.nchunks, a.skew), t_end = chunk_begin(c + 1, a.T, a.nchunks, a.skew);
  const int s_begin = t_begin + (sub * (t_end - t_begin)) / kEvalSub, s_end = t_begin + ((sub + 1) * (t_end - t_begin)) / kEvalSub;
  const float* xrow = a.x2_in + (long long)b * a.L;
  const float* tailrow = a.xtail_in + (long long)b * a.nchunks * NB * HOP;
  const float half_scale = 0.5f * a.fwd_scale;
  TwRegs<R> twr;
#pragma unroll
  for (int k1 = 1; k1 < R; ++k1) twr.w[k1 - 1] = lds_tw1[(k1 - 1) * 64 + lane];
  double sd = 0.0, so = 0.0;
  v2f xq[NB][QU], xn[QU];
#pragma unroll
  for (int q = 0; q < NB; ++q)
    td_load_block<R, OV>(xrow, tailrow, a.L, a.T, c, t_begin, t_end, s_begin + q, lane, a.pad_mode, xq[q]);
  td_load_block<R, OV>(xrow, tailrow, a.L, a.T, c, t_begin, t_end, s_begin + NB, lane, a.pad_mode, xn);
  for (int t = s_begin; t < s_end; ++t) {
    asm volatile("" ::: "memory");
    v2f wn = k.wn;
    asm volatile("" : "+v"(wn));
    const long long fi = (long long)b * a.T + t;
    v4f mm[H / 2];
    float mmid = 0.0f;
    {
      const v4f* min_ = a.m_pairs + fi * (H / 2 * 64);
#pragma unroll
      for (int j = 0; j < H / 2; ++j) mm[j] = ld_stream(&min_[j * 64u + ulane]);
      if (lane == 0) mmid = a.m_mid[fi];
    }
    v2f z[R];
#pragma unroll
    for (int i = 0; i < QU; ++i) {
#pragma unroll
      for (int q = 0; q < NB; ++q) z[q * QU + i] = xq[q][i] * lds_win[64 * (q * QU + i) + lane];
      z[NB * QU + i] = xn[i] * lds_win[64 * (NB * QU + i) + lane];
#pragma unroll
      for (int q = 0; q + 1 < NB; ++q) xq[q][i] = xq[q + 1][i];
      xq[NB - 1][i] = xn[i];
    }
    if (t + 1 < s_end) {
      td_load_block<R, OV>(xrow, tailrow, a.L, a.T, c, t_begin, t_end, t + OV, lane, a.pad_mode, xn);
    } else {      // (no reader: see fused_td_body)
#pragma unroll
      for (int i = 0; i < QU; ++i) asm volatile("" : "=v"(xn[i]));
    }
    td_fft_forward<R>(z, k, twr, tr, tsc);
    v2f rc[H];
#pragma unroll
    for (int m = H; m < R; ++m) {
      const v2f got = shfl2(z[m], k.partner);
      const v2f own = z[(m + 1) % R];
      rc[m - H] = v2f{lane == 0 ? own.x : got.x, lane == 0 ? own.y : got.y};
    }
    float fd = 0.0f, fo = 0.0f;
#pragma unroll
    for (int j = 0; j < H; ++j) {
      const v2f wk = pair_twiddle<R>(wn, j);
      v2f xk, xm;
      td_split<R>(z[j], rc[R - 1 - j - H], wk, half_scale, xk, xm);
      const float mk = (j & 1) ? mm[j / 2].z : mm[j / 2].x;
      const float mq = (j & 1) ? mm[j / 2].w : mm[j / 2].y;
      const float ok = fast_abs(xk), om = fast_abs(xm);
      const float dk = ok - mk, dm = om - mq;
      fd = fmaf(dk, dk, fmaf(dm, dm, fd));
      fo = fmaf(ok, ok, fmaf(om, om, fo));
    }
    if (lane == 0) {
      const float o = fast_abs(z[H] * v2f{a.fwd_scale, -a.fwd_scale});
      const float d = o - mmid;
      fd = fmaf(d, d, fd);
      fo = fmaf(o, o, fo);
    }
    sd += (double)fd;
    so += (double)fo;
  }
  const double d = wave_sum(sd), o = wave_sum(so);
  if (lane == 0) {
    a.partials[2 * (long long)w] = d;
    a.partials[2 * (long long)w + 1] = o;
  }
}

}  // namespace fast
}  // namespace specinv
