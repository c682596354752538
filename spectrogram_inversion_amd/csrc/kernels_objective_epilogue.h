// k_objective_epilogue: the one launch behind either one-launch objective kernel (seams, margins, statistics, loss - and the
// decisions of the device-resident optimiser's two-launch iteration), and the kernel that finishes its rows.  Launched by
// objective_host.h.
#pragma once
#include "common.h"
#include "kernels_generic.h"
#include "objective_args.h"
#include "lbfgs_state.h"

namespace specinv {

// What follows k_objective_logmel, in ONE launch of kObjRows blocks (grid-stride over the work):
//   * chunk seams: grad[n] += the previous tile's tail over the first n_fft - hop samples of tiles 1.. (k_hop_tails_raw),
//   * fold of the padded margins onto the signal (k_grad_fold_margins with `margins` given),
//   * the statistics of the gradient (fast::ObjStatReq; none: st.rows == nullptr): the pass over the seams becomes a pass over the
//     WHOLE gradient with g_prev and d beside it - every sample counted once, by the thread that finishes it - and leaves the
//     first level of the reduction tree: block j adds the squared-error sums of the tiles [j n_tiles / kObjRows, (j + 1) n_tiles /
//     kObjRows) of the objective kernel to its own figures and writes ONE row of kObjStatRow doubles - {g.d, sum|g|, y.s, y.y,
//     g.g, g.g_prev, max|g|, max|d|, squared error}, stored component-major [kObjStatRow][kObjRows]; whoever needs the figures (k_objective_finish_rows, the optimiser's
//     decision kernels) reads kObjRows rows.  (Round 4: k_lbd_pair_stats, a pass of its own after this kernel.  Taken inside the
//     objective kernel's gather instead, the statistics cost more than that pass: 0.156 against 0.124 ms per evaluation at C5 -
//     with one workgroup per CU nothing hides the loads of g_prev and d.)
//   * without statistics: loss = scale * sum(partials) by one extra block (block kObjRows), as k_finish_scaled would.
// A margin sample that also lies in a seam region is finished by its margin thread (own + tail first, then the fold: the order
// of the separate launches); the seam threads leave those samples alone, so no two threads touch the same sample.
constexpr int kObjEpiThreads = 1024;   // a streaming pass wants waves in flight: 16 per CU at one block per CU
constexpr int kObjEpiGroup = 128;      // threads that walk one tile together in the statistics pass (C5: 512 / 256 / 128 threads
                                       // -> 122.7 / 121.2 / 120.8 ms per step)
// the tail's hand-over of the rows by write-through stores + vmcnt(0) instead of a release (see the tail below): only where the
// ISA documents it
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx942__) && !defined(__gfx950__)
constexpr bool kTailSc1Protocol = false;
#else
constexpr bool kTailSc1Protocol = true;
#endif
static __global__ __launch_bounds__(kObjEpiThreads) void k_objective_epilogue(float* __restrict__ grad, const float* __restrict__ xtail,
                                                                   const float* __restrict__ margins, const double* __restrict__ part,
                                                                   double* __restrict__ slot, int T, int nchunks, int n_fft, int hop,
                                                                   int keep, int pad, int pad_mode, int64_t len, int64_t rows,
                                                                   int64_t n_tail, int64_t n_margin, int n_part, double scale,
                                                                   fast::ObjCtl ctl, fast::ObjStatReq st, int vec_ok, int skew,
                                                                   fast::ObjDecide dec) {
  // (chunks of frames: k_objective_logmel's tiles - even, skew 0 - or k_objective_walk's, which may be skewed in pairs)
  auto hop_chunk_begin_ = [&](int c_, int T_, int n_) { return fast::chunk_begin(c_, T_, n_, skew); };
  float* grad_other = ctl.grad_alt;
  if (ctl.do_eval != nullptr) {                  // device-resident optimiser: gate and gradient ping-pong (lbfgs_dev.h)
    if (*ctl.do_eval == 0) {
      if (dec.ticket != nullptr && blockIdx.x == 0) lbd_tail_pass(dec);
      return;
    }
    if ((*ctl.cur ^ 1) != 0) {
      grad_other = grad;
      grad = ctl.grad_alt;
    }
  }
  __shared__ double red[16];
  __shared__ LbdState lbd_r;
  if (dec.ticket != nullptr) lbd_tail_preload(dec, lbd_r);
  if (st.rows == nullptr && blockIdx.x == fast::kObjRows) {
    double sacc = 0;
    for (int i = threadIdx.x; i < n_part; i += blockDim.x) sacc += part[i];
    const double t = block_sum(sacc, red);
    if (threadIdx.x == 0) *slot = scale * t;
    return;
  }
  const bool st_on = st.rows != nullptr;
  const float* st_d = st.d;
  const float* st_gp = st.gp;
  float st_t = st.t;
  bool d_impl = false;
  double c0_d = 0.0;
  if (st_on && st.have != nullptr) {
    const bool have = *st.have != 0;
    st_t = (float)*st.t_dev;
    st_gp = have ? grad_other : nullptr;
    st_d = have ? st.d : nullptr;
    if (have && st.d_implicit != nullptr && *st.d_implicit != 0) {    // d = (float)(c0 (double)g_prev): recomputed, not read
      d_impl = true;
      c0_d = *st.c0_d;
      st_d = nullptr;
    }
  }
  auto d_of = [&](float gpv) { return (float)(c0_d * (double)gpv); };
  fast::ObjStatAcc sta;
  const bool fold = pad > 0 && pad_mode != SPECINV_PAD_CONSTANT;
  const bool seams = keep > 0 && nchunks > 1;
  const int64_t covered = (int64_t)(T - 1) * hop + n_fft;                // padded positions that receive any frame
  const int64_t stride = (int64_t)fast::kObjRows * blockDim.x, first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  // the seam sample n may lie in: the first n_fft - hop padded positions of the tile that holds frame (n + pad) / hop (at most one
  // seam: tiles are longer than a frame); returns the index into xtail or -1
  const bool small = covered < ((int64_t)1 << 31) && (int64_t)T * nchunks < ((int64_t)1 << 31);   // 32-bit divisions (a 64-bit one is ~200 instructions)
  auto seam_of = [&](int64_t b, int64_t n) -> int64_t {
    if (!seams) return -1;
    int64_t f0 = small ? (int64_t)((unsigned)(n + pad) / (unsigned)hop) : (n + pad) / hop;
    if (f0 > T - 1) f0 = T - 1;
    int c = small ? (int)(((unsigned)(f0 + 1) * (unsigned)nchunks - 1u) / (unsigned)T) : (int)(((f0 + 1) * nchunks - 1) / T);   // largest c with c * T / nchunks <= f0, up to rounding: corrected below
    while (c + 1 < nchunks && hop_chunk_begin_(c + 1, T, nchunks) <= f0) ++c;
    while (c > 0 && hop_chunk_begin_(c, T, nchunks) > f0) --c;
    if (c < 1) return -1;
    const int64_t j0 = n + pad - (int64_t)hop_chunk_begin_(c, T, nchunks) * hop;
    return (j0 >= 0 && j0 < keep) ? (b * nchunks + (c - 1)) * keep + j0 : -1;
  };
  if (st_on) {
    // ---- the whole gradient: seams finished on the way, every sample outside the folded stretches counted
    if (vec_ok) {
      // 16-byte pieces (keep, hop, pad, len multiples of 4), tile by tile: the samples between the first frame of tile c and the
      // first frame of tile c + 1 (the first tile from 0, the last to the end), whose first n_fft - hop are the seam with tile c - 1
      // - no division per piece; a piece lies in a seam whole or not at all
      // Two groups of 512 threads walk tiles of their own, three pieces per thread and trip with their loads all requested first:
      // 9 - 12 loads of 16 bytes in flight per thread (four pieces: 46 registers spilled at 16 waves per CU).
      const int64_t n_pairs = rows * nchunks;
      constexpr int GT = kObjEpiGroup, NG = kObjEpiThreads / GT;
      const int grp = threadIdx.x / GT, tig = threadIdx.x - grp * GT;
      // (b, c) of a group's tiles advance by additions: an integer division per tile - and the plain form had three, one of them
      // 64-bit - is a few hundred vector instructions that every wave of the group repeats (round 5: 15 of the pass's 29 us went
      // into index arithmetic)
      const unsigned pr0 = (unsigned)(NG * (int)blockIdx.x + grp), pstep = (unsigned)(NG * (int)gridDim.x);
      unsigned bq = pr0 / (unsigned)nchunks, cq = pr0 - bq * (unsigned)nchunks;
      const unsigned bstep = pstep / (unsigned)nchunks, cstep = pstep - bstep * (unsigned)nchunks;
      for (int64_t pr = pr0; pr < n_pairs; pr += pstep, bq += bstep, cq += cstep) {
        if (cq >= (unsigned)nchunks) {
          cq -= (unsigned)nchunks;
          ++bq;
        }
        const int64_t b = bq;
        const int c = (int)cq;
        const int64_t t_lo = (int64_t)hop_chunk_begin_(c, T, nchunks) * hop - pad;       // span[0] of tile c (may be < 0)
        const int64_t t_hi = (int64_t)hop_chunk_begin_(c + 1, T, nchunks) * hop - pad;
        const int64_t n_lo = c == 0 ? 0 : (t_lo < 0 ? 0 : (t_lo > len ? len : t_lo));
        const int64_t n_hi = c == nchunks - 1 ? len : (t_hi < 0 ? 0 : (t_hi > len ? len : t_hi));
        // (offsets inside a tile are ints: pointers to the tile's first sample, the fold stretches as offsets too)
        const int span = (int)(n_hi - n_lo), seam_end = (seams && c >= 1) ? (int)(t_lo + keep - n_lo) : 0;   // pieces below seam_end: + tail
        const float* tl = xtail + (b * nchunks + (c - 1)) * keep + (n_lo - t_lo);
        float* gb = grad + b * len + n_lo;
        const float* pb = st_gp ? st_gp + b * len + n_lo : nullptr;
        const float* db = st_d ? st_d + b * len + n_lo : nullptr;
        // offsets o with n_lo + o <= pad or n_lo + o >= len - 1 - pad lie in a folded stretch
        const int64_t fl = fold ? pad - n_lo : -1, fh = fold ? len - 1 - pad - n_lo : (int64_t)1 << 40;
        const int f_lo = fl < -1 ? -1 : (fl > span ? span : (int)fl), f_hi = fh > span ? span : (fh < 0 ? 0 : (int)fh);
        constexpr int U = 3;
        for (int o0 = 4 * tig; o0 < span; o0 += U * 4 * GT) {
          int of[U];
          fast::v4f gv[U], pv[U], dv[U], tv[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            of[u] = o0 + u * 4 * GT < span ? o0 + u * 4 * GT : o0;
            gv[u] = *reinterpret_cast<const fast::v4f*>(gb + of[u]);
            pv[u] = pb ? *reinterpret_cast<const fast::v4f*>(pb + of[u]) : gv[u];
            dv[u] = db ? *reinterpret_cast<const fast::v4f*>(db + of[u]) : gv[u];
            if (d_impl) {
#pragma unroll
              for (int e = 0; e < 4; ++e) dv[u][e] = d_of(pv[u][e]);
            }
            tv[u] = of[u] < seam_end ? *reinterpret_cast<const fast::v4f*>(tl + of[u]) : fast::v4f{0.0f, 0.0f, 0.0f, 0.0f};
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            if (u > 0 && o0 + u * 4 * GT >= span) continue;
            const int o = of[u];
            const bool sm = o < seam_end;
            if (o > f_lo && o + 3 < f_hi) {
              if (sm) {
                gv[u] = gv[u] + tv[u];
                *reinterpret_cast<fast::v4f*>(gb + o) = gv[u];
              }
#pragma unroll
              for (int e = 0; e < 4; ++e) sta.add(gv[u][e], pb ? pv[u][e] : gv[u][e], (db || d_impl) ? dv[u][e] : gv[u][e], st_t);
            } else {
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                if (o + e <= f_lo || o + e >= f_hi) continue;             // finished - and counted - by the margin thread of this sample
                const float g1 = sm ? gv[u][e] + tv[u][e] : gv[u][e];
                if (sm) gb[o + e] = g1;
                sta.add(g1, pb ? pv[u][e] : g1, (db || d_impl) ? dv[u][e] : g1, st_t);
              }
            }
          }
        }
      }
    } else {
      const int64_t items = rows * len;
      for (int64_t i = first; i < items; i += stride) {
        const int64_t b = i / len, n = i - b * len;
        if (fold && (n <= pad || n >= len - 1 - pad)) continue;
        float g1 = grad[i];
        const int64_t sx = seam_of(b, n);
        if (sx >= 0) {
          g1 += xtail[sx];
          grad[i] = g1;
        }
        sta.add(g1, st_gp ? st_gp[i] : g1, d_impl ? d_of(st_gp[i]) : st_d ? st_d[i] : g1, st_t);
      }
    }
  } else if (vec_ok) {
    // ---- seams only
    const int n4 = keep / 4;
    const int64_t items = n_tail / 4;
    for (int64_t i = first; i < items; i += stride) {
      const int q = (int)(i / n4), j = 4 * (int)(i - (int64_t)q * n4);
      const int b = q / (nchunks - 1), c = q - b * (nchunks - 1) + 1;
      const int64_t n = (int64_t)hop_chunk_begin_(c, T, nchunks) * hop + j - pad;
      if (n < 0 || n >= len) continue;
      const fast::v4f tv = *reinterpret_cast<const fast::v4f*>(xtail + ((int64_t)b * nchunks + (c - 1)) * keep + j);
      float* gq = grad + (int64_t)b * len + n;
      const fast::v4f gv = *reinterpret_cast<const fast::v4f*>(gq);
      if (!(fold && (n <= pad || n + 3 >= len - 1 - pad))) {
        *reinterpret_cast<fast::v4f*>(gq) = gv + tv;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int64_t ne = n + e;
          if (ne <= pad || ne >= len - 1 - pad) continue;                 // finished by the margin thread of this sample
          gq[e] = gv[e] + tv[e];
        }
      }
    }
  } else {
    for (int64_t i = first; i < n_tail; i += stride) {                   // (b, c - 1, j)
      const int j = (int)(i % keep);
      const int c = (int)((i / keep) % (nchunks - 1)) + 1;
      const int64_t b = i / ((int64_t)keep * (nchunks - 1));
      const int64_t n = (int64_t)hop_chunk_begin_(c, T, nchunks) * hop + j - pad;
      if (n < 0 || n >= len) continue;
      if (fold && (n <= pad || n >= len - 1 - pad)) continue;             // finished by the margin thread of this sample
      grad[b * len + n] += xtail[(b * nchunks + (c - 1)) * keep + j];
    }
  }
  // ---- margins
  for (int64_t i = first; i < n_margin; i += stride) {
    const int64_t per_row = 2 * ((int64_t)pad + 1);
    const int64_t bi = n_margin < ((int64_t)1 << 31) ? (int64_t)((unsigned)i / (unsigned)per_row) : i / per_row, j = i - bi * per_row;
    int64_t n;
    if (j <= pad) {
      n = j;                                            // left stretch 0 .. pad
      if (n >= len) continue;
    } else {
      n = len - 1 - pad + (j - pad - 1);                // right stretch len-1-pad .. len-1
      if (n <= pad || n >= len) continue;               // (short signals: already covered by the left stretch)
    }
    const float* mg = margins + bi * 2 * pad;
    auto at = [&](int64_t np) -> float {                // gradient w.r.t. padded sample np
      if (np < 0 || np >= covered) return 0.0f;
      if (np < pad) return mg[np];
      const int64_t r = np - pad - len;
      return (r >= 0 && r < pad) ? mg[pad + r] : 0.0f;
    };
    float g = 0;
    switch (pad_mode) {
      case SPECINV_PAD_REFLECT:
        if (n >= 1 && n <= pad) g += at(pad - n);
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
    float v = grad[bi * len + n];
    const int64_t sx = seam_of(bi, n);
    if (sx >= 0) v += xtail[sx];
    const float g1 = v + g;
    grad[bi * len + n] = g1;
    if (st_on) sta.add(g1, st_gp ? st_gp[bi * len + n] : g1, d_impl ? d_of(st_gp[bi * len + n]) : st_d ? st_d[bi * len + n] : g1, st_t);
  }
  if (!st_on) return;
  // ---- this block's row: its own figures + the squared-error sums of its share of the objective kernel's tiles
  __shared__ double red9[kObjEpiThreads / 64][9];
  double v[9] = {sta.s[0], sta.s[1], sta.s[2], sta.s[3], sta.s[4], sta.s[5], 0.0, (double)sta.mg, (double)sta.md};
  const int lo = (int)((int64_t)n_part * blockIdx.x / fast::kObjRows), hi = (int)((int64_t)n_part * (blockIdx.x + 1) / fast::kObjRows);
  for (int tl = lo + threadIdx.x; tl < hi; tl += blockDim.x) v[6] += part[tl];
  block_reduce9(v, red9);
  const bool tail = dec.ticket != nullptr;
  __shared__ int last;
  if (threadIdx.x == 0) {                       // component-major: readers take one component of every row with one coalesced load
    double* row = st.rows + blockIdx.x;
    auto w = [&](int c) { return c < 6 ? v[c] : c == 6 ? v[7] : c == 7 ? v[8] : v[6]; };
    if (!tail) {
#pragma unroll
      for (int c = 0; c < 9; ++c) row[c * fast::kObjRows] = w(c);
    } else {
      // ---- the optimiser's decisions ride along, taken by the workgroup that finishes last.  Two forms of the hand-over:
      // (a) dec.fence (the default since round 6): the HIP memory model's own - the ticket is an acquire-release
      // read-modify-write at agent scope drawn by the ONE thread that wrote the row, the last workgroup's row loads follow an
      // acquire fence.  Measured at C5 against (b): 112.4 / 114.0 / 112.8 against 111.7 / 113.7 / 111.9 ms per step (+0.5 %;
      // round 5 had measured a release FENCE executed by every thread of every workgroup: +11 us per launch).
      // (b) SPECINV_LBFGS_TAIL_FENCE=0, gfx942 / gfx950 only - round 5's ISA-level protocol: the row goes out with agent-scope
      // atomic stores (`sc1`: written THROUGH this XCD's L2), `s_waitcnt vmcnt(0)` retires them (a write-through store is
      // acknowledged by the memory side: the wait the release sequence `buffer_wbl2 sc1; s_waitcnt vmcnt(0)` itself relies on)
      // before a RELAXED ticket is drawn; the reader's row loads are agent-scope atomic loads issued after its ticket has
      // returned.  Not a synchronises-with edge of the language's model; kept for the A/B and pinned against (a) bit for bit at
      // full size (tests/test_gpu_bench_sizes.py::test_c5_optimiser_step_full_size).
#pragma unroll
      for (int c = 0; c < 9; ++c) __hip_atomic_store(row + c * fast::kObjRows, w(c), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (kTailSc1Protocol && !dec.fence) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_s_waitcnt(0);
        last = __hip_atomic_fetch_add(dec.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1 ? 1 : 0;
      } else {
        last = __hip_atomic_fetch_add(dec.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1 ? 1 : 0;
      }
    }
  }
  if (!tail) return;
  __syncthreads();
  if (!last) return;
  if (!kTailSc1Protocol || dec.fence) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  if (threadIdx.x == 0) __hip_atomic_store(dec.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  lbd_tail_decide(dec, scale, red9, lbd_r);
}

// the second level of the tree: out = {loss, g.d, sum|g|, max|g|, max|d|, y.s, y.y, g.g, g.g_prev} from the epilogue's rows (one
// workgroup, fixed order; the layout lbfgs.py:_batch reads from its board)
static __global__ __launch_bounds__(256) void k_objective_finish_rows(const double* __restrict__ rows, double scale, double* __restrict__ out,
                                                                      int n_out) {
  __shared__ double red9[4][9];
  double v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int r = threadIdx.x; r < fast::kObjRows; r += blockDim.x) {
    const double* q = rows + r;
#pragma unroll
    for (int c = 0; c < 6; ++c) v[c] += q[c * fast::kObjRows];
    v[6] += q[8 * fast::kObjRows];
    v[7] = fmax(v[7], q[6 * fast::kObjRows]);
    v[8] = fmax(v[8], q[7 * fast::kObjRows]);
  }
  block_reduce9(v, red9);
  if (threadIdx.x == 0) {
    out[0] = scale * v[6];
    out[1] = v[0];
    out[2] = v[1];
    out[3] = v[7];
    out[4] = v[8];
    if (n_out > 5) {
      out[5] = v[2];
      out[6] = v[3];
      out[7] = v[4];
      out[8] = v[5];
    }
  }
}

}  // namespace specinv
