// The host side of the L_BFGS objective: the transform (tf_setup, tf_forward), which kernel serves loss and gradient (obj_route),
// the launches (tf_loss_grad_fused with launch_objective_epilogue; the kernel chain in tf_loss_grad) and the environment switches of
// all of it and of the device-resident optimiser in lbfgs_dev.h (ObjKnobs).
#pragma once
#include <type_traits>
#include <vector>

#include "common.h"
#include "fast_state.h"
#include "objective_args.h"
#include "kernels_vec.h"
#include "kernels_mel_dense.h"
#include "kernels_objective_epilogue.h"

namespace specinv {

// The environment switches of the objective and of the device-resident optimiser, read once per call of the C ABI (tf_loss_grad,
// lbd_step_run) and handed down.  Not once per plan: plans are cached across calls (plan.py), and tests and A-B runs flip a switch
// between two calls on the same plan.
struct ObjKnobs {
  bool sparse = true;           // SPECINV_OBJ_SPARSE=0: the filterbank as a dense matrix (contractions on the matrix cores), no frame walk
  bool walk = true;             // SPECINV_OBJ_WALK=0: the tile kernel where the frame walk would run
  bool disable_fused = false;   // SPECINV_DISABLE_FUSED_OBJECTIVE=1: the kernel chain
  bool require_fused = false;   // SPECINV_REQUIRE_FUSED_OBJECTIVE=1 (tests): the shape must be on a one-launch kernel
  bool defer = true;            // SPECINV_LBFGS_DEFER=0 (tests / A-B runs): the optimiser's own kernels apply the step
  bool tail_fence = true;       // SPECINV_LBFGS_TAIL_FENCE=0: the epilogue's rows by round 5's write-through protocol, not release / acquire
  bool lean = true;             // SPECINV_LBFGS_LEAN=0 (tests / A-B runs): the full form from the first iteration
  bool lean2 = true;            // SPECINV_LBFGS_LEAN2=0: the lean iteration in three launches where two would do

  static ObjKnobs read() {
    auto starts = [](const char* name, char c) {
      const char* e = getenv(name);
      return e != nullptr && e[0] == c;
    };
    ObjKnobs k;
    k.sparse = !starts("SPECINV_OBJ_SPARSE", '0');
    k.walk = !starts("SPECINV_OBJ_WALK", '0');
    k.disable_fused = starts("SPECINV_DISABLE_FUSED_OBJECTIVE", '1');
    k.require_fused = starts("SPECINV_REQUIRE_FUSED_OBJECTIVE", '1');
    k.defer = !starts("SPECINV_LBFGS_DEFER", '0');
    k.tail_fence = !starts("SPECINV_LBFGS_TAIL_FENCE", '0');
    k.lean = !starts("SPECINV_LBFGS_LEAN", '0');
    k.lean2 = !starts("SPECINV_LBFGS_LEAN2", '0');
    return k;
  }
};

// 16-row mel tiles the one-launch objective is instantiated for (0: not covered)
// (n_fft 1024 takes NINE tiles for 81 ... 128 bands, the last one empty: k_objective_logmel<8, 8> is the one instantiation the
// register allocator loses - 256 registers and 978 spilled, 0.204 ms per evaluation at B16 x T1024 where <8, 5> takes 0.113 -
// while <8, 7>, <8, 9> and <8, 10> allocate 180 ... 193 and spill nothing)
inline int obj_mel_tiles(int n_mels, int R) {
  const int mt = (n_mels + 15) / 16;
  return mt <= 3 ? 3 : mt <= 4 ? 4 : mt <= 5 ? 5 : mt <= 8 ? (R == 8 ? 9 : 8) : 0;
}

// Which kernel serves loss and gradient of a plan's objective (the numbering of Plan::objective_kind), and what follows from the
// choice.  kObjChain: none of the one-launch kernels - the kernel chain of tf_loss_grad.
enum : int { kObjChain = 0, kObjTiles = 1, kObjBands = 2, kObjWalk = 3 };
struct ObjRoute {
  int kind = kObjChain;
  const void* fn = nullptr;   // the kernel
  size_t lds = 0;             // its dynamic LDS, bytes
  int nch = 0;                // chunks of frames per signal: tiles of kObjTile frames, or the walk's chunks (one wave each)
  int skew = 0;               // the walk: frames a chunk pair's long chunk takes from its short one (fast::chunk_begin)
  int keep = 0;               // n_fft - hop: samples of a chunk's tail that belong to the next chunk's seam
};

// The eligibility tests, once.  Precedence: the frame walk, then the tile kernel (band form, then matrix tiles), then the chain.
template <typename P>
ObjRoute obj_route(P& pl, int64_t len, const ObjKnobs& kn) {
  ObjRoute r;
  const bool mag = pl.tf_kind == SPECINV_TF_MAG;
  if (pl.force_generic || !pl.cfg.onesided || !pl.fast.xform_ok || (pl.fast.xform_R != 8 && pl.fast.xform_R != 16)) return r;
  const bool sparse = !mag && pl.tf_sp_ok && kn.sparse;   // the filterbank in band form: contractions on the vector units
  if (!mag && (pl.tf_kind != SPECINV_TF_LOGMEL || (pl.tf_obj_mt == 0 && !sparse))) return r;
  if (kn.disable_fused) return r;
  const int N = pl.N(), hop = pl.cfg.hop_length, T = pl.Tn(), B = pl.B(), pad = pl.pad, R = pl.fast.xform_R;
  if (hop > N || hop < 2 || pad >= len) return r;
  // ---- the frame walk (kernels_objective_walk.h): hop = n_fft / {2, 4, 8}, centred, a signal of whole hops, a filterbank with at
  // most two rows per bin
  const int ov = N % hop == 0 ? N / hop : 0;
  if (sparse && kn.walk && pl.tf_walk_ok && (ov == 2 || ov == 4 || ov == 8) && 2 * pad == N && len == (int64_t)(T - 1) * hop &&
      T >= (ov == 8 ? 16 : 8)) {
    const size_t lds = R == 16 ? fast::obj_walk_lds_bytes<16>(pl.tf_walk.total) : fast::obj_walk_lds_bytes<8>(pl.tf_walk.total);
    if (lds <= 160 * 1024 - 512) {
      // chunks: one round of two waves per SIMD where the frames allow it (>= 8 frames per wave), an even count so that the two
      // waves of a SIMD can take a long and a short chunk (the older wave runs faster: kernels_fast_td.h)
      // (hop = n_fft / 8: seven of a chunk's hop-blocks are its seam with the chunk before - chunks of >= 16 frames there)
      const int floor_ch = ov == 8 ? 16 : 8;
      int nch = (int)std::max<int64_t>(1, std::min<int64_t>(T / floor_ch, 2048 / std::max(1, B)));
      if (nch > 1 && (nch & 1)) --nch;
      const int len_ch = T / nch;
      // (C5, chunks of 8 frames, one box: skew 0 / 1 / 2 / 3 -> 126.1 / 122.0 / 124.9 / 128.0 ms per step: an eighth of the chunk -
      // the contractions' LDS waits leave the younger wave more of the SIMD than the Griffin-Lim kernel's pure transforms do)
      if ((nch & 1) == 0 && (int64_t)B * nch > 1024 && len_ch >= 8) r.skew = std::max(1, len_ch / 8);
      if (len_ch - r.skew < std::max(ov, 6)) r.skew = 0;        // (the shorter chunk of a pair still holds its seam and a frame more)
      r.fn = R == 16 ? (ov == 2 ? (const void*)fast::k_objective_walk<16, 2> : ov == 4 ? (const void*)fast::k_objective_walk<16, 4>
                                                                                       : (const void*)fast::k_objective_walk<16, 8>)
                     : (ov == 2 ? (const void*)fast::k_objective_walk<8, 2> : ov == 4 ? (const void*)fast::k_objective_walk<8, 4>
                                                                                      : (const void*)fast::k_objective_walk<8, 8>);
      r.kind = kObjWalk;
      r.lds = lds;
      r.nch = nch;
      r.keep = N - hop;
      return r;
    }
  }
  // ---- the tile kernel (kernels_objective.h)
  const int nch = (T + fast::kObjTile - 1) / fast::kObjTile;
  if (nch > 1 && T / nch < (N - 1) / hop + 1) return r;                // a seam must not reach a tile's own tail
  const int MT = mag ? 3 : sparse ? 9 : pl.tf_obj_mt;
#define SPECINV_OBJ_CASE(RR, MM)                                   \
  if (R == RR && MT == MM) {                                       \
    r.fn = (const void*)fast::k_objective_logmel<RR, MM>;          \
    r.lds = fast::ObjGeo<RR, MM>::lds_bytes();                     \
  }
  if (mag) {
    if (R == 16) r.fn = (const void*)fast::k_objective_logmel<16, 3, true>;
    else r.fn = (const void*)fast::k_objective_logmel<8, 3, true>;
    r.lds = R == 16 ? fast::ObjGeo<16, 3>::lds_bytes() : fast::ObjGeo<8, 3>::lds_bytes();
  } else if (sparse) {
    if (R == 16) r.fn = (const void*)fast::k_objective_logmel<16, 9, false, true>;
    else r.fn = (const void*)fast::k_objective_logmel<8, 9, false, true>;
    r.lds = R == 16 ? fast::ObjGeo<16, 9>::lds_bytes() : fast::ObjGeo<8, 9>::lds_bytes();
  } else {
    SPECINV_OBJ_CASE(16, 3) SPECINV_OBJ_CASE(16, 4) SPECINV_OBJ_CASE(16, 5) SPECINV_OBJ_CASE(16, 8)
    SPECINV_OBJ_CASE(8, 3) SPECINV_OBJ_CASE(8, 4) SPECINV_OBJ_CASE(8, 5) SPECINV_OBJ_CASE(8, 9)
  }
#undef SPECINV_OBJ_CASE
  if (r.fn == nullptr || r.lds > 160 * 1024) return ObjRoute{};
  r.kind = sparse ? kObjBands : kObjTiles;
  r.nch = nch;
  r.keep = N - hop;
  return r;
}

// the loss from the plan's slot to the host (synchronises)
template <typename P>
int obj_read_loss(P& pl, double* loss) {
  SI_HIP(hipMemcpyAsync(loss, pl.sums.p, sizeof(double), hipMemcpyDeviceToHost, pl.stream));
  SI_HIP(si_stream_wait_short(pl.stream));
  return SPECINV_OK;
}

// k_objective_epilogue behind the objective kernel of `rt`: seams of the B * rt.nch chunks, margins, loss (to loss_dev, or the plan's
// slot) or - st->rows given - the rows of the statistics, which the caller finishes.
// (vec_ok picks the epilogue's 16-byte path.  The shapes of the frame walk pass its geometric tests by construction - 2 pad = n_fft,
// hop = n_fft / {2, 4, 8}, n_fft 1024 or 2048, at most 2048 chunks - so there only the alignment of len and of the pointers decides.)
template <typename P>
int launch_objective_epilogue(P& pl, const ObjRoute& rt, float* grad, int64_t len, double numel, double* loss_dev,
                              const fast::ObjCtl* ctl, const fast::ObjStatReq* st, const fast::ObjDecide* dec) {
  const int N = pl.N(), hop = pl.cfg.hop_length, T = pl.Tn(), pad = pl.pad, nch = rt.nch, keep = rt.keep;
  const int64_t B = pl.B();
  const bool fold = pad > 0 && pl.cfg.pad_mode != SPECINV_PAD_CONSTANT;
  const int64_t n_tail = (nch > 1 && keep > 0) ? B * (nch - 1) * keep : 0;
  const int64_t n_margin = fold ? B * 2 * (pad + 1) : 0;
  const bool with_rows = st && st->rows;
  const int blocks = fast::kObjRows + (with_rows ? 0 : 1);
  double* slot = loss_dev ? loss_dev : pl.sums.template as<double>();
  const int vec_ok = ((keep | hop | pad) & 3) == 0 && (len & 3) == 0 && ((uintptr_t)grad & 15) == 0 &&
                     (!ctl || ((uintptr_t)ctl->grad_alt & 15) == 0) && n_tail / 4 / std::max(1, keep / 4) < (1ll << 31) &&
                     (!with_rows || ((((uintptr_t)st->d | (uintptr_t)st->gp) & 15) == 0));
  hipLaunchKernelGGL(k_objective_epilogue, dim3((unsigned)blocks), dim3(kObjEpiThreads), 0, pl.stream, grad,
                     (const float*)pl.fast.hop_inv_tail.template as<float>(), (const float*)pl.fast.hop_inv_margins.template as<float>(),
                     (const double*)pl.partials.template as<double>(), slot, T, nch, N, hop, keep, pad, pl.cfg.pad_mode, len, B, n_tail,
                     n_margin, (int)(B * nch), 1.0 / numel, ctl ? *ctl : fast::ObjCtl{}, with_rows ? *st : fast::ObjStatReq{}, vec_ok,
                     rt.skew, with_rows && dec ? *dec : fast::ObjDecide{});
  SI_HIP(hipGetLastError());
  return SPECINV_OK;
}

// what the frame walk and the tile kernel take alike (ObjWalkArgs, ObjArgs)
template <typename P, typename A>
void obj_fill_args(P& pl, A& a, const ObjRoute& rt, const float* x, float* grad, const float* target, int64_t len, double numel,
                   const fast::ObjCtl* ctl) {
  a.x = x;
  a.grad = grad;
  a.margins = pl.fast.hop_inv_margins.template as<float>();
  a.xtail = pl.fast.hop_inv_tail.template as<float>();
  a.target = target;
  a.window = pl.window.template as<float>();
  a.partials = pl.partials.template as<double>();
  a.len = len;
  a.T = pl.Tn();
  a.nchunks = rt.nch;
  a.pad_mode = pl.cfg.pad_mode;
  a.n_mels = pl.tf_mels;
  a.fwd_scale = pl.fc.fwd_scale;
  a.dscale = (float)(2.0 / numel);
  if (ctl) {
    a.ctl_eval = ctl->do_eval;
    a.ctl_cur = ctl->cur;
    a.grad_alt = ctl->grad_alt;
    if constexpr (std::is_same<A, fast::ObjWalkArgs>::value) {
      a.x_alt = ctl->x_alt;
      a.px_sel = ctl->x_sel;
      a.px_pending = ctl->x_pending;
      a.pt_pend = ctl->t_pend;
      a.pc0_pend = ctl->c0_pend;
    }
  }
}

// loss and gradient of the objective by the one-launch kernel of `rt` (obj_route; not the chain) and its epilogue.  The loss goes to
// *loss (synchronises), to loss_dev, or - st->rows given - into the rows of the statistics with the rest of the figures.
template <typename P>
int tf_loss_grad_fused(P& pl, const ObjRoute& rt, const float* x, int64_t len, const float* target, double* loss, float* grad,
                       double* loss_dev = nullptr, const fast::ObjCtl* ctl = nullptr, const fast::ObjStatReq* st = nullptr,
                       const fast::ObjDecide* dec = nullptr) {
  SI_CHECK(rt.kind != kObjChain, SPECINV_EUNSUPPORTED, "the one-launch objective does not cover this configuration");
  const bool walk = rt.kind == kObjWalk;
  SI_CHECK(walk || !ctl || !ctl->x_sel, SPECINV_ESTATE, "a deferred step without the frame walk");
  const int hop = pl.cfg.hop_length, T = pl.Tn(), B = pl.B(), pad = pl.pad;
  const int64_t n_chunks = (int64_t)B * rt.nch;
  SI_TRY(pl.fast.hop_inv_tail.reserve((size_t)n_chunks * std::max(1, rt.keep) * sizeof(float) + 16));
  SI_TRY(pl.fast.hop_inv_margins.reserve((size_t)B * 2 * std::max(1, pad) * sizeof(float)));
  SI_TRY(pl.partials.reserve(std::max<size_t>((size_t)n_chunks, 3 * 1024) * sizeof(double)));
  const double numel = (double)B * T * (pl.tf_kind == SPECINV_TF_MAG ? pl.n_freq : pl.tf_mels);
  fast::ObjWalkArgs wa{};
  fast::ObjArgs ta{};
  void* kargs[1];
  if (walk) {
    obj_fill_args(pl, wa, rt, x, grad, target, len, numel, ctl);
    wa.blob = pl.tf_walk_blob.template as<fast::f32x4>();
    wa.n_waves = (int)n_chunks;
    wa.skew = rt.skew;
    wa.w = pl.tf_walk;
    kargs[0] = &wa;
  } else {
    obj_fill_args(pl, ta, rt, x, grad, target, len, numel, ctl);
    ta.melA = pl.tf_mel_a.template as<fast::f32x4>();
    ta.melB = pl.tf_mel_b.template as<fast::f32x4>();
    ta.tab = pl.tf_obj_tab.template as<int>();
    if (rt.kind == kObjBands) {
      ta.melA = pl.tf_sp_blob.template as<fast::f32x4>();
      ta.melB = nullptr;
      ta.tab = pl.tf_sp_tab.template as<int>();
      ta.sp_rm = pl.tf_sp.rm;
      ta.sp_cm = pl.tf_sp.cm;
      ta.sp_cw = pl.tf_sp.cw;
      ta.sp_total = pl.tf_sp.total;
      ta.sp_cmax = pl.tf_sp.cmax;
      ta.sp_rows = pl.tf_sp.rows;
    }
    ta.hop = hop;
    ta.pad = pad;
    ta.hop_magic = (unsigned)(((1ull << 32) + hop - 1) / hop);
    kargs[0] = &ta;
  }
  // (the walk: one wave per chunk, kWalkWaves to the workgroup; the tile kernel: one workgroup per tile)
  const dim3 grid((unsigned)(walk ? ceil_div(n_chunks, fast::kWalkWaves) : n_chunks)), block(64 * (walk ? fast::kWalkWaves : fast::kObjWaves));
  SI_HIP(hipFuncSetAttribute(rt.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rt.lds));
  SI_HIP(hipLaunchKernel(rt.fn, grid, block, kargs, rt.lds, pl.stream));
  pl.objective_kind = rt.kind;
  SI_TRY(launch_objective_epilogue(pl, rt, grad, len, numel, loss_dev, ctl, st, dec));
  if ((st && st->rows) || loss_dev) return SPECINV_OK;      // (rows: loss and figures are in them, the caller finishes them)
  return obj_read_loss(pl, loss);
}

template <typename P, typename T>
int tf_setup(P& pl, int kind, const T* mel_fb, int n_mels) {
  SI_CHECK(kind == SPECINV_TF_MAG || kind == SPECINV_TF_LOGMEL, SPECINV_EINVAL, "unknown transform kind %d", kind);
  SI_CHECK(kind != SPECINV_TF_LOGMEL || (mel_fb && n_mels > 0), SPECINV_EINVAL, "log-mel transform needs a filterbank");
  // what the one-launch kernels have of the filterbank (obj_route): built below where they cover the transform
  pl.tf_obj_mt = 0;
  pl.tf_sp_ok = false;
  pl.tf_walk_ok = false;
  pl.tf_mels = kind == SPECINV_TF_LOGMEL ? n_mels : 0;
  if (kind == SPECINV_TF_LOGMEL) {
    SI_TRY(pl.tf_mel.reserve((size_t)n_mels * pl.n_freq * sizeof(T)));
    SI_HIP(hipMemcpyAsync(pl.tf_mel.p, mel_fb, (size_t)n_mels * pl.n_freq * sizeof(T), hipMemcpyDeviceToDevice, pl.stream));
    if constexpr (std::is_same<T, float>::value) {
      const int mt = (n_mels + 31) / 32;
      if (mt <= 4) {
        const int ksteps = (pl.n_freq + 31) / 32;
        const int64_t total = (int64_t)ksteps * 32 * mt * 32;
        SI_TRY(pl.tf_mel_tiled.reserve((size_t)total * sizeof(float)));
        hipLaunchKernelGGL(k_mel_tile, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, pl.stream,
                           pl.tf_mel.template as<float>(), pl.tf_mel_tiled.template as<float>(), pl.n_freq, n_mels, mt * 32,
                           total);
        SI_HIP(hipGetLastError());
        SI_TRY(pl.tf_mel_tiled_t.reserve((size_t)total * sizeof(float)));
        hipLaunchKernelGGL(k_mel_tile_t, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, pl.stream,
                           pl.tf_mel.template as<float>(), pl.tf_mel_tiled_t.template as<float>(), pl.n_freq, n_mels, mt * 32,
                           total);
        SI_HIP(hipGetLastError());
      }
      // the operands of the one-launch kernels (one-sided spectra on the wave-level FFT), built on the host from the filterbank
      const int mt16 = obj_mel_tiles(n_mels, pl.fast.xform_R);
      const bool bands = n_mels <= 16 * 9;
      if ((mt16 > 0 || bands) && pl.cfg.onesided && pl.fast.xform_ok && (pl.fast.xform_R == 8 || pl.fast.xform_R == 16)) {
        std::vector<float> h_mel((size_t)n_mels * pl.n_freq);
        SI_HIP(hipMemcpyAsync(h_mel.data(), pl.tf_mel.p, h_mel.size() * sizeof(float), hipMemcpyDeviceToHost, pl.stream));
        SI_HIP(hipStreamSynchronize(pl.stream));
        if (mt16 > 0) {       // operand tiles of k_objective_logmel<R, MT> (kernels_objective.h)
          std::vector<float> hA, hB;
          std::vector<int> h_tab;
          fast::obj_build_blocks(h_mel.data(), pl.n_freq, n_mels, mt16, hA, hB, h_tab);
          SI_TRY(pl.tf_mel_a.reserve(hA.size() * sizeof(float)));
          SI_TRY(pl.tf_mel_b.reserve(hB.size() * sizeof(float)));
          SI_TRY(pl.tf_obj_tab.reserve(h_tab.size() * sizeof(int)));
          SI_HIP(hipMemcpy(pl.tf_mel_a.p, hA.data(), hA.size() * sizeof(float), hipMemcpyHostToDevice));
          SI_HIP(hipMemcpy(pl.tf_mel_b.p, hB.data(), hB.size() * sizeof(float), hipMemcpyHostToDevice));
          SI_HIP(hipMemcpy(pl.tf_obj_tab.p, h_tab.data(), h_tab.size() * sizeof(int), hipMemcpyHostToDevice));
          pl.tf_obj_mt = mt16;
        }
        if (bands) {
          // ... its band form, when the filterbank is sparse enough (a mel filterbank is): k_objective_logmel<R, 9, false, true>
          std::vector<float> blob;
          std::vector<int> h_tab;
          const int uni = pl.fast.xform_R == 16 ? fast::ObjGeo<16, 9>::UNI : fast::ObjGeo<8, 9>::UNI;
          fast::ObjSparseInfo inf;
          if (fast::obj_build_sparse(h_mel.data(), pl.n_freq, n_mels, uni, blob, h_tab, inf)) {
            SI_TRY(pl.tf_sp_blob.reserve(blob.size() * sizeof(float)));
            SI_TRY(pl.tf_sp_tab.reserve(h_tab.size() * sizeof(int)));
            SI_HIP(hipMemcpy(pl.tf_sp_blob.p, blob.data(), blob.size() * sizeof(float), hipMemcpyHostToDevice));
            SI_HIP(hipMemcpy(pl.tf_sp_tab.p, h_tab.data(), h_tab.size() * sizeof(int), hipMemcpyHostToDevice));
            pl.tf_sp = inf;
            pl.tf_sp_ok = true;
          }
          // ... and the tables of the frame walk (kernels_objective_walk.h)
          std::vector<float> wblob;
          fast::ObjWalkInfo winf;
          if (fast::obj_build_walk(h_mel.data(), pl.n_freq, n_mels, pl.fast.xform_R, wblob, winf)) {
            SI_TRY(pl.tf_walk_blob.reserve(wblob.size() * sizeof(float)));
            SI_HIP(hipMemcpy(pl.tf_walk_blob.p, wblob.data(), wblob.size() * sizeof(float), hipMemcpyHostToDevice));
            pl.tf_walk = winf;
            pl.tf_walk_ok = true;
          }
        }
      }
    }
  }
  pl.tf_kind = kind;
  return SPECINV_OK;
}

template <typename P, typename T>
int tf_mel_forward(P& pl) {
  const int64_t BT = (int64_t)pl.B() * pl.Tn();
  SI_TRY(pl.tf_v.reserve((size_t)BT * pl.tf_mels * sizeof(T)));
  if constexpr (std::is_same<T, float>::value) {
    const int mt = (pl.tf_mels + 31) / 32;
    if (mt <= 4) {
      const void* fn = mt == 1 ? (const void*)k_mel_forward_splitk<1> : mt == 2 ? (const void*)k_mel_forward_splitk<2>
                       : mt == 3 ? (const void*)k_mel_forward_splitk<3> : (const void*)k_mel_forward_splitk<4>;
      const size_t lds = (size_t)4 * (32 * mt * 32 + 32 * 33) * sizeof(float);
      SI_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      const cplx<float>* sp = pl.tf_spec.template as<cplx<float>>();
      const float* ml = pl.tf_mel_tiled.template as<float>();
      float* out = pl.tf_v.template as<float>();
      int64_t bt = BT;
      int F = pl.n_freq, nm = pl.tf_mels;
      void* kargs[] = {&sp, &ml, &out, &bt, &F, &nm};
      SI_HIP(hipLaunchKernel(fn, dim3((unsigned)ceil_div(BT, 32)), dim3(256), kargs, lds, pl.stream));
    } else {
      hipLaunchKernelGGL(k_mel_forward_mfma, dim3((unsigned)ceil_div(BT, 32), (unsigned)ceil_div(pl.tf_mels, 32)), dim3(64), 0,
                         pl.stream, pl.tf_spec.template as<cplx<float>>(), pl.tf_mel.template as<float>(),
                         pl.tf_v.template as<float>(), BT, pl.n_freq, pl.tf_mels);
    }
  } else {
    hipLaunchKernelGGL((k_mel_forward_valu<T>), dim3((unsigned)ceil_div(BT * pl.tf_mels, 256)), dim3(256), 0, pl.stream,
                       pl.tf_spec.template as<cplx<T>>(), pl.tf_mel.template as<T>(), pl.tf_v.template as<T>(), BT, pl.n_freq,
                       pl.tf_mels);
  }
  SI_HIP(hipGetLastError());
  return SPECINV_OK;
}

template <typename P, typename T>
int tf_forward(P& pl, const T* x, int64_t len, T* v_out) {
  SI_CHECK(pl.tf_kind >= 0, SPECINV_ESTATE, "specinv_transform_setup has not been called");
  SI_CHECK(x && v_out, SPECINV_EINVAL, "null pointer");
  using C = cplx<T>;
  SI_TRY(pl.tf_spec.reserve(pl.nspec() * sizeof(C)));
  SI_TRY(pl.stft_internal(x, len, pl.tf_spec.template as<C>()));
  if (pl.tf_kind == SPECINV_TF_MAG) {
    const int64_t n = pl.nspec();
    hipLaunchKernelGGL((k_mag_to_user<T>), dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, pl.stream,
                       pl.tf_spec.template as<C>(), v_out, pl.B(), pl.Tn(), pl.n_freq);
  } else {
    SI_TRY((tf_mel_forward<P, T>(pl)));
    const int64_t n = (int64_t)pl.B() * pl.Tn() * pl.tf_mels;
    hipLaunchKernelGGL((k_log1p_to_user<T>), dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, pl.stream,
                       pl.tf_v.template as<T>(), v_out, pl.B(), pl.Tn(), pl.tf_mels);
  }
  SI_HIP(hipGetLastError());
  return SPECINV_OK;
}

template <typename P, typename T>
int tf_loss_grad(P& pl, const T* x, int64_t len, const T* target, double* loss, T* grad, double* loss_dev = nullptr,
                 bool with_stats = false, const T* stat_d = nullptr) {
  // with_stats: loss_dev[0 .. 4] = {loss, g.d, sum|g|, max|g|, max|d|} (stat_d == nullptr: d = g) - from the objective's own launch
  // where the one-launch kernel serves the configuration, by a pass over g and d otherwise
  SI_CHECK(pl.tf_kind >= 0, SPECINV_ESTATE, "specinv_transform_setup has not been called");
  SI_CHECK(x && target && (loss || loss_dev) && grad, SPECINV_EINVAL, "null pointer");
  SI_CHECK(!with_stats || loss_dev, SPECINV_EINVAL, "statistics go to device memory");
  const ObjKnobs kn = ObjKnobs::read();
  using C = cplx<T>;
  const int64_t BT = (int64_t)pl.B() * pl.Tn();
  {
    const int64_t tcheck = 1 + (len + 2 * pl.pad - pl.N()) / pl.cfg.hop_length;
    SI_CHECK(len + 2 * pl.pad >= pl.N() && tcheck == pl.Tn(), SPECINV_EINVAL,
             "signal length %lld gives %lld frames, plan has %d", (long long)len, (long long)tcheck, pl.Tn());
  }
  if constexpr (std::is_same<T, float>::value) {
    const ObjRoute rt = obj_route(pl, len, kn);
    if (rt.kind != kObjChain) {
      if (with_stats && (((uintptr_t)stat_d | (uintptr_t)grad) & 15) == 0) {
        SI_TRY(pl.tf_rows.reserve((size_t)fast::kObjRows * fast::kObjStatRow * sizeof(double)));
        fast::ObjStatReq sr{};
        sr.d = stat_d;
        sr.rows = pl.tf_rows.template as<double>();
        SI_TRY(tf_loss_grad_fused(pl, rt, x, len, target, nullptr, grad, loss_dev, nullptr, &sr));
        const double numel = (double)BT * (pl.tf_kind == SPECINV_TF_MAG ? pl.n_freq : pl.tf_mels);
        hipLaunchKernelGGL(k_objective_finish_rows, dim3(1), dim3(256), 0, pl.stream, (const double*)sr.rows, 1.0 / numel, loss_dev, 5);
        SI_HIP(hipGetLastError());
        return SPECINV_OK;
      }
      SI_TRY(tf_loss_grad_fused(pl, rt, x, len, target, loss, grad, loss_dev));
      if (with_stats) return lb_stats(pl, (const T*)grad, stat_d ? stat_d : (const T*)grad, (int64_t)pl.B() * len, nullptr, loss_dev + 1);
      return SPECINV_OK;
    }
  }
  // ---- the kernel chain
  SI_CHECK(!kn.require_fused, SPECINV_EUNSUPPORTED, "the one-launch objective does not cover this configuration");
  pl.objective_kind = kObjChain;
  SI_TRY(pl.tf_spec.reserve(pl.nspec() * sizeof(C)));
  SI_TRY(pl.stft_internal(x, len, pl.tf_spec.template as<C>()));
  const int nb = 1024;
  SI_TRY(pl.partials.reserve(std::max<size_t>((size_t)nb, 3 * 1024) * sizeof(double)));
  double numel;
  if (pl.tf_kind == SPECINV_TF_MAG) {
    numel = (double)pl.nspec();
    // the target comes in the caller's (B, F, T) layout; one tiled transpose makes the loss kernel's reads contiguous
    SI_TRY(pl.tf_v.reserve((size_t)pl.nspec() * sizeof(T)));
    SI_TRY((pl.template transpose<T>(target, pl.tf_v.template as<T>(), pl.n_freq, pl.Tn())));
    hipLaunchKernelGGL((k_mag_loss_grad<T>), dim3(nb), dim3(256), 0, pl.stream, pl.tf_spec.template as<C>(),
                       pl.tf_v.template as<T>(), 1, pl.B(), pl.Tn(), pl.n_freq, pl.N(), pl.cfg.onesided, 1.0 / numel,
                       pl.partials.template as<double>());
    SI_HIP(hipGetLastError());
  } else {
    numel = (double)BT * pl.tf_mels;
    SI_TRY((tf_mel_forward<P, T>(pl)));
    hipLaunchKernelGGL((k_logmel_loss_dm<T>), dim3(nb), dim3(256), 0, pl.stream, pl.tf_v.template as<T>(), target, pl.B(),
                       pl.Tn(), pl.tf_mels, 1.0 / numel, pl.partials.template as<double>());
    SI_HIP(hipGetLastError());
    if constexpr (std::is_same<T, float>::value) {
      const int mt = (pl.tf_mels + 31) / 32;
      if (mt <= 4) {
        const void* fn = mt == 1 ? (const void*)k_mel_backward_tiles<1> : mt == 2 ? (const void*)k_mel_backward_tiles<2>
                         : mt == 3 ? (const void*)k_mel_backward_tiles<3> : (const void*)k_mel_backward_tiles<4>;
        const size_t lds = (size_t)(mt * 32 * 33 + 4 * mt * 32 * 32) * sizeof(float);
        SI_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        cplx<float>* sp = pl.tf_spec.template as<cplx<float>>();
        const float* ml = pl.tf_mel_tiled_t.template as<float>();
        const float* dm = pl.tf_v.template as<float>();
        int64_t bt = BT;
        int F = pl.n_freq, nm = pl.tf_mels, nf = pl.N(), os = pl.cfg.onesided;
        void* kargs[] = {&sp, &ml, &dm, &bt, &F, &nm, &nf, &os};
        SI_HIP(hipLaunchKernel(fn, dim3((unsigned)ceil_div(BT, 32)), dim3(256), kargs, lds, pl.stream));
      } else {
        hipLaunchKernelGGL(k_mel_backward_mfma, dim3((unsigned)ceil_div(BT, 32), (unsigned)ceil_div(pl.n_freq, 32)), dim3(64), 0,
                           pl.stream, pl.tf_spec.template as<cplx<float>>(), pl.tf_mel.template as<float>(),
                           pl.tf_v.template as<float>(), BT, pl.n_freq, pl.tf_mels, pl.N(), pl.cfg.onesided);
      }
    } else {
      hipLaunchKernelGGL((k_mel_backward_valu<T>), dim3((unsigned)ceil_div(BT * pl.n_freq, 256)), dim3(256), 0, pl.stream,
                         pl.tf_spec.template as<C>(), pl.tf_mel.template as<T>(), pl.tf_v.template as<T>(), BT, pl.n_freq,
                         pl.tf_mels, pl.N(), pl.cfg.onesided);
    }
    SI_HIP(hipGetLastError());
  }
  // (the sum is finished before the next kernel that uses the partials scratch)
  hipLaunchKernelGGL(k_finish_scaled, dim3(1), dim3(256), 0, pl.stream, pl.partials.template as<double>(), nb, 1.0 / numel,
                     loss_dev ? loss_dev : pl.sums.template as<double>());
  SI_HIP(hipGetLastError());
  // frames of the gradient: irfft-style inverse with the forward scale
  SI_TRY(pl.grad_from_spec(pl.tf_spec.template as<C>(), grad, pl.fc.fwd_scale, len));
  if (with_stats) return lb_stats(pl, (const T*)grad, stat_d ? stat_d : (const T*)grad, (int64_t)pl.B() * len, nullptr, loss_dev + 1);
  if (loss_dev) return SPECINV_OK;
  return obj_read_loss(pl, loss);
}

}  // namespace specinv
