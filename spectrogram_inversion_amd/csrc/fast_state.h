// Host side of the wave-level kernels: FastState<float> picks the kernel, sizes the launch and owns the device state.
#pragma once
#include <algorithm>
#include "dev_buf.h"
#include "fast_core.h"
#include "kernels_layout.h"

namespace specinv {

// ---- host side ---------------------------------------------------------------------------------------
template <typename T>
struct FastState {
  bool supported = false;
  bool semi = false;
  bool hopk = false;
  bool xform_ok = false;
  bool two = false;
  bool keep_state = false;
  bool plain_state = false;
  int n_partials = 0;
  int nchunks = 0, skew = 0, OV = 0;
  int max_partials() const { return 0; }
  T* state_rows() const { return nullptr; }
  const T* state_tails() const { return nullptr; }
  int setup(const specinv_stft_cfg&, const std::vector<T>&, int64_t, int) { return SPECINV_OK; }
  void geometry(int out[4]) const { out[0] = out[1] = out[2] = out[3] = 0; }
  template <typename P>
  int launch_xform(P&, bool, const T*, long long, void*, T*, T, int = -1) { return fail(SPECINV_EUNSUPPORTED, "no fused path"); }
  template <typename P>
  int launch_inverse_ola(P&, const void*, T*, long long, T, T**, bool* used) {
    *used = false;
    return SPECINV_OK;
  }
  template <typename P>
  int begin(P&, int, const void*, const void*, double*) { return fail(SPECINV_EUNSUPPORTED, "no fused path for this dtype"); }
  template <typename P>
  int iterate(P&, int, bool) { return fail(SPECINV_EUNSUPPORTED, "no fused path for this dtype"); }
  template <typename P>
  int get_wave(P&, T*) { return fail(SPECINV_EUNSUPPORTED, "no fused path for this dtype"); }
  template <typename P>
  int get_state_spec(P&, int, cplx<T>*) { return fail(SPECINV_EUNSUPPORTED, "no fused path for this dtype"); }
};

// run STMT with `RR` bound to the compile-time registers-per-lane count R = n_fft / 128
#define SPECINV_R_SWITCH(RV, ...)                      \
  switch (RV) {                                        \
    case 4: { constexpr int RR = 4; __VA_ARGS__; } break;   \
    case 8: { constexpr int RR = 8; __VA_ARGS__; } break;   \
    case 16: { constexpr int RR = 16; __VA_ARGS__; } break; \
    default: { constexpr int RR = 32; __VA_ARGS__; } break; \
  }

// the address of K<..., EARLY, EVAL> (a signal-form kernel; `...`: its leading template arguments) for run-time `early` / `ev`
#define SPECINV_EARLY_EVAL(early, ev, K, ...)                                                                     \
  ((early) ? ((ev) ? (const void*)K<__VA_ARGS__, true, true> : (const void*)K<__VA_ARGS__, true, false>)          \
           : ((ev) ? (const void*)K<__VA_ARGS__, false, true> : (const void*)K<__VA_ARGS__, false, false>))

// The environment knobs of this file, read once when a plan is set up (FastState::setup): what a plan does afterwards does not
// depend on when the environment was last changed.
struct FastKnobs {
  bool disable_fast = false;       // SPECINV_DISABLE_FAST=1: none of the kernels of this file
  bool disable_twosided = false;   // SPECINV_DISABLE_TWOSIDED=1: two-sided spectrograms on the coverage kernels
  bool disable_fused = false;      // SPECINV_DISABLE_FUSED=1 (tests): put the shape on the frame kernel
  bool disable_hop = false;        // SPECINV_DISABLE_HOP=1: no overlap-add on the chip (k_semi + k_ola, inverse frames + gather)
  bool fused_template = false;     // SPECINV_FUSED_TEMPLATE=1 (tests): k_fused<R, 4> where the tuned copy k_fused4<R> would run
  bool eval_kernel = true;         // SPECINV_EVAL_KERNEL=0: the fused evaluating variant where k_eval_td would run
  bool debug = false;              // SPECINV_DEBUG: the chosen launch on stderr
  bool has_small_frames = false;   // SPECINV_SMALL_FRAMES=n: the frame count from which the chunk-walking kernels run (frames_from;
  long long small_frames = 0;      //   tests pin them with 0)
  int fast_chunk = 0;              // SPECINV_FAST_CHUNK=n: frames per chunk (experiments; 0: the planner's choice)
  int cu_budget = 0;               // SPECINV_CU_BUDGET=k: plan for a chip of 256 - k compute units (setup)
  bool has_k4_skew = false;        // SPECINV_K4_SKEW="s1,s2" (experiments; "0,0" switches the chunk triples off)
  int k4_s1 = 0, k4_s2 = 0;
  bool has_td_skew = false;        // SPECINV_TD_SKEW=n (experiments; 0 switches the skewed chunk pairs off)
  int td_skew = 0;

  static FastKnobs read() {
    auto starts = [](const char* name, char c) {
      const char* e = getenv(name);
      return e != nullptr && e[0] == c;
    };
    FastKnobs k;
    k.disable_fast = starts("SPECINV_DISABLE_FAST", '1');
    k.disable_twosided = starts("SPECINV_DISABLE_TWOSIDED", '1');
    k.disable_fused = starts("SPECINV_DISABLE_FUSED", '1');
    k.disable_hop = starts("SPECINV_DISABLE_HOP", '1');
    k.fused_template = starts("SPECINV_FUSED_TEMPLATE", '1');
    k.eval_kernel = !starts("SPECINV_EVAL_KERNEL", '0');
    k.debug = getenv("SPECINV_DEBUG") != nullptr;
    if (const char* e = getenv("SPECINV_SMALL_FRAMES")) {
      k.has_small_frames = true;
      k.small_frames = atoll(e);
    }
    if (const char* e = getenv("SPECINV_FAST_CHUNK")) k.fast_chunk = atoi(e);
    if (const char* e = getenv("SPECINV_CU_BUDGET")) k.cu_budget = atoi(e);
    if (const char* e = getenv("SPECINV_K4_SKEW")) k.has_k4_skew = sscanf(e, "%d,%d", &k.k4_s1, &k.k4_s2) == 2;
    if (const char* e = getenv("SPECINV_TD_SKEW")) {
      k.has_td_skew = true;
      k.td_skew = atoi(e);
    }
    return k;
  }
  // a frame-count threshold: the measured crossover unless SPECINV_SMALL_FRAMES overrides it
  long long frames_from(long long measured) const { return has_small_frames ? small_frames : measured; }
};

// Frames per wave.  A launch takes about rounds x (longest chunk) frame times, rounds = ceil(waves / wave slots), e.g. 64 x 1024
// frames on 2048 slots -> 32 chunks of 32 (2048 waves, one round), 96 x 1024 -> 21 chunks of 49 (2016 waves, one round) instead of
// 32 chunks (3072 waves, two rounds).
// (+2: what a chunk boundary costs - split blocks, pipeline fill; measured: 2 rounds of 16-frame chunks are 8 % slower than 1 round
// of 32.  Last factor: chunks beyond 32 frames measured ~5 % slower than two rounds of 32)
inline double chunk_cost(int batch, int n_frames, int nch, long long slots) {
  const long long waves = (long long)batch * nch;
  const long long rounds = (waves + slots - 1) / slots;
  const int longest = (n_frames + nch - 1) / nch;
  return (double)rounds * (longest + 2.0) * (1.0 + 0.0015 * std::max(0, longest - 32));
}
struct ChunkPick {
  int nch = 0;
  double cost = 1e300;
};
// the cheapest count of chunks per item among the multiples of `mult` in [lo, hi] (nch = 0: there is none); of costs within `tie`
// of each other the larger count wins
inline ChunkPick pick_chunks(int batch, int n_frames, long long slots, int lo, int hi, int mult = 1, double tie = 1e-9) {
  ChunkPick best;
  for (int nch = lo; nch <= hi; ++nch) {
    if (nch % mult != 0) continue;
    const double cost = chunk_cost(batch, n_frames, nch, slots);
    if (cost < best.cost + tie) best = ChunkPick{nch, cost};
  }
  return best;
}

// the kernel FastState<float>::geometry reports (specinv_plan_launch_geometry, out[3]; plan.py's table of names goes by these values)
enum FastKernel {
  kKernelFused4 = 1,     // k_fused4
  kKernelFused = 2,      // k_fused<R, OV>
  kKernelSemi = 3,       // k_semi
  kKernelHop = 4,        // k_hop
  kKernelFused4Td = 5,   // k_fused4_td (hop = n_fft / 4 at n_fft 1024 / 2048)
  kKernelFusedTd = 6,    // k_fused_td<R, OV> otherwise
  kKernelHopTd = 7,      // k_hop_td
};

template <>
struct FastState<float> {
  using v2f = fast::v2f;
  using v4f = fast::v4f;
  bool supported = false;
  bool semi = false;   // frame kernels instead of k_fused (hop != n_fft/2, /4, /8, centre = False, small problems)
  bool hopk = false;   // ... k_hop (overlap-add in LDS, chunks of frames) rather than k_semi + k_ola
  int semi_grid = 0;
  int R = 0;
  int OV = 0;          // n_fft / hop of the fused kernel (2, 4 or 8)
  FastKnobs knobs;
  int chunk = 32, nchunks = 0, n_waves = 0, n_partials = 0;
  int skew = 0;        // frames every odd chunk cedes to the even chunk before it (chunk_begin; set per Griffin-Lim run in begin_t)
  int cur = 0;   // index of the signal buffers (xb, xtail, zb) holding the current state
  int mode = fast::MODE_GLA;
  // x (and the chunk tails) ping-pong between iterations; the spectral state of a frame is read and written by the same lane, so it
  // lives in one buffer (Pb, Pmid: same speed as ping-pong buffers, measured; a third less memory)
  DevBuf xb[2], xtail[2], Pb, Pmid, mpairs, mmid, scratch;
  // a two-sided spectrogram (onesided=False): the frame kernel k_semi2 with the mirror bins' state and target beside the lower
  // half's (FastArgs::P2_out); no fused / chunked / signal-form kernels, no stand-alone transforms
  bool two = false;
  DevBuf Pb2, Pmid2, mpairs2, mmid2;
  // ADMM carries Y = X + U in Pb (FastArgs).  X and U themselves are only written when the caller has asked for them
  // (specinv_plan_keep_state), by the last iteration of every iterate() call.
  bool keep_state = false, xu_valid = false;
  DevBuf Xb, Xmid, Ub, Umid;
  // A method that edits the signal between two launches (MISI's coupling step, kernels_misi.h) runs Griffin-Lim on the kernels
  // that keep it as xb[cur] (+ xtail[cur] on the fused kernels), never in the signal form below - the routing keep_state selects.
  // state_rows(): the rows the next launch reads; state_tails(): the chunk tails it adds on load (nullptr: the rows are whole)
  bool plain_state = false;
  float* state_rows() const { return xb[cur].template as<float>(); }
  const float* state_tails() const { return (!semi && nchunks > 1) ? xtail[cur].template as<float>() : nullptr; }
  // Griffin-Lim on k_fused4_td: the momentum state is the signal z (zb), Pb keeps the starting spectrum c0
  bool td = false;
  int td_t = 0;          // closure calls so far (z_1 = x_1: the first call reads x itself)
  DevBuf zb[2];

  // the optional X / U outputs of an ADMM iteration (`last`: the last iteration of an iterate() call)
  template <typename P>
  int want_xu(P& pl, fast::FastArgs& a, bool last) {
    if (mode != fast::MODE_ADMM) return SPECINV_OK;
    xu_valid = false;
    if (!keep_state || !last) return SPECINV_OK;
    SI_TRY(reserve_xu(pl));
    a.X_out = Xb.template as<v4f>();
    a.U_out = Ub.template as<v4f>();
    a.Xmid_out = Xmid.template as<v2f>();
    a.Umid_out = Umid.template as<v2f>();
    xu_valid = true;
    return SPECINV_OK;
  }
  template <typename P>
  int reserve_xu(P& pl) {
    const long long nf = (long long)pl.B() * pl.Tn();
    const size_t pbytes = (size_t)nf * (R / 2) * 64 * sizeof(v4f);
    SI_TRY(Xb.reserve(pbytes));
    SI_TRY(Ub.reserve(pbytes));
    SI_TRY(Xmid.reserve(nf * sizeof(v2f)));
    SI_TRY(Umid.reserve(nf * sizeof(v2f)));
    return SPECINV_OK;
  }

  int setup(const specinv_stft_cfg& cfg, const std::vector<float>&, int64_t length, int pad) {
    supported = false;
    xform_ok = false;
    two = false;
    if (cfg.dtype != SPECINV_F32) return SPECINV_OK;
    knobs = FastKnobs::read();
    if (knobs.disable_fast) return SPECINV_OK;
    const bool size_ok = cfg.n_fft == 512 || cfg.n_fft == 1024 || cfg.n_fft == 2048 || cfg.n_fft == 4096;
    if (!size_ok) return SPECINV_OK;
    if (!cfg.onesided) {
      // two-sided: the frame kernels only - k_semi2 + gather overlap-add, or k_hop2 over chunks of frames (round 5;
      // SPECINV_DISABLE_TWOSIDED=1: the coverage kernels); no fused / signal-form kernels, no stand-alone transforms
      if (knobs.disable_twosided) return SPECINV_OK;
      if (pad >= length) return SPECINV_OK;
      two = true;
    } else {
      xform_ok = true;              // any hop, any pad mode, centred or not
      xform_R = cfg.n_fft / 128;
    }
    R = cfg.n_fft / 128;
    semi = false;
    // fused kernel: hop = n_fft / 2, / 4 or / 8 (whole registers per hop-block), centred, enough frames
    OV = 0;
    for (int o : {2, 4, 8})
      if (cfg.hop_length * o == cfg.n_fft && R % o == 0) OV = o;
    if (two || knobs.disable_fused) OV = 0;
    const long long n_all = (long long)cfg.batch * cfg.n_frames;
    // small problems are latency-bound on the fused kernel (a wave walks >= 8 frames one after the other): below
    // ~6 k frames the frame kernel, one frame per wave, finishes an iteration sooner (measured: 1 x 512 frames at
    // n_fft 1024 10 vs 27 us, 16 x 256 26 vs 32 us; 16 x 512 at n_fft 2048 69 vs 55 us)
    const bool small = n_all < knobs.frames_from(6144);
    if (!cfg.center || OV == 0 || cfg.n_frames < OV + 2 || pad >= length || small) {
      // any other hop / centring: frame kernel on the wave-level FFT + gather overlap-add (k_semi)
      semi = true;
      hopk = false;
      OV = 0;
      chunk = cfg.n_frames;
      nchunks = 1;
      semi_grid = (int)std::min<long long>((n_all + 3) / 4, 256 * 8);
      n_waves = semi_grid * 4;
      supported = true;
      // Large enough problems keep the overlap-add on the chip (k_hop): a wave per chunk of frames, 8-wave workgroups,
      // one per CU (2048 wave slots).  A chunk must emit the n_fft - hop samples it shares with its predecessor with
      // its regular frames: at least (n_fft - 1) / hop + 1 frames.  n_fft 4096 does not fit (ring + scratch in LDS).
      // (a wave walks >= 8 frames one after the other there: measured against k_semi + k_ola, it pays from ~12 k frames
      // at n_fft 2048 and ~32 k frames at 1024 and 512)
      // (round 5's sweep, n_fft 2048 / hop 333, T 300: B 48 = 14 400 frames 145 M against 128 M it*frames/s for k_semi + k_ola,
      // B 32 = 9 600 frames 102 against 120: the crossover at n_fft 2048 is nearer 12 k; n_fft 1024 / hop 300 at 14 400: 260 vs 257)
      const bool want_hop = !knobs.disable_hop && R <= 16 && n_all >= knobs.frames_from(R >= 16 ? 12288 : 32768) && !small &&
                            cfg.hop_length >= 1 && cfg.hop_length <= cfg.n_fft && pad < length;
      if (want_hop) {
        const int floor_ch = std::max(8, (cfg.n_fft - 1) / cfg.hop_length + 1);
        // wave slots: one 8-wave workgroup per CU at n_fft 2048 (LDS), two at 1024, three at 512 (registers allow it)
        const long long slots = R >= 16 ? 2048 : R == 8 ? 4096 : 6144;
        hopk = true;
        nchunks = pick_chunks(cfg.batch, cfg.n_frames, slots, 1, std::max(1, cfg.n_frames / floor_ch)).nch;
        if (knobs.fast_chunk >= 1) nchunks = std::max(1, cfg.n_frames / std::min(std::max(knobs.fast_chunk, floor_ch), cfg.n_frames));
        chunk = (cfg.n_frames + nchunks - 1) / nchunks;
        n_waves = cfg.batch * nchunks;
        if (knobs.debug) fprintf(stderr, "specinv: frame kernel with LDS overlap-add R=%d hop=%d chunks=%d of <=%d frames, %d waves\n", R, cfg.hop_length, nchunks, chunk, n_waves);
      }
      return SPECINV_OK;
    }
    // Frames per wave: the chunk count that minimises chunk_cost (the chip holds 2 waves of these kernels per SIMD, 3 at n_fft
    // 512, 1 at 4096).  A chunk boundary costs OV - 1 split hop-blocks, and the reflected edge samples must not fall on split
    // blocks (first / last chunk long enough): chunks of >= 8 (16) frames.
    const int floor_ch = OV == 8 ? 16 : 8;
    long long slots = 1024LL * (R >= 32 ? 1 : R <= 4 ? 3 : 2);
    if (R == 8) slots = 1024LL * fast::kR8Waves;
    // SPECINV_CU_BUDGET=k: plan the launch for a chip of 256 - k compute units - the chunk count is chosen so that one round of
    // workgroups leaves k CUs free.  For multi-GPU runs whose RCCL gather overlaps the next step's launches: an iteration
    // workgroup takes a whole CU's registers, so RCCL's workgroups can only run beside a launch that does not fill the chip
    // (bench.py --gather-kernel-budget; C2: 30 chunks of 34 frames on 240 CUs instead of 32 x 32 on 256: +6 % per launch).
    if (knobs.cu_budget > 0 && knobs.cu_budget < 256) slots = slots * (256 - knobs.cu_budget) / 256;
    const int most = std::max(1, cfg.n_frames / floor_ch);
    ChunkPick best = pick_chunks(cfg.batch, cfg.n_frames, slots, 1, most);
    // The waves of a SIMD do not run at the same speed (begin_t: skewed chunks): where the skew applies - hop = n_fft/4 at n_fft
    // 2048 (chunk pairs) and 1024 (chunk triples) - a chunk count that pairs / triples up is preferred when it costs at most 4 %
    // more frame times than the best one (round 5: B 65 or 100 at T 1024 took 31 / 20 chunks and ran unskewed); of two that cost
    // the same, the smaller
    if (OV == 4 && (R == 16 || R == 8)) {
      const int mult = R == 16 ? 2 : 3;
      if (best.nch % mult != 0) {
        const ChunkPick pick = pick_chunks(cfg.batch, cfg.n_frames, slots, std::max(mult, best.nch - mult), std::min(best.nch + mult, most), mult, 0.0);
        if (pick.nch > 0 && pick.cost <= 1.04 * best.cost) best = pick;
      }
    }
    nchunks = best.nch;
    if (knobs.fast_chunk >= 4) nchunks = std::max(1, cfg.n_frames / std::min(std::max(knobs.fast_chunk, OV == 8 ? 13 : 4), cfg.n_frames));
    chunk = (cfg.n_frames + nchunks - 1) / nchunks;   // frames split as evenly as possible (sizes differ by at most one)
    n_waves = cfg.batch * nchunks;
    if (knobs.debug) fprintf(stderr, "specinv: fused R=%d OV=%d chunks=%d of <=%d frames, %d waves (%lld slots)\n", R, OV, nchunks, chunk, n_waves, slots);
    supported = true;
    return SPECINV_OK;
  }

  // The FastArgs fields every launch shares; a call site adds the signal and state pointers that are its own.  Every kernel gets
  // all of them: k_semi never reads env, nchunks, n_waves or skew, the k_hop family reads its env from HopArgs and has no skew (it is
  // 0 whenever `semi`: begin_t), k_fused_istft reads neither the target nor partials, pad_mode, coef and inv1p.
  template <typename P>
  fast::FastArgs base_args(P& pl) const {
    fast::FastArgs a{};
    a.m_pairs = mpairs.template as<v4f>();
    a.m_mid = mmid.template as<float>();
    if (two) {
      a.P2_out = Pb2.template as<v4f>();
      a.Pmid2_out = Pmid2.template as<v2f>();
      a.m2_pairs = mpairs2.template as<v4f>();
      a.m2_mid = mmid2.template as<float>();
    }
    a.window = pl.window.template as<float>();
    a.env = pl.env.template as<float>();
    a.partials = pl.partials_out();
    a.T = pl.Tn();
    a.nchunks = nchunks;
    a.skew = skew;
    a.n_waves = n_waves;
    a.pad_mode = pl.cfg.pad_mode;
    a.L = pl.length;
    a.coef = pl.coef;
    a.inv1p = 1.0f / (float)(1.0 + (double)pl.coef);
    a.fwd_scale = pl.fc.fwd_scale;
    a.inv_scale = pl.fc.inv_scale;
    return a;
  }

  // fn(args) over `waves` waves: ceil(waves / wgw) workgroups of wgw waves, `lds` bytes of dynamic LDS each
  template <typename P, typename A>
  static int launch_waves(P& pl, const void* fn, const A& args, int waves, int wgw, size_t lds) {
    SI_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    A copy = args;
    void* kargs[] = {&copy};
    SI_HIP(hipLaunchKernel(fn, dim3((waves + wgw - 1) / wgw), dim3(64 * wgw), kargs, lds, pl.stream));
    return SPECINV_OK;
  }

  // `spec_user` (B, F, T) complex and `mag_user` (B, F, T) are the caller's / phase_init's arrays
  // spec_user == nullptr: the starting spectrum is phase_init(mag_user), produced in pair order by k_phase_init_pairs
  template <int RR, typename P>
  int begin_t(P& pl, int md, const v2f* spec_user, const float* mag_user, double* sum_m2_out) {
    using G = fast::Geo<RR>;
    const int hop = pl.cfg.hop_length;
    mode = md;
    // (n_fft 4096 runs one wave per SIMD: its vector latency, not the state traffic, is what bounds it there - the signal form
    // measured 0.360 against 0.340 ms per iteration and is not used)
    td = md == fast::MODE_GLA && (!semi || hopk) && !knobs.fused_template && !keep_state && !plain_state && RR <= 16 && !two;
    // (the signal-form kernels leave the real-FFT split unscaled, which is exact only for a power-of-two fwd_scale / 2)
    if (pl.cfg.normalized && !hopk) td = false;
    // k_hop_td writes two signals and re-reads z_t where k_hop writes one: at large hops its emission loop overtakes the saved state
    // traffic.  Measured crossovers (late iterations, 65 536 frames, tools/log/EXPERIMENTS.md r02 hop_td2), emission two samples at a time (even hop,
    // padding and length) / one at a time: n_fft 2048: wins up to hop 768 (0.350 vs 0.367 ms), loses at 1000 / wins at 333, loses at
    // 601; n_fft 1024: wins everywhere measured (hop 800: 0.195 vs 0.240) / wins at 301; n_fft 512: wins at 300, loses at 400 / wins
    // at 100, loses at 201
    const bool emit_pairs = ((hop | pl.pad) & 1) == 0 && (pl.length & 1) == 0;
    int hop_td_max = emit_pairs ? (RR == 4 ? 320 : RR == 8 ? 1024 : 800) : (RR == 4 ? 128 : RR == 8 ? 448 : 416);
    if (hopk && hop > hop_td_max) td = false;
    td_t = 0;
    // Skewed chunks.  Two waves share a SIMD and the arbiter serves the OLDER one first whenever both have an instruction ready:
    // at BASELINE C2 the wave in hardware slot 0 ran 0.132 frames per kilotick against its neighbour's 0.077 and finished after
    // 69 % of the launch (237 k against 337 k ticks on every one of the 1024 SIMDs); the neighbour ran the last
    // third alone at 0.143 - a SIMD with two waves does 0.209.  Chunks of 42 and 22 frames instead of 32 and 32 let both finish
    // nearly together (late launch 0.172-0.176 -> 0.166-0.168 ms at 8 ... 10 frames of skew, 0.169 / 0.172 at 12 / 14; the
    // evaluating launches and the initial ISTFT like less of it: whole C2 step 20.54 / 20.18 / 20.12 / 20.14 / 20.41 ms at
    // 0 / 6 / 8 / 10 / 12, tools/log/EXPERIMENTS.md r03 skewstep; the other overlaps of n_fft 2048 gain 3.5 % (hop 256) and 2 % (hop 1024)
    // at the same 8, r03 skew_ov).  Only for
    // the launch shape this was measured on - the signal-form kernel at two waves per SIMD with exactly as many waves as the
    // chip has slots for them (BASELINE C2 per GPU: 2048).  SPECINV_TD_SKEW overrides (experiments; 0 switches it off).
    // Also tried: s_setprio by frame parity or by time slice so that the two waves take turns (-2...3 %, no better with the skew).
    // Round 5: not only at the launch shape this was measured on.  With one 8-wave workgroup per CU (fused_wgw) waves i and i + 4
    // of a workgroup share a SIMD whatever the number of workgroups or rounds, so the pairing holds for any launch that puts two
    // waves on a SIMD (more waves than SIMDs); the skew scales with the chunk: a quarter of its frames (10 of 32 at C2), the
    // shorter chunk keeping >= 8 (the floor of a chunk: its seams).
    // (every rule below asks for !semi: the frame kernels, k_hop's chunks included, always run with skew = 0)
    skew = 0;
    {
      const int len_ch = pl.Tn() / std::max(1, nchunks);
      if (td && !semi && RR == 16 && OV == 4 && n_waves > 1024 && (nchunks & 1) == 0 && len_ch >= 12) {
        constexpr int kSkewC2 = 10;   // frames, at BASELINE C2's launch shape (2048 waves, chunks of 32): measured above
        skew = n_waves == 2048 && len_ch == 32 ? kSkewC2 : std::min((len_ch + 2) / 4, len_ch - 8);
        if (skew < 2) skew = 0;
      }
      // ... and the n_fft 1024 kernels (spectral state or signal form) at three waves per SIMD (12-wave workgroups, the hardware
      // slot is the wave's index in the workgroup / 4, kernels_fused.h): chunk triples, the oldest wave the longest.  BASELINE
      // C4's shard: 3072 waves, chunks of 64 frames, begin shifts 4 / 6; other chunk lengths scale them.
      if (!semi && RR == 8 && OV == 4 && !knobs.fused_template && fused_wgw() == 12 && nchunks % 3 == 0 && len_ch >= 16) {
        // (C4 step, two runs each: "0,0" 30.38 / 30.38 ms, "3,4" 30.29 / 30.26, "4,6" 29.93 / 29.97, "5,8" 30.49 / 30.20, "6,9"
        // 30.27 / 30.21: the kernel sits on the memory system, the balance buys 1.4 %)
        constexpr int kSkew1 = 4, kSkew2 = 6;
        const int s1 = len_ch == 64 ? kSkew1 : (kSkew1 * len_ch + 32) / 64;
        const int s2 = len_ch == 64 ? kSkew2 : (kSkew2 * len_ch + 32) / 64;
        if ((s1 | s2) && len_ch - s2 >= 8 && len_ch + s2 - s1 >= 8) skew = 0x10000 | (s1 << 8) | s2;
      }
    }
    if (knobs.has_k4_skew) {
      const int s1 = knobs.k4_s1, s2 = knobs.k4_s2;
      if (!semi && fused_wgw() == 12 && nchunks % 3 == 0 && n_waves % 12 == 0 && s1 >= 0 && s2 >= 0 && s1 < 200 && s2 < 200 &&
          pl.Tn() / nchunks - s2 >= 8 && pl.Tn() / nchunks + s2 - s1 >= 8)
        skew = (s1 | s2) ? (0x10000 | (s1 << 8) | s2) : 0;
    }
    if (knobs.has_td_skew) {
      const int v = knobs.td_skew;
      if (v == 0 || (td && !semi && (nchunks & 1) == 0 && (n_waves & 1) == 0 && pl.Tn() / nchunks - v >= 8)) skew = v;
    }
    if (td) {
      SI_TRY(zb[0].reserve((size_t)pl.B() * pl.length * sizeof(float)));
      SI_TRY(zb[1].reserve((size_t)pl.B() * pl.length * sizeof(float)));
    }
    const long long nf = (long long)pl.B() * pl.Tn();
    const size_t pbytes = (size_t)nf * G::H * 64 * sizeof(v4f);
    const size_t tail_bytes = (size_t)pl.B() * nchunks * (OV > 0 ? OV - 1 : 0) * hop * sizeof(float);
    if (hopk) SI_TRY(xtail[0].reserve((size_t)pl.B() * nchunks * (pl.N() - hop) * sizeof(float) + 16));
    for (int i = 0; i < ((semi && !hopk) ? 1 : 2); ++i) {     // (k_semi + k_ola rewrite x in place)
      if (!semi) SI_TRY(xtail[i].reserve(tail_bytes));
      SI_TRY(xb[i].reserve((size_t)pl.B() * pl.length * sizeof(float)));
    }
    SI_TRY(Pb.reserve(pbytes));
    SI_TRY(Pmid.reserve(nf * sizeof(v2f)));
    if (semi && !hopk) SI_TRY(pl.frames_needed());
    SI_TRY(mpairs.reserve((size_t)nf * (G::H / 2) * 64 * sizeof(v4f)));
    SI_TRY(mmid.reserve(nf * sizeof(float)));
    if (two) {
      SI_TRY(Pb2.reserve(pbytes));
      SI_TRY(Pmid2.reserve(nf * sizeof(v2f)));
      SI_TRY(mpairs2.reserve((size_t)nf * (G::H / 2) * 64 * sizeof(v4f)));
      SI_TRY(mmid2.reserve(nf * sizeof(float)));
    }
    cur = 0;
    SI_CHECK(!two || spec_user != nullptr, SPECINV_ESTATE, "the two-sided frame kernel takes its starting spectrum in the user layout");
    if (spec_user == nullptr) {
      const int nwg = pl.B() * G::H;
      SI_TRY(pl.partials.reserve(std::max<size_t>((size_t)nwg, 3 * 1024) * sizeof(double)));
      const size_t lds = (size_t)64 * 129 * (sizeof(v2f) + sizeof(float));
      const void* fn = (const void*)fast::k_phase_init_pairs<RR>;
      SI_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      const float* mg = mag_user;
      v4f* pp = Pb.template as<v4f>();
      v2f* pm = Pmid.template as<v2f>();
      float* mp = mpairs.template as<float>();
      float* mm = mmid.template as<float>();
      double* part = pl.partials.template as<double>();
      int Tn = pl.Tn(), hp = hop;
      void* kargs[] = {&mg, &pp, &pm, &mp, &mm, &part, &Tn, &hp};
      SI_HIP(hipLaunchKernel(fn, dim3(nwg), dim3(1024), kargs, lds, pl.stream));
      hipLaunchKernelGGL(k_finish_partials, dim3(1), dim3(256), 0, pl.stream, pl.partials.template as<double>(), (int64_t)nwg, 1,
                         pl.sums.template as<double>() + 4);
      SI_HIP(hipGetLastError());
      SI_HIP(hipMemcpyAsync(sum_m2_out, pl.sums.template as<double>() + 4, sizeof(double), hipMemcpyDeviceToHost, pl.stream));
    } else {
      const int rows = pl.n_freq;                   // G::M + 1, or N for a two-sided spectrogram
      const dim3 grid((pl.Tn() + 31) / 32, (G::M + 1 + 31) / 32, pl.B()), blk(32, 8);
      hipLaunchKernelGGL((fast::k_user_spec_to_pairs<RR>), grid, blk, 0, pl.stream, spec_user, Pb.template as<v2f>(),
                         Pmid.template as<v2f>(), pl.Tn(), rows, 0);
      SI_HIP(hipGetLastError());
      const long long nblk1 = (long long)grid.x * grid.y * grid.z, nblk = two ? 2 * nblk1 : nblk1;
      SI_TRY(pl.partials.reserve(std::max<size_t>((size_t)nblk, 3 * 1024) * sizeof(double)));
      hipLaunchKernelGGL((fast::k_user_mag_to_pairs<RR>), grid, blk, 0, pl.stream, mag_user, mpairs.template as<float>(),
                         mmid.template as<float>(), pl.Tn(), pl.partials.template as<double>(), rows, 0);
      SI_HIP(hipGetLastError());
      if (two) {                                    // the mirror rows N - f into the same layout (sum of m^2: their partials behind)
        hipLaunchKernelGGL((fast::k_user_spec_to_pairs<RR>), grid, blk, 0, pl.stream, spec_user, Pb2.template as<v2f>(),
                           Pmid2.template as<v2f>(), pl.Tn(), rows, 1);
        hipLaunchKernelGGL((fast::k_user_mag_to_pairs<RR>), grid, blk, 0, pl.stream, mag_user, mpairs2.template as<float>(),
                           mmid2.template as<float>(), pl.Tn(), pl.partials.template as<double>() + nblk1, rows, 1);
        SI_HIP(hipGetLastError());
      }
      hipLaunchKernelGGL(k_finish_partials, dim3(1), dim3(256), 0, pl.stream, pl.partials.template as<double>(), nblk, 1,
                         pl.sums.template as<double>() + 4);
      SI_HIP(hipGetLastError());
      SI_HIP(hipMemcpyAsync(sum_m2_out, pl.sums.template as<double>() + 4, sizeof(double), hipMemcpyDeviceToHost, pl.stream));
    }
    xu_valid = false;
    if (md == fast::MODE_ADMM && keep_state) {      // methods.py:447-449: X = the start spectrum, U = 0 (Y = X is already in Pb)
      SI_TRY(reserve_xu(pl));
      SI_HIP(hipMemcpyAsync(Xb.p, Pb.p, pbytes, hipMemcpyDeviceToDevice, pl.stream));
      SI_HIP(hipMemcpyAsync(Xmid.p, Pmid.p, nf * sizeof(v2f), hipMemcpyDeviceToDevice, pl.stream));
      SI_HIP(hipMemsetAsync(Ub.p, 0, pbytes, pl.stream));
      SI_HIP(hipMemsetAsync(Umid.p, 0, nf * sizeof(v2f), pl.stream));
      xu_valid = true;
    }
    if (semi) {
      // x0 = ISTFT(start spectrum): synthesis frames from the pair layout, then the overlap-add
      if constexpr (RR <= 16) {
        if (hopk) SI_TRY((launch_hop<RR, fast::MODE_INIT, false>(pl)));
      }
      if (!hopk) SI_TRY((launch_semi<RR, fast::MODE_INIT, false>(pl)));
      SI_HIP(hipStreamSynchronize(pl.stream));   // *sum_m2_out is valid from here on
      return SPECINV_OK;
    }
    SI_HIP(hipMemsetAsync(xtail[0].p, 0, tail_bytes, pl.stream));   // x0 below is written whole
    // x0 = ISTFT(start spectrum) (methods.py:233 / :453) straight from the pair layout
    fast::FastArgs a = base_args(pl);
    a.x_out = xb[0].template as<float>();
    a.P_in = Pb.template as<v4f>();
    a.Pmid_in = Pmid.template as<v2f>();
    const void* fn = nullptr;
    if constexpr (RR % 8 == 0) {
      if (OV == 8) fn = (const void*)fast::k_fused_istft<RR, 8>;
    }
    if (OV == 4) fn = (const void*)fast::k_fused_istft<RR, 4>;
    if (OV == 2) fn = (const void*)fast::k_fused_istft<RR, 2>;
    SI_CHECK(fn != nullptr, SPECINV_EUNSUPPORTED, "no fused kernel for n_fft / hop = %d", OV);
    SI_TRY(launch_waves(pl, fn, a, n_waves, 4, G::lds_bytes(4)));
    SI_HIP(hipStreamSynchronize(pl.stream));   // *sum_m2_out is valid from here on
    return SPECINV_OK;
  }

  template <typename P>
  int begin(P& pl, int md, const void* spec_user, const void* mag_user, double* sum_m2_out) {
    const v2f* s = static_cast<const v2f*>(spec_user);
    const float* m = static_cast<const float*>(mag_user);
    int rc = SPECINV_OK;
    SPECINV_R_SWITCH(R, rc = begin_t<RR>(pl, md, s, m, sum_m2_out));
    return rc;
  }

  // wave-level FFT usable for stand-alone transforms of this plan (any hop / frame count)
  bool xform_ok = false;
  int xform_R = 0;

  template <typename P>
  int launch_xform(P& pl, bool forward, const float* x, long long len, fast::v2f* spec, float* frames, float scale,
                   int pad_mode = -1) {
    fast::FastXformArgs a{};
    a.x = x;
    a.spec = spec;
    a.frames = frames;
    a.window = pl.window.template as<float>();
    a.len = len;
    a.n_frames_total = (long long)pl.B() * pl.Tn();
    a.T = pl.Tn();
    a.hop = pl.cfg.hop_length;
    a.pad = pl.pad;
    a.pad_mode = pad_mode >= 0 ? pad_mode : pl.cfg.pad_mode;
    a.scale = scale;
    size_t lds = 0;
    const void* fn = nullptr;
    SPECINV_R_SWITCH(xform_R, lds = fast::Geo<RR>::lds_bytes(4);
                     fn = forward ? (const void*)fast::k_fast_stft<RR> : (const void*)fast::k_fast_inverse_frames<RR>);
    const unsigned grid = (unsigned)std::min<long long>((a.n_frames_total + 3) / 4, 256 * 12);
    SI_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    void* kargs[] = {&a};
    SI_HIP(hipLaunchKernel(fn, dim3(grid), dim3(256), kargs, lds, pl.stream));
    return SPECINV_OK;
  }

  // Adjoint of the analysis (gradient frames -> overlap-add over the padded signal) in one launch for big batches of
  // frames; `*used` stays false when the shape is not covered (the caller then runs inverse frames + gather).
  // `margins` receives the pad samples on either side of the signal.
  template <typename P>
  int launch_inverse_ola(P& pl, const fast::v2f* spec, float* out, long long len, float scale, float** margins, bool* used) {
    *used = false;
    if (!xform_ok || xform_R > 16 || pl.force_generic || knobs.disable_hop) return SPECINV_OK;
    const int N = pl.N(), hop = pl.cfg.hop_length, T = pl.Tn(), B = pl.B();
    const long long from = knobs.frames_from(xform_R >= 16 ? 16384 : 32768);
    if ((long long)B * T < from || hop < 1 || hop > N || pl.pad >= len) return SPECINV_OK;
    // the kernel writes every sample of `out` only if the frames cover the padded signal exactly
    if ((long long)(T - 1) * hop + N != len + 2LL * pl.pad) return SPECINV_OK;
    const int floor_ch = std::max(8, (N - 1) / hop + 1);
    const int nch = (int)std::max(1LL, std::min<long long>(T / floor_ch, std::max(1, 2048 / B)));
    const int wgw = 8, keep = N - hop, n_w = B * nch;
    SI_TRY(hop_inv_tail.reserve((size_t)B * nch * keep * sizeof(float) + 16));
    SI_TRY(hop_inv_margins.reserve((size_t)B * 2 * std::max(1, pl.pad) * sizeof(float)));
    fast::HopInvArgs a{};
    a.spec = spec;
    a.out = out;
    a.margins = hop_inv_margins.template as<float>();
    a.xtail = hop_inv_tail.template as<float>();
    a.window = pl.window.template as<float>();
    a.len = len;
    a.T = T;
    a.nchunks = nch;
    a.n_waves = n_w;
    a.hop = hop;
    a.pad = pl.pad;
    a.scale = scale;
    size_t lds = 0;
    const void* fn = nullptr;
    SPECINV_R_SWITCH(xform_R, if constexpr (RR <= 16) {
      lds = fast::Geo<RR>::lds_bytes(wgw) + (size_t)wgw * fast::Geo<RR>::N * sizeof(float);
      fn = (const void*)fast::k_hop_inverse<RR>;
    });
    SI_CHECK(fn != nullptr, SPECINV_EUNSUPPORTED, "no k_hop_inverse instantiation");
    SI_TRY(launch_waves(pl, fn, a, n_w, wgw, lds));
    if (nch > 1 && keep > 0) {
      const long long total = (long long)B * (nch - 1) * keep;
      hipLaunchKernelGGL(fast::k_hop_tails_raw, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, pl.stream, out,
                         (const float*)a.xtail, T, nch, hop, keep, pl.pad, len, total);
      SI_HIP(hipGetLastError());
    }
    *margins = a.margins;
    *used = true;
    return SPECINV_OK;
  }
  DevBuf hop_inv_tail, hop_inv_margins;

  // waves per workgroup of the fused iteration kernel: k_fused4 takes 8-wave workgroups (one per CU) once every wave
  // slot is filled; fewer waves than slots: smaller workgroups reach more CUs
  int fused_wgw() const {
    if (R == 8 && OV == 4 && !knobs.fused_template) {
      // three waves per SIMD: a 12-wave workgroup is a whole CU, and 8-wave workgroups do not pair up there (2 + 2 waves on a SIMD
      // that holds 3: at 2048 ... 3071 waves every CU's second workgroup waited for the first - round 5's sweep, B 64 x T 300:
      // 316 M against 400 M at B 48).  Below a full chip, 4-wave workgroups: three fit a CU.
      return n_waves >= 3072 ? 12 : 4;
    }
    // (the signal-form kernel at n_fft 2048 measured 2 % faster with two 4-wave workgroups per CU than with one 8-wave one:
    // C2 25.8 vs 26.3 ms per step on one box, three runs each - the opposite of k_fused4)
    // ... except when the chunks are skewed (begin_t): one 8-wave workgroup per CU makes the hardware slot of a wave its index in
    // the workgroup / 4, whatever else runs on the chip - the 4-wave form has to infer it from the dispatch order (measured with
    // the skew: 19.89-20.09 against 20.02-20.16 ms per C2 step, tools/log/EXPERIMENTS.md r03 wgw8)
    if (td && R == 16 && OV == 4) return (skew != 0 && skew < 0x10000) ? 8 : 4;
    if ((R == 8 || R == 16) && OV == 4 && !knobs.fused_template) return n_waves >= 2048 ? fast::kFused4Waves : 4;
    return 4;
  }
  // {waves per workgroup, chunks per item, waves, kernel (FastKernel)}
  void geometry(int out[4]) const {
    if (semi) {
      out[0] = hopk ? 8 : 4;
      out[3] = hopk ? (td ? kKernelHopTd : kKernelHop) : kKernelSemi;
    } else {
      const bool tuned = (R == 8 || R == 16) && OV == 4 && !knobs.fused_template;
      out[0] = fused_wgw();
      out[3] = tuned ? (td ? kKernelFused4Td : kKernelFused4) : (td ? kKernelFusedTd : kKernelFused);
    }
    out[1] = nchunks;
    out[2] = n_waves;
  }

  template <int RR, int MODE, bool EVAL, typename P>
  int launch(P& pl, const fast::FastArgs& a) {
    const void* fn = nullptr;
    if constexpr (RR % 8 == 0) {
      if (OV == 8) fn = (const void*)fast::k_fused<RR, 8, MODE, EVAL>;
    }
    if constexpr (RR == 8 || RR == 16) {
      if (OV == 4)                                                       // the tuned copy for the headline shapes
        fn = knobs.fused_template ? (const void*)fast::k_fused<RR, 4, MODE, EVAL> : (const void*)fast::k_fused4<RR, MODE, EVAL>;
    } else {
      if (OV == 4) fn = (const void*)fast::k_fused<RR, 4, MODE, EVAL>;
    }
    if (OV == 2) fn = (const void*)fast::k_fused<RR, 2, MODE, EVAL>;
    SI_CHECK(fn != nullptr, SPECINV_EUNSUPPORTED, "no fused kernel for n_fft / hop = %d", OV);
    const int wgw = fused_wgw();
    return launch_waves(pl, fn, a, n_waves, wgw, fast::Geo<RR>::lds_bytes(wgw));
  }

  template <typename P>
  int launch_td(P& pl, const fast::FastArgs& a, bool early, bool ev) {
    const void* fn = nullptr;
    size_t lds_used = 0;
    const int wgw = fused_wgw();
    SPECINV_R_SWITCH(R, if constexpr (RR <= 16) {                      // (n_fft 4096 never takes the signal form: begin_t)
                       lds_used = fast::Geo<RR>::lds_bytes_td(wgw);
                       if constexpr (RR % 8 == 0) { if (OV == 8) fn = SPECINV_EARLY_EVAL(early, ev, fast::k_fused_td, RR, 8); }
                       if constexpr (RR == 8 || RR == 16) { if (OV == 4) fn = SPECINV_EARLY_EVAL(early, ev, fast::k_fused4_td, RR); }
                       else { if (OV == 4) fn = SPECINV_EARLY_EVAL(early, ev, fast::k_fused_td, RR, 4); }
                       if (OV == 2) fn = SPECINV_EARLY_EVAL(early, ev, fast::k_fused_td, RR, 2);
                     });
    SI_CHECK(fn != nullptr, SPECINV_EUNSUPPORTED, "no fused kernel for n_fft / hop = %d", OV);
    return launch_waves(pl, fn, a, n_waves, wgw, lds_used);
  }

  template <int RR, int MODE, bool EVAL, typename P>
  int launch_semi(P& pl, bool last = false) {
    using G = fast::Geo<RR>;
    fast::SemiArgs s{};
    fast::FastArgs& a = s.f;
    a = base_args(pl);
    a.x_in = xb[0].template as<float>();
    a.P_out = Pb.template as<v4f>();
    a.Pmid_out = Pmid.template as<v2f>();
    if (MODE == fast::MODE_ADMM) SI_TRY(want_xu(pl, a, last));
    s.frames = pl.frames.template as<float>();
    s.n_frames_total = (long long)pl.B() * pl.Tn();
    s.hop = pl.cfg.hop_length;
    s.pad = pl.pad;
    const size_t lds = G::lds_bytes(4);
    const void* fn = two ? (const void*)fast::k_semi2<RR, MODE, EVAL> : (const void*)fast::k_semi<RR, MODE, EVAL>;
    SI_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    void* kargs[] = {&s};
    SI_HIP(hipLaunchKernel(fn, dim3(semi_grid), dim3(256), kargs, lds, pl.stream));
    return pl.launch_ola(pl.frames.template as<float>(), xb[0].template as<float>(), true);
  }

  // one iteration (or the initial ISTFT) of k_hop: reads x from xb[cur], writes xb[cur ^ 1], then mends the chunk seams
  template <int RR, int MODE, bool EVAL, typename P>
  int launch_hop(P& pl, bool last = false) {
    using G = fast::Geo<RR>;
    const int wgw = 8, hop = pl.cfg.hop_length, keep = pl.N() - hop;
    const int nx = MODE == fast::MODE_INIT ? 0 : (cur ^ 1);
    fast::HopArgs s{};
    fast::FastArgs& a = s.f;
    a = base_args(pl);
    a.x_in = xb[cur].template as<float>();
    a.x_out = xb[nx].template as<float>();
    a.P_out = Pb.template as<v4f>();
    a.Pmid_out = Pmid.template as<v2f>();
    if (MODE == fast::MODE_ADMM) SI_TRY(want_xu(pl, a, last));
    s.env = a.env;
    s.xtail = xtail[0].template as<float>();
    s.hop = hop;
    s.pad = pl.pad;
    const void* fn = two ? (const void*)fast::k_hop2<RR, MODE, EVAL> : (const void*)fast::k_hop<RR, MODE, EVAL>;
    SI_TRY(launch_waves(pl, fn, s, n_waves, wgw, G::lds_bytes(wgw) + (size_t)wgw * G::N * sizeof(float)));
    if (nchunks > 1 && keep > 0) {
      const long long total = (long long)pl.B() * (nchunks - 1) * keep;
      hipLaunchKernelGGL(fast::k_hop_tails, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, pl.stream, a.x_out,
                         (const float*)s.xtail, s.env, pl.Tn(), nchunks, hop, keep, pl.pad, (long long)pl.length, total);
      SI_HIP(hipGetLastError());
    }
    cur = nx;
    return SPECINV_OK;
  }

  // the same for Griffin-Lim with the momentum carried as a signal: z from zb[cur] (the first closure call: x itself) to
  // zb[cur ^ 1], x to xb[cur ^ 1]
  template <int RR, typename P>
  int launch_hop_td(P& pl, bool ev, bool need_x) {
    using G = fast::Geo<RR>;
    const int wgw = 8, hop = pl.cfg.hop_length, keep = pl.N() - hop;
    const int nx = cur ^ 1;
    ++td_t;
    const double tds = std::pow(-(double)pl.coef, (double)td_t);
    const bool early = std::fabs(tds) >= fast::kTdsFloor;
    fast::HopArgs s{};
    fast::FastArgs& a = s.f;
    a = base_args(pl);
    a.x_in = td_t == 1 ? xb[cur].template as<float>() : zb[cur].template as<float>();
    a.x_out = zb[nx].template as<float>();
    a.x2_in = xb[cur].template as<float>();
    a.x2_out = xb[nx].template as<float>();
    a.P_in = Pb.template as<v4f>();
    a.Pmid_in = Pmid.template as<v2f>();
    a.tds = (float)tds;
    s.env = a.env;
    s.xtail = xtail[0].template as<float>();
    s.hop = hop;
    s.pad = pl.pad;
    s.write_x = need_x ? 1 : 0;
    const void* fn = SPECINV_EARLY_EVAL(early, ev, fast::k_hop_td, RR);
    SI_TRY(launch_waves(pl, fn, s, n_waves, wgw, G::lds_bytes(wgw) + (size_t)wgw * G::N * sizeof(float)));
    if (nchunks > 1 && keep > 0) {
      const long long total = (long long)pl.B() * (nchunks - 1) * keep;
      hipLaunchKernelGGL(fast::k_hop_tails_td, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, pl.stream, a.x2_out, a.x_out,
                         a.x_in, (const float*)s.xtail, s.env, a.coef, pl.Tn(), nchunks, hop, keep, pl.pad, (long long)pl.length,
                         total);
      SI_HIP(hipGetLastError());
    }
    cur = nx;
    return SPECINV_OK;
  }

  // the most pairs of partial sums an evaluating launch of this plan leaves (n_partials after it): what a slab of a run with
  // deferred read-back holds
  int max_partials() const { return semi ? n_waves : n_waves * fast::kEvalPieces; }

  template <typename P>
  int iterate_semi(P& pl, int n_iter, bool eval_last) {
    SI_TRY(pl.partials.reserve(std::max<size_t>((size_t)n_waves * 2, 3 * 1024) * sizeof(double)));
    for (int i = 0; i < n_iter; ++i) {
      const bool last = i == n_iter - 1, ev = eval_last && last;
      int rc = SPECINV_OK;
      if (hopk) {
        SPECINV_R_SWITCH(R, if constexpr (RR <= 16) {
          if (td) rc = launch_hop_td<RR>(pl, ev, last || (eval_last && i == n_iter - 2));
          else if (mode == fast::MODE_GLA) rc = ev ? launch_hop<RR, fast::MODE_GLA, true>(pl) : launch_hop<RR, fast::MODE_GLA, false>(pl);
          else rc = ev ? launch_hop<RR, fast::MODE_ADMM, true>(pl, last) : launch_hop<RR, fast::MODE_ADMM, false>(pl, last);
        });
        SI_TRY(rc);
        continue;
      }
      SPECINV_R_SWITCH(R, if (mode == fast::MODE_GLA) rc = ev ? launch_semi<RR, fast::MODE_GLA, true>(pl)
                                                               : launch_semi<RR, fast::MODE_GLA, false>(pl);
                       else rc = ev ? launch_semi<RR, fast::MODE_ADMM, true>(pl, last) : launch_semi<RR, fast::MODE_ADMM, false>(pl, last));
      SI_TRY(rc);
    }
    n_partials = n_waves;
    return SPECINV_OK;
  }

  template <typename P>
  int iterate(P& pl, int n_iter, bool eval_last) {
    if (semi) return iterate_semi(pl, n_iter, eval_last);
    SI_TRY(pl.partials.reserve(std::max<size_t>((size_t)n_waves * 2 * fast::kEvalPieces, 3 * 1024) * sizeof(double)));
    int eval_pieces = 1;
    for (int i = 0; i < n_iter; ++i) {
      const bool last = i == n_iter - 1, ev = eval_last && last;
      const int nx = cur ^ 1;
      fast::FastArgs a = base_args(pl);
      a.x_in = xb[cur].template as<float>();
      a.x_out = xb[nx].template as<float>();
      a.xtail_in = xtail[cur].template as<float>();
      a.xtail_out = xtail[nx].template as<float>();
      a.P_in = Pb.template as<v4f>();          // (the signal form: the starting spectrum c0)
      a.P_out = Pb.template as<v4f>();
      a.Pmid_in = Pmid.template as<v2f>();
      a.Pmid_out = Pmid.template as<v2f>();
      SI_TRY(want_xu(pl, a, last));
      if (td) {
        ++td_t;
        const double tds = std::pow(-(double)pl.coef, (double)td_t);
        const bool early = std::fabs(tds) >= fast::kTdsFloor;
        a.x_in = td_t == 1 ? xb[cur].template as<float>() : zb[cur].template as<float>();
        a.x_out = zb[nx].template as<float>();
        a.x2_in = xb[cur].template as<float>();
        // x_{t+1} has a reader only after the last iteration of a call (get_wave, the next call) and before an evaluating launch
        const bool need_x = last || (eval_last && i == n_iter - 2);
        a.x2_out = need_x ? xb[nx].template as<float>() : nullptr;
        a.tds = (float)tds;
        // an evaluating iteration on the headline shapes: the plain kernel, then the evaluation of x_t as a kernel of its own
        // (kernels_fast_td.h: k_eval_td; SPECINV_EVAL_KERNEL=0: the fused evaluating variant)
        if (ev && knobs.eval_kernel && OV == 4 && (R == 8 || R == 16)) {
          SI_TRY(launch_td(pl, a, early, false));
          const void* fn = R == 16 ? (const void*)fast::k_eval_td<16, 4> : (const void*)fast::k_eval_td<8, 4>;
          const size_t lds_used = R == 16 ? fast::Geo<16>::lds_bytes(4) : fast::Geo<8>::lds_bytes(4);
          SI_TRY(launch_waves(pl, fn, a, n_waves * fast::kEvalPieces, 4, lds_used));
          eval_pieces = fast::kEvalPieces;
        } else {
          SI_TRY(launch_td(pl, a, early, ev));
        }
        cur = nx;
        continue;
      }
      int rc = SPECINV_OK;
      SPECINV_R_SWITCH(R, if (mode == fast::MODE_GLA) rc = ev ? launch<RR, fast::MODE_GLA, true>(pl, a)
                                                               : launch<RR, fast::MODE_GLA, false>(pl, a);
                       else rc = ev ? launch<RR, fast::MODE_ADMM, true>(pl, a) : launch<RR, fast::MODE_ADMM, false>(pl, a));
      SI_TRY(rc);
      cur = nx;
    }
    n_partials = n_waves * eval_pieces;
    return SPECINV_OK;
  }

  template <typename P>
  int get_wave(P& pl, float* out) {
    if (semi || nchunks <= 1) {      // the rows are whole
      SI_HIP(hipMemcpyAsync(out, xb[cur].p, (size_t)pl.B() * pl.length * sizeof(float), hipMemcpyDeviceToDevice, pl.stream));
      return SPECINV_OK;
    }
    // the rows and the chunk tails beside them, added on the way out (k_wave_out)
    const bool wide = pl.length % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    const void* fn = nullptr;
    SPECINV_R_SWITCH(R, if constexpr (RR % 8 == 0) {
                       if (OV == 8) fn = wide ? (const void*)fast::k_wave_out<RR, 8, v4f> : (const void*)fast::k_wave_out<RR, 8, float>;
                     }
                     if (OV == 4) fn = wide ? (const void*)fast::k_wave_out<RR, 4, v4f> : (const void*)fast::k_wave_out<RR, 4, float>;
                     if (OV == 2) fn = wide ? (const void*)fast::k_wave_out<RR, 2, v4f> : (const void*)fast::k_wave_out<RR, 2, float>);
    SI_CHECK(fn != nullptr, SPECINV_EUNSUPPORTED, "no fused kernel for n_fft / hop = %d", OV);
    float* xo = out;
    const float* xi = xb[cur].template as<float>();
    const float* tl = xtail[cur].template as<float>();
    int Tn = pl.Tn(), nc = nchunks, sk = skew;
    long long Ln = (long long)pl.length;
    int nblk = (int)ceil_div(Ln, (long long)pl.cfg.hop_length);
    long long tot = (long long)pl.B() * nblk;
    void* kargs[] = {&xo, &xi, &tl, &Tn, &nc, &Ln, &nblk, &tot, &sk};
    SI_HIP(hipLaunchKernel(fn, dim3((unsigned)ceil_div(tot, 4LL * fast::kWaveOutBlocks)), dim3(256), kargs, 0, pl.stream));
    return SPECINV_OK;
  }

  template <typename P>
  int get_state_spec(P& pl, int which, cplx<float>* out) {
    const long long nf = (long long)pl.B() * pl.Tn();
    SI_TRY(scratch.reserve((size_t)nf * pl.n_freq * sizeof(v2f)));
    const bool admm = mode == fast::MODE_ADMM;
    SI_CHECK(admm || !td || td_t == 0, SPECINV_ESTATE,
             "Griffin-Lim carries its momentum as a signal on this path (pre_spec is never formed); call "
             "specinv_plan_keep_state(plan, 1) before specinv_gla_init to iterate on pre_spec itself");
    SI_CHECK(!admm || which == 2 || xu_valid, SPECINV_ESTATE,
             "ADMM carries Y = X + U; call specinv_plan_keep_state(plan, 1) before iterating to read X and U (which = 2 reads Y)");
    const DevBuf& src = (!admm || which == 2) ? Pb : which == 0 ? Xb : Ub;
    const DevBuf& mid = (!admm || which == 2) ? Pmid : which == 0 ? Xmid : Umid;
    SI_CHECK(!two || !admm || which == 2, SPECINV_EUNSUPPORTED, "X and U of a two-sided ADMM run are not kept on this path");
    SPECINV_R_SWITCH(R, const long long np = nf * fast::Geo<RR>::H * 64;
                     hipLaunchKernelGGL((fast::k_pairs_to_spec<RR>), dim3((unsigned)ceil_div(np, 256)), dim3(256), 0, pl.stream,
                                        src.template as<v4f>(), mid.template as<v2f>(), scratch.template as<v2f>(), nf, pl.n_freq, 0);
                     if (two) hipLaunchKernelGGL((fast::k_pairs_to_spec<RR>), dim3((unsigned)ceil_div(np, 256)), dim3(256), 0,
                                                 pl.stream, Pb2.template as<v4f>(), Pmid2.template as<v2f>(),
                                                 scratch.template as<v2f>(), nf, pl.n_freq, 1));
    SI_HIP(hipGetLastError());
    return pl.template transpose<cplx<float>>(scratch.template as<cplx<float>>(), out, pl.Tn(), pl.n_freq);
  }
};

}  // namespace specinv
