// What k_mel_nnls (tu_mel_nnls.hip) and its adjoint (tu_mel_nnls_adjoint.hip) share on the host: the plan's mel state, the
// momentum table and the LDS layout rule.
#pragma once
#include <algorithm>
#include <cmath>
#include <mutex>
#include <vector>

#include "dev_buf.h"
#include "plan.h"

namespace specinv {

struct MelNnlsState {
  int n_mels = 0, nseg = 0, nwr = 0, nwc = 0, piece = 0;
  double lipschitz = 0;
  DevBuf wr, wc, seg, rowseg, col, beta;
  int n_beta = 0;
  long long stage_bytes = 0;   // the band form's bytes in LDS
};

namespace mel_nnls {

constexpr int kLdsBytes = 160 * 1024;

inline int upload(DevBuf& d, const void* src, size_t n, hipStream_t stream) {
  SI_TRY(d.reserve(n));
  if (n) SI_HIP(hipMemcpyAsync(d.p, src, n, hipMemcpyHostToDevice, stream));
  return SPECINV_OK;
}

// momentum table: beta_k = (t_k - 1) / t_{k+1}, t_0 = 1, t_{k+1} = (1 + sqrt(1 + 4 t_k^2)) / 2 - grown, never recomputed: a run of
// n iterations reads the first n entries whatever the longest run so far
inline int ensure_beta(PlanBase& pl, MelNnlsState& st, int n_iter) {
  if (n_iter <= st.n_beta) return SPECINV_OK;
  const int n = std::max(n_iter, 128);
  std::vector<double> beta(n);
  double t = 1.0;
  for (int k = 0; k < n; ++k) {
    const double tn = (1.0 + std::sqrt(1.0 + 4.0 * t * t)) / 2.0;
    beta[k] = (t - 1.0) / tn;
    t = tn;
  }
  DevBuf fresh;
  SI_TRY(upload(fresh, beta.data(), beta.size() * sizeof(double), pl.stream));
  SI_HIP(hipStreamSynchronize(pl.stream));
  std::swap(st.beta.p, fresh.p);
  std::swap(st.beta.bytes, fresh.bytes);
  st.n_beta = n;
  return SPECINV_OK;
}

struct Pick {
  bool staged = false;
  int waves = 0, per_wave = 0, lds = 0;
  int slice_bytes = 0;         // a wave's slice: per_wave elements, then `extra` bytes at the next multiple of 8
};

// the layout that puts the most waves on a CU by LDS (at most 32): the band form staged beside the slices or read from global
// memory (L1 / L2), one to eight waves per workgroup; on a tie the staged form, then four waves (the finer grain of the two that
// fill a CU).  `extra` >= 0: bytes a wave keeps after its elements, 8-byte aligned (the adjoint's mask words).
template <typename T>
Pick pick_layout(const MelNnlsState& st, int F, long long extra = -1) {
  Pick p;
  p.per_wave = 2 * F + 2 * st.n_mels + st.nseg;
  long long slice = (long long)p.per_wave * sizeof(T);
  if (extra >= 0) slice = ((slice + 7) & ~7LL) + extra;
  int best = 0;
  for (bool staged : {true, false})
    for (int w : {4, 8, 2, 1}) {
      const long long lds = (staged ? st.stage_bytes : 0) + w * slice;
      if (lds > kLdsBytes) continue;
      const int waves_cu = (int)std::min<long long>(32, w * (kLdsBytes / lds));
      if (waves_cu > best) {
        best = waves_cu;
        p.staged = staged;
        p.waves = w;
        p.lds = (int)lds;
        p.slice_bytes = (int)slice;
      }
    }
  return p;
}

inline int cu_count() {
  static int n_cu = 0;
  static std::once_flag once;
  std::call_once(once, [] {
    int dev = 0;
    hipDeviceProp_t prop{};
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) n_cu = prop.multiProcessorCount;
    if (n_cu <= 0) n_cu = 256;
  });
  return n_cu;
}

// the band form, the momentum table and the shape into a kernel's arguments (MelNnlsArgs)
template <typename T, typename A>
void fill_args(A& a, const MelNnlsState& st, const PlanBase& pl, const Pick& pk, int n_iter, double power) {
  a.beta = static_cast<const double*>(st.beta.p);
  a.wr = static_cast<const T*>(st.wr.p);
  a.wc = static_cast<const T*>(st.wc.p);
  a.seg = static_cast<const int4*>(st.seg.p);
  a.rowseg = static_cast<const int*>(st.rowseg.p);
  a.col = static_cast<const int2*>(st.col.p);
  a.F = pl.n_freq;
  a.n_mels = st.n_mels;
  a.nseg = st.nseg;
  a.nwr = st.nwr;
  a.nwc = st.nwc;
  a.frames = pl.cfg.n_frames;
  a.tgroups = (pl.cfg.n_frames + pk.waves - 1) / pk.waves;
  a.n_groups = a.tgroups * pl.cfg.batch;
  a.n_iter = n_iter;
  a.per_wave = pk.per_wave;
  a.stage_bytes = pk.staged ? (int)st.stage_bytes : 0;
  a.step = (T)(1.0 / st.lipschitz);
  a.root = power == 1.0 ? 1 : power == 2.0 ? 2 : 0;
  a.inv_power = (T)(1.0 / power);
}

// one workgroup per group of frames while the chip has room; past that every workgroup walks groups (the band form staged once)
inline int grid_size(const Pick& pk, int n_groups) {
  const int per_cu = std::max(1, std::min(kLdsBytes / pk.lds, 32 / pk.waves));
  return std::max(1, std::min(n_groups, cu_count() * per_cu));
}

}  // namespace mel_nnls
}  // namespace specinv
