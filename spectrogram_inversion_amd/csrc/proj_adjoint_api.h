// Host interface of the projection layer's kernels (kernels_proj_adjoint.h, compiled in tu_proj_adjoint.hip):
// the element-wise projection of gla_projection's forward pass and the fused adjoint of
//     P(x; m) = ISTFT(m S / (|S| + 1e-16)) ,  S = STFT(x)
// - both transforms of a frame, the bin arithmetic of k_misi_proj_adjoint and the inverse transform in one launch, no spectrum
// in device memory.
#pragma once
#include "kernels_generic.h"

namespace specinv {

template <typename T>
struct ProjAdjArgs {
  FrameCfg<T> c;            // the plan's frame_cfg(length): padding and forward scale are those of x's transform
  const T* x;               // (B, length): where the projection was taken
  const T* g;               // (B, length): the cotangent of y = P(x; m), not yet divided by the envelope
  const T* env;             // (length): the window-square envelope
  const T* mag;             // (B, T, F) frame-major
  T* gmag;                  // (B, T, F) frame-major out: written in full, every element by one lane
  T* frames;                // (B, T, n_fft) out: the windowed frames of A^T gR, for launch_grad_fold
  int batch;
  int max_waves;            // > 0: the launch takes at most so many waves (SPECINV_PROJ_ADJ_WAVES)
};

// one-sided n_fft 128 / 256 / 512 / 1024 / 2048 in float32 and float64
bool proj_adjoint_covers(int n_fft, int elem_size);
template <typename T>
int proj_adjoint_launch(const ProjAdjArgs<T>& a, hipStream_t stream);

// spec[i] <- spec[i] mag[i] / (|spec[i]| + 1e-16), i < n: methods.py:246-247 on the internal frame-major arrays, in place
template <typename T>
int project_launch(cplx<T>* spec, const T* mag_fm, int64_t n, hipStream_t stream);

}  // namespace specinv
