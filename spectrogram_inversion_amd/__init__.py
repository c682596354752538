"""spectrogram_inversion_amd - MI355X-native spectrogram inversion.

Drop-in for the public surface of `torch_specinv` v0.2.1
(torch_specinv/__init__.py:6: L_BFGS, RTISI_LA, griffin_lim, ADMM, phase_init; plus
torch_specinv.metrics: sc, snr, ser), implemented as HIP kernels for gfx950 behind the C ABI
of include/specinv.h.  Importing the package does not load the HIP library; the first call
does, and fails loudly if it is missing (no CPU fallback).

    import spectrogram_inversion_amd as torch_specinv
    y = torch_specinv.griffin_lim(mag, max_iter=100, alpha=0.3, hop_length=512, window=w)
"""
name = "spectrogram_inversion_amd"
__version__ = "0.1.0"

from .methods import L_BFGS, RTISI_LA, griffin_lim, ADMM, phase_init   # noqa: E402,F401
from . import metrics                                                   # noqa: E402,F401
from .metrics import sc, snr, ser                                       # noqa: E402,F401
from .transforms import MagSTFT, LogMelSTFT                             # noqa: E402,F401
from .streaming import RTISIStream                                      # noqa: E402,F401
from .mel import mel_filterbank                                         # noqa: E402,F401
from .mel_inverse import mel_to_stft, mel_to_audio, mel_to_stft_unfolded, mel_to_audio_unfolded   # noqa: E402,F401
from .misi import misi, misi_unfolded                                   # noqa: E402,F401
from .agla import accelerated_griffin_lim, agla_unfolded                # noqa: E402,F401
from .constrained import constrained_griffin_lim, constrained_unfolded  # noqa: E402,F401
from .projection import gla_projection, stft, istft                     # noqa: E402,F401
from .timescale import phase_vocoder, time_stretch, stretched_frames, pitch_shift   # noqa: E402,F401
from .resample import resample                                          # noqa: E402,F401
from .hpss import hpss, hpss_medians, hpss_audio, harmonic, percussive   # noqa: E402,F401
from .envelope import spectral_envelope, impose_envelope, default_envelope_order, envelope_order_for_f0   # noqa: E402,F401
from .pitch import pyin, pyin_bins, pyin_decode, pyin_observations, yin, yin_cmnd, yin_frames   # noqa: E402,F401
from .tsm import wsola, ola, time_stretch_hpss                          # noqa: E402,F401
from .pghi import rtpghi                                                # noqa: E402,F401
from .wiener import consistent_wiener, consistent_wiener_audio          # noqa: E402,F401
from .enhance import noise_psd, spectral_gain, denoise                  # noqa: E402,F401
from .dereverb import wpe, wpe_apply, dereverb                          # noqa: E402,F401
from .beamform import spatial_covariance, beamform, beamform_apply, beamform_audio   # noqa: E402,F401
from .plan import set_exact_projection, has_approx                      # noqa: E402,F401
