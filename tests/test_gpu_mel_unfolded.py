"""`mel_to_stft_unfolded` / `mel_to_audio_unfolded` on the device: the forward against `mel_to_stft` (bits) and the torch restatement
of the mel oracle (tests/_mel_torch.py), the gradient of k_mel_nnls_adjoint against autograd on that restatement, and the layer's
properties.  Needs an MI355X: `-m gpu`."""
import ctypes as C

import numpy as np
import pytest
import torch

import _mel_torch as mt
from _util import rel_l2

pytestmark = pytest.mark.gpu

import spectrogram_inversion_amd as si                                    # noqa: E402
from spectrogram_inversion_amd import _lib                                # noqa: E402
from spectrogram_inversion_amd.mel import mel_filterbank                  # noqa: E402
from spectrogram_inversion_amd.plan import Plan, args_helper, get_plan    # noqa: E402

DEV = torch.device("cuda", 0)
TDT = {np.float32: torch.float32, np.float64: torch.float64}
F32_FLOOR = 1e-4                # tests/test_gpu_mel.py's float32 TOL
F64_GATE = 1e-10                # the project's float64 gate


def N(t):
    return t.detach().cpu().numpy()


def T_(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(mt.BANKS))
def test_output_and_gradient_match_the_restatement(name, dtype):
    """Every power and n_iter of the case table.  float64: 1e-10.  float32: against the float64 restatement on the same float32
    inputs, the larger of 1e-4 and 6 x the restatement's own float32-against-float64 rel-L2 on the case (tests/test_gpu_agla.py's
    rule; tests/test_mel_unfolded_host.py keeps the gradient's at or below 1e-3)."""
    for power in mt.POWERS:
        M, mel, w = mt.inputs(name, power, dtype)
        T = mel.shape[2]
        for n_iter in mt.N_ITERS:
            case = (name, power, n_iter)
            y = T_(mel).requires_grad_(True)
            out = si.mel_to_stft_unfolded(y, torch.from_numpy(M), power=power, n_iter=n_iter)
            assert out.requires_grad and out.shape == w.shape and out.dtype == TDT[dtype] and out.device == DEV
            plain = si.mel_to_stft(y.detach(), M, power=power, n_iter=n_iter)
            assert torch.equal(out.detach(), plain), "under grad the forward output is mel_to_stft's, bit for bit"
            with torch.no_grad():
                assert torch.equal(si.mel_to_stft_unfolded(y, M, power=power, n_iter=n_iter), plain)
            quiet = si.mel_to_stft_unfolded(y.detach(), M, power=power, n_iter=n_iter)
            assert not quiet.requires_grad and torch.equal(quiet, plain)
            (out * T_(w)).sum().backward()
            g = N(y.grad)
            assert g.shape == mel.shape and y.grad.dtype == TDT[dtype] and np.all(np.isfinite(g))
            assert not g[:, :, mt.SILENT(T)].any(), "a silent frame's gradient column is exactly zero"
            if name == "zero_row_col40x257":
                assert not g[:, 5].any(), "the row of a band that touches no bin is exactly zero"
            ref = mt.reference(case, dtype, np.float64)
            if n_iter == 0:
                assert not g.any() and not N(out).any()
                continue
            gates = [F64_GATE, F64_GATE]
            if dtype == np.float32:
                own = [rel_l2(a, b) for a, b in zip(mt.reference(case, dtype), ref)]
                assert own[1] <= 1e-3, own
                gates = [max(F32_FLOOR, 6 * o) for o in own]
            e_out, e_grad = rel_l2(N(out), ref[0]), rel_l2(g, ref[1])
            print(f"{case} {np.dtype(dtype).name}: out {e_out:.3e} (gate {gates[0]:.1e}) grad {e_grad:.3e} (gate {gates[1]:.1e})")
            assert e_out <= gates[0] and e_grad <= gates[1], (case, e_out, e_grad, gates)


def test_shapes_devices_and_narrow_dtypes():
    M, mel, w = mt.inputs("nonorm40x257", 1.0, np.float32)
    ref = N(_grad(T_(mel), M, T_(w)))
    # 2-D
    y2 = T_(mel[1]).requires_grad_(True)
    out2 = si.mel_to_stft_unfolded(y2, M, n_iter=7)
    assert out2.shape == w.shape[1:]
    (out2 * T_(w[1])).sum().backward()
    assert y2.grad.shape == y2.shape and np.array_equal(N(y2.grad), ref[1]), "a frame's gradient does not depend on its batch"
    # CPU in: CPU out, the gradient on the CPU
    yc = torch.from_numpy(mel).requires_grad_(True)
    outc = si.mel_to_stft_unfolded(yc, M, n_iter=7)
    assert outc.device.type == "cpu"
    (outc * torch.from_numpy(w)).sum().backward()
    assert yc.grad.device.type == "cpu" and yc.grad.shape == yc.shape and np.array_equal(yc.grad.numpy(), ref)
    # bfloat16 / float16: computed in float32, the gradient in the input's dtype
    for half in (torch.bfloat16, torch.float16):
        yh = T_(mel).to(half).requires_grad_(True)
        outh = si.mel_to_stft_unfolded(yh, M, n_iter=7)
        assert outh.dtype == half and torch.equal(outh.detach(), si.mel_to_stft(yh.detach(), M, n_iter=7))
        (outh.float() * T_(w)).sum().backward()
        assert yh.grad.dtype == half and yh.grad.shape == yh.shape and yh.grad.device == DEV
        assert torch.isfinite(yh.grad).all() and yh.grad.abs().max() > 0
    # no items: zeros, zero gradient
    for shape in ((0, 40, 5), (2, 40, 0)):
        y0 = torch.zeros(shape, device=DEV, requires_grad=True)
        out0 = si.mel_to_stft_unfolded(y0, M, n_iter=7)
        assert out0.shape == (shape[0], 257, shape[2]) and out0.requires_grad
        out0.sum().backward()
        assert y0.grad.shape == shape and not y0.grad.any()


def _grad(mel, M, w, n_iter=7, **kw):
    y = mel.clone().requires_grad_(True)
    (si.mel_to_stft_unfolded(y, M, n_iter=n_iter, **kw) * w).sum().backward()
    return y.grad


def test_adjoint_before_setup_is_einval():
    plan = Plan(args_helper(torch.empty(1, 257, 1)), 1, 4, torch.float32, DEV)
    y = torch.zeros(1, 40, 4, device=DEV)
    g = torch.zeros(1, 257, 4, device=DEV)
    assert plan.lib.specinv_mel_nnls_adjoint(plan._h, y.data_ptr(), 10, 1.0, g.data_ptr(), y.data_ptr()) == _lib.EINVAL
    assert b"setup" in plan.lib.specinv_last_error()
    most = C.c_int(-7)
    assert plan.lib.specinv_mel_nnls_adjoint_max_iter(plan._h, C.byref(most)) == _lib.EINVAL and most.value == -7
    assert b"setup" in plan.lib.specinv_last_error()


def test_too_long_an_unroll_raises_at_the_forward_call():
    """n_fft 8192 in float64: a frame's slice takes 70 KB of the 160, the mask words 65 * 8 bytes per iteration.  The longest unroll
    that fits runs; one more raises before anything is launched, and the C entry itself refuses it."""
    M = mel_filterbank(44100, 8192, 96).astype(np.float64)
    mel = T_(mt.mel_input(M, 2, 1.0, seed=3)[:1])                                  # (1, 96, 2)
    si.mel_to_stft(mel, M, n_iter=1)                                   # (the plan and its setup)
    plan = get_plan(args_helper(torch.empty(1, 4097, 1, dtype=torch.float64)), 1, 2, torch.float64, DEV)
    most = C.c_int()
    _lib.check(plan.lib.specinv_mel_nnls_adjoint_max_iter(plan._h, C.byref(most)))
    assert 100 < most.value < 300, most.value
    y = mel.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match=f"n_iter <= {most.value}"):
        si.mel_to_stft_unfolded(y, M, n_iter=most.value + 1)
    g = torch.ones(1, 4097, 2, dtype=torch.float64, device=DEV)
    gm = torch.full_like(mel, 7.0)
    assert plan.lib.specinv_mel_nnls_adjoint(plan._h, mel.data_ptr(), most.value + 1, 1.0, g.data_ptr(), gm.data_ptr()) == _lib.EUNSUPPORTED
    assert f"n_iter <= {most.value}".encode() in plan.lib.specinv_last_error()
    torch.cuda.synchronize()
    assert bool((gm == 7.0).all()), "nothing was launched"
    # the longest unroll that fits: against the NumPy sweep
    out = si.mel_to_stft_unfolded(y, M, n_iter=most.value)
    out.backward(g)
    ref = mt.sweep(M, N(mel), N(g), most.value)
    assert rel_l2(N(y.grad), ref) <= F64_GATE


def test_mel_to_audio_unfolded_is_the_two_calls_and_reaches_the_mel():
    """n_fft 128 / hop 32, 16 bands, 10 frames, 7 NNLS iterations, 3 AGLA iterations"""
    M = mel_filterbank(16000, 128, 16)
    mel = T_(mt.mel_input(M.astype(np.float64), 10, 1.0, seed=5)).float()
    kw = dict(n_fft=128, hop_length=32, window=torch.hann_window(128))
    y = mel.clone().requires_grad_(True)
    a = si.mel_to_audio_unfolded(y, M, nnls_iter=7, n_iter=3, alpha=0.5, beta=1.2, gamma=0.7, **kw)
    b = si.agla_unfolded(si.mel_to_stft_unfolded(y, M, 1.0, 7, **kw), 3, 0.5, 1.2, 0.7, **kw)
    assert a.requires_grad and a.shape == b.shape and torch.equal(a, b)
    with torch.no_grad():
        assert torch.equal(si.mel_to_audio_unfolded(y, M, nnls_iter=7, n_iter=3, **kw),
                           si.agla_unfolded(si.mel_to_stft(mel, M, n_iter=7, **kw), 3, **kw))
    loss = (a ** 2).mean()
    loss.backward()
    assert y.grad.shape == mel.shape and torch.isfinite(y.grad).all() and y.grad.abs().max() > 0


def test_a_backward_leaves_the_plan_as_it_was():
    """mel_to_stft and griffin_lim on the same plan, before and after a backward pass (with another filterbank in between, which the
    backward pass has to notice): the same bits."""
    M, mel, w = mt.inputs("nonorm40x257", 1.0, np.float32)
    other = mel_filterbank(16000, 512, 40)
    kw = dict(hop_length=128, window=torch.hann_window(512))
    y = T_(mel)
    mag0 = si.mel_to_stft(y, M, n_iter=30, **kw)
    x0 = si.griffin_lim(mag0, max_iter=5, tol=0, verbose=False, **kw)
    g0 = _grad(y, M, T_(w), **kw)
    yg = y.clone().requires_grad_(True)
    out = si.mel_to_stft_unfolded(yg, M, n_iter=7, **kw)
    si.mel_to_stft(y, other, n_iter=3, **kw)                     # the plan now holds another band form
    (out * T_(w)).sum().backward()
    assert torch.equal(yg.grad, g0)
    assert torch.equal(si.mel_to_stft(y, M, n_iter=30, **kw), mag0)
    assert torch.equal(si.griffin_lim(mag0, max_iter=5, tol=0, verbose=False, **kw), x0)
