"""Every entry point on the layouts callers really pass (tests/_layouts.py): strided like `torch.stft`'s output, a step, stride 0,
an offset from a 16-byte boundary, the lazy conjugate and negative bits.

One rule for all of them.  A call with the view gives, bit for bit, what the call with the freshly made dense twin gives - same
shape, dtype and device - and leaves the buffer the view looks into as it was.  `_ingest.ingest` hands the kernels the same dense
bytes either way and the kernels are deterministic (`test_results_are_bitwise_reproducible`), so equality is exact; the one
exception, `L_BFGS`'s `init_x0` at an offset, says why where it is tested.  The dense result is computed once per entry point.
Independent anchors at the end keep the view and the twin from being wrong together.
"""
import numpy as np
import pytest
import torch

import _layouts as L
import oracle
import spectrogram_inversion_amd as si
from _hpss_oracle import masks_of, medians, times
from _pvoc_torch import max_err, pvoc_ref
from _util import hann, rel_l2
from spectrogram_inversion_amd.plan import args_helper, get_plan

pytestmark = pytest.mark.gpu

F32, F64, C64, C128 = torch.float32, torch.float64, torch.complex64, torch.complex128
CPLX = {F32: C64, F64: C128}
DEV = torch.device("cuda", 0)
B, T = 2, 12                                                       # items, frames: the smallest that still take each route

REAL3 = ("strided", "offset", "step_batch", "step_last", "expanded", "neg")
CPLX3 = ("strided", "offset", "step_batch", "step_last", "expanded", "conj", "conj_strided")
VEC = ("offset", "step_last", "neg")                               # a 1-D tensor


def _real(shape, dtype, seed, positive=True):
    g = torch.Generator().manual_seed(seed)
    z = torch.rand(shape, generator=g, dtype=F64) + 0.05 if positive else torch.randn(shape, generator=g, dtype=F64)
    return z.to(dtype).to(DEV)


def _cplx(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.view_as_complex(torch.randn(tuple(shape) + (2,), generator=g, dtype=F64))
    return z.to(CPLX.get(dtype, dtype)).to(DEV)


def _kw(n_fft, hop, dtype=F32):
    return dict(hop_length=hop, window=torch.hann_window(n_fft, dtype=dtype))


def _length(n_fft, hop, frames=T):
    return (frames - 1) * hop


def _plan(n_fft, hop, dtype, batch=B, frames=T):
    kw = _kw(n_fft, hop, dtype)
    return get_plan(args_helper(torch.empty((1, n_fft // 2 + 1, 1), dtype=dtype), **kw), batch, frames, dtype, DEV)


def _flat(out):
    return tuple(out) if isinstance(out, (tuple, list)) else (out,)


def _bits(t):
    t = t.resolve_conj().resolve_neg()
    return torch.view_as_real(t) if t.is_complex() else t


def assert_same(got, want):
    got, want = _flat(got), _flat(want)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.shape == b.shape and a.dtype == b.dtype and a.device == b.device, (a.shape, b.shape, a.dtype, b.dtype)
        assert torch.equal(_bits(a), _bits(b)), float((_bits(a).double() - _bits(b).double()).abs().max())


# ---------------------------------------------------------------------------------------------------------------------------
# the table: id -> (fn(**tensors), {argument: maker of its dense value}, {argument: builders}, route check or None)
# ---------------------------------------------------------------------------------------------------------------------------
CASES = {}


def case(cid, fn, args, views, route=None):
    CASES[cid] = (fn, args, views, route)


# griffin_lim / ADMM / accelerated_griffin_lim on the four routes
GEOM = {"fused": (512, 128, F32, "fused"), "frame": (512, 64, F32, "frame"), "wave": (256, 64, F32, "generic"),
        "f64": (256, 64, F64, "generic")}
SOLVERS = {"griffin_lim": lambda s, kw: si.griffin_lim(s, max_iter=3, tol=0, verbose=False, **kw),
           "ADMM": lambda s, kw: si.ADMM(s, max_iter=3, tol=0, verbose=False, **kw),
           "accelerated_griffin_lim": lambda s, kw: si.accelerated_griffin_lim(s, max_iter=3, tol=0, verbose=False, **kw)}


def _route(n_fft, hop, dtype, path):
    def check():
        plan = _plan(n_fft, hop, dtype)
        geo = plan.launch_geometry
        print(f"{n_fft}/{hop} {dtype}: path {plan.path}, {geo}")
        assert plan.path == path, (plan.path, geo)
        if dtype == F32 and path == "generic":
            assert geo["kernel"] == "k_wave_iter", geo
    return check


for _s, _run in SOLVERS.items():
    for _g, (_n, _h, _d, _p) in GEOM.items():
        _shape = (B, _n // 2 + 1, T)
        case(f"{_s}-{_g}-mag", lambda spec, _run=_run, _n=_n, _h=_h, _d=_d: _run(spec, _kw(_n, _h, _d)),
             {"spec": lambda _shape=_shape, _d=_d: _real(_shape, _d, 1)}, {"spec": REAL3}, _route(_n, _h, _d, _p))
        case(f"{_s}-{_g}-start", lambda spec, _run=_run, _n=_n, _h=_h, _d=_d: _run(spec, _kw(_n, _h, _d)),
             {"spec": lambda _shape=_shape, _d=_d: _cplx(_shape, _d, 2)}, {"spec": CPLX3}, _route(_n, _h, _d, _p))

MAG257 = lambda: _real((B, 257, T), F32, 3)                        # noqa: E731
MAG129 = lambda: _real((B, 129, T), F32, 4)                        # noqa: E731
SPEC129 = lambda: _cplx((B, 129, T), F32, 5)                       # noqa: E731
WAVE = lambda: _real((B, _length(256, 64)), F32, 6, positive=False)   # noqa: E731
KW = _kw(256, 64)

case("RTISI_LA", lambda spec: si.RTISI_LA(spec, look_ahead=2, max_iter=2, verbose=0, **_kw(512, 128)), {"spec": MAG257},
     {"spec": REAL3})
case("phase_init", lambda spec: si.phase_init(spec, **KW), {"spec": MAG129}, {"spec": REAL3})


def _stream(a, b):
    st = si.RTISIStream(257, batch=B, look_ahead=2, max_iter=2, max_push=8, dtype=F32, device=DEV, **_kw(512, 128))
    return torch.cat([st.push(a), st.push(b), st.flush()], 1)


case("RTISIStream.push", _stream, {"a": lambda: _real((B, 257, 5), F32, 7), "b": lambda: _real((B, 257, 7), F32, 8)},
     {"a": REAL3, "b": REAL3})

X0 = lambda: 1e-2 * _real((B, _length(256, 64)), F32, 9, positive=False)   # noqa: E731


def _lbfgs(spec, x0=None):
    tr = si.MagSTFT(256, hop_length=64, window=torch.hann_window(256))
    return si.L_BFGS(spec, tr, init_x0=X0() if x0 is None else x0, outer_max_iter=2, verbose=0, max_iter=5)


case("L_BFGS", _lbfgs, {"spec": MAG129}, {"spec": REAL3})

case("stft", lambda x: si.stft(x, n_fft=256, **KW), {"x": WAVE}, {"x": REAL3})
case("istft", lambda spec: si.istft(spec, **KW), {"spec": SPEC129}, {"spec": CPLX3})
case("gla_projection", lambda x, mag: si.gla_projection(x, mag, **KW), {"x": WAVE, "mag": MAG129}, {"x": REAL3, "mag": REAL3})
case("gla_projection-frame_major", lambda x, mag: si.gla_projection(x, mag, frame_major=True, **KW),
     {"x": WAVE, "mag": lambda: _real((B, T, 129), F32, 10)}, {"x": REAL3, "mag": REAL3})

MIX = lambda: _real((B, _length(256, 64) + 3), F32, 11, positive=False)   # noqa: E731
for _name, _fn in (("misi", lambda s, m: si.misi(s, m, max_iter=2, tol=0, verbose=False, **KW)),
                   ("misi_unfolded", lambda s, m: si.misi_unfolded(s, m, n_iter=2, **KW))):
    case(f"{_name}-mag", lambda specs, mixture, _fn=_fn: _fn(specs, mixture),
         {"specs": lambda: _real((B, 2, 129, T), F32, 12), "mixture": MIX}, {"specs": REAL3, "mixture": REAL3})
    case(f"{_name}-start", lambda specs, mixture, _fn=_fn: _fn(specs, mixture),
         {"specs": lambda: _cplx((B, 2, 129, T), F32, 13), "mixture": MIX}, {"specs": CPLX3, "mixture": ("expanded", "offset")})

ALPHA = lambda: torch.tensor([0.9, 0.5, 0.7], dtype=F64)           # noqa: E731  (a schedule, so that the layer's own path runs)
SMASK = lambda: (_real((B, 129, T), F32, 14) > 0.8)                # noqa: E731
WMASK = lambda: (_real((B, _length(256, 64)), F32, 15) > 0.8)      # noqa: E731
case("agla_unfolded-mag", lambda spec, alpha: si.agla_unfolded(spec, 3, alpha, None, 1.2, **KW), {"spec": MAG129, "alpha": ALPHA},
     {"spec": REAL3, "alpha": ("step_last",)})
case("agla_unfolded-start", lambda spec, alpha: si.agla_unfolded(spec, 3, alpha, None, 1.2, **KW), {"spec": SPEC129, "alpha": ALPHA},
     {"spec": CPLX3, "alpha": ("step_last",)})
_CG = {"spec": MAG129, "known_spec": SPEC129, "known_wave": WAVE, "wave_mask": WMASK}
_CGV = {"spec": REAL3, "known_spec": CPLX3, "known_wave": REAL3, "wave_mask": ("strided",)}
case("constrained_griffin_lim",
     lambda spec, known_spec, known_wave, wave_mask: si.constrained_griffin_lim(
         spec, known_spec, SMASK(), known_wave, wave_mask, max_iter=3, tol=0, verbose=False, **KW), _CG, _CGV)
case("constrained_griffin_lim-start",
     lambda spec, known_wave, wave_mask: si.constrained_griffin_lim(
         spec, None, None, known_wave, wave_mask, max_iter=3, tol=0, verbose=False, **KW),
     {"spec": SPEC129, "known_wave": WAVE, "wave_mask": WMASK}, {"spec": CPLX3})
case("constrained_unfolded",
     lambda spec, known_spec, known_wave, wave_mask, alpha: si.constrained_unfolded(
         spec, known_spec, SMASK(), known_wave, wave_mask, 3, alpha, None, 1.2, **KW), dict(_CG, alpha=ALPHA),
     dict(_CGV, alpha=("step_last",)))

MEL_FB = lambda: torch.from_numpy(si.mel_filterbank(8000, 256, 20)).to(DEV)   # noqa: E731
MEL = lambda: _real((B, 20, T), F32, 16)                           # noqa: E731
case("mel_to_stft", lambda mel, mel_fb: si.mel_to_stft(mel, mel_fb, n_iter=5, **KW), {"mel": MEL, "mel_fb": MEL_FB},
     {"mel": REAL3, "mel_fb": ("strided", "offset")})
case("mel_to_stft_unfolded", lambda mel, mel_fb: si.mel_to_stft_unfolded(mel, mel_fb, n_iter=5, **KW), {"mel": MEL, "mel_fb": MEL_FB},
     {"mel": REAL3, "mel_fb": ("strided",)})

for _lock in (None, "identity"):
    case(f"phase_vocoder-{_lock}", lambda spec, _lock=_lock: si.phase_vocoder(spec, 0.8, _lock, **KW), {"spec": SPEC129},
         {"spec": CPLX3})

_IT = dict(max_iter=2, tol=0, verbose=False)
case("time_stretch", lambda x: si.time_stretch(x, 0.8, n_fft=256, **_IT, **KW), {"x": WAVE}, {"x": REAL3})
case("pitch_shift", lambda x: si.pitch_shift(x, 8000, 2, n_fft=256, **_IT, **KW), {"x": WAVE}, {"x": REAL3})
case("resample", lambda x: si.resample(x, 3, 2), {"x": WAVE}, {"x": REAL3})
case("wsola", lambda x, window: si.wsola(x, 0.8, frame_length=64, window=window, return_lags=True),
     {"x": WAVE, "window": lambda: torch.hann_window(64).to(DEV)}, {"x": REAL3, "window": VEC})
case("ola", lambda x: si.ola(x, 0.8, frame_length=64), {"x": WAVE}, {"x": REAL3})
case("time_stretch_hpss", lambda x: si.time_stretch_hpss(x, 0.8, n_fft=256, kernel_size=5, perc_frame=64, **_IT, **KW),
     {"x": WAVE}, {"x": REAL3})

HS = (B, 33, 40)                                                   # (33 rows: past the 32-row tile of the median kernel)
case("hpss-real", lambda spec: si.hpss(spec, 5), {"spec": lambda: _real(HS, F32, 17)}, {"spec": REAL3})
case("hpss-complex", lambda spec: si.hpss(spec, 5), {"spec": lambda: _cplx(HS, F32, 18)}, {"spec": CPLX3})
case("hpss-complex128", lambda spec: si.hpss(spec, 5), {"spec": lambda: _cplx(HS, F64, 18)}, {"spec": CPLX3})
case("hpss_medians-real", lambda spec: si.hpss_medians(spec, 5), {"spec": lambda: _real(HS, F32, 17)}, {"spec": REAL3})
case("hpss_medians-complex", lambda spec: si.hpss_medians(spec, 5), {"spec": lambda: _cplx(HS, F32, 18)}, {"spec": CPLX3})
case("hpss_audio", lambda x: si.hpss_audio(x, 256, kernel_size=5, **KW), {"x": WAVE}, {"x": REAL3})
case("rtpghi", lambda spec: si.rtpghi(spec, **KW), {"spec": MAG129}, {"spec": REAL3})
for _m in ("sc", "snr", "ser"):
    case(_m, lambda a, b, _m=_m: getattr(si, _m)(a, b), {"a": MAG129, "b": lambda: _real((B, 129, T), F32, 19)},
         {"a": REAL3, "b": REAL3})

PARAMS = [(cid, arg, name) for cid, (_, _, views, _) in CASES.items() for arg, names in views.items() for name in names]
_DENSE = {}


def _args(cid):
    return {k: make() for k, make in CASES[cid][1].items()}


def dense(cid):
    """The entry point on dense inputs, once; its route is asserted there."""
    if cid not in _DENSE:
        fn, _, _, route = CASES[cid]
        _DENSE[cid] = fn(**_args(cid))
        if route is not None:
            route()
    return _DENSE[cid]


@pytest.mark.parametrize("cid,arg,name", PARAMS, ids=["-".join(p) for p in PARAMS])
def test_a_view_gives_the_bits_of_its_dense_twin(cid, arg, name, request):
    if "-fused-" in cid:
        request.getfixturevalue("chunked_kernel")                  # (12 frames: the small-problem rule would pick the frame kernel)
    fn = CASES[cid][0]
    Z = _args(cid)
    if name == "expanded":
        Z[arg] = L.repeated(Z[arg])
    view, base = L.build(name, Z[arg])
    twin = L.dense_twin(view, Z[arg])
    before = base.clone()
    want = fn(**dict(Z, **{arg: twin})) if name == "expanded" else dense(cid)      # (equal items are another input)
    got = fn(**dict(Z, **{arg: view}))
    assert_same(got, want)
    assert torch.equal(base, before), "the call wrote into the caller's buffer"


def test_metrics_with_both_operands_in_different_layouts():
    a, b = MAG129(), _real((B, 129, T), F32, 19)
    for name in ("sc", "snr", "ser"):
        for la, lb in (("strided", "offset"), ("neg", "step_last"), ("step_batch", "strided")):
            (va, ba), (vb, bb) = L.build(la, a), L.build(lb, b)
            keep = ba.clone(), bb.clone()
            assert_same(getattr(si, name)(va, vb), dense(name))
            assert torch.equal(ba, keep[0]) and torch.equal(bb, keep[1])


def test_mel_fb_as_a_fortran_order_ndarray():
    fb = si.mel_filterbank(8000, 256, 20)
    f_order = np.asfortranarray(fb)
    assert f_order.flags.f_contiguous and not f_order.flags.c_contiguous and np.array_equal(f_order, fb)
    keep = f_order.copy()
    assert_same(si.mel_to_stft(MEL(), f_order, n_iter=5, **KW), dense("mel_to_stft"))
    assert np.array_equal(f_order, keep)


def test_l_bfgs_init_x0_at_an_offset():
    """`init_x0` is optimised in place: the view holds the result, the rest of the buffer is untouched.  Not bit for bit: a float32
    `init_x0` on a 16-byte boundary is optimised by the device-resident loop, one off it by the host-driven loop
    (`lbfgs.LBFGS._device_ok`), and the two take their float64 sums in different orders.  The bound is the one
    `test_device_resident_optimiser_retraces_the_host_driven_loop` holds those two loops to while the memory is short: 1e-6."""
    x0 = X0()
    view, base = L.build("offset", x0)
    before = base.clone()
    want = dense("L_BFGS")
    got = _lbfgs(MAG129(), view)
    assert got.shape == want.shape and got.dtype == want.dtype and got.device == want.device
    assert got.data_ptr() == view.data_ptr()
    e = rel_l2(got.cpu().numpy(), want.cpu().numpy())
    print(f"L_BFGS, init_x0 at an offset against the aligned run: rel-L2 {e:.3e}")
    assert e < 1e-6
    assert not torch.equal(view, x0) and torch.equal(base[:1], before[:1]) and torch.equal(base[1 + x0.numel():], before[1 + x0.numel():])


# ---------------------------------------------------------------------------------------------------------------------------
# gradients: the leaf keeps its strides and bits, the cotangent comes expanded, strided and at an offset
# ---------------------------------------------------------------------------------------------------------------------------
class _Probe(torch.autograd.Function):
    """identity behind `out`: records the layout of the cotangent that arrives"""

    @staticmethod
    def forward(ctx, x, log):
        ctx.log = log
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        ctx.log.append((g.is_conj(), tuple(g.stride()), g.data_ptr() % 16))
        return g, None


GRADS = {}


def grad_case(cid, fn, args, leaf, builders):
    GRADS[cid] = (fn, args, leaf, builders)


_GIT = dict(max_iter=3, tol=0, verbose=False)
grad_case("griffin_lim-mag", lambda spec: si.griffin_lim(spec, **_GIT, **KW), {"spec": MAG129}, "spec", ("strided", "offset"))
grad_case("griffin_lim-start", lambda spec: si.griffin_lim(spec, **_GIT, **KW), {"spec": SPEC129}, "spec",
          ("strided", "offset", "conj", "conj_strided"))
grad_case("ADMM-mag", lambda spec: si.ADMM(spec, **_GIT, **KW), {"spec": MAG129}, "spec", ("strided", "offset"))
grad_case("ADMM-start", lambda spec: si.ADMM(spec, **_GIT, **KW), {"spec": SPEC129}, "spec", ("conj", "conj_strided"))
grad_case("RTISI_LA", lambda spec: si.RTISI_LA(spec, look_ahead=2, max_iter=2, verbose=0, **KW), {"spec": MAG129}, "spec",
          ("strided", "offset"))
grad_case("agla_unfolded-mag", lambda spec: si.agla_unfolded(spec, 3, 0.9, None, 1.2, **KW), {"spec": MAG129}, "spec",
          ("strided", "offset"))
grad_case("agla_unfolded-start", lambda spec: si.agla_unfolded(spec, 3, 0.9, None, 1.2, **KW), {"spec": SPEC129}, "spec",
          ("strided", "offset", "conj", "conj_strided"))
grad_case("constrained_unfolded-known_spec",
          lambda spec, known_spec, known_wave: si.constrained_unfolded(spec, known_spec, SMASK(), known_wave, WMASK(), 3, 0.9, None,
                                                                       1.2, **KW),
          {"spec": MAG129, "known_spec": SPEC129, "known_wave": WAVE}, "known_spec", ("strided", "conj", "conj_strided"))
grad_case("constrained_unfolded-start",
          lambda spec, known_spec, known_wave: si.constrained_unfolded(spec, known_spec, SMASK(), known_wave, WMASK(), 3, 0.9, None,
                                                                       1.2, **KW),
          {"spec": SPEC129, "known_spec": SPEC129, "known_wave": WAVE}, "spec", ("offset", "conj"))
grad_case("constrained_unfolded-known_wave",
          lambda spec, known_spec, known_wave: si.constrained_unfolded(spec, known_spec, SMASK(), known_wave, WMASK(), 3, 0.9, None,
                                                                       1.2, **KW),
          {"spec": MAG129, "known_spec": SPEC129, "known_wave": WAVE}, "known_wave", ("strided", "offset"))
grad_case("misi_unfolded-mag", lambda specs, mixture: si.misi_unfolded(specs, mixture, n_iter=2, **KW),
          {"specs": lambda: _real((B, 2, 129, T), F32, 12), "mixture": MIX}, "specs", ("strided", "offset"))
grad_case("misi_unfolded-start", lambda specs, mixture: si.misi_unfolded(specs, mixture, n_iter=2, **KW),
          {"specs": lambda: _cplx((B, 2, 129, T), F32, 13), "mixture": MIX}, "specs", ("strided", "conj", "conj_strided"))
grad_case("misi_unfolded-mixture", lambda specs, mixture: si.misi_unfolded(specs, mixture, n_iter=2, **KW),
          {"specs": lambda: _real((B, 2, 129, T), F32, 12), "mixture": MIX}, "mixture", ("strided", "offset"))
grad_case("mel_to_stft_unfolded", lambda mel: si.mel_to_stft_unfolded(mel, MEL_FB(), n_iter=5, **KW), {"mel": MEL}, "mel",
          ("strided", "offset"))
grad_case("gla_projection-x", lambda x, mag: si.gla_projection(x, mag, **KW), {"x": WAVE, "mag": MAG129}, "x", ("strided", "offset"))
grad_case("gla_projection-mag", lambda x, mag: si.gla_projection(x, mag, **KW), {"x": WAVE, "mag": MAG129}, "mag",
          ("strided", "offset"))
grad_case("stft", lambda x: si.stft(x, n_fft=256, **KW), {"x": WAVE}, "x", ("strided", "offset"))
grad_case("istft", lambda spec: si.istft(spec, **KW), {"spec": SPEC129}, "spec", ("strided", "offset", "conj", "conj_strided"))

G_LAYOUTS = ("expanded", "strided", "offset")
GPARAMS = [(cid, name, gl) for cid, (_, _, _, names) in GRADS.items() for name in names for gl in G_LAYOUTS]
_GDENSE = {}


def _gargs(cid):
    return {k: make() for k, make in GRADS[cid][1].items()}


def _cotangent(out, gl):
    G = _cplx(out.shape, out.dtype, 21) if out.is_complex() else _real(out.shape, out.dtype, 21, positive=False)
    return L.repeated(G) if gl == "expanded" else G


def _dense_grad(cid, gl):
    """The leaf's gradient on dense inputs under a dense cotangent: one per entry point and kind of cotangent (an expanded one
    has equal items, another value)."""
    key = (cid, gl == "expanded")
    if key not in _GDENSE:
        fn, _, leaf, _ = GRADS[cid]
        Z = _gargs(cid)
        Z[leaf] = Z[leaf].clone().requires_grad_()
        out = fn(**Z)
        _GDENSE[key] = (out.detach(), torch.autograd.grad(out, Z[leaf], grad_outputs=_cotangent(out, gl))[0])
    return _GDENSE[key]


@pytest.mark.parametrize("cid,name,gl", GPARAMS, ids=["-".join(p) for p in GPARAMS])
def test_gradient_of_a_view_under_a_laid_out_cotangent(cid, name, gl):
    fn, _, leaf, _ = GRADS[cid]
    Z = _gargs(cid)
    view, base = L.build(name, Z[leaf])
    before = base.clone()
    want_out, want = _dense_grad(cid, gl)
    x = view.detach().requires_grad_()
    assert x.stride() == view.stride() and x.is_conj() == view.is_conj() and x.data_ptr() == view.data_ptr()
    out = fn(**dict(Z, **{leaf: x}))
    assert_same(out.detach(), want_out)
    g, gbase = L.build(gl, _cotangent(out, gl))
    gkeep = gbase.clone()
    log = []
    got, = torch.autograd.grad(_Probe.apply(out, log), x, grad_outputs=g)
    assert log == [(g.is_conj(), tuple(g.stride()), g.data_ptr() % 16)], (log, g.stride())     # the layout did reach backward
    assert got.shape == x.shape
    assert_same(got, want)
    assert torch.equal(base, before) and torch.equal(gbase, gkeep)


def test_stft_backward_takes_a_lazily_conjugated_gradient():
    """`(S.conj() * k).real.sum().backward()`: the gradient that reaches `stft`'s backward is contiguous with the conjugate bit
    set - the probe shows it - and `x.grad` must be what the resolved gradient gives: 2 Re<.,.> pairs k with S, so the dense run
    is `stft`'s adjoint applied to k itself."""
    x = WAVE()
    k = _cplx((B, 129, T), F32, 22)
    log = []
    leaf = x.clone().requires_grad_()
    out = _Probe.apply(si.stft(leaf, n_fft=256, **KW), log)
    (out.conj() * k).real.sum().backward()
    assert len(log) == 1 and log[0][0] is True, log
    dense_leaf = x.clone().requires_grad_()
    want, = torch.autograd.grad(si.stft(dense_leaf, n_fft=256, **KW), dense_leaf, grad_outputs=k)
    assert_same(leaf.grad, want)
    # ... and against torch's own transform in float64 (test_gpu_projection.test_stft_and_istft: 1e-9 in float64; here float32
    # data, so the transform's float32 rounding, 2e-5 as in test_gradients_come_back_as_the_inputs_are)
    x64 = x.double().cpu().requires_grad_()
    s64 = torch.stft(x64, 256, hop_length=64, window=torch.hann_window(256, dtype=F64), return_complex=True)
    (s64.conj() * k.cpu().to(C128)).real.sum().backward()
    assert rel_l2(leaf.grad.cpu().numpy(), x64.grad.numpy()) <= 2e-5


# ---------------------------------------------------------------------------------------------------------------------------
# independent anchors: the conjugate view against something that is not this library
# ---------------------------------------------------------------------------------------------------------------------------
def test_anchor_istft_of_a_conjugate_view_against_torch_istft():
    """float64, `test_gpu_projection.test_stft_and_istft`'s bound for this transform: 1e-9"""
    S = _cplx((B, 129, T), F64, 23)
    S[:, 0].imag = 0
    S[:, -1].imag = 0                                              # (torch.istft's one-sided input: real DC and Nyquist bins)
    view, _ = L.build("conj", S)
    w = torch.hann_window(256, dtype=F64)
    y = si.istft(view, hop_length=64, window=w)
    ref = torch.istft(view.resolve_conj().cpu(), 256, hop_length=64, window=w, length=_length(256, 64))
    e = rel_l2(y.cpu().numpy(), ref.numpy())
    print(f"istft(conj view) against torch.istft: {e:.3e}")
    assert y.shape == ref.shape and e <= 1e-9


@pytest.mark.parametrize("dtype", (F32, F64), ids=("f32", "f64"))
def test_anchor_phase_vocoder_of_a_conjugate_view_against_the_definition(dtype):
    """`test_gpu_pvoc.test_parity_with_the_float64_definition`'s bounds"""
    s = _cplx((B, 65, 40), dtype, 24)
    view, _ = L.build("conj", s)
    kw = dict(hop_length=32, window=torch.hann_window(128, dtype=dtype))
    ref = pvoc_ref(s.cpu(), 0.8, 128, 32)
    err = max_err(si.phase_vocoder(view, 0.8, **kw).cpu(), ref)
    wrong = max_err(pvoc_ref(s.conj().resolve_conj().cpu(), 0.8, 128, 32), ref)
    print(f"phase_vocoder(conj view) {dtype}: error {err:.2e}; the conjugate's own result is {wrong:.2e} away")
    if dtype == F64:
        assert err <= 1e-11
    else:
        e_cal = max_err(pvoc_ref(s.cpu(), 0.8, 128, 32, angle_dtype=F32), ref)
        assert err <= 4 * e_cal + 2.0 ** -22
    assert wrong > 1e-2                                            # (the test can tell the two apart)


def test_anchor_griffin_lim_from_a_conjugate_view_on_the_fused_route(chunked_kernel):
    """`test_gpu_fast`'s bar against the oracle: waveform rel-L2 < 1e-4"""
    n_fft, hop = 512, 128
    mag = np.random.default_rng(5).random((B, n_fft // 2 + 1, T), dtype=np.float32)
    w = hann(n_fft)
    init = oracle.phase_init(mag, hop_length=hop, window=w)
    ref = oracle.griffin_lim(init, max_iter=3, alpha=0.3, tol=0, hop_length=hop, window=w)
    view, _ = L.build("conj", torch.from_numpy(init).to(C64).to(DEV))
    y = si.griffin_lim(view, max_iter=3, alpha=0.3, tol=0, verbose=False, hop_length=hop, window=torch.from_numpy(w))
    assert _plan(n_fft, hop, F32).path == "fused"
    e = rel_l2(y.cpu().numpy(), ref.reshape(y.shape))
    print(f"griffin_lim from a conjugate-view start, fused route, against the oracle: {e:.3e}")
    assert e < 1e-4


def test_anchor_complex_hpss_of_a_conjugate_view_against_the_definition():
    """`test_gpu_hpss.test_masks_and_components`'s bound, 2^-23 per part in float32"""
    x = _cplx(HS, F32, 18)
    view, _ = L.build("conj", x)
    H, P = si.hpss(view, 5)
    xn = x.cpu().numpy()
    harm, perc = medians(xn, 5, 5)
    ref_h, ref_p = masks_of(harm, perc, 2.0, 1.0, 1.0, real_dtype=np.float32)
    for got, ref in ((H, times(xn, ref_h)), (P, times(xn, ref_p))):
        wide = got.cpu().numpy().astype(np.complex128)
        for g, r in ((wide.real, ref.real), (wide.imag, ref.imag)):
            assert (np.abs(g - r) <= 2.0 ** -23 * np.abs(r)).all()
    assert H.dtype == P.dtype == C64 and not H.is_conj()


# ---------------------------------------------------------------------------------------------------------------------------
# the metric reduction: k_metric_partials / k_finish_partials decide every stop rule
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (F32, F64), ids=("f32", "f64"))
@pytest.mark.parametrize("n", (1, 255, 256, 257, 2047, 2049, (1 << 21) + 1))
def test_metric_sums_against_fsum(n, dtype):
    """sum((a-b)^2), sum(a^2), sum(b^2) in float64 of the inputs' values against `math.fsum` of the float64 terms.  The terms are
    non-negative and each takes at most three roundings (the difference, the square - or an fma -, the add): whatever the order
    of summation, every sum is within (n + 3) 2^-53 of the exact one, relatively.  2^21 + 1 is past the 1024-block cap."""
    import math
    from spectrogram_inversion_amd.metrics import _sums
    g = torch.Generator().manual_seed(n)
    a = torch.randn(n, generator=g, dtype=F64).to(dtype)
    b = (a.double() + 0.1 * torch.randn(n, generator=g, dtype=F64)).to(dtype)
    s = _sums(a.to(DEV), b.to(DEV))
    a64, b64 = a.double().numpy(), b.double().numpy()
    exact = (math.fsum((a64 - b64) ** 2), math.fsum(a64 ** 2), math.fsum(b64 ** 2))
    bound = (n + 3) * 2.0 ** -53
    for k, (got, ref) in enumerate(zip(s[:3], exact)):
        err = abs(got - ref) / ref
        print(f"n {n} {dtype} sum {k}: relative error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (k, err, bound)
    assert s[3] == n
