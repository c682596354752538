#!/usr/bin/env python3
"""Generate the golden fixtures under tests/golden/ from the UNMODIFIED reference.

Run only in the build container, where the reference checkout is mounted:

    PYTHONPATH=/root/reference python tests/golden/make_golden.py

It imports `torch_specinv` (v0.2.1) with the torch CPU path (torch 2.10.0 here)
and stores inputs + expected outputs as small .npz files.  Nothing of the
reference's source is stored - only data.  The fixtures travel to the GPU box;
this script and the reference do not need to.

Inputs come from `numpy.random.default_rng(seed)` so they are regenerable
without torch.  Each case also stores the reference's own float32-vs-float64
self-difference where that is the natural tolerance yardstick.
"""
import os
import sys

import numpy as np
import torch

REF = os.environ.get("SPECINV_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import torch_specinv.methods as M          # noqa: E402
import torch_specinv.metrics as MET        # noqa: E402
from spectrogram_inversion_amd.mel import mel_filterbank   # noqa: E402

torch.set_num_threads(8)


# ---- progress-bar stand-in that records what _training_loop reports -------- #
class _Bar:
    last = None

    def __init__(self, *a, total=None, disable=False, **k):
        self.post = []
        self.n = 0
        _Bar.last = self

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def set_postfix(self, **kw):
        self.post.append(dict(kw))

    def update(self, n=1):
        self.n += n


M.tqdm = _Bar


def save(name, **arrays):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"{name}: {os.path.getsize(path) / 1024:.1f} KiB")


def hann(n, dtype=np.float32):
    return (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)).astype(dtype)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def trace_of(bar, metric):
    return np.array([[p[metric.upper()], p["loss"]] for p in bar.post], dtype=np.float64)


# --------------------------------------------------------------------------- #
def g0_stft():
    """Pins oracle.stft / istft / envelope against torch.stft and the reference's _istft."""
    rng = np.random.default_rng(100)
    x = rng.standard_normal((2, 1500)).astype(np.float32)
    out = {"x": x}
    cases = [
        dict(n_fft=256, hop_length=64, window="hann", center=True, pad_mode="reflect",
             normalized=False, onesided=True),
        dict(n_fft=256, hop_length=100, window="rect", center=True, pad_mode="constant",
             normalized=True, onesided=True),
        dict(n_fft=128, hop_length=32, window="hann", center=False, pad_mode="reflect",
             normalized=False, onesided=False),
        dict(n_fft=256, hop_length=64, window="hann200", center=True, pad_mode="replicate",
             normalized=False, onesided=True),
        dict(n_fft=256, hop_length=64, window="hann", center=True, pad_mode="circular",
             normalized=True, onesided=False),
    ]
    for i, c in enumerate(cases):
        n = c["n_fft"]
        kw = dict(hop_length=c["hop_length"], center=c["center"], pad_mode=c["pad_mode"],
                  normalized=c["normalized"], onesided=c["onesided"])
        if c["window"] == "hann":
            kw["window"] = t(hann(n))
        elif c["window"] == "hann200":
            kw["window"] = t(hann(200))
            kw["win_length"] = 200
        s = torch.stft(t(x), n, return_complex=True, **kw)
        n_fft, pa = M._args_helper(s.abs(), **kw)
        assert n_fft == n
        w = M._get_ola_weight(pa["window"])
        xr, env = M._istft(s, n_fft, w, **pa)
        out[f"spec{i}"] = s.numpy()
        out[f"istft{i}"] = xr.numpy()
        out[f"env{i}"] = env.numpy()
        out[f"win{i}"] = pa["window"].numpy()
    out["n_cases"] = np.array(len(cases))
    save("g0_stft", **out)


def g1_phase_init():
    out = {}
    for i, (shape, n_hop, seed) in enumerate([((2, 129, 40), None, 1), ((2, 513, 64), 256, 2),
                                              ((1, 33, 1024), 16, 3)]):
        rng = np.random.default_rng(seed)
        mag = rng.random(shape, dtype=np.float32)
        kw = {} if n_hop is None else {"hop_length": n_hop}
        out[f"mag{i}"] = mag
        out[f"hop{i}"] = np.array(0 if n_hop is None else n_hop)
        out[f"out{i}"] = M.phase_init(t(mag), **kw).numpy()
        out[f"out64_{i}"] = M.phase_init(t(mag.astype(np.float64)), **kw).numpy()
    # 2-D input keeps its shape (methods.py:615)
    mag2 = np.random.default_rng(4).random((65, 12), dtype=np.float32)
    out["mag3"] = mag2
    out["hop3"] = np.array(0)
    out["out3"] = M.phase_init(t(mag2)).numpy()
    out["out64_3"] = M.phase_init(t(mag2.astype(np.float64))).numpy()
    out["n_cases"] = np.array(4)
    save("g1_phase_init", **out)


def g2_gla():
    rng = np.random.default_rng(20)
    mag = rng.random((2, 257, 40), dtype=np.float32)
    win = hann(512)
    kw = dict(hop_length=128, window=t(win))
    init = M.phase_init(t(mag), **kw)
    out = {"mag": mag, "window": win, "hop": np.array(128), "init": init.numpy()}
    for alpha in (0.0, 0.3, 0.99):
        for it in (1, 10, 100):
            y = M.griffin_lim(init, max_iter=it, alpha=alpha, tol=0, verbose=True, eva_iter=10, **kw)
            y64 = M.griffin_lim(init.to(torch.complex128), max_iter=it, alpha=alpha, tol=0, verbose=True,
                                eva_iter=10, window=t(win.astype(np.float64)), hop_length=128)
            key = f"a{alpha}_it{it}"
            out["wave_" + key] = y.numpy()
            out["wave64_" + key] = y64.numpy()
            if it == 100:
                M.griffin_lim(init, max_iter=it, alpha=alpha, tol=0, verbose=True, eva_iter=10, **kw)
                out["trace_" + key] = trace_of(_Bar.last, "sc")
    # magnitude input (goes through phase_init), other metrics
    for metric in ("snr", "ser"):
        y = M.griffin_lim(t(mag), max_iter=20, alpha=0.3, tol=0, eva_iter=5, metric=metric, **kw)
        out["wave_mag_" + metric] = y.numpy()
        out["trace_mag_" + metric] = trace_of(_Bar.last, metric)
    # default tol=1e-6, default alpha: record where it stops
    y = M.griffin_lim(init, max_iter=2000, eva_iter=10, **kw)
    out["wave_tol"] = y.numpy()
    out["iters_tol"] = np.array(_Bar.last.n)
    out["trace_tol"] = trace_of(_Bar.last, "sc")
    # 2-D input and (1, F, T) input shape rules
    out["wave_2d"] = M.griffin_lim(t(mag[0]), max_iter=3, alpha=0.3, tol=0, **kw).numpy()
    out["wave_1ft"] = M.griffin_lim(t(mag[:1]), max_iter=3, alpha=0.3, tol=0, **kw).numpy()
    save("g2_gla", **out)


def _sweep_cases():
    cases = []
    wins = [(None, "none"), (300, "none"), (300, "hann300")]
    # a reduced cartesian design that still touches every option value with
    # both center settings and every pad mode (test/test_griffin.py:24-32)
    idx = 0
    for wl, wname in wins:
        for hop in (None, 128, 100):
            for center in (True, False):
                for normalized in (False, True):
                    for onesided in (True, False):
                        pads = ["reflect", "constant", "replicate", "circular"] if center else ["reflect"]
                        for pad in pads:
                            idx += 1
                            if idx % 5 != 0:          # keep every 5th combination
                                continue
                            cases.append(dict(win_length=wl, wname=wname, hop_length=hop, center=center,
                                              normalized=normalized, onesided=onesided, pad_mode=pad))
    return cases


def g3_sweep():
    rng = np.random.default_rng(30)
    x = rng.standard_normal(2205).astype(np.float32)
    out = {"x": x}
    cases = _sweep_cases()
    meta = []
    for i, c in enumerate(cases):
        kw = dict(hop_length=c["hop_length"], win_length=c["win_length"], center=c["center"],
                  pad_mode=c["pad_mode"], normalized=c["normalized"], onesided=c["onesided"])
        kw["window"] = t(hann(300)) if c["wname"] == "hann300" else None
        spec = torch.stft(t(x), 512, return_complex=True, **kw).abs()
        for name, fn, extra in (("gla", M.griffin_lim, dict(alpha=0.5)), ("admm", M.ADMM, dict(rho=0.5))):
            y = fn(spec, max_iter=2, verbose=False, **extra, **kw)
            out[f"{name}{i}"] = y.numpy()
        out[f"spec{i}"] = spec.numpy()
        meta.append(f"{c['win_length']}|{c['wname']}|{c['hop_length']}|{int(c['center'])}|"
                    f"{int(c['normalized'])}|{int(c['onesided'])}|{c['pad_mode']}")
    out["meta"] = np.array(meta)
    save("g3_sweep", **out)
    print("  sweep cases:", len(cases))


def g4_admm():
    rng = np.random.default_rng(40)
    mag = rng.random((2, 257, 40), dtype=np.float32)
    win = hann(512)
    kw = dict(hop_length=128, window=t(win))
    kw64 = dict(hop_length=128, window=t(win.astype(np.float64)))
    init = M.phase_init(t(mag), **kw)
    out = {"mag": mag, "window": win, "hop": np.array(128), "init": init.numpy()}
    for rho in (0.1, 1.0):
        for it in (1, 2, 5, 200):
            y = M.ADMM(init, max_iter=it, rho=rho, tol=0, verbose=True, eva_iter=10, **kw)
            bar = _Bar.last
            y64 = M.ADMM(init.to(torch.complex128), max_iter=it, rho=rho, tol=0, verbose=True, eva_iter=10, **kw64)
            key = f"r{rho}_it{it}"
            if it < 200:
                out["wave_" + key] = y.numpy()
                out["wave64_" + key] = y64.numpy()
            else:
                out["trace_" + key] = trace_of(bar, "sc")
                out["trace64_" + key] = trace_of(_Bar.last, "sc")
    y = M.ADMM(t(mag), max_iter=2000, **kw)           # default tol / rho
    out["iters_tol"] = np.array(_Bar.last.n)
    out["trace_tol"] = trace_of(_Bar.last, "sc")
    save("g4_admm", **out)


def g5_rtisi():
    out = {}
    meta = []
    i = 0
    for hop in (64, 100):
        rng = np.random.default_rng(50 + hop)
        mag = rng.random((2, 129, 14), dtype=np.float32)
        win = hann(256)
        out[f"mag_h{hop}"] = mag
        for la in (-1, 0, 2):
            for asym in (True, False):
                for alpha in (0.0, 0.99):
                    kw = dict(hop_length=hop, window=t(win))
                    y = M.RTISI_LA(t(mag), look_ahead=la, asymmetric_window=asym, max_iter=3, alpha=alpha,
                                   verbose=False, **kw)
                    y64 = M.RTISI_LA(t(mag.astype(np.float64)), look_ahead=la, asymmetric_window=asym, max_iter=3,
                                     alpha=alpha, verbose=False, hop_length=hop,
                                     window=t(win.astype(np.float64)))
                    out[f"wave{i}"] = y.numpy()
                    out[f"wave64_{i}"] = y64.numpy()
                    meta.append(f"{hop}|{la}|{int(asym)}|{alpha}")
                    i += 1
    out["meta"] = np.array(meta)
    out["window"] = hann(256)
    # one-iteration, few-frame runs: the output is a direct image of single inner steps
    rng = np.random.default_rng(59)
    mag = rng.random((1, 129, 3), dtype=np.float32)
    out["mag_single"] = mag
    for asym in (True, False):
        y = M.RTISI_LA(t(mag), look_ahead=1, asymmetric_window=asym, max_iter=1, alpha=0.99, verbose=False,
                       hop_length=64, window=t(hann(256)))
        out[f"wave_single_asym{int(asym)}"] = y.numpy()
    # other stft options through RTISI (test/test_rtisila.py:24-34)
    x = np.random.default_rng(58).standard_normal(1200).astype(np.float32)
    out["x_opts"] = x
    opts = [dict(win_length=300, window=None, hop_length=None, center=True, normalized=True, onesided=True),
            dict(win_length=300, window=t(hann(300)), hop_length=128, center=False, normalized=False, onesided=False),
            dict(win_length=None, window=None, hop_length=128, center=True, normalized=False, onesided=False)]
    for j, kw in enumerate(opts):
        spec = torch.stft(t(x), 512, return_complex=True, pad_mode="reflect", **kw).abs()
        for asym in (True, False):
            y = M.RTISI_LA(spec, look_ahead=2, asymmetric_window=asym, max_iter=2, verbose=False, **kw)
            out[f"opt{j}_asym{int(asym)}"] = y.numpy()
        out[f"opt{j}_spec"] = spec.numpy()
    # larger-size SC value (N=2048, hop=512, T=64, 25 it) for both window settings
    rng = np.random.default_rng(57)
    mag = rng.random((1, 1025, 64), dtype=np.float32)
    out["mag_big_seed"] = np.array(57)
    for asym in (True, False):
        kw = dict(hop_length=512, window=t(hann(2048)))
        y = M.RTISI_LA(t(mag), look_ahead=3, asymmetric_window=asym, max_iter=25, verbose=False, **kw)
        s = torch.stft(y, 2048, return_complex=True, **kw).abs()
        out[f"big_sc_asym{int(asym)}"] = np.array(MET.sc(s, t(mag)[..., :s.shape[-1]]).item())
        out[f"big_wave_asym{int(asym)}"] = y.numpy()
    save("g5_rtisi", **out)


def g6_lbfgs():
    out = {}
    # (a) |STFT| transform, like test/test_lbfgs.py
    rng = np.random.default_rng(60)
    x_true = rng.standard_normal((2, 2000)).astype(np.float32)
    nfft = 256

    def trsfn(x):
        return torch.stft(x, nfft, return_complex=True).abs()

    spec = trsfn(t(x_true))
    x0 = (rng.standard_normal((2, 2000)) * 1e-2).astype(np.float32)
    out["mag_spec"] = spec.numpy()
    out["mag_x0"] = x0
    # forward / loss / gradient at x0
    xp = t(x0.copy()).requires_grad_(True)
    loss = torch.nn.functional.mse_loss(trsfn(xp), spec)
    loss.backward()
    out["mag_loss0"] = np.array(loss.item())
    out["mag_grad0"] = xp.grad.numpy()
    for tag, kw in (("plain", dict(max_iter=10)),
                    ("wolfe", dict(max_iter=10, line_search_fn="strong_wolfe")),
                    ("hist3", dict(max_iter=12, history_size=3))):
        y = M.L_BFGS(spec, trsfn, init_x0=t(x0.copy()), outer_max_iter=2, tol=0, eva_iter=1, verbose=True, **kw)
        out[f"mag_x_{tag}"] = y.numpy()
        out[f"mag_trace_{tag}"] = trace_of(_Bar.last, "sc")
    y = M.L_BFGS(spec, trsfn, init_x0=t(x0.copy()), outer_max_iter=1, tol=0, eva_iter=1, verbose=True, max_iter=3)
    out["mag_x_3inner"] = y.numpy()

    # (b) log-mel transform, BASELINE config 5 shape at small T
    n_fft, hop, T = 2048, 512, 12
    fb = mel_filterbank(22050, n_fft, 80)
    win = hann(n_fft)
    L = (T - 1) * hop
    xs = (0.1 * rng.standard_normal((2, L))).astype(np.float32)

    def mel_fn(x):
        s = torch.stft(x, n_fft, hop_length=hop, window=t(win), return_complex=True).abs()
        return torch.log1p(torch.matmul(t(fb), s))

    tgt = mel_fn(t(xs))
    xi = (1e-2 * rng.standard_normal((2, L))).astype(np.float32)
    xp = t(xi.copy()).requires_grad_(True)
    v = mel_fn(xp)
    loss = torch.nn.functional.mse_loss(v, tgt)
    loss.backward()
    out["mel_target"] = tgt.numpy()
    out["mel_x"] = xi
    out["mel_fwd"] = v.detach().numpy()
    out["mel_loss"] = np.array(loss.item())
    out["mel_grad"] = xp.grad.numpy()
    out["mel_fb_check"] = fb[:, ::64].copy()
    for tag, kw in (("plain", dict()), ("wolfe", dict(line_search_fn="strong_wolfe"))):
        y = M.L_BFGS(tgt, mel_fn, init_x0=t(xi.copy()), outer_max_iter=1, tol=0, eva_iter=1, verbose=True, **kw)
        out[f"mel_x_{tag}"] = y.numpy()
        out[f"mel_trace_{tag}"] = trace_of(_Bar.last, "sc")
    save("g6_lbfgs", **out)


def g7_metrics():
    rng = np.random.default_rng(70)
    a = rng.random((2, 65, 30), dtype=np.float32)
    b = rng.random((2, 65, 30), dtype=np.float32)
    vals = np.array([MET.sc(t(a), t(b)).item(), MET.snr(t(a), t(b)).item(), MET.ser(t(a), t(b)).item(),
                     torch.nn.functional.mse_loss(t(a), t(b)).item()], dtype=np.float64)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    vals64 = np.array([MET.sc(t(a64), t(b64)).item(), MET.snr(t(a64), t(b64)).item(),
                       MET.ser(t(a64), t(b64)).item(),
                       torch.nn.functional.mse_loss(t(a64), t(b64)).item()], dtype=np.float64)
    save("g7_metrics", a=a, b=b, vals=vals, vals64=vals64)


def g8_f64():
    rng = np.random.default_rng(80)
    mag = rng.random((2, 129, 24))
    win = hann(256, np.float64)
    kw = dict(hop_length=64, window=t(win))
    init = M.phase_init(t(mag), **kw)
    out = {"mag": mag, "window": win, "init": init.numpy()}
    out["gla1"] = M.griffin_lim(init, max_iter=1, alpha=0.3, tol=0, verbose=False, **kw).numpy()
    out["gla5"] = M.griffin_lim(init, max_iter=5, alpha=0.3, tol=0, verbose=False, **kw).numpy()
    out["admm1"] = M.ADMM(init, max_iter=1, rho=0.1, tol=0, verbose=False, **kw).numpy()
    out["admm5"] = M.ADMM(init, max_iter=5, rho=0.1, tol=0, verbose=False, **kw).numpy()
    out["rtisi"] = M.RTISI_LA(t(mag), look_ahead=2, asymmetric_window=True, max_iter=2, verbose=False, **kw).numpy()
    save("g8_f64", **out)


def g9_lbfgs_rosen():
    """torch.optim.LBFGS on a well-conditioned analytic problem in float64: pins the
    two-loop recursion and the strong-Wolfe search of the restatement without the
    float32 loss-rounding sensitivity of the STFT objectives."""
    def rosen(x):
        return (100.0 * (x[1:] - x[:-1] ** 2) ** 2 + (1.0 - x[:-1]) ** 2).sum()

    out = {}
    x0 = np.linspace(-1.2, 1.0, 10)
    out["x0"] = x0
    for tag, kw in (("wolfe", dict(max_iter=40, history_size=5, line_search_fn="strong_wolfe")),
                    ("wolfe_h100", dict(max_iter=25, line_search_fn="strong_wolfe")),
                    ("fixed", dict(max_iter=30, lr=1e-3, history_size=4))):
        x = torch.nn.Parameter(t(x0.copy()))
        opt = torch.optim.LBFGS([x], **kw)
        losses = []

        def closure():
            opt.zero_grad()
            l = rosen(x)
            l.backward()
            losses.append(l.item())
            return l

        for _ in range(2):            # two optimizer.step calls: state carries over
            opt.step(closure)
        out[f"x_{tag}"] = x.detach().numpy().copy()
        out[f"losses_{tag}"] = np.array(losses)
    save("g9_lbfgs_rosen", **out)


def g10_autograd():
    """Gradients of the reference's griffin_lim w.r.t. the input spectrogram (torch autograd)."""
    out = {}
    rng = np.random.default_rng(110)
    cases = [("f32_hann", np.float32, 128, 32, True, dict()), ("f64_hann", np.float64, 128, 32, True, dict()),
             ("f64_rect_default", np.float64, 128, None, False, dict()),
             ("f64_const_pad", np.float64, 64, 16, True, dict(pad_mode="constant")),
             ("f64_normalized", np.float64, 64, 16, True, dict(normalized=True))]
    for tag, dt, n_fft, hop, use_hann, extra in cases:
        mag = (rng.random((2, n_fft // 2 + 1, 12)) + 0.05).astype(dt)
        kw = dict(extra)
        if hop:
            kw["hop_length"] = hop
        if use_hann:
            kw["window"] = t(hann(n_fft, dt))
        spec = t(mag).requires_grad_(True)
        y = M.griffin_lim(spec, max_iter=3, alpha=0.5, tol=0, verbose=False, **kw)
        wv = rng.standard_normal(tuple(y.shape)).astype(dt)
        (y * t(wv)).sum().backward()
        out[f"mag_{tag}"] = mag
        out[f"w_{tag}"] = wv
        out[f"y_{tag}"] = y.detach().numpy()
        out[f"grad_{tag}"] = spec.grad.numpy()
    # complex (warm-start) input: gradient w.r.t. the complex spectrogram
    mag = (rng.random((1, 65, 10)) + 0.05)
    c = (mag * np.exp(1j * rng.uniform(-np.pi, np.pi, mag.shape))).astype(np.complex128)
    spec = t(c).requires_grad_(True)
    y = M.griffin_lim(spec, max_iter=2, alpha=0.3, tol=0, verbose=False, hop_length=32, window=t(hann(128, np.float64)))
    wv = rng.standard_normal(tuple(y.shape))
    (y * t(wv)).sum().backward()
    out["c_complex"], out["w_complex"], out["grad_complex"] = c, wv, spec.grad.numpy()
    # the reference's own test pattern (test/test_griffin.py:53-66): mse against the original signal
    x = rng.standard_normal(2000).astype(np.float32)
    sp = torch.stft(t(x), 256, return_complex=True).abs().requires_grad_(True)
    y = M.griffin_lim(sp, max_iter=2, verbose=False)
    torch.nn.functional.mse_loss(t(x)[:y.shape[0]], y).backward()
    out["x_ref_test"], out["grad_ref_test"] = x, sp.grad.numpy()
    save("g10_autograd", **out)


def g11_autograd_admm():
    """Gradients of the reference's ADMM w.r.t. the input spectrogram (torch autograd; test/test_admm.py:54-66)."""
    out = {}
    rng = np.random.default_rng(111)
    cases = [("f32_hann", np.float32, 128, 32, True, 0.1, dict()), ("f64_hann", np.float64, 128, 32, True, 0.1, dict()),
             ("f64_rect_default", np.float64, 64, None, False, 0.5, dict()),
             ("f64_twosided", np.float64, 64, 16, True, 0.2, dict(onesided=False, pad_mode="constant"))]
    for tag, dt, n_fft, hop, use_hann, rho, extra in cases:
        F_ = n_fft if extra.get("onesided") is False else n_fft // 2 + 1
        mag = (rng.random((2, F_, 12)) + 0.05).astype(dt)
        kw = dict(extra)
        if hop:
            kw["hop_length"] = hop
        if use_hann:
            kw["window"] = t(hann(n_fft, dt))
        spec = t(mag).requires_grad_(True)
        y = M.ADMM(spec, max_iter=3, rho=rho, tol=0, verbose=False, **kw)
        wv = rng.standard_normal(tuple(y.shape)).astype(dt)
        (y * t(wv)).sum().backward()
        out[f"mag_{tag}"], out[f"w_{tag}"] = mag, wv
        out[f"y_{tag}"], out[f"grad_{tag}"] = y.detach().numpy(), spec.grad.numpy()
    mag = (rng.random((1, 65, 10)) + 0.05)
    c = (mag * np.exp(1j * rng.uniform(-np.pi, np.pi, mag.shape))).astype(np.complex128)
    spec = t(c).requires_grad_(True)
    y = M.ADMM(spec, max_iter=2, rho=0.3, tol=0, verbose=False, hop_length=32, window=t(hann(128, np.float64)))
    wv = rng.standard_normal(tuple(y.shape))
    (y * t(wv)).sum().backward()
    out["c_complex"], out["w_complex"], out["grad_complex"] = c, wv, spec.grad.numpy()
    save("g11_autograd_admm", **out)


def g12_autograd_rtisi():
    """Gradients of the reference's RTISI_LA w.r.t. the magnitudes (torch autograd; test/test_rtisila.py:58-70)."""
    out = {}
    rng = np.random.default_rng(112)
    cases = [("f64_la_default_asym", np.float64, 128, 32, -1, True, 0.99, 2, dict()),
             ("f64_la_default_sym", np.float64, 128, 32, -1, False, 0.99, 2, dict()),
             ("f64_la0", np.float64, 128, 32, 0, True, 0.5, 3, dict()),
             ("f64_la1_hop50", np.float64, 128, 50, 1, True, 0.99, 2, dict()),
             ("f64_la5_alpha0", np.float64, 64, 16, 5, False, 0.0, 2, dict()),
             ("f64_twosided_norm", np.float64, 64, 16, 2, True, 0.99, 2, dict(onesided=False, normalized=True)),
             ("f64_rect_default", np.float64, 64, None, -1, True, 0.99, 1, dict()),
             ("f32_la2", np.float32, 128, 32, 2, True, 0.99, 2, dict())]
    meta = []
    for tag, dt, n_fft, hop, la, asym, alpha, iters, extra in cases:
        F_ = n_fft if extra.get("onesided") is False else n_fft // 2 + 1
        mag = (rng.random((2, F_, 9)) + 0.05).astype(dt)
        kw = dict(extra)
        if hop:
            kw["hop_length"] = hop
        if tag != "f64_rect_default":
            kw["window"] = t(hann(n_fft, dt))
        spec = t(mag).requires_grad_(True)
        y = M.RTISI_LA(spec, look_ahead=la, asymmetric_window=asym, max_iter=iters, alpha=alpha, verbose=False, **kw)
        wv = rng.standard_normal(tuple(y.shape)).astype(dt)
        (y * t(wv)).sum().backward()
        out[f"mag_{tag}"], out[f"w_{tag}"] = mag, wv
        out[f"y_{tag}"], out[f"grad_{tag}"] = y.detach().numpy(), spec.grad.numpy()
        meta.append(f"{tag}|{n_fft}|{hop or 0}|{la}|{int(asym)}|{alpha}|{iters}|{int(extra.get('onesided', True))}|"
                    f"{int(extra.get('normalized', False))}")
    out["meta"] = np.array(meta)
    # the reference's own test pattern (test/test_rtisila.py:46-70)
    x = rng.standard_normal(2000).astype(np.float32)
    sp = torch.stft(t(x), 256, return_complex=True).abs().requires_grad_(True)
    y = M.RTISI_LA(sp, max_iter=2, verbose=False)
    torch.nn.functional.mse_loss(t(x)[:y.shape[0]], y).backward()
    out["x_ref_test"], out["grad_ref_test"] = x, sp.grad.numpy()
    # same pattern in float64 (in float32 the symmetric-window recursion decorrelates between implementations)
    sp = torch.stft(t(x.astype(np.float64)), 256, return_complex=True).abs().requires_grad_(True)
    y = M.RTISI_LA(sp, max_iter=2, verbose=False)
    torch.nn.functional.mse_loss(t(x.astype(np.float64))[:y.shape[0]], y).backward()
    out["grad_ref_test64"] = sp.grad.numpy()
    save("g12_autograd_rtisi", **out)


def g13_wave_level_shapes():
    """The reference itself at the shapes the wave-level kernels specialise in (fused hop = n_fft/2, /4, /8 at n_fft
    512 ... 4096, and the frame kernel at another hop): Griffin-Lim and ADMM waveforms after a few iterations, RTISI-LA
    with the asymmetric window."""
    out, meta = {}, []
    rng = np.random.default_rng(113)
    for n_fft, hop, frames in [(1024, 128, 40), (2048, 1024, 14), (512, 128, 48), (4096, 1024, 12), (2048, 256, 24),
                               (512, 256, 30), (1024, 160, 30), (4096, 2048, 10), (2048, 512, 40), (1024, 256, 40)]:
        tag = f"{n_fft}_{hop}"
        mag = (rng.random((1, n_fft // 2 + 1, frames)) + 0.02).astype(np.float32)
        w = hann(n_fft, np.float32)
        kw = dict(hop_length=hop, window=t(w))
        init = M.phase_init(t(mag), **kw)
        out[f"mag_{tag}"] = mag
        out[f"init_{tag}"] = init.numpy()
        out[f"gla_{tag}"] = M.griffin_lim(init, max_iter=5, alpha=0.3, tol=0, verbose=False, **kw).numpy()
        out[f"admm_{tag}"] = M.ADMM(init, max_iter=3, rho=1.0, tol=0, verbose=False, **kw).numpy()
        if n_fft <= 2048:
            out[f"rtisi_{tag}"] = M.RTISI_LA(t(mag[:, :, :12]), look_ahead=-1 if hop * 8 > n_fft else 3, asymmetric_window=True,
                                             max_iter=2, alpha=0.99, verbose=False, **kw).numpy()
            out[f"rtisi64_{tag}"] = M.RTISI_LA(t(mag[:, :, :12].astype(np.float64)), look_ahead=-1 if hop * 8 > n_fft else 3,
                                               asymmetric_window=True, max_iter=2, alpha=0.99, verbose=False,
                                               hop_length=hop, window=t(hann(n_fft, np.float64))).numpy()
        meta.append(tag)
    out["meta"] = np.array(meta)
    save("g13_wave_level_shapes", **out)


def g14_wellcond(name="g14_wellcond", n_fft=512, hop=128, frames=40, seed=140):
    """A well-conditioned 100-iteration case: the magnitudes ARE the STFT of a signal (chirps + harmonics + a noise
    floor) and the starting phase is the true phase perturbed by 0.5 rad rms, so the iterates stay close to a consistent
    spectrogram and no bin with a sizeable target passes through zero - unlike g2's random (inconsistent) magnitudes,
    where one such event decorrelates a neighbourhood.  Griffin-Lim after 100 iterations, alpha 0 / 0.3 / 0.99, float32
    and float64: the strict waveform gate min(1e-4, 6 x float32-vs-float64 noise) applies to every kernel path."""
    rng = np.random.default_rng(seed)
    n = (frames - 1) * hop
    tt = np.arange(n) / 16000.0
    x = np.stack([
        0.5 * np.sin(2 * np.pi * (300 * tt + 2500 * tt * tt)) + 0.3 * np.sin(2 * np.pi * 1250 * tt + 3 * np.sin(2 * np.pi * 5 * tt)),
        sum(0.4 / k * np.sin(2 * np.pi * 220 * k * tt * (1 + 0.3 * tt)) for k in range(1, 9)),
    ]) + 0.05 * rng.standard_normal((2, n))
    win = hann(n_fft)
    kw = dict(hop_length=hop, window=t(win))
    spec = torch.stft(t(x.astype(np.float32)), n_fft, return_complex=True, **kw)
    assert spec.shape == (2, n_fft // 2 + 1, frames)
    phase = torch.angle(spec) + t((0.5 * rng.standard_normal(spec.shape)).astype(np.float32))
    init = (spec.abs() * torch.exp(1j * phase)).to(torch.complex64)
    out = {"x": x.astype(np.float32), "window": win, "hop": np.array(hop), "init": init.numpy()}
    for alpha in (0.0, 0.3, 0.99):
        y = M.griffin_lim(init, max_iter=100, alpha=alpha, tol=0, verbose=False, eva_iter=10, **kw)
        y64 = M.griffin_lim(init.to(torch.complex128), max_iter=100, alpha=alpha, tol=0, verbose=False, eva_iter=10,
                            window=t(win.astype(np.float64)), hop_length=hop)
        out[f"wave_a{alpha}"] = y.numpy()
        out[f"wave64_a{alpha}"] = y64.numpy()
        e = float((y.double() - y64).norm() / y64.norm())
        print(f"  {name} alpha {alpha}: float32 vs float64 after 100 it {e:.2e}")
    save(name, **out)


def g15_wellcond_1024():
    """g14's construction at n_fft 1024 / hop 256 (60 frames): the shape class of the hop = n_fft/4 kernels (k_fused4 and
    k_fused4_td, which carries the momentum as a signal), 100 iterations, strict gate."""
    g14_wellcond("g15_wellcond_1024", n_fft=1024, hop=256, frames=60, seed=150)


def g16_headline_2048():
    """The headline instantiation (n_fft 2048 / hop 512: k_fused4_td<16>, k_fused4<16>, k_hop<16>) against the reference itself.
    (a) g14's well-conditioned construction at 2048 / 512, 2 items x 64 frames, 100 iterations, alpha 0 / 0.3 / 0.99, float32 and
    float64 (strict waveform gate).  (b) BASELINE configs[1] exactly as bench.py runs it on rank 0 - magnitudes
    default_rng(1234).random((64, 1025, 1024), float32), periodic Hann, 100 iterations, alpha 0.3, eva_iter 10, tol 0 - through the
    unmodified reference: the ten (SC dB, loss) evaluations of the WHOLE batch (+ the SC that follows from the loss and the exact
    target norm: the reference's own float32 `norm` is 4e-3 off at this size), the final waveforms of items 0 and 63, and a float64
    run of those two items (its trace, and the reference's own float32-vs-float64 error per hop segment as the noise yardstick)."""
    import time
    g14_wellcond("g16a_wellcond_2048", n_fft=2048, hop=512, frames=64, seed=160)
    n_fft, hop, frames, batch = 2048, 512, 1024, 64
    rng = np.random.default_rng(1234)
    mag = rng.random((batch, n_fft // 2 + 1, frames), dtype=np.float32)
    win = hann(n_fft)
    kw = dict(hop_length=hop, window=t(win))
    t0 = time.time()
    y = M.griffin_lim(t(mag), max_iter=100, alpha=0.3, tol=0, verbose=True, eva_iter=10, metric="sc", **kw)
    trace = trace_of(_Bar.last, "sc")
    print(f"  reference C2 (B=64, float32): {time.time() - t0:.0f} s, trace {trace[:, 0]}")
    assert trace.shape == (10, 2) and y.shape == (batch, (frames - 1) * hop)
    items = [0, 63]
    pair = np.ascontiguousarray(mag[items])
    y2 = M.griffin_lim(t(pair), max_iter=100, alpha=0.3, tol=0, verbose=True, eva_iter=10, metric="sc", **kw)
    trace_pair = trace_of(_Bar.last, "sc")
    same = [bool(torch.equal(y2[i], y[it])) for i, it in enumerate(items)]
    print(f"  items {items} alone (B=2) equal their rows of the B=64 run bit for bit: {same}")
    # float64 run of the two items from the float32 phase_init (the reference's float64 phase_init would start elsewhere)
    init = M.phase_init(t(pair), **kw)
    y64 = M.griffin_lim(init.to(torch.complex128), max_iter=100, alpha=0.3, tol=0, verbose=True, eva_iter=10, metric="sc",
                        hop_length=hop, window=t(win.astype(np.float64)))
    trace64_pair = trace_of(_Bar.last, "sc")
    # The reference's metric is `20 (log10 ||out - target|| - log10 ||target||)` with torch's float32 `norm` (metrics.py:14): over
    # the 6.7e7 elements of this batch that norm accumulates in float32 and is off by 4e-3 (relative) for ||target|| alone, so the SC
    # column of `trace` is only good to ~1e-3; its loss column (`F.mse_loss`, a cascade sum) is good to 1e-7.  The spectral
    # convergence the reference's iterates really have follows from the loss and the exact ||target||: stored as `sc_db_from_loss`
    # (for the two-item runs the two agree to 1e-4 dB).
    tnorm_exact = float(np.sqrt((mag.astype(np.float64) ** 2).sum()))
    tnorm_torch = float(t(mag).norm())
    sc_from_loss = 20.0 * np.log10(np.sqrt(trace[:, 1] * mag.size) / tnorm_exact)
    print(f"  ||target||: torch float32 norm {tnorm_torch:.4f}, exact {tnorm_exact:.4f} ({tnorm_torch / tnorm_exact - 1:+.2e}); "
          f"SC from the loss trace {sc_from_loss[-1]:.5f} dB vs reported {trace[-1, 0]:.5f} dB")
    out = {"window": win, "hop": np.array(hop), "items": np.array(items), "seed": np.array(1234),
           "target_norm_exact": np.array(tnorm_exact), "target_norm_torch_f32": np.array(tnorm_torch),
           "sc_db_from_loss": sc_from_loss,
           "mag_checksum": np.array([float(mag.astype(np.float64).sum()), float(mag[0, 5, 7]), float(mag[63, 1024, 1023])]),
           "trace": trace, "trace_pair": trace_pair, "trace64_pair": trace64_pair,
           "rows_equal_pair_run": np.array(same)}
    for i, it in enumerate(items):
        a, b = y[it].double().numpy(), y64[i].numpy()
        seg = np.linalg.norm((a - b).reshape(-1, hop), axis=1) / (np.linalg.norm(b.reshape(-1, hop), axis=1) + 1e-30)
        out[f"wave_{it}"] = y[it].numpy()
        out[f"segerr_{it}"] = seg.astype(np.float32)
        out[f"segnorm64_{it}"] = np.linalg.norm(b.reshape(-1, hop), axis=1).astype(np.float32)
        out[f"noise_{it}"] = np.array(np.linalg.norm(a - b) / np.linalg.norm(b))
        print(f"  item {it}: float32 vs float64 rel-L2 {float(out[f'noise_{it}']):.2e}, median segment {np.median(seg):.2e}, "
              f"segments above 1e-3: {(seg > 1e-3).mean():.3f}")
    save("g16b_c2_headline", **out)


G17_CASES = [("512_128_la3", 512, 128, 3, True, 0.5), ("1024_256_la3_asym", 1024, 256, 3, True, 0.99),
             ("1024_128_la_default", 1024, 128, -1, True, 0.99), ("2048_512_la3_alpha0", 2048, 512, 3, True, 0.0),
             ("2048_512_la2_sym", 2048, 512, 2, False, 0.5)]


def g17_autograd_rtisi_sizes():
    """Gradients of the reference's RTISI_LA at the frame sizes its adjoint kernel launches differently for (256 threads below
    n_fft 1024, 512 from 1024, 1024 from 2048): float64, the magnitudes of tests/_gla_torch.py::wellcond's STFT (computed in float32,
    so float32-representable), batch 2, 16 frames, 2 inner iterations.  One file per case (each below 1 MiB): the magnitudes and the
    weights of the loss sum(w y) as float32, y and the gradient as float64, and the reference's own sensitivity - the relative change
    of its gradient when every magnitude is multiplied by 1 +- 2^-52 with random signs (rng 52), the yardstick of the test's gate."""
    sys.path.insert(0, os.path.dirname(HERE))
    import _gla_torch as gt
    for tag, n_fft, hop, la, asym, alpha in G17_CASES:
        kw = dict(hop_length=hop, window=hann(n_fft, np.float32))
        mag = np.abs(gt.wellcond_spec(2, n_fft, 16, kw, 170 + n_fft + hop)[0]).astype(np.float32)
        kw64 = dict(hop_length=hop, window=t(hann(n_fft, np.float64)))

        def run(m):
            spec = t(m).requires_grad_(True)
            y = M.RTISI_LA(spec, look_ahead=la, asymmetric_window=asym, max_iter=2, alpha=alpha, verbose=False, **kw64)
            return spec, y

        spec, y = run(mag.astype(np.float64))
        wv = np.random.default_rng(17).standard_normal(tuple(y.shape)).astype(np.float32)
        (y * t(wv.astype(np.float64))).sum().backward()
        spec1, y1 = run(gt.ulp_perturbed(mag.astype(np.float64), np.random.default_rng(52)))
        (y1 * t(wv.astype(np.float64))).sum().backward()
        sens = float((spec1.grad - spec.grad).norm() / spec.grad.norm())
        print(f"  g17 {tag}: sens64 {sens:.2e}")
        save(f"g17_autograd_rtisi_sizes_{tag}", mag=mag, w=wv, y=y.detach().numpy(), grad=spec.grad.numpy(), sens64=np.array(sens),
             meta=np.array(f"{n_fft}|{hop}|{la}|{int(asym)}|{alpha}|2"))


if __name__ == "__main__":
    which = sys.argv[1:] or ["g0", "g1", "g2", "g3", "g4", "g5", "g6", "g7", "g8", "g9", "g10", "g11", "g12", "g13", "g14", "g15", "g16", "g17"]
    table = dict(g0=g0_stft, g1=g1_phase_init, g2=g2_gla, g3=g3_sweep, g4=g4_admm, g5=g5_rtisi,
                 g6=g6_lbfgs, g7=g7_metrics, g8=g8_f64, g9=g9_lbfgs_rosen, g10=g10_autograd, g11=g11_autograd_admm, g12=g12_autograd_rtisi, g13=g13_wave_level_shapes,
                 g14=g14_wellcond, g15=g15_wellcond_1024, g16=g16_headline_2048, g17=g17_autograd_rtisi_sizes)
    for w in which:
        table[w]()
