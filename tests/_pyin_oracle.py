"""pYIN (Mauch & Dixon 2014, as librosa.pyin states it) in NumPy, float64, on this package's d': the definition of
spectrogram_inversion_amd/pitch.py written out, what the GPU tests compare against.  `viterbi` is the dense decode on the literal
2P x 2P matrix; `viterbi_banded` is the kernel's arithmetic restated (tables, folded Z, the floor through the group maximum)."""
import math

import numpy as np

import _yin_oracle as yo

TINY = float(np.finfo(np.float64).tiny)


# ---- the threshold prior

def beta_cdf(x, a, b):
    """I_x(a, b) for integer a, b: the binomial sum over j = a ... n, n = a + b - 1"""
    n = a + b - 1
    return sum(math.comb(n, j) * x ** j * (1.0 - x) ** (n - j) for j in range(a, n + 1))


def beta_tail(x, a, b):
    """1 - I_x(a, b): the other part of the same binomial sum, j = 0 ... a - 1"""
    n = a + b - 1
    return sum(math.comb(n, j) * x ** j * (1.0 - x) ** (n - j) for j in range(a))


def prior(n_thresholds=100, a=2, b=18):
    """w_k = I_{s_k} - I_{s_{k-1}}, k = 1 ... K, formed from the tails so that the small weights near s = 1 keep their digits"""
    q = [beta_tail(k / n_thresholds, a, b) for k in range(n_thresholds + 1)]
    return np.array([q[k - 1] - q[k] for k in range(1, n_thresholds + 1)])


def boltzmann(lam, n):
    """(boltz[0 ... n - 1], inv[0 ... n]): (1 - e^-lam) e^(-lam r) and 1 / (1 - e^(-lam c)), inv[0] = 0"""
    boltz = (1.0 - math.exp(-lam)) * np.exp(-lam * np.arange(n, dtype=np.float64))
    inv = np.zeros(n + 1)
    inv[1:] = 1.0 / (1.0 - np.exp(-lam * np.arange(1, n + 1, dtype=np.float64)))
    return boltz, inv


# ---- the observation stage

def n_bins(fmin, fmax, resolution=0.1):
    bps = math.ceil(1.0 / resolution)
    return math.floor(12 * bps * math.log2(fmax / fmin)) + 1


def troughs(row, tau_min, tau_max):
    """the lags of the range with d'(tau) < d'(tau - 1) and d'(tau) <= d'(tau + 1), compared in the row's own dtype"""
    row = np.asarray(row)
    assert 1 <= tau_min < tau_max <= row.shape[-1] - 2
    t = np.arange(tau_min, tau_max + 1)
    return t[(row[t] < row[t - 1]) & (row[t] <= row[t + 1])]


def candidates(row, tau_min, tau_max, w, lam=2.0, q=0.01):
    """(lags, p): the troughs of one frame's d' and their probabilities, operation by operation as the kernel forms them"""
    taus = troughs(row, tau_min, tau_max)
    p = np.zeros(len(taus))
    if len(taus) == 0:
        return taus, p
    d = np.asarray(row)[taus].astype(np.float64)
    k_thr = len(w)
    boltz, inv = boltzmann(lam, len(taus))
    for k in range(1, k_thr + 1):
        hit = d < k / k_thr
        n = int(hit.sum())
        if n:
            rank = np.cumsum(hit) - 1
            p[hit] = p[hit] + (w[k - 1] * inv[n]) * boltz[rank[hit]]
    g = int(np.argmin(d))
    m = sum(1 for k in range(1, k_thr + 1) if d[g] >= k / k_thr)
    cum = np.concatenate([[0.0], np.cumsum(w)])
    p[g] = p[g] + q * cum[m]
    return taus, p


def raw_bins(row, taus, sample_rate, fmin, bps):
    """the unrounded bin 12 bps log2(sample_rate / period / fmin) of each lag, period = tau + shift"""
    period = np.array([yo.refine(np.asarray(row), int(t))[0] for t in taus], dtype=np.float64)
    return 12 * bps * np.log2(sample_rate / period / fmin)


def observations(dp, sample_rate, fmin, fmax, tau_min, tau_max, w, lam=2.0, q=0.01, resolution=0.1):
    """(obs (T, P) float64, voiced_prob (T,) float64, raw): `raw` is the list of the unrounded bins of every candidate with p > 0"""
    dp = np.asarray(dp)
    bps = math.ceil(1.0 / resolution)
    n_pitch = n_bins(fmin, fmax, resolution)
    obs = np.zeros((dp.shape[0], n_pitch))
    raw_all = []
    for t, row in enumerate(dp):
        taus, p = candidates(row, tau_min, tau_max, w, lam, q)
        keep = p > 0
        taus, p = taus[keep], p[keep]
        raw = raw_bins(row, taus, sample_rate, fmin, bps)
        raw_all.append(raw)
        for b, v in zip(np.rint(raw), p):                    # rising lag: the last write stands
            b = max(int(b), 0)
            if b <= n_pitch - 1:
                obs[t, b] = v
    return obs, np.clip(obs.sum(axis=-1), 0.0, 1.0), raw_all


def bin_margin(raw_all):
    """the smallest distance of any candidate's unrounded bin from a half-integer"""
    m = math.inf
    for raw in raw_all:
        if len(raw):
            m = min(m, float(np.abs(raw - np.floor(raw) - 0.5).min()))
    return m


def collisions(raw_all, n_pitch):
    """how many candidates lost their bin to a larger lag"""
    lost = 0
    for raw in raw_all:
        b = np.maximum(np.rint(raw), 0)
        b = b[b <= n_pitch - 1]
        lost += len(b) - len(np.unique(b))
    return lost


# ---- the HMM

def band(n_pitch, half):
    """A (P, P): tri(j - i) / Z_i inside |j - i| <= half, 0 outside"""
    width = 2 * half + 1
    a = np.zeros((n_pitch, n_pitch))
    for i in range(n_pitch):
        j = np.arange(max(0, i - half), min(n_pitch, i + half + 1))
        tri = 1.0 - np.abs(j - i) / ((width + 1) / 2)
        a[i, j] = tri / tri.sum()
    return a


def transition(n_pitch, half, switch=0.01):
    return np.kron(np.array([[1.0 - switch, switch], [switch, 1.0 - switch]]), band(n_pitch, half))


def log_emission(obs, voiced_prob):
    """(T, 2P): log(p + tiny) of the voiced observations and of (1 - voiced_prob) / P on every unvoiced state"""
    obs = np.asarray(obs, dtype=np.float64)
    vp = np.asarray(voiced_prob, dtype=np.float64)
    n_pitch = obs.shape[-1]
    unv = np.repeat(((1.0 - vp) / n_pitch)[:, None], n_pitch, axis=1)
    return np.log(np.concatenate([obs, unv], axis=1) + TINY)


def log_init(n_pitch):
    return np.log(np.concatenate([np.zeros(n_pitch), np.full(n_pitch, 1.0 / n_pitch)]) + TINY)


def _second_gap(vals):
    """best minus second best down every column"""
    part = np.partition(vals, -2, axis=0)
    return part[-1] - part[-2]


def viterbi(obs, voiced_prob, half, switch=0.01, gaps=False):
    """The dense decode: (states (T,), score), and with gaps=True also (T,) the margin by which each state of the path was chosen:
    state T - 1 as the final arg-max over its runner-up, state t < T - 1 as the best predecessor of state t + 1 over the runner-up.
    Ties go to the lowest index."""
    log_b = log_emission(obs, voiced_prob)
    n_frames, n_states = log_b.shape
    log_a = np.log(transition(n_states // 2, half, switch) + TINY)
    delta = log_init(n_states // 2) + log_b[0]
    ptr = np.zeros((n_frames, n_states), dtype=np.int64)
    gap = np.zeros((n_frames, n_states))
    for t in range(1, n_frames):
        vals = delta[:, None] + log_a
        ptr[t] = np.argmax(vals, axis=0)
        if gaps:
            gap[t] = _second_gap(vals)
        delta = vals[ptr[t], np.arange(n_states)] + log_b[t]
    states = np.zeros(n_frames, dtype=np.int64)
    states[-1] = int(np.argmax(delta))
    for t in range(n_frames - 1, 0, -1):
        states[t - 1] = ptr[t, states[t]]
    score = float(delta[states[-1]])
    if not gaps:
        return states, score
    final = np.sort(delta)
    g = np.concatenate([gap[np.arange(1, n_frames), states[1:]], [final[-1] - final[-2]]])
    return states, score, g


def path_gap(obs, voiced_prob, half, switch=0.01):
    """(T,): the margin by which each state of the dense path was chosen (see `viterbi`)"""
    return viterbi(obs, voiced_prob, half, switch, gaps=True)[2]


def path_score(states, obs, voiced_prob, half, switch=0.01):
    """the log-probability of a state path under the dense model"""
    states = np.asarray(states, dtype=np.int64)
    log_b = log_emission(obs, voiced_prob)
    n_pitch = log_b.shape[1] // 2
    log_a = np.log(transition(n_pitch, half, switch) + TINY)
    t = np.arange(len(states))
    return float(log_init(n_pitch)[states[0]] + log_b[t, states].sum() + log_a[states[:-1], states[1:]].sum())


def decode_tables(n_pitch, half):
    """(log tri(0 ... half), -log Z_i)"""
    width = 2 * half + 1
    tri = 1.0 - np.arange(half + 1) / ((width + 1) / 2)
    z = np.array([tri[np.abs(np.arange(max(0, i - half), min(n_pitch, i + half + 1)) - i)].sum() for i in range(n_pitch)])
    return np.log(tri), -np.log(z)


def _take(best_v, best_i, v, i):
    better = (v > best_v) | ((v == best_v) & (i < best_i))
    return np.where(better, v, best_v), np.where(better, i, best_i)


def viterbi_banded(obs, voiced_prob, half, switch=0.01):
    """The kernel's arithmetic: a = delta - log Z, the banded max-plus with log tri for both groups in rising i with a strict
    comparison, stay and switch, and each group's maximum plus log tiny as the floor: (states, score)"""
    log_b = log_emission(obs, voiced_prob)
    n_frames, n_states = log_b.shape
    n_pitch = n_states // 2
    ltri, nlz = decode_tables(n_pitch, half)
    l_stay, l_switch, l_tiny = math.log(1.0 - switch + TINY), math.log(switch + TINY), math.log(TINY)
    delta = log_init(n_pitch) + log_b[0]
    ptr = np.zeros((n_frames, n_states), dtype=np.int64)
    j = np.arange(n_pitch)
    for t in range(1, n_frames):
        m, arg = [], []
        for g in range(2):
            a = np.full(n_pitch + 2 * half, -math.inf)
            a[half:half + n_pitch] = delta[g * n_pitch:(g + 1) * n_pitch] + nlz
            mv, iv = np.full(n_pitch, -math.inf), np.zeros(n_pitch, dtype=np.int64)
            for kk in range(2 * half + 1):
                c = a[j + kk] + ltri[abs(kk - half)]
                better = c > mv
                mv, iv = np.where(better, c, mv), np.where(better, kk, iv)
            m.append(mv)
            arg.append(iv + j - half + g * n_pitch)
        gi = [int(np.argmax(delta[:n_pitch])), n_pitch + int(np.argmax(delta[n_pitch:]))]
        new = np.empty(n_states)
        for g in range(2):                                   # the target group
            bv, bi = m[0] + (l_stay if g == 0 else l_switch), arg[0]
            bv, bi = _take(bv, bi, m[1] + (l_switch if g == 0 else l_stay), arg[1])
            for h in range(2):
                bv, bi = _take(bv, bi, np.full(n_pitch, delta[gi[h]] + l_tiny), np.full(n_pitch, gi[h]))
            ptr[t, g * n_pitch:(g + 1) * n_pitch] = bi
            new[g * n_pitch:(g + 1) * n_pitch] = bv + log_b[t, g * n_pitch:(g + 1) * n_pitch]
        delta = new
    states = np.zeros(n_frames, dtype=np.int64)
    states[-1] = int(np.argmax(delta))
    for t in range(n_frames - 1, 0, -1):
        states[t - 1] = ptr[t, states[t]]
    return states, float(delta[states[-1]])


def transition_width(sample_rate, hop, resolution=0.1, max_transition_rate=35.92):
    """(half, bps) of the band: m = round(rate 12 hop / sample_rate), width = m bps + 1"""
    bps = math.ceil(1.0 / resolution)
    width = round(max_transition_rate * 12 * hop / sample_rate) * bps + 1
    assert width % 2 == 1
    return (width - 1) // 2, bps


def decode(obs, voiced_prob, fmin, half, resolution=0.1, switch=0.01, fill_na=math.nan):
    """(f0, voiced_flag, states) of the dense decode"""
    states, _ = viterbi(obs, voiced_prob, half, switch)
    n_pitch = np.asarray(obs).shape[-1]
    bps = math.ceil(1.0 / resolution)
    voiced = states < n_pitch
    f0 = fmin * 2.0 ** ((states % n_pitch) / (12 * bps))
    return np.where(voiced, f0, fill_na), voiced, states
