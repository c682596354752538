"""rtpghi in NumPy, twice: `definition` is the package's definition as it is written (the two clamp recurrences run sequentially,
the phases follow the parent codes), `heap` is a literal RTPGHI with one look-ahead frame on `heapq` (Prusa & Sondergaard 2016,
algorithm 1 with the centred time difference), kept only to show that the definition is the heap's result.  Neither is taken from
the reference project, which has no PGHI.

Both return `(phase, parents)`: the unwrapped phase (F, T) in `real` and the int8 codes, 0 time direction, 1 from bin m - 1, 2 from
bin m + 1, 3 below the floor.  `real` is the dtype of every logarithm, gradient and sum (np.float64 is the definition;
np.longdouble measures its rounding noise); the decisions compare the float64 inputs and do not depend on it."""
import heapq

import numpy as np

HANN_GAMMA = 0.25645


def gradients(s, n_fft, hop, gamma, tol=1e-6, real=np.float64):
    """(live, wt, wf) of the definition for one item `s` (F, T); wt and wf are None for an item with no live bin."""
    s = np.asarray(s, np.float64)
    F, T = s.shape
    assert F == n_fft // 2 + 1 and n_fft % 2 == 0 and F >= 2
    floor = tol * max(0.0, float(s.max()))
    live = (s > 0) & (s >= floor)
    if not live.any():
        return live, None, None
    ell = np.log(np.maximum(s, floor).astype(real))
    ext = np.concatenate([ell[1:2], ell, ell[F - 2:F - 1]], 0)
    m = np.arange(F, dtype=np.int64)
    base = (real(2.0) * real(np.pi) / real(n_fft)) * ((hop * m) % n_fft).astype(real)
    wt = base[:, None] + (real(hop) * real(n_fft) / real(gamma)) * ((ext[2:] - ext[:-2]) / real(2.0))
    D = np.zeros((F, T), real)
    if T > 1:
        D[:, 1:-1] = (ell[:, 2:] - ell[:, :-2]) / real(2.0)
        D[:, 0] = ell[:, 1] - ell[:, 0]
        D[:, -1] = ell[:, -1] - ell[:, -2]
    wf = real(np.pi) - (real(gamma) / (real(hop) * real(n_fft))) * D
    return live, wt, wf


def _seed(s, live):
    """p of frame 0: -inf but for the lowest-index maximum of s[:, 0], +inf if that bin is live"""
    p = np.full(s.shape[0], -np.inf)
    k = int(np.argmax(s[:, 0]))
    if live[k, 0]:
        p[k] = np.inf
    return p


def definition(s, n_fft, hop, gamma, tol=1e-6, real=np.float64):
    s = np.asarray(s, np.float64)
    F, T = s.shape
    live, wt, wf = gradients(s, n_fft, hop, gamma, tol, real)
    phase = np.zeros((F, T), real)
    parents = np.full((F, T), 3, np.int8)
    if wt is None:
        return phase, parents
    two = real(2.0)
    for n in range(T):
        c = np.where(live[:, n], s[:, n], -np.inf)
        p = _seed(s, live) if n == 0 else np.where(live[:, n - 1], s[:, n - 1], -np.inf)
        Lf = np.full(F, -np.inf)
        for m in range(1, F):
            Lf[m] = min(c[m - 1], max(p[m - 1], Lf[m - 1]))
        Rg = np.full(F, -np.inf)
        for m in range(F - 2, -1, -1):
            Rg[m] = min(c[m + 1], max(p[m + 1], Rg[m + 1]))
        code = np.full(F, 3, np.int8)
        for m in range(F):
            if live[m, n]:
                b = max(p[m], Lf[m], Rg[m])
                code[m] = 0 if p[m] >= b else 1 if Lf[m] >= b else 2
        parents[:, n] = code
        for m in range(F):
            if code[m] == 0 and n > 0:
                phase[m, n] = phase[m, n - 1] + (wt[m, n - 1] + wt[m, n]) / two
        for m in range(F - 2, -1, -1):                        # chains of code 2 hang off a root to their right
            if code[m] == 2:
                phase[m, n] = phase[m + 1, n] - (wf[m + 1, n] + wf[m, n]) / two
        for m in range(1, F):                                 # chains of code 1 off a code-0 or code-2 root to their left
            if code[m] == 1:
                phase[m, n] = phase[m - 1, n] + (wf[m - 1, n] + wf[m, n]) / two
    return phase, parents


def heap(s, n_fft, hop, gamma, tol=1e-6, real=np.float64):
    """RTPGHI as published: per frame a max-heap that starts with the live bins of frame n - 1 (frame 0: with its largest bin, phase
    0); a popped bin of frame n - 1 sets the bin above it in time, a popped bin of frame n sets its unset neighbours in frequency,
    and every bin that is set is pushed with its own magnitude.  A live bin the heap never reaches starts from the phase 0 of the
    bin before it.  Among equal keys Python's tuple order decides, which is why the definition fixes its own tie rule."""
    s = np.asarray(s, np.float64)
    F, T = s.shape
    live, wt, wf = gradients(s, n_fft, hop, gamma, tol, real)
    phase = np.zeros((F, T), real)
    parents = np.full((F, T), 3, np.int8)
    if wt is None:
        return phase, parents
    two = real(2.0)
    for n in range(T):
        done = np.zeros(F, bool)
        h = []
        if n == 0:
            k = int(np.argmax(s[:, 0]))
            if live[k, 0]:
                parents[k, 0], done[k] = 0, True
                heapq.heappush(h, (-s[k, 0], k, 1))
        else:
            for m in range(F):
                if live[m, n - 1]:
                    heapq.heappush(h, (-s[m, n - 1], m, 0))
        while h:
            _, m, cur = heapq.heappop(h)
            if not cur:
                if live[m, n] and not done[m]:
                    phase[m, n] = phase[m, n - 1] + (wt[m, n - 1] + wt[m, n]) / two
                    parents[m, n], done[m] = 0, True
                    heapq.heappush(h, (-s[m, n], m, 1))
                continue
            if m + 1 < F and live[m + 1, n] and not done[m + 1]:
                phase[m + 1, n] = phase[m, n] + (wf[m, n] + wf[m + 1, n]) / two
                parents[m + 1, n], done[m + 1] = 1, True
                heapq.heappush(h, (-s[m + 1, n], m + 1, 1))
            if m - 1 >= 0 and live[m - 1, n] and not done[m - 1]:
                phase[m - 1, n] = phase[m, n] - (wf[m, n] + wf[m - 1, n]) / two
                parents[m - 1, n], done[m - 1] = 2, True
                heapq.heappush(h, (-s[m - 1, n], m - 1, 1))
        for m in range(F):
            if live[m, n] and not done[m]:
                parents[m, n] = 0
                if n > 0:
                    phase[m, n] = phase[m, n - 1] + (wt[m, n - 1] + wt[m, n]) / two
    return phase, parents


def random_magnitudes(F, T, seed, batch=None, zeros=0.1):
    """Seeded magnitudes: per item the F T points of a geometric grid from 1e-7 to 1 in seeded order (neighbours on the grid differ
    by a factor of at least 1.003, so the values stay distinct in float32; those under 1e-6 fall below the default floor), a
    fraction of them set to exact zero, and for a batch a different maximum per item (0.1, 1, 10, ...)."""
    rng = np.random.default_rng(seed)
    items = []
    for b in range(1 if batch is None else batch):
        grid = np.exp(np.linspace(np.log(1e-7), 0.0, F * T))
        s = grid[rng.permutation(F * T)].reshape(F, T)
        s[rng.random((F, T)) < zeros] = 0.0
        items.append(s * 10.0 ** (b - 1 if batch is not None else 0))
    return items[0] if batch is None else np.stack(items)


def assert_distinct(s):
    """all non-zero magnitudes of one item differ: a tie is the one place where heap and definition may part"""
    v = np.asarray(s)[np.asarray(s) > 0].ravel()
    assert np.unique(v).size == v.size


def wrapped(d):
    """a phase difference wrapped to [-pi, pi), in the dtype it comes in"""
    d = np.asarray(d)
    two_pi = d.dtype.type(2.0) * d.dtype.type(np.pi)
    return d - two_pi * np.round(d / two_pi)
