"""Numpy restatement of the noise-floor fit, written from its definition
(include/ppfit.h, ppf_find_kc_rows and ppf_noise_fit_rows): the CPU yardstick
of tests/test_noise_fit_cpu.py, tests/test_gpu_noise_fit.py and
tools/time_noise_fit.py.

find_kc is a grid search: d = log10(pows), and over

    a_i  = i (a_hi - a_lo) / 19 + a_lo     a in [1/n, 1] (exp_dc), [1, n] (half_tri)
    b_i  = i (max d - min d) / 19
    dc_i = i (max d - min d) / 19 + min d

the smallest S(a, b, dc) = sum_k w_k (d_k - b f_a(k) - dc)^2 wins, the first
one in C order among equals and the first NaN before any number
(numpy.argmin).  `direct` evaluates S term by term; `factorised` from the six
sums per a that make S a quadratic in (b, dc), as the device does.
"""
import numpy as np

NS = 20
FLOOR = 0.005


def axis(lo, hi):
    """The 20 grid values of [lo, hi]: i * step + lo."""
    step = (hi - lo) / float(NS - 1)
    return np.arange(NS, dtype=np.float64) * step + lo


def a_axis(n, fn):
    return axis(1.0 / n, 1.0) if fn == "exp_dc" else axis(1.0, float(n))


def basis(a, n, fn):
    k = np.arange(n)
    if fn == "exp_dc":
        return np.exp(-a * k)
    fa = int(np.floor(a))
    f = np.zeros(n)
    m = min(fa, n)
    f[:m] = 1.0 - k[:m] / float(fa)
    return f


def objective_direct(d, w, fn):
    """S on the whole grid, [20, 20, 20] (ia, ib, idc)."""
    n = len(d)
    with np.errstate(all="ignore"):
        bs = axis(0.0, d.max() - d.min())
        dcs = axis(d.min(), d.max())
        out = np.empty((NS, NS, NS))
        for ia, a in enumerate(a_axis(n, fn)):
            f = basis(a, n, fn)
            for ib, b in enumerate(bs):
                r = d[None, :] - b * f[None, :] - dcs[:, None]
                out[ia, ib] = np.sum(w * r * r, axis=1)
    return out


def objective_factorised(d, w, fn):
    n = len(d)
    with np.errstate(all="ignore"):
        dmin, dmax = d.min(), d.max()
        step = (dmax - dmin) / float(NS - 1)
        g = np.arange(NS) * step
        dp = d - dmin
        sw, sd, sdd = np.sum(w * np.ones(n)), np.sum(w * dp), np.sum(w * dp * dp)
        q0 = sdd + g * (g * sw - 2.0 * sd)  # [idc]
        out = np.empty((NS, NS, NS))
        for ia, a in enumerate(a_axis(n, fn)):
            f = basis(a, n, fn)
            se, see, sde = np.sum(w * f), np.sum(w * f * f), np.sum(w * dp * f)
            b = g[:, None]
            out[ia] = q0[None, :] + b * (b * see + 2.0 * (g[None, :] * se - sde))
    return out


def kc_of(a, n, fn):
    if fn == "half_tri":
        return int(np.floor(a))
    hit = np.where(np.exp(-a * np.arange(n)) < FLOOR)[0]
    return int(hit.min()) if len(hit) else n - 1


def find_kc(pows, errs=1.0, fn="exp_dc", how="direct", full=False):
    """kc (and, with full, the flat grid index and the best S per a)."""
    pows = np.asarray(pows, dtype=np.float64)
    n = len(pows)
    with np.errstate(all="ignore"):
        d = np.log10(pows)
        w = np.broadcast_to(1.0 / np.asarray(errs, dtype=np.float64) ** 2, (n,))
        if not (np.isfinite(d).all() and np.isfinite(w).all()):
            idx = 0  # the objective is NaN (or inf everywhere) at index 0
            per_a = np.full(NS, np.nan)
        else:
            S = (objective_direct if how == "direct" else objective_factorised)(d, w, fn)
            idx = int(np.argmin(S))
            per_a = S.reshape(NS, -1).min(axis=1)
    kc = kc_of(a_axis(n, fn)[idx // (NS * NS)], n, fn)
    return (kc, idx, per_a) if full else kc


def power_spectrum(row):
    row = np.asarray(row, dtype=np.float64)
    X = np.fft.rfft(row)
    return (X.real ** 2 + X.imag ** 2) / len(row)


def noise_from_kc(pows, kc, fact=1.1):
    k_crit = fact * kc
    if k_crit >= len(pows):
        k_crit = min(int(0.99 * len(pows)), k_crit)
    return float(np.sqrt(np.mean(pows[int(k_crit):]))), int(k_crit)


def get_noise_fit(row, fact=1.1, how="direct"):
    pows = power_spectrum(row)
    return noise_from_kc(pows, find_kc(pows, how=how), fact)[0]


def get_noise_PS(row, frac=4):
    pows = power_spectrum(row)
    return float(np.sqrt(np.mean(pows[int((1 - 1.0 / frac) * len(pows)):])))


def separated(per_a, idx, tol=1e-9):
    """The winner is safe from rounding: the two smallest of the per-a minima
    differ by more than tol (relative), or they tie exactly on the b = 0
    plane, which is the same for every a (the lowest index wins)."""
    if not np.isfinite(per_a).all():
        return True  # the NaN rule decides, not a comparison
    s = np.sort(per_a)
    if s[1] == s[0] and (idx // NS) % NS == 0:
        return True
    return (s[1] - s[0]) > tol * abs(s[1])
