"""Exact references for load_data's preparation kernels (include/ppfit.h:
ppf_remove_baseline, ppf_profile_snr, ppf_tscrunch), written so that they
share nothing with the kernels.

Every fp64 number is a dyadic rational m 2^e, so an array is held as Python
integers over one common power of two (``_ints``).  Sums, products, window
sums and running sums of such integers are exact in any order: no summation
order exists here, let alone the device's.  A result is rounded to fp64 once,
by Python's correctly rounded int / int division or Fraction -> float; the
one exception is the square root in the S/N, whose error is stated there.

Conventions the references restate from the header, not from the kernels:
windows are circular, the smallest sum wins, the first start wins a tie, a
window whose sum is NaN never wins, and with no ordered sum the window starts
at 0.  Infinities are not supported.

The ``*_bound`` functions bound |device - exact| from the summation bound
(n - 1) u sum|terms| (u = 2^-53, any order of n terms) applied to each sum a
kernel forms, plus one u per further rounded operation.  They hold first-order
terms only (u^2 terms are kept where a large factor multiplies them) and no
measured constant.
"""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53


def _ints(a):
    """(object array of ints I, exponent e) with a == I * 2**e exactly."""
    a = np.asarray(a, dtype=np.float64)
    if not np.all(np.isfinite(a)):
        raise ValueError("finite values only")
    m, e = np.frexp(a)
    mi = (m * 2.0 ** 53).astype(np.int64).astype(object)  # exact: |m| < 1, 53 bits
    nz = a != 0.0
    emin = int(e[nz].min()) if nz.any() else 0
    sh = np.where(nz, e - emin, 0).astype(np.int64).astype(object)
    return mi * (2 ** sh), emin - 53


def _ratio(num, den):
    """float(num / den) for integers, rounded once; 0 / 0 -> 0."""
    return float(Fraction(int(num), int(den))) if den else 0.0


def _window(T, nan, width):
    """Start (first on ties, NaN windows never win, 0 when none is ordered),
    the gap between the smallest and the second-smallest ordered window sum
    (None with fewer than two ordered windows) of integers T with NaN mask."""
    n = len(T)
    ext = list(T) + list(T[:width])
    bad = list(nan) + list(nan[:width])
    P, B = [0], [0]
    for v, b in zip(ext, bad):
        P.append(P[-1] + (0 if b else v))
        B.append(B[-1] + (1 if b else 0))
    sums = [(P[j + width] - P[j], j) for j in range(n) if B[j + width] == B[j]]
    if not sums:
        return 0, None
    sums.sort()  # by sum, then by start: sums[0] is the first smallest
    gap = sums[1][0] - sums[0][0] if len(sums) > 1 else None
    return sums[0][1], gap


def baseline_window(t, width):
    """(start, margin) of the circular window of `width` bins of smallest sum
    of the fp64 vector t: first start on ties; margin = (second-smallest sum -
    smallest sum) / sum|t| (0.0 on an exact tie; nan when t holds a NaN)."""
    t = np.asarray(t, dtype=np.float64)
    nan = np.isnan(t)
    T, _ = _ints(np.where(nan, 0.0, t))
    j0, gap = _window(list(T), list(nan), int(width))
    if nan.any() or gap is None:
        return j0, (float("nan") if nan.any() else float("inf"))
    return j0, _ratio(gap, sum(abs(v) for v in T))


def remove_baseline_exact(subints, weights, ntot, width):
    """ppf_remove_baseline of include/ppfit.h, exactly: (out, starts, margins).

    Per subint the total t[j] = sum_{n: w != 0} w[n] sum_{p < ntot} d[p][n][j]
    is formed as integers (products and sums exact), its window found on the
    exact sums, and out = row - (exact window mean of the row), rounded once.
    margins[s] = (second-smallest - smallest window sum) / sum_j sum_n sum_p
    |w d| (at least sum|t|, so no larger than the margin over sum|t|).  A row
    that holds a NaN comes out all NaN; a NaN in a weighted channel of the
    total makes the windows over it NaN (module docstring), margin nan."""
    d = np.array(subints, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    nsub, npol, nchan, nbin = d.shape
    width = int(width)
    out = np.empty_like(d)
    starts = np.zeros(nsub, dtype=int)
    margins = np.zeros(nsub)
    for s in range(nsub):
        on = np.flatnonzero(w[s] != 0.0)
        tot = d[s, :ntot][:, on]  # [ntot, non, nbin]
        nan = np.isnan(tot).any(axis=(0, 1)) if len(on) else np.zeros(nbin, bool)
        if len(on):
            D, _ = _ints(np.where(np.isnan(tot), 0.0, tot))
            W, _ = _ints(w[s][on])
            T = (W[None, :, None] * D).sum(axis=(0, 1))
            A = (abs(W)[None, :, None] * abs(D)).sum()
        else:
            T, A = np.zeros(nbin, dtype=object), 0
        j0, gap = _window(list(T), list(nan), width)
        starts[s] = j0
        margins[s] = float("nan") if nan.any() else (
            float("inf") if gap is None else (_ratio(gap, A) if A else 0.0))
        idx = (j0 + np.arange(width)) % nbin
        for p in range(npol):
            for n in range(nchan):
                row = d[s, p, n]
                if np.isnan(row[idx]).any():
                    out[s, p, n] = np.nan
                    continue
                ok = ~np.isnan(row)
                R, e = _ints(np.where(ok, row, 0.0))
                S = int(R[idx].sum())
                num = R * width - S  # (row - mean) * width, exact
                val = np.array([x / width for x in num], dtype=np.float64)  # rounded once
                out[s, p, n] = np.where(ok, np.ldexp(val, e), np.nan)
    return out, starts, margins


def remove_baseline_error(got, subints, starts, width):
    """max_j |got - exact| per row, [nsub, npol, nchan]: the difference to the
    unrounded exact result, itself formed exactly and rounded once (so the
    reference adds no rounding of its own to what the bound must cover).
    Finite rows only."""
    g = np.asarray(got, dtype=np.float64)
    d = np.asarray(subints, dtype=np.float64)
    nsub, npol, nchan, nbin = d.shape
    err = np.zeros((nsub, npol, nchan))
    for s in range(nsub):
        idx = (int(starts[s]) + np.arange(width)) % nbin
        for p in range(npol):
            for n in range(nchan):
                both, e = _ints(np.concatenate([d[s, p, n], g[s, p, n]]))
                R, G = both[:nbin], both[nbin:]
                S = int(R[idx].sum())
                worst = max(abs(int(x)) for x in (G * width - (R * width - S)))
                err[s, p, n] = math.ldexp(worst / width, e)
    return err


def remove_baseline_bound(subints, width):
    """Bound on |device - exact| per row of ppf_remove_baseline,
    [nsub, npol, nchan]: (width + 3) u max|row|.

    The kernel forms m = (sum of `width` bins) * (1 / width) and out = row - m.
    The sum, in any order: (width - 1) u sum|bins| <= (width - 1) u width M
    with M = max|row|; 1 / width is rounded (u) and so is the product (u), so
    |dm| <= (width + 1) u M.  The subtraction rounds once more: u |out| <= u
    (|row| + |m|) <= 2 u M.  Total (width + 3) u M."""
    d = np.asarray(subints, dtype=np.float64)
    return (int(width) + 3) * U * np.abs(d).max(axis=-1)


def tscrunch_exact(subints, weights):
    """ppf_tscrunch of include/ppfit.h, exactly: (out [npol, nchan, nbin],
    wsum [nchan]).  out = sum_s w d / sum_s w over the subints with w != 0 (a
    sample under zero weight is never read, so it may be NaN), 0 where every
    weight is 0; numerator and denominator are exact integers and the
    quotient is rounded once.  wsum is the exact sum, rounded once."""
    d = np.asarray(subints, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    nsub, npol, nchan, nbin = d.shape
    on = w != 0.0
    D, e = _ints(np.where(on[:, None, :, None], d, 0.0))
    W, ew = _ints(w)
    num = (W[:, None, :, None] * D).sum(axis=0)  # [npol, nchan, nbin], scale 2^(e + ew)
    den = W.sum(axis=0)  # [nchan], scale 2^ew
    out = np.zeros((npol, nchan, nbin))
    for n in range(nchan):
        if den[n]:
            q = np.array([x / den[n] for x in num[:, n].ravel()], dtype=np.float64)
            out[:, n] = np.ldexp(q, e).reshape(npol, nbin)
    wsum = np.array([float(Fraction(int(x)) * Fraction(2) ** ew) for x in den])
    return out, wsum


def tscrunch_bound(subints, weights):
    """Bound on |device - tscrunch_exact| per output sample, [npol, nchan,
    nbin]: (nsub + 2) u sum_s|w d| / sum_s w, for weights whose running fp64
    sum is exact (float32-valued weights of like magnitude, as PSRFITS stores
    DAT_WTS: the caller checks wsum against the exact sum bitwise).

    The kernel forms acc = sum_s w d with one fused multiply-add per subint:
    nsub roundings, nsub u sum|w d|.  The quotient acc / wsum is rounded (u)
    and so is the reference's quotient (u).  Zero-weight samples are left out
    of sum|w d| (they are never read)."""
    d = np.asarray(subints, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    nsub = d.shape[0]
    on = (w != 0.0)[:, None, :, None]
    a = np.abs(np.where(on, d, 0.0) * w[:, None, :, None]).sum(axis=0)
    ws = np.abs(w).sum(axis=0)[None, :, None]
    return (nsub + 2) * U * a / np.where(ws > 0, ws, 1.0)


def profile_snr_exact(rows, width, thr):
    """ppf_profile_snr of include/ppfit.h, exactly.  Returns a dict of arrays
    over the rows: snr, window, rise, fall (-1 where there is none),
    window_margin, rise_margin, fall_margin, and bound (below).

    With X the row as integers and S the exact window sum, y_i = x - m is held
    as Y_i = X W - S (y = Y / W), its running sum c and total C are exact
    integers, and the edges are the first i with c_i q >= p C for thr = p / q
    (the fp64 value of thr) and for 1 - thr.  snr^2 = E^2 (W - 1) / (n sum_win
    Y^2) with E = sum_{rise..fall} Y is an exact rational; it is rounded once
    and its square root once more (relative error below 2 u).

    window_margin = (second-smallest - smallest window sum) / sum|x|;
    rise_margin = min_i |c_i - thr C| / sum|y|, fall_margin = min_i |c_i -
    (1 - thr) C| / sum|y|, over every i.  At thr = 0 the fall margin is 0 for
    every row: the window's own y sum to 0, so the running sum equals C
    exactly at the last bin before the window and again at the last bin.
    Threshold 0 is therefore only meaningful where the device's sums are
    exact too (integer-valued rows with an integer window mean).

    A row with a NaN bin: the window by the NaN rule, snr 0 (C is NaN), no
    edges, margins nan.

    bound: on |device - exact| of the snr, first order, from the sums the
    kernel forms (W = width, all quantities of the exact row):
      m:  a sum of W bins then a division: |dm| <= ((W - 1) SA / W + |m|) u
          <= u SA, SA = sum_win|x|.
      v:  d_k = fl(x_k - m - dm); sum_win d_k^2 = sum d^2 + W dm^2 exactly
          (sum_win d = 0: the error of the mean enters in second order, kept
          because SA may dwarf d), each d_k carries u |d_k| (2 u d_k^2 on the
          square, and 2 dm u |d_k| across), the square u, the sum of W squares
          (W - 1) u, the division by W - 1 u:
          dv / v <= (W dm^2 + 2 dm u sum|d| + (W + 3) u sum d^2) / sum d^2;
          sqrt(v) then carries dv / (2 v) + u.
      E:  the kernel takes c_fall - c_rise + y_rise from running sums, each
          built as segment totals (sums of `per` = ceil(nbin / 64) bins: per -
          1 additions over their own bins), at most 63 additions of totals,
          then at most `per` further bins: c_i carries (2 per + 62) u SY_i,
          SY_i = sum_{k <= i}|y_k| (every partial sum is at most SY_i); the
          last two additions u (|c_fall - c_rise| + |E|); the bins rise..fall
          (n of them) carry dm each and u |y| (the bins before rise enter both
          running sums as the same numbers):
          dE <= n dm + u (sum_{rise..fall}|y| + (2 per + 62) (SY_fall +
          SY_rise) + |c_fall - c_rise| + |E|).
      snr = E / sqrt(n) / sqrt(v): two square roots and two divisions, 4 u, and
          the reference's own 2 u:
          bound = |snr| (dE / |E| + dv / (2 v) + 6 u)."""
    x = np.asarray(rows, dtype=np.float64)
    x = x.reshape(-1, x.shape[-1])
    nrow, nbin = x.shape
    W = int(width)
    tf = Fraction(float(thr))
    cuts = (tf, 1 - tf)
    per = -(-nbin // 64)
    res = {k: np.zeros(nrow) for k in ("snr", "window_margin", "rise_margin", "fall_margin",
                                       "bound")}
    res.update({k: np.full(nrow, -1, dtype=int) for k in ("window", "rise", "fall")})
    for r in range(nrow):
        nan = np.isnan(x[r])
        X, _ = _ints(np.where(nan, 0.0, x[r]))
        X = [int(v) for v in X]
        j0, gap = _window(X, list(nan), W)
        res["window"][r] = j0
        if nan.any():
            for k in ("window_margin", "rise_margin", "fall_margin", "bound"):
                res[k][r] = np.nan
            continue
        SX = sum(abs(v) for v in X)
        res["window_margin"][r] = float("inf") if gap is None else (_ratio(gap, SX) if SX else 0.0)
        win = [X[(j0 + i) % nbin] for i in range(W)]
        S = sum(win)
        Y = [X[(j0 + W + i) % nbin] * W - S for i in range(nbin)]
        c, run = [], 0
        for v in Y:
            run += v
            c.append(run)
        C = run
        SY = sum(abs(v) for v in Y)
        edges, margins = [], []
        for t, cut in enumerate(cuts):
            p, q = cut.numerator, cut.denominator
            gaps = [ci * q - p * C for ci in c]
            first = next((i for i, g in enumerate(gaps) if g >= 0), -1)
            edges.append(first)
            margins.append(_ratio(min(abs(g) for g in gaps), q * SY) if SY else 0.0)
        rise, fall = edges
        res["rise"][r], res["fall"][r] = rise, fall
        res["rise_margin"][r], res["fall_margin"][r] = margins
        D2 = sum((v * W - S) ** 2 for v in win)  # sum_win (x - m)^2 W^2
        if not (C > 0 and D2 > 0 and W > 1 and rise >= 0 and fall >= rise):
            continue  # snr 0, bound 0: the device must give exactly 0
        n = fall - rise + 1
        E = sum(Y[rise:fall + 1])
        snr = math.copysign(math.sqrt(float(Fraction(E * E * (W - 1), n * D2))), E)
        res["snr"][r] = snr
        # the bound, in the row's own units (x = X 2^e: the scale cancels)
        SA = sum(abs(v) for v in win)
        dm = U * SA  # units of X
        sd = sum(abs(v * W - S) for v in win) / W  # sum|d|
        sd2 = D2 / (W * W)  # sum d^2
        rv = (W * dm * dm + 2.0 * dm * U * sd + (W + 3) * U * sd2) / sd2
        ay = [abs(v) for v in Y]
        sums = (2 * per + 62) * (sum(ay[:fall + 1]) + sum(ay[:rise + 1]))
        last = abs(c[fall] - c[rise]) + abs(E)
        dE = n * dm + U * ((sum(ay[rise:fall + 1]) + sums + last) / W)
        res["bound"][r] = abs(snr) * (dE / (abs(E) / W) + 0.5 * rv + 6 * U) if E else 0.0
    return res
