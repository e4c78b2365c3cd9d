"""Inputs shared by tests/test_archive_prep_cpu.py (which proves on the CPU
that every random input is well separated: window and crossing margins of at
least MARGIN, no row left out, and that the tie rows tie exactly) and
tests/test_gpu_archive_prep.py (which runs them on the device).  Everything
is generated from fixed seeds; nothing here touches a device."""
import numpy as np

DUTY = 0.15
MARGIN = 1e-9  # about 1000 nbin u at nbin 8192

# remove_baseline: (nbin, npol, ntot, nchan); nsub is 3.  npol * nchan is also
# no multiple of the four waves; 8192 stays at three rows.
BASELINE_CASES = [(5, 1, 1, 1), (13, 2, 2, 3), (14, 4, 2, 5), (63, 4, 1, 3), (64, 1, 1, 5),
                  (65, 2, 2, 1), (100, 4, 2, 3), (255, 4, 1, 5), (256, 2, 2, 3), (257, 1, 1, 3),
                  (1000, 4, 2, 5), (8192, 1, 1, 1)]

SNR_NBINS = [5, 13, 14, 63, 64, 65, 100, 1000, 4097, 8192]
# (nbin, threshold) on the random rows, and the seed of each.  0.1 runs at every
# nbin with seed 1000 + nbin, except at 4097, where that seed draws a pulse so
# weak that the error bound passes 1e-12 |snr| (ill-conditioned): 4000 + nbin.
# At 0.49 the edge sum is the difference of two running sums of about C / 2
# that differ by 2 % of C, so its bound grows with nbin: 1000 + nbin serves up
# to 100; at 1000 and at 2048 seed 14 meets the margins and the bound on all
# eight rows; at 4097 and 8192 none of the seeds 1 to 40 does (the smallest
# worst-row bound among them is 1.6e-12 and 2.4e-12 |snr|), nor 1000 + nbin to
# 8000 + nbin in steps of 1000, so 0.49 stops at 2048.  Threshold 0 runs on
# integer_snr_rows (see there).
SNR_SEEDS = {(n, 0.1): (4000 if n == 4097 else 1000) + n for n in SNR_NBINS}
SNR_SEEDS.update({(n, 0.49): 1000 + n for n in SNR_NBINS if n <= 100})
SNR_SEEDS.update({(1000, 0.49): 14, (2048, 0.49): 14})
SNR_CASES = list(SNR_SEEDS)
SNR_THRESHOLDS = [0.0, 0.1, 0.49]  # all three on integer_snr_rows, at every nbin

# tscrunch: (npol, nsub, nbin); nchan is 4
TSCRUNCH_CASES = [(1, 1, 100), (4, 1, 1), (1, 2, 8192), (4, 2, 100), (4, 37, 100), (1, 37, 1)]

# 400: width 60, so dips 64 bins apart stay apart (at 512 and 1000 they merge)
TIE_NBINS = [400, 512, 1000]
TIE_A = 37  # no multiple of 64: a lane in the middle of a wave


def width_of(nbin, duty=DUTY):
    return max(1, int(duty * nbin))


def _f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def baseline_case(nbin, npol, ntot, nchan):
    """(subints [3, npol, nchan, nbin], weights [3, nchan]) for
    remove_baseline.  Every row: an offset, unit noise and a pulse; the
    polarisations past ntot are noise about 0 (they must not enter the total).
    Subint 0: a bowl whose minimum sits on the seam between the last bin and
    bin 0, so the best window wraps.  Subint 1: every weight 0 (window 0, rows
    still de-meaned over it).  With ntot 2 the first polarisation alone has
    its minimum elsewhere.  Subint 2: with three channels or more, channel
    1 has weight 0 and carries an offset of 1e6 with a deep dip at phase 0.7
    that would take the window if it were counted.  Weights are float32-valued
    and not 1."""
    rng = np.random.default_rng(7000 + nbin)
    ph = (np.arange(nbin) + 0.5) / nbin
    d = rng.normal(0.0, 1.0, (3, npol, nchan, nbin))
    d[:, :ntot] += rng.uniform(-20.0, 40.0, (3, ntot, nchan, 1))
    for s, lo in enumerate((0.0, 0.35, 0.2)):  # phase of the bowl's minimum
        dist = np.abs(np.angle(np.exp(2j * np.pi * (ph - lo)))) / np.pi  # 0 at lo, 1 opposite
        amp = rng.uniform(5.0, 20.0, (ntot, nchan, 1))
        d[s, :ntot] += amp * dist ** 2
        d[s, :ntot] += amp * np.exp(-0.5 * ((ph - (lo + 0.5) % 1.0) / 0.03) ** 2)
        if ntot == 2:  # a decoy: a dip in the first polarisation that the second fills
            dip = 50.0 * np.exp(-0.5 * ((ph - (lo + 0.3) % 1.0) / 0.05) ** 2)
            d[s, 0] -= dip
            d[s, 1] += dip
    w = _f32(rng.uniform(0.5, 2.0, (3, nchan)))
    w[1] = 0.0
    if nchan >= 3:
        w[2, 1] = 0.0
        d[2, :, 1] += 1e6
        d[2, :, 1] -= 5e5 * np.exp(-0.5 * ((ph - 0.7) / 0.05) ** 2)
    return d, w


def tie_rows(nbin):
    """[(name, integer-valued row, expected window start)] at width_of(nbin):
    10 everywhere with dips of zeros, so every window sum is an exact integer
    in any order and ties are exact.  The wrapping dip starts at nbin - 10; its
    partner sits at 100 where the two stay apart (nbin 512), else at twice the
    width."""
    wd, a = width_of(nbin), TIE_A
    out = []

    def row(*dips):
        r = np.full(nbin, 10.0)
        for start, length in dips:
            r[(start + np.arange(length)) % nbin] = 0.0
        return r

    out.append(("constant", row(), 0))
    out.append(("adjacent", row((a, wd + 1)), a))
    out.append(("plus64", row((a, wd), (a + 64, wd)), a))
    out.append(("plus256", row((a, wd), (a + 256, wd)), a))
    b = 100 if wd - 10 < 100 else 2 * wd
    out.append(("wrap", row((nbin - 10, wd), (b, wd)), b))
    return out


def tie_subints(nbin):
    """The tie rows as the total of a two-channel, two-polarisation subint
    each: weights 1 and 2, ntot 2, every sample a small integer, so
    1 (A0 + B0) + 2 (A1 + B1) is the tie row exactly.  Returns (subints
    [5, 2, 2, nbin], weights [5, 2], expected starts)."""
    rng = np.random.default_rng(4242 + nbin)
    rows = tie_rows(nbin)
    d = rng.integers(-5, 6, (len(rows), 2, 2, nbin)).astype(np.float64)
    for s, (_, r, _) in enumerate(rows):
        d[s, 0, 0] = r - d[s, 1, 0] - 2.0 * (d[s, 0, 1] + d[s, 1, 1])
    w = np.tile([1.0, 2.0], (len(rows), 1))
    return d, w, np.array([e for _, _, e in rows])


def tie_snr_rows(nbin):
    """The tie rows for ppf_profile_snr, which returns the S/N only: +1, -1,
    ... by bin parity laid over every dip (tied windows still tie exactly,
    now with mean 0 and a positive variance; sums stay exact integers) and one
    bin of 1000 on the first bin outside every dip from five bins after the
    expected window on, so that the edges, and with them the S/N, depend on
    where the reading starts."""
    wd = width_of(nbin)
    rows = []
    for _, row, want in tie_rows(nbin):
        x = row.copy()
        zero = np.flatnonzero(x == 0.0)
        x[zero] = np.where(zero % 2 == 0, 1.0, -1.0)
        if len(zero):
            k = (want + wd + 5) % nbin
            while row[k] == 0.0:
                k = (k + 1) % nbin
            x[k] = 1000.0
        rows.append(x)
    return np.stack(rows)


def snr_rows(nbin, thr=0.1):
    """The rows of the profile_snr tests: tests.test_gpu_snr._rows(8, nbin,
    SNR_SEEDS[nbin, thr]), the first four of them at nbin 8192."""
    from tests.test_gpu_snr import _rows
    x = _rows(8, nbin, SNR_SEEDS[nbin, thr])
    return x[:4] if nbin == 8192 else x


# integer_snr_rows: the edge sum, n and sum d^2 are exact, so what is rounded is
# v = sum d^2 / (W - 1) (u, u / 2 under the root), two square roots (2 u), two
# divisions (2 u), and in the reference one quotient (u / 2 under the root)
# and one root (u): 4.5 u + 1.5 u
INTEGER_SNR_ULPS = 6


def integer_snr_rows(nbin):
    """[3, nbin] integer-valued rows on which every sum ppf_profile_snr forms
    is exact in fp64, whatever its order: the off-pulse window (placed so
    that it wraps past the last bin) is +1, -1, +1, ... (and a final 0 when
    the width is odd), so its mean is exactly 0 and y = x; every other bin is
    2 or 4 plus an integer pulse, so a window that leaves the pattern by k
    bins gains at least 2 k - 1: the minimum is unique.  With nothing rounded
    before the final quotient, threshold 0 (whose upper crossing is an exact
    tie, c = C at the last bin before the window) has one answer."""
    wd = width_of(nbin)
    ph = np.arange(nbin) / nbin
    rows = []
    for r, (loc, amp) in enumerate([(0.3, 21.0), (0.5, 7.0), (0.62, 50.0)]):
        x = 2.0 + 2.0 * (np.arange(nbin) % 2) + np.rint(amp * np.exp(-0.5 * ((ph - loc) / 0.04) ** 2))
        pat = np.where(np.arange(wd) % 2 == 0, 1.0, -1.0)
        if wd % 2:
            pat[-1] = 0.0
        x[(nbin - wd // 2 - r + np.arange(wd)) % nbin] = pat
        rows.append(x)
    return np.stack(rows)


def zero_total_row(nbin=64):
    """0, 10, 0, 10, ...: every window of the (even) width has the same sum,
    so m is the row's mean, the variance is positive and C is exactly 0."""
    return np.tile([0.0, 10.0], nbin // 2)


def tscrunch_case(npol, nsub, nbin):
    """(subints [nsub, npol, 4, nbin], weights [nsub, 4]): float32-valued
    weights in [0.5, 2); channel 1 has weight 0 in every subint; channel 2 has
    weight 0 in subint 0, whose samples there are NaN."""
    rng = np.random.default_rng(9000 + 100 * nsub + npol + nbin)
    d = rng.normal(3.0, 5.0, (nsub, npol, 4, nbin))
    w = _f32(rng.uniform(0.5, 2.0, (nsub, 4)))
    w[:, 1] = 0.0
    w[0, 2] = 0.0
    d[0, :, 2] = np.nan
    return d, w


def unpack_case(dtype, nbin):
    """(raw [2, 4, 3, nbin], scl, offs [2, 4, 3]) with float32-valued DAT_SCL
    and DAT_OFFS and the sample type's extremes among the samples."""
    rng = np.random.default_rng(300 + nbin)
    shape = (2, 4, 3, nbin)
    if dtype == "float32":
        raw = rng.normal(0.0, 100.0, shape).astype(np.float32)
    else:
        info = np.iinfo(dtype)
        raw = rng.integers(info.min, info.max + 1, shape).astype(dtype)
        flat = raw.reshape(-1)
        flat[::5] = info.min
        flat[2::5] = info.max
    scl = _f32(rng.uniform(1e-3, 2.0, shape[:3]))
    offs = _f32(rng.normal(0.0, 50.0, shape[:3]))
    return raw, scl, offs


E2E_SHAPE = dict(nsub=3, nchan=7, nbin=256, seed=53)
