"""tests/archive_prep_reference.py and tests/archive_prep_cases.py on the CPU:
the exact references agree with the oracle's restatements on ordinary rows,
every random input of tests/test_gpu_archive_prep.py is well separated
(window and crossing margins of at least MARGIN, no row left out, so the
device tests never skip a row), the S/N error bound stays below 1e-12 |snr|
on every row (a row past that is ill-conditioned and is not used), and the
tie rows tie exactly."""
import numpy as np
import pytest

from oracle import ppfit_oracle as O
from tests import archive_prep_cases as K
from tests import archive_prep_reference as R


def test_ints_are_exact():
    rng = np.random.default_rng(0)
    from fractions import Fraction
    a = np.concatenate([rng.normal(0, 1e3, 50), [0.0, 2.0 ** -40, -2.0 ** 30, 5e-324]])
    I, e = R._ints(a)
    assert all(isinstance(v, int) for v in I)
    assert [Fraction(v) * Fraction(2) ** e for v in I] == [Fraction(float(v)) for v in a]
    with pytest.raises(ValueError):
        R._ints([1.0, np.nan])


def test_baseline_window_rules():
    t = np.array([3.0, 1.0, 1.0, 5.0, 1.0, 1.0, 4.0])
    assert R.baseline_window(t, 2) == (1, 0.0)  # first of two exact ties
    j0, margin = R.baseline_window(np.array([5.0, 1.0, 2.0, 9.0]), 2)
    assert j0 == 1 and margin == (6.0 - 3.0) / 17.0
    assert R.baseline_window(np.array([1.0, 7.0, 7.0, 0.0]), 2)[0] == 3  # wraps
    nan = np.array([np.nan, 1.0, 2.0, 0.5, 3.0])
    assert R.baseline_window(nan, 2)[0] == 2  # 2.0 + 0.5; the windows over bin 0 never win
    assert R.baseline_window(np.full(4, np.nan), 2)[0] == 0
    assert O._first_min(np.array([np.nan, 3.0, np.nan, 1.0, 1.0])) == 3
    assert O._first_min(np.full(3, np.nan)) == 0
    assert O._first_min(np.array([np.nan, np.inf, np.inf])) == 1


@pytest.mark.parametrize("case", K.BASELINE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_baseline_inputs_are_separated_and_match_oracle(case):
    nbin, npol, ntot, nchan = case
    wd = K.width_of(nbin)
    d, w = K.baseline_case(*case)
    out, starts, margins = R.remove_baseline_exact(d, w, ntot, wd)
    print(case, "starts", starts, "margins", margins)
    assert margins[0] >= K.MARGIN and margins[2] >= K.MARGIN
    # the unweighted subint: a total of exact zeros, an exact tie at start 0
    assert starts[1] == 0 and margins[1] == 0.0
    if nbin >= 63:
        assert starts[0] + wd > nbin  # the best window wraps past the last bin
    if nchan >= 3:  # the unweighted channel would move the window if it counted
        w1 = w.copy()
        w1[2, 1] = 1.0
        assert R.remove_baseline_exact(d[2:], w1[2:], ntot, wd)[1][0] != starts[2]
    if ntot > 1:  # and so would dropping the second polarisation from the total
        one = R.remove_baseline_exact(d, w, 1, wd)[1]
        assert one[0] != starts[0] and one[2] != starts[2]
    ref, ostarts = O.remove_baseline(d, w, ntot=ntot, width=wd)
    np.testing.assert_array_equal(ostarts, starts)
    # the oracle forms the same sum, quotient and difference in its own order:
    # the device's bound holds for it too
    assert (R.remove_baseline_error(ref, d, starts, wd) <= R.remove_baseline_bound(d, wd)).all()
    # the exact error of the rounded reference itself is within one rounding
    err = R.remove_baseline_error(out, d, starts, wd)
    assert (err <= R.U * np.abs(out).max(axis=-1)).all()


def test_baseline_full_width_inputs():
    """duty 1.0: every window is the whole row.  Integer rows tie exactly
    (start 0); on random rows any start gives the same exact mean."""
    d, w, _ = K.tie_subints(512)
    out, starts, margins = R.remove_baseline_exact(d, w, 2, 512)
    assert (starts == 0).all() and (margins == 0.0).all()
    ref, ostarts = O.remove_baseline(d, w, ntot=2, duty=1.0)
    np.testing.assert_array_equal(ostarts, starts)
    d, w = K.baseline_case(100, 4, 2, 3)
    a = R.remove_baseline_exact(d, w, 2, 100)[0]
    for j0 in (1, 57):
        assert (R.remove_baseline_error(a, d, [j0] * 3, 100) <=
                R.U * np.abs(a).max(axis=-1)).all()


@pytest.mark.parametrize("nbin", K.TIE_NBINS)
def test_tie_rows_tie_exactly(nbin):
    wd = K.width_of(nbin)
    for name, row, want in K.tie_rows(nbin):
        assert (row == np.rint(row)).all()
        j0, margin = R.baseline_window(row, wd)
        assert (j0, margin) == (want, 0.0), name
        # the construction really holds a second window of the same sum
        sums = np.array([row[(j + np.arange(wd)) % nbin].sum() for j in range(nbin)])
        assert (sums == sums.min()).sum() >= 2 and sums[want] == sums.min(), name
        assert not (sums[:want] == sums.min()).any(), name
    d, w, want = K.tie_subints(nbin)
    assert (d == np.rint(d)).all() and np.abs(d).max() < 100
    for s, (name, row, _) in enumerate(K.tie_rows(nbin)):
        np.testing.assert_array_equal(w[s, 0] * (d[s, 0, 0] + d[s, 1, 0]) +
                                      w[s, 1] * (d[s, 0, 1] + d[s, 1, 1]), row)
    out, starts, margins = R.remove_baseline_exact(d, w, 2, wd)
    np.testing.assert_array_equal(starts, want)
    assert (margins == 0.0).all()
    # one polarisation alone does not give these windows: the test can tell
    assert (R.remove_baseline_exact(d, w, 1, wd)[1] != want).any()
    snr = R.profile_snr_exact(np.stack([r for _, r, _ in K.tie_rows(nbin)]), wd, 0.1)
    np.testing.assert_array_equal(snr["window"], want)
    assert (snr["snr"] == 0.0).all()  # windows of zeros (or a constant): v = 0
    # the S/N variant: same windows, still exact ties, an S/N that is not 0,
    # integer running sums clear of the (rounded) thresholds
    x = K.tie_snr_rows(nbin)
    assert (x == np.rint(x)).all()
    ex = R.profile_snr_exact(x, wd, 0.1)
    np.testing.assert_array_equal(ex["window"], want)
    assert (ex["window_margin"] == 0.0).all() and (ex["snr"][1:] > 0).all()
    assert (ex["rise_margin"][1:] >= K.MARGIN).all() and (ex["fall_margin"][1:] >= K.MARGIN).all()
    # separate dips: the S/N tells which of the tied windows was taken (dips
    # 64 bins apart are separate only where the width is below 64)
    for r in (2, 3, 4) if wd < 64 else (3, 4):
        j0 = {2: K.TIE_A + 64, 3: K.TIE_A + 256, 4: nbin - 10}[r]  # the other window, rolled to bin 0
        alt = R.profile_snr_exact(np.roll(x[r], -j0)[None], wd, 0.1)
        assert alt["window"][0] == 0
        assert abs(alt["snr"][0] - ex["snr"][r]) > 1e-3 * ex["snr"][r]


@pytest.mark.parametrize("thr", K.SNR_THRESHOLDS)
@pytest.mark.parametrize("nbin", K.SNR_NBINS)
def test_integer_snr_rows_are_exact(nbin, thr):
    """Integer-valued, window mean exactly 0, every partial sum far below
    2^53: the device's sums are exact in any order, so its edges are the
    exact ones even at threshold 0, where the upper crossing is a tie."""
    x = K.integer_snr_rows(nbin)
    wd = K.width_of(nbin)
    assert (x == np.rint(x)).all() and np.abs(x).sum(axis=-1).max() * wd < 2.0 ** 40
    ex = R.profile_snr_exact(x, wd, thr)
    want = (nbin - wd // 2 - np.arange(3)) % nbin
    np.testing.assert_array_equal(ex["window"], want)
    for r in range(3):
        assert x[r][(want[r] + np.arange(wd)) % nbin].sum() == 0.0  # m = 0: y = x exactly
    assert (ex["window_margin"] > 0).all()  # no tie for the window
    if wd == 1:
        assert (ex["snr"] == 0.0).all()
        return
    assert (ex["snr"] > 0).all()
    if thr == 0.0:
        assert (ex["rise"] == 0).all() and (ex["fall"] == nbin - wd - 1).all()
        assert (ex["fall_margin"] == 0.0).all()  # the tie that rounding would decide
    else:  # thr C is rounded on the device: the integer running sums stay clear of it
        assert (ex["rise_margin"] >= K.MARGIN).all() and (ex["fall_margin"] >= K.MARGIN).all()
    got = O.profile_snr(x, threshold=thr)
    assert (np.abs(got - ex["snr"]) <= K.INTEGER_SNR_ULPS * R.U * ex["snr"]).all()


@pytest.mark.parametrize("nbin,thr", K.SNR_CASES)
def test_snr_inputs_are_separated_and_match_oracle(nbin, thr):
    x = K.snr_rows(nbin, thr)
    assert len(x) == (4 if nbin == 8192 else 8)
    wd = K.width_of(nbin)
    ex = R.profile_snr_exact(x, wd, thr)
    print(nbin, thr, "margins", ex["window_margin"].min(), ex["rise_margin"].min(),
          ex["fall_margin"].min(), "bound/snr", (ex["bound"] / np.maximum(ex["snr"], 1e-300)).max())
    for k in ("window_margin", "rise_margin", "fall_margin"):
        assert (ex[k] >= K.MARGIN).all(), (k, ex[k])  # every row, none left out
    if wd == 1:
        assert (ex["snr"] == 0.0).all()
    else:
        assert (ex["snr"] > 0).all()
        assert (ex["bound"] <= 1e-12 * ex["snr"]).all()  # else ill-conditioned: another seed
    # the oracle's restatement (the device's order of sums) gives the same
    # window and edges -- a different one moves the snr by far more than the
    # bound -- and the same values within it
    got = O.profile_snr(x, threshold=thr)
    assert (np.abs(got - ex["snr"]) <= ex["bound"]).all()
    # C >= 0 for every finite row (m is the smallest window mean, never above
    # the row's mean), so "a negative total" cannot be built from finite data
    assert (ex["fall"] >= ex["rise"]).all() and (ex["rise"] >= 0).all()


def test_snr_zero_total_and_nan_rows():
    z = K.zero_total_row()
    ex = R.profile_snr_exact(z, K.width_of(len(z)) + 1, 0.1)  # even width 10
    assert ex["snr"][0] == 0.0 and ex["window"][0] == 0
    x = K.snr_rows(100)[:3].copy()
    x[1] = np.nan
    x[2, 40:43] = np.nan
    ex = R.profile_snr_exact(x, 15, 0.1)
    assert ex["window"][1] == 0 and ex["snr"][1] == 0.0 and ex["snr"][2] == 0.0
    assert not (40 - 15 < ex["window"][2] < 43)
    got = O.profile_snr(x)
    assert got[1] == 0.0 and got[2] == 0.0 and abs(got[0] - ex["snr"][0]) <= ex["bound"][0]


def test_remove_baseline_nan_rule():
    d, w = K.baseline_case(100, 2, 2, 3)
    d[0, 1, 2] = np.nan  # a weighted channel of the total
    out, starts, _ = R.remove_baseline_exact(d, w, 2, 15)
    ref, ostarts = O.remove_baseline(d, w, ntot=2, width=15)
    assert starts[0] == 0 and ostarts[0] == 0
    assert np.isnan(out[0, 1, 2]).all() and np.isnan(ref[0, 1, 2]).all()
    keep = np.ones((2, 3), bool)
    keep[1, 2] = False
    assert np.isfinite(out[0][keep]).all()
    fin = np.where(np.isnan(d), 0.0, d)
    err = R.remove_baseline_error(np.where(np.isnan(ref), 0.0, ref), fin, starts, 15)
    assert (err[0][keep] <= R.remove_baseline_bound(fin, 15)[0][keep]).all()
    clean = R.remove_baseline_exact(K.baseline_case(100, 2, 2, 3)[0], w, 2, 15)[0]
    np.testing.assert_array_equal(out[1:], clean[1:])


@pytest.mark.parametrize("case", K.TSCRUNCH_CASES, ids=lambda c: "x".join(map(str, c)))
def test_tscrunch_exact_and_weights(case):
    npol, nsub, nbin = case
    d, w = K.tscrunch_case(*case)
    out, wsum = R.tscrunch_exact(d, w)
    assert np.isfinite(out).all()
    assert (out[:, 1] == 0.0).all() and wsum[1] == 0.0
    run = np.zeros(4)
    for s in range(nsub):
        run = run + w[s]
    np.testing.assert_array_equal(run, wsum)  # the in-order fp64 sum is exact (bound's premise)
    dd = np.where(np.isnan(d), 0.0, d)
    want = np.einsum("sn,spnj->pnj", w, dd) / np.where(wsum > 0, wsum, 1.0)[None, :, None]
    assert (np.abs(out - want) <= R.tscrunch_bound(d, w) + 1e-300).all()
    if nsub > 1:
        o2, _ = R.tscrunch_exact(d[1:, :, 2:3], w[1:, 2:3])
        np.testing.assert_array_equal(out[:, 2:3], o2)


def test_e2e_archive_is_separated(tmp_path):
    """The coherence archive of the load_data test: its physical values are
    DATA * DAT_SCL + DAT_OFFS (bitwise what the device unpacks), and their
    ntot = 2 windows are separated."""
    from tests.test_gpu_psrfits import _coherence_archive
    _, raw, scl, offs, wts = _coherence_archive(str(tmp_path / "c.fits"), **K.E2E_SHAPE)
    phys = raw.astype(np.float64) * scl[..., None].astype(np.float64) + \
        offs[..., None].astype(np.float64)
    assert phys.shape[1] == 4 and wts[2, 5] == 0.0
    wd = K.width_of(phys.shape[-1])
    _, starts, margins = R.remove_baseline_exact(phys, wts, 2, wd)
    assert (margins >= K.MARGIN).all()
    assert (R.remove_baseline_exact(phys, wts, 1, wd)[1] != starts).any()
