"""Wavelet smoothing on the device (pplib.wavelet_smooth, smart_smooth,
fit_wavelet_smooth_function; ppspline's smooth="swt") against the numpy
restatement of its definition, tests/swt_reference.py, at run time.  Nothing
here is pinned against PyWavelets.

Tolerances.  Smoothed profiles: 1e-12 max|prof|, derived: at most 13 levels x
32 taps x 2^-53 ~ 5e-14 of rounding each way, with slack for the order of the
sums.  Objective: 1e3 x the largest relative difference between the
restatement in float64 and in np.longdouble over the same inputs (the named
64- and 128-bin profiles, levels 1, 3 and log2 nbin, the 30 grid points),
computed by the test; measured at 1.9e-11 (128 bins, seed 3, level 3, where
the smoothed profile's top-quarter noise is 1e-8 of its signal), so the bound
is 1.9e-8.  The 1e3 covers the device's different order of summation.  The
named profiles are stable inputs (tests/test_swt_cpu.py).
"""
import numpy as np
import pytest

from tests import swt_reference as R

pytestmark = pytest.mark.gpu

CASES = R.case_list()
TOL = 1e-12


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from pulseportraiture_amd.engine import get_engine
    return get_engine(0)


def levels_of(nbin):
    return (1, 3, int(np.log2(nbin)))


# ---------------------------------------------------------------------------
# wavelet_smooth
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nbin,seed,sigma", CASES)
def test_wavelet_smooth_matches_restatement(gpu, nbin, seed, sigma):
    from pulseportraiture_amd import pplib
    prof = R.named_profile(nbin, seed, sigma)
    combos = [(lev, fact, tt) for lev in levels_of(nbin) for fact in (0.0, 0.7, 1.9)
              for tt in ("hard", "soft")]
    worst = 0.0
    for tt in ("hard", "soft"):
        sel = [c for c in combos if c[2] == tt]
        out = gpu.wavelet_smooth_rows(np.tile(prof, (len(sel), 1)), [c[0] for c in sel],
                                      [c[1] for c in sel], tt).cpu().numpy()
        for (lev, fact, _), y in zip(sel, out):
            ref = R.wavelet_smooth(prof, lev, tt, fact)
            err = np.abs(y - ref).max() / np.abs(prof).max()
            worst = max(worst, err)
            assert err <= TOL, (lev, fact, tt, err)
            if fact == 0.0:
                assert np.abs(y - prof).max() <= TOL * np.abs(prof).max(), (lev, tt)
    print("nbin %d seed %d: worst error %.2e of max|prof|" % (nbin, seed, worst))
    # the pplib wrapper, one profile
    y = pplib.wavelet_smooth(prof, nlevel=3, threshtype="soft", fact=0.7)
    assert y.shape == prof.shape
    assert np.abs(y - R.wavelet_smooth(prof, 3, "soft", 0.7)).max() <= TOL * np.abs(prof).max()


def test_wavelet_smooth_8192_level_13(gpu):
    from pulseportraiture_amd import pplib
    prof = R.named_profile(8192, 1, 0.02)
    for fact in (0.0, 1.1):
        y = pplib.wavelet_smooth(prof, nlevel=13, fact=fact)
        ref = R.wavelet_smooth(prof, 13, "hard", fact)
        assert np.abs(y - ref).max() <= TOL * np.abs(prof).max(), fact
    assert np.abs(pplib.wavelet_smooth(prof, nlevel=13, fact=0.0) - prof).max() \
        <= TOL * np.abs(prof).max()


def test_wavelet_smooth_level_that_wraps(gpu):
    """nbin 64 at level 6: the dilated filter (span 481) wraps 8 times."""
    from pulseportraiture_amd import pplib
    prof = R.named_profile(64, 2, 0.05)
    for lev in (5, 6):
        y = pplib.wavelet_smooth(prof, nlevel=lev, fact=0.9)
        assert np.abs(y - R.wavelet_smooth(prof, lev, "hard", 0.9)).max() \
            <= TOL * np.abs(prof).max()


def test_wavelet_smooth_nbin_96(gpu):
    from pulseportraiture_amd import pplib
    prof = R.named_profile(96, 1, 0.05)
    y = pplib.wavelet_smooth(prof, nlevel=1, fact=0.7)
    assert np.abs(y - R.wavelet_smooth(prof, 1, "hard", 0.7)).max() <= TOL * np.abs(prof).max()
    with pytest.raises(ValueError):
        pplib.wavelet_smooth(prof, nlevel=6)
    with pytest.raises(NotImplementedError):
        pplib.wavelet_smooth(prof, wavelet="db4", nlevel=1)
    # the C entry point refuses it too (not only the wrapper)
    from pulseportraiture_amd.engine import PPFitError
    with pytest.raises(PPFitError):
        gpu.wavelet_smooth_rows(prof, 6, 1.0)
    with pytest.raises(PPFitError):
        gpu.wavelet_smooth_rows(np.ones(63), 1, 1.0)


def test_wavelet_smooth_batch_is_bitwise_rows(gpu):
    rng = np.random.default_rng(7)
    rows = np.stack([R.named_profile(256, s, 0.02) for s in (1, 2, 3, 4, 5)])
    levels = [1, 8, 3, 5, 2]
    facts = list(rng.uniform(0.0, 2.5, 5))
    for tt in ("hard", "soft"):
        batch = gpu.wavelet_smooth_rows(rows, levels, facts, tt).cpu().numpy()
        again = gpu.wavelet_smooth_rows(rows, levels, facts, tt).cpu().numpy()
        assert np.array_equal(batch, again)
        for i in range(len(rows)):
            one = gpu.wavelet_smooth_rows(rows[i], levels[i], facts[i], tt).cpu().numpy()
            assert np.array_equal(one, batch[i]), (tt, i)


# ---------------------------------------------------------------------------
# fit_wavelet_smooth_function
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rounding():
    return R.objective_rounding(levels_of)


def test_objective_matches_restatement(gpu, rounding):
    from pulseportraiture_amd import pplib
    worst80, vals = rounding
    rtol = 1e3 * worst80
    print("float64 against longdouble: %.3g; tolerance %.3g" % (worst80, rtol))
    assert 0.0 < worst80 < 1e-9  # (the measurement itself is sane)
    facts = [g * (3.0 / 29) for g in range(30)]
    worst = 0.0
    for (nbin, seed, level), (ref, ref_rc) in sorted(vals.items()):
        assert np.all(np.abs(np.abs(ref_rc - 1.0) - 0.1) > 1e-9), (nbin, seed, level)
        sigma = 0.05
        prof = R.named_profile(nbin, seed, sigma)
        obj, rc = gpu.wavelet_objective_rows(np.tile(prof, (30, 1)), level, facts, "hard", 0.1)
        obj, rc = obj.cpu().numpy(), rc.cpu().numpy()
        assert np.array_equal(obj == 0.0, ref == 0.0), (nbin, seed, level)
        nzr = ref != 0.0
        err = np.abs(obj[nzr] - ref[nzr]) / np.abs(ref[nzr])
        if err.size:
            worst = max(worst, err.max())
            assert err.max() <= rtol, (nbin, seed, level, err.max())
        assert np.abs(rc - ref_rc).max() <= 1e-12 * np.abs(ref_rc).max()
    print("device against restatement: %.3g" % worst)
    prof = R.named_profile(64, 1, 0.05)
    f = pplib.fit_wavelet_smooth_function(0.9, prof, "db8", 2, "hard", 0.1)
    ref = R.fit_wavelet_smooth_function(0.9, prof, 2)
    assert ref != 0.0 and abs(f - ref) <= rtol * abs(ref)


# ---------------------------------------------------------------------------
# smart_smooth
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nbin,seed,sigma", CASES)
def test_smart_smooth_matches_restatement(gpu, nbin, seed, sigma):
    from pulseportraiture_amd import pplib
    prof = R.named_profile(nbin, seed, sigma)
    ref = R.named_smart(nbin, seed, sigma)
    res = pplib.smart_smooth(prof, full=True)
    print("nbin %d seed %d: nlevel %d / %d, fact %.6f / %.6f, red_chi2 %.6f / %.6f"
          % (nbin, seed, res["nlevel"], ref["nlevel"], res["fact"], ref["fact"],
             res["red_chi2"], ref["red_chi2"]))
    assert int(res["nlevel"]) == ref["nlevel"]
    assert bool(res["zeroed"]) == ref["zeroed"]
    assert np.abs(res["smooth"] - ref["smooth"]).max() <= TOL * np.abs(prof).max()
    assert res["fun_vals"].shape == (int(np.log2(nbin)),)
    assert np.array_equal(pplib.smart_smooth(prof), res["smooth"])


def test_smart_smooth_soft(gpu):
    from pulseportraiture_amd import pplib
    prof = R.named_profile(128, 2, 0.05)
    ref = R.named_smart(128, 2, 0.05, "soft")
    res = pplib.smart_smooth(prof, full=True, threshtype="soft")
    assert int(res["nlevel"]) == ref["nlevel"] and bool(res["zeroed"]) == ref["zeroed"]
    # a soft threshold's output moves with fact: the polished facts must agree too
    assert abs(res["fact"] - ref["fact"]) <= 1e-9
    assert np.abs(res["smooth"] - ref["smooth"]).max() <= TOL * np.abs(prof).max()


def test_smart_smooth_special_rows(gpu):
    from pulseportraiture_amd import pplib
    # an all-zero row stays zero
    z = pplib.smart_smooth(np.zeros(128), full=True)
    assert not np.any(z["smooth"]) and z["nlevel"] == 0 and not z["zeroed"]
    # pure noise: every level's objective is 0, so level 1 at fact 0 (the
    # identity), red chi2 0, zeroed
    noise = np.random.default_rng(2).standard_normal(128)
    r = pplib.smart_smooth(noise, full=True)
    assert np.all(r["fun_vals"] == 0.0) and r["fact"] == 0.0
    # (red chi2 is 0 up to the identity's rounding: residuals within the
    # fact = 0 bound, TOL max|row|, over the row's noise, squared)
    assert 0.0 <= r["red_chi2"] <= (TOL * np.abs(noise).max() / R.get_noise(noise)) ** 2
    assert r["nlevel"] == 1 and r["zeroed"] and not np.any(r["smooth"])
    ref = R.smart_smooth(noise, full=True)
    assert ref["zeroed"] and ref["nlevel"] == 1 and np.all(ref["fun_vals"] == 0.0)
    # odd nbin: returned unchanged
    odd = R.named_profile(63, 1, 0.05)
    assert pplib.smart_smooth(odd) is odd
    # try_nlevels = 0: the identity
    p64 = R.named_profile(64, 1, 0.05)
    assert pplib.smart_smooth(p64, try_nlevels=0) is p64
    # nbin 96: one level, whatever is asked
    p96 = R.named_profile(96, 1, 0.05)
    r96 = pplib.smart_smooth(p96, try_nlevels=5, full=True)
    ref96 = R.smart_smooth(p96, try_nlevels=5, full=True)
    assert r96["fun_vals"].shape == (1,) and ref96["fun_vals"].shape == (1,)
    assert r96["nlevel"] == ref96["nlevel"] == 1 and bool(r96["zeroed"]) == ref96["zeroed"]
    assert np.abs(r96["smooth"] - ref96["smooth"]).max() <= TOL * np.abs(p96).max()
    with pytest.raises(NotImplementedError):
        pplib.smart_smooth(p64, wavelet="sym8")


def test_smart_smooth_2d_is_bitwise_rows(gpu):
    from pulseportraiture_amd import pplib
    rows = np.stack([R.named_profile(128, 1, 0.05), np.zeros(128), R.named_profile(128, 3, 0.05),
                     np.random.default_rng(2).standard_normal(128)])
    both = pplib.smart_smooth(rows, full=True)
    again = pplib.smart_smooth(rows, full=True)
    for key in ("smooth", "nlevel", "fact", "red_chi2", "zeroed", "fun_vals"):
        assert np.array_equal(both[key], again[key]), key
    for i, row in enumerate(rows):
        one = pplib.smart_smooth(row, full=True)
        for key in ("smooth", "nlevel", "fact", "red_chi2", "zeroed", "fun_vals"):
            assert np.array_equal(one[key], both[key][i]), (key, i)


def test_get_red_chi2(gpu):
    from pulseportraiture_amd import pplib
    prof = R.named_profile(128, 1, 0.05)
    model = R.wavelet_smooth(prof, 2, "hard", 0.8)
    ref = R.get_red_chi2(prof, model)
    assert abs(pplib.get_red_chi2(prof, model) - ref) <= 1e-12 * ref
    two = pplib.get_red_chi2(np.stack([prof, prof]), np.stack([model, model]))
    assert abs(two - 2 * 128 * ref / (2 + 128)) <= 1e-12 * ref


# ---------------------------------------------------------------------------
# more than one chunk of the workspace limit; more than 65,535 rows
# ---------------------------------------------------------------------------
def swt_row_bytes(nbin, L):
    """Workspace a row takes (SwtPlan, ppfit_capi.hip): L levels of 2 nbin
    doubles, L x (3 + 30 grid points) doubles, 16 bytes of per-row scalars and
    64 of alignment slack; a chunk is limit / that, at least 1, at most 65,535
    rows.  L is the deepest level of the whole call."""
    return L * 2 * nbin * 8 + L * 33 * 8 + 16 + 64


def at_limits(gpu, call, nbin, L):
    """call() at the default limit, in chunks of one row (1 byte) and in
    chunks of three; the limit is restored."""
    limit = gpu.workspace_limit()
    per_row = swt_row_bytes(nbin, L)
    try:
        whole = call()
        gpu.set_workspace_limit(1)
        ones = call()
        gpu.set_workspace_limit(3 * per_row + per_row // 2)
        threes = call()
    finally:
        gpu.set_workspace_limit(limit)
    return whole, ones, threes


CHUNK_LEVELS = [1, 3, 2, 5, 8, 4, 6, 7]  # the deepest in the second chunk of three
# every row its own fact; where a fact with red_chi2 within 0.1 of 1 exists on a
# 0.05 grid (rows 0, 1, 2, 3 and, hard, 5) it is one, so that the objective is
# not 0 in the first two chunks of three
CHUNK_FACTS = {"hard": [0.9, 1.95, 1.65, 0.15, 1.3, 0.3, 1.8, 2.05],
               "soft": [0.4, 0.55, 0.45, 0.05, 1.3, 1.55, 1.8, 2.05]}


def chunk_rows():
    return np.stack([R.named_profile(256, s, 0.02) for s in range(1, 9)])


@pytest.mark.parametrize("tt", ["hard", "soft"])
def test_wavelet_smooth_more_than_one_chunk(gpu, tt):
    """ppf_wavelet_smooth_rows offsets rows, nlevel, fact and out by the
    chunk's first row and reuses the workspace slices: 8 rows with their own
    level and fact in one chunk, in chunks of one and in chunks of 3, 3, 2 are
    bitwise the same, and the last chunk's rows are the restatement's."""
    rows = chunk_rows()
    whole, ones, threes = at_limits(
        gpu, lambda: gpu.wavelet_smooth_rows(rows, CHUNK_LEVELS, CHUNK_FACTS[tt],
                                             tt).cpu().numpy(), 256, max(CHUNK_LEVELS))
    assert np.array_equal(whole, ones)
    assert np.array_equal(whole, threes)
    for i in (6, 7):
        ref = R.wavelet_smooth(rows[i], CHUNK_LEVELS[i], tt, CHUNK_FACTS[tt][i])
        for y in (whole, ones, threes):
            assert np.abs(y[i] - ref).max() <= TOL * np.abs(rows[i]).max(), (tt, i)
        assert np.any(ref != rows[i])  # (the threshold did act)


@pytest.mark.parametrize("tt", ["hard", "soft"])
def test_wavelet_objective_more_than_one_chunk(gpu, tt):
    """The same for ppf_wavelet_objective_rows (obj + r0, red_chi2 + r0, the
    per-chunk noise slice)."""
    rows = chunk_rows()

    def call():
        obj, rc = gpu.wavelet_objective_rows(rows, CHUNK_LEVELS, CHUNK_FACTS[tt], tt, 0.1)
        return obj.cpu().numpy(), rc.cpu().numpy()
    whole, ones, threes = at_limits(gpu, call, 256, max(CHUNK_LEVELS))
    for k, name in enumerate(("objective", "red_chi2")):
        assert np.array_equal(whole[k], ones[k]), name
        assert np.array_equal(whole[k], threes[k]), name
    print("%s: objective %s red_chi2 %s" % (tt, whole[0], whole[1]))
    assert len(set(whole[1])) == 8  # every row's red chi2 is its own
    ref = np.array([R.fit_wavelet_smooth_function(f, row, lev, tt)
                    for row, lev, f in zip(rows, CHUNK_LEVELS, CHUNK_FACTS[tt])])
    assert np.array_equal(whole[0] == 0.0, ref == 0.0)
    assert np.count_nonzero(ref) == (5 if tt == "hard" else 4)


def test_smart_smooth_more_than_one_chunk(gpu):
    """ppf_smart_smooth_rows with the table: 8 rows at nbin 128, four levels;
    row 4 is all zero (the second row of the second chunk of three, in the
    slices a noisy profile, row 1, has just used): it stays zero with zero
    table entries at every limit, and all six outputs are bitwise the same."""
    rows = np.stack([R.named_profile(128, s, 0.05) for s in range(1, 9)])
    rows[4] = 0.0

    def call():
        return [t.cpu().numpy() for t in gpu.smart_smooth_rows(rows, 4, table=True)]
    whole, ones, threes = at_limits(gpu, call, 128, 4)
    names = ("smooth", "nlevel", "fact", "red_chi2", "zeroed", "table")
    for k, name in enumerate(names):
        assert np.array_equal(whole[k], ones[k]), name
        assert np.array_equal(whole[k], threes[k]), name
    for res in (whole, ones, threes):
        out = dict(zip(names, res))
        assert out["table"].shape == (8, 4)
        assert not np.any(out["smooth"][4]) and not np.any(out["table"][4])
        assert out["nlevel"][4] == 0 and not out["zeroed"][4]
        assert np.all(out["nlevel"][[0, 1, 2, 3, 5, 6, 7]] >= 1)
        assert np.any(out["table"][1]) and np.any(out["table"][5])


# five stable 16-bin profiles (as tests/test_swt_cpu.py defines stable: with
# try_nlevels = 2 the restatement's threshold gap is at least 1.6e-2 and its
# level gap at least 0.30; two choose level 1, three level 2, none is zeroed)
ROWCAP_SEEDS = (1, 3, 5, 8, 9)
# per-profile facts at level 1: the hard-threshold objective is not 0 at any of
# them, and the nearest |coefficient| is 9e-3 of the threshold away
ROWCAP_FACTS = [2.95, 63.0 / 29, 2.5, 2.9, 2.55]
ROWCAP_NROW = 65538  # a chunk holds at most 65,535 rows: 65,535 + 3


@pytest.fixture(scope="module")
def rowcap():
    five = np.stack([R.named_profile(16, s, 0.05) for s in ROWCAP_SEEDS])
    i = np.arange(ROWCAP_NROW) % 5
    return five, i, np.ascontiguousarray(five[i]), np.asarray(ROWCAP_FACTS)[i]


def test_wavelet_smooth_past_the_row_cap(gpu, rowcap):
    """65,538 rows of 16 bins at level 1: row i is bitwise row i % 5 of the
    call on the five profiles alone, which is the restatement's."""
    five, i, rows, facts = rowcap
    small = gpu.wavelet_smooth_rows(five, 1, ROWCAP_FACTS).cpu().numpy()
    for j in range(5):
        y, lam, mags = R.wavelet_smooth(five[j], 1, "hard", ROWCAP_FACTS[j], details=True)
        assert np.abs(mags - lam).min() >= 1e-6 * lam  # (the input condition)
        assert np.abs(small[j] - y).max() <= TOL * np.abs(five[j]).max(), j
    big = gpu.wavelet_smooth_rows(rows, 1, facts).cpu().numpy()
    assert big.shape == (ROWCAP_NROW, 16)
    assert np.array_equal(big, small[i])


def test_wavelet_objective_past_the_row_cap(gpu, rowcap):
    """The same for the objective.  Its bar at 16 bins is the module's recipe
    on these inputs: 1e3 x the largest relative difference between the
    restatement in float64 and in np.longdouble (measured at 3.8e-15, so
    3.8e-12); red_chi2 to 1e-12 as in test_objective_matches_restatement."""
    five, i, rows, facts = rowcap
    obj, rc = [t.cpu().numpy() for t in gpu.wavelet_objective_rows(five, 1, ROWCAP_FACTS)]
    ref = np.array([R.fit_wavelet_smooth_function(f, p, 1, full=True)
                    for p, f in zip(five, ROWCAP_FACTS)], dtype=np.float64)
    ref80 = np.array([R.fit_wavelet_smooth_function(f, p, 1, dtype=np.longdouble, full=True)
                      for p, f in zip(five, ROWCAP_FACTS)])
    assert np.all(ref[:, 0] != 0.0)
    assert np.all(np.abs(np.abs(ref[:, 1] - 1.0) - 0.1) > 1e-9)
    worst80 = float(np.abs(ref[:, 0] / ref80[:, 0] - 1).max())
    err = np.abs(obj / ref[:, 0] - 1).max()
    print("16 bins: float64 against longdouble %.3g, device against restatement %.3g"
          % (worst80, err))
    assert 0.0 < worst80 < 1e-12
    assert err <= 1e3 * worst80
    assert np.abs(rc - ref[:, 1]).max() <= 1e-12 * np.abs(ref[:, 1]).max()
    big = [t.cpu().numpy() for t in gpu.wavelet_objective_rows(rows, 1, facts)]
    assert big[0].shape == (ROWCAP_NROW,)
    assert np.array_equal(big[0], obj[i]) and np.array_equal(big[1], rc[i])


def test_smart_smooth_past_the_row_cap(gpu, rowcap):
    """The same for smart_smooth_rows(try_nlevels=2, table=True), all six
    outputs."""
    five, i, rows, _ = rowcap
    small = [t.cpu().numpy() for t in gpu.smart_smooth_rows(five, 2, table=True)]
    for j in range(5):
        ref = R.smart_smooth(five[j], try_nlevels=2, full=True)
        assert int(small[1][j]) == ref["nlevel"] and bool(small[4][j]) == ref["zeroed"]
        assert not ref["zeroed"]
        assert np.abs(small[0][j] - ref["smooth"]).max() <= TOL * np.abs(five[j]).max(), j
    assert set(small[1]) == {1, 2}
    big = [t.cpu().numpy() for t in gpu.smart_smooth_rows(rows, 2, table=True)]
    assert big[0].shape == (ROWCAP_NROW, 16) and big[5].shape == (ROWCAP_NROW, 2)
    for a, b in zip(big, small):
        assert np.array_equal(a, b[i])


# ---------------------------------------------------------------------------
# ppspline with smooth="swt"
# ---------------------------------------------------------------------------
NCHAN, NBIN, SNR_CUTOFF = 32, 256, 150.0


def swt_archive(seed, name, sigma=0.02):
    """32 x 256: two fixed shapes whose amplitudes vary smoothly with
    frequency, plus noise, as load_data's dict archive."""
    from pulseportraiture_amd.mjd import MJD
    rng = np.random.default_rng(seed)
    t = np.arange(NBIN) / NBIN
    freqs = np.linspace(1100.0, 1900.0, NCHAN)
    x = (freqs - 1500.0) / 400.0
    s1 = np.exp(-0.5 * ((t - 0.3) / 0.04) ** 2)
    s2 = np.exp(-0.5 * ((t - 0.45) / 0.02) ** 2)
    port = (np.outer(1.0 + 0.5 * x, s1) + np.outer(0.4 + 0.3 * x ** 2 - 0.2 * x, s2)
            + sigma * rng.standard_normal((NCHAN, NBIN)))
    noise = np.full(NCHAN, sigma)
    snrs = np.sqrt((port ** 2).sum(axis=1)) / sigma
    return dict(subints=port[None, None].copy(), freqs=freqs[None].copy(),
                weights=np.ones((1, NCHAN)), SNRs=snrs[None, None].copy(),
                noise_stds=noise[None, None].copy(), Ps=[0.003], epochs=[MJD(57300.0)], bw=800.0,
                source="J0000+0000", filename=name)


def host_significant(eigvec, snr_cutoff, rchi2_tol=0.1):
    """find_significant_eigvec's control flow (check_max = return_max = 10)
    with the restatement's smart_smooth; also every examined vector's S/N."""
    from pulseportraiture_amd.pplib import count_crossings
    smooth_eigvec = np.zeros(eigvec.shape)
    ieig, snrs = [], []
    for ivec in range(10):
        add = False
        ev = R.smart_smooth(eigvec[:, ivec], rchi2_tol=rchi2_tol)
        ev_noise = R.get_noise(eigvec[:, ivec]) * np.sqrt(len(ev) / 2.0)
        ev_snr = np.sum(np.abs(np.fft.rfft(ev)[1:]) ** 2) / ev_noise
        snrs.append(ev_snr)
        if ev_snr >= snr_cutoff:
            if ev_snr < 3 * snr_cutoff:
                ncross = count_crossings(abs(ev), 0.1 * abs(ev).max())
                if ncross < int(0.02 * len(ev)):
                    add = True
            else:
                add = True
        if add:
            ieig.append(ivec)
            smooth_eigvec[:, ivec] = ev
        if len(ieig) == 10:
            break
    return np.array(ieig, dtype=int), smooth_eigvec, np.array(snrs)


@pytest.fixture(scope="module")
def spline_model(gpu):
    from pulseportraiture_amd import ppspline
    arch = swt_archive(11, "swt_a.fits")
    dp = ppspline.DataPortrait(arch, quiet=True)
    dp.make_spline_model(smooth="swt", quiet=True)
    return arch, dp, host_significant(dp.eigvec, SNR_CUTOFF), R.smart_smooth(dp.mean_prof)


def test_spline_model_smoothed(gpu, spline_model):
    from pulseportraiture_amd import ppspline, pplib
    arch, dp, (ieig, smooth_eigvec, snrs), smooth_mean = spline_model
    print("S/N of the examined vectors:", " ".join("%.4g" % v for v in snrs))
    # the input condition: no examined vector sits on a decision boundary
    for edge in (SNR_CUTOFF, 3 * SNR_CUTOFF):
        assert np.all(np.abs(snrs - edge) >= 0.01 * edge), snrs
    assert len(ieig) >= 1 and list(dp.ieig) == list(ieig) and dp.ncomp == len(ieig)
    assert dp.smooth_eigvec.shape == dp.eigvec.shape
    assert np.abs(dp.smooth_eigvec[:, ieig] - smooth_eigvec[:, ieig]).max() \
        <= TOL * np.abs(dp.eigvec[:, ieig]).max()
    assert np.abs(dp.smooth_mean_prof - smooth_mean).max() <= TOL * np.abs(dp.mean_prof).max()
    assert np.any(dp.smooth_mean_prof != dp.mean_prof)  # (it did smooth)
    # the host composition of the rest of ppspline.py:100-172
    basis = smooth_eigvec[:, ieig]
    proj = np.dot(dp.portx - dp.mean_prof, basis)
    assert np.abs(dp.proj_port - proj).max() <= 1e-11 * np.abs(proj).max()
    s = ppspline.spline_smoothing(len(proj), dp.SNRsxs, dp.noise_stdsxs)
    (tck, _), _, ier, _ = ppspline.fit_spline_curve(proj, dp.pca_weights(), dp.freqsxs[0], s,
                                                    dp.bw, quiet=True)
    assert ier == dp.ier and tck[2] == dp.tck[2] and len(tck[0]) == len(dp.tck[0])
    assert np.abs(np.asarray(dp.tck[0]) - tck[0]).max() <= 1e-12 * np.abs(tck[0]).max()
    from scipy.interpolate import splev
    model = np.dot(basis, np.array(splev(dp.freqs[0], tck, der=0, ext=0))).T + smooth_mean
    scale = np.abs(model).max()
    assert np.abs(dp.model - model).max() <= 1e-11 * scale
    assert np.abs(dp.modelx - model[dp.ok_ichans[0]]).max() <= 1e-11 * scale
    assert np.array_equal(dp.model_masked, dp.model * dp.masks[0, 0])
    # without smoothing the same portrait passes more (noise) vectors
    plain = ppspline.DataPortrait(arch, quiet=True)
    plain.make_spline_model(quiet=True)
    assert not hasattr(plain, "smooth_eigvec") and plain.ncomp >= dp.ncomp
    assert pplib is not None


def test_spline_model_file_round_trip(gpu, spline_model, tmp_path):
    from pulseportraiture_amd import pplib
    _, dp, _, _ = spline_model
    path = str(tmp_path / "smooth.spl")
    dp.write_model(path, quiet=True)
    _, _, _, mean_prof, eigvec, _ = pplib.load_spline_model_file(path)
    assert np.array_equal(mean_prof, dp.smooth_mean_prof)
    assert np.array_equal(eigvec, dp.smooth_eigvec[:, dp.ieig])
    _, port = pplib.read_spline_model(path, dp.freqs[0], dp.nbin, quiet=True)
    assert np.max(np.abs(port - dp.model)) <= 1e-13 * np.max(np.abs(dp.model))


def test_spline_models_batch_equals_single_calls(gpu, spline_model):
    from pulseportraiture_amd import ppspline
    arch, single, _, _ = spline_model
    arch2 = swt_archive(12, "swt_b.fits")
    batch = [ppspline.DataPortrait(a, quiet=True) for a in (arch, arch2)]
    ppspline.make_spline_models(batch, smooth="swt", quiet=True)
    second = ppspline.DataPortrait(arch2, quiet=True)
    second.make_spline_model(smooth="swt", quiet=True)
    for one, dpb in zip((single, second), batch):
        assert list(one.ieig) == list(dpb.ieig)
        for name in ("eigvec", "mean_prof", "smooth_eigvec", "smooth_mean_prof", "proj_port",
                     "reconst_port", "model", "modelx"):
            assert np.array_equal(getattr(one, name), getattr(dpb, name)), name
        assert np.array_equal(one.tck[0], dpb.tck[0])


def test_find_significant_eigvec_swt(gpu, spline_model):
    from pulseportraiture_amd import pplib
    _, dp, _, _ = spline_model
    ieig, smooth_eigvec = pplib.find_significant_eigvec(dp.eigvec, smooth="swt",
                                                        return_smooth=True, try_nlevels=3)
    assert smooth_eigvec.shape == dp.eigvec.shape and len(ieig) >= 1
    for i in ieig:
        ref = R.smart_smooth(dp.eigvec[:, i], try_nlevels=3)
        assert np.abs(smooth_eigvec[:, i] - ref).max() <= TOL * np.abs(dp.eigvec[:, i]).max()
    rest = [i for i in range(dp.eigvec.shape[1]) if i not in ieig]
    assert not np.any(smooth_eigvec[:, rest])
    only = pplib.find_significant_eigvec(dp.eigvec, smooth="swt", try_nlevels=3)
    assert np.array_equal(only, ieig)
    with pytest.raises(NotImplementedError, match="PyWavelets"):
        pplib.find_significant_eigvec(dp.eigvec, return_smooth=True, try_nlevels=3)
    with pytest.raises(NotImplementedError, match="PyWavelets"):
        pplib.find_significant_eigvec(dp.eigvec, smooth=True)


def test_smooth_portrait(gpu):
    from pulseportraiture_amd import ppspline, pplib
    dp = ppspline.DataPortrait(swt_archive(11, "swt_a.fits"), quiet=True)
    port = dp.port.copy()
    dp.smooth_portrait(nlevel=3, fact=1.2)
    assert np.abs(dp.port[5] - R.wavelet_smooth(port[5], 3, "hard", 1.2)).max() \
        <= TOL * np.abs(port[5]).max()
    assert np.array_equal(dp.portx, dp.port[dp.ok_ichans[0]])
    assert np.array_equal(dp.noise_stdsxs, pplib.get_noise(dp.portx, chans=True))
    assert np.array_equal(dp.flux_prof, dp.port.mean(axis=1))
    dp2 = ppspline.DataPortrait(swt_archive(11, "swt_a.fits"), quiet=True)
    dp2.smooth_portrait(smart=True)
    ref = R.smart_smooth(port[7], try_nlevels=8)
    assert np.abs(dp2.port[7] - ref).max() <= TOL * np.abs(port[7]).max()


def test_swt_model_feeds_get_toas(gpu, tmp_path):
    """align -> ppspline(smooth="swt") -> TOAs: GetTOAs takes the written
    model and returns finite TOAs with the unsmoothed model's return codes.
    The two models are different templates (smoothed vectors, possibly fewer
    of them), so their phases differ by template offsets that no bound
    derived here covers: the differences are printed, not asserted."""
    import os
    from tests.conftest import GOLDEN
    from tests.test_gpu_ppspline import dict_archive
    from pulseportraiture_amd import archive, ppspline, pptoas, synth
    from pulseportraiture_amd.mjd import MJD
    z = np.load(os.path.join(GOLDEN, "ppspline.npz"))
    key, nsub = "48x512", 4
    files = {}
    for smooth in (False, "swt"):
        dp = ppspline.DataPortrait(dict_archive(z, key), quiet=True)
        dp.make_spline_model(smooth=smooth, max_ncomp=3, quiet=True)
        files[smooth] = str(tmp_path / ("model_%s.spl" % smooth))
        dp.write_model(files[smooth], quiet=True)
    w = synth.make_workload(nsub, 48, 512, seed=3, sigma=0.05)
    b = dict(subints=synth.workload_data_host(w)[:, None], freqs=np.tile(w.freqs, (nsub, 1)),
             weights=np.ones((nsub, 48)), SNRs=np.ones((nsub, 1, 48)), Ps=np.full(nsub, w.P),
             epochs=[MJD(57300.0 + 0.001 * i) for i in range(nsub)], DM=w.DM0, bw=800.0,
             nu0=1500.0, telescope="GBT", telescope_code="1", subtimes=[30.0] * nsub)
    archive.register_archive("swt_pipeline.fits", b)
    res = {}
    try:
        for smooth, model in files.items():
            gt = pptoas.GetTOAs(["swt_pipeline.fits"], model, quiet=True)
            gt.get_TOAs(quiet=True)
            res[smooth] = gt
    finally:
        archive.unregister_archive("swt_pipeline.fits")
    a, r = res["swt"], res[False]
    assert np.array_equal(a.rcs[0], r.rcs[0])
    for par, err in [("phis", "phi_errs"), ("DMs", "DM_errs")]:
        e = a.__dict__[err][0]
        d = np.abs(a.__dict__[par][0] - r.__dict__[par][0])
        print(par, "max |swt - unsmoothed| / sigma = %.3g" % np.max(d / e))
        assert np.all(np.isfinite(a.__dict__[par][0])) and np.all(np.isfinite(e)) and np.all(e > 0)
