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
