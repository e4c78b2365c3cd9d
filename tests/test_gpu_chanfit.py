"""Fits across channels on the device: Engine.powlaw_fit_rows /
line_fit_rows (ppf_powlaw_fit_rows, ppf_line_fit_rows, ppfit_chanfit.hip),
pplib.fit_powlaw(s) and fit_DM(s)_to_freq_resids, DataPortrait.fit_flux_profile
and GetTOAs.get_channel_fits.  The yardstick is tests/chanfit_reference.py.

Bars.
- Power law: truth is scipy's leastsq restarted with the analytic Jacobian and
  ftol = xtol = 1e-15.  The device (leastsq's default tolerances) must end
  within 4 x the distance from that truth at which the reference's own
  configuration ends (leastsq, forward differences, default tolerances, from
  [1, 0]), and within 1e-3 sigma in any case; distances are in units of the
  truth's errors.  The reference's distance is taken as the largest over the
  rows of the call (the 72 rows of one n): the truth is restarted from the
  reference's own end point, so on a single row that distance can be exactly
  0 and says nothing about the stopping rule's reach.  Errors and covariance:
  relative deviation from the truth's cov_x chi2 / dof within 4 x the
  reference's own (largest over the rows), and within 1e-3.
- Line: truth is the closed form in np.longdouble.  Each of a, b, var(a),
  var(b), cov(a, b) and sum (w r)^2 must be within 8 x np.polyfit's own
  relative deviation from it (largest over the rows of the call) plus 4 ulp.
"""
import functools
import os
import shutil

import numpy as np
import pytest

from tests import chanfit_reference as CR

pytestmark = pytest.mark.gpu

TOL = 1.49012e-8
EPS = np.finfo(np.float64).eps
OK_STATUS = (1, 2, 3)
UNUSABLE = -3
PAR = ("PSR J1234+5678\nRAJ 12:34:00.0\nDECJ +56:07:08.9\nF0 345.67890123456789\n"
       "PEPOCH 57000.0\nDM 0.0\n")


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from pulseportraiture_amd.engine import get_engine
    return get_engine(0)


def powlaw_dev(eng, c, rows=slice(None), init=(1.0, 0.0)):
    out, info = eng.powlaw_fit_rows(c["y"][rows], c["errs"][rows], c["freqs"][rows],
                                    c["nu_ref"][rows], np.array(init))
    return out.cpu().numpy(), info.cpu().numpy()


@functools.lru_cache(maxsize=None)
def powlaw_yardstick(n):
    """Inputs of check 1 at n points with, per row, the truth and the
    reference's own configuration as arrays [72, 5] = amp, alpha, amp_err,
    alpha_err, cov."""
    c = CR.powlaw_inputs(n)
    keys = ("amp", "alpha", "amp_err", "alpha_err", "cov")
    truth, ref = [], []
    for r in range(len(c["y"])):
        a = (c["y"][r], c["errs"][r], c["freqs"][r], c["nu_ref"][r], [1.0, 0.0])
        t, f = CR.powlaw_truth(*a), CR.powlaw_reference(*a)
        truth.append([t[k] for k in keys])
        ref.append([f[k] for k in keys])
    return c, np.array(truth), np.array(ref)


def check_powlaw(tag, out, info, c, truth, ref, rows=slice(None)):
    t = truth[rows]
    dist = lambda v: np.abs(v[:, [0, 1]] - truth[:, [0, 1]]) / truth[:, [2, 3]]
    rel = lambda v: np.abs(v[:, 2:] / truth[:, 2:] - 1.0)
    d_ref, e_ref = dist(ref).max(), rel(ref).max()
    dev = out[:, [0, 2, 1, 3, 4]]
    d_dev = (np.abs(dev[:, [0, 1]] - t[:, [0, 1]]) / t[:, [2, 3]]).max()
    e_dev = np.abs(dev[:, 2:] / t[:, 2:] - 1.0).max()
    print("%s: distance from truth device %.3g reference %.3g sigma; errors device %.3g "
          "reference %.3g; nfev max %d; status %s" % (
              tag, d_dev, d_ref, e_dev, e_ref, info[:, 1].max(), sorted(set(info[:, 0]))))
    n_used = CR.usable(c["errs"][rows]).sum(axis=1)
    assert np.all(np.isin(info[:, 0], OK_STATUS)), (tag, info[:, 0])
    np.testing.assert_array_equal(info[:, 3], n_used)
    np.testing.assert_array_equal(info[:, 2], n_used - 2)
    assert info[:, 1].max() <= 6000
    assert d_dev <= min(4.0 * d_ref, 1e-3), (tag, d_dev, d_ref)
    assert e_dev <= min(4.0 * e_ref, 1e-3), (tag, e_dev, e_ref)
    # chi2 at the device's parameters.  The model differs from numpy's power by
    # a few ulp, a residual by that times the S/N (up to 500): 1e-13, against
    # residuals of order one, so chi2 agrees far inside 1e-9
    r = [CR.powlaw_resid([o[0], o[2]], y[ok], e[ok], f[ok], 1500.0) for o, y, e, f, ok in zip(
        out, c["y"][rows], c["errs"][rows], c["freqs"][rows], CR.usable(c["errs"][rows]))]
    np.testing.assert_allclose(out[:, 5], [x @ x for x in r], rtol=1e-9)


# -- 1. power-law fits against scipy -----------------------------------------
@pytest.mark.parametrize("n", CR.NS)
def test_powlaw_fits_against_scipy(eng, n):
    c, truth, ref = powlaw_yardstick(n)
    out, info = powlaw_dev(eng, c)
    if n > 5:  # masks on a lane's first and last point
        bad = ~CR.usable(c["errs"])
        assert bad[:, 0].any() and bad[:, n - 1].any() and bad[:, 64 * ((n - 1) // 64)].any()
        assert (bad.sum(axis=1) >= n // 10 - 2).all()
    check_powlaw("n %d" % n, out, info, c, truth, ref)


# -- 2. line fits against np.polyfit -------------------------------------------
@pytest.mark.parametrize("n", CR.NS)
def test_line_fits_against_polyfit(eng, n):
    c = CR.line_inputs(n)
    out = eng.line_fit_rows(c["x"], c["y"], c["w"]).cpu().numpy()
    truth = np.array([CR.line_truth(x, y, w) for x, y, w in zip(c["x"], c["y"], c["w"])])
    poly = np.array([CR.line_polyfit(x, y, w) for x, y, w in zip(c["x"], c["y"], c["w"])])
    e_poly = np.abs((poly - truth) / truth).astype(np.float64).max(axis=0)
    e_dev = np.abs((out[:, :6] - truth) / truth).astype(np.float64).max(axis=0)
    print("n %d: relative deviation from the long-double line, in ulp: device %s polyfit %s" % (
        n, np.round(e_dev / EPS, 1), np.round(e_poly / EPS, 1)))
    np.testing.assert_array_equal(out[:, 6], CR.usable(c["errs"]).sum(axis=1))
    np.testing.assert_array_equal(out[:, 7], 0.0)
    assert np.all(e_dev <= 8.0 * e_poly + 4.0 * EPS), (n, e_dev / EPS, e_poly / EPS)


def test_fit_DM_to_freq_resids_fields(eng):
    """The DataBunch against the same fields recomputed on the host from
    np.polyfit.  a, b and their covariance agree with polyfit's to a few
    hundred ulp (the check above), and DM, offset, their errors, ab_cov, the
    residuals and chi2 are smooth in them: rtol 1e-9.  nu_ref_err takes the
    difference (a_err / a)^2 + (b_err / b)^2 - 2 cov / (a b), whose terms
    cancel (a and b are strongly anticorrelated over a band this narrow in
    nu^-2) and so amplify those ulp: rtol 1e-6.  Rows with -b / a < 0 give a
    NaN nu_ref in both."""
    from pulseportraiture_amd import pplib
    c = CR.line_inputs(64)
    # a row whose slope and offset share a sign: -b / a < 0
    c["y"][0] = (CR.Dconst * 1e-3 * c["x"][0] + 5e-6 +
                 np.where(CR.usable(c["errs"][0]), c["errs"][0], 0.0) * 0.1)
    got = pplib.fit_DMs_to_freq_resids(c["freqs"], c["y"], c["errs"])
    one = pplib.fit_DM_to_freq_resids(c["freqs"][3], c["y"][3], c["errs"][3])
    nan_rows = 0
    for r in range(len(c["y"])):
        want = CR.dm_bunch(c["freqs"][r], c["y"][r], c["errs"][r])
        for k, v in want.items():
            g = got[k][r]
            rtol = 1e-6 if k == "nu_ref_err" else 1e-9
            if k == "residuals":
                ok = CR.usable(c["errs"][r])
                np.testing.assert_allclose(g[ok], v[ok], rtol=0, atol=1e-9 * np.abs(c["y"][r]).max())
            elif k == "dof":
                assert g == v
            elif np.isnan(v):
                assert np.isnan(g), (r, k, g)
            else:
                np.testing.assert_allclose(g, v, rtol=rtol, err_msg="row %d %s" % (r, k))
        nan_rows += int(np.isnan(want["nu_ref"]))
        if r == 3:
            for k in want:
                np.testing.assert_array_equal(np.asarray(one[k]), np.asarray(got[k][r]))
    assert np.isnan(got.nu_ref[0]) and nan_rows >= 1 and nan_rows < len(c["y"])
    assert set(one) == {"DM", "DM_err", "offset", "offset_err", "nu_ref", "nu_ref_err", "ab_cov",
                        "residuals", "chi2", "dof", "red_chi2"}


# -- 3. shapes and independence -------------------------------------------------
def many_rows(make, nrow):
    """nrow rows of 64 points from the generator's calls with seeds of their own."""
    parts, have = [], 0
    while have < nrow:
        parts.append(make(64, seed=900 + len(parts)))
        have += len(parts[-1]["y"])
    return {k: np.concatenate([p[k] for p in parts])[:nrow] for k in parts[0]}


def test_rows_are_independent_of_the_call(eng):
    import torch
    c = many_rows(CR.powlaw_inputs, 257)
    li = many_rows(CR.line_inputs, 257)
    dev = lambda a: torch.as_tensor(a, device=eng.device)
    y, e, f, nr = dev(c["y"]), dev(c["errs"]), dev(c["freqs"]), dev(c["nu_ref"])
    x, ly, w = dev(li["x"]), dev(li["y"]), dev(li["w"])
    init = dev(np.array([1.0, 0.0]))

    def both(lo, hi):
        o, i = eng.powlaw_fit_rows(y[lo:hi], e[lo:hi], f[lo:hi], nr[lo:hi], init)
        return o.cpu().numpy(), i.cpu().numpy(), eng.line_fit_rows(x[lo:hi], ly[lo:hi],
                                                                   w[lo:hi]).cpu().numpy()
    out, info, line = both(0, 257)
    assert np.all(np.isin(info[:, 0], OK_STATUS)) and np.all(line[:, 7] == 0.0)
    assert len(np.unique(out[:, 0])) == 257
    for lo, hi in [(0, 4), (4, 9)] + [(r, r + 1) for r in range(257)]:  # nrow 4, 5, 1
        o, i, ln = both(lo, hi)
        assert o.tobytes() == out[lo:hi].tobytes(), (lo, hi)
        assert i.tobytes() == info[lo:hi].tobytes(), (lo, hi)
        assert ln.tobytes() == line[lo:hi].tobytes(), (lo, hi)


def test_one_row_of_16384_points(eng):
    """Rows above 512 points are read again in every evaluation.  The
    reference's distance is the largest over the 72 rows at this n, as in
    check 1; the device fits them in one call and the first one alone."""
    c, truth, ref = powlaw_yardstick(16384)
    out, info = powlaw_dev(eng, c)
    check_powlaw("n 16384", out, info, c, truth, ref)
    one, one_info = powlaw_dev(eng, c, slice(0, 1))
    assert one.tobytes() == out[:1].tobytes() and one_info.tobytes() == info[:1].tobytes()
    li = CR.line_inputs(16384, nrow=2)
    line = eng.line_fit_rows(li["x"], li["y"], li["w"]).cpu().numpy()
    truth = np.array([CR.line_truth(x, y, w) for x, y, w in zip(li["x"], li["y"], li["w"])])
    poly = np.array([CR.line_polyfit(x, y, w) for x, y, w in zip(li["x"], li["y"], li["w"])])
    e_poly = np.abs((poly - truth) / truth).astype(np.float64).max(axis=0)
    e_dev = np.abs((line[:, :6] - truth) / truth).astype(np.float64).max(axis=0)
    print("line n 16384 (ulp): device %s polyfit %s" % (np.round(e_dev / EPS, 1),
                                                        np.round(e_poly / EPS, 1)))
    assert np.all(e_dev <= 8.0 * e_poly + 4.0 * EPS)


def test_unusable_rows_do_not_disturb_their_neighbours(eng):
    c = {k: v[:5].copy() for k, v in CR.powlaw_inputs(64).items()}
    li = {k: v[:5].copy() for k, v in CR.line_inputs(64).items()}
    out0, info0 = powlaw_dev(eng, c)
    line0 = eng.line_fit_rows(li["x"], li["y"], li["w"]).cpu().numpy()
    # row 2 masked down to 2 usable points; a NaN y at a usable point of row 4
    c["errs"][2] = 0.0
    c["errs"][2, [5, 9]] = 1.0
    li["w"][2] = 0.0
    li["w"][2, [5, 9]] = 1e11
    i4 = int(np.flatnonzero(CR.usable(c["errs"][4]))[3])
    c["y"][4, i4] = np.nan
    j4 = int(np.flatnonzero(CR.usable(li["w"][4]))[3])
    li["y"][4, j4] = np.nan
    out, info = powlaw_dev(eng, c)
    line = eng.line_fit_rows(li["x"], li["y"], li["w"]).cpu().numpy()
    for r in (0, 1, 3):
        assert out[r].tobytes() == out0[r].tobytes() and info[r].tobytes() == info0[r].tobytes()
        assert line[r].tobytes() == line0[r].tobytes()
    for r in (2, 4):
        assert info[r, 0] == UNUSABLE and np.isnan(out[r]).all()
        assert line[r, 7] == UNUSABLE and np.isnan(line[r, :6]).all()
    assert info[2, 3] == 2 and info[2, 2] == 0 and line[2, 6] == 2
    assert info[4, 3] == info0[4, 3] and line[4, 6] == line0[4, 6]
    # a NaN y at a point that is left out is not looked at
    c2 = {k: v[:2].copy() for k, v in CR.powlaw_inputs(64).items()}
    o_ref, i_ref = powlaw_dev(eng, c2)
    c2["y"][0, int(np.flatnonzero(~CR.usable(c2["errs"][0]))[0])] = np.nan
    o2, i2 = powlaw_dev(eng, c2)
    assert o2.tobytes() == o_ref.tobytes() and i2.tobytes() == i_ref.tobytes()
    # n = 1 and n = 2: too few points whatever they hold
    for n in (1, 2):
        o, i = eng.powlaw_fit_rows(np.ones((3, n)), np.ones((3, n)),
                                   np.full((3, n), 1400.0) + np.arange(n), 1500.0, [1.0, 0.0])
        assert np.isnan(o.cpu().numpy()).all()
        np.testing.assert_array_equal(i.cpu().numpy(), [[UNUSABLE, 0, n - 2, n]] * 3)
        ln = eng.line_fit_rows(np.arange(n) + np.ones((3, n)), np.ones((3, n)),
                               np.ones((3, n))).cpu().numpy()
        assert np.isnan(ln[:, :6]).all() and np.all(ln[:, 6] == n) and np.all(ln[:, 7] == UNUSABLE)
    # nu_ref <= 0 and nu <= 0
    c3 = {k: v[:3].copy() for k, v in CR.powlaw_inputs(5).items()}
    c3["nu_ref"][0] = 0.0
    c3["freqs"][1, 2] = -1.0
    o3, i3 = powlaw_dev(eng, c3)
    np.testing.assert_array_equal(i3[:, 0] == UNUSABLE, [True, True, False])
    assert np.isnan(o3[:2]).all() and np.isfinite(o3[2]).all()


def test_shape_limits_are_invalid_arguments(eng):
    import ctypes
    import torch
    from pulseportraiture_amd.engine import PPFitError
    buf = torch.zeros(64, dtype=torch.float64, device=eng.device)
    ibuf = torch.zeros(64, dtype=torch.int32, device=eng.device)
    p, ip = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(ibuf.data_ptr())
    for nrow, n in [(1, 0), (1, 16385), (0, 64), (1, -1)]:
        assert eng.lib.ppf_powlaw_fit_rows(eng.ctx, nrow, n, p, p, p, p, p, TOL, TOL, 0, p,
                                           ip) == -1, (nrow, n)
        assert eng.lib.ppf_line_fit_rows(eng.ctx, nrow, n, p, p, p, p) == -1, (nrow, n)
    with pytest.raises(PPFitError):
        eng.powlaw_fit_rows(np.ones((1, 16385)), 1.0, 1400.0, 1500.0, [1.0, 0.0])
    with pytest.raises(PPFitError):
        eng.line_fit_rows(np.ones((1, 16385)), np.ones((1, 16385)), 1.0)


# -- 4. DataPortrait.fit_flux_profile ------------------------------------------
@pytest.fixture(scope="module")
def flux_archive(eng, tmp_path_factory):
    """16 channels x 64 bins: one Gaussian whose amplitude follows a power law
    of index -1.7 across the band, channels 3 and 11 zapped."""
    from pulseportraiture_amd import pplib
    d = tmp_path_factory.mktemp("chanfit_flux")
    par = d / "fake.par"
    par.write_text(PAR)
    nchan, nbin = 16, 64
    freqs = np.linspace(1125.0, 1875.0, nchan)
    rng = np.random.default_rng(12)
    prof = np.exp(-0.5 * ((np.arange(nbin) / nbin - 0.5) / 0.05) ** 2)
    amp = 4.0 * (freqs / 1500.0) ** -1.7
    port = amp[:, None] * prof[None] + 0.02 * rng.standard_normal((nchan, nbin))
    weights = np.ones((1, nchan))
    weights[0, [3, 11]] = 0.0
    name = str(d / "flux.fits")
    pplib.write_archive(port[None, None], str(par), freqs, outfile=name, weights=weights,
                        dedispersed=True, quiet=True)
    return name


@pytest.mark.parametrize("module", ["ppspline", "ppgauss"])
def test_fit_flux_profile(eng, flux_archive, module, capsys):
    import importlib
    from pulseportraiture_amd import pplib
    mod = importlib.import_module("pulseportraiture_amd." + module)
    dp = mod.DataPortrait(flux_archive, quiet=True)
    assert len(dp.flux_profx) == 14
    capsys.readouterr()
    dp.fit_flux_profile(quiet=True)
    assert capsys.readouterr().out == ""
    errs = np.ones(14)
    r = pplib.fit_powlaws(dp.flux_profx[None], [1.0, 0.0], errs[None], dp.freqsxs[0][None],
                          dp.nu0)
    for got, want in [(dp.spect_A, r.amp[0]), (dp.spect_A_err, r.amp_err[0]),
                      (dp.spect_index, r.alpha[0]), (dp.spect_index_err, r.alpha_err[0])]:
        assert np.float64(got).tobytes() == np.float64(want).tobytes()
    assert dp.spect_A_ref == dp.nu0 and dp.flux_fit.dof == 12 and dp.flux_fit.status in OK_STATUS
    np.testing.assert_allclose(
        dp.flux_fit.residuals,
        dp.flux_profx - pplib.powlaw(dp.freqsxs[0], dp.nu0, dp.spect_A, dp.spect_index),
        rtol=0, atol=1e-14 * dp.spect_A)
    t = CR.powlaw_truth(dp.flux_profx, errs, np.asarray(dp.freqsxs[0]), dp.nu0, [1.0, 0.0])
    print("%s: A %.6f +/- %.6f alpha %.6f +/- %.6f; scipy %.6f %.6f" % (
        module, dp.spect_A, dp.spect_A_err, dp.spect_index, dp.spect_index_err, t["amp"],
        t["alpha"]))
    assert abs(dp.spect_A - t["amp"]) <= 1e-3 * t["amp_err"]
    assert abs(dp.spect_index - t["alpha"]) <= 1e-3 * t["alpha_err"]
    assert abs(dp.spect_index + 1.7) < 0.1  # the injected index
    # the summary, and the note in place of a plot
    dp.fit_flux_profile(nu_ref=1400.0, plot=True)
    text = capsys.readouterr().out
    assert "Flux-density power-law fit" in text and "(flux at 1400.00 MHz)" in text
    assert "plotting is not part of this build" in text
    assert dp.spect_A_ref == 1400.0
    dp.fit_flux_profile(savefig="x.png", quiet=True)
    assert "plotting is not part of this build" in capsys.readouterr().out
    assert not os.path.exists("x.png")


# -- 5. GetTOAs.get_channel_fits -------------------------------------------------
DDM = 2e-3
ZAP = 6
CHANFIT_LISTS = {
    "nb": ["nb_DMs", "nb_DM_errs", "nb_offsets", "nb_offset_errs", "nb_nu_refs", "nb_nu_ref_errs",
           "nb_red_chi2s"],
    "scat": ["scat_amps", "scat_amp_errs", "scat_indices", "scat_index_errs", "scat_nu_refs",
             "scat_red_chi2s"],
    "spect": ["spect_As", "spect_A_errs", "spect_indices", "spect_index_errs",
              "spect_red_chi2s"]}


@pytest.fixture(scope="module")
def fake_archives(eng, tmp_path_factory):
    """Two seeded make_fake_pulsar archives, 3 x 16 x 128, channel ZAP with
    weight 0, a dDM, a scattering time of 0.03 rotations at 1500 MHz and a
    phase offset of +0.01 (first archive) or -0.01 (second) injected.  The ephemeris DM is 0, so that the stored (dispersed) profiles'
    phases stay well inside one turn across the band: the line is fitted to
    the phases as they are, as the reference's function takes residuals."""
    from pulseportraiture_amd import pplib, synth
    d = tmp_path_factory.mktemp("chanfit_toas")
    par = d / "fake.par"
    par.write_text(PAR)
    model = str(d / "example.gmodel")
    shutil.copy(synth.EXAMPLE_GMODEL, model)
    weights = np.ones((3, 16))
    weights[:, ZAP] = 0.0
    names = []
    for k in range(2):
        names.append(str(d / ("fake%d.fits" % k)))
        pplib.make_fake_pulsar(model, str(par), outfile=names[-1], nsub=3, nchan=16, nbin=128,
                               noise_stds=0.02, dDM=DDM, phase=0.01 * (1 - 2 * k), weights=weights,
                               t_scat=0.03 / 345.67890123456789, dedispersed=False, tsub=60.0,
                               seed=41 + k, quiet=True)
    return names, model


def snapshot(gt):
    from pulseportraiture_amd.pptoas import _LIST_ATTRS
    snap = {}
    for a in _LIST_ATTRS:
        v = getattr(gt, a)
        snap[a] = [np.array(x, copy=True) if isinstance(x, np.ndarray) else x for x in v] \
            if isinstance(v, list) else v
    return snap


def same_snapshot(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if not isinstance(a[k], list):
            continue
        assert len(a[k]) == len(b[k]), k
        for x, y in zip(a[k], b[k]):
            if isinstance(x, np.ndarray) and x.dtype != object:
                np.testing.assert_array_equal(x, y, err_msg=k)


def tim_text(gt, path):
    from pulseportraiture_amd import pplib
    pplib.write_TOAs(gt.TOA_list, SNR_cutoff=0.0, outfile=str(path), append=False)
    return open(path).read()


def test_get_channel_fits_narrowband(eng, fake_archives, tmp_path, capsys):
    from pulseportraiture_amd import archive, pplib, pptoas
    names, model = fake_archives
    gt = pptoas.GetTOAs(names, model, quiet=True)
    with pytest.raises(RuntimeError, match="get_channel_fits"):
        gt.get_channel_fits()
    gt.get_narrowband_TOAs(fit_scat=True, print_flux=True, quiet=True)
    before, tim = snapshot(gt), tim_text(gt, tmp_path / "a.tim")
    capsys.readouterr()
    gt.get_channel_fits(quiet=False)
    text = capsys.readouterr().out
    assert all(sum(ln.startswith(n + ":") for ln in text.splitlines()) == 1 for n in names)
    same_snapshot(before, snapshot(gt))
    assert tim_text(gt, tmp_path / "b.tim") == tim
    for kind in CHANFIT_LISTS.values():
        for a in kind:
            v = getattr(gt, a)
            assert len(v) == 2 and all(x.shape == (3,) for x in v), a
            if a not in ("nb_nu_refs", "nb_nu_ref_errs"):
                assert all(np.isfinite(x).all() for x in v), (a, v)
    # the crossing frequency exists where offset and DM differ in sign (the two
    # archives' phase offsets have opposite signs), and is NaN elsewhere
    crossing = [-o / d > 0.0 for o, d in zip(gt.nb_offsets, gt.nb_DMs)]
    assert sorted(bool(c.all()) for c in crossing) == [False, True] and \
        sorted(bool(c.any()) for c in crossing) == [False, True], crossing
    for i in range(2):
        assert np.array_equal(np.isfinite(gt.nb_nu_refs[i]), crossing[i])
        assert np.array_equal(np.isfinite(gt.nb_nu_ref_errs[i]), crossing[i])
    for i in range(2):
        meta = archive.open_archive(names[i], pscrunch=True).meta
        freqs, nu0 = np.asarray(meta.freqs, dtype=np.float64), float(meta.nu0)
        np.testing.assert_allclose(freqs, np.tile(np.linspace(1125.0, 1875.0, 16), (3, 1)))
        assert nu0 == 1500.0
        P = gt.Ps[i][:, None]
        used = lambda e: np.where(np.isfinite(e) & (e > 0.0), e, 0.0)
        e = used(gt.phi_errs[i] * P)
        assert (e[:, ZAP] == 0.0).all() and (np.delete(e, ZAP, axis=1) > 0.0).all()
        r = pplib.fit_DMs_to_freq_resids(freqs, gt.phis[i] * P, e)
        assert (r.n_used == 15).all() and (r.dof == 13).all()
        for a, want in zip(CHANFIT_LISTS["nb"], [r.DM, r.DM_err, r.offset, r.offset_err, r.nu_ref,
                                                 r.nu_ref_err, r.red_chi2]):
            assert getattr(gt, a)[i].tobytes() == want.tobytes(), a
        print("archive %d: nb_DMs %s +/- %s (injected %g)" % (i, gt.nb_DMs[i], gt.nb_DM_errs[i],
                                                              DDM))
        assert np.all(np.abs(gt.nb_DMs[i] - DDM) <= 5.0 * gt.nb_DM_errs[i])
        assert gt.log10_tau
        tau = 10.0 ** gt.taus[i] * P
        sig = used(np.log(10.0) * tau * gt.tau_errs[i])
        init = np.column_stack([[np.median(t[s > 0.0]) for t, s in zip(tau, sig)],
                                np.full(3, pplib.scattering_alpha)])
        r = pplib.fit_powlaws(tau, init, sig, freqs, nu0)
        assert (r.n_used == 15).all() and np.all(np.isin(r.status, OK_STATUS))
        for a, want in zip(CHANFIT_LISTS["scat"], [r.amp, r.amp_err, r.alpha, r.alpha_err,
                                                   r.nu_ref, r.chi2 / r.dof]):
            assert getattr(gt, a)[i].tobytes() == want.tobytes(), a
        print("archive %d: scat_indices %s +/- %s, scat_amps %s s" % (
            i, gt.scat_indices[i], gt.scat_index_errs[i], gt.scat_amps[i]))
        y, e = gt.profile_fluxes[i], used(gt.profile_flux_errs[i])
        init = np.column_stack([[yy[ee > 0.0].mean() for yy, ee in zip(y, e)], np.zeros(3)])
        r = pplib.fit_powlaws(y, init, e, freqs, nu0)
        assert (r.n_used == 15).all()
        for a, want in zip(CHANFIT_LISTS["spect"], [r.amp, r.amp_err, r.alpha, r.alpha_err,
                                                    r.chi2 / r.dof]):
            assert getattr(gt, a)[i].tobytes() == want.tobytes(), a
    # an explicit nu_ref moves the amplitudes' reference, quietly
    capsys.readouterr()
    gt.get_channel_fits(nu_ref=1200.0, quiet=True)
    assert capsys.readouterr().out == ""
    assert len(gt.scat_nu_refs) == 2 and np.all(gt.scat_nu_refs[0] == 1200.0)


def test_get_channel_fits_wideband(eng, fake_archives, tmp_path):
    from pulseportraiture_amd import pptoas
    names, model = fake_archives
    gt = pptoas.GetTOAs(names, model, quiet=True)
    gt.get_TOAs(print_flux=True, quiet=True)
    before, tim = snapshot(gt), tim_text(gt, tmp_path / "a.tim")
    gt.get_channel_fits(quiet=True)
    same_snapshot(before, snapshot(gt))
    assert tim_text(gt, tmp_path / "b.tim") == tim
    for a in CHANFIT_LISTS["nb"] + CHANFIT_LISTS["scat"]:
        assert getattr(gt, a) == [], a
    for a in CHANFIT_LISTS["spect"]:
        v = getattr(gt, a)
        assert len(v) == 2 and all(x.shape == (3,) and np.isfinite(x).all() for x in v), a
    # without print_flux nothing is left to fit
    gt2 = pptoas.GetTOAs(names[:1], model, quiet=True)
    gt2.get_TOAs(quiet=True)
    gt2.get_channel_fits(quiet=True)
    for kind in CHANFIT_LISTS.values():
        for a in kind:
            assert getattr(gt2, a) == [], a
