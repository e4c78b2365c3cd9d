"""The automatic Gaussian-component search on the device
(pplib.auto_gaussian_profiles, ppf_gauss_bank) against its numpy + scipy
restatement (tests/auto_gauss_reference.py) and MINPACK fits started from the
true parameters (tests/golden/auto_gauss.npz, made by
tests/golden/make_golden_auto_gauss.py): the filter bank cell by cell, the
search end to end, batching, the model-building pipeline and the refusals."""
import os

import numpy as np
import pytest

from tests import auto_gauss_reference as R
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

Y = R.Y
FTOL = Y.FTOL
CONVERGED = (1, 2, 3)
CASES = {64: ["A1_64", "B3sep_64", "C2blend_64", "wrap_64", "noise_64"],
         128: ["C2tau_128", "C2taufit_128"],
         256: ["A1_256", "B3sep_256", "C2blend_256", "wrap_256", "ex3_256", "noise_256"]}
ALL = [n for names in CASES.values() for n in names]


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from pulseportraiture_amd.engine import get_engine
    return get_engine(0)


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(GOLDEN, "auto_gauss.npz"))


def _search(z, names):
    from pulseportraiture_amd import pplib
    how = {(float(z[n + "_tau"]), bool(z[n + "_fit_tau"])) for n in names}
    assert len(how) == 1
    tau, fit_tau = how.pop()
    return pplib.auto_gaussian_profiles([z[n + "_profile"] for n in names],
                                        [float(z[n + "_sigma"]) for n in names], tau=tau,
                                        fit_scattering=fit_tau)


@pytest.fixture(scope="module")
def singles(gpu, z):
    """Every golden case searched on its own, once."""
    return {n: _search(z, [n])[0] for n in ALL}


# -- 1. the bank ---------------------------------------------------------------
@pytest.mark.parametrize("name", ["wrap_64", "wrap_256", "C2blend_64", "C2blend_256",
                                  "C2tau_128"])
def test_bank_matches_numpy(gpu, z, name):
    """The s2 map of the first-stage residual to 1e-9 of its maximum (fp64
    sums of at most 1e5 terms, as test_gauss_eval_matches_numpy), the same
    best cell, amp to 1e-9; the grid runs from 2 / nbin to 0.25."""
    prof, err = z[name + "_profile"], float(z[name + "_sigma"])
    nbin, taun = len(prof), float(z[name + "_tau"]) / len(prof)
    resid = prof - np.mean(prof)
    wids = R.widths(nbin)
    assert wids[0] == 2.0 / nbin and wids[-1] == 0.25
    s2_ref, best_ref, idx_ref = R.bank(resid, err, taun, wids)
    best, idx, s2 = gpu.gauss_bank(resid[None], [err], [taun], wids, full=True)
    best, idx, s2 = best.cpu().numpy()[0], idx.cpu().numpy()[0], s2.cpu().numpy()[0]
    e_map = np.max(np.abs(s2 - s2_ref)) / s2_ref.max()
    e_amp = abs(best[3] / best_ref[3] - 1.0)
    print("%s: map %.2e  amp %.2e  best %s" % (name, e_map, e_amp, tuple(idx)))
    assert e_map <= 1e-9
    assert tuple(idx) == idx_ref
    assert e_amp <= 1e-9 and abs(best[0] / best_ref[0] - 1.0) <= 1e-9
    assert best[1] == best_ref[1] and best[2] == best_ref[2]
    assert best[0] == s2[idx[0], idx[1]] == s2.max()
    # without the map: the same answer
    b2, i2 = gpu.gauss_bank(resid[None], [err], [taun], wids)
    assert np.array_equal(b2.cpu().numpy()[0], best) and np.array_equal(i2.cpu().numpy()[0], idx)


def test_bank_ends_of_the_grid_and_nothing_positive(gpu, z):
    """A residual that is exactly a template of the narrowest (widest) width
    is found at that end of the grid; an all-negative residual gives -1."""
    from pulseportraiture_amd import pplib
    nbin = 128
    wids = R.widths(nbin)
    locs = pplib.get_bin_centers(nbin)
    for w, j in ((0, 5), (len(wids) - 1, 127)):
        resid = pplib.gen_gaussian_profile([0.0, 0.0, locs[j], wids[w], 0.7], nbin)
        best, idx = gpu.gauss_bank(resid[None], [0.01], [0.0], wids)
        best, idx = best.cpu().numpy()[0], idx.cpu().numpy()[0]
        assert tuple(idx) == (w, j)
        assert best[1] == locs[j] and best[2] == wids[w] and abs(best[3] / 0.7 - 1.0) <= 1e-9
    neg = -np.abs(z["C2tau_128_profile"]) - 1.0
    best, idx, s2 = gpu.gauss_bank(np.stack([neg, -neg]), [0.01, 0.01], [0.0, 0.0], wids,
                                   full=True)
    best, idx, s2 = best.cpu().numpy(), idx.cpu().numpy(), s2.cpu().numpy()
    assert tuple(idx[0]) == (-1, -1) and not np.any(best[0]) and not np.any(s2[0])
    assert idx[1, 0] >= 0 and best[1, 0] > 0


def test_bank_is_independent_of_the_batch(gpu, z):
    """Seven profiles (two of them scattered) in one call, bitwise the single
    calls and a repeat; the same with a workspace too small for all seven."""
    nbin = 128
    wids = R.widths(nbin, 5)
    base = z["C2tau_128_profile"] - np.mean(z["C2tau_128_profile"])
    rows = np.stack([np.roll(base, 9 * i) * (1.0 + 0.1 * i) for i in range(7)])
    errs = 0.01 * (1.0 + np.arange(7))
    taun = np.array([0.0, 2.5 / nbin, 0.0, 0.0, 1.0 / nbin, 0.0, 0.0])

    def run(sel):
        out = gpu.gauss_bank(rows[sel], errs[sel], taun[sel], wids, full=True)
        return [v.cpu().numpy() for v in out]

    every = list(range(7))
    batch, again = run(every), run(every)
    for a, b in zip(batch, again):
        assert np.array_equal(a, b)
    for i in every:
        for a, b in zip(batch, run([i])):
            assert np.array_equal(a[i], b[0]), i
    # a profile's scratch is 65 spectrum cells of 16 B and 5 records of 32 B:
    # 4 KB cannot hold all seven, so the call is split over profiles
    gpu.set_workspace_limit(4096)
    try:
        split = run(every)
    finally:
        gpu.set_workspace_limit(32 << 30)
    for a, b in zip(batch, split):
        assert np.array_equal(a, b)


# -- 2. the search -------------------------------------------------------------
def _check_search(z, name, r):
    """The bounds of tests/test_gpu_ppgauss.py::_check_fit with the
    restatement as "ref": no more than twice as far from the minimum as the
    restatement's own run, or what the stopping rule itself guarantees."""
    ngauss = int(z[name + "_ngauss"])
    assert r.ngauss == ngauss and len(r.fitted_params) == 2 + 3 * ngauss
    assert len(r.history) == int(z[name + "_nstage"]) == ngauss + 1
    assert [h.accepted for h in r.history] == [True] * ngauss + [False]
    assert r.history[-1].stop == "min_snr" and r.history[-1].s2 < 25.0
    assert all(h.stop is None and h.s2 >= 25.0 and len(h.candidate) == 3
               and h.chi2_new + 3 * np.log(len(r.residuals)) < h.chi2_old
               for h in r.history[:-1])
    if not ngauss:
        assert r.lm_results is None and r.fitted_params[0] == np.mean(z[name + "_profile"])
        return
    p_t, s_t, c_t = z[name + "_p_truth"], z[name + "_sig_truth"], float(z[name + "_chi2_truth"])
    p_r, c_r = z[name + "_p_ref"], float(z[name + "_chi2_ref"])
    free = s_t > 0
    order = R.match_order(r.fitted_params, p_t)
    p, sig = R.reorder(r.fitted_params, order), R.reorder(r.fit_errs, order)
    p_r = R.reorder(p_r, R.match_order(p_r, p_t))
    d_chi2, d_chi2_ref = r.chi2 - c_t, c_r - c_t
    dist = np.max(np.abs(R.delta(p, p_t))[free] / s_t[free])
    dist_ref = np.max(np.abs(R.delta(p_r, p_t))[free] / s_t[free])
    e_sig = np.max(np.abs(sig[free] / s_t[free] - 1.0))
    print("%s: chi2 - chi2_truth %.3e (ref %.3e)  max|p - p_truth|/sigma %.3e (ref %.3e)  "
          "errs rel %.2e" % (name, d_chi2, d_chi2_ref, dist, dist_ref, e_sig))
    assert r.lm_results.status in CONVERGED and r.dof == int(z[name + "_dof"])
    assert d_chi2 <= max(2.0 * d_chi2_ref, FTOL * c_t)
    assert dist <= max(2.0 * dist_ref, np.sqrt(FTOL * c_t))
    assert e_sig <= 1e-3
    if not z[name + "_fit_tau"]:
        assert p[1] == float(z[name + "_tau"]) and sig[1] == 0.0
    # components in order of discovery: the first stage's candidate is the first
    assert abs((r.fitted_params[2] - r.history[0].candidate[0] + 0.5) % 1.0 - 0.5) < 0.05


@pytest.mark.parametrize("name", ALL)
def test_search_end_to_end(singles, z, name):
    from pulseportraiture_amd import pplib
    r = singles[name]
    _check_search(z, name, r)
    prof = z[name + "_profile"]
    model = pplib.gen_gaussian_profile(r.fitted_params, len(prof)) if r.ngauss else \
        r.fitted_params[0]
    assert np.array_equal(r.residuals, prof - model)
    assert abs(np.sum((r.residuals / float(z[name + "_sigma"])) ** 2) - r.chi2) <= 1e-9 * r.chi2


# -- 3. batching ---------------------------------------------------------------
def _same(a, b):
    assert a.ngauss == b.ngauss and a.chi2 == b.chi2 and a.dof == b.dof
    for k in ("fitted_params", "fit_errs", "residuals"):
        assert np.array_equal(a[k], b[k]), k
    assert len(a.history) == len(b.history)
    for h, g in zip(a.history, b.history):
        assert h.s2 == g.s2 and h.stop == g.stop and h.accepted == g.accepted
        # (a stage that stops without a refit has chi2_new NaN and no candidate)
        assert np.array_equal(h.chi2_new, g.chi2_new, equal_nan=True) and h.chi2_old == g.chi2_old
        assert (h.candidate is None and g.candidate is None) or \
            np.array_equal(h.candidate, g.candidate)


@pytest.mark.parametrize("nbin", [64, 256])
def test_batch_is_bitwise_single_calls(gpu, singles, z, nbin):
    """All cases of one nbin in one call -- they leave at different stages --
    equal the single calls bit for bit, also with the workspace split."""
    names = CASES[nbin]
    assert len({int(z[n + "_nstage"]) for n in names}) >= 3
    batch = _search(z, names)
    for n, b in zip(names, batch):
        _same(b, singles[n])
    gpu.set_workspace_limit(1 << 20)
    try:
        split = _search(z, names)
    finally:
        gpu.set_workspace_limit(32 << 30)
    for n, b in zip(names, split):
        _same(b, singles[n])


# -- 4. the pipeline -----------------------------------------------------------
def _archive(z, name, scale=1.0):
    """The pipeline fixture as load_data's dict archive."""
    from pulseportraiture_amd.mjd import MJD
    freqs, port, errs = z["pipe_freqs"], z["pipe_data"] * scale, z["pipe_errs"] * scale
    snrs = port.max(axis=1) / errs
    return dict(subints=port[None, None].copy(), freqs=freqs[None].copy(),
                weights=np.ones((1, len(freqs))), SNRs=snrs[None, None].copy(),
                noise_stds=errs[None, None].copy(), Ps=[0.003], epochs=[MJD(57300.0)], bw=400.0,
                nu0=1400.0, source="J0000+0000", filename=name)


def _portrait_order(p, p_t):
    """p (DC, tau, 6 per component, alpha) with its components in p_t's order."""
    prof = lambda v: np.concatenate([v[:2], v[2:-1].reshape(-1, 6)[:, 0::2].ravel()])  # noqa: E731
    order = R.match_order(prof(p), prof(p_t))
    return np.concatenate([p[:2], p[2:-1].reshape(-1, 6)[order].ravel(), p[-1:]]), order


def test_pipeline_make_gaussian_model(gpu, z, tmp_path):
    """make_gaussian_model(max_ngauss=6) on a three-component portrait with
    no typed parameter: three components, a .gmodel that reads back to the
    fit, and the minimum of the portrait fit started from the truth."""
    from pulseportraiture_amd import ppgauss, pplib
    out = str(tmp_path / "auto.gmodel")
    dp = ppgauss.DataPortrait(_archive(z, "auto_pipe.fits"), quiet=True)
    dp.make_gaussian_model(max_ngauss=6, writemodel=True, outfile=out, quiet=True)
    assert dp.ngauss == 3 and dp.profile_fit.ngauss == 3 and len(dp.profile_fit.history) == 4
    assert dp.fgp.lm_results.status in CONVERGED
    # component 0 is the strongest
    assert dp.init_params[4] == max(dp.init_params[4::3])
    p_t, s_t, c_t = z["pipe_p_truth"], z["pipe_sig_truth"], float(z["pipe_chi2_truth"])
    p_r, c_r = z["pipe_p_ref"], float(z["pipe_chi2_ref"])
    free = z["pipe_flags"] != 0
    p_fit = np.append(dp.model_params, dp.scattering_index)
    p, order = _portrait_order(p_fit, p_t)
    sig = np.append(dp.model_param_errs, dp.scattering_index_err)
    sig = np.concatenate([sig[:2], sig[2:-1].reshape(-1, 6)[order].ravel(), sig[-1:]])

    def dist_to_truth(q):
        d = q - p_t
        d[2:-1:6] = (d[2:-1:6] + 0.5) % 1.0 - 0.5
        return np.max(np.abs(d)[free] / s_t[free])

    d_chi2, d_chi2_ref = dp.chi2 - c_t, c_r - c_t
    dist, dist_ref = dist_to_truth(p), dist_to_truth(p_r)
    e_sig = np.max(np.abs(sig[free] / s_t[free] - 1.0))
    print("pipeline: chi2 - chi2_truth %.3e (ref %.3e)  max|p - p_truth|/sigma %.3e (ref %.3e)  "
          "errs rel %.2e" % (d_chi2, d_chi2_ref, dist, dist_ref, e_sig))
    assert dp.dof == int(z["pipe_dof"])
    assert d_chi2 <= max(2.0 * d_chi2_ref, FTOL * c_t)
    assert dist <= max(2.0 * dist_ref, np.sqrt(FTOL * c_t))
    assert e_sig <= 1e-3
    assert np.all(sig[~free] == 0.0) and p[1] == 0.0 and p[-1] == p_t[-1]
    # the written model reads back to the fitted parameters (8 decimals; locs
    # wrapped into [0, 1), tau in seconds)
    name, code, nu_ref, ngauss, params, flags, alpha, fit_alpha = pplib.read_model(out, quiet=True)
    assert (code, ngauss, nu_ref, alpha, fit_alpha) == ("000", 3, 1400.0, p_fit[-1], 0)
    want = dp.model_params.copy()
    want[2::6] = np.where(want[2::6] >= 1.0, want[2::6] % 1, want[2::6])
    want[1] *= 0.003 / 256
    assert np.all(np.abs(params - want) <= 0.5e-8 + 1e-15)
    assert np.array_equal(flags, dp.fit_flags) and flags[1] == 0


def test_batch_helper_equals_single_calls(gpu, z, tmp_path):
    """make_gaussian_models on two portraits: one search call for both
    reference profiles, bitwise the single calls."""
    from pulseportraiture_amd import ppgauss
    arch = [_archive(z, "a.fits"), _archive(z, "b.fits", scale=1.7)]
    batch = [ppgauss.DataPortrait(a, quiet=True) for a in arch]
    outs = [str(tmp_path / "a.gmodel"), str(tmp_path / "b.gmodel")]
    ppgauss.make_gaussian_models(batch, max_ngauss=6, writemodel=True, outfiles=outs, quiet=True)
    for a, dpb, o in zip(arch, batch, outs):
        dps = ppgauss.DataPortrait(a, quiet=True)
        single = o + ".single"
        dps.make_gaussian_model(max_ngauss=6, writemodel=True, outfile=single, quiet=True)
        assert dps.ngauss == dpb.ngauss == 3
        for name in ("init_params", "init_param_errs", "model_params", "model_param_errs",
                     "model"):
            assert np.array_equal(getattr(dps, name), getattr(dpb, name)), name
        assert dps.chi2 == dpb.chi2 and dps.dof == dpb.dof
        assert open(single).read() == open(o).read()


# -- 5. refusals ---------------------------------------------------------------
def test_refusals(gpu, z):
    from pulseportraiture_amd import ppgauss, pplib
    from pulseportraiture_amd.engine import PPFitError
    with pytest.raises(PPFitError, match="error -3"):  # nbin no power of two
        gpu.gauss_bank(np.zeros((1, 100)), [1.0], [0.0], R.widths(128))
    with pytest.raises(PPFitError, match="error -3"):  # more than 64 widths
        gpu.gauss_bank(np.zeros((1, 128)), [1.0], [0.0], np.linspace(0.02, 0.25, 65))
    with pytest.raises(PPFitError, match="error -3"):
        pplib.auto_gaussian_profile(np.zeros(100), 1.0)
    with pytest.raises(ValueError):
        pplib.auto_gaussian_profile(z["A1_64_profile"], 0.01, max_ngauss=17)
    # a noise-only portrait: nothing to model
    rng = np.random.default_rng(41)
    noise = dict(_archive(z, "noise.fits"))
    noise["subints"] = 0.02 + z["pipe_errs"][None, None, :, None] * rng.standard_normal(
        (1, 1, 16, 256))
    dp = ppgauss.DataPortrait(noise, quiet=True)
    with pytest.raises(RuntimeError, match="noise.fits"):
        dp.make_gaussian_model(max_ngauss=6, quiet=True)
    with pytest.raises(NotImplementedError):  # none of the three given: as before
        ppgauss.DataPortrait(_archive(z, "c.fits"), quiet=True).make_gaussian_model(quiet=True)
