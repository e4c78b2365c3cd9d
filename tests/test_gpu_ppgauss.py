"""ppgauss on the device against the CPU yardstick of
tests/golden/make_golden_ppgauss.py: ppf_gauss_eval against the numpy
restatement of the analytic Jacobian, the fits against scipy's MINPACK runs
(ref: leastsq at its defaults with forward differences, what the reference
does; truth: the analytic Jacobian at ftol = xtol = 1e-13), batching, the
model-building pipeline and the refusals."""
import importlib.util
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

FTOL = 1.49012e-8
CONVERGED = (1, 2, 3)


def _yardstick():
    spec = importlib.util.spec_from_file_location(
        "make_golden_ppgauss", os.path.join(GOLDEN, "make_golden_ppgauss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


Y = _yardstick()


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from pulseportraiture_amd.engine import get_engine
    return get_engine(0)


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(GOLDEN, "ppgauss.npz"))


# DC, tau, (loc, dloc, wid, dwid, amp, damp) per component, alpha; one
# component within a bin of phase 0 (the wrap is crossed)
P2_000 = np.array([0.02, 0.0, 0.40, 0.004, 0.050, -0.3, 1.0, -1.2,
                   0.004, -0.003, 0.030, 0.2, 0.6, -0.8, -4.0])
P2_111 = np.array([0.02, 0.0, 0.40, 2e-5, 0.050, -1e-5, 1.0, -4e-4,
                   0.004, -1e-5, 0.030, 1e-5, 0.6, 2e-4, -4.0])
P3_000 = np.array([0.01, 1.5, 0.30, 0.002, 0.040, 0.1, 1.0, -1.0, 0.999, 0.001, 0.020, -0.2, 0.5,
                   0.5, 0.62, 0.0, 0.10, 0.3, 0.3, -2.0, -3.5])
EVAL_CASES = [("8x64_000_tau0", "000", P2_000, 0.0, 8, 64),
              ("8x64_111_tau0", "111", P2_111, 0.0, 8, 64),
              ("8x64_000_tau2.5", "000", P2_000, 2.5, 8, 64),
              ("8x64_111_tau2.5", "111", P2_111, 2.5, 8, 64),
              ("5x128_3comp", "000", P3_000, 1.5, 5, 128)]


@pytest.mark.parametrize("case", EVAL_CASES, ids=[c[0] for c in EVAL_CASES])
def test_gauss_eval_matches_numpy(gpu, case):
    """chi2, J^T r and J^T J at the true parameters and at a perturbed point,
    to 1e-9 of the largest entry (fp64 sums of at most 1e5 terms)."""
    _, code, p, tau, nchan, nbin = case
    p = p.copy()
    p[1] = tau
    freqs, data, errs = Y.synth(code, p, nchan, nbin, 1500.0, 0.02, 5, 1200.0, 1800.0)
    rng = np.random.default_rng(6)
    pert = p * (1.0 + 0.02 * rng.uniform(-1, 1, len(p)))
    for point in (p, pert):
        chi2, jtr, jtj = gpu.gauss_eval(data, freqs, errs, point, code, 1500.0)
        c_ref, g_ref, h_ref = Y.eval_numpy(code, point, data, errs, freqs, 1500.0)
        chi2, jtr, jtj = chi2.cpu().numpy()[0], jtr.cpu().numpy()[0], jtj.cpu().numpy()[0]
        e_c = abs(chi2 - c_ref) / c_ref
        e_g = np.max(np.abs(jtr - g_ref)) / np.max(np.abs(g_ref))
        e_h = np.max(np.abs(jtj - h_ref)) / np.max(np.abs(h_ref))
        # entry by entry on the scale of its own row and column as well
        # (alpha's column is zero at tau = 0)
        d = np.sqrt(np.diag(h_ref))
        d[d == 0.0] = 1.0
        e_hs = np.max(np.abs(jtj - h_ref) / np.outer(d, d))
        print(case[0], "chi2 %.2e  JTr %.2e  JTJ %.2e  JTJ scaled %.2e" % (e_c, e_g, e_h, e_hs))
        assert e_c <= 1e-9 and e_g <= 1e-9 and e_h <= 1e-9 and e_hs <= 1e-9
        assert np.array_equal(jtj, jtj.T)


def _fit_case(z, name):
    return dict(code=str(z[name + "_code"]), data=z[name + "_data"], errs=z[name + "_errs"],
                freqs=z[name + "_freqs"], nu_ref=float(z[name + "_nu_ref"]),
                init=z[name + "_init"], flags=z[name + "_flags"])


def _check_fit(z, name, p, sig, chi2, dof, status):
    """The issue's bounds: no more than twice as far from the minimum as the
    reference's own run, or what the stopping rule itself guarantees."""
    free = z[name + "_flags"] != 0
    p_t, s_t, c_t = z[name + "_p_truth"], z[name + "_sig_truth"], float(z[name + "_chi2_truth"])
    p_r, c_r = z[name + "_p_ref"], float(z[name + "_chi2_ref"])
    d_chi2, d_chi2_ref = chi2 - c_t, c_r - c_t
    dist = np.max(np.abs(p - p_t)[free] / s_t[free])
    dist_ref = np.max(np.abs(p_r - p_t)[free] / s_t[free])
    e_sig = np.max(np.abs(sig[free] / s_t[free] - 1.0))
    print("%s: chi2 - chi2_truth %.3e (ref %.3e)  max|p - p_truth|/sigma %.3e (ref %.3e)  "
          "errs rel %.2e  status %d" % (name, d_chi2, d_chi2_ref, dist, dist_ref, e_sig, status))
    assert status in CONVERGED
    assert dof == int(z[name + "_dof"])
    assert d_chi2 <= max(2.0 * d_chi2_ref, FTOL * c_t)
    assert dist <= max(2.0 * dist_ref, np.sqrt(FTOL * c_t))
    assert e_sig <= 1e-3
    assert np.all(sig[~free] == 0.0) and np.array_equal(p[~free], z[name + "_init"][~free])


@pytest.mark.parametrize("name", ["port_notau", "port_tau"])
def test_fit_portrait_matches_minpack(gpu, z, name):
    from pulseportraiture_amd import pplib
    c = _fit_case(z, name)
    nbin = c["data"].shape[1]
    r = pplib.fit_gaussian_portrait(c["code"], c["data"], c["init"][:-1], c["init"][-1],
                                    np.outer(c["errs"], np.ones(nbin)), c["flags"][:-1],
                                    bool(c["flags"][-1]), pplib.get_bin_centers(nbin), c["freqs"],
                                    c["nu_ref"])
    p = np.append(r.fitted_params, r.scattering_index)
    sig = np.append(r.fit_errs, r.scattering_index_err)
    _check_fit(z, name, p, sig, r.chi2, r.dof, r.lm_results.status)
    assert r.lm_results.nfev > 1 and r.lm_results.covar.shape == (len(p), len(p))
    assert np.allclose(np.sqrt(np.diag(r.lm_results.covar)), sig, rtol=1e-12)


def test_zero_column_stays_put(gpu, z):
    """tau free at 0 sits on its bound, where the transform's gradient is 0:
    its column of J is zero, it stays put (no NaN), the others converge as
    before, and with J^T J singular every error is 0.0."""
    c = _fit_case(z, "port_notau")
    flags = c["flags"].copy()
    flags[1] = 1
    out = gpu.gauss_fit(c["data"], c["freqs"], c["errs"], c["init"], flags, c["code"], c["nu_ref"])
    p, sig = out["params"].cpu().numpy()[0], out["param_errs"].cpu().numpy()[0]
    info = out["info"].cpu().numpy()[0]
    assert info[0] in CONVERGED and info[3] == int(flags.sum())
    assert p[1] == 0.0 and np.all(np.isfinite(p)) and np.all(sig == 0.0)
    free = c["flags"] != 0
    dist = np.max(np.abs(p - z["port_notau_p_truth"])[free] / z["port_notau_sig_truth"][free])
    assert dist <= np.sqrt(FTOL * float(z["port_notau_chi2_truth"]))


def test_fit_profile_matches_minpack(gpu, z):
    """fit_gaussian_profile at nbin 256 with scattering: the same solver
    with one channel."""
    from pulseportraiture_amd import pplib
    name = "profile_tau"
    c = _fit_case(z, name)
    keep = [0, 1, 2, 4, 6]
    r = pplib.fit_gaussian_profile(c["data"][0], c["init"][keep], c["errs"][0] * np.ones(256),
                                   None, True)
    p, sig = c["init"].copy(), np.zeros(len(c["init"]))
    p[keep], sig[keep] = r.fitted_params, r.fit_errs
    _check_fit(z, name, p, sig, r.chi2, r.dof, r.lm_results.status)
    model = pplib.gen_gaussian_profile(r.fitted_params, 256)
    assert np.array_equal(r.residuals, c["data"][0] - model)
    assert abs(np.sum((r.residuals / c["errs"][0]) ** 2) - r.chi2) <= 1e-9 * r.chi2


def test_batch_is_bitwise_single_calls(gpu, z):
    """Three portraits in one call equal three single calls bit for bit, and
    a repeated call equals itself."""
    a, b = _fit_case(z, "port_notau"), _fit_case(z, "port_tau")
    c = dict(a, data=a["data"][::-1].copy(), freqs=a["freqs"][::-1].copy(),
             errs=a["errs"][::-1].copy())
    cases = [a, b, c]

    def run(cs):
        out = gpu.gauss_fit(np.stack([x["data"] for x in cs]), np.stack([x["freqs"] for x in cs]),
                            np.stack([x["errs"] for x in cs]), np.stack([x["init"] for x in cs]),
                            np.stack([x["flags"] for x in cs]), [x["code"] for x in cs],
                            [x["nu_ref"] for x in cs])
        return {k: v.cpu().numpy() for k, v in out.items()}

    batch, again = run(cases), run(cases)
    for k in batch:
        assert np.array_equal(batch[k], again[k], equal_nan=True), k
    assert np.all(np.isin(batch["info"][:, 0], CONVERGED))
    for i, x in enumerate(cases):
        one = run([x])
        for k in batch:
            assert np.array_equal(batch[k][i], one[k][0], equal_nan=True), (k, i)
    # a workspace limit that holds one portrait splits the call over portraits
    gpu.set_workspace_limit(1 << 20)
    try:
        split = run(cases)
    finally:
        gpu.set_workspace_limit(32 << 30)
    for k in batch:
        assert np.array_equal(batch[k], split[k], equal_nan=True), k


def _archive(z, name="ppgauss_pipe.fits", scale=1.0):
    """The pipeline fixture as load_data's dict archive."""
    from pulseportraiture_amd.mjd import MJD
    freqs, port, errs = z["pipe_freqs"], z["pipe_data"] * scale, z["pipe_errs"] * scale
    snrs = port.max(axis=1) / errs
    return dict(subints=port[None, None].copy(), freqs=freqs[None].copy(),
                weights=np.ones((1, len(freqs))), SNRs=snrs[None, None].copy(),
                noise_stds=errs[None, None].copy(), Ps=[0.003], epochs=[MJD(57300.0)], bw=400.0,
                nu0=1400.0, source="J0000+0000", filename=name)


def _start_model(tmp_path, name="start.gmodel"):
    """example.gmodel with TAU = 0 fixed (at its bound lmfit's transform has
    no gradient)."""
    from pulseportraiture_amd import pplib
    mf = os.path.join(os.path.dirname(pplib.__file__), "data", "example.gmodel")
    mname, code, nu_ref, ngauss, params, flags, alpha, fit_alpha = pplib.read_model(mf)
    flags[1] = 0
    out = str(tmp_path / name)
    pplib.write_model(out, mname, code, nu_ref, params, flags, alpha, fit_alpha, quiet=True)
    return out


def test_pipeline_make_gaussian_model(gpu, z, tmp_path):
    """make_gaussian_model from a model file on a portrait of example.gmodel
    plus seeded noise: the written model, read back and rendered, matches
    truth's; GetTOAs runs with it; check_convergence is truthy."""
    from pulseportraiture_amd import archive, ppgauss, pplib, pptoas
    from pulseportraiture_amd.mjd import MJD
    start = _start_model(tmp_path)
    out = str(tmp_path / "fitted.gmodel")
    dp = ppgauss.DataPortrait(_archive(z), quiet=True)
    dp.make_gaussian_model(modelfile=start, niter=2, writemodel=True, outfile=out,
                           writeerrfile=True, quiet=True)
    assert dp.cnvrgnc and dp.fgp.lm_results.status in CONVERGED
    assert os.path.exists(out) and os.path.exists(out + "_errs")
    p_t, s_t, c_t = z["pipe_p_truth"], z["pipe_sig_truth"], float(z["pipe_chi2_truth"])
    name, code, nu_ref, ngauss, params, flags, alpha, fit_alpha = pplib.read_model(out)
    free = np.append(flags, fit_alpha) != 0
    p = np.append(params, alpha)
    p[1] *= 256 / 0.003
    # the file holds 8 decimals: half a unit of the last one is allowed for
    tol = np.sqrt(FTOL * c_t) * s_t[free] + 0.5e-8
    print("pipeline: max |p - p_truth| / sigma = %.3e"
          % np.max(np.abs(p - p_t)[free] / s_t[free]))
    assert np.all(np.abs(p - p_t)[free] <= tol)
    phases, freqs = pplib.get_bin_centers(256), z["pipe_freqs"]
    ours = pplib.gen_gaussian_portrait(code, p[:-1], p[-1], phases, freqs, nu_ref)
    truth = pplib.gen_gaussian_portrait(code, p_t[:-1], p_t[-1], phases, freqs, nu_ref)
    _, jac = Y.model_and_jac(code, p_t, 256, freqs, nu_ref)
    bound = np.sum(np.abs(jac[free]) * tol[:, None, None], axis=0)
    assert np.all(np.abs(ours - truth) <= bound + 1e-12)
    # TOAs with the written model
    nsub = 2
    b = dict(subints=np.tile(z["pipe_data"][None, None], (nsub, 1, 1, 1)),
             freqs=np.tile(freqs, (nsub, 1)), weights=np.ones((nsub, len(freqs))),
             SNRs=np.ones((nsub, 1, len(freqs))), Ps=np.full(nsub, 0.003),
             epochs=[MJD(57300.0 + 0.001 * i) for i in range(nsub)], DM=10.0, bw=400.0,
             nu0=1400.0, telescope="GBT", telescope_code="1", subtimes=[30.0] * nsub)
    archive.register_archive("ppgauss_toas.fits", b)
    try:
        gt = pptoas.GetTOAs(["ppgauss_toas.fits"], out, quiet=True)
        gt.get_TOAs(quiet=True)
    finally:
        archive.unregister_archive("ppgauss_toas.fits")
    assert len(gt.TOA_list) == nsub and np.all(np.isfinite(gt.phis[0]))
    assert np.all(gt.phi_errs[0] > 0) and np.all(np.isfinite(gt.DMs[0]))


def test_auto_gauss_start(gpu, z):
    """The non-interactive start: one component placed by fit_phase_shift and
    fitted to the profile, then the portrait fit."""
    from pulseportraiture_amd import ppgauss
    dp = ppgauss.DataPortrait(_archive(z), quiet=True)
    dp.make_gaussian_model(auto_gauss=0.03, quiet=True)
    assert dp.ngauss == 1 and dp.fgp.lm_results.status in CONVERGED
    assert len(dp.model_params) == 8 and dp.fit_flags[1] == 0
    assert 0.2 < dp.model_params[2] % 1 < 0.26 and dp.model_params[6] > 0
    assert dp.model.shape == dp.port.shape and np.isfinite(dp.chi2)


def test_batch_helper_equals_single_calls(gpu, z, tmp_path):
    from pulseportraiture_amd import ppgauss
    start = _start_model(tmp_path)
    arch = [_archive(z, "a.fits"), _archive(z, "b.fits", scale=1.7)]
    batch = [ppgauss.DataPortrait(a, quiet=True) for a in arch]
    outs = [str(tmp_path / "a.gmodel"), str(tmp_path / "b.gmodel")]
    res = ppgauss.make_gaussian_models(batch, modelfiles=[start, start], niter=1, writemodel=True,
                                       outfiles=outs, quiet=True)
    assert res[0] is batch[0]
    for a, dpb, o in zip(arch, batch, outs):
        dps = ppgauss.DataPortrait(a, quiet=True)
        single = o + ".single"
        dps.make_gaussian_model(modelfile=start, niter=1, writemodel=True, outfile=single,
                                quiet=True)
        for name in ("model_params", "model_param_errs", "model", "modelx", "port", "portx"):
            assert np.array_equal(getattr(dps, name), getattr(dpb, name)), name
        assert dps.chi2 == dpb.chi2 and dps.dof == dpb.dof and dps.phi == dpb.phi
        assert open(single).read() == open(o).read()


def test_refusals(gpu):
    from pulseportraiture_amd.engine import PPFitError
    freqs = np.linspace(1200.0, 1800.0, 4)
    for ngauss, nbin in ((17, 64), (1, 100)):
        p = np.concatenate([[0.0, 0.0], np.tile([0.5, 0.0, 0.05, 0.0, 1.0, 0.0], ngauss), [-4.0]])
        data = np.zeros((4, nbin))
        with pytest.raises(PPFitError, match="error -3"):
            gpu.gauss_eval(data, freqs, np.ones(4), p, "000", 1500.0)
        with pytest.raises(PPFitError, match="error -3"):
            gpu.gauss_fit(data, freqs, np.ones(4), p, np.ones(len(p)), "000", 1500.0)
