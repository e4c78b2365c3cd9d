"""Joint fits of several receivers' portraits on the device against the CPU
yardstick of tests/golden/make_golden_ppgauss_join.py: ppf_gauss_eval_join
against the numpy restatement of the rotated model and its Jacobian, the fits
against scipy's MINPACK runs, the unchanged no-join path, batching, the
metafile pipeline of ppgauss and the refusals."""
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
        "make_golden_ppgauss_join", os.path.join(GOLDEN, "make_golden_ppgauss_join.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


YJ = _yardstick()


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from pulseportraiture_amd.engine import get_engine
    return get_engine(0)


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(GOLDEN, "ppgauss_join.npz"))


@pytest.fixture(scope="module")
def z0():
    return np.load(os.path.join(GOLDEN, "ppgauss.npz"))


# DC, tau, (loc, dloc, wid, dwid, amp, damp) per component; the 0.030 wide
# component is two bins wide at nbin 64 and within a bin of phase 0
P2_000 = [0.02, 0.0, 0.40, 0.004, 0.050, -0.3, 1.0, -1.2, 0.004, -0.003, 0.030, 0.2, 0.6, -0.8]
P2_111 = [0.02, 0.0, 0.40, 2e-5, 0.050, -1e-5, 1.0, -4e-4, 0.004, -1e-5, 0.030, 1e-5, 0.6, 2e-4]
P3_000 = [0.01, 1.5, 0.30, 0.002, 0.040, 0.1, 1.0, -1.0, 0.999, 0.001, 0.020, -0.2, 0.5, 0.5, 0.62,
          0.0, 0.10, 0.3, 0.3, -2.0]
J2 = [0.21, 1.0, 1.3, -2.0]  # (phase, DM) per group: theta beyond one turn
J3 = [0.21, 1.0, 1.3, -2.0, -0.4, 6.0]
G2 = [np.arange(0, 8, 2), np.arange(1, 8, 2)]  # interleaved
G3 = [np.array([0, 3]), np.array([2]), np.array([1, 4])]  # one group of a single channel
EVAL_CASES = [("8x64_000_tau0", "000", P2_000, J2, G2, 0.0, 8, 64),
              ("8x64_111_tau0", "111", P2_111, J2, G2, 0.0, 8, 64),
              ("8x64_000_tau2.5", "000", P2_000, J2, G2, 2.5, 8, 64),
              ("8x64_111_tau2.5", "111", P2_111, J2, G2, 2.5, 8, 64),
              ("5x128_3comp_3groups", "000", P3_000, J3, G3, 1.5, 5, 128)]
PERIOD = 0.005


@pytest.mark.parametrize("case", EVAL_CASES, ids=[c[0] for c in EVAL_CASES])
def test_gauss_eval_join_matches_numpy(gpu, case):
    """chi2, J^T r and J^T J at the true parameters and at a 2 % perturbed
    point, to 1e-9 of the largest entry (the bounds of
    test_gauss_eval_matches_numpy)."""
    from pulseportraiture_amd import pplib
    _, code, p0, jp, groups, tau, nchan, nbin = case
    p = np.array(list(p0) + list(jp) + [-4.0 if len(p0) == 14 else -3.5])
    p[1] = tau
    njoin = len(groups)
    freqs = np.linspace(1200.0, 1800.0, nchan)
    data, errs = YJ.synth(code, p, freqs, nbin, 1500.0, groups, PERIOD, 0.02, 5)
    join_of = YJ.join_of(groups, nchan)
    dm_coef = pplib.join_dm_coef(PERIOD, freqs, 1500.0)
    theta, _ = YJ.rotations(jp, groups, PERIOD, freqs, 1500.0)
    assert np.max(np.abs(theta)) > 1.0
    rng = np.random.default_rng(6)
    pert = p * (1.0 + 0.02 * rng.uniform(-1, 1, len(p)))
    for point in (p, pert):
        chi2, jtr, jtj = gpu.gauss_eval_join(data, freqs, errs, point, code, 1500.0, join_of,
                                             dm_coef, njoin)
        c_ref, g_ref, h_ref = YJ.eval_numpy(code, point, data, errs, freqs, 1500.0, groups, PERIOD)
        chi2, jtr, jtj = chi2.cpu().numpy()[0], jtr.cpu().numpy()[0], jtj.cpu().numpy()[0]
        e_c = abs(chi2 - c_ref) / c_ref
        e_g = np.max(np.abs(jtr - g_ref)) / np.max(np.abs(g_ref))
        e_h = np.max(np.abs(jtj - h_ref)) / np.max(np.abs(h_ref))
        d = np.sqrt(np.diag(h_ref))
        d[d == 0.0] = 1.0
        e_hs = np.max(np.abs(jtj - h_ref) / np.outer(d, d))
        print(case[0], "chi2 %.2e  JTr %.2e  JTJ %.2e  JTJ scaled %.2e" % (e_c, e_g, e_h, e_hs))
        assert e_c <= 1e-9 and e_g <= 1e-9 and e_h <= 1e-9 and e_hs <= 1e-9
        assert np.array_equal(jtj, jtj.T)


def test_zero_join_equals_no_join_fit(gpu, z0):
    """Join parameters of zero, all fixed: a unit phasor and a zero
    chain-rule coefficient change no sum, so the joint fit of port_tau is
    gauss_fit's, bit for bit."""
    from pulseportraiture_amd import pplib
    name = "port_tau"
    data, errs, freqs = z0[name + "_data"], z0[name + "_errs"], z0[name + "_freqs"]
    init, flags = z0[name + "_init"], z0[name + "_flags"]
    code, nu_ref = str(z0[name + "_code"]), float(z0[name + "_nu_ref"])
    plain = gpu.gauss_fit(data, freqs, errs, init, flags, code, nu_ref)
    join_of = np.arange(len(freqs)) % 2
    init_j = np.concatenate([init[:-1], np.zeros(4), init[-1:]])
    flags_j = np.concatenate([flags[:-1], np.zeros(4, dtype=int), flags[-1:]])
    joint = gpu.gauss_fit_join(data, freqs, errs, init_j, flags_j, code, nu_ref, join_of,
                               pplib.join_dm_coef(PERIOD, freqs, nu_ref), 2)
    plain = {k: v.cpu().numpy()[0] for k, v in plain.items()}
    joint = {k: v.cpu().numpy()[0] for k, v in joint.items()}
    keep = np.r_[0:len(init) - 1, len(init_j) - 1]
    assert plain["info"][0] in CONVERGED
    assert np.array_equal(joint["params"][keep], plain["params"])
    assert np.array_equal(joint["param_errs"][keep], plain["param_errs"])
    assert np.array_equal(joint["params"][len(init) - 1:-1], np.zeros(4))
    assert np.array_equal(joint["param_errs"][len(init) - 1:-1], np.zeros(4))
    assert np.array_equal(joint["chi2"], plain["chi2"])
    assert np.array_equal(joint["info"], plain["info"])  # status, nfev, dof, nfree


def _fit_case(z, name):
    src = str(z[name + "_data_of"])
    join_of = z[name + "_join_of"]
    njoin = int(join_of.max()) + 1
    return dict(code=str(z[name + "_code"]), data=z[src + "_data"], errs=z[src + "_errs"],
                freqs=z[src + "_freqs"], nu_ref=float(z[name + "_nu_ref"]), P=float(z[name + "_P"]),
                init=z[name + "_init"], flags=z[name + "_flags"], join_of=join_of, njoin=njoin,
                groups=[np.flatnonzero(join_of == g) for g in range(njoin)])


def _check_fit(z, name, p, sig, chi2, dof, status):
    """The rule of tests/test_gpu_ppgauss.py: no more than twice as far from
    the minimum as the reference's own run, or what the stopping rule itself
    guarantees; errors within 1e-3 of truth's; fixed parameters untouched."""
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


@pytest.mark.parametrize("name", ["two_band", "default_flags", "overlap_tau"])
def test_joint_fit_matches_minpack(gpu, z, name):
    from pulseportraiture_amd import pplib
    c = _fit_case(z, name)
    nbin, nj = c["data"].shape[1], 2 * c["njoin"]
    init, flags = c["init"], c["flags"]
    r = pplib.fit_gaussian_portrait(
        c["code"], c["data"], init[:-nj - 1], init[-1], np.outer(c["errs"], np.ones(nbin)),
        flags[:-nj - 1], bool(flags[-1]), pplib.get_bin_centers(nbin), c["freqs"], c["nu_ref"],
        [c["groups"], init[-nj - 1:-1], flags[-nj - 1:-1]], c["P"])
    assert len(r.fitted_params) == len(init) - 1 and len(r.fit_errs) == len(init) - 1
    p = np.append(r.fitted_params, r.scattering_index)
    sig = np.append(r.fit_errs, r.scattering_index_err)
    _check_fit(z, name, p, sig, r.chi2, r.dof, r.lm_results.status)
    assert r.lm_results.nfev > 1 and r.lm_results.covar.shape == (len(p), len(p))
    assert np.allclose(np.sqrt(np.diag(r.lm_results.covar)), sig, rtol=1e-12)


def test_batch_is_bitwise_single_calls(gpu, z):
    """Three portraits in one call equal three single calls bit for bit, a
    repeated call equals itself, and a workspace limit that holds one
    portrait splits the call with the same bits."""
    from pulseportraiture_amd import pplib
    cases = [_fit_case(z, n) for n in ("two_band", "default_flags", "overlap_tau")]

    def run(cs):
        out = gpu.gauss_fit_join(
            np.stack([x["data"] for x in cs]), np.stack([x["freqs"] for x in cs]),
            np.stack([x["errs"] for x in cs]), np.stack([x["init"] for x in cs]),
            np.stack([x["flags"] for x in cs]), [x["code"] for x in cs],
            [x["nu_ref"] for x in cs], np.stack([x["join_of"] for x in cs]),
            np.stack([pplib.join_dm_coef(x["P"], x["freqs"], x["nu_ref"]) for x in cs]), 2)
        return {k: v.cpu().numpy() for k, v in out.items()}

    batch, again = run(cases), run(cases)
    for k in batch:
        assert np.array_equal(batch[k], again[k], equal_nan=True), k
    assert np.all(np.isin(batch["info"][:, 0], CONVERGED))
    for i, x in enumerate(cases):
        one = run([x])
        for k in batch:
            assert np.array_equal(batch[k][i], one[k][0], equal_nan=True), (k, i)
    gpu.set_workspace_limit(1 << 20)
    try:
        split = run(cases)
    finally:
        gpu.set_workspace_limit(32 << 30)
    for k in batch:
        assert np.array_equal(batch[k], split[k], equal_nan=True), k


# -- the pipeline: two archives, a metafile, ppgauss --------------------------
def _archives(z, tag, scale=1.0, nbin_b=None):
    """The pipe fixture's two bands as load_data's dict archives."""
    from pulseportraiture_amd.mjd import MJD
    out = []
    for g, (lo, hi) in enumerate(((1150.0, 1360.0), (1400.0, 1680.0))):
        rows = np.flatnonzero(z["pipe_join_of"] == g)
        freqs, port = z["pipe_freqs"][rows], z["pipe_data"][rows] * scale
        errs = z["pipe_errs"][rows] * scale
        if g == 1 and nbin_b:
            port = port[:, :nbin_b]
        half = (hi - lo) / 14.0
        out.append(dict(subints=port[None, None].copy(), freqs=freqs[None].copy(),
                        weights=np.ones((1, len(freqs))),
                        SNRs=(port.max(axis=1) / errs)[None, None].copy(),
                        noise_stds=errs[None, None].copy(), Ps=[float(z["pipe_P"])],
                        epochs=[MJD(57300.0)], bw=hi - lo + 2 * half, nu0=0.5 * (lo + hi),
                        source="J0000+0000", filename="%s_band%d.fits" % (tag, g)))
    return out


class _Registered(object):
    """Two registered archives and the metafile that names them."""

    def __init__(self, z, tmp_path, tag, **kw):
        from pulseportraiture_amd import archive
        self.archive, self.arch = archive, _archives(z, tag, **kw)
        self.names = [a["filename"] for a in self.arch]
        self.metafile = str(tmp_path / (tag + ".meta"))
        with open(self.metafile, "w") as mf:
            mf.write("".join(n + "\n" for n in self.names))

    def __enter__(self):
        for a in self.arch:
            self.archive.register_archive(a["filename"], a)
        return self

    def __exit__(self, *exc):
        for n in self.names:
            self.archive.unregister_archive(n)


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


def test_pipeline_metafile_model(gpu, z, tmp_path):
    from pulseportraiture_amd import ppgauss, pplib
    start = _start_model(tmp_path)
    out = str(tmp_path / "fitted.gmodel")
    p_t, s_t, c_t = z["pipe_p_truth"], z["pipe_sig_truth"], float(z["pipe_chi2_truth"])
    P, nu_ref = float(z["pipe_P"]), float(z["pipe_nu_ref"])
    with _Registered(z, tmp_path, "pipe") as reg:
        dp = ppgauss.DataPortrait(reg.metafile, quiet=True)
        # the concatenated portrait
        assert dp.njoin == 2 and dp.datafiles == reg.names and dp.port.shape == (16, 256)
        assert np.all(np.diff(dp.freqs[0]) > 0) and np.array_equal(dp.freqs[0], z["pipe_freqs"])
        assert np.array_equal(dp.freqsxs[0], dp.freqs[0]) and dp.nchan == dp.nchanx == 16
        for g in range(2):
            rows = np.flatnonzero(z["pipe_join_of"] == g)
            assert np.array_equal(dp.join_ichans[g], rows)
            assert np.array_equal(dp.join_ichanxs[g], rows)
        assert dp.Ps == [P] and dp.nu0 == dp.freqs.mean()
        assert abs(dp.bw - (1680.0 + 20.0 - (1150.0 - 15.0))) < 1e-9
        assert list(dp.join_fit_flags) == [0, 1, 1, 1]
        assert dp.join_params[0] == 0.0 and dp.join_params[1] == 0.0 == dp.join_params[3]
        print("starting join phase %.6f (truth %.6f)" % (dp.join_params[2], p_t[-3]))
        assert abs(dp.join_params[2] - p_t[-3]) <= 1.0 / 256
        assert dp.all_join_params[0] is dp.join_ichanxs
        portx0 = dp.portx.copy()
        # the joint model
        name = str(tmp_path / "joint")
        dp.make_gaussian_model(modelfile=start, niter=1, writemodel=True, outfile=out,
                               model_name=name, quiet=True)
        assert dp.fgp.lm_results.status in CONVERGED and dp.fgp.lm_results.covar.shape == (25, 25)
        free = z["pipe_flags"] != 0
        tol = np.sqrt(FTOL * c_t) * s_t
        p = np.concatenate([dp.model_params, dp.join_params, [dp.scattering_index]])
        print("pipeline: max |p - p_truth| / sigma = %.3e"
              % np.max(np.abs(p - p_t)[free] / s_t[free]))
        assert np.all(np.abs(p - p_t)[free] <= tol[free]) and dp.join_params[0] == 0.0
        # ... as the files hold them
        _, code, nu, ngauss, params, flags, alpha, fit_alpha = pplib.read_model(out)
        pf = np.append(params, alpha)
        pf[1] *= 256 / P
        keep = np.r_[0:20, 24]
        assert np.all(np.abs(pf - p_t[keep])[free[keep]] <= tol[keep][free[keep]] + 0.5e-8)
        lines = open(name + ".join").readlines()
        nfit = len(lines) // 3
        assert len(lines) == 3 * nfit and lines[-3].startswith("# archive name")
        jf = np.array([[float(v) for v in line.split()[1:]] for line in lines[-2:]])
        assert [line.split()[0] for line in lines[-2:]] == reg.names
        assert np.all(np.abs(jf[:, 0] - p_t[[20, 22]]) <= tol[[20, 22]] + 0.5e-10)
        assert np.all(np.abs(jf[:, 2] - p_t[[21, 23]]) <= tol[[21, 23]] + 0.5e-6)
        # the data and the model end de-rotated by the fitted join parameters
        derot = pplib.rotate_join_rows(portx0, dp.join_ichanxs, dp.join_params, P, dp.freqsxs[0],
                                       dp.nu_ref, -1.0)
        assert np.array_equal(dp.portx, derot) and np.array_equal(dp.modelx, dp.model)
        assert np.max(np.abs(dp.portx - dp.modelx)) < 8 * np.max(z["pipe_errs"])
        # the joinfile read back, applied and undone
        dj = ppgauss.DataPortrait(reg.metafile, quiet=True, joinfile=name + ".join")
        assert np.array_equal(dj.join_params, jf[:, [0, 2]].ravel())
        before = dj.portx.copy()
        dj.apply_joinfile(nu_ref)
        assert np.max(np.abs(dj.portx - before)) > 0.1 * np.max(before)
        dj.apply_joinfile(nu_ref, undo=True)
        assert np.max(np.abs(dj.portx - before)) <= 1e-12 * np.max(np.abs(before))
        dj.apply_joinfile(nu_ref, undo=True)  # with nothing to undo it rotates the other way
        assert np.max(np.abs(dj.portx - before)) > 0.1 * np.max(before)
        # ppspline takes the metafile portrait as it is
        from pulseportraiture_amd import ppspline
        ds = ppspline.DataPortrait(reg.metafile, quiet=True)
        ds.make_spline_model(max_ncomp=2, quiet=True)
        assert ds.model.shape == ds.port.shape and np.all(np.isfinite(ds.model))


def test_batch_helper_equals_single_calls(gpu, z, tmp_path):
    from pulseportraiture_amd import ppgauss
    start = _start_model(tmp_path)
    with _Registered(z, tmp_path, "a") as ra, _Registered(z, tmp_path, "b", scale=1.7) as rb:
        metas = [ra.metafile, rb.metafile]
        batch = [ppgauss.DataPortrait(m, quiet=True) for m in metas]
        outs = [str(tmp_path / "a.gmodel"), str(tmp_path / "b.gmodel")]
        names = [str(tmp_path / "a_batch"), str(tmp_path / "b_batch")]
        ppgauss.make_gaussian_models(batch, modelfiles=[start, start], niter=1, writemodel=True,
                                     outfiles=outs, model_names=names, quiet=True)
        for m, dpb, o, nm in zip(metas, batch, outs, names):
            dps = ppgauss.DataPortrait(m, quiet=True)
            dps.make_gaussian_model(modelfile=start, niter=1, writemodel=True,
                                    outfile=o + ".single", model_name=nm + "_single", quiet=True)
            for attr in ("model_params", "model_param_errs", "join_params", "join_param_errs",
                         "model", "modelx", "port", "portx"):
                assert np.array_equal(getattr(dps, attr), getattr(dpb, attr)), attr
            assert dps.chi2 == dpb.chi2 and dps.dof == dpb.dof and dps.phi == dpb.phi
            assert open(nm + "_single.join").read() == open(nm + ".join").read()


def test_metafile_starts(gpu, z, tmp_path):
    """max_ngauss, auto_gauss and init_params starts on a metafile portrait."""
    from pulseportraiture_amd import ppgauss
    with _Registered(z, tmp_path, "s") as reg:
        for kw in (dict(max_ngauss=3), dict(auto_gauss=0.03),
                   dict(init_params=[0.0, 0.0, 0.23, 0.03, 9.0])):
            dp = ppgauss.DataPortrait(reg.metafile, quiet=True)
            dp.make_gaussian_model(ref_prof=(1250.0, 200.0), quiet=True,
                                   model_name=str(tmp_path / "starts"), **kw)
            assert dp.ngauss >= 1 and np.isfinite(dp.chi2)
            assert len(dp.join_params) == 4 and dp.join_params[0] == 0.0
            assert len(dp.model_params) == 2 + 6 * dp.ngauss
            assert dp.model.shape == dp.port.shape


def test_refusals(gpu, z, tmp_path):
    from pulseportraiture_amd import ppgauss, pplib
    from pulseportraiture_amd.engine import PPFitError
    freqs = np.linspace(1200.0, 1800.0, 4)
    data, errs = np.zeros((4, 64)), np.ones(4)
    dm = pplib.join_dm_coef(PERIOD, freqs, 1500.0)
    for ngauss, njoin in ((1, 9), (15, 4)):  # njoin > 8; 6 ngauss + 2 njoin = 98 > 96
        p = np.concatenate([[0.0, 0.0], np.tile([0.5, 0.0, 0.05, 0.0, 1.0, 0.0], ngauss),
                            np.zeros(2 * njoin), [-4.0]])
        join_of = np.arange(4) % njoin
        with pytest.raises(PPFitError, match="error -3"):
            gpu.gauss_eval_join(data, freqs, errs, p, "000", 1500.0, join_of, dm, njoin)
        with pytest.raises(PPFitError, match="error -3"):
            gpu.gauss_fit_join(data, freqs, errs, p, np.ones(len(p)), "000", 1500.0, join_of, dm,
                               njoin)
    p = np.array([0.0, 0.0, 0.5, 0.0, 0.05, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, -4.0])
    join_of = np.array([0, 1, 2, 1])  # a group equal to njoin
    with pytest.raises(PPFitError, match="error -1"):
        gpu.gauss_eval_join(data, freqs, errs, p, "000", 1500.0, join_of, dm, 2)
    with pytest.raises(PPFitError, match="error -1"):
        gpu.gauss_fit_join(data, freqs, errs, p, np.ones(len(p)), "000", 1500.0, join_of, dm, 2)
    with _Registered(z, tmp_path, "mixed", nbin_b=128) as reg:
        with pytest.raises(ValueError, match="nbin"):
            ppgauss.DataPortrait(reg.metafile, quiet=True)
