"""ppgauss without a device: the numpy restatement of the analytic Jacobian
(tests/golden/make_golden_ppgauss.py, the yardstick of the device kernels)
against central differences of the host generator, lmfit's bound transforms,
fit_gaussian_profile's flag convention, the .gmodel round trip and the
refusals."""
import importlib.util
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN


def _yardstick():
    spec = importlib.util.spec_from_file_location(
        "make_golden_ppgauss", os.path.join(GOLDEN, "make_golden_ppgauss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


Y = _yardstick()

# DC, tau, (loc, dloc, wid, dwid, amp, damp) x 2, alpha; the second
# component sits within a bin of phase 0, so the wrap is crossed
P000 = np.array([0.02, 2.5, 0.40, 0.004, 0.050, -0.3, 1.0, -1.2,
                 0.004, -0.003, 0.030, 0.2, 0.6, -0.8, -4.0])
P111 = np.array([0.02, 2.5, 0.40, 2e-5, 0.050, -1e-5, 1.0, -4e-4,
                 0.004, -1e-5, 0.030, 1e-5, 0.6, 2e-4, -4.0])
SCALE = np.array([1.0, 1.0] + [1.0, 1.0, 0.05, 1.0, 1.0, 1.0] * 2 + [1.0])
SCALE111 = np.array([1.0, 1.0] + [1.0, 1e-4, 0.05, 1e-4, 1.0, 1e-3] * 2 + [1.0])


@pytest.mark.parametrize("code,p,scale,tau", [("000", P000, SCALE, 2.5), ("000", P000, SCALE, 0.0),
                                              ("111", P111, SCALE111, 2.5)])
def test_numpy_jacobian_matches_central_differences(code, p, scale, tau):
    """Each column to 1e-6 of its norm, step 1e-6 of the parameter's scale
    (truncation ~1e-12, rounding ~1e-10 relative)."""
    from pulseportraiture_amd import pplib
    p = p.copy()
    p[1] = tau
    nbin, freqs, nu_ref = 64, np.linspace(1200.0, 1800.0, 8), 1500.0
    phases = pplib.get_bin_centers(nbin)
    model, jac = Y.model_and_jac(code, p, nbin, freqs, nu_ref)
    assert np.array_equal(model, pplib.gen_gaussian_portrait(code, p[:-1], p[-1], phases, freqs,
                                                             nu_ref)) or \
        np.max(np.abs(model - pplib.gen_gaussian_portrait(code, p[:-1], p[-1], phases, freqs,
                                                          nu_ref))) < 1e-14
    for q in range(len(p)):
        if tau == 0.0 and q in (1, len(p) - 1):
            continue  # gen_gaussian_portrait does not scatter at tau = 0 on either side
        h = 1e-6 * scale[q]
        up, dn = p.copy(), p.copy()
        up[q] += h
        dn[q] -= h
        num = (pplib.gen_gaussian_portrait(code, up[:-1], up[-1], phases, freqs, nu_ref) -
               pplib.gen_gaussian_portrait(code, dn[:-1], dn[-1], phases, freqs, nu_ref)) / (2 * h)
        err = np.linalg.norm(num - jac[q]) / np.linalg.norm(jac[q])
        assert err <= 1e-6, (q, err)


def test_bound_transforms_round_trip():
    npar = 15
    kind = Y.kinds(npar)
    assert list(kind) == [0, 1, 0, 0, 2, 0, 1, 0, 0, 0, 2, 0, 1, 0, 0]
    rng = np.random.default_rng(1)
    v = rng.uniform(0.01, 0.24, npar)
    x = Y.to_internal(v, kind)
    assert np.max(np.abs(Y.to_external(x, kind) - v)) <= 1e-15
    # the gradient factors are the transforms' derivatives
    h = 1e-6
    num = (Y.to_external(x + h, kind) - Y.to_external(x - h, kind)) / (2 * h)
    assert np.max(np.abs(num - Y.dexternal(x, kind))) <= 1e-9
    # every internal value maps inside the bounds
    far = Y.to_external(rng.uniform(-50, 50, npar), kind)
    assert np.all(far[kind == 1] >= 0.0)
    assert np.all((far[kind == 2] >= 0.0) & (far[kind == 2] <= Y.WID_MAX))


def test_profile_fit_flags_mapping():
    """pplib.py:1868-1873: fit_flags holds DC and the component parameters,
    tau follows fit_scattering."""
    from pulseportraiture_amd.pplib import profile_fit_flags
    assert profile_fit_flags(8) == [True, False] + [True] * 6
    assert profile_fit_flags(8, None, True) == [True] * 8
    ff = [0, 1, 0, 1, 1, 0, 1]
    assert profile_fit_flags(8, ff, True) == [False, True, True, False, True, True, False, True]
    assert profile_fit_flags(8, ff, False)[1] is False


def test_write_model_round_trip(tmp_path):
    """DataPortrait.write_model -> read_model: parameters, flags and code,
    loc >= 1 wrapped, TAU back in seconds."""
    from pulseportraiture_amd import ppgauss, pplib
    dp = ppgauss.DataPortrait.__new__(ppgauss.DataPortrait)
    dp.datafile, dp.model_name, dp.model_code, dp.nu_ref = "x.fits", "J0000", "010", 1400.0
    dp.Ps, dp.nbin = [0.004], 256
    dp.model_params = np.array([0.01, 3.0, 1.25, 0.001, 0.04, -0.2, 2.0, -1.5,
                                0.5, 0.0, 0.02, 0.1, 1.0, 0.3])
    dp.model_param_errs = 0.01 * np.abs(dp.model_params) + 1e-4
    dp.fit_flags = np.array([1, 0, 1, 1, 1, 0, 1, 1, 0, 1, 1, 1, 0, 1])
    dp.scattering_index, dp.scattering_index_err, dp.fitalpha = -4.4, 0.2, 1
    out = str(tmp_path / "m.gmodel")
    dp.write_model(out, quiet=True)
    dp.write_errfile(out + "_errs", quiet=True)
    name, code, nu_ref, ngauss, params, flags, alpha, fit_alpha = pplib.read_model(out)
    want = dp.model_params.copy()
    want[2] = 0.25
    want[1] = 3.0 * 0.004 / 256
    assert (name, code, nu_ref, ngauss, fit_alpha) == ("J0000", "010", 1400.0, 2, 1)
    assert np.allclose(params, want, rtol=0, atol=5.1e-9) and alpha == -4.4
    assert np.array_equal(flags, dp.fit_flags)
    assert abs(params[1] * 256 / 0.004 - 3.0) < 1e-3  # TAU [s] -> [bin]
    ename, _, _, _, eparams, eflags, ealpha, _ = pplib.read_model(out + "_errs")
    assert ename == "J0000_errors" and ealpha == 0.2
    assert np.allclose(eparams[2:], dp.model_param_errs[2:], rtol=0, atol=5.1e-9)


def test_start_flags():
    """make_gaussian_model's starting parameters and flags from a profile
    fit (ppgauss.py:140-159): slopes and indices start at 0, fix* clear the
    evolution flags, fiducial_gaussian fixes the first component's only."""
    from pulseportraiture_amd import ppgauss
    dp = ppgauss.DataPortrait.__new__(ppgauss.DataPortrait)
    dp.source, dp.ngauss = "J0000", 2
    dp.init_params = np.array([0.01, 0.5, 0.3, 0.04, 1.0, 0.6, 0.02, 0.5])

    def start(**kw):
        a = dict(modelfile=None, ref_prof=(None, None), tau=0.0, fixloc=False, fixwid=False,
                 fixamp=False, fixscat=True, fixalpha=True, scattering_index=-4.0,
                 model_code="000", fiducial_gaussian=False, auto_gauss=0.0, model_name=None,
                 init_params=None)
        a.update(kw)
        dp._start_model(**a)
        return dp.fit_flags

    assert list(start()) == [1, 0] + [1] * 12
    assert list(dp.init_model_params) == [0.01, 0.5, 0.3, 0, 0.04, 0, 1.0, 0, 0.6, 0, 0.02, 0,
                                          0.5, 0]
    assert dp.model_name == "J0000" and dp.fitalpha == 0
    assert list(start(fixscat=False, fixloc=True)) == [1, 1] + [1, 0, 1, 1, 1, 1] * 2
    assert list(start(fixwid=True, fixamp=True)) == [1, 0] + [1, 1, 1, 0, 1, 0] * 2
    assert list(start(fixloc=True, fiducial_gaussian=True)) == \
        [1, 0] + [1, 0, 1, 1, 1, 1] + [1, 1, 1, 1, 1, 1]
    assert start(fixalpha=False, model_name="m") is dp.fit_flags and dp.fitalpha == 1
    assert dp.model_name == "m"


def test_refusals():
    from pulseportraiture_amd import ppgauss, pplib
    phases = pplib.get_bin_centers(64)
    data, p = np.zeros((4, 64)), np.array([0.0, 0.0, 0.5, 0.0, 0.05, 0.0, 1.0, 0.0])
    with pytest.raises(NotImplementedError):  # joinfile parameters
        pplib.fit_gaussian_portrait("000", data, p, -4.0, np.ones((4, 64)), np.ones(8), False,
                                    phases, np.linspace(1, 2, 4), 1.5,
                                    join_params=[[np.arange(2)], [0.0, 0.0], [1, 1]])
    errs = np.ones((4, 64))
    errs[1, 3] = 2.0
    with pytest.raises(NotImplementedError):  # errs varying along a row
        pplib.fit_gaussian_portrait("000", data, p, -4.0, errs, np.ones(8), False, phases,
                                    np.linspace(1, 2, 4), 1.5)
    with pytest.raises(NotImplementedError):
        pplib.fit_gaussian_profile(data[0], [0.0, 0.0, 0.5, 0.05, 1.0], np.arange(64) + 1.0)
    dp = ppgauss.DataPortrait.__new__(ppgauss.DataPortrait)
    with pytest.raises(NotImplementedError):  # the interactive selector
        dp.fit_profile(np.zeros(64), auto_gauss=0.0)
    with pytest.raises(NotImplementedError):
        ppgauss.make_gaussian_models([dp], residplot="x.png")
    with pytest.raises(NotImplementedError):
        ppgauss.DataPortrait("x.fits", joinfile="j.txt")


def test_golden_inputs_meet_their_conditions(golden):
    """Every fit case of ppgauss.npz: the reference's own run within 1e-3 of
    truth's errors, no fitted wid or amp on a bound."""
    z = golden("ppgauss.npz")
    for name in ("port_notau", "port_tau", "profile_tau"):
        flags = z[name + "_flags"] != 0
        st, sr = z[name + "_sig_truth"][flags], z[name + "_sig_ref"][flags]
        assert np.all(st > 0) and np.max(np.abs(sr / st - 1.0)) <= 1e-3
        kind = Y.kinds(len(flags))
        p = z[name + "_p_truth"]
        assert np.all(p[flags & (kind > 0)] > 0) and np.all(p[flags & (kind == 2)] < Y.WID_MAX)
        assert z[name + "_chi2_ref"] >= z[name + "_chi2_truth"] - 1e-9
