"""Joint fits of several receivers' portraits without a device: the numpy
restatement of the join rotation and its Jacobian
(tests/golden/make_golden_ppgauss_join.py, the yardstick of the device
kernels) against central differences of the host generator, the host
generator against the restatement, the .join writer's lines and the joinfile
reader."""
import importlib.util
import os
import types

import numpy as np
import pytest

from tests.conftest import GOLDEN


def _yardstick():
    spec = importlib.util.spec_from_file_location(
        "make_golden_ppgauss_join", os.path.join(GOLDEN, "make_golden_ppgauss_join.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


YJ = _yardstick()

# DC, tau, (loc, dloc, wid, dwid, amp, damp) x 2, (phase, DM) x 2, alpha; the
# second component is two bins wide at nbin 64 and within a bin of phase 0
JOIN = [0.21, 1.0, 1.3, -2.0]
P000 = np.array([0.02, 2.5, 0.40, 0.004, 0.050, -0.3, 1.0, -1.2,
                 0.004, -0.003, 0.030, 0.2, 0.6, -0.8] + JOIN + [-4.0])
P111 = np.array([0.02, 2.5, 0.40, 2e-5, 0.050, -1e-5, 1.0, -4e-4,
                 0.004, -1e-5, 0.030, 1e-5, 0.6, 2e-4] + JOIN + [-4.0])
SCALE = np.array([1.0, 1.0] + [1.0, 1.0, 0.05, 1.0, 1.0, 1.0] * 2 + [0.01, 0.1] * 2 + [1.0])
SCALE111 = np.array([1.0, 1.0] + [1.0, 1e-4, 0.05, 1e-4, 1.0, 1e-3] * 2 + [0.01, 0.1] * 2 + [1.0])
GROUPS = [np.arange(0, 8, 2), np.arange(1, 8, 2)]
PERIOD = 0.005


@pytest.mark.parametrize("code,p,scale,tau", [("000", P000, SCALE, 2.5), ("000", P000, SCALE, 0.0),
                                              ("111", P111, SCALE111, 2.5)])
def test_numpy_jacobian_matches_central_differences(code, p, scale, tau):
    """Each column to 1e-6 of its norm, step 1e-6 of the parameter's scale,
    as tests/test_ppgauss_cpu.py checks the restatement without the join; the
    host generator equals the restatement to 1e-13 of the row maximum."""
    from pulseportraiture_amd import pplib
    p = p.copy()
    p[1] = tau
    nbin, freqs, nu_ref = 64, np.linspace(1200.0, 1800.0, 8), 1500.0
    phases = pplib.get_bin_centers(nbin)

    def host(q):
        return pplib.gen_gaussian_portrait(code, q[:-1], q[-1], phases, freqs, nu_ref, GROUPS,
                                           PERIOD)

    model, jac = YJ.model_and_jac(code, p, nbin, freqs, nu_ref, GROUPS, PERIOD)
    assert jac.shape == (len(p), 8, nbin)
    assert np.all(np.abs(model - host(p)) <= 1e-13 * np.abs(model).max(axis=1)[:, None])
    for q in range(len(p)):
        if tau == 0.0 and q in (1, len(p) - 1):
            continue  # gen_gaussian_portrait does not scatter at tau = 0 on either side
        h = 1e-6 * scale[q]
        up, dn = p.copy(), p.copy()
        up[q] += h
        dn[q] -= h
        num = (host(up) - host(dn)) / (2 * h)
        err = np.linalg.norm(num - jac[q]) / np.linalg.norm(jac[q])
        assert err <= 1e-6, (q, err)


def test_join_file_lines(tmp_path):
    """write_join_parameters: the reference's format strings, digit for digit
    (pplib.py:509-519); the file is appended to."""
    from pulseportraiture_amd import ppspline
    long_name = "a_directory_name/with_an_archive_name_longer_than_45.fits"
    assert len(long_name) > 45
    dp = types.SimpleNamespace(
        joinfile=None, model_name=str(tmp_path / "J0000"), datafiles=["lband.fits", long_name],
        join_params=np.array([0.0, 0.00123456789, -0.123456789012, 12.3456789]),
        join_param_errs=np.array([0.0, 1.5e-4, 2.5e-6, 0.0012346]))
    ppspline.DataPortrait.write_join_parameters(dp)
    header = ("# archive name                                -phase offset & err [rot]"
              "  -delta-DM & err [cm**-3 pc]\n")
    first = "lband.fits                                    0.0000000000 0.0000000000   0.001235 0.000150\n"
    second = (long_name + " " * (len(long_name) - 45) +
              "-0.1234567890 0.0000025000   12.345679 0.001235\n")
    path = str(tmp_path / "J0000.join")
    assert open(path).read() == header + first + second
    dp.join_params = np.array([0.0, 0.0, 0.25, -1.0])
    ppspline.DataPortrait.write_join_parameters(dp)
    lines = open(path).readlines()
    assert len(lines) == 6 and lines[:3] == [header, first, second] and lines[3] == header
    assert lines[5] == (long_name + " " * (len(long_name) - 45) +
                        " 0.2500000000 0.0000025000  -1.000000 0.001235\n")
    # joinfile= names the file instead
    dp.joinfile = str(tmp_path / "other.join")
    ppspline.DataPortrait.write_join_parameters(dp)
    assert len(open(dp.joinfile).readlines()) == 3 and len(open(path).readlines()) == 6


def test_joinfile_parsing(tmp_path):
    """The last njoin lines, matched by archive name, in the new layout
    (name, phase, error, DM, error) and the old one (name, phase, DM)."""
    from pulseportraiture_amd import ppspline
    files = ["a.fits", "b.fits"]
    start = np.array([0.0, 0.0, 0.3, 0.0])
    new = tmp_path / "new.join"
    new.write_text(ppspline.JOIN_HEADER +
                   ppspline.join_parameter_line("a.fits", 0.9, 0.1, 9.0, 0.1) +
                   ppspline.join_parameter_line("b.fits", 0.8, 0.1, 8.0, 0.1) +
                   ppspline.JOIN_HEADER +
                   ppspline.join_parameter_line("b.fits", -0.125, 0.001, 0.5, 0.01) +
                   ppspline.join_parameter_line("a.fits", 0.0, 0.0, -0.25, 0.02))
    got = ppspline.read_joinfile(str(new), files, start)
    assert np.array_equal(got, [0.0, -0.25, -0.125, 0.5]) and start[2] == 0.3
    old = tmp_path / "old.join"
    old.write_text("a.fits 0.0 0.75\nb.fits 0.0625 -1.5\n")
    assert np.array_equal(ppspline.read_joinfile(str(old), files, start), [0.0, 0.75, 0.0625, -1.5])
    bad = tmp_path / "bad.join"
    bad.write_text("a.fits 0.5 1.0\nc.fits 0.1 0.2\n")
    assert np.array_equal(ppspline.read_joinfile(str(bad), files, start), [0.5, 1.0, 0.3, 0.0])


def test_join_groups_and_coefficients():
    from pulseportraiture_amd import pplib
    assert list(pplib.join_groups([np.array([1, 3]), np.array([0, 2])], 4)) == [1, 0, 1, 0]
    with pytest.raises(NotImplementedError):
        pplib.join_groups([np.array([0, 1])], 4)
    freqs = np.array([1000.0, 2000.0])
    coef = pplib.join_dm_coef(0.01, freqs, 2000.0)
    assert coef[1] == 0.0 and abs(coef[0] - pplib.Dconst * 7.5e-7 / 0.01) <= 1e-12 * coef[0]
    theta = pplib.join_row_rotations([np.array([1]), np.array([0])], [0.1, 5.0, 0.2, 2.0], 0.01,
                                     freqs, 2000.0)
    assert theta[1] == 0.1 and abs(theta[0] - (0.2 + 2.0 * coef[0])) <= 1e-15
    with pytest.raises(ValueError):  # join parameters without the period
        pplib.fit_gaussian_portrait("000", np.zeros((2, 64)), np.zeros(8), -4.0, np.ones((2, 64)),
                                    np.ones(8), False, pplib.get_bin_centers(64), freqs, 1500.0,
                                    join_params=[[np.array([0]), np.array([1])], np.zeros(4),
                                                 np.ones(4)])


def test_golden_inputs_meet_their_conditions(golden):
    """Every fit case of ppgauss_join.npz has finite figures and its ref run
    a finite distance from truth."""
    from pulseportraiture_amd import pplib
    z = golden("ppgauss_join.npz")
    for name in ("two_band", "default_flags", "overlap_tau"):
        join_of = z[name + "_join_of"]
        groups = [np.flatnonzero(join_of == g) for g in range(2)]
        assert np.array_equal(pplib.join_groups(groups, len(join_of)), join_of)
        free = z[name + "_flags"] != 0
        d = np.abs(z[name + "_p_ref"] - z[name + "_p_truth"])[free] / z[name + "_sig_truth"][free]
        assert np.all(np.isfinite(d)) and np.all(z[name + "_sig_truth"][free] > 0)
        assert np.all(z[name + "_sig_truth"][~free] == 0)
    assert list(z["two_band_flags"][14:18]) == [0, 0, 1, 1]
    assert list(z["default_flags_flags"][14:18]) == [0, 1, 1, 1]
    assert abs(z["two_band_p_true"][16] - 0.37) == 0 and z["overlap_tau_p_true"][1] != 0
