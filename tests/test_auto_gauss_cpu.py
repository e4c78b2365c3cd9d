"""The automatic component search on the CPU: the golden inputs meet their
conditions, the numpy restatement of the filter bank equals a brute-force
double loop, and the package exposes the search (no device needed)."""
import importlib.util
import os

import numpy as np
import pytest

from tests import auto_gauss_reference as R
from tests.conftest import GOLDEN


def _generator():
    spec = importlib.util.spec_from_file_location(
        "make_golden_auto_gauss", os.path.join(GOLDEN, "make_golden_auto_gauss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator()


@pytest.fixture(scope="module")
def z(golden):
    return golden("auto_gauss.npz")


@pytest.mark.parametrize("name", G.case_names())
def test_golden_inputs_meet_their_conditions(z, name):
    """The restatement finds the true count, every stage's best cell leads
    by >= 1e-6 in s2, no end point sits on a bound, and the stored end point
    is the restatement's."""
    a = R.auto(z[name + "_profile"], float(z[name + "_sigma"]), tau=float(z[name + "_tau"]),
               fit_scattering=bool(z[name + "_fit_tau"]))
    G.check_search(name, a, int(z[name + "_ngauss"]))
    assert len(a["history"]) == int(z[name + "_nstage"])
    assert np.allclose(a["p"], z[name + "_p_ref"], rtol=1e-9, atol=1e-12)
    assert abs(a["chi2"] - float(z[name + "_chi2_ref"])) <= 1e-9 * a["chi2"]
    if a["ngauss"]:
        st = z[name + "_sig_truth"]
        free = st > 0
        order = R.match_order(a["p"], z[name + "_p_truth"])
        assert np.max(np.abs(R.reorder(a["sig"], order)[free] / st[free] - 1.0)) <= 1e-3
        assert float(z[name + "_chi2_ref"]) >= float(z[name + "_chi2_truth"]) - 1e-9


def test_pipeline_inputs_meet_their_conditions(z):
    free = z["pipe_flags"] != 0
    p_r, p_t, s_t = z["pipe_p_ref"], z["pipe_p_truth"], z["pipe_sig_truth"]
    c_r, c_t = float(z["pipe_chi2_ref"]), float(z["pipe_chi2_truth"])
    d = p_r - p_t
    d[2:-1:6] = (d[2:-1:6] + 0.5) % 1.0 - 0.5
    assert np.all(s_t[free] > 0) and len(p_t) == 21
    assert 0.0 <= c_r - c_t + 1e-9 <= G.Y.FTOL * c_t + 1e-9
    assert np.max(np.abs(d)[free] / s_t[free]) <= np.sqrt(G.Y.FTOL * c_t)
    kind = G.Y.kinds(len(p_t))
    assert np.all(p_t[free & (kind > 0)] > R.EDGE)
    assert np.all(p_t[free & (kind == 2)] < R.WID_MAX - R.EDGE)


@pytest.mark.parametrize("taun", [0.0, 2.5 / 64])
def test_bank_equals_brute_force(z, taun):
    """bank() against the definition, cell by cell, at nbin 64."""
    from pulseportraiture_amd import pplib
    nbin, err = 64, 0.01
    resid = z["wrap_64_profile"] - np.mean(z["wrap_64_profile"])
    wids = R.widths(nbin)
    s2, best, idx = R.bank(resid, err, taun, wids)
    locs = pplib.get_bin_centers(nbin)
    brute, amp = np.zeros((len(wids), nbin)), np.zeros((len(wids), nbin))
    for w, wid in enumerate(wids):
        for j in range(nbin):
            g = pplib.gen_gaussian_profile([0.0, taun * nbin, locs[j], wid, 1.0], nbin)
            c, gg = float(np.dot(resid, g)), float(np.dot(g, g))
            amp[w, j] = c / gg
            brute[w, j] = c * c / (gg * err * err) if c > 0 else 0.0
    assert np.max(np.abs(s2 - brute)) <= 1e-12 * brute.max()
    w, j = np.unravel_index(np.argmax(brute), brute.shape)
    assert idx == (w, j)
    assert np.allclose(best, [brute[w, j], locs[j], wids[w], amp[w, j]], rtol=1e-12)
    assert wids[0] == 2.0 / nbin and wids[-1] == 0.25
    s2n, bestn, idxn = R.bank(-np.abs(resid) - 1.0, err, taun, wids)
    assert idxn == (-1, -1) and not np.any(bestn) and not np.any(s2n)
    # the correlation form is the same map
    s2f, bestf, idxf = R.bank_fft(resid, err, taun, wids)
    assert np.max(np.abs(s2f - brute)) <= 1e-12 * brute.max() and idxf == idx
    assert np.allclose(bestf, best, rtol=1e-12)


def test_search_is_exposed():
    """The package carries the search and the library's binding the bank."""
    from pulseportraiture_amd import _lib, pplib, ppgauss
    import inspect
    assert "ppf_gauss_bank" in _lib.EXPORTS
    assert callable(pplib.auto_gaussian_profile) and callable(pplib.auto_gaussian_profiles)
    sig = inspect.signature(pplib.auto_gaussian_profiles)
    assert [(k, v.default) for k, v in sig.parameters.items()][1:] == [
        ("errs", None), ("max_ngauss", 8), ("tau", 0.0), ("fit_scattering", False),
        ("min_snr", 5.0), ("nwid", 16), ("quiet", True)]
    for fn in (ppgauss.DataPortrait.fit_profile, ppgauss.DataPortrait.make_gaussian_model,
               ppgauss.make_gaussian_models):
        assert inspect.signature(fn).parameters["max_ngauss"].default == 0
    with pytest.raises(ValueError):  # before any device work
        pplib.auto_gaussian_profiles([np.zeros(64)], [1.0], max_ngauss=17)


def test_accept_rules():
    """auto_gaussian_accept: convergence, the BIC for three parameters, and
    no amplitude or width on a bound."""
    from pulseportraiture_amd.pplib import auto_gaussian_accept as acc
    p = np.array([0.0, 0.0, 0.5, 0.05, 1.0])
    pen = 3.0 * np.log(256)
    assert acc(1, 100.0, 100.0 + pen + 1e-6, p, 256)
    assert not acc(1, 100.0, 100.0 + pen, p, 256)
    assert not acc(5, 100.0, 1000.0, p, 256) and not acc(-1, 100.0, 1000.0, p, 256)
    for q, v in ((4, 5e-7), (3, 5e-7), (3, 0.25 - 5e-7)):
        bad = p.copy()
        bad[q] = v
        assert not acc(1, 100.0, 1000.0, bad, 256)
