"""Host steps of ppspline model building (no device): count_crossings, the
splprep arguments (smoothing condition, frequency flip, max_nbreak refit) and
the curve fit itself on the fixture's reference projections."""
import json
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN


@pytest.fixture(scope="module")
def fx():
    return (np.load(os.path.join(GOLDEN, "ppspline.npz")),
            np.load(os.path.join(GOLDEN, "ppspline_variants.npz")),
            json.load(open(os.path.join(GOLDEN, "ppspline.json"))))


def test_count_crossings():
    from pulseportraiture_amd.pplib import count_crossings
    assert count_crossings(np.array([0.0, 1.0, 0.0, 1.0, 0.0]), 0.5) == 4
    assert count_crossings(np.array([0.0, 0.1, 0.2]), 0.5) == 0
    assert count_crossings(np.array([1.0, 2.0, 3.0]), 0.5) == 0
    # an exact hit makes two sign changes and is taken off once: one crossing
    assert count_crossings(np.array([0.0, 0.5, 1.0]), 0.5) == 1
    # ... also when the array only touches the threshold and turns back
    assert count_crossings(np.array([0.0, 0.5, 0.0]), 0.5) == 1
    # a hit at the end makes one sign change and is taken off: none
    assert count_crossings(np.array([0.0, 0.2, 0.5]), 0.5) == 0
    # two neighbouring hits: sign changes -1 -> 0 and 0 -> 1, less two hits
    assert count_crossings(np.array([0.0, 0.5, 0.5, 1.0]), 0.5) == 0
    assert count_crossings(np.array([3, 1, 3, 1]), 2) == 3  # integers


def test_spline_smoothing_formula():
    from pulseportraiture_amd.ppspline import spline_smoothing
    snr, sig = np.array([10.0, 20.0, 40.0]), np.array([0.5, 0.25, 0.125])
    want = 3 * (25.0 + 25.0 + 25.0) / 70.0 ** 2
    assert spline_smoothing(3, snr, sig) == pytest.approx(want, rel=1e-15)
    assert spline_smoothing(3, snr, sig, sfac=2.5) == pytest.approx(2.5 * want, rel=1e-15)
    assert spline_smoothing(3, snr, sig, sfac=0) == 0.0


class Recorder:
    """Stands in for splprep: records its arguments, returns nknot knots."""

    def __init__(self, nknots):
        self.nknots, self.calls = list(nknots), []

    def __call__(self, x, **kw):
        self.calls.append((x, kw))
        n = self.nknots[len(self.calls) - 1]
        k = kw["k"]
        nin = n - 2 * k
        t = np.concatenate([np.zeros(k), np.arange(nin, dtype=float), np.ones(k) * nin])
        return ([t, [np.zeros(n)] * len(x), k], kw["u"]), 0.0, 0, "ok"


def test_fit_arguments_flip_and_refit():
    from pulseportraiture_amd.ppspline import fit_spline_curve
    proj = np.arange(12.0).reshape(6, 2)
    w = np.linspace(0.1, 0.6, 6)
    up = np.linspace(1000.0, 1500.0, 6)
    # positive bandwidth: rows as they are, one call (no max_nbreak)
    rec = Recorder([12])
    fit_spline_curve(proj, w, up, 0.7, bw=800.0, k=3, splprep=rec)
    (x, kw), = rec.calls
    assert np.array_equal(np.array(x), proj.T) and np.array_equal(kw["w"], w)
    assert np.array_equal(kw["u"], up) and (kw["ub"], kw["ue"]) == (1000.0, 1500.0)
    assert kw["s"] == 0.7 and kw["k"] == 3 and kw["nest"] is None and kw["task"] == 0
    assert kw["per"] == 0 and kw["t"] is None and kw["full_output"] == 1 and kw["quiet"] == 1
    # negative bandwidth: frequencies descend, every per-channel array is reversed
    rec = Recorder([12])
    fit_spline_curve(proj, w, up[::-1], 0.7, bw=-800.0, k=3, splprep=rec)
    (x, kw), = rec.calls
    assert np.array_equal(np.array(x), proj[::-1].T) and np.array_equal(kw["w"], w[::-1])
    assert np.array_equal(kw["u"], up) and (kw["ub"], kw["ue"]) == (1000.0, 1500.0)
    # 12 knots at k = 3 are 7 breakpoints: more than 4 -> refit with nest = 4 + 2 k, same s
    rec = Recorder([12, 10])
    (tck, u), fp, ier, msg = fit_spline_curve(proj, w, up, 0.7, k=3, max_nbreak=4, splprep=rec)
    assert len(rec.calls) == 2 and len(tck[0]) == 10
    assert rec.calls[1][1]["nest"] == 10 and rec.calls[1][1]["s"] == 0.7
    # at most 7 allowed: no refit
    rec = Recorder([12])
    fit_spline_curve(proj, w, up, 0.7, k=3, max_nbreak=7, splprep=rec)
    assert len(rec.calls) == 1
    # two breakpoints: s = inf; fewer than two are taken as two
    for nb in (2, 1, 0):
        rec = Recorder([12, 8])
        fit_spline_curve(proj, w, up, 0.7, k=3, max_nbreak=nb, splprep=rec)
        assert rec.calls[1][1]["nest"] == 8 and rec.calls[1][1]["s"] == np.inf
    rec = Recorder([16, 14])
    fit_spline_curve(proj, w, up, 0.0, k=5, max_nbreak=3, splprep=rec)
    assert rec.calls[1][1]["nest"] == 13 and rec.calls[1][1]["s"] == 0.0


@pytest.mark.parametrize("key", ["32x256", "20x250", "24x128", "48x512"])
def test_curve_fit_on_reference_projections(fx, key):
    """splprep through fit_spline_curve on the reference's projections gives
    the reference's knots and coefficients."""
    from pulseportraiture_amd.ppspline import fit_spline_curve, spline_smoothing
    z, _, meta = fx
    m = meta["cases"][key]
    proj, snr, sig = z["proj_port_" + key], z["SNRs_" + key], z["noise_stds_" + key]
    s = spline_smoothing(len(proj), snr, sig)
    (tck, u), fp, ier, msg = fit_spline_curve(proj, z["pca_weights_" + key], z["freqs_" + key], s,
                                              bw=float(z["bw_" + key]), k=3)
    assert ier == m["ier"] and tck[2] == m["k"] and fp == pytest.approx(m["fp"], rel=1e-9)
    np.testing.assert_allclose(tck[0], z["t_" + key], rtol=1e-13)
    np.testing.assert_allclose(np.array(tck[1]), z["c_" + key], rtol=0,
                               atol=1e-12 * np.max(np.abs(z["c_" + key])))


def test_find_significant_eigvec_on_reference_vectors(fx):
    """The reference's control flow on its own eigenvectors, the noise values
    handed in (get_noise itself runs on the device)."""
    from pulseportraiture_amd.pplib import find_significant_eigvec
    z, _, meta = fx
    for key, m in meta["cases"].items():
        vec = z["eigvec10_" + key].T
        # get_noise_PS (pplib.py:2227-2253) on the host
        pows = np.abs(np.fft.rfft(vec, axis=0)) ** 2 / vec.shape[0]
        kc = int((1 - 1.0 / 4) * len(pows))
        noise = np.sqrt(np.mean(pows[kc:], axis=0))
        got = find_significant_eigvec(vec, check_max=10, return_max=10, noise=noise,
                                      rchi2_tol=0.1)
        assert list(got) == m["ieig_pca"], key
        got2 = find_significant_eigvec(vec, check_max=10, return_max=2, noise=noise)
        assert list(got2) == m["ieig_pca"][:2], key
