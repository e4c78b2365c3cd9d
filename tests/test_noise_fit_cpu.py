"""The noise-floor fit, the parts that need no device: the numpy restatement
the device is tested against (tests/noise_fit_reference.py) reproduces the
reference's fixtures (tests/golden/noise_fit.npz, written by
tests/golden/make_golden_noise_fit.py), in its term-by-term and its
factorised form; pplib's plain-numpy helpers; the returns for an unknown fn
or method; and the ABI.
"""
import os
import re

import numpy as np
import pytest

from tests import noise_fit_reference as R
from tests.conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "noise_fit.npz"), allow_pickle=False)


def test_fixture_rows_are_separated(fx):
    """The generator's own condition, rechecked on what it stored: at least
    90 % of the rows have a winner safe from rounding (here: all 60)."""
    sep = np.concatenate([fx["separated_%d" % n] for n in fx["nbins"]])
    assert len(sep) == 60 and sep.sum() >= 0.9 * len(sep)
    for n in fx["nbins"]:
        for per_a, idx, s in zip(fx["per_a_%d" % n], fx["idx_%d" % n], fx["separated_%d" % n]):
            assert R.separated(per_a, int(idx)) == bool(s)


@pytest.mark.parametrize("how", ["direct", "factorised"])
def test_restatement_reproduces_kc_and_noise(fx, how):
    for n in fx["nbins"]:
        rows = fx["rows_%d" % n]
        for i, row in enumerate(rows):
            pows = R.power_spectrum(row)
            kc, idx, per_a = R.find_kc(pows, how=how, full=True)
            if how == "direct" or fx["separated_%d" % n][i]:
                assert kc == fx["kc_%d" % n][i], (n, i)
            if how == "direct":
                assert idx == fx["idx_%d" % n][i], (n, i)
                np.testing.assert_allclose(per_a, fx["per_a_%d" % n][i], rtol=1e-12)
            if kc == fx["kc_%d" % n][i]:
                for fact, key in ((1.1, "noise_chans_%d"), (2.0, "noise_fact2_%d")):
                    got = R.noise_from_kc(pows, kc, fact)[0]
                    assert abs(got - fx[key % n][i]) <= 1e-12 * fx[key % n][i], (n, i, fact)
            assert abs(R.get_noise_fit(row) - fx["noise_%d" % n][i]) <= 1e-12 * fx["noise_%d" % n][i]
            for frac in (2, 8):
                ref = fx["ps%d_%d" % (frac, n)][i]
                assert abs(R.get_noise_PS(row, frac) - ref) <= 1e-12 * ref


def test_restatement_zero_power_rows(fx):
    """A zero power makes the objective NaN at flat index 0: a = 1/n, whose
    decay never reaches 0.005 within n harmonics, so kc = n - 1."""
    pz = R.power_spectrum(fx["zero_row"])
    for how in ("direct", "factorised"):
        kc, idx, _ = R.find_kc(pz, how=how, full=True)
        assert (kc, idx) == (len(pz) - 1, 0) and kc == int(fx["zero_kc"])
        kc, idx, _ = R.find_kc(fx["zero_dc_pows"], how=how, full=True)
        assert (kc, idx) == (len(fx["zero_dc_pows"]) - 1, 0) and kc == int(fx["zero_dc_kc"])
    noise, k_crit = R.noise_from_kc(pz, len(pz) - 1)
    assert k_crit == int(0.99 * len(pz)) and noise == float(fx["zero_noise"]) == 0.0


def test_restatement_half_tri_and_weights(fx):
    for i in range(int(fx["n_spectra"])):
        p, e = fx["ht_pows_%d" % i], fx["w_errs_%d" % i]
        for how in ("direct", "factorised"):
            for errs, fn, pre in ((1.0, "half_tri", "ht"), (e, "exp_dc", "w"),
                                  (e, "half_tri", "w_ht")):
                kc, idx, per_a = R.find_kc(p, errs=errs, fn=fn, how=how, full=True)
                if how == "direct" or R.separated(fx[pre + "_per_a_%d" % i],
                                                  int(fx[pre + "_idx_%d" % i])):
                    assert kc == int(fx[pre + "_kc_%d" % i]), (i, how, pre)
                if how == "direct":
                    assert idx == int(fx[pre + "_idx_%d" % i])


def test_restatement_portrait(fx):
    port = fx["port"]
    ref = float(fx["port_noise_fit"])
    assert abs(R.get_noise_fit(port.ravel()) - ref) <= 1e-12 * ref
    for row, r in zip(port, fx["port_noise_fit_chans"]):
        assert abs(R.get_noise_fit(row) - r) <= 1e-12 * r


def test_pure_noise_ties_on_the_b0_plane():
    """The factorised b = 0 plane is bitwise the same for every a."""
    d = np.log10(R.power_spectrum(np.random.default_rng(2).standard_normal(256)))
    S = R.objective_factorised(d, np.ones(len(d)), "exp_dc")
    for ia in range(1, R.NS):
        assert np.array_equal(S[ia, 0], S[0, 0])


def test_pplib_numpy_helpers():
    from pulseportraiture_amd import pplib
    f = pplib.half_triangle_function(4.7, 2.0, 0.5, 8)
    np.testing.assert_allclose(f, [2.5, 2.0, 1.5, 1.0, 0.5, 0.5, 0.5, 0.5], rtol=0, atol=1e-15)
    d = np.array([3.0, 2.0, 1.5, 1.0, 1.0, 1.0])
    k = np.arange(6)
    assert pplib.find_kc_function((0.5, 2.0, 1.0), d) == \
        np.sum((d - (2.0 * np.exp(-0.5 * k) + 1.0)) ** 2)
    assert pplib.find_kc_function((3.0, 2.0, 1.0), d, errs=2.0, fn="half_tri") == \
        np.sum(((d - pplib.half_triangle_function(3.0, 2.0, 1.0, 6)) / 2.0) ** 2)
    assert pplib.find_kc_function((1.0, 1.0, 1.0), d, fn="nope") == 0.0
    # the restatement's objective is pplib's
    S = R.objective_direct(d, np.ones(6), "half_tri")
    a, b, dc = R.a_axis(6, "half_tri")[7], R.axis(0.0, 2.0)[3], R.axis(1.0, 3.0)[5]
    assert abs(S[7, 3, 5] - pplib.find_kc_function((a, b, dc), d, fn="half_tri")) < 1e-13


def test_unknown_fn_and_method_returns(capsys):
    """As the reference: find_kc of an unknown fn is 0, get_noise of an
    unknown method prints a note and returns 0 (neither touches the device)."""
    from pulseportraiture_amd import pplib
    assert pplib.find_kc(np.ones(8), fn="triangle") == 0
    assert pplib.get_noise(np.ones(64), method="median") == 0
    assert "Unknown get_noise method." in capsys.readouterr().out
    assert pplib.default_noise_method == "PS"


def test_binding():
    from pulseportraiture_amd import _lib, build, engine
    txt = open(os.path.join(ROOT, "include", "ppfit.h")).read()
    assert re.search(r"^int ppf_noise_fit_rows\(ppf_ctx\* ctx, int32_t nrow, int32_t nbin, "
                     r"const double\* in,\s+double fact, double\* noise_out, int32_t\* kc_out, "
                     r"int32_t\* idx_out\);", txt, re.M)
    assert re.search(r"^int ppf_find_kc_rows\(ppf_ctx\* ctx, int32_t nrow, int32_t n, "
                     r"const double\* pows,\s+const double\* errs, int32_t fn, int32_t\* kc_out, "
                     r"int32_t\* idx_out\);", txt, re.M)
    assert re.search(r"^int ppf_noise_rows_frac\(ppf_ctx\* ctx, int32_t nrow, int32_t nbin, "
                     r"double frac,\s+const double\* in, double\* out\);", txt, re.M)
    for name, nargs in (("ppf_noise_fit_rows", 8), ("ppf_find_kc_rows", 8),
                        ("ppf_noise_rows_frac", 6)):
        assert name in _lib.EXPORTS and len(_lib.EXPORTS[name][0]) == nargs, name
    build.build()
    lib = _lib.load_library()
    for name in ("ppf_noise_fit_rows", "ppf_find_kc_rows", "ppf_noise_rows_frac"):
        assert hasattr(lib, name)
    assert "ppfit_noisefit.hip" in build.DEPS
    for name in ("noise_fit_rows", "find_kc_rows", "noise_rows"):
        assert hasattr(getattr(engine.Engine, name), "__wrapped__")  # on the engine's stream
