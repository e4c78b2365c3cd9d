"""Wavelet smoothing, the parts that need no device: the committed db8 filter,
the numpy restatement the device is tested against (tests/swt_reference.py),
the stability of the named test profiles, and the ABI.

Stability is a condition on the test inputs, not a measurement of the device:
a profile is usable only if the restatement's own answer does not hang on
rounding.  All ten named profiles (tests/swt_reference.py: CASES) meet it with
the committed filter literals; none was replaced.  Measured here: the smallest
threshold gap is 3.6e-4 (256, seed 3) and the smallest level gap 1.3e-1 (64,
seed 1).
"""
import os
import re

import numpy as np
import pytest

from tests import swt_reference as R
from tests.conftest import ROOT

CASES = R.case_list()


def test_case_table():
    assert len(CASES) == 10
    assert CASES[0] == (64, 1, 0.05) and CASES[-1] == (2048, 1, 0.02)


def device_filter():
    txt = open(os.path.join(ROOT, "pulseportraiture_amd", "csrc", "ppfit_swt.hip")).read()
    body = re.search(r"kSwtH\[16\] = \{(.*?)\};", txt, re.S).group(1)
    return np.array([float(v) for v in body.replace("\n", " ").split(",")])


def test_filter_literals():
    """The committed literals -- the device's and the restatement's are the
    same 16 numbers -- are the db8 scaling filter: sum h = sqrt 2, the
    double-shift orthogonality and unit norm to 1e-15, h[0] = 0.0544..."""
    h = device_filter()
    assert h.shape == (16,)
    assert np.array_equal(h, R.H)
    assert abs(h.sum() - np.sqrt(2.0)) <= 1e-15
    assert abs(np.dot(h, h) - 1.0) <= 1e-15
    for m in range(1, 8):
        assert abs(np.dot(h[:16 - 2 * m], h[2 * m:])) <= 1e-15, m
    assert abs(h[0] - 0.0544158422431) < 1e-12 and abs(h[15] + 0.000117476784) < 1e-12
    # the high-pass partner has 8 vanishing moments' worth of zero sum
    assert abs(R.G.sum()) <= 1e-15


@pytest.mark.parametrize("nbin,level", [(64, 1), (64, 3), (64, 6), (96, 1), (128, 7), (256, 8)])
def test_restatement_reconstructs(nbin, level):
    """fact = 0 keeps every coefficient: the inverse gives the input back,
    also where the dilated filter wraps round the row many times (64, 6)."""
    x = np.random.default_rng(nbin + level).standard_normal(nbin)
    for threshtype in ("hard", "soft"):
        y = R.wavelet_smooth(x, level, threshtype, 0.0)
        assert np.abs(y - x).max() <= 1e-13 * np.abs(x).max()


def test_restatement_shift_equivariant():
    x = R.named_profile(128, 2, 0.05)
    for level, shift in ((3, 1), (5, 37), (7, 64)):
        for threshtype in ("hard", "soft"):
            y = R.wavelet_smooth(x, level, threshtype, 1.3)
            ys = R.wavelet_smooth(np.roll(x, shift), level, threshtype, 1.3)
            assert np.array_equal(np.roll(y, shift), ys)


def test_restatement_refuses_indivisible():
    with pytest.raises(ValueError):
        R.wavelet_smooth(np.ones(96), 6)
    R.wavelet_smooth(np.ones(96), 1)


def kept_set(prof, res):
    _, lam, mags = R.wavelet_smooth(prof, res["nlevel"], "hard", res["fact"], details=True)
    return lam, mags, mags >= lam


@pytest.mark.parametrize("nbin,seed,sigma", CASES)
def test_named_case_is_stable(nbin, seed, sigma):
    prof = R.named_profile(nbin, seed, sigma)
    res = R.named_smart(nbin, seed, sigma)
    assert not res["zeroed"]
    lam, mags, kept = kept_set(prof, res)
    gap = np.abs(mags - lam).min() / lam
    fv = np.sort(res["fun_vals"])
    level_gap = (fv[1] - fv[0]) / abs(fv[0])
    print("nbin %d seed %d: nlevel %d fact %.4f threshold gap %.2e level gap %.2e"
          % (nbin, seed, res["nlevel"], res["fact"], gap, level_gap))
    assert gap >= 1e-6
    assert level_gap >= 1e-6
    pert = prof * (1.0 + 1e-13 * np.random.default_rng(1000 + seed).standard_normal(nbin))
    res2 = R.smart_smooth(pert, full=True)
    assert res2["nlevel"] == res["nlevel"]
    assert np.array_equal(kept_set(pert, res2)[2], kept)


def test_abi_carries_the_entry_points():
    from pulseportraiture_amd import _lib
    txt = open(os.path.join(ROOT, "include", "ppfit.h")).read()
    for name in ("ppf_wavelet_smooth_rows", "ppf_wavelet_objective_rows", "ppf_smart_smooth_rows"):
        assert re.search(r"^int %s\(" % name, txt, re.M), name
        assert name in _lib.EXPORTS, name
    assert _lib.KERNEL_IDS["swt"] == int(re.search(r"#define PPF_K_SWT (\d+)", txt).group(1))
    assert _lib.PPF_THRESH == {"hard": 0, "soft": 1}


def test_library_exports_the_entry_points():
    from pulseportraiture_amd import build, _lib
    build.build()
    lib = _lib.load_library()
    for name in ("ppf_wavelet_smooth_rows", "ppf_wavelet_objective_rows", "ppf_smart_smooth_rows"):
        assert hasattr(lib, name), name


def test_smart_smooth_levels():
    from pulseportraiture_amd.pplib import smart_smooth_levels
    assert smart_smooth_levels(63) == 0
    assert smart_smooth_levels(64, 0) == 0
    assert smart_smooth_levels(96) == 1
    assert smart_smooth_levels(96, 5) == 1
    assert smart_smooth_levels(64) == 6
    assert smart_smooth_levels(2048, 8) == 8
    assert smart_smooth_levels(8192) == 13
