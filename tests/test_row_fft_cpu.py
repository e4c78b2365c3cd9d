"""The mixed-radix row FFT's host side (no GPU): which nbin take which row
transform (ppf_row_transform, the predicate every launch uses), the option
that switches it, the plan and passes run on the host for every eligible
length (tools/rowfft_plan_check.cpp), and the reference fixture at nbin 1000
and 1536 (tests/golden/generic_nbin.npz) against the oracle.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

SMOOTH = [96, 100, 768, 1000, 1536, 2000, 3000, 6144, 8000, 8100]


@pytest.fixture(scope="module")
def lib():
    from pulseportraiture_amd import build, _lib
    build.build()
    return _lib.load_library()


def _kind(lib, nbin):
    from pulseportraiture_amd import _lib
    k = ctypes.c_int32(-1)
    rc = lib.ppf_row_transform(None, nbin, ctypes.byref(k))
    return rc, (_lib.ROW_TRANSFORMS[k.value] if rc == 0 else None)


def test_row_transform_table(lib):
    """ppf_row_transform with no context (the default options)."""
    for nbin in SMOOTH:
        assert _kind(lib, nbin) == (0, "smooth"), nbin
    for nbin in list(range(17, 8192, 2)) + [8190]:
        assert _kind(lib, nbin) == (0, "direct"), nbin
    for nbin in (64, 128, 256, 512, 1024, 2048, 4096, 8192):
        assert _kind(lib, nbin) == (0, "pow2"), nbin
    # the smallest lengths: 16 and 32 are no FFT instantiation of the
    # power-of-two family and take the mixed-radix one; the test lengths of
    # tests/test_gpu_row_fft.py are all eligible
    for nbin in (16, 32, 18, 20, 24, 30, 48, 50, 162, 250, 2560, 7290):
        assert _kind(lib, nbin) == (0, "smooth"), nbin
    for nbin in (22, 26, 28, 34, 998, 6002):  # a prime factor above 5 in nbin / 2
        assert _kind(lib, nbin) == (0, "direct"), nbin
    for nbin in (15, 0, -4, 8193, 8194):
        assert _kind(lib, nbin)[0] == -3, nbin  # PPF_ERR_UNSUPPORTED
    assert lib.ppf_row_transform(None, 1000, None) != 0


def test_row_fft_option_id():
    from pulseportraiture_amd import _lib
    assert _lib.OPTIONS["row_fft"] == 7
    assert "ppf_row_transform" in _lib.EXPORTS


def test_rowfft_plan_check(tmp_path):
    """Forward and inverse transform of every eligible length on the host,
    through the kernels' own plan and pass functions, against a direct DFT
    in long double at 1e-12 of the largest value."""
    exe = str(tmp_path / "rowfft_plan_check")
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Werror",
                           "-I" + os.path.join(ROOT, "pulseportraiture_amd", "csrc"),
                           os.path.join(ROOT, "tools", "rowfft_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    word = out.stdout.split()
    assert word[0] == "ok" and int(word[1]) >= 100, out.stdout
    assert float(word[2]) <= 1e-12 and float(word[3]) <= 1e-12, out.stdout


@pytest.mark.parametrize("case", [0, 1])
def test_generic_nbin_fixture_oracle(case):
    """The oracle against the reference's own fit at nbin 1000 / 1536, at
    the wideband bars: 1e-3 sigma on phi and DM, 1e-4 relative on their
    errors, 1e-6 on red_chi2, the same return code, no subint excluded."""
    from oracle import ppfit_oracle as O
    z = np.load(os.path.join(GOLDEN, "generic_nbin.npz"))
    g = lambda k: z["c%d_%s" % (case, k)]  # noqa: E731
    assert int(g("nbin")) == (1000, 1536)[case]
    data, model, freqs, P = g("data"), g("model"), g("freqs"), float(g("P"))
    assert data.shape == (2, 8, int(g("nbin")))
    for i in range(data.shape[0]):
        nu = float(g("nu_fit")[i])
        o = O.fit_portrait_full(data[i], model, list(g("init")[i]), P, freqs, [nu] * 3, [None] * 3,
                                g("errs")[i], [1, 1, 0, 0, 0], log10_tau=False,
                                method="trust-ncg")
        assert abs(o.phi - g("phi")[i]) <= 1e-3 * g("phi_err")[i]
        assert abs(o.DM - g("DM")[i]) <= 1e-3 * g("DM_err")[i]
        np.testing.assert_allclose(o.phi_err, g("phi_err")[i], rtol=1e-4)
        np.testing.assert_allclose(o.DM_err, g("DM_err")[i], rtol=1e-4)
        np.testing.assert_allclose(o.red_chi2, g("red_chi2")[i], rtol=1e-6)
        assert o.return_code == int(g("return_code")[i])
