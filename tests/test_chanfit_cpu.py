"""The host side of the fits across channels (pplib): powlaw, powlaw_integral,
powlaw_freqs, get_WRMS and fit_powlaw_function against their definitions, and
the yardstick of the device tests (tests/chanfit_reference.py) against itself.
The device fits are in tests/test_gpu_chanfit.py."""
import numpy as np
import pytest
from scipy.integrate import quad

from pulseportraiture_amd import pplib
from tests import chanfit_reference as CR


@pytest.mark.parametrize("alpha", [-4.4, -1.6, -1.0, 0.0, 2.0])
def test_powlaw_integral_against_quadrature(alpha):
    nu1, nu2, nu_ref, A = 1100.0, 1900.0, 1500.0, 3.7
    want, err = quad(lambda nu: pplib.powlaw(nu, nu_ref, A, alpha), nu1, nu2, epsabs=0.0,
                     epsrel=1e-13)
    got = pplib.powlaw_integral(nu2, nu1, nu_ref, A, alpha)
    assert abs(got - want) <= 1e-12 * abs(want) + err
    # orientation and the empty interval
    assert pplib.powlaw_integral(nu1, nu2, nu_ref, A, alpha) == -got
    assert pplib.powlaw_integral(nu1, nu1, nu_ref, A, alpha) == 0.0


@pytest.mark.parametrize("alpha", [-4.4, -1.6, -1.0, 0.0, 2.0])
@pytest.mark.parametrize("N", [1, 7, 64])
def test_powlaw_freqs_equal_flux_channels(alpha, N):
    lo, hi = 1100.0, 1900.0
    nus = pplib.powlaw_freqs(lo, hi, N, alpha)
    assert nus.shape == (N + 1,)
    np.testing.assert_allclose(nus[[0, -1]], [lo, hi], rtol=1e-14)
    assert np.all(np.diff(nus) > 0.0)
    flux = pplib.powlaw_integral(nus[1:], nus[:-1], 1500.0, 1.0, alpha)
    total = pplib.powlaw_integral(hi, lo, 1500.0, 1.0, alpha)
    # N differences of values up to |C| hi**(1 + alpha) or lo**(1 + alpha)
    np.testing.assert_allclose(flux, total / N, rtol=1e-10)
    mid = pplib.powlaw_freqs(lo, hi, N, alpha, mid=True)
    assert mid.shape == (N,)
    np.testing.assert_array_equal(mid, 0.5 * (nus[:-1] + nus[1:]))


def test_get_WRMS_formula():
    rng = np.random.default_rng(3)
    d = rng.normal(2.0, 1.0, 50)
    e = rng.uniform(0.5, 2.0, 50)
    e[[4, 17]] = 0.0  # left out
    ok = e > 0.0
    w = e[ok] ** -2.0
    mean = (d[ok] * w).sum() / w.sum()
    want = np.sqrt(((d[ok] - mean) ** 2 * w).sum() / w.sum())
    assert pplib.get_WRMS(d, e) == pytest.approx(want, rel=1e-14)
    # unit errors: the plain rms about the mean
    assert pplib.get_WRMS(d) == pytest.approx(d.std(), rel=1e-13)


def test_fit_powlaw_function_is_the_weighted_residual():
    f = np.linspace(1100.0, 1900.0, 9)
    y = pplib.powlaw(f, 1500.0, 2.5, -1.7)
    e = np.linspace(0.1, 0.3, 9)
    r = pplib.fit_powlaw_function([2.0, -1.0], f, 1500.0, data=y, errs=e)
    np.testing.assert_array_equal(r, (y - 2.0 * (f / 1500.0) ** -1.0) / e)
    np.testing.assert_array_equal(pplib.fit_powlaw_function((2.5, -1.7), f, 1500.0, y, e), 0.0)


def test_reference_jacobian_and_line_truth():
    """The yardstick's analytic Jacobian against central differences, and its
    long-double line against np.polyfit."""
    c = CR.powlaw_inputs(5)
    a = (c["y"][0], c["errs"][0], c["freqs"][0], 1500.0)
    p = np.array([3.0, -1.2])
    J = CR.powlaw_jac(p, *a)
    for k, h in enumerate((1e-6, 1e-6)):
        d = np.zeros(2)
        d[k] = h
        num = (CR.powlaw_resid(p + d, *a) - CR.powlaw_resid(p - d, *a)) / (2 * h)
        np.testing.assert_allclose(J[:, k], num, rtol=1e-7, atol=1e-7)
    li = CR.line_inputs(64)
    for r in range(4):
        t = CR.line_truth(li["x"][r], li["y"][r], li["w"][r]).astype(np.float64)
        np.testing.assert_allclose(CR.line_polyfit(li["x"][r], li["y"][r], li["w"][r]), t,
                                   rtol=1e-9)
    assert (~CR.usable(li["errs"])).sum(axis=1).min() >= 5  # a tenth of 64 left out
