"""The CPU oracle, one channel at a time, against the reference's per-channel
phase + tau fits (tests/golden/nb_scat.npz, make_golden_nb_scat.py; at the odd
lengths 999 and 2049 tests/golden/nb_scat_odd.npz, make_golden_nb_scat_odd.py).

Bar: 1e-4 sigma on phi and tau (the oracle restates the reference's numpy
code; scipy's trust-ncg is deterministic, so what is left is rounding in the
objective, measured at 7e-6 sigma at worst) and the same status; on the
scattered cases also 1e-6 relative on the errors and the other outputs.  The
unscattered case ends with tau near 1e-8 and an error near 1e5: its
covariance is singular to rounding, so the errors there are not compared.
Each case prints its margins; the odd-length rows were chosen to stay within
half of each bar (their generator checks it).
"""
import numpy as np
import pytest

from tests import nb_scat_cases as NB


def check_case(name, ic):
    c = NB.case(ic, name)
    worst = worst_rel = 0.0
    for n in range(len(c["freqs"])):
        r = NB.oracle_channel(c["data"][n], c["model"][n], float(c["freqs"][n]),
                              float(c["errs"][n]), c["P"], float(c["phi0"][n]),
                              float(c["tau0"][n]), c["log10"])
        dphi = abs(r["phi"] - c["phi"][n]) / c["phi_err"][n]
        dtau = abs(r["tau"] - c["tau"][n]) / c["tau_err"][n]
        worst = max(worst, dphi, dtau)
        assert dphi <= 1e-4 and dtau <= 1e-4, (ic, n, dphi, dtau)
        assert r["return_code"] == int(c["return_code"][n])
        if float(c["tau_inj"]) == 0.0:
            continue
        for k in ["phi_err", "tau_err", "scale", "scale_err", "snr", "red_chi2"]:
            worst_rel = max(worst_rel, abs(r[k] / c[k][n] - 1.0))
            np.testing.assert_allclose(r[k], c[k][n], rtol=1e-6, err_msg="%s case %d chan %d" % (
                k, ic, n))
        worst_rel = max(worst_rel, np.abs(r["cov"] / c["cov"][n] - 1.0).max())
        np.testing.assert_allclose(r["cov"], c["cov"][n], rtol=1e-6)
    print("%s case %d nbin %d: worst |delta| %.3g sigma, %.3g relative" % (
        name, ic, c["nbin"], worst, worst_rel))


@pytest.mark.parametrize("ic", range(NB.ncase()))
def test_oracle_reproduces_reference(ic):
    check_case(NB.MAIN, ic)


@pytest.mark.parametrize("ic", range(NB.ncase(NB.ODD)))
def test_oracle_reproduces_reference_odd_lengths(ic):
    """nbin 999 (log10 tau) and 2049 (linear): no Nyquist term, a half-integer
    in errs_FT, dof = nbin - 3."""
    assert NB.case(ic, NB.ODD)["nbin"] % 2 == 1
    check_case(NB.ODD, ic)
