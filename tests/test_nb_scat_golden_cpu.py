"""The CPU oracle, one channel at a time, against the reference's per-channel
phase + tau fits (tests/golden/nb_scat.npz, make_golden_nb_scat.py).

Bar: 1e-4 sigma on phi and tau (the oracle restates the reference's numpy
code; scipy's trust-ncg is deterministic, so what is left is rounding in the
objective, measured at 7e-6 sigma at worst) and the same status; on the
scattered cases also 1e-6 relative on the errors and the other outputs.  The
unscattered case ends with tau near 1e-8 and an error near 1e5: its
covariance is singular to rounding, so the errors there are not compared.
"""
import numpy as np
import pytest

from tests import nb_scat_cases as NB


@pytest.mark.parametrize("ic", range(NB.ncase()))
def test_oracle_reproduces_reference(ic):
    c = NB.case(ic)
    worst = 0.0
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
            np.testing.assert_allclose(r[k], c[k][n], rtol=1e-6, err_msg="%s case %d chan %d" % (
                k, ic, n))
        np.testing.assert_allclose(r["cov"], c["cov"][n], rtol=1e-6)
    print("case %d: worst |delta| %.3g sigma" % (ic, worst))
