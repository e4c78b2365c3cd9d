"""CPU yardstick of the automatic Gaussian-component search
(pplib.auto_gaussian_profiles; tests/auto_gauss_reference.py restates it in
numpy + scipy).  Writes tests/golden/auto_gauss.npz.

Profiles of known components with DC 0.02 and seeded noise of sigma 0.01
(example.gmodel's components: 0.01 of their peak).  Per case: the profile,
sigma, the expected count, the restatement's end point (p_ref, chi2_ref) and
the MINPACK fit from the true parameters at ftol = xtol = 1e-13 (p_truth,
sig_truth, chi2_truth).  The pipeline case is a 16 x 256 portrait of B3sep
with mild power-law evolution: the restatement's search on its reference
profile, then the portrait fit from what it found, against the portrait fit
from the true parameters.

The conditions on the inputs are asserted here (a seed that breaks one is
replaced, never the condition):
  - the restatement finds the true count;
  - at every stage the best (width, bin) cell of the bank beats every other
    cell by a relative margin >= 1e-6 in s2, so a device map good to 1e-9
    picks the same cell;
  - no end point sits on a bound.

Run on the CPU:  python tests/golden/make_golden_auto_gauss.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from pulseportraiture_amd import pplib  # noqa: E402
from tests import auto_gauss_reference as R  # noqa: E402

Y = R.Y
DC, SIGMA, MARGIN = 0.02, 0.01, 1e-6


def example_components():
    mf = os.path.join(os.path.dirname(pplib.__file__), "data", "example.gmodel")
    params = pplib.read_model(mf, quiet=True)[4]
    return [(params[2 + 6 * c], params[4 + 6 * c], params[6 + 6 * c]) for c in range(3)]


C2 = [(0.40, 0.05, 1.0), (0.46, 0.03, 0.6)]
B3 = [(0.2, 0.03, 1.0), (0.5, 0.06, 0.5), (0.8, 0.015, 0.7)]
# name -> (components, nbins, tau [bin], seed, tau the search starts from or
# None: the true one held fixed)
CASES = {"A1": ([(0.35, 0.05, 1.0)], (64, 256), 0.0, 1, None),
         "B3sep": (B3, (64, 256), 0.0, 2, None),
         "C2blend": (C2, (64, 256), 0.0, 3, None),
         "wrap": ([(0.004, 0.03, 0.8), (0.6, 0.1, 0.3)], (64, 256), 0.0, 4, None),
         "ex3": (example_components(), (256,), 0.0, 5, None),
         "noise": ([], (64, 256), 0.0, 6, None),
         "C2tau": (C2, (128,), 2.5, 7, None),
         # beyond the issue's list: the same profile with tau fitted inside the
         # search, from 1 bin
         "C2taufit": (C2, (128,), 2.5, 7, 1.0)}


def case_names():
    return ["%s_%d" % (name, nbin) for name, c in CASES.items() for nbin in c[1]]


def check_search(name, a, ngauss):
    """The conditions on a search's inputs."""
    assert a["ngauss"] == ngauss, (name, a["ngauss"], ngauss)
    for h in a["history"]:
        assert h["margin"] >= MARGIN, (name, h["margin"])
    assert a["history"][-1]["stop"] == "min_snr", name
    wids, amps = a["p"][3::3], a["p"][4::3]
    assert np.all(amps > R.EDGE) and np.all(wids > R.EDGE) and np.all(wids < R.WID_MAX - R.EDGE)


def profile_case(name, comps, nbin, tau, seed, tau_start):
    fit_tau = tau_start is not None
    p_true = np.concatenate([[DC, tau]] + [list(c) for c in comps])
    clean = pplib.gen_gaussian_profile(p_true, nbin)
    sigma = SIGMA * (clean.max() - DC) if name == "ex3" else SIGMA
    profile = clean + sigma * np.random.default_rng(seed).standard_normal(nbin)
    a = R.auto(profile, sigma, tau=tau_start if fit_tau else tau, fit_scattering=fit_tau)
    check_search(name, a, len(comps))
    assert not fit_tau or a["p"][1] > R.EDGE, name
    out = {"profile": profile, "sigma": np.array(sigma), "ngauss": np.array(len(comps)),
           "tau": np.array(tau_start if fit_tau else tau), "fit_tau": np.array(fit_tau),
           "p_true": p_true, "p_ref": a["p"], "chi2_ref": np.array(a["chi2"]),
           "nstage": np.array(len(a["history"]))}
    if comps:
        t = R.truth(profile, sigma, p_true, fit_tau)
        assert t["ier"] in (1, 2, 3, 4), name
        order = R.match_order(a["p"], t["p"])
        d = np.abs(R.delta(R.reorder(a["p"], order), t["p"]))
        free = t["sig"] > 0
        dist = np.max(d[free] / t["sig"][free])
        rel = np.max(np.abs(R.reorder(a["sig"], order)[free] / t["sig"][free] - 1.0))
        print("%s_%d: %d components in %d stages; chi2_ref - chi2_truth %.3e (chi2 %.4f); "
              "max|p_ref - p_truth|/sigma %.3e; errs rel %.2e; least margin %.2e"
              % (name, nbin, a["ngauss"], len(a["history"]), a["chi2"] - t["chi2"], t["chi2"],
                 dist, rel, min(h["margin"] for h in a["history"])))
        assert rel <= 1e-3, (name, rel)
        out.update({"p_truth": t["p"], "sig_truth": t["sig"], "chi2_truth": np.array(t["chi2"]),
                    "dof": np.array(t["dof"])})
    else:
        print("%s_%d: no component; best s2 %.3f" % (name, nbin, a["history"][0]["s2"]))
    return {"%s_%d_%s" % (name, nbin, k): v for k, v in out.items()}


# -- the pipeline case ---------------------------------------------------------
PIPE_NU_REF, PIPE_SEED = 1400.0, 31
# DC, tau, (loc, dloc, wid, dwid, amp, damp) of B3sep, alpha
PIPE_P = np.array([DC, 0.0, 0.2, 0.002, 0.03, -0.2, 1.0, -1.0, 0.5, -0.003, 0.06, 0.3, 0.5, -0.5,
                   0.8, 0.001, 0.015, -0.1, 0.7, -1.5, -4.0])


def to_portrait_layout(p_prof, alpha):
    """DC, tau, then loc, 0, wid, 0, amp, 0 per component, alpha."""
    comps = np.zeros((len(p_prof[2:]) // 3, 6))
    comps[:, 0::2] = np.asarray(p_prof[2:]).reshape(-1, 3)
    return np.concatenate([p_prof[:2], comps.ravel(), [alpha]])


def pipeline_case():
    """make_gaussian_model(max_ngauss=6) restated: the reference profile is
    the unweighted mean of the channels strictly inside nu0 +- bw / 2, its
    noise is get_noise's, the portrait fit starts from the search's
    components with the evolution parameters at 0; tau and alpha fixed."""
    freqs, data, errs = Y.synth("000", PIPE_P, 16, 256, PIPE_NU_REF, 0.02, PIPE_SEED, 1200.0,
                                1600.0)
    inside = (PIPE_NU_REF - 200.0 < freqs) & (PIPE_NU_REF + 200.0 > freqs)
    profile = data[inside].mean(axis=0)
    a = R.auto(profile, R.noise_ps(profile), max_ngauss=6)
    check_search("pipe", a, 3)
    flags = np.ones(len(PIPE_P), dtype=int)
    flags[1] = flags[-1] = 0
    from scipy.optimize import leastsq
    pr = Y.Problem("000", data, errs, freqs, PIPE_NU_REF, to_portrait_layout(a["p"], -4.0), flags)
    x, cov_x, info, _, ier = leastsq(pr.resid, pr.x0(), Dfun=pr.jac, full_output=True)
    assert ier in (1, 2, 3, 4)
    p_ref, chi2_ref = pr.external(x), float(np.sum(info["fvec"] ** 2))
    t = Y.Problem("000", data, errs, freqs, PIPE_NU_REF, PIPE_P, flags).solve(True)
    assert t["ier"] in (1, 2, 3, 4)
    # the restatement's pipeline reaches the truth run's minimum
    order = R.match_order(a["p"], PIPE_P[[0, 1] + list(range(2, 20, 2))])
    p_m = np.concatenate([p_ref[:2], p_ref[2:-1].reshape(-1, 6)[order].ravel(), p_ref[-1:]])
    d = p_m - t["p"]
    d[2:-1:6] = (d[2:-1:6] + 0.5) % 1.0 - 0.5
    free = flags != 0
    dist = np.max(np.abs(d)[free] / t["sig"][free])
    print("pipe: %d components; chi2_ref - chi2_truth %.3e (chi2 %.4f); "
          "max|p_ref - p_truth|/sigma %.3e" % (a["ngauss"], chi2_ref - t["chi2"], t["chi2"], dist))
    assert chi2_ref - t["chi2"] <= Y.FTOL * t["chi2"] and dist <= np.sqrt(Y.FTOL * t["chi2"])
    return {"pipe_data": data, "pipe_errs": errs, "pipe_freqs": freqs, "pipe_flags": flags,
            "pipe_p_ref": p_m, "pipe_chi2_ref": np.array(chi2_ref), "pipe_p_truth": t["p"],
            "pipe_sig_truth": t["sig"], "pipe_chi2_truth": np.array(t["chi2"]),
            "pipe_dof": np.array(t["dof"])}


def main():
    out = {}
    for name, (comps, nbins, tau, seed, tau_start) in CASES.items():
        for nbin in nbins:
            out.update(profile_case(name, comps, nbin, tau, seed, tau_start))
    out.update(pipeline_case())
    np.savez_compressed(os.path.join(HERE, "auto_gauss.npz"), **out)


if __name__ == "__main__":
    main()
