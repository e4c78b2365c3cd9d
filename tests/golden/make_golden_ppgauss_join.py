"""CPU yardstick of the joint Gaussian-component fits of several receivers'
portraits (ppgauss on a metafile: fit_gaussian_portrait with join_params).

Writes tests/golden/ppgauss_join.npz.  It extends make_golden_ppgauss.py,
loaded the way the tests load it: the parameter vector gains a phase [rot]
and a DM per join group before alpha (lmfit's order, pplib.py:1964-2020), and
the model rows of a group are rotated as rotate_data does it
(pplib.py:2378-2421), restated here in numpy:

  theta_n = phase_g + Dconst DM_g / P (f_n^-2 - nu_ref^-2)
  row_n  <- irfft(rfft(row_n) exp(2 pi i k theta_n))

  ref    leastsq at its defaults, forward differences -- what the reference
         does;
  truth  the analytic Jacobian below as Dfun at ftol = xtol = 1e-13: p_truth,
         sigma_truth (lmfit's stderr with scale_covar) and chi2_truth.

A fixture is written only if both MINPACK runs end with ier in 1..3 and the
ref run's own largest |p_ref - p_truth| / sigma_truth over the free
parameters is finite.

Run on the CPU:  python tests/golden/make_golden_ppgauss_join.py
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from pulseportraiture_amd import pplib  # noqa: E402


def _base():
    spec = importlib.util.spec_from_file_location(
        "make_golden_ppgauss", os.path.join(HERE, "make_golden_ppgauss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


Y = _base()
FTOL = Y.FTOL


def kinds(npar, njoin):
    """make_golden_ppgauss.kinds with 2 njoin unbounded join parameters
    before alpha."""
    k = np.zeros(npar, dtype=int)
    k[:npar - 2 * njoin - 1] = Y.kinds(npar - 2 * njoin)[:-1]
    return k


def split(p, njoin):
    """(DC, tau, components, alpha), join parameters."""
    p = np.asarray(p, dtype=float)
    return np.append(p[:len(p) - 2 * njoin - 1], p[-1]), p[len(p) - 2 * njoin - 1:-1]


def rotations(join_params, join_ichans, P, freqs, nu_ref):
    """theta_n [nchan] and d theta_n / d DM_g [nchan] (rotate_data,
    pplib.py:2389-2413)."""
    theta, dm_coef = np.zeros(len(freqs)), np.zeros(len(freqs))
    for g, ic in enumerate(join_ichans):
        fterm = freqs[ic] ** -2.0 - nu_ref ** -2.0
        D = pplib.Dconst * join_params[2 * g + 1] / P
        theta[ic] = join_params[2 * g] + D * fterm
        dm_coef[ic] = pplib.Dconst / P * fterm
    return theta, dm_coef


def model_and_jac(model_code, p, nbin, freqs, nu_ref, join_ichans, P):
    """gen_gaussian_portrait(model_code, p[:-1], p[-1], ..., join_ichans, P)
    [nchan, nbin] and its derivatives [npar, nchan, nbin] to p = DC, tau,
    components, (phase_g, DM_g) per group, alpha."""
    njoin = len(join_ichans)
    p0, jp = split(p, njoin)
    model, jac = Y.model_and_jac(model_code, p0, nbin, freqs, nu_ref)
    theta, dm_coef = rotations(jp, join_ichans, P, freqs, nu_ref)
    k = np.arange(nbin // 2 + 1)
    phasor = np.exp(2.0j * np.pi * np.outer(theta, k))

    def rot(r, filt=phasor):
        return np.fft.irfft(np.fft.rfft(r, axis=-1) * filt, n=nbin, axis=-1)

    dtheta = rot(model, 2.0j * np.pi * k * phasor)
    model = rot(model)
    jac = rot(jac)
    jac[0] = 1.0
    cols = np.zeros((2 * njoin, len(freqs), nbin))
    for g, ic in enumerate(join_ichans):
        cols[2 * g, ic] = dtheta[ic]
        cols[2 * g + 1, ic] = dm_coef[ic, None] * dtheta[ic]
    return model, np.concatenate([jac[:-1], cols, jac[-1:]])


def eval_numpy(model_code, p, data, errs, freqs, nu_ref, join_ichans, P):
    """chi2, J^T r and J^T J over the external parameters."""
    model, jac = model_and_jac(model_code, p, data.shape[-1], freqs, nu_ref, join_ichans, P)
    r = ((data - model) / errs[:, None]).ravel()
    J = -(jac / errs[None, :, None]).reshape(len(p), -1)
    return r @ r, J @ r, J @ J.T


class Problem(Y.Problem):
    """make_golden_ppgauss.Problem with join parameters."""

    def __init__(self, model_code, data, errs, freqs, nu_ref, init, flags, join_ichans, P):
        Y.Problem.__init__(self, model_code, data, errs, freqs, nu_ref, init, flags)
        self.join_ichans, self.P = join_ichans, P
        self.kind = kinds(len(self.init), len(join_ichans))

    def resid(self, x):
        p = self.external(x)
        model = pplib.gen_gaussian_portrait(self.code, p[:-1], p[-1], self.phases, self.freqs,
                                            self.nu_ref, self.join_ichans, self.P)
        return ((self.data - model) / self.errs[:, None]).ravel()

    def jac(self, x):
        p = self.external(x)
        _, d = model_and_jac(self.code, p, self.data.shape[-1], self.freqs, self.nu_ref,
                             self.join_ichans, self.P)
        J = -(d / self.errs[None, :, None]).reshape(len(p), -1)[self.free]
        return (J * Y.dexternal(x, self.kind[self.free])[:, None]).T


def synth(model_code, p, freqs, nbin, nu_ref, join_ichans, P, sigma, seed):
    phases = pplib.get_bin_centers(nbin)
    port = pplib.gen_gaussian_portrait(model_code, p[:-1], p[-1], phases, freqs, nu_ref,
                                       join_ichans, P)
    rng = np.random.default_rng(seed)
    errs = sigma * (1.0 + 0.5 * rng.uniform(size=len(freqs)))
    return port + errs[:, None] * rng.standard_normal(port.shape), errs


def join_of(join_ichans, nchan):
    out = np.zeros(nchan, dtype=np.int32)
    for g, ic in enumerate(join_ichans):
        out[ic] = g
    return out


# DC, tau, two components
BASE000 = np.array([0.02, 0.0, 0.40, 0.004, 0.050, -0.3, 1.0, -1.2,
                    0.46, -0.003, 0.030, 0.2, 0.6, -0.8])
BASE111 = np.array([0.02, 3.0, 0.40, 2e-5, 0.050, -1e-5, 1.0, -4e-4,
                    0.46, -1e-5, 0.030, 1e-5, 0.6, 2e-4])
P_TWO = 0.005  # [sec]


def fit_cases():
    """name -> dict(code, data, errs, freqs, nu_ref, P, join_of, init, flags,
    p_true); `data_of` names the case whose data a case shares."""
    cases = {}
    # two receivers, 700-900 and 1100-1900 MHz, 8 x 128 each; the second is
    # off by 0.37 rot and a DM of 3 (1.4 turns across its band)
    freqs = np.concatenate([np.linspace(700.0, 900.0, 8), np.linspace(1100.0, 1900.0, 8)])
    groups = [np.arange(8), np.arange(8, 16)]
    p = np.concatenate([BASE000, [0.0, 0.0, 0.37, 3.0], [-4.0]])
    data, errs = synth("000", p, freqs, 128, 1500.0, groups, P_TWO, 0.02, 31)
    init = p.copy()
    rng = np.random.default_rng(131)
    init[:14] *= 1.0 + 0.03 * rng.uniform(-1, 1, 14)
    init[1] = 0.0
    init[16:18] = [0.372, 2.97]
    flags = np.ones(len(p), dtype=int)
    flags[[1, 14, 15, -1]] = 0
    cases["two_band"] = dict(code="000", data=data, errs=errs, freqs=freqs, nu_ref=1500.0,
                             P=P_TWO, groups=groups, init=init, flags=flags, p_true=p)
    # the same data with the flags DataPortrait sets: phase 0 fixed, every DM free
    flags = flags.copy()
    flags[15] = 1
    cases["default_flags"] = dict(cases["two_band"], flags=flags, data_of="two_band")
    # two receivers whose channels interleave, tau free, linear evolution
    freqs = np.linspace(1100.0, 1900.0, 16)
    groups = [np.arange(0, 16, 2), np.arange(1, 16, 2)]
    p = np.concatenate([BASE111, [0.0, 0.0, -0.12, 1.5], [-4.0]])
    data, errs = synth("111", p, freqs, 128, 1500.0, groups, P_TWO, 0.02, 32)
    init = p.copy()
    rng = np.random.default_rng(132)
    init[:14] *= 1.0 + 0.03 * rng.uniform(-1, 1, 14)
    init[1] = 2.4
    init[16:18] = [-0.118, 1.47]
    flags = np.ones(len(p), dtype=int)
    flags[[14, 15, -1]] = 0
    cases["overlap_tau"] = dict(code="111", data=data, errs=errs, freqs=freqs, nu_ref=1500.0,
                                P=P_TWO, groups=groups, init=init, flags=flags, p_true=p)
    return cases


PIPE_P = 0.003
PIPE_JOIN = (0.12, 0.005)  # the second archive's phase [rot] and DM offsets


def pipeline_case():
    """Two 8 x 256 archives of example.gmodel with seeded noise, the second
    rotated by PIPE_JOIN about the model's reference frequency, and the joint
    problem a metafile DataPortrait sets up from them (rows sorted by
    frequency, phase 0 fixed, the DMs and the second phase free)."""
    mf = os.path.join(os.path.dirname(pplib.__file__), "data", "example.gmodel")
    name, code, nu_ref, ngauss, params, flags, alpha, fit_alpha = pplib.read_model(mf)
    fa, fb = np.linspace(1150.0, 1360.0, 8), np.linspace(1400.0, 1680.0, 8)
    freqs = np.concatenate([fa, fb])
    groups = [np.arange(8), np.arange(8, 16)]
    p = np.concatenate([params, [0.0, 0.0], PIPE_JOIN, [alpha]])
    data, errs = synth(code, p, freqs, 256, nu_ref, groups, PIPE_P, 0.02, 41)
    fl = np.concatenate([flags, [0, 1, 1, 1], [fit_alpha]]).astype(int)
    fl[1] = 0  # TAU = 0 stays fixed: at its bound the transform's gradient is 0
    return dict(code=code, data=data, errs=errs, freqs=freqs, nu_ref=nu_ref, P=PIPE_P,
                groups=groups, init=p, flags=fl, p_true=p)


def main():
    out = {}
    cases = fit_cases()
    for name, c in cases.items():
        pr = Problem(c["code"], c["data"], c["errs"], c["freqs"], c["nu_ref"], c["init"],
                     c["flags"], c["groups"], c["P"])
        ref, truth = pr.solve(False), pr.solve(True)
        free = pr.free
        d_ref = np.max(np.abs(ref["p"] - truth["p"])[free] / truth["sig"][free])
        rel = np.max(np.abs(ref["sig"][free] / truth["sig"][free] - 1.0))
        print("%s: ref ier %d nfev %d, truth ier %d nfev %d; chi2_ref - chi2_truth %.3e "
              "(chi2 %.6f, dof %d); max|p_ref - p_truth|/sigma %.3e; stderr rel %.2e"
              % (name, ref["ier"], ref["nfev"], truth["ier"], truth["nfev"],
                 ref["chi2"] - truth["chi2"], truth["chi2"], truth["dof"], d_ref, rel))
        # the conditions on a fixture
        assert ref["ier"] in (1, 2, 3) and truth["ier"] in (1, 2, 3), name
        assert np.isfinite(d_ref), name
        if "data_of" not in c:
            out.update({name + "_data": c["data"], name + "_errs": c["errs"],
                        name + "_freqs": c["freqs"]})
        out.update({name + "_code": np.array(c["code"]), name + "_nu_ref": np.array(c["nu_ref"]),
                    name + "_data_of": np.array(c.get("data_of", name)),
                    name + "_P": np.array(c["P"]),
                    name + "_join_of": join_of(c["groups"], len(c["freqs"])),
                    name + "_init": c["init"], name + "_flags": c["flags"],
                    name + "_p_true": c["p_true"], name + "_p_ref": ref["p"],
                    name + "_chi2_ref": np.array(ref["chi2"]), name + "_sig_ref": ref["sig"],
                    name + "_p_truth": truth["p"], name + "_sig_truth": truth["sig"],
                    name + "_chi2_truth": np.array(truth["chi2"]),
                    name + "_dof": np.array(truth["dof"])})
    c = pipeline_case()
    pr = Problem(c["code"], c["data"], c["errs"], c["freqs"], c["nu_ref"], c["init"], c["flags"],
                 c["groups"], c["P"])
    truth = pr.solve(True)
    print("pipe: truth ier %d nfev %d chi2 %.6f; join truth %s +/- %s"
          % (truth["ier"], truth["nfev"], truth["chi2"], truth["p"][-5:-1], truth["sig"][-5:-1]))
    assert truth["ier"] in (1, 2, 3)
    out.update({"pipe_data": c["data"], "pipe_errs": c["errs"], "pipe_freqs": c["freqs"],
                "pipe_join_of": join_of(c["groups"], 16), "pipe_P": np.array(c["P"]),
                "pipe_nu_ref": np.array(c["nu_ref"]), "pipe_flags": c["flags"],
                "pipe_p_true": c["p_true"], "pipe_p_truth": truth["p"],
                "pipe_sig_truth": truth["sig"], "pipe_chi2_truth": np.array(truth["chi2"])})
    path = os.path.join(HERE, "ppgauss_join.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "ppgauss.npz"))


if __name__ == "__main__":
    main()
