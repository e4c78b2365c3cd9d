"""Taylor-moment solver (ppfit_taylor.hip) against the exact cross-spectrum
sweeps on the device and against the oracle.

The Taylor path replaces every trust-ncg evaluation of a phase-family fit by
a per-channel series that is exact to fp64 rounding (truncation < 1e-17 of the
sum magnitudes), so it must reproduce the exact path's parameters far inside
the north_star tolerance (|dphi| <= 1e-3 sigma_phi, |dDM| <= 1e-3 sigma_DM),
with identical solver status.  The bar is the north_star tolerance both
between the two device paths and against the oracle: with gtol = -1 the last
accepted trust-ncg step is chosen where the predicted reduction is at the
objective's rounding floor, so a different (equally exact) summation order of
the moments moves the stopping point by up to a few 1e-4 sigma (seen: 2e-4
sigma on 2 of 6 subints at 16 x 256 when the moment sweep was split into two
accumulator chains).

nfev is counted as scipy counts it (a proposal that repeats the last
evaluated point is memoised, not re-evaluated) and compared within four:
with gtol = -1 trust-ncg stops when the predicted reduction rounds to <= 0,
and the last accept / reject decisions before that are taken on differences
at the objective's rounding, where the two paths' sums differ.
"""
import numpy as np
import pytest

from oracle import ppfit_oracle as O
from pulseportraiture_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from pulseportraiture_amd.engine import Engine
    return Engine(0)


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items() if not k.startswith("_")}


def _pair(eng, w, data, flags, init, mask=None, guess=True, **kw):
    nu = O.guess_fit_freq(w.freqs)
    args = dict(nu_fit=[nu, nu, nu], chan_mask=mask, guess=guess, **kw)
    t = _np(eng.fit_batch(data, w.model, w.freqs, w.P, init, flags, **args))
    e = _np(eng.fit_batch(data, w.model, w.freqs, w.P, init, flags, exact=True, **args))
    return t, e


def _statuses_agree(t, e):
    """Identical status, except for scipy's exact-zero-gradient stop: when the
    gradient at the accepted point rounds to exactly 0.0, Steihaug CG returns
    a NaN step (0/0 in get_boundaries_intersections), no proposal is ever
    accepted and trust-ncg ends at maxiter (status 1, nfev 1001) -- as the
    reference does on the same rounding.  Whether the last Newton step lands
    on a point whose float gradient is exactly 0 depends on summation order
    (observed ~1 in 10^3 converged subints), so the two device paths may
    differ there while their parameters agree to rounding."""
    for i in np.where(t["status"] != e["status"])[0]:
        pair = {int(t["status"][i]), int(e["status"][i])}
        assert pair == {1, 2} and max(t["nfev"][i], e["nfev"][i]) == 1001, (i, pair)


def _assert_close(t, e, flags, tol=1e-3):
    _statuses_agree(t, e)
    assert np.abs(t["nfev"] - e["nfev"]).max() <= 4, (t["nfev"], e["nfev"])
    for i in range(5):
        if flags[i]:
            sig = e["param_errs"][:, i]
            assert np.all(np.abs(t["params"][:, i] - e["params"][:, i]) <= tol * sig), i
            np.testing.assert_allclose(t["param_errs"][:, i], sig, rtol=1e-6)
    np.testing.assert_allclose(t["nu_out"], e["nu_out"], rtol=1e-9)
    np.testing.assert_allclose(t["red_chi2"], e["red_chi2"], rtol=1e-10)
    np.testing.assert_allclose(t["snr"], e["snr"], rtol=1e-9)
    np.testing.assert_allclose(t["scales"], e["scales"], rtol=1e-7, atol=1e-12)
    np.testing.assert_allclose(t["scale_errs"], e["scale_errs"], rtol=1e-7, atol=1e-12)


@pytest.mark.parametrize("nbin,nchan", [(64, 4), (128, 8), (256, 16), (1024, 33), (2048, 64),
                                        (4096, 8), (8192, 4)])
def test_taylor_matches_exact_phase_dm(eng, nbin, nchan):
    w = synth.make_workload(6, nchan, nbin, seed=100 + nbin)
    data = synth.workload_data_host(w)
    init = np.array([[0.0, w.DM0, 0, 0, 0]] * 6)
    t, e = _pair(eng, w, data, [1, 1, 0, 0, 0], init)
    _assert_close(t, e, [1, 1, 0, 0, 0])


@pytest.mark.parametrize("flags", [[1, 0, 0, 0, 0], [1, 1, 1, 0, 0], [1, 0, 1, 0, 0]])
def test_taylor_matches_exact_flags(eng, flags):
    w = synth.make_workload(5, 32, 512, seed=7, gm=2e-6)
    data = synth.workload_data_host(w)
    init = np.array([[0.0, w.DM0, 0, 0, 0]] * 5)
    t, e = _pair(eng, w, data, flags, init)
    _assert_close(t, e, flags)


def test_taylor_masked_channels(eng):
    w = synth.make_workload(4, 48, 1024, seed=21)
    data = synth.workload_data_host(w)
    mask = np.ones((4, 48), np.uint8)
    mask[0, ::3] = 0
    mask[1, :40] = 0
    mask[2, 47] = 0
    init = np.array([[0.0, w.DM0, 0, 0, 0]] * 4)
    t, e = _pair(eng, w, data, [1, 1, 0, 0, 0], init, mask=mask)
    _assert_close(t, e, [1, 1, 0, 0, 0])
    assert np.all(t["scales"][mask == 0] == 0.0)


def test_taylor_recentres_far_start(eng):
    """No guess and a start 0.002-0.01 rot / 0.005 DM off: the first
    proposals leave the radius (|y| ~ 6-30 > 3), so the subints park and
    recentre; results must still match the exact path and the oracle.  (From
    much farther starts trust-ncg's status-2 stop becomes trajectory-
    sensitive and the reference itself moves by ~1e-3 sigma with rounding.)"""
    nsub, nchan, nbin = 6, 16, 1024
    w = synth.make_workload(nsub, nchan, nbin, seed=5)
    data = synth.workload_data_host(w)
    nu = O.guess_fit_freq(w.freqs)
    init = np.zeros((nsub, 5))
    init[:, 0] = -w.phi + np.linspace(0.002, 0.01, nsub)
    init[:, 1] = w.DM0 + w.dDM + 0.005 * np.array([1, -1, 1, 0, 1, -1])
    # rotate the true phase to nu_fit for the start: phase at nu_ref -> nu_fit
    init[:, 0] = [O.phase_transform(p, d, w.nu_ref, nu, w.P) for p, d in zip(init[:, 0], init[:, 1])]
    t, e = _pair(eng, w, data, [1, 1, 0, 0, 0], init, guess=False)
    _assert_close(t, e, [1, 1, 0, 0, 0])
    errs = np.array([O.get_noise_PS(d, chans=True) for d in data])
    for i in range(nsub):
        ref = O.fit_portrait_full(data[i], w.model, list(init[i]), w.P, w.freqs, [nu] * 3,
                                  [None] * 3, errs[i], [1, 1, 0, 0, 0], log10_tau=False)
        assert t["status"][i] == ref.return_code
        assert abs(t["params"][i][0] - ref.phi) <= 1e-3 * ref.phi_err
        assert abs(t["params"][i][1] - ref.DM) <= 1e-3 * ref.DM_err


def test_taylor_vs_oracle_headline_shape(eng):
    """Config 2's shape (64 x 2048, guess + phase+DM) against the oracle."""
    nsub = 4
    w = synth.make_workload(nsub, 64, 2048, seed=77)
    data = synth.workload_data_host(w)
    nu = O.guess_fit_freq(w.freqs)
    out = _np(eng.fit_batch(data, w.model, w.freqs, w.P, [0.0, w.DM0, 0, 0, 0], [1, 1, 0, 0, 0],
                            nu_fit=[nu, nu, nu], guess=True))
    errs = np.array([O.get_noise_PS(d, chans=True) for d in data])
    for i in range(nsub):
        ref = O.fit_portrait_full(data[i], w.model, list(out["init_used"][i]), w.P, w.freqs,
                                  [nu] * 3, [None] * 3, errs[i], [1, 1, 0, 0, 0],
                                  log10_tau=False)
        assert out["status"][i] == ref.return_code
        assert abs(out["params"][i][0] - ref.phi) <= 1e-3 * ref.phi_err
        assert abs(out["params"][i][1] - ref.DM) <= 1e-3 * ref.DM_err
        assert out["param_errs"][i][0] == pytest.approx(ref.phi_err, rel=1e-6)
        assert out["red_chi2"][i] == pytest.approx(ref.red_chi2, rel=1e-9)


def test_taylor_vs_oracle_headline_masked(eng):
    """64 x 2048 (the register-FFT data pass) with masked channels against the
    oracle fitting only the unmasked channels, as get_TOAs does with its
    zero-weight channels removed."""
    nsub, nchan = 3, 64
    w = synth.make_workload(nsub, nchan, 2048, seed=91)
    data = synth.workload_data_host(w)
    mask = np.ones((nsub, nchan), np.uint8)
    mask[0, ::4] = 0
    mask[1, 32:] = 0
    mask[2, [0, 1, 62, 63]] = 0
    nu = O.guess_fit_freq(w.freqs)
    out = _np(eng.fit_batch(data, w.model, w.freqs, w.P, [0.0, w.DM0, 0, 0, 0], [1, 1, 0, 0, 0],
                            nu_fit=[nu, nu, nu], chan_mask=mask, guess=True))
    for i in range(nsub):
        ok = mask[i].astype(bool)
        errs = O.get_noise_PS(data[i][ok], chans=True)
        ref = O.fit_portrait_full(data[i][ok], w.model[ok], list(out["init_used"][i]), w.P,
                                  w.freqs[ok], [nu] * 3, [None] * 3, errs, [1, 1, 0, 0, 0],
                                  log10_tau=False)
        assert out["status"][i] == ref.return_code
        assert abs(out["params"][i][0] - ref.phi) <= 1e-3 * ref.phi_err
        assert abs(out["params"][i][1] - ref.DM) <= 1e-3 * ref.DM_err
        assert out["param_errs"][i][0] == pytest.approx(ref.phi_err, rel=1e-6)
        assert out["red_chi2"][i] == pytest.approx(ref.red_chi2, rel=1e-9)
        assert np.all(out["scales"][i][~ok] == 0.0)


@pytest.mark.parametrize("pieces", [2, 3, 8])
def test_pipeline_pieces_bitwise(eng, pieces):
    """The two-queue piece pipeline (ppf_set_pipeline) runs the same kernels on
    disjoint workspace slices: results are bitwise those of one queue, also
    for a chunk smaller than the batch (workspace limit) and ragged pieces."""
    nsub = 301
    w = synth.make_workload(nsub, 64, 2048, seed=123)
    data = synth.workload_data_host(w)
    nu = O.guess_fit_freq(w.freqs)
    args = (data, w.model, w.freqs, w.P, [0.0, w.DM0, 0, 0, 0], [1, 1, 0, 0, 0])
    try:
        eng.set_pipeline(1)
        ref = _np(eng.fit_batch(*args, nu_fit=[nu, nu, nu], guess=True))
        eng.set_pipeline(pieces)
        out = _np(eng.fit_batch(*args, nu_fit=[nu, nu, nu], guess=True))
        eng.set_workspace_limit(120 * 1100 * 1024)  # chunks of ~110 subints
        out2 = _np(eng.fit_batch(*args, nu_fit=[nu, nu, nu], guess=True))
    finally:
        eng.set_pipeline(0)
        eng.set_workspace_limit(32 << 30)
    for o in (out, out2):
        for k in ["params", "param_errs", "nu_out", "cov", "scales", "red_chi2", "snr", "nfev",
                  "status"]:
            np.testing.assert_array_equal(o[k], ref[k], err_msg=k)


def test_pipeline_mixed_tau_bitwise(eng):
    """Subints that start with tau != 0 (tau not fitted) leave the Taylor path
    for the pipeline's k_solve<true> leg.  Mixed with Taylor subints, over
    ragged pieces and several chunks, every result is bitwise that of one
    queue."""
    nsub, nchan, nbin = 26, 32, 256
    w = synth.make_workload(nsub, nchan, nbin, seed=321)
    data = synth.workload_data_host(w)
    nu = O.guess_fit_freq(w.freqs)
    init = np.zeros((nsub, 5))
    init[:, 1] = w.DM0
    init[::3, 3] = 1e-3
    args = (data, w.model, w.freqs, w.P, init, [1, 1, 0, 0, 0])

    def run():
        eng.reset_kernel_times()
        out = _np(eng.fit_batch(*args, nu_fit=[nu, nu, nu], guess=True))
        return out, eng.kernel_time("data_xspec")[1]

    try:
        eng.set_timing(True)
        eng.set_pipeline(1)
        ref, _ = run()
        eng.set_pipeline(3)
        out, n_whole = run()
        eng.set_workspace_limit(900000)  # ~104 KB a subint: chunks of 8, 8, 8, 2
        out2, n_chunked = run()
    finally:
        eng.set_timing(False)
        eng.set_pipeline(0)
        eng.set_workspace_limit(32 << 30)
    # one data pass per piece: 3 + 3 + 3 + 2 against 3
    assert n_chunked > 3 and n_chunked > n_whole, (n_whole, n_chunked)
    for o in (out, out2):
        assert o.keys() == ref.keys()
        for k in ref:
            assert np.array_equal(o[k], ref[k]), k
