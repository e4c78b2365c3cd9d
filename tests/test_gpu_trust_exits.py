"""The ways out of the trust-ncg solver, through Engine.fit_batch.

The three kernels that run scipy's trust-region loop -- k_solve (one
workgroup per subint), k_scat_sweep / k_scat_step (the split scattering
solve) and k_fit_taylor (phase family, Taylor moments) -- share one solver
step, and every exit of it ends in the same epilogue (fun, nfev, status, the
accepted slot, grad and hess).  These cases pin what that epilogue writes on
the exits the other tests do not reach: a subint with no fitted channel
(status -1), a partly masked one, the objective-only evaluation
(eval_only: status 1, nfev 1), and grad / hess / fun / cov of the split solve
against the one-workgroup solve, bitwise, at channel counts that give one
sweep block (20, not a multiple of 8) and two (136: split = 2, the second
block's last group partial).

The NaN-gradient exit (status 0) has no case here on purpose: reaching it
means feeding NaN data through the guess and post-fit kernels.  The maxiter
exit is held by test_gpu_taylor.py, the repeat-point count by
test_gpu_configs.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NSUB = 6
MASKED, PARTIAL = 2, 4  # subints with every / three channels masked
SCAT_FLAGS = [1, 1, 0, 1, 1]
PHASE_FLAGS = [1, 1, 0, 0, 0]


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from pulseportraiture_amd.engine import get_engine
    return get_engine(0)


def _keys():
    from pulseportraiture_amd.engine import RESULT_F64
    return [k for k, _ in RESULT_F64] + ["nfev", "status"]


def _mask(nchan):
    mask = np.ones((NSUB, nchan), dtype=np.uint8)
    mask[MASKED] = 0
    mask[PARTIAL, 3:6] = 0
    return mask


def _batch(eng, nchan, nbin, seed, tau=0.0):
    from pulseportraiture_amd import synth
    w = synth.make_workload(NSUB, nchan, nbin, seed=seed, tau=tau)
    return w, eng.synth(w.template, w.phase, w.sigma, w.seed, sub0=w.sub0)


def _fit(eng, w, data, flags, log10_tau, opts=None, **kw):
    from pulseportraiture_amd import pplib
    opts = opts or {}
    saved = {k: eng.get_option(k) for k in opts}
    for k, v in opts.items():
        eng.set_option(k, v)
    try:
        nu = pplib.guess_fit_freq(w.freqs)
        init = np.tile([0.0, w.DM0, 0.0, 0.0, 0.0], (NSUB, 1))
        gt = None
        if flags[3]:
            tg = 2e-3 * (nu / w.nu_ref) ** w.alpha
            init[:, 3], init[:, 4] = np.log10(tg), w.alpha
            gt = np.full(NSUB, tg)
        out = eng.fit_batch(data, w.model, w.freqs, w.P, init, flags, nu_fit=[nu] * 3,
                            log10_tau=log10_tau, guess=True, guess_Ns=100, guess_tau=gt,
                            chan_mask=_mask(data.shape[1]), **kw)
        return {k: out[k].cpu().numpy() for k in _keys()}
    finally:
        for k, v in saved.items():
            eng.set_option(k, v)


# what the library writes for a subint with no fitted channel; its rows of
# the other keys are never written (whatever the result buffer held)
MASKED_KEYS = ["params", "param_errs", "scales", "scale_errs", "channel_snrs", "grad", "hess",
               "errs", "nfev", "status"]


def _same(a, b, keys):
    rows = _fitted()
    for k in keys:
        if k in MASKED_KEYS:
            assert np.array_equal(a[k], b[k], equal_nan=True), k
        else:
            assert np.array_equal(a[k][rows], b[k][rows], equal_nan=True), k


def _fitted():
    return [i for i in range(NSUB) if i != MASKED]


@pytest.fixture(scope="module", params=[20, 136])
def scat_batch(request, gpu):
    nchan = request.param
    return _batch(gpu, nchan, 128, seed=5100 + nchan, tau=2e-3)


def test_scattering_split_matches_one_workgroup(gpu, scat_batch):
    w, data = scat_batch
    one = _fit(gpu, w, data, SCAT_FLAGS, True, opts={"scat_split": 0})
    spl = _fit(gpu, w, data, SCAT_FLAGS, True, opts={"scat_split": 1})
    _same(one, spl, _keys())
    for r in (one, spl):
        assert r["status"][MASKED] == -1 and r["nfev"][MASKED] == 0
        for k in ("params", "grad", "hess"):
            assert np.isnan(r[k][MASKED]).all(), k
        assert (r["status"][_fitted()] >= 0).all()
        for k in ("grad", "hess", "fun"):
            assert np.isfinite(r[k][_fitted()]).all(), k
        plain = [i for i in _fitted() if i != PARTIAL]
        assert (r["nfev"][plain] > 8).any()  # past the first graph group


def test_scattering_eval_only(gpu, scat_batch):
    w, data = scat_batch
    one = _fit(gpu, w, data, SCAT_FLAGS, True, opts={"scat_split": 0}, eval_only=True)
    spl = _fit(gpu, w, data, SCAT_FLAGS, True, opts={"scat_split": 1}, eval_only=True)
    for r in (one, spl):
        assert (r["status"][_fitted()] == 1).all() and (r["nfev"][_fitted()] == 1).all()
        assert r["status"][MASKED] == -1 and r["nfev"][MASKED] == 0
    _same(one, spl, ["grad", "hess"])
    assert np.isfinite(one["grad"][_fitted()]).all() and np.isfinite(one["hess"][_fitted()]).all()


def test_phase_family_eval_only(gpu):
    w, data = _batch(gpu, 16, 256, seed=5200)
    for exact in (False, True):  # k_fit_taylor, k_solve<false>
        r = _fit(gpu, w, data, PHASE_FLAGS, False, eval_only=True, exact=exact)
        assert (r["status"][_fitted()] == 1).all() and (r["nfev"][_fitted()] == 1).all(), exact
        assert r["status"][MASKED] == -1 and r["nfev"][MASKED] == 0, exact
