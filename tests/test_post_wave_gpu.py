"""The one-wave post-fit k_post_w against the block's k_post<false>.

post_wave (ppf_set_option) moves the phase-family post-fit of a subint from a
256-thread workgroup to one wave that plays the block's threads
(csrc/ppfit_vthread.hpp): every sum keeps the block's operands and order, so
every output must be bitwise the same with the option off and on, NaNs in
the same places.  The shapes are the smallest at which a wave version can go
wrong: fewer channels than an 8-channel group, a partial group, one more than
a group, one more than the 32 rows of the block's sweep table, 64 channels
(one slot of the wave), 72 (a second slot with one group), 100 and 128 (the
dispatch rule's limit: four slots, every row of the block's table in use) and
130, where the rule leaves every subint with the block.  Also the default
path (now the wave kernel) on the committed headline fixture, with the
values and tolerances of
test_gpu_configs.test_headline_2000_subints_vs_reference.
"""
import itertools
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN
from tests.golden_consts import DM0

pytestmark = pytest.mark.gpu

NSUB, NBIN = 7, 64
FLAGS = {"phi": [1, 0, 0, 0, 0], "phi_dm": [1, 1, 0, 0, 0], "phi_dm_gm": [1, 1, 1, 0, 0]}


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from pulseportraiture_amd.engine import get_engine
    return get_engine(0)


_WORK = {}


def _workload(gpu, nchan):
    """(workload, device data) of NSUB subints at nchan x NBIN, made once."""
    if nchan not in _WORK:
        from pulseportraiture_amd import synth
        w = synth.make_workload(NSUB, nchan, NBIN, seed=9100 + nchan)
        _WORK[nchan] = (w, gpu.synth(w.template, w.phase, w.sigma, w.seed, sub0=w.sub0))
    return _WORK[nchan]


def _fit(gpu, w, data, flags, post_wave, **kw):
    from pulseportraiture_amd import pplib
    saved = gpu.get_option("post_wave")
    gpu.set_option("post_wave", post_wave)
    try:
        nu = pplib.guess_fit_freq(w.freqs)
        out = gpu.fit_batch(data, w.model, w.freqs, w.P, [0.0, w.DM0, 0.0, 0.0, 0.0], flags,
                            nu_fit=[nu] * 3, guess=True, guess_Ns=100, **kw)
        return {k: v.cpu().numpy() for k, v in out.items() if not k.startswith("_")}
    finally:
        gpu.set_option("post_wave", saved)


def _same(a, b):
    assert set(a) == set(b)
    for k in sorted(a):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        # the bit patterns: NaNs in the same places, signed zeros alike
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def _both(gpu, nchan, flags, **kw):
    w, data = _workload(gpu, nchan)
    off = _fit(gpu, w, data, flags, 0, **kw)
    on = _fit(gpu, w, data, flags, 1, **kw)
    _same(off, on)
    return on


def test_option_default_and_roundtrip(gpu):
    assert gpu.get_option("post_wave") == 1
    gpu.set_option("post_wave", 0)
    assert gpu.get_option("post_wave") == 0
    gpu.set_option("post_wave", 1)


@pytest.mark.parametrize("nchan", [1, 5, 8, 9, 33, 64, 72, 100, 128, 130])
def test_post_wave_bitwise(gpu, nchan):
    """Every flag set, nu_out given and NaN (the zero-covariance frequencies,
    for phi+DM+GM through the cubic's root finder), is_toa on and off; the
    no-scales covariance (cov_nosc) is among the outputs of every fit."""
    nu_given = np.array([1390.0, 1455.0, 1520.0])
    for (name, flags), nu_out, is_toa in itertools.product(
            FLAGS.items(), (None, nu_given), (True, False)):
        r = _both(gpu, nchan, flags, nu_out=nu_out, is_toa=is_toa)
        assert "cov_nosc" in r and r["status"].shape == (NSUB,), name
        if nu_out is not None and not is_toa:
            assert np.array_equal(r["nu_out"], np.tile(nu_given, (NSUB, 1))), name


@pytest.mark.parametrize("nchan", [9, 33, 64, 100])
@pytest.mark.parametrize("fname", ["phi_dm", "phi_dm_gm"])
def test_post_wave_masked_bitwise(gpu, nchan, fname):
    """Masked channels: a few per subint at places that leave partial groups,
    one subint with a single channel left, and one with every channel masked
    (the `bad` path: status -1, NaN parameters)."""
    rng = np.random.default_rng(77 + nchan)
    mask = (rng.random((NSUB, nchan)) > 0.3).astype(np.uint8)
    mask[0] = 1
    mask[1, 0] = 0           # the first channel of the first group
    mask[1, nchan - 1] = 0   # the last channel of the last group
    mask[2] = 0
    mask[3] = 0
    mask[3, nchan // 2] = 1
    mask[4:, 1] = 1          # at least two channels on the rest
    mask[4:, nchan - 2] = 1
    r = _both(gpu, nchan, FLAGS[fname], chan_mask=mask)
    assert int(r["status"][2]) == -1 and np.isnan(r["params"][2]).all()
    assert (r["status"][[0, 1, 4, 5, 6]] != -1).all()
    assert (r["scales"][mask == 0] == 0).all()
    r = _both(gpu, nchan, FLAGS[fname], chan_mask=mask, nu_out=[1400.0, 1400.0, 1500.0])
    assert int(r["status"][2]) == -1


@pytest.mark.parametrize("nchan", [5, 33, 64])
def test_post_wave_weights_bitwise(gpu, nchan):
    """Non-unit channel weights, with and without masked channels."""
    rng = np.random.default_rng(5 + nchan)
    wts = rng.uniform(0.25, 4.0, (NSUB, nchan))
    mask = np.ones((NSUB, nchan), np.uint8)
    mask[:, nchan // 3] = 0
    for flags in FLAGS.values():
        _both(gpu, nchan, flags, weights=wts)
        _both(gpu, nchan, flags, weights=wts, chan_mask=mask)


def test_headline_fixture_default_path(gpu):
    """The first 64 subints of headline_2k.npz (64 x 2048, phase + DM, guess +
    trust-ncg) through the default path, against the reference's values with
    test_headline_2000_subints_vs_reference's tolerances."""
    from pulseportraiture_amd import synth
    assert gpu.get_option("post_wave") == 1
    z = np.load(os.path.join(GOLDEN, "headline_2k.npz"))
    n, seed = 64, int(z["seed"])
    data = np.stack([synth.workload_data_host(synth.make_workload(1, 64, 2048, seed=seed,
                                                                  sub0=i))[0] for i in range(n)])
    w = synth.make_workload(1, 64, 2048, seed=seed)
    nu = z["nu_fit"][:n]
    out = gpu.fit_batch(data, w.model, w.freqs, w.P, [0.0, DM0, 0, 0, 0], [1, 1, 0, 0, 0],
                        nu_fit=np.stack([nu] * 3, 1), guess=True, guess_Ns=100)
    r = {k: v.cpu().numpy() for k, v in out.items() if not k.startswith("_")}
    np.testing.assert_allclose(r["init_used"][:, 0], z["phi_guess"][:n], rtol=0, atol=1e-6)
    assert np.array_equal(r["status"], z["status"][:n].astype(int))
    dphi = np.abs(r["params"][:, 0] - z["phi"][:n]) / z["phi_err"][:n]
    ddm = np.abs(r["params"][:, 1] - z["DM"][:n]) / z["DM_err"][:n]
    dn = r["nfev"] - z["nfev"][:n].astype(int)
    print("headline 64: |dphi|/sigma max %.3g |dDM|/sigma max %.3g nfev equal on %d of %d, "
          "max |dnfev| %d" % (dphi.max(), ddm.max(), (dn == 0).sum(), n, np.abs(dn).max()))
    assert dphi.max() <= 1e-3 and ddm.max() <= 1e-3
    np.testing.assert_allclose(r["param_errs"][:, 0], z["phi_err"][:n], rtol=1e-6)
    np.testing.assert_allclose(r["red_chi2"], z["red_chi2"][:n], rtol=1e-9)
    np.testing.assert_allclose(r["snr"], z["snr"][:n], rtol=1e-8)
    assert np.abs(dn).max() <= 4 and (dn == 0).mean() >= 0.75
