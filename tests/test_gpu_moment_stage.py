"""The staged first moment pass of k_fit_taylor against k_moments.

With fuse_moments 1 (the default) the first moment pass runs inside
k_fit_taylor and fetches X by rows through LDS, one block of 16 harmonics
ahead (moment_tile16_staged); with fuse_moments 0 it is k_moments' launch,
whose lanes load their own cells directly (moment_tile16).  Both feed every
MFMA the same operands in the same order, so the moments and with them every
fit output are equal bit for bit.  Each case fits one small batch twice on
one engine, staged and then direct, at a shape that takes another path
through the staging: partial blocks and tiles, idle waves, a wave with two
tiles, the LDS region shared with the T copy, generic and odd nbin, masks,
the GM leg and the HBM channel tables."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ["params", "param_errs", "nu_out", "red_chi2", "snr", "nfev", "status", "init_used",
        "scales", "cov"]
PD, PDG = [1, 1, 0, 0, 0], [1, 1, 1, 0, 0]


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from pulseportraiture_amd.engine import get_engine
    return get_engine(0)


def _masks(nsub, nchan):
    """test_taylor_masked_channels' masks: alternate channels, a whole tile
    (and more), the last channel."""
    mask = np.ones((nsub, nchan), np.uint8)
    mask[0, ::3] = 0
    mask[1, :40] = 0
    mask[2, nchan - 1] = 0
    return mask


def _fit(eng, w, data, flags, mask, **opts):
    from pulseportraiture_amd import pplib
    saved = {k: eng.get_option(k) for k in opts}
    for k, v in opts.items():
        eng.set_option(k, v)
    try:
        nu = pplib.guess_fit_freq(w.freqs)
        init = np.tile([0.0, w.DM0, 0.0, 0.0, 0.0], (w.nsub, 1))
        out = eng.fit_batch(data, w.model, w.freqs, w.P, init, flags, nu_fit=[nu] * 3,
                            chan_mask=mask, guess=True, guess_Ns=100)
        return {k: out[k].cpu().numpy() for k in KEYS}
    finally:
        for k, v in saved.items():
            eng.set_option(k, v)


CASES = [
    # id, nchan, nbin, flags, gm, masked, options
    ("4x64_partial_block_idle_waves", 4, 64, PD, 0.0, False, {}),
    ("33x1024_one_channel_tile", 33, 1024, PD, 0.0, False, {}),
    ("64x2048_headline", 64, 2048, PD, 0.0, False, {}),
    ("80x512_two_tiles_on_wave0", 80, 512, PD, 0.0, False, {}),
    ("256x256_shares_T_copy", 256, 256, PD, 0.0, False, {}),
    ("16x100_generic_nbin", 16, 100, PD, 0.0, False, {}),
    ("16x99_odd_nbin", 16, 99, PD, 0.0, False, {}),
    ("48x1024_masked", 48, 1024, PD, 0.0, True, {}),
    ("64x2048_gm", 64, 2048, PDG, 2e-6, False, {}),
    ("33x1024_hbm_tables", 33, 1024, PD, 0.0, False, {"hbm_tables": 1}),
]


@pytest.mark.parametrize("nchan,nbin,flags,gm,masked,opts", [c[1:] for c in CASES],
                         ids=[c[0] for c in CASES])
def test_staged_moments_bitwise(gpu, nchan, nbin, flags, gm, masked, opts):
    from pulseportraiture_amd import synth
    nsub = 3
    w = synth.make_workload(nsub, nchan, nbin, seed=1000 + nchan + nbin, gm=gm)
    data = synth.workload_data_host(w)
    mask = _masks(nsub, nchan) if masked else None
    staged = _fit(gpu, w, data, flags, mask, fuse_moments=1, **opts)
    direct = _fit(gpu, w, data, flags, mask, fuse_moments=0, **opts)
    assert np.isfinite(staged["params"][:, :2]).all()
    for k in KEYS:
        assert np.array_equal(staged[k], direct[k]), \
            (k, int(np.isnan(np.asarray(staged[k], float)).sum()))
