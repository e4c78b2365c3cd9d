"""ppf_rotate_fscrunch / Engine.rotate_fscrunch: the weighted sum over
channels of the rotated rows, one profile per unit.

- against numpy, sum_n w irfft(rfft(x) e^{2 pi i k phase}, n = nbin), at
  atol = 1e-12 max|ref| (the bound of this project's transform tests,
  test_gpu_generic_nbin.py): the LDS-FFT kernel (nbin 64, 256), the
  register-FFT one (nbin 2048), the generic-length one (nbin 100 and the odd
  45), zero weights in one unit, in
  all units, a unit of zero weights only, phases beyond +-1 turn;
- three channel slices reducing (nchan = 2 slices + 5), on each kernel;
- a unit's profile is bitwise the same alone and inside a 7-unit call, and
  from call to call; chunking over units under a small workspace limit
  changes nothing;
- against rotate_rows followed by a float64 weighted sum on the device;
- what the entry point refuses, and the empty call."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SLICE = 32  # kFsSlice (csrc/ppfit_kernels.hpp)
SHAPES = [(4, 5, 64), (3, 5, 256), (2, 3, 2048), (3, 5, 100), (3, 4, 45)]


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from pulseportraiture_amd.engine import get_engine
    return get_engine(0)


def reference(x, ph, w):
    nbin = x.shape[-1]
    k = np.arange(nbin // 2 + 1)
    rot = np.fft.irfft(np.fft.rfft(x, axis=-1) * np.exp(2j * np.pi * ph[..., None] * k), n=nbin,
                       axis=-1)
    return (w[..., None] * rot).sum(axis=1)


def inputs(nunit, nchan, nbin, seed=0):
    rng = np.random.default_rng(1000 * nbin + 10 * nchan + nunit + seed)
    x = rng.normal(size=(nunit, nchan, nbin)) + 3.0
    ph = rng.uniform(-2.5, 2.5, (nunit, nchan))  # beyond +-1 turn
    w = rng.uniform(0.5, 2.0, (nunit, nchan))
    return x, ph, w


def test_kernel_slice_constant():
    import os
    import re
    from tests.conftest import ROOT
    txt = open(os.path.join(ROOT, "pulseportraiture_amd", "csrc", "ppfit_kernels.hpp")).read()
    assert int(re.search(r"constexpr int kFsSlice = (\d+);", txt).group(1)) == SLICE


@pytest.mark.parametrize("nunit,nchan,nbin", SHAPES)
def test_against_numpy(eng, nunit, nchan, nbin):
    x, ph, w = inputs(nunit, nchan, nbin)
    w[0, 1] = 0.0       # one channel off in one unit
    w[:, nchan - 1] = 0.0  # one channel off in every unit
    w[nunit - 1] = 0.0  # one unit with no weight at all: zeros
    # a channel of weight 0 is skipped, not multiplied: whatever it holds
    x[0, 1] = np.nan
    got = eng.rotate_fscrunch(x, ph, w).cpu().numpy()
    x[0, 1] = 0.0
    ref = reference(x, ph, w)
    assert got.shape == (nunit, nbin)
    assert np.abs(ref).max() > 1.0
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    assert not got[nunit - 1].any()


@pytest.mark.parametrize("nbin", [64, 100, 2048])
def test_three_slices(eng, nbin):
    nchan = 2 * SLICE + 5
    x, ph, w = inputs(1, nchan, nbin)
    w[0, SLICE] = 0.0
    got = eng.rotate_fscrunch(x, ph, w).cpu().numpy()
    ref = reference(x, ph, w)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize("nchan,nbin", [(5, 64), (2 * SLICE + 5, 64), (5, 2048),
                                        (2 * SLICE + 5, 2048), (5, 100), (2 * SLICE + 5, 100)])
def test_unit_independent_of_the_call(eng, nchan, nbin):
    x, ph, w = inputs(7, nchan, nbin)
    w[3, 2] = 0.0
    all7 = eng.rotate_fscrunch(x, ph, w).cpu().numpy()
    np.testing.assert_array_equal(eng.rotate_fscrunch(x, ph, w).cpu().numpy(), all7)
    for u in (0, 3, 6):
        alone = eng.rotate_fscrunch(x[u:u + 1], ph[u:u + 1], w[u:u + 1]).cpu().numpy()
        np.testing.assert_array_equal(alone[0], all7[u])
    # units in chunks of two under a small workspace limit: the same bits
    nslice = (nchan + SLICE - 1) // SLICE
    per_unit = (nslice + 1) * (nbin // 2 + 1) * 16 + 512
    limit = eng.workspace_limit()
    eng.set_workspace_limit(2 * per_unit + 64)
    try:
        chunked = eng.rotate_fscrunch(x, ph, w).cpu().numpy()
    finally:
        eng.set_workspace_limit(limit)
    np.testing.assert_array_equal(chunked, all7)


@pytest.mark.parametrize("nunit,nchan,nbin", SHAPES)
def test_against_rotate_rows(eng, nunit, nchan, nbin):
    import torch
    x, ph, w = inputs(nunit, nchan, nbin, seed=1)
    w[0, 0] = 0.0
    got = eng.rotate_fscrunch(x, ph, w)
    rot = eng.rotate_rows(torch.as_tensor(x, device=eng.device), ph)
    ref = (torch.as_tensor(w, device=eng.device)[..., None] * rot).sum(dim=1)
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


def test_refusals_and_empty(eng):
    from pulseportraiture_amd.engine import PPFitError
    for nbin in (8, 8200):
        with pytest.raises(PPFitError, match="error -3"):
            eng.rotate_fscrunch(np.zeros((2, 3, nbin)), np.zeros((2, 3)), np.ones((2, 3)))
    out = eng.rotate_fscrunch(np.zeros((0, 3, 64)), np.zeros((0, 3)), np.zeros((0, 3)))
    assert tuple(out.shape) == (0, 64)
    # no channels: an empty sum per unit
    out = eng.rotate_fscrunch(np.zeros((2, 0, 64)), np.zeros((2, 0)), np.zeros((2, 0)))
    assert tuple(out.shape) == (2, 64) and not out.cpu().numpy().any()
    # the C entry point itself: null pointers, nothing to do, and no channels
    # (zeros written first; data, phase and weight are not read)
    import ctypes
    import torch
    lib, ctx = eng.lib, eng.ctx
    assert lib.ppf_rotate_fscrunch(ctx, 1, 1, 64, None, None, None, None) == -1
    prof = torch.ones((2, 64), dtype=torch.float64, device=eng.device)
    p = ctypes.c_void_p(prof.data_ptr())
    assert lib.ppf_rotate_fscrunch(ctx, 2, 0, 64, p, p, p, p) == 0
    eng.synchronize()
    assert not prof.cpu().numpy().any()
    assert lib.ppf_rotate_fscrunch(ctx, 0, 0, 64, ctypes.c_void_p(8), ctypes.c_void_p(8),
                                   ctypes.c_void_p(8), ctypes.c_void_p(8)) == 0
