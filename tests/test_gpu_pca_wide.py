"""The PCA above 2,048 channels: ppf_pca_gram_portraits (ppfit_gram.hip: the
nbin x nbin covariance on the fp64 matrix cores, then the Jacobi on it) and
ppf_pca_project's raised channel cap, against numpy_pca of
tests/test_gpu_pca.py (np.cov + np.linalg.eigh) and to that file's bounds:
ten leading eigenvalues to 1e-12 lambda_0, vectors 0-2 to 64 eps lambda_0 /
gap_i after sign alignment, the mean profile to nchan eps max|port|, info
[<= 15, 1], the sign rule.

The forced-"gram" shapes are the smallest at which the tiling can go wrong:
300 x 80 has a full and a partial 64-bin tile and two slabs of channels (256
+ a ragged 44); 24 x 64 and 16 x 64 have a covariance of rank below nbin, so
they converge only through the Gram path's null threshold.
"""
import ctypes
import functools

import numpy as np
import pytest

from tests.test_gpu_pca import (EPS, check_against, check_sign_rule, numpy_pca,
                                rank_deficient_inputs)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from pulseportraiture_amd.engine import get_engine
    return get_engine(0)


def port_of(nchan, nbin, seed, noise=0.05):
    rng = np.random.default_rng(seed)
    ph = (np.arange(nbin) + 0.5) / nbin
    f = np.linspace(0, 1, nchan)[:, None]
    p = np.exp(-0.5 * ((ph - 0.45 - 0.05 * f) / (0.04 + 0.03 * f)) ** 2) * (1 + 0.5 * f) \
        + 0.4 * np.exp(-0.5 * ((ph - 0.6 + 0.03 * f ** 2) / 0.03) ** 2)
    return p + noise * rng.standard_normal((nchan, nbin)), rng.uniform(0.5, 2.0, nchan)


# key: (nchan, nbin, stride of the zeroed weights or 0)
GENERATED = {"2112x64": (2112, 64, 0), "2049x16": (2049, 16, 0), "4096x128_zap40": (4096, 128, 40),
             "3000x250": (3000, 250, 0), "300x80": (300, 80, 0), "70x64_zap10": (70, 64, 10),
             "24x64": (24, 64, 0)}
DEFAULT = ["2112x64", "2049x16", "4096x128_zap40", "3000x250"]
FORCED = ["300x80", "70x64_zap10", "24x64", "40x16", "16x64_dup_zero"]


@functools.lru_cache(maxsize=None)
def case(key):
    """(port, w, numpy_pca's mean, eigenvalues, vectors): made once per key; no test writes to them."""
    if key in GENERATED:
        nchan, nbin, zap = GENERATED[key]
        port, w = port_of(nchan, nbin, nchan + nbin)
        if zap:
            w[::zap] = 0.0
    else:
        port, w = rank_deficient_inputs()[key]
    return (port, w) + numpy_pca(port, w)


def run_pca(gpu, port, w, ncomp=None, method=None):
    mean, lam, vec, info = gpu.pca_portraits(port, w, ncomp, method)
    return mean.cpu().numpy(), lam.cpu().numpy(), vec.cpu().numpy(), info.cpu().numpy()


def check_case(gpu, key, method):
    port, w, mean_ref, lam_ref, vec_ref = case(key)
    mean, lam, vec, info = run_pca(gpu, port, w, None, method)
    r = min(port.shape)
    assert lam.shape == (r,) and vec.shape == (r, port.shape[1])
    print(key, "sweeps %d, converged %d" % tuple(info))
    e_mean = np.max(np.abs(mean - mean_ref))
    print(key, "mean err %.3g, bound %.3g" % (e_mean, len(port) * EPS * np.max(np.abs(port))))
    assert e_mean <= len(port) * EPS * np.max(np.abs(port))
    assert np.all(np.diff(lam) <= 0.0)
    check_against(lam, vec, lam_ref, vec_ref, [0, 1, 2], key)
    check_sign_rule(vec)
    assert info[1] == 1 and info[0] <= 15, info


@pytest.mark.parametrize("key", DEFAULT)
def test_wide_default_dispatch(gpu, key):
    """More than 2,048 channels: the default takes the Gram path."""
    check_case(gpu, key, None)


@pytest.mark.parametrize("key", FORCED)
def test_gram_forced(gpu, key):
    check_case(gpu, key, "gram")


def test_gram_mean_is_rows_mean_and_default_is_rows(gpu):
    port, w = case("300x80")[:2]
    rows = run_pca(gpu, port, w, None, "rows")
    for a, b in zip(run_pca(gpu, port, w), rows):
        assert np.array_equal(a, b)
    gram = run_pca(gpu, port, w, None, "gram")
    assert np.array_equal(gram[0], rows[0])  # the mean profile, bitwise
    with pytest.raises(ValueError):
        gpu.pca_portraits(port, w, None, "cov")


def test_gram_batch_is_bitwise_single(gpu):
    port = case("300x80")[0]
    rng = np.random.default_rng(3)
    ports = np.stack([port, port[::-1] * 1.5, port + 0.01 * rng.standard_normal(port.shape)])
    ws = np.stack([case("300x80")[1], rng.uniform(0.1, 1.0, 300), np.ones(300)])
    ws[1, 5] = 0.0
    batch = run_pca(gpu, ports, ws, None, "gram")
    again = run_pca(gpu, ports, ws, None, "gram")
    for a, b in zip(batch, again):
        assert np.array_equal(a, b)
    for i in range(3):
        single = run_pca(gpu, ports[i], ws[i], None, "gram")
        for a, b in zip(batch, single):
            assert np.array_equal(a[i], b)
    # ... and of how the workspace limit splits the call over portraits: one
    # portrait's covariance and partial tiles (2 slabs x 3 tile pairs) fit, two do not
    gpu.set_workspace_limit(80 * 80 * 8 + 2 * 3 * 64 * 64 * 8 + 300 * 8 + 16384)
    try:
        split = run_pca(gpu, ports, ws, None, "gram")
    finally:
        gpu.set_workspace_limit(32 << 30)
    for a, b in zip(batch, split):
        assert np.array_equal(a, b)


def test_project_wide(gpu):
    port, w, mean_ref, lam_ref, vec_ref = case("2112x64")
    basis = np.ascontiguousarray(vec_ref[:3])
    proj, rec = gpu.pca_project(port, mean_ref, basis, reconstruct=True)
    ref = np.dot(port - mean_ref, basis.T)
    tol = 1e-12 * np.max(np.abs(port))
    e_proj = np.max(np.abs(proj.cpu().numpy() - ref))
    e_rec = np.max(np.abs(rec.cpu().numpy() - (np.dot(ref, basis) + mean_ref)))
    print("2112x64 proj err %.3g, reconst err %.3g, tol %.3g" % (e_proj, e_rec, tol))
    assert e_proj <= tol and e_rec <= tol


def test_gram_errors(gpu):
    import torch
    from pulseportraiture_amd.engine import PPFitError
    lib, ctx, dev = gpu.lib, gpu.ctx, gpu.device

    def call(nchan, nbin, w, ncomp):
        port = torch.zeros((nchan, nbin), dtype=torch.float64, device=dev)
        wt = torch.as_tensor(np.asarray(w, dtype=np.float64), device=dev)
        nc = max(ncomp, 1)
        mean = torch.empty(nbin, dtype=torch.float64, device=dev)
        lam = torch.empty(nc, dtype=torch.float64, device=dev)
        vec = torch.empty((nc, nbin), dtype=torch.float64, device=dev)
        info = torch.zeros(2, dtype=torch.int32, device=dev)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        rc = lib.ppf_pca_gram_portraits(ctx, 1, nchan, nbin, p(port), p(wt), ncomp, p(mean),
                                        p(lam), p(vec), p(info))
        return rc, lib.ppf_last_error(ctx).decode()

    INVALID, UNSUPPORTED = -1, -3
    bad = [(16385, 16, np.ones(16385), 1, UNSUPPORTED),     # nchan above PPF_MAX_NCHAN
           (8, 4096, np.ones(8), 1, UNSUPPORTED),           # nbin above 2,048
           (1, 64, [1.0], 1, INVALID),                      # nchan 1
           (8, 64, [1, 1, -1, 1, 1, 1, 1, 1], 2, INVALID),  # a negative weight
           (8, 64, [1, 1, np.nan, 1, 1, 1, 1, 1], 2, INVALID),
           (8, 64, [0, 0, 0, 2, 0, 0, 0, 0], 2, INVALID),   # one positive weight
           (8, 64, np.ones(8), 0, INVALID),                 # ncomp 0
           (8, 64, np.ones(8), 9, INVALID),                 # ncomp > min(nchan, nbin)
           (80, 64, np.ones(80), 65, INVALID)]
    for nchan, nbin, w, ncomp, code in bad:
        rc, msg = call(nchan, nbin, w, ncomp)
        assert rc == code and msg, (nchan, nbin, ncomp, rc, msg)
    assert "2048" in call(8, 4096, np.ones(8), 1)[1]
    with pytest.raises(PPFitError):
        gpu.pca_portraits(np.zeros((8, 64)), np.ones(8), 0, "gram")
    # the context stays usable
    check_case(gpu, "70x64_zap10", "gram")
