"""ppf_pca_portraits / ppf_pca_project (ppfit_pca.hip) against the reference's
pca (np.cov + np.linalg.eigh; tests/golden/make_golden_ppspline.py) and
against numpy on rank-deficient shapes built here.

Bounds: eigenvalues to 1e-12 lambda_0 (eigh's O(n eps |C|) backward error);
a significant eigenvector to 64 eps lambda_0 / gap_i in the max norm after
aligning its sign (Davis-Kahan: gap_i = distance to the nearest other
eigenvalue); projections and reconstructions to 1e-12 max|port|.
"""
import ctypes
import json
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from pulseportraiture_amd.engine import get_engine
    return get_engine(0)


@pytest.fixture(scope="module")
def fx():
    return (np.load(os.path.join(GOLDEN, "ppspline.npz")),
            np.load(os.path.join(GOLDEN, "ppspline_models.npz")),
            json.load(open(os.path.join(GOLDEN, "ppspline.json"))))


CASES = ["32x256", "20x250", "24x128", "16x64", "48x512"]


def run_pca(gpu, port, w, ncomp=None):
    mean, lam, vec, info = gpu.pca_portraits(port, w, ncomp)
    return mean.cpu().numpy(), lam.cpu().numpy(), vec.cpu().numpy(), info.cpu().numpy()


def check_sign_rule(vec):
    for v in vec:
        if np.any(v):
            assert v[np.argmax(np.abs(v))] > 0.0


def gaps(lam):
    d = np.abs(lam[:, None] - lam[None, :])
    np.fill_diagonal(d, np.inf)
    return d.min(axis=1)


def check_against(lam, vec, lam_ref, vec_ref, which, tag):
    """lam_ref: every reference eigenvalue (descending); vec_ref rows."""
    n = min(10, len(lam))
    dl = np.max(np.abs(lam[:n] - lam_ref[:n]))
    print(tag, "max |dlambda| / lambda_0 = %.3g" % (dl / lam_ref[0]))
    assert dl <= 1e-12 * lam_ref[0], (tag, dl / lam_ref[0])
    gap = gaps(lam_ref)
    for i in which:
        s = np.sign(np.dot(vec[i], vec_ref[i]))
        err = np.max(np.abs(s * vec[i] - vec_ref[i]))
        bound = 64 * EPS * lam_ref[0] / gap[i]
        print(tag, "vector %d: err %.3g, bound %.3g" % (i, err, bound))
        assert err <= bound, (tag, i, err, bound)


@pytest.mark.parametrize("key", CASES)
def test_pca_matches_reference(gpu, fx, key):
    z, _, meta = fx
    port, w = z["port_" + key], z["pca_weights_" + key]
    mean, lam, vec, info = run_pca(gpu, port, w)
    assert lam.shape == (min(port.shape),) and vec.shape == (min(port.shape), port.shape[1])
    # (nchan additions, each rounding by at most eps / 2 of a partial sum)
    assert np.max(np.abs(mean - z["mean_prof_" + key])) <= len(port) * EPS * np.max(np.abs(port))
    assert np.all(np.diff(lam) <= 0.0)
    check_against(lam, vec, z["eigval_" + key], z["eigvec10_" + key], meta["cases"][key]["ieig"],
                  key)
    check_sign_rule(vec)
    print(key, "sweeps %d, converged %d" % tuple(info))
    assert info[1] == 1 and info[0] <= 15, info


def numpy_pca(port, w):
    mean = (port.T * w).T.sum(axis=0) / w.sum()
    lam, vec = np.linalg.eigh(np.cov((port - mean).T, aweights=w, ddof=1))
    return mean, lam[::-1], vec[:, ::-1].T


def rank_deficient_inputs():
    rng = np.random.default_rng(11)
    out = {}
    for nchan, nbin in [(24, 16), (40, 16), (33, 100), (256, 64)]:
        out["%dx%d" % (nchan, nbin)] = (rng.standard_normal((nchan, nbin)),
                                        rng.uniform(0.5, 2.0, nchan))
    port, w = rng.standard_normal((16, 64)), rng.uniform(0.5, 2.0, 16)
    port[7] = port[2]   # a duplicated row
    port[11], w[11] = 0.0, 0.0  # a zero-weight all-zero row
    out["16x64_dup_zero"] = (port, w)
    return out


@pytest.mark.parametrize("key", ["24x16", "40x16", "16x64_dup_zero", "33x100", "256x64"])
def test_pca_rank_deficient(gpu, key):
    port, w = rank_deficient_inputs()[key]
    mean, lam, vec, info = run_pca(gpu, port, w)
    mean_ref, lam_ref, vec_ref = numpy_pca(port, w)
    assert info[1] == 1 and info[0] <= 15, info
    assert np.max(np.abs(mean - mean_ref)) <= len(port) * EPS * np.max(np.abs(port))
    check_against(lam, vec, lam_ref, vec_ref, [0, 1, 2], key)
    check_sign_rule(vec)


def test_pca_batch_is_bitwise_single(gpu, fx):
    z = fx[0]
    port = z["port_32x256"]
    rng = np.random.default_rng(3)
    ports = np.stack([port, port[::-1] * 1.5, port + 0.01 * rng.standard_normal(port.shape)])
    ws = np.stack([z["pca_weights_32x256"], rng.uniform(0.1, 1.0, 32), np.ones(32)])
    ws[1, 5] = 0.0
    batch = run_pca(gpu, ports, ws)
    again = run_pca(gpu, ports, ws)
    for a, b in zip(batch, again):
        assert np.array_equal(a, b)
    for i in range(3):
        single = run_pca(gpu, ports[i], ws[i])
        for a, b in zip(batch, single):
            assert np.array_equal(a[i], b)
    # ... and of how the workspace limit splits the call over portraits
    gpu.set_workspace_limit(2 * 32 * 256 * 8)
    try:
        split = run_pca(gpu, ports, ws)
    finally:
        gpu.set_workspace_limit(32 << 30)
    for a, b in zip(batch, split):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("key", [k for k in CASES if k != "16x64"])  # (16x64: the test below)
def test_pca_project(gpu, fx, key):
    z, zm, meta = fx
    ieig = meta["cases"][key]["ieig"]
    assert ieig
    port, w = z["port_" + key], z["pca_weights_" + key]
    mean, lam, vec, info = run_pca(gpu, port, w, 10)
    basis = vec[ieig]
    proj, rec = gpu.pca_project(port, mean, basis, reconstruct=True)
    proj, rec = proj.cpu().numpy(), rec.cpu().numpy()
    only = gpu.pca_project(port, mean, basis)
    assert only[1] is None and np.array_equal(only[0].cpu().numpy(), proj)
    signs = np.sign(np.sum(basis * z["eigvec10_" + key][ieig], axis=1))
    tol = 1e-12 * np.max(np.abs(port))
    e_proj = np.max(np.abs(proj * signs - z["proj_port_" + key]))
    e_rec = np.max(np.abs(rec - zm["reconst_port_" + key]))
    print(key, "proj err %.3g, reconst err %.3g, tol %.3g" % (e_proj, e_rec, tol))
    assert e_proj <= tol and e_rec <= tol


def test_pca_project_mean_only_case(gpu, fx):
    """16x64 has no significant vector; its projections are checked against
    numpy on the leading vector instead."""
    z = fx[0]
    port, w = z["port_16x64"], z["pca_weights_16x64"]
    mean, lam, vec, info = run_pca(gpu, port, w, 1)
    proj, rec = gpu.pca_project(port, mean, vec, reconstruct=True)
    ref = np.dot(port - mean, vec.T)
    tol = 1e-12 * np.max(np.abs(port))
    assert np.max(np.abs(proj.cpu().numpy() - ref)) <= tol
    assert np.max(np.abs(rec.cpu().numpy() - (np.dot(ref, vec) + mean))) <= tol


def test_pca_errors(gpu):
    import torch
    from pulseportraiture_amd.engine import PPFitError
    lib, ctx, dev = gpu.lib, gpu.ctx, gpu.device
    rng = np.random.default_rng(2)

    def call(nchan, nbin, w, ncomp):
        port = torch.zeros((nchan, nbin), dtype=torch.float64, device=dev)
        wt = torch.as_tensor(np.asarray(w, dtype=np.float64), device=dev)
        nc = max(ncomp, 1)
        mean = torch.empty(nbin, dtype=torch.float64, device=dev)
        lam = torch.empty(nc, dtype=torch.float64, device=dev)
        vec = torch.empty((nc, nbin), dtype=torch.float64, device=dev)
        info = torch.zeros(2, dtype=torch.int32, device=dev)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        rc = lib.ppf_pca_portraits(ctx, 1, nchan, nbin, p(port), p(wt), ncomp, p(mean), p(lam),
                                   p(vec), p(info))
        return rc, lib.ppf_last_error(ctx).decode()

    INVALID, UNSUPPORTED = -1, -3
    bad = [(1, 64, [1.0], 1, INVALID),                      # nchan 1
           (8, 64, np.zeros(8), 2, INVALID),                # all-zero weights
           (8, 64, [1, 1, -1, 1, 1, 1, 1, 1], 2, INVALID),  # a negative weight
           (8, 64, [1, 1, np.nan, 1, 1, 1, 1, 1], 2, INVALID),
           (8, 64, [0, 0, 0, 2, 0, 0, 0, 0], 2, INVALID),   # one positive weight
           (8, 64, np.ones(8), 0, INVALID),                 # ncomp 0
           (8, 64, np.ones(8), 9, INVALID),                 # ncomp > min(nchan, nbin)
           (80, 64, np.ones(80), 65, INVALID),
           (2049, 16, np.ones(2049), 1, UNSUPPORTED),       # nchan 2049
           (8, 15, np.ones(8), 1, UNSUPPORTED)]             # nbin 15
    for nchan, nbin, w, ncomp, code in bad:
        rc, msg = call(nchan, nbin, w, ncomp)
        assert rc == code and msg, (nchan, nbin, ncomp, rc, msg)
    with pytest.raises(PPFitError):
        gpu.pca_portraits(np.zeros((8, 64)), np.ones(8), 0)
    # the context stays usable
    port, w = rng.standard_normal((8, 64)), np.ones(8)
    mean, lam, vec, info = run_pca(gpu, port, w)
    mean_ref, lam_ref, vec_ref = numpy_pca(port, w)
    check_against(lam, vec, lam_ref, vec_ref, [0, 1, 2], "after errors")


def test_pplib_pca_shapes(gpu, fx):
    """pplib.pca returns column vectors, r = min(nchan, nbin) or ncomp of them."""
    from pulseportraiture_amd import pplib
    z = fx[0]
    port, w = z["port_24x128"], z["pca_weights_24x128"]
    lam, vec = pplib.pca(port, None, w, quiet=True)
    assert lam.shape == (24,) and vec.shape == (128, 24)
    lam3, vec3 = pplib.pca(port, np.zeros(128), w, quiet=True, ncomp=3)  # mean_prof is unused
    assert np.array_equal(lam3, lam[:3]) and np.array_equal(vec3, vec[:, :3])
    rec = pplib.reconstruct_portrait(port, z["mean_prof_24x128"], vec3)
    ref = np.dot(np.dot(port - z["mean_prof_24x128"], vec3), vec3.T) + z["mean_prof_24x128"]
    assert np.max(np.abs(rec - ref)) <= 1e-12 * np.max(np.abs(port))
