"""The wide ppspline fixture (tests/golden/make_golden_ppspline_wide.py: the
reference's make_spline_model on a 2,112-channel portrait) does not hold its
input portrait: make_input regenerates it from its seeds.  This pins that the
regenerated input is the one the reference saw -- its numpy_pca (np.cov +
eigh, what the reference's pca runs) reproduces the stored eigenvalues to
1e-12 lambda_0 and the stored mean profile to nchan eps max|port|.
"""
import functools
import importlib.util
import json
import os

import numpy as np

from tests.conftest import GOLDEN
from tests.test_gpu_pca import EPS, numpy_pca


def fixture():
    return (np.load(os.path.join(GOLDEN, "ppspline_wide.npz")),
            json.load(open(os.path.join(GOLDEN, "ppspline_wide.json"))))


@functools.lru_cache(maxsize=None)
def wide_input():
    """(freqs, port) of the fixture's case, from make_golden_ppspline.make_input."""
    spec = importlib.util.spec_from_file_location(
        "make_golden_ppspline", os.path.join(GOLDEN, "make_golden_ppspline.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    m = fixture()[1]
    return mod.make_input(m["nchan"], m["nbin"], m["sigma"])


def test_fixture_case():
    z, m = fixture()
    assert (m["nchan"], m["nbin"]) == (2112, 128) and m["ncomp"] >= 1
    # the first candidate with a significant eigenvector was kept
    assert [t["ncomp"] for t in m["tried"]] == [0, 1]
    assert z["basis"].shape == (m["nbin"], m["ncomp"]) and z["c"].shape[0] == m["ncomp"]
    assert z["modelx_sub"].shape == (len(range(0, m["nchan"], m["chan_step"])), m["nbin"])
    size = sum(os.path.getsize(os.path.join(GOLDEN, "ppspline_wide" + e)) for e in (".npz", ".json"))
    assert size < 1000000


def test_input_regenerates():
    z, m = fixture()
    freqs, port = wide_input()
    assert port.shape == (m["nchan"], m["nbin"]) and freqs.shape == (m["nchan"],)
    mean, lam, vec = numpy_pca(port, z["pca_weights"])
    e_lam = np.max(np.abs(lam - z["eigval"])) / z["eigval"][0]
    e_mean = np.max(np.abs(mean - z["mean_prof"]))
    print("eigenvalues: %.3g lambda_0; mean: %.3g (bound %.3g)"
          % (e_lam, e_mean, m["nchan"] * EPS * np.max(np.abs(port))))
    assert e_lam <= 1e-12
    assert e_mean <= m["nchan"] * EPS * np.max(np.abs(port))
