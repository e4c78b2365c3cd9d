"""ppspline above 2,048 channels against the reference
(tests/golden/make_golden_ppspline_wide.py: its make_spline_model on a 2,112 x
128 portrait, which make_input regenerates here): the model by check_model's
bounds of tests/test_gpu_ppspline.py -- ieig, ncomp, ier and k equal, knots to
1e-12, the model at the stored channels to 1e-11 of max|model| -- and the
align -> ppspline -> TOAs pipeline end: GetTOAs with the model built and
written here against GetTOAs with the reference's spline, phases and DMs to
1e-3 sigma, identical statuses.
"""
import pickle

import numpy as np
import pytest

from tests.test_gpu_ppspline import dict_archive
from tests.test_ppspline_wide_golden_cpu import fixture, wide_input

pytestmark = pytest.mark.gpu

KEY = "2112x128"


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from pulseportraiture_amd.engine import get_engine
    return get_engine(0)


@pytest.fixture(scope="module")
def model(gpu):
    """The fixture, and the DataPortrait with its spline model made here."""
    from pulseportraiture_amd import ppspline
    z, m = fixture()
    assert "%dx%d" % (m["nchan"], m["nbin"]) == KEY
    freqs, port = wide_input()
    arch = {"freqs_" + KEY: freqs, "port_" + KEY: port, "SNRs_" + KEY: z["SNRs"],
            "noise_stds_" + KEY: z["noise_stds"]}
    dp = ppspline.DataPortrait(dict_archive(arch, KEY), quiet=True)
    dp.make_spline_model(quiet=True)
    return z, m, dp


def test_make_spline_model_wide_matches_reference(model):
    z, m, dp = model
    assert dp.datafile == m["datafile"] and dp.model_name == m["model_name"]
    print(KEY, "PCA sweeps %d, converged %d" % tuple(dp.pca_info))
    assert dp.pca_info[1] == 1
    lam0 = z["eigval"][0]
    print(KEY, "max |dlambda| / lambda_0 = %.3g"
          % (np.max(np.abs(dp.eigval[:10] - z["eigval"][:10])) / lam0))
    assert list(dp.ieig) == m["ieig"] and dp.ncomp == m["ncomp"], dp.ieig
    assert dp.ier == m["ier"], (dp.ier, dp.msg)
    t = np.asarray(dp.tck[0])
    assert t.shape == z["t"].shape and dp.tck[2] == m["k"]
    assert np.max(np.abs(t - z["t"])) <= 1e-12 * np.max(np.abs(z["t"]))
    ref = z["modelx_sub"]
    scale = np.max(np.abs(ref))
    step = m["chan_step"]
    ex = np.max(np.abs(dp.modelx[::step] - ref)) / scale
    em = np.max(np.abs(dp.model[::step] - ref)) / scale
    print(KEY, "modelx err %.3g, model err %.3g (of max|model|)" % (ex, em))
    assert dp.modelx.shape == dp.model.shape == (m["nchan"], m["nbin"])
    assert ex <= 1e-11 and em <= 1e-11, (ex, em)
    assert np.array_equal(dp.model_masked, dp.model * dp.masks[0, 0])
    assert dp.eigvec.shape == (m["nbin"], m["nbin"])
    assert dp.proj_port.shape == (m["nchan"], m["ncomp"])
    signs = np.sign(np.sum(dp.eigvec[:, dp.ieig] * z["basis"], axis=0))
    assert np.max(np.abs(dp.proj_port * signs - z["proj_port"])) <= 1e-12 * np.max(np.abs(dp.portx))


def test_pipeline_toas_wide(model, tmp_path):
    """write_model -> read_spline_model -> GetTOAs on two subints of the
    fixture's shape, with the model built here and with the reference's
    spline rebuilt from its stored knots, coefficients, mean profile and
    eigenvectors."""
    from pulseportraiture_amd import archive, pplib, pptoas, synth
    from pulseportraiture_amd.mjd import MJD
    z, m, dp = model
    nchan, nbin, nsub = m["nchan"], m["nbin"], 2
    ours, theirs = str(tmp_path / "ours.spl"), str(tmp_path / "reference.spl")
    dp.write_model(ours, quiet=True)
    with open(theirs, "wb") as f:  # the reference's model file (ppspline.py:206-230)
        pickle.dump([m["model_name"], m["source"], m["datafile"], z["mean_prof"], z["basis"],
                     [z["t"], list(z["c"]), m["k"]]], f, protocol=2)
    _, port = pplib.read_spline_model(ours, dp.freqs[0], nbin, quiet=True)
    assert np.max(np.abs(port - dp.model)) <= 1e-13 * np.max(np.abs(dp.model))
    _, ref_port = pplib.read_spline_model(theirs, dp.freqs[0], nbin, quiet=True)
    d_model = np.max(np.abs(port - ref_port)) / np.max(np.abs(ref_port))
    print("model portraits of the two files: %.3g of max|model|, %d cells differ"
          % (d_model, np.count_nonzero(port != ref_port)))
    assert d_model <= 1e-11
    w = synth.make_workload(nsub, nchan, nbin, seed=3, sigma=0.05)
    assert np.array_equal(w.freqs, dp.freqs[0])
    b = dict(subints=synth.workload_data_host(w)[:, None], freqs=np.tile(w.freqs, (nsub, 1)),
             weights=np.ones((nsub, nchan)), SNRs=np.ones((nsub, 1, nchan)), Ps=np.full(nsub, w.P),
             epochs=[MJD(57300.0 + 0.001 * i) for i in range(nsub)], DM=w.DM0, bw=800.0,
             nu0=1500.0, telescope="GBT", telescope_code="1", subtimes=[30.0] * nsub)
    archive.register_archive("ppspline_wide_pipeline.fits", b)
    res = []
    try:
        for mf in (ours, theirs):
            gt = pptoas.GetTOAs(["ppspline_wide_pipeline.fits"], mf, quiet=True)
            gt.get_TOAs(quiet=True)
            res.append(gt)
    finally:
        archive.unregister_archive("ppspline_wide_pipeline.fits")
    a, r = res
    assert np.array_equal(a.rcs[0], r.rcs[0])
    for par, err in [("phis", "phi_errs"), ("DMs", "DM_errs")]:
        e = r.__dict__[err][0]
        d = np.abs(a.__dict__[par][0] - r.__dict__[par][0])
        print(par, "max |diff| / sigma = %.3g" % np.max(d / e))
        assert np.all(e > 0) and np.all(d <= 1e-3 * e), par
