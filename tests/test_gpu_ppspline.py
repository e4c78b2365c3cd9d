"""ppspline.DataPortrait.make_spline_model / write_model against the reference's
(tests/golden/make_golden_ppspline.py: its make_spline_model with smooth=False,
try_nlevels=0 on the same portraits), and the align -> ppspline -> TOAs
pipeline end: GetTOAs with a model written here against GetTOAs with the
reference's model file.
"""
import json
import os
import pickle
import pickletools

import numpy as np
import pytest

from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu


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
            np.load(os.path.join(GOLDEN, "ppspline_variants.npz")),
            json.load(open(os.path.join(GOLDEN, "ppspline.json"))))


CASES = ["32x256", "20x250", "24x128", "16x64", "48x512"]
VARIANTS = [v + "_" + c for c in ("32x256", "20x250")
            for v in ("ncomp2_k5_s0", "nbreak3", "zap_negbw")]


def dict_archive(z, key, zap=(), negbw=False, name=None):
    """The fixture input as load_data's dict archive (the stub of
    make_golden_ppspline.make_stub)."""
    from pulseportraiture_amd.mjd import MJD
    freqs, port = z["freqs_" + key], z["port_" + key]
    snrs, noise = z["SNRs_" + key], z["noise_stds_" + key]
    bw = 800.0
    if negbw:
        freqs, port, snrs, noise, bw = freqs[::-1], port[::-1], snrs[::-1], noise[::-1], -bw
    weights = np.ones(len(freqs))
    weights[list(zap)] = 0.0
    return dict(subints=port[None, None].copy(), freqs=freqs[None].copy(), weights=weights[None],
                SNRs=snrs[None, None].copy(), noise_stds=noise[None, None].copy(), Ps=[0.003],
                epochs=[MJD(57300.0)], bw=bw, source="J0000+0000",
                filename=name or "ppspline_%s.fits" % key)


def check_model(dp, m, t_ref, modelx_ref, model_ref, tag):
    assert list(dp.ieig) == m["ieig"] and dp.ncomp == m["ncomp"], (tag, dp.ieig)
    assert dp.ier == m["ier"], (tag, dp.ier, dp.msg)
    t = np.asarray(dp.tck[0])
    assert t.shape == t_ref.shape and dp.tck[2] == m["k"]
    assert np.max(np.abs(t - t_ref)) <= 1e-12 * np.max(np.abs(t_ref)), tag
    scale = np.max(np.abs(model_ref))
    ex = np.max(np.abs(dp.modelx - modelx_ref)) / scale
    em = np.max(np.abs(dp.model - model_ref)) / scale
    print(tag, "modelx err %.3g, model err %.3g (of max|model|)" % (ex, em))
    assert dp.modelx.shape == modelx_ref.shape and dp.model.shape == model_ref.shape
    assert ex <= 1e-11 and em <= 1e-11, (tag, ex, em)
    assert np.array_equal(dp.model_masked, dp.model * dp.masks[0, 0])


@pytest.mark.parametrize("key", CASES)
def test_make_spline_model_matches_reference(gpu, fx, key):
    from pulseportraiture_amd import ppspline
    z, zm, _, meta = fx
    m = meta["cases"][key]
    dp = ppspline.DataPortrait(dict_archive(z, key), quiet=True)
    assert dp.datafile == m["datafile"] and dp.source == m["source"]
    dp.make_spline_model(quiet=True)
    assert dp.model_name == m["model_name"]
    if m["ncomp"] == 0:  # the mean-only model: the tiled weighted mean, an empty tck
        assert dp.ncomp == 0 and len(dp.ieig) == 0
        assert len(dp.tck[0]) == 0 and len(dp.tck[1]) == 0 and dp.tck[2] == 0
        assert dp.fp is None and dp.ier is None and dp.msg is None
        assert dp.proj_port.shape == (m["nchan"], 0)
        w = dp.SNRsxs / dp.SNRsxs.sum()
        mean = (dp.portx.T * w).T.sum(axis=0) / w.sum()
        assert np.max(np.abs(dp.mean_prof - mean)) <= 1e-15 * np.max(np.abs(mean)) * m["nchan"]
        assert np.array_equal(dp.model, np.tile(dp.mean_prof, (m["nchan"], 1)))
        assert np.array_equal(dp.modelx, dp.model) and np.array_equal(dp.reconst_port, dp.model)
        scale = np.max(np.abs(zm["modelx_" + key]))
        assert np.max(np.abs(dp.model - zm["modelx_" + key])) <= 1e-11 * scale
        return
    check_model(dp, m, z["t_" + key], zm["modelx_" + key], zm["modelx_" + key], key)
    scale = np.max(np.abs(dp.portx))
    assert np.max(np.abs(dp.reconst_port - zm["reconst_port_" + key])) <= 1e-12 * scale
    assert dp.eigvec.shape == (m["nbin"], min(m["nchan"], m["nbin"]))
    assert dp.proj_port.shape == (m["nchan"], m["ncomp"]) and len(dp.u) == m["nchan"]


@pytest.mark.parametrize("vkey", VARIANTS)
def test_make_spline_model_variants(gpu, fx, vkey):
    from pulseportraiture_amd import ppspline
    z, _, zv, meta = fx
    m = meta["variants"][vkey]
    dp = ppspline.DataPortrait(dict_archive(z, m["case"], m["zap"], m["negbw"]), quiet=True)
    assert len(dp.portx) == len(dp.port) - len(m["zap"])
    dp.make_spline_model(quiet=True, **m["kwargs"])
    modelx = zv["modelx_" + vkey]
    model = zv["model_" + vkey] if m["zap"] else modelx
    check_model(dp, m, zv["t_" + vkey], modelx, model, vkey)


def test_refusals(gpu, fx, tmp_path):
    from pulseportraiture_amd import ppspline, pplib
    z = fx[0]
    dp = ppspline.DataPortrait(dict_archive(z, "16x64"), quiet=True)
    with pytest.raises(NotImplementedError, match="PyWavelets"):
        dp.make_spline_model(smooth=True, quiet=True)
    with pytest.raises(NotImplementedError, match="PyWavelets"):
        pplib.find_significant_eigvec(np.eye(64)[:, :4], return_smooth=True)
    with pytest.raises(NotImplementedError, match="PyWavelets"):
        pplib.find_significant_eigvec(np.eye(64)[:, :4], try_nlevels=3)
    meta = tmp_path / "portraits.meta"
    meta.write_text("a.fits\nb.fits\n")
    with pytest.raises(NotImplementedError, match="metafile"):
        ppspline.DataPortrait(str(meta), quiet=True)
    with pytest.raises(NotImplementedError, match="joinfile"):
        ppspline.DataPortrait(dict_archive(z, "16x64"), quiet=True, joinfile="x.join")


@pytest.mark.parametrize("key", ["48x512", "16x64"])
def test_model_file_round_trip(gpu, fx, key, tmp_path):
    from pulseportraiture_amd import ppspline, pplib
    z = fx[0]
    dp = ppspline.DataPortrait(dict_archive(z, key), quiet=True)
    dp.make_spline_model(quiet=True)
    path = str(tmp_path / "model.spl")
    dp.write_model(path, quiet=True)
    name, source, datafile, mean_prof, eigvec, tck = pplib.load_spline_model_file(path)
    assert (name, source, datafile) == (dp.model_name, dp.source, dp.datafile)
    assert np.array_equal(mean_prof, dp.mean_prof)
    assert eigvec.shape == (dp.nbin, dp.ncomp) and np.array_equal(eigvec, dp.eigvec[:, dp.ieig])
    assert np.array_equal(tck[0], dp.tck[0]) and tck[2] == dp.tck[2]
    assert len(tck[1]) == len(dp.tck[1])
    for a, b in zip(tck[1], dp.tck[1]):
        assert np.array_equal(a, b)
    blob = open(path, "rb").read()
    assert blob[:2] == b"\x80\x02"  # protocol 2
    assert max(op.proto for op, _, _ in pickletools.genops(blob)) <= 2
    assert b"numpy._core" not in blob  # a module a Python-2 numpy does not have
    plain = pickle.loads(blob, encoding="latin1")
    assert plain[0] == dp.model_name and np.array_equal(plain[3], dp.mean_prof)
    # the model read back builds the model portrait
    _, port = pplib.read_spline_model(path, dp.freqs[0], dp.nbin, quiet=True)
    assert np.max(np.abs(port - dp.model)) <= 1e-13 * np.max(np.abs(dp.model))


def test_pipeline_toas_match_reference_model(gpu, fx, tmp_path):
    """GetTOAs on a 4-subint archive of the 48x512 truth (injected phi and
    DM offsets) with the model built and written here, against GetTOAs with
    the reference's model file: phi and DM within 1e-3 sigma, same statuses."""
    from pulseportraiture_amd import archive, ppspline, pptoas, synth
    from pulseportraiture_amd.mjd import MJD
    z = fx[0]
    key, nsub = "48x512", 4
    dp = ppspline.DataPortrait(dict_archive(z, key), quiet=True)
    dp.make_spline_model(quiet=True)
    ours, theirs = str(tmp_path / "ours.spl"), str(tmp_path / "reference.spl")
    dp.write_model(ours, quiet=True)
    with open(theirs, "wb") as f:
        f.write(bytes(z["model_file_" + key]))
    w = synth.make_workload(nsub, 48, 512, seed=3, sigma=0.05)
    assert np.array_equal(w.freqs, z["freqs_" + key])
    b = dict(subints=synth.workload_data_host(w)[:, None], freqs=np.tile(w.freqs, (nsub, 1)),
             weights=np.ones((nsub, 48)), SNRs=np.ones((nsub, 1, 48)), Ps=np.full(nsub, w.P),
             epochs=[MJD(57300.0 + 0.001 * i) for i in range(nsub)], DM=w.DM0, bw=800.0,
             nu0=1500.0, telescope="GBT", telescope_code="1", subtimes=[30.0] * nsub)
    archive.register_archive("ppspline_pipeline.fits", b)
    res = []
    try:
        for model in (ours, theirs):
            gt = pptoas.GetTOAs(["ppspline_pipeline.fits"], model, quiet=True)
            gt.get_TOAs(quiet=True)
            res.append(gt)
    finally:
        archive.unregister_archive("ppspline_pipeline.fits")
    a, r = res
    assert np.array_equal(a.rcs[0], r.rcs[0])
    for par, err in [("phis", "phi_errs"), ("DMs", "DM_errs")]:
        e = r.__dict__[err][0]
        d = np.abs(a.__dict__[par][0] - r.__dict__[par][0])
        print(par, "max |diff| / sigma = %.3g" % np.max(d / e))
        assert np.all(e > 0) and np.all(d <= 1e-3 * e), par
    print("DM - injected [sigma]:", (a.DMs[0] - (w.DM0 + w.dDM)) / a.DM_errs[0])


def test_batch_helper_equals_single_calls(gpu, fx):
    from pulseportraiture_amd import ppspline
    z = fx[0]
    rng = np.random.default_rng(9)
    arch = [dict_archive(z, "24x128", name="a.fits"), dict_archive(z, "24x128", name="b.fits")]
    arch[1]["subints"] = arch[1]["subints"] * (1.0 + 0.3 * rng.uniform(size=(1, 1, 24, 1)))
    arch[1]["SNRs"] = arch[1]["SNRs"] * rng.uniform(0.5, 1.5, size=(1, 1, 24))
    batch = [ppspline.DataPortrait(a, quiet=True) for a in arch]
    out = ppspline.make_spline_models(batch, max_ncomp=3, model_names=["A", None], quiet=True)
    assert out[0] is batch[0] and batch[0].model_name == "A" and batch[1].model_name == "b.fits.spl"
    for a, dpb in zip(arch, batch):
        dps = ppspline.DataPortrait(a, quiet=True)
        dps.make_spline_model(max_ncomp=3, quiet=True)
        assert dpb.ncomp > 0 and list(dps.ieig) == list(dpb.ieig)
        for name in ("eigval", "eigvec", "mean_prof", "proj_port", "reconst_port", "model",
                     "modelx", "model_masked", "u"):
            assert np.array_equal(getattr(dps, name), getattr(dpb, name)), name
        assert np.array_equal(dps.tck[0], dpb.tck[0]) and dps.fp == dpb.fp and dps.ier == dpb.ier
        for c1, c2 in zip(dps.tck[1], dpb.tck[1]):
            assert np.array_equal(c1, c2)
    with pytest.raises(ValueError):
        ppspline.make_spline_models([batch[0], ppspline.DataPortrait(dict_archive(z, "16x64"),
                                                                     quiet=True)], quiet=True)


def test_normalize_round_trip(gpu, fx):
    from pulseportraiture_amd import ppspline
    z = fx[0]
    dp = ppspline.DataPortrait(dict_archive(z, "32x256", zap=(3, 11)), quiet=True)
    port, portx, noise = dp.port.copy(), dp.portx.copy(), dp.noise_stdsxs.copy()
    dp.normalize_portrait("prof")
    assert np.all(dp.norm_values[[3, 11]] == 1.0) and not np.any(dp.port[[3, 11]])
    ok = dp.ok_ichans[0]
    assert np.max(np.abs(dp.norm_values[ok] - 1.0)) > 1e-3  # it did something
    assert np.allclose(dp.portx, portx / dp.norm_values[ok][:, None], rtol=1e-6, atol=0)
    dp.unnormalize_portrait()
    assert np.max(np.abs(dp.port - port)) <= 1e-13 * np.max(np.abs(port))
    assert np.max(np.abs(dp.portx - portx)) <= 1e-13 * np.max(np.abs(portx))
    assert np.array_equal(dp.noise_stdsxs, noise) and np.all(dp.norm_values == 1.0)
    assert not hasattr(dp, "unnorm_noise_stds")
