"""Which template portrait each GetTOAs driver gives a subint, pinned bitwise.

Every case rebuilds the templates through the public API (pplib.read_model /
read_model_device / gen_gaussian_portraits_device / read_spline_model,
archive.load_data for an archive template, Engine.instrumental_response_rows),
feeds them to the same row kernels the driver uses (Engine.phase_shift_batch,
resid_chi2_rows, scatter_rotate_rows) and asserts np.array_equal with what the
driver stored.  What differs between the drivers, each after a line of the
reference:

- get_narrowband_TOAs (pptoas.py:888-926): read_model with the subint's own
  P; the response with P and chan_bw = |f[1] - f[0]| of the ok channels.
- show_fit / get_channels_to_zap (pptoas.py:1356-1388): the unscattered
  Gaussian model whenever the fitted tau != 0, else read_model with
  data.Ps.mean(); the response with the subint's P and chan_bw over all
  channels.

One 3 x 8 x 256 archive serves every case: channel 0 of subint 1 has weight 0,
the channel frequencies are unevenly spaced (|f[1] - f[0]| = 70 MHz over all
channels, 100 MHz over subint 1's ok channels), the three (frequency row, P)
pairs are distinct with two distinct periods.  Fit quality does not matter
here, only the template given whatever was fitted.

A one-channel archive template is not pinned: no driver runs with one (get_TOAs
skips the archive on the nchan mismatch, so nothing is fitted for show_fit or
get_channels_to_zap, and get_narrowband_TOAs indexes the template's one-element
weight row with the data's channel index)."""
import os
import shutil

import numpy as np
import pytest

from tests.conftest import GOLDEN
from tests.golden_consts import DM0
from tests.test_gpu_configs import register_synth_archive

pytestmark = pytest.mark.gpu

NAME = "tsrc.fits"
NSUB, NCHAN, NBIN = 3, 8, 256
IRD = {"DM": 5.0, "wids": [0.004, 0.01], "irf_types": ["rect", "gauss"]}
TAU, ALPHA = 1.0e-4, -3.7  # [s] at the model's reference frequency


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from pulseportraiture_amd.engine import get_engine
    return get_engine(0)


@pytest.fixture(scope="module")
def arc(gpu, tmp_path_factory):
    """The registered archive (as load_data returns it) and the model files."""
    from pulseportraiture_amd import archive, pplib, synth
    w = register_synth_archive(NAME, NSUB, NCHAN, NBIN, 4242, 0.0, 0.0)
    b = dict(archive.load_data(NAME))
    b["weights"] = np.array(b["weights"])
    b["weights"][1, 0] = 0.0
    f = np.array(w.freqs)
    f[0] += 30.0
    b["freqs"] = np.array([f, f * (1 + 1e-5), f])
    b["Ps"] = w.P * np.array([1.0, 1.001, 1.001])
    b["noise_stds"] = gpu.noise_rows(np.asarray(b["subints"])).cpu().numpy()
    for k in ("ok_ichans", "ok_isubs", "masks"):
        b.pop(k)
    archive.register_archive(NAME, b)
    d = archive.load_data(NAME)
    assert len(set(d.Ps.tolist())) == 2 and list(d.ok_ichans[1]) == list(range(1, NCHAN))
    fx = d.freqs[1, d.ok_ichans[1]]
    assert abs(fx[1] - fx[0]) != abs(d.freqs[1, 1] - d.freqs[1, 0])
    tmp = tmp_path_factory.mktemp("tsrc")
    paths = {"gmodel": str(tmp / "plain.gmodel"), "scat": str(tmp / "scat.gmodel"),
             "spline": str(tmp / "m3.spl"), "fits": "tsrc_model.fits"}
    shutil.copy(synth.EXAMPLE_GMODEL, paths["gmodel"])
    name, code, nu_ref, ngauss, params, flags, alpha, fit_alpha = pplib.read_model(
        synth.EXAMPLE_GMODEL, quiet=True)
    assert params[1] == 0.0
    params = np.array(params)
    params[1] = TAU
    pplib.write_model(paths["scat"], name, code, nu_ref, params, flags, ALPHA, fit_alpha,
                      quiet=True)
    z = np.load(os.path.join(GOLDEN, "templates_r3.npz"))
    with open(paths["spline"], "wb") as fh:
        fh.write(bytes(z["spl_m3_file"]))
    archive.register_archive(paths["fits"], dict(subints=w.model[None, None], freqs=w.freqs,
                                                 Ps=[w.P], epochs=[(57300, 0, 0.0)], DM=DM0))
    return d, paths


def _respond(eng, m, freqs, P, chan_bw):
    return eng.instrumental_response_rows(np.asarray(m, dtype=np.float64), freqs, IRD["DM"], P,
                                          IRD["wids"], IRD["irf_types"],
                                          chan_bw=chan_bw).cpu().numpy()


def _fits_template(name):
    from pulseportraiture_amd import archive
    md = archive.load_data(name, dedisperse=False, dededisperse=False, tscrunch=True,
                           pscrunch=True, rm_baseline=True, quiet=True)
    return np.asarray((md.masks * md.subints)[0, 0])


def _model_template(kind, path, freqs, P):
    """read_model(modelfile, phases, freqs, P) / read_spline_model(modelfile,
    freqs, nbin) / the archive template, on the device."""
    from pulseportraiture_amd import pplib
    if kind == "fits":
        return _fits_template(path)
    if kind == "spline":
        return pplib.read_spline_model(path, freqs, NBIN, quiet=True)[1]
    return pplib.read_model_device(path, NBIN, freqs, P, quiet=True)[2]


NARROWBAND = [("gmodel", False), ("scat", False), ("spline", False), ("gmodel", True)]


@pytest.mark.parametrize("kind,irf", NARROWBAND,
                         ids=["gmodel", "gmodel_tau", "spline", "gmodel_irf"])
def test_narrowband_templates(gpu, arc, kind, irf):
    from pulseportraiture_amd import pptoas
    d, paths = arc
    gt = pptoas.GetTOAs([NAME], paths[kind], quiet=True)
    if irf:
        gt.ird = gt.instrumental_response_dict = dict(IRD)
    gt.get_narrowband_TOAs(add_instrumental_response=irf, quiet=True)
    rows, tmpl, noise, where = [], [], [], []
    for isub in d.ok_isubs:
        f, P, okc = d.freqs[isub], d.Ps[isub], d.ok_ichans[isub]
        m = _model_template(kind, paths[kind], f, P)
        if irf:
            m = _respond(gpu, m, f, P, abs(f[okc][1] - f[okc][0]))
        for ichan in okc:
            rows.append(d.subints[isub, 0, ichan])
            tmpl.append(m[ichan])
            noise.append(d.noise_stds[isub, 0, ichan])
            where.append((isub, ichan))
    out = gpu.phase_shift_batch(np.array(rows), np.array(tmpl), noise=np.array(noise), Ns=100,
                                bounds=(-0.5, 0.5),
                                model_idx=np.arange(len(rows), dtype=np.int32)).cpu().numpy()
    exp = {k: np.zeros((NSUB, NCHAN)) for k in
           ("phis", "phi_errs", "scales", "channel_snrs", "channel_red_chi2s")}
    for (isub, ichan), r in zip(where, out):
        exp["phis"][isub, ichan], exp["phi_errs"][isub, ichan] = r[0], r[1]
        exp["scales"][isub, ichan], exp["channel_snrs"][isub, ichan] = r[2], r[4]
        exp["channel_red_chi2s"][isub] = r[5]  # the whole row (pptoas.py:1011)
    assert np.count_nonzero(exp["phi_errs"]) == NSUB * NCHAN - 1
    for k, v in exp.items():
        assert np.array_equal(getattr(gt, k)[0], v), k


# (template, get_TOAs keywords, response on, fitted tau != 0)
FITTED = {"gmodel": ("gmodel", {}, False, False),
          "gmodel_tau_fit_scat": ("scat", dict(fit_scat=True), False, True),
          "gmodel_tau": ("scat", {}, False, False),
          "spline": ("spline", {}, False, False),
          "fits": ("fits", {}, False, False),
          "gmodel_irf": ("gmodel", dict(add_instrumental_response=True), True, False)}


@pytest.mark.parametrize("case", sorted(FITTED))
def test_zap_and_show_fit_templates(gpu, arc, case):
    from pulseportraiture_amd import pplib, pptoas
    from pulseportraiture_amd.pptoaslib import phase_shifts
    d, paths = arc
    kind, kw, irf, scattered = FITTED[case]
    gt = pptoas.GetTOAs([NAME], paths[kind], quiet=True)
    if irf:
        gt.ird = gt.instrumental_response_dict = dict(IRD)
    gt.get_TOAs(quiet=True, **kw)
    gt.get_channels_to_zap()
    port, model_scaled = gt.show_fit(isub=1, show=False, return_fit=True, quiet=True)[:2]
    assert list(gt.ok_isubs[0]) == list(range(NSUB))
    assert np.all((gt.taus[0] != 0.0) == scattered)
    code, nu_ref, gparams = None, None, None
    if scattered:
        code, nu_ref, gparams = [pplib.read_model(paths[kind], quiet=True)[i] for i in (1, 2, 4)]
        gparams = np.copy(gparams)
        gparams[1] = 0.0
    for isub in range(NSUB):
        f, P, okc = d.freqs[isub], d.Ps[isub], d.ok_ichans[isub]
        DM = gt.DMs[0][isub] / gt.doppler_fs[0][isub]  # bary (pptoas.py:1348-1350)
        GM = gt.GMs[0][isub] / gt.doppler_fs[0][isub] ** 3
        nu_DM, nu_GM, nu_tau = gt.nu_refs[0][isub]
        if scattered:  # the fit scatters it: the unscattered model (pptoas.py:1372-1378)
            m = pplib.gen_gaussian_portraits_device(code, gparams, 0.0, NBIN, f, nu_ref)
            tau = gt.taus[0][isub]
            tch = pplib.scattering_times(10 ** tau if gt.log10_tau else tau, gt.alphas[0][isub],
                                         f, nu_tau)
        else:  # read_model with the archive's mean period (pptoas.py:1369-1371)
            m = _model_template(kind, paths[kind], f, d.Ps.mean())
            tch = np.zeros(NCHAN)
        if irf:  # the subint's P, chan_bw over all channels (pptoas.py:1382-1388)
            m = _respond(gpu, m, f, P, abs(f[1] - f[0]))
        m = np.asarray(m, dtype=np.float64)
        phs = phase_shifts(gt.phis[0][isub], DM, GM, f, nu_DM, nu_GM, P)
        rows = d.subints[isub, 0, okc]
        scale = gt.scales[0][isub][okc]
        chi2 = gpu.resid_chi2_rows(rows, phs[okc], m[okc], scale, d.noise_stds[isub, 0, okc],
                                   NBIN - 2, tau=tch[okc],
                                   model_row=np.arange(len(okc), dtype=np.int32)).cpu().numpy()
        assert np.array_equal(gt.channel_red_chi2s[0][isub], chi2), (case, isub)
        if isub == 1:
            exp_port, exp_model = np.zeros((NCHAN, NBIN)), np.zeros((NCHAN, NBIN))
            exp_port[okc] = gpu.scatter_rotate_rows(rows, phs[okc] + 0.0).cpu().numpy()
            exp_port *= np.asarray(d.masks[isub, 0])
            exp_model[okc] = scale[:, None] * gpu.scatter_rotate_rows(
                m[okc], np.zeros(len(okc)), tch[okc]).cpu().numpy()
            assert np.array_equal(port, exp_port), case
            assert np.array_equal(model_scaled, exp_model), case
            assert np.any(exp_model[okc] != 0.0) and not np.any(exp_model[0])
