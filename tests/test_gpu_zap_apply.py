"""Zapping end to end without PSRCHIVE: get_TOAs -> get_channels_to_zap ->
ppzap.apply_zap_channels -> get_TOAs on the .zap file.

A 2 x 8 x 256 fake pulsar has one channel's noise raised tenfold, so its S/N
(7.5 where the others have 55 to 170) falls under get_channels_to_zap's cut at
SNR_threshold = 40 (40 / sqrt(8) = 14 per channel).  The reduced-chi2 cut is
set to 2: at 256 bins the good channels of this model reach 1.26 to 1.31 with
no channel raised at all, on either side of the default 1.3.  The raise is
kept moderate on purpose: a channel a thousand times noisier moves the
off-pulse window remove_baseline finds on the summed profile.  After apply_zap_channels the
.zap file must fit exactly as the original file's own values do with that
weight set to 0 by hand (a registered bunch): TOAs, DMs and their errors
bitwise, and the flagged channel absent from ok_ichans."""
import os
import shutil

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAR = ("PSR J1234+5678\nRAJ 12:34:00.0\nDECJ +56:07:08.9\nF0 345.67890123456789\n"
       "PEPOCH 57000.0\nDM 34.56789\n")
BAD = 5


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from pulseportraiture_amd.engine import get_engine
    return get_engine(0)


def toas_of(datafile, model):
    from pulseportraiture_amd import pptoas
    gt = pptoas.GetTOAs([datafile], model, quiet=True)
    gt.get_TOAs(quiet=True)
    return gt


def test_zap_apply_and_refit(eng, tmp_path):
    from pulseportraiture_amd import archive, pplib, ppzap, psrfits, synth
    par = tmp_path / "fake.par"
    par.write_text(PAR)
    nsub, nchan, nbin = 2, 8, 256
    name = str(tmp_path / "noisy.fits")
    model = str(tmp_path / "example.gmodel")
    shutil.copy(synth.EXAMPLE_GMODEL, model)
    # S/N of about a hundred per channel, a tenth of it in channel BAD
    freqs = np.linspace(1100.0 + 50.0, 1900.0 - 50.0, nchan)
    _, _, port = pplib.read_model_device(model, nbin, freqs, 1.0 / 345.67890123456789, quiet=True)
    port = port.cpu().numpy() if hasattr(port, "cpu") else np.asarray(port)
    sigma = np.full(nchan, np.sqrt((port ** 2).sum(axis=1)).mean() / 100.0)
    sigma[BAD] *= 10.0
    pplib.make_fake_pulsar(model, str(par), outfile=name, nsub=nsub, nchan=nchan, nbin=nbin,
                           noise_stds=sigma, dDM=1e-3, phase=0.02, dedispersed=False, tsub=60.0,
                           seed=5, quiet=True)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        gt = toas_of(name, "example.gmodel")
        gt.get_channels_to_zap(SNR_threshold=40.0, rchi2_threshold=2.0)
        zap = gt.zap_channels
        print("zap_channels", zap)
        assert [[list(map(int, z)) for z in arch] for arch in zap] == [[[BAD], [BAD]]]

        before = open(name, "rb").read()
        out = ppzap.apply_zap_channels([name], zap, quiet=True)
        assert out == [str(tmp_path / "noisy.zap")]
        assert open(name, "rb").read() == before
        f = psrfits.PSRFITSFile(out[0])
        w = f.meta()["weights"]
        f.close()
        want = np.ones((nsub, nchan))
        want[:, BAD] = 0.0
        np.testing.assert_array_equal(w, want)

        # the original file's values with that weight set to 0 by hand, in the
        # state the file is stored in (baseline not yet removed, noise and
        # S/N still to be estimated): what get_TOAs opens the .zap file as
        b = archive.load_data(name, pscrunch=True, rm_baseline=False, get_SNRs=False, host=False,
                              quiet=True)
        for key in ("ok_isubs", "ok_ichans", "masks"):
            b.pop(key, None)
        b.weights = np.array(b.weights, dtype=np.float64)
        b.weights[:, BAD] = 0.0
        b.noise_stds = None
        b.SNRs = np.ones((nsub, 1, nchan))
        b.snr_deferred = True
        b.baseline_removed = False
        archive.register_archive("byhand", b)
        try:
            hand = toas_of("byhand", "example.gmodel")
        finally:
            archive.unregister_archive("byhand")
        zapped = toas_of(out[0], "example.gmodel")
    finally:
        os.chdir(cwd)

    assert len(zapped.TOA_list) == len(hand.TOA_list) == nsub
    for attr in ("TOA_errs", "DMs", "DM_errs", "phis", "phi_errs"):
        np.testing.assert_array_equal(np.asarray(getattr(zapped, attr)[0], dtype=np.float64),
                                      np.asarray(getattr(hand, attr)[0], dtype=np.float64),
                                      err_msg=attr)
    for a, c in zip(zapped.TOA_list, hand.TOA_list):
        assert (a.MJD.days, a.MJD.secs, a.MJD.fracsec) == (c.MJD.days, c.MJD.secs, c.MJD.fracsec)
        assert a.TOA_error == c.TOA_error and a.DM == c.DM and a.DM_error == c.DM_error
    # the flagged channel is gone from the fit
    data = archive.load_data(out[0], pscrunch=True, quiet=True)
    assert all(BAD not in list(c) for c in data.ok_ichans)
    assert all(len(c) == nchan - 1 for c in data.ok_ichans)
    # ... and the fit differs from the one that had it
    assert not np.array_equal(np.asarray(gt.DMs[0]), np.asarray(zapped.DMs[0]))
