"""Archive writing on the device: ppf_pack_subints against its numpy
restatement, ppf_fake_subints against ppf_synth_portraits, its own packing
and the host Philox twin, then make_fake_pulsar, write_archive /
unload_new_archive and ppalign's .fits output read back by load_data.
Nothing is pinned against PSRCHIVE (absent); the yardsticks are the package's
reader, synth.quantize_host / fake_subints_host and the host numpy formulas.

The quantisation bound used after a rotation: a stored profile differs from
its value by e with |e_j| <= scl / 2; dedispersing it is a unitary map of the
row (a phase per harmonic), so the loaded row differs from the true one by a
vector of at most that 2-norm: rms <= scl / 2 and max <= sqrt(nbin) scl / 2.
(At most: each rotation of an even-length row keeps only the real part of its
Nyquist harmonic -- numpy's irfft and the device kernels alike -- so that one
harmonic shrinks.  For the same reason the expected value of a profile that
was stored dispersed and loaded dedispersed is the profile put through those
two rotations in host numpy, not the profile rotated once: the two differ in
the Nyquist harmonic alone, which the example model's narrow high-frequency
profiles do not lack at 256 bins.)"""
import os
import shutil

import numpy as np
import pytest

from tests.test_psrfits_write_cpu import edge_rows

pytestmark = pytest.mark.gpu

PAR = ("PSR J1234+5678\nRAJ 12:34:00.0\nDECJ +56:07:08.9\nF0 345.67890123456789\n"
       "PEPOCH 57000.0\nDM 34.56789\n")
P0 = 1.0 / 345.67890123456789
DM0 = 34.56789
SHAPES = [(nbin, npol, nchan) for nbin in (64, 2048, 100) for npol, nchan in ((1, 3), (4, 5))]


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from pulseportraiture_amd.engine import get_engine
    return get_engine(0)


@pytest.fixture()
def par(tmp_path):
    p = tmp_path / "fake.par"
    p.write_text(PAR)
    return str(p)


def host(ts):
    return [t.cpu().numpy() for t in ts]


@pytest.mark.parametrize("nbin,npol,nchan", SHAPES)
def test_pack_matches_numpy(gpu, nbin, npol, nchan):
    """raw, scl and offs sample for sample, on the rows a quantiser can get
    wrong and on ordinary ones."""
    from pulseportraiture_amd.synth import quantize_host
    nsub = 3
    edge = edge_rows(nbin)
    rng = np.random.default_rng(nbin + nchan)
    data = rng.normal(size=(nsub * npol * nchan, nbin)) * 10.0 ** rng.integers(-3, 4, (nsub * npol * nchan, 1))
    n = min(len(edge), len(data))
    data[:n] = edge[:n]
    data = data.reshape(nsub, npol, nchan, nbin)
    raw, scl, offs = host(gpu.pack_subints(data))
    raw_h, scl_h, offs_h = quantize_host(data)
    np.testing.assert_array_equal(scl, scl_h)
    np.testing.assert_array_equal(offs, offs_h)
    np.testing.assert_array_equal(raw, raw_h)
    # and back through the unpack kernel: within half a step
    import torch
    back = gpu.unpack_subints(torch.as_tensor(raw, device=gpu.device),
                              torch.as_tensor(scl, device=gpu.device),
                              torch.as_tensor(offs, device=gpu.device)).cpu().numpy()
    eps = np.finfo(np.float64).eps
    assert (np.abs(back - data) <= 0.5 * scl[..., None] * (1 + 1e-9) + 4 * eps * np.abs(data)).all()


def test_pack_every_edge_row_and_nonfinite(gpu):
    """All edge rows at each nbin (one subint of them), and a non-finite
    sample: an error status, no fault, the other rows still packed."""
    from pulseportraiture_amd.engine import PPFitError
    from pulseportraiture_amd.synth import quantize_host
    for nbin in (16, 64, 100, 2048):
        data = edge_rows(nbin)[None, None]
        for got, want in zip(host(gpu.pack_subints(data)), quantize_host(data)):
            np.testing.assert_array_equal(got, want)
    bad = edge_rows(64)[None, None].copy()
    bad[0, 0, 5, 63] = np.nan
    with pytest.raises(PPFitError, match="non-finite"):
        gpu.pack_subints(bad)
    bad[0, 0, 5, 63] = np.inf
    with pytest.raises(PPFitError, match="non-finite"):
        gpu.pack_subints(bad)


@pytest.mark.parametrize("nbin,npol,nchan", SHAPES)
def test_fake_subints(gpu, nbin, npol, nchan):
    import torch
    from pulseportraiture_amd import synth
    nsub, seed, sub0 = 3, 12345, 7
    rng = np.random.default_rng(nbin * npol)
    model = rng.normal(0, 1, (nchan, nbin))
    ph = rng.uniform(-2, 2, (nsub, nchan))
    # the reducible case is bitwise ppf_synth_portraits
    one = gpu.fake_subints(model, ph, 1.0, 1.5, seed, sub0=sub0)
    assert torch.equal(one[:, 0], gpu.synth(model, ph, 1.5, seed, sub0=sub0))
    quiet = gpu.fake_subints(model, ph, 1.0, 0.0, seed, sub0=sub0)
    assert torch.equal(quiet[:, 0], gpu.synth(model, ph, 0.0, seed, sub0=sub0))
    # amplitudes, per-channel noise, polarisations: the host twin, at the
    # tolerance of test_synth_matches_numpy (amp and sigma of order 1)
    amp = rng.uniform(0.5, 1.5, (nsub, nchan))
    sigma = rng.uniform(0.5, 1.5, nchan)
    sigma[1] = 0.0
    full = gpu.fake_subints(model, ph, amp, sigma, seed, sub0=sub0, npol=npol)
    ref = synth.fake_subints_host(model, ph, amp, sigma, seed, sub0=sub0, npol=npol)
    np.testing.assert_allclose(full.cpu().numpy(), ref, atol=1e-11)
    if npol > 1:  # each polarisation has its own noise
        assert not torch.equal(full[:, 0], full[:, 1])
    # one call equals two with sub0
    parts = [gpu.fake_subints(model, ph[lo:hi], amp[lo:hi], sigma, seed, sub0=sub0 + lo, npol=npol)
             for lo, hi in ((0, 1), (1, nsub))]
    assert torch.equal(full, torch.cat(parts))
    # the packed output is bitwise the packed fp64 output (fused kernel for
    # nbin 64 and 2048, generator + pack for 100), also in two calls
    packed = gpu.fake_subints(model, ph, amp, sigma, seed, sub0=sub0, npol=npol, packed=True)
    for got, want in zip(packed, gpu.pack_subints(full)):
        assert torch.equal(got, want)
    pparts = [gpu.fake_subints(model, ph[lo:hi], amp[lo:hi], sigma, seed, sub0=sub0 + lo,
                               npol=npol, packed=True) for lo, hi in ((0, 1), (1, nsub))]
    for i, want in enumerate(packed):
        assert torch.equal(torch.cat([p[i] for p in pparts]), want)


def test_fake_subints_nonfinite_and_arguments(gpu):
    from pulseportraiture_amd.engine import PPFitError
    model = np.ones((3, 64))
    ph = np.zeros((2, 3))
    amp = np.ones((2, 3))
    amp[1, 2] = np.inf
    with pytest.raises(PPFitError, match="non-finite"):
        gpu.fake_subints(model, ph, amp, 1.0, 1, packed=True)
    with pytest.raises(PPFitError):
        gpu.fake_subints(np.ones((3, 8)), ph, 1.0, 1.0, 1)  # nbin below 16


def rotate(x, ph):
    """irfft(rfft(x) e^{2 pi i k ph}) per row in host numpy (rotate_data's convention)."""
    nbin = x.shape[-1]
    k = np.arange(nbin // 2 + 1)
    return np.fft.irfft(np.fft.rfft(x, axis=-1) * np.exp(2j * np.pi * np.asarray(ph)[..., None] * k),
                        nbin, axis=-1)


def dispersion(freqs, DM, nu0):
    """archive.dedispersion_phases for one period: the rotation [rot] that dedisperses."""
    from pulseportraiture_amd import pplib
    return pplib.Dconst * DM * (freqs ** -2.0 - nu0 ** -2.0) / P0


def noise_free(nsub, nchan, nbin, phase, dDM, nu0=1500.0, bw=800.0, stored_DM=None):
    """rotate_data(model, -phase, -dDM, P, freqs, nu0) in host numpy; with
    stored_DM, as it comes back from a file that holds it dispersed by that
    DM: one rotation to the stored state, one back (module docstring)."""
    from pulseportraiture_amd import pplib, synth
    freqs = synth.channel_freqs(nchan, nu0, bw)
    _, _, model = pplib.read_model(synth.EXAMPLE_GMODEL, pplib.get_bin_centers(nbin), freqs, P0,
                                   quiet=True)
    rot = -(np.ones(nsub) * phase)[:, None] - (np.ones(nsub) * dDM)[:, None] * \
        dispersion(freqs, 1.0, nu0)
    if stored_DM is None:
        return freqs, model, rotate(model[None], rot)
    back = dispersion(freqs, stored_DM, nu0)
    return freqs, model, rotate(rotate(model[None], rot - back), back)


def assert_within_rotated_quantisation(got, want, scl):
    """got, want [..., nbin]; scl [...] the stored steps (module docstring)."""
    nbin = got.shape[-1]
    d = got - want
    slack = 1e-9 * np.abs(want).max()
    assert (np.sqrt((d ** 2).mean(axis=-1)) <= 0.5 * scl + slack).all()
    assert (np.abs(d).max(axis=-1) <= 0.5 * np.sqrt(nbin) * scl + slack).all()


def test_make_fake_pulsar_noise_free(gpu, par, tmp_path):
    """The stored, dispersed profiles dedispersed by load_data equal the model
    rotated by -phase and -dDM about nu0 (through the stored state: module
    docstring; baseline left in: the comparison is of the stored values)."""
    from pulseportraiture_amd import archive, pplib, psrfits, synth
    out = str(tmp_path / "fake.fits")
    nsub, nchan, nbin = 8, 16, 256
    pplib.make_fake_pulsar(synth.EXAMPLE_GMODEL, par, outfile=out, nsub=nsub, nchan=nchan,
                           nbin=nbin, noise_stds=0, dDM=2e-3, phase=0.03, dedispersed=False,
                           tsub=60.0, quiet=True)
    freqs, model, port = noise_free(nsub, nchan, nbin, 0.03, 2e-3, stored_DM=DM0)
    f = psrfits.PSRFITSFile(out)
    scl = f.meta()["scl"][:, 0]
    assert f.info.dedispersed == 0 and f.text("source") == "J1234+5678"
    f.close()
    d = archive.load_data(out, dedisperse=True, rm_baseline=False, quiet=True)
    assert d.subints.shape == (nsub, 1, nchan, nbin) and d.dmc == 1 and d.DM == DM0
    assert_within_rotated_quantisation(d.subints[:, 0], port, scl)
    np.testing.assert_array_equal(d.freqs, np.tile(freqs, (nsub, 1)))
    np.testing.assert_array_equal(d.Ps, P0)
    np.testing.assert_array_equal(d.weights, 1.0)
    assert [e.as_tuple() for e in d.epochs] == [(57000, 30 + 60 * i, 0.0) for i in range(nsub)]
    assert d.nu0 == 1500.0 and d.bw == 800.0 and d.telescope == "GBT"
    # stored dispersed: without dedispersion the low channels are far from the model
    raw = archive.load_data(out, rm_baseline=False, quiet=True)
    assert raw.dmc == 0 and np.abs(raw.subints[:, 0] - port).max() > 0.1 * np.abs(port).max()


def test_make_fake_pulsar_options(gpu, par, tmp_path):
    """Per-subint phase and dDM, the DM(nu) law, the scattering override,
    scales, explicit scintillation, four polarisations, stored dedispersed:
    the host helpers applied in the reference's order."""
    from pulseportraiture_amd import archive, pplib, psrfits, synth
    out = str(tmp_path / "opts.fits")
    nsub, nchan, nbin = 2, 5, 64
    phase, dDM = np.array([0.03, -0.2]), np.array([2e-3, -1e-3])
    xs, Cs, scint = [-2.0, -4.0], [1.0, 0.1], [0.7, 2.5, 0.1, 0.3, 4.0, 0.6]
    scales = np.linspace(0.5, 2.0, nchan)
    wts = np.ones((nsub, nchan))
    wts[1, 3] = 0.0
    pplib.make_fake_pulsar(synth.EXAMPLE_GMODEL, par, outfile=out, nsub=nsub, npol=4, nchan=nchan,
                           nbin=nbin, noise_stds=0.0, scales=scales, phase=phase, dDM=dDM,
                           weights=wts, dedispersed=True, t_scat=2e-5, xs=xs, Cs=Cs, nu_DM=1400.0,
                           scint=scint, state="Stokes", quiet=True)
    freqs, model, _ = noise_free(nsub, nchan, nbin, 0.0, 0.0)
    taus = pplib.scattering_times(2e-5 / P0, pplib.scattering_alpha, freqs, 1500.0)
    f = psrfits.PSRFITSFile(out)
    scl = f.meta()["scl"]
    assert f.text("pol_type") == "IQUV" and f.info.dedispersed == 1
    f.close()
    d = archive.load_data(out, pscrunch=False, rm_baseline=False, quiet=True)
    assert d.subints.shape == (nsub, 4, nchan, nbin) and d.dmc == 1
    np.testing.assert_array_equal(d.weights, wts)
    eps = np.finfo(np.float64).eps
    for s in range(nsub):
        ph = pplib.phase_transform(phase[s], DM0 + dDM[s], 1500.0, 1400.0, P0)
        want = pplib.add_DM_nu(model, -ph, -dDM[s], P0, freqs, xs, Cs, 1400.0)
        want = np.fft.irfft(pplib.scattering_portrait_FT(taus, nbin) * np.fft.rfft(want, axis=-1),
                            nbin, axis=-1)
        want = pplib.add_scintillation(want, scint) * scales[:, None]
        for p in range(4):  # stored as generated (no rotation on load): half a step
            tol = 0.5 * scl[s, p][:, None] * (1 + 1e-9) + 1e-9 * np.abs(want).max() + \
                4 * eps * np.abs(want)
            assert (np.abs(d.subints[s, p] - want) <= tol).all()


def test_make_fake_pulsar_get_toas(gpu, par, tmp_path):
    """Injection and recovery: S/N of a few hundred per channel, so the fits
    converge and the weighted mean DM offset is the injected one within 5 of
    its standard errors.  Converged statuses are scipy trust-ncg's 0 (gradient
    below tolerance) and 2 (no predicted reduction: the fp64 floor at the
    minimum); 1 (iteration cap) and 3 (linear-algebra failure) are not."""
    from pulseportraiture_amd import pplib, pptoas, synth
    out = str(tmp_path / "noisy.fits")
    nsub, nchan, nbin, dDM = 8, 16, 256, 2e-3
    _, model, _ = noise_free(1, nchan, nbin, 0.0, 0.0)
    sigma = np.sqrt((model ** 2).sum(axis=1)).mean() / 300.0
    pplib.make_fake_pulsar(synth.EXAMPLE_GMODEL, par, outfile=out, nsub=nsub, nchan=nchan,
                           nbin=nbin, noise_stds=sigma, dDM=dDM, phase=0.03, dedispersed=False,
                           tsub=60.0, seed=20240917, quiet=True)
    # the seed fixes the file, however the subints are chunked: a workspace
    # limit of three subints' worth makes three chunks of the eight
    again = str(tmp_path / "again.fits")
    limit = gpu.workspace_limit()
    gpu.set_workspace_limit(3 * 10 * nchan * nbin)
    try:
        assert pplib._chunk_subints(gpu, 1, nchan, nbin) == 3
        pplib.make_fake_pulsar(synth.EXAMPLE_GMODEL, par, outfile=again, nsub=nsub, nchan=nchan,
                               nbin=nbin, noise_stds=sigma, dDM=dDM, phase=0.03,
                               dedispersed=False, tsub=60.0, seed=20240917, quiet=True)
    finally:
        gpu.set_workspace_limit(limit)
    assert open(out, "rb").read() == open(again, "rb").read()
    shutil.copy(synth.EXAMPLE_GMODEL, str(tmp_path / "example.gmodel"))
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        gt = pptoas.GetTOAs([out], "example.gmodel", quiet=True)
        gt.get_TOAs(quiet=True)
    finally:
        os.chdir(cwd)
    assert len(gt.TOA_list) == nsub
    assert set(int(r) for r in gt.rcs[0]) <= {0, 2}
    dd = np.asarray(gt.DMs[0]) - DM0
    w = np.asarray(gt.DM_errs[0]) ** -2.0
    mean, err = (w * dd).sum() / w.sum(), w.sum() ** -0.5
    print("mean dDM %.6e +- %.2e (injected %.1e)" % (mean, err, dDM))
    assert abs(mean - dDM) <= 5.0 * err
    assert err < 0.05 * dDM  # the data can tell dDM from zero


@pytest.mark.parametrize("npol,state", [(1, "Intensity"), (4, "Coherence")])
def test_write_and_unload_archive_roundtrip(gpu, par, tmp_path, npol, state):
    import torch
    from pulseportraiture_amd import archive, pplib, psrfits
    from pulseportraiture_amd.mjd import MJD
    nsub, nchan, nbin = 3, 5, 64
    rng = np.random.default_rng(npol)
    data = rng.normal(size=(nsub, npol, nchan, nbin)) + 5.0
    freqs = np.linspace(1180.0, 1820.0, nchan)
    wts = rng.integers(0, 3, (nsub, nchan)).astype(np.float64)
    a, b = str(tmp_path / "a.fits"), str(tmp_path / "b.fits")
    start = MJD(56000, 100, 0.5)
    kw = dict(tsub=10.0, start_MJD=start, weights=wts, dedispersed=False, state=state, quiet=True)
    pplib.write_archive(data, par, freqs, outfile=a, **kw)
    dev = torch.as_tensor(data, device=gpu.device)
    pplib.write_archive(dev, par, freqs, outfile=b, **kw)
    assert torch.equal(dev.cpu(), torch.as_tensor(data))  # the caller's tensor is not rotated
    assert open(a, "rb").read() == open(b, "rb").read()
    f = psrfits.PSRFITSFile(a)
    scl = f.meta()["scl"]
    assert f.info.dedispersed == 0
    f.close()
    d = archive.load_data(a, dedisperse=True, pscrunch=False, rm_baseline=False, quiet=True)
    back = dispersion(freqs, DM0, freqs.mean())[None, None]
    assert_within_rotated_quantisation(d.subints, rotate(rotate(data, -back), back), scl)
    np.testing.assert_array_equal(d.weights, wts)
    np.testing.assert_array_equal(d.freqs, np.tile(freqs, (nsub, 1)))
    np.testing.assert_array_equal(d.Ps, P0)
    assert [e.as_tuple() for e in d.epochs] == [(start + (5.0 + 10.0 * i)).as_tuple()
                                                for i in range(nsub)]
    assert d.DM == DM0 and d.dmc == 1 and d.nu0 == freqs.mean() and d.bw == 800.0
    assert d.source == "J1234+5678" and list(d.subtimes) == [10.0] * nsub
    assert archive.load_data(a, pscrunch=False, rm_baseline=False, quiet=True).dmc == 0
    # unload_new_archive: new data, DM and weights in the loaded archive's frame
    new = d.subints * 2.0 + 1.0
    w2 = np.ones((nsub, nchan))
    w2[0, 1] = 0.0
    c = str(tmp_path / "c.fits")
    pplib.unload_new_archive(new, d, c, DM=1.5, dmc=1, weights=w2, quiet=True)
    f = psrfits.PSRFITSFile(c)
    scl = f.meta()["scl"]
    f.close()
    e = archive.load_data(c, dedisperse=True, pscrunch=False, rm_baseline=False, quiet=True)
    eps = np.finfo(np.float64).eps
    assert (np.abs(e.subints - new) <= 0.5 * scl[..., None] * (1 + 1e-9) + 4 * eps * np.abs(new)).all()
    assert e.DM == 1.5 and e.dmc == 1 and e.state == d.state
    np.testing.assert_array_equal(e.weights, w2)
    np.testing.assert_array_equal(e.freqs, d.freqs)
    np.testing.assert_array_equal(e.Ps, d.Ps)
    for x, y in zip(e.epochs, d.epochs):
        assert (x.days, x.secs) == (y.days, y.secs) and abs(x.fracsec - y.fracsec) < 1e-9
    # arch by file name, metadata unchanged, stored dispersed
    c2 = str(tmp_path / "c2.fits")
    pplib.unload_new_archive(torch.as_tensor(new, device=gpu.device), a, c2, quiet=True)
    e2 = archive.load_data(c2, pscrunch=False, rm_baseline=False, quiet=True)
    assert e2.DM == DM0 and e2.dmc == 0
    np.testing.assert_array_equal(e2.weights, wts)


def test_align_archives_writes_fits(gpu, par, tmp_path):
    """align_archives(metafile) leaves <metafile>.algnd.fits: the returned
    portrait within half a quantisation step (one dedispersed subint, DM 0,
    nothing to rotate), weight 0 where no archive had weight, and
    ppspline.DataPortrait opens it.  DataPortrait removes a baseline (one
    constant per profile), so its port is compared up to that constant: the
    rest differs by the quantisation error minus its window mean, at most one
    step."""
    from pulseportraiture_amd import archive, ppalign, pplib, ppspline, psrfits, synth
    nchan, nbin = 8, 128
    _, model, _ = noise_free(1, nchan, nbin, 0.0, 0.0)
    sigma = np.sqrt((model ** 2).sum(axis=1)).mean() / 100.0
    wts = np.ones((2, nchan))
    wts[:, 2] = 0.0
    names = []
    for i in range(2):
        names.append(str(tmp_path / ("arch%d.fits" % i)))
        pplib.make_fake_pulsar(synth.EXAMPLE_GMODEL, par, outfile=names[-1], nsub=2, nchan=nchan,
                               nbin=nbin, noise_stds=sigma, phase=0.1 * i, dDM=1e-3 * i,
                               weights=wts, seed=5 + i, quiet=True)
    guess = str(tmp_path / "guess.fits")
    pplib.make_fake_pulsar(synth.EXAMPLE_GMODEL, par, outfile=guess, nsub=1, nchan=nchan,
                           nbin=nbin, noise_stds=0.0, quiet=True)
    meta = tmp_path / "archives.meta"
    meta.write_text("\n".join(names) + "\n")
    port = ppalign.align_archives(str(meta), guess, niter=1, quiet=True)
    out = str(meta) + ".algnd.fits"
    assert os.path.exists(out) and port.shape == (1, nchan, nbin)
    f = psrfits.PSRFITSFile(out)
    scl = f.meta()["scl"][0, 0]
    assert f.nsub == 1 and f.npol == 1 and f.info.dedispersed == 1 and f.info.dm == 0.0
    f.close()
    d = archive.load_data(out, dedisperse=True, rm_baseline=False, quiet=True)
    eps = np.finfo(np.float64).eps
    assert (np.abs(d.subints[0, 0] - port[0]) <=
            0.5 * scl[:, None] * (1 + 1e-9) + 4 * eps * np.abs(port[0])).all()
    want_w = np.ones(nchan)
    want_w[2] = 0.0
    np.testing.assert_array_equal(d.weights[0], want_w)
    assert d.DM == 0.0 and d.dmc == 1
    dp = ppspline.DataPortrait(out, quiet=True)
    assert dp.port.shape == (nchan, nbin) and not dp.port[2].any()
    ok = want_w > 0
    diff = (dp.port - port[0])[ok]
    assert (np.abs(diff - diff.mean(axis=1, keepdims=True)) <= scl[ok][:, None] * (1 + 1e-9)).all()
    # a list of names and no outfile: nothing is written, as before
    before = set(os.listdir(tmp_path))
    ppalign.align_archives(names, guess, niter=1, quiet=True)
    assert set(os.listdir(tmp_path)) == before
