"""ppalign's starting template made by the package: add_archives (the
stand-in for psradd -T [-P]), pplib.make_constant_portrait, smooth_archive
(the stand-in for psrsmooth -W) and the driver run().  Nothing here is pinned
against psradd or psrsmooth, which are not available: the yardsticks are the
numpy restatement tests/add_archives_reference.py (the oracle's
fit_phase_shift and profile_snr), the package's own reader and writer, and
pplib.smart_smooth.

Archives are written with pplib.write_archive into a temporary directory and
every comparison is against what load_data reads back from them (the stored,
quantised values)."""
import os

import numpy as np
import pytest

from tests import add_archives_reference as R
from tests.test_gpu_fake_pulsar import PAR, DM0, dispersion

pytestmark = pytest.mark.gpu

FREQS = np.array([1250.0, 1350.0, 1450.0, 1550.0])
ROTS = np.array([0.0, 0.13, -0.31, 0.42])
AMPS = np.array([1.0, 0.8, 1.2, 0.9])
# test_palign_noiseless: ten times the residual of one fit_phase_shift on the
# same noiseless profiles (docstring there)
NOISELESS_RESID = {64: 1.453e-4, 100: 1.070e-6}


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from pulseportraiture_amd.engine import get_engine
    return get_engine(0)


def write(path, data, par, weights=None, dedispersed=True, freqs=FREQS, **kw):
    from pulseportraiture_amd import pplib
    pplib.write_archive(np.asarray(data), par, freqs, outfile=str(path), tsub=10.0,
                        weights=weights, dedispersed=dedispersed, state="Intensity", quiet=True,
                        **kw)
    return str(path)


def load(name, **kw):
    from pulseportraiture_amd import archive
    kw.setdefault("rm_baseline", False)
    return archive.load_data(name, quiet=True, **kw)


def stored_steps(name):
    from pulseportraiture_amd import psrfits
    f = psrfits.PSRFITSFile(name)
    scl = f.meta()["scl"]
    f.close()
    return scl


def within_half_step(got, want, scl):
    eps = np.finfo(np.float64).eps
    return (np.abs(got - want) <= 0.5 * scl[..., None] * (1 + 1e-9) + 4 * eps * np.abs(want)).all()


def two_component(nbin):
    from pulseportraiture_amd.pplib import gaussian_profile
    return gaussian_profile(nbin, 0.4, 0.08) + 0.5 * gaussian_profile(nbin, 0.58, 0.15)


@pytest.fixture(scope="module")
def par(tmp_path_factory):
    p = tmp_path_factory.mktemp("par") / "fake.par"
    p.write_text(PAR)
    return str(p)


def palign_case(tmp, par, nbin, sigma, tag):
    """Four one-subint archives (units) of the two-component profile over four
    channels, rotated by ROTS; returns (metafile, names)."""
    prof = two_component(nbin)
    rng = np.random.default_rng(nbin)
    names = []
    for u, rot in enumerate(ROTS):
        x = AMPS[:, None] * R.rotate(prof, rot)[None]
        x = x + sigma * prof.max() * rng.normal(size=x.shape)
        names.append(write(tmp / ("%s%d_%d.fits" % (tag, nbin, u)), x[None, None], par))
    meta = tmp / ("%s%d.meta" % (tag, nbin))
    meta.write_text("\n".join(names) + "\n")
    return str(meta), names


@pytest.fixture(scope="module")
def noisy(tmp_path_factory, par, gpu):
    tmp = tmp_path_factory.mktemp("palign")
    return {nbin: palign_case(tmp, par, nbin, 0.02, "noisy") for nbin in (64, 100)}


def units_of(names):
    ds = [load(n) for n in names]
    x = np.concatenate([d.subints for d in ds])
    w = np.concatenate([d.weights for d in ds])
    return x, w


def test_add_archives_plain(gpu, par, tmp_path, capsys):
    """palign=False: the weighted mean of the loaded data, per channel, over
    every (archive, subint) -- tscrunched first or not, the same mean -- to
    1e-12 max; one archive with a zapped channel, one channel zapped in all,
    an archive of another nbin skipped with a note; the file within half a
    quantisation step (no rotation on the way), weights 1 or 0, the first
    archive's DM and dedispersed state."""
    from pulseportraiture_amd import ppalign
    rng = np.random.default_rng(3)
    nsub, nchan, nbin = 2, 4, 64
    names = []
    for i in range(3):
        w = rng.uniform(0.5, 2.0, (nsub, nchan))
        if i == 1:
            w[:, 2] = 0.0
        w[:, 3] = 0.0
        x = rng.normal(size=(nsub, 1, nchan, nbin)) + 5.0 + i
        names.append(write(tmp_path / ("a%d.fits" % i), x, par, weights=w, dedispersed=False))
    other = write(tmp_path / "other.fits", rng.normal(size=(1, 1, nchan, 128)), par,
                  dedispersed=False)
    missing = str(tmp_path / "missing.fits")
    meta = tmp_path / "plain.meta"
    meta.write_text("\n".join(names[:2] + [other, missing, names[2]]) + "\n")
    x, w = units_of(names)
    want, want_w = R.add_units(x, w, np.zeros(len(x)))
    np.testing.assert_array_equal(want_w, [1.0, 1.0, 1.0, 0.0])
    out = str(tmp_path / "sum.fits")
    port, phases, wout = ppalign.add_archives(str(meta), out, quiet=True)
    note = capsys.readouterr().out
    assert "other.fits" in note and "Skipping" in note
    assert port.shape == (1, nchan, nbin) and phases.shape == (3,) and not phases.any()
    np.testing.assert_array_equal(wout, want_w)
    assert np.abs(port - want).max() <= 1e-12 * np.abs(want).max()
    assert not port[0, 3].any()
    # one unit per subint: the same mean, six units
    port2, phases2, _ = ppalign.psradd_archives(str(meta), None, tscrunch=False, quiet=True)
    assert phases2.shape == (6,)
    assert np.abs(port2 - want).max() <= 1e-12 * np.abs(want).max()
    # the file
    d = load(out)
    assert d.subints.shape == (1, 1, nchan, nbin) and d.dmc == 0 and d.DM == DM0
    assert within_half_step(d.subints[0], port, stored_steps(out)[0])
    np.testing.assert_array_equal(d.weights[0], want_w)
    np.testing.assert_array_equal(d.freqs[0], FREQS)
    with pytest.raises(RuntimeError, match="no usable archive"):
        ppalign.add_archives([missing], None, quiet=True)


@pytest.mark.parametrize("nbin", [64, 100])
def test_add_archives_palign(gpu, noisy, tmp_path, nbin):
    """palign=True on four noisy units (sigma = 0.02 of the peak): every final
    phase within 1e-3 phase_err of the restatement's (the project's bound for
    FFTFIT against the oracle), the phase differences within 5 phase_err of
    minus the injected rotations (modulo 1, relative to unit 0), and the
    portrait within 1e-9 max of the restatement's portrait -- the one it forms
    with its own phases, and the sum restated with the phases the function
    returns.  (The first holds because the device's brute-force search and
    Nelder-Mead polish follow scipy's step for step on these profiles, so the
    phases agree far inside the 1e-3 phase_err asked of them: a difference of
    1e-3 phase_err would move the portrait by about 1e-5 of its maximum.)"""
    from pulseportraiture_amd import ppalign
    meta, names = noisy[nbin]
    x, w = units_of(names)
    ref_ph, ustar, errs = R.palign_phases(x[:, 0], np.zeros_like(w), w)
    out = str(tmp_path / "palign.fits")
    port, phases, wout = ppalign.add_archives(meta, out, palign=True, quiet=True)
    d = (phases - ref_ph + 0.5) % 1.0 - 0.5
    print("nbin %d: reference unit %d, phases %s, restatement %s, |diff| / phase_err %s" % (
        nbin, ustar, phases, ref_ph, np.abs(d) / errs))
    assert phases[ustar] == 0.0
    assert (np.abs(d) <= 1e-3 * errs).all()
    inj = ((phases - phases[0]) + ROTS + 0.5) % 1.0 - 0.5
    print("injected-rotation residuals / phase_err: %s" % (np.abs(inj) / errs))
    assert (np.abs(inj) <= 5.0 * errs).all()
    want, want_w = R.add_units(x, w, phases)
    own, _ = R.add_units(x, w, ref_ph)
    print("portrait - restatement / max: %.3e with its own phases, %.3e with the returned ones" % (
        np.abs(port - own).max() / np.abs(own).max(), np.abs(port - want).max() / np.abs(want).max()))
    assert np.abs(port - own).max() <= 1e-9 * np.abs(own).max()
    assert np.abs(port - want).max() <= 1e-9 * np.abs(want).max()
    np.testing.assert_array_equal(wout, want_w)
    back = load(out)
    assert back.dmc == 1 and within_half_step(back.subints[0], port, stored_steps(out)[0])
    # the sum is better aligned than the plain one: its peak is higher
    plain, _, _ = ppalign.add_archives(meta, None, quiet=True)
    assert port.max() > 1.5 * plain.max()


def fit_residual(gpu, x, w):
    """The residual of one fit_phase_shift per unit on the units' profiles,
    with phase_shift_batch: max |rotate(p_u, phase_u) - p_ref| / max |p_ref|
    over the units, p_ref the first unit's profile."""
    p = R.fscrunch(x[:, 0], np.zeros_like(w), w)
    ph = gpu.phase_shift_batch(p, p[0], Ns=p.shape[-1])[:, 0].cpu().numpy()
    return np.abs(R.rotate(p, ph) - p[0]).max() / np.abs(p[0]).max()


@pytest.mark.parametrize("nbin", [64, 100])
def test_palign_noiseless(gpu, par, tmp_path, nbin):
    """Without noise the sum of the four rotated copies is the reference
    unit's own portrait, to ten times the residual of a single fit (the sum
    compounds four fits).  That residual -- fit_residual above, the existing
    phase_shift_batch on these profiles as stored (16-bit samples) -- was
    measured on an MI355X as 1.453e-05 at nbin 64 (where each rotation also
    drops the imaginary part of the Nyquist harmonic) and 1.070e-07 at nbin
    100; NOISELESS_RESID holds ten times those.  The portrait itself then
    differed from the reference unit's by 8.6e-06 and 8.7e-10."""
    from pulseportraiture_amd import ppalign
    meta, names = palign_case(tmp_path, par, nbin, 0.0, "clean")
    x, w = units_of(names)
    resid = fit_residual(gpu, x, w)
    port, phases, _ = ppalign.add_archives(meta, None, palign=True, quiet=True)
    ustar = int(np.flatnonzero(phases == 0.0)[0])
    got = np.abs(port[0] - x[ustar, 0]).max() / np.abs(x[ustar, 0]).max()
    print("nbin %d: single-fit residual %.3e, portrait - reference unit %.3e" % (nbin, resid, got))
    assert got <= NOISELESS_RESID[nbin]


def test_make_constant_portrait_given_profile(gpu, par, tmp_path):
    from pulseportraiture_amd import pplib
    nsub, nchan, nbin = 2, 4, 64
    rng = np.random.default_rng(5)
    src = write(tmp_path / "src.fits", rng.normal(size=(nsub, 1, nchan, nbin)), par,
                dedispersed=False)
    prof = two_component(nbin)
    wts = np.ones((nsub, nchan))
    wts[1, 2] = 0.0
    wts[0, 0] = 3.0
    out = str(tmp_path / "const.fits")
    pplib.make_constant_portrait(src, out, profile=prof, DM=1.5, dmc=False, weights=wts,
                                 quiet=True)
    d = load(out)
    assert d.subints.shape == (nsub, 1, nchan, nbin) and d.DM == 1.5 and d.dmc == 0
    assert within_half_step(d.subints, np.broadcast_to(prof, d.subints.shape), stored_steps(out))
    np.testing.assert_array_equal(d.weights, wts)
    np.testing.assert_array_equal(d.freqs, load(src).freqs)
    # weights=None: ones
    pplib.make_constant_portrait(src, out, profile=prof, quiet=True)
    np.testing.assert_array_equal(load(out).weights, 1.0)
    for bad in (prof[:-1], np.zeros(nbin + 1), np.zeros((2, nbin))):
        with pytest.raises(ValueError):
            pplib.make_constant_portrait(src, out, profile=bad, quiet=True)


@pytest.mark.parametrize("nbin", [64, 100])
def test_make_constant_portrait_own_profile(gpu, par, tmp_path, nbin):
    """profile=None: every row is the archive's T-, P- and F-scrunched profile
    as the restatement forms it from the loaded data -- stored dispersed, so
    the sum dedisperses; one channel zapped in one subint."""
    from pulseportraiture_amd import pplib
    nsub, nchan = 2, 4
    rng = np.random.default_rng(nbin)
    x = AMPS[:, None] * two_component(nbin) + 0.01 * rng.normal(size=(nsub, 1, nchan, nbin))
    wts = rng.uniform(0.5, 2.0, (nsub, nchan))
    wts[1, 1] = 0.0
    src = write(tmp_path / "src.fits", x, par, weights=wts, dedispersed=False)
    d = load(src)
    assert d.dmc == 0
    dd = np.tile(dispersion(FREQS, DM0, d.nu0), (nsub, 1))
    want = R.scrunched_profile(d.subints[:, 0], dd, d.weights)
    # the scrunched profile keeps the pulse (it was dedispersed, not smeared)
    assert want.max() > 0.75 * (AMPS[:, None] * two_component(nbin)).mean(axis=0).max()
    got = pplib.scrunched_profile(load(src, pscrunch=True, host=False))
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    out = str(tmp_path / "own.fits")
    pplib.make_constant_portrait(src, out, profile=None, quiet=True)
    e = load(out)
    assert e.subints.shape == (nsub, 1, nchan, nbin) and e.DM == 0.0 and e.dmc == 0
    assert within_half_step(e.subints, np.broadcast_to(want, e.subints.shape), stored_steps(out))
    np.testing.assert_array_equal(e.weights, 1.0)


def test_smooth_archive(gpu, par, tmp_path):
    """<archive>.sm: rows of positive weight are pplib.smart_smooth of the
    loaded rows (the levels DataPortrait.smooth_portrait(smart=True) searches),
    a row of weight 0 is unchanged, both within half a quantisation step; an
    odd nbin is refused."""
    from pulseportraiture_amd import ppalign, pplib
    nsub, nchan, nbin = 2, 3, 64
    rng = np.random.default_rng(11)
    x = np.array([1.0, 0.7, 1.3])[:, None] * two_component(nbin) + \
        0.05 * rng.normal(size=(nsub, 1, nchan, nbin))
    wts = np.ones((nsub, nchan))
    wts[1, 0] = 0.0
    src = write(tmp_path / "noisy.fits", x, par, weights=wts, freqs=FREQS[:3])
    d = load(src)
    name = ppalign.smooth_archive(src, quiet=True)
    assert name == src + ".sm" and os.path.exists(name)
    s = load(name)
    scl = stored_steps(name)
    want = pplib.smart_smooth(d.subints.reshape(-1, nbin),
                              try_nlevels=min(8, int(np.log2(nbin)))).reshape(d.subints.shape)
    assert np.abs(want - d.subints).max() > 0.01  # something was smoothed
    on = wts > 0
    assert within_half_step(s.subints[:, 0][on], want[:, 0][on], scl[:, 0][on])
    assert within_half_step(s.subints[1, 0, 0], d.subints[1, 0, 0], scl[1, 0, 0])
    np.testing.assert_array_equal(s.weights, wts)
    assert s.dmc == d.dmc and s.DM == d.DM
    # smart=False and an explicit name: wavelet_smooth at the given level
    name2 = ppalign.psrsmooth_archive(src, outfile=str(tmp_path / "w.fits"), smart=False, nlevel=3,
                                      fact=1.5, quiet=True)
    s2 = load(name2)
    want2 = pplib.wavelet_smooth(d.subints[0, 0], nlevel=3, fact=1.5)
    assert within_half_step(s2.subints[0, 0], want2, stored_steps(name2)[0, 0])
    odd = write(tmp_path / "odd.fits", rng.normal(size=(1, 1, 3, 45)), par, freqs=FREQS[:3])
    with pytest.raises(ValueError, match="multiple of 2"):
        ppalign.smooth_archive(odd, quiet=True)
    assert not os.path.exists(odd + ".sm")


def leftovers(path):
    return sorted(f for f in os.listdir(path) if f.startswith("ppalign.") or ".tmp" in f)


def test_run(gpu, noisy, par, tmp_path, monkeypatch):
    """run() with no guess is add_archives then align_archives by hand, with
    fwhm the hand-made constant portrait then align_archives (bitwise); the
    temporary guess is gone afterwards, also when align_archives raises."""
    from pulseportraiture_amd import ppalign, pplib
    meta, names = noisy[64]
    monkeypatch.chdir(tmp_path)
    got = ppalign.run(meta, palign=True, outfile=str(tmp_path / "run.fits"), smooth=True)
    assert leftovers(tmp_path) == []
    assert os.path.exists(str(tmp_path / "run.fits.sm"))
    guess = str(tmp_path / "guess.fits")
    ppalign.add_archives(meta, guess, palign=True, quiet=True)
    want = ppalign.align_archives(meta, guess, outfile=str(tmp_path / "hand.fits"), quiet=True)
    np.testing.assert_array_equal(got, want)
    assert open(str(tmp_path / "run.fits"), "rb").read() == \
        open(str(tmp_path / "hand.fits"), "rb").read()
    # -g fwhm
    got = ppalign.run(meta, fwhm=0.05, outfile=str(tmp_path / "run2.fits"))
    assert leftovers(tmp_path) == []
    pplib.make_constant_portrait(names[0], guess, profile=pplib.gaussian_profile(64, 0.5, 0.05),
                                 DM=0.0, dmc=False, weights=None, quiet=True)
    want = ppalign.align_archives(meta, guess, outfile=str(tmp_path / "hand2.fits"), quiet=True)
    np.testing.assert_array_equal(got, want)
    # a one-channel guess: the first archive's own profile in every channel
    one = write(tmp_path / "one.fits", two_component(64)[None, None, None], par,
                freqs=np.array([1400.0]), nu0=1400.0, bw=100.0)
    got = ppalign.run(meta, initial_guess=one, outfile=str(tmp_path / "run3.fits"))
    assert leftovers(tmp_path) == []
    pplib.make_constant_portrait(names[0], guess, profile=None, quiet=True)
    want = ppalign.align_archives(meta, guess, outfile=str(tmp_path / "hand3.fits"), quiet=True)
    np.testing.assert_array_equal(got, want)

    # align_archives raising: the temporary file is still removed
    seen = []

    def boom(metafile, initial_guess=None, **kw):
        seen.append((initial_guess, os.path.exists(initial_guess)))
        raise RuntimeError("boom")
    monkeypatch.setattr(ppalign, "align_archives", boom)
    with pytest.raises(RuntimeError, match="boom"):
        ppalign.run(meta)
    assert len(seen) == 1 and seen[0][1] and not os.path.exists(seen[0][0])
    assert os.path.realpath(os.path.dirname(seen[0][0])) == os.path.realpath(str(tmp_path))
    assert leftovers(tmp_path) == []
