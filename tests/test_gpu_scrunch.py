"""ppf_scrunch_subints / Engine.scrunch_subints, archive.scrunch,
pplib.scrunch_archive and load_data(fscrunch=True): the stand-ins for pam's
-f / -b.  Nothing here is pinned against pam, which is not available; the
yardstick is the numpy restatement of the definition, tests/scrunch_reference.py.

- against numpy at 1e-12 max|ref| -- the bound test_gpu_fscrunch.py holds the
  channel sum to, applied to the sum's output after the division and the bin
  mean -- on the LDS-FFT kernel (nbin 64), the register-FFT one (2048), the
  generic-length sums (100 and the odd 63) and with a group that crosses a
  kFsSlice = 32 boundary (f = 40); every case has a zero-weight channel
  inside a group with a NaN under it, and one all-zero group;
- f = 1, b = 1, phase 0 returns the input where w != 0;
- int16 RawSubints input equals unpack_subints followed by the fp64 call,
  BITWISE, at nbin 64 and 2048, with every polarisation kept, AA + BB summed
  and a single ipol; raw input the kernels do not read (uint8, nbin 100)
  goes through bounded unpacked chunks to the same bits;
- a group alone in a call equals itself among others, and three subints equal
  the same call under a workspace limit of one subint's units, bitwise;
- refusals: f not dividing nchan, b not dividing nbin, nbin / b = 8, nulls;
- file level: scrunch_archive of a 2 x 16 x 256 dispersed make_fake_pulsar file
  to 4 channels x 128 bins -- shapes, freqs and weights exactly the
  restatement's, samples within half a stored quantisation step;
  load_data(fscrunch=True) equals archive.scrunch(nchan=1)."""
import ctypes

import numpy as np
import pytest

from tests import scrunch_reference as R

pytestmark = pytest.mark.gpu

SLICE = 32  # kFsSlice
PAR = ("PSR J1234+5678\nRAJ 12:34:00.0\nDECJ +56:07:08.9\nF0 345.67890123456789\n"
       "PEPOCH 57000.0\nDM 34.56789\n")

# nbin, b, f, nchan, npol
CASES = [(64, 4, 4, 8, 1), (64, 4, 4, 8, 4), (2048, 2, 4, 8, 1), (2048, 2, 4, 8, 4),
         (100, 5, 4, 8, 1), (100, 5, 4, 8, 4), (63, 3, 4, 8, 1), (63, 3, 4, 8, 4),
         (64, 4, 40, 80, 1), (2048, 2, 40, 80, 1)]


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from pulseportraiture_amd.engine import get_engine
    return get_engine(0)


def inputs(nsub, npol, nchan, nbin, seed=0):
    rng = np.random.default_rng(100000 * nbin + 100 * nchan + 10 * npol + nsub + seed)
    x = rng.normal(size=(nsub, npol, nchan, nbin)) + 3.0
    ph = rng.uniform(-2.5, 2.5, (nsub, nchan))  # beyond +-1 turn
    w = rng.uniform(0.5, 2.0, (nsub, nchan))
    return x, ph, w


def host(ts):
    return [t.cpu().numpy() for t in ts]


@pytest.mark.parametrize("nbin,b,f,nchan,npol", CASES)
def test_against_numpy(eng, nbin, b, f, nchan, npol):
    nsub = 2
    x, ph, w = inputs(nsub, npol, nchan, nbin)
    w[0, 1] = 0.0               # a zero-weight channel inside group 0 of subint 0 ...
    w[0, f - 1] = 0.0
    w[1, f:2 * f] = 0.0         # ... and group 1 of subint 1 all zero
    xn = x.copy()
    xn[0, :, 1] = np.nan        # never read: whatever it holds
    xn[1, :, f + 1] = np.nan
    got, wgot = host(eng.scrunch_subints(xn, w, ph, f, b))
    x[0, :, 1] = 0.0
    x[1, :, f + 1] = 0.0
    ref, wref = R.scrunch(x, w, ph, f, b)
    assert got.shape == (nsub, npol, nchan // f, nbin // b) and wgot.shape == (nsub, nchan // f)
    np.testing.assert_array_equal(wgot, wref)
    assert np.abs(ref).max() > 1.0
    err = np.abs(got - ref).max()
    print("nbin %d b %d f %d npol %d: max|got - ref| = %.3e, max|ref| = %.3e" % (
        nbin, b, f, npol, err, np.abs(ref).max()))
    assert np.isfinite(got).all()
    assert err <= 1e-12 * np.abs(ref).max()
    assert not got[1, :, 1].any() and wgot[1, 1] == 0.0


@pytest.mark.parametrize("nbin", [64, 2048, 100, 63])
def test_identity(eng, nbin):
    x, _, w = inputs(2, 2, 5, nbin)
    w[1, 2] = 0.0
    got, wgot = host(eng.scrunch_subints(x, w, np.zeros_like(w), 1, 1))
    np.testing.assert_array_equal(wgot, w)
    ref = x * (w != 0.0)[:, None, :, None]
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    assert not got[1, :, 2].any()


def raw_inputs(eng, nsub, npol, nchan, nbin, dtype=np.int16, seed=0):
    import torch
    rng = np.random.default_rng(7 * nbin + nchan + npol + seed)
    if dtype == np.uint8:
        raw = rng.integers(0, 256, size=(nsub, npol, nchan, nbin)).astype(dtype)
    else:
        raw = rng.integers(-32767, 32768, size=(nsub, npol, nchan, nbin)).astype(dtype)
    scl = rng.uniform(1e-3, 2.0, size=(nsub, npol, nchan))
    offs = rng.normal(size=(nsub, npol, nchan))
    ph = rng.uniform(-1.5, 1.5, (nsub, nchan))
    w = rng.uniform(0.5, 2.0, (nsub, nchan))
    w[0, 1] = 0.0
    w[nsub - 1, nchan - 2:] = 0.0
    dev = eng.device
    return [torch.as_tensor(a, device=dev) for a in (raw, scl, offs)], ph, w


def unpacked(eng, raw, scl, offs, pmode, ipol):
    if pmode == 0 and ipol is not None:
        raw, scl, offs = [t[:, ipol:ipol + 1].contiguous() for t in (raw, scl, offs)]
    return eng.unpack_subints(raw, scl, offs, pmode=pmode)


MODES = [(0, None), (1, 0), (0, 2), (2, 0)]  # every polarisation, AA + BB, ipol 2, Stokes I


@pytest.mark.parametrize("pmode,ipol", MODES)
@pytest.mark.parametrize("nbin,b,f,nchan", [(64, 4, 4, 8), (2048, 2, 4, 8), (64, 2, 40, 40),
                                            (2048, 4, 40, 40), (4096, 2, 2, 4)])
def test_raw_equals_unpacked_bitwise(eng, nbin, b, f, nchan, pmode, ipol):
    from pulseportraiture_amd.engine import RawSubints
    (raw, scl, offs), ph, w = raw_inputs(eng, 3, 4, nchan, nbin)
    rs = RawSubints(raw, scl, offs, pmode=pmode, ipol=0 if ipol is None else ipol)
    got, wgot = host(eng.scrunch_subints(rs, w, ph, f, b, all_pols=ipol is None and pmode == 0))
    x = unpacked(eng, raw, scl, offs, pmode, ipol)
    ref, wref = host(eng.scrunch_subints(x, w, ph, f, b))
    assert got.shape == ref.shape == (3, 4 if (pmode == 0 and ipol is None) else 1, nchan // f,
                                      nbin // b)
    assert np.abs(ref).max() > 0.0
    np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(wgot, wref)


@pytest.mark.parametrize("dtype,nbin", [(np.uint8, 64), (np.int16, 100), (np.float32, 2048)])
def test_raw_unpacked_in_chunks(eng, dtype, nbin):
    """Raw input the kernels do not read themselves: unpacked a bounded chunk
    at a time (here one subint), to the bits of unpacking it all first."""
    from pulseportraiture_amd.engine import RawSubints
    (raw, scl, offs), ph, w = raw_inputs(eng, 3, 2, 8, nbin, dtype=dtype)
    x = unpacked(eng, raw, scl, offs, 1, 0)
    ref, wref = host(eng.scrunch_subints(x, w, ph, 4, 2))
    keep = eng.SCRUNCH_UNPACK_BYTES
    eng.SCRUNCH_UNPACK_BYTES = 8 * 8 * nbin  # one subint of the summed polarisation
    try:
        got, wgot = host(eng.scrunch_subints(RawSubints(raw, scl, offs, pmode=1), w, ph, 4, 2))
    finally:
        eng.SCRUNCH_UNPACK_BYTES = keep
    np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(wgot, wref)


@pytest.mark.parametrize("nbin,b,f,nchan", [(64, 4, 4, 8), (2048, 2, 4, 8), (100, 5, 4, 8),
                                            (64, 4, 40, 80), (2048, 2, 40, 80)])
def test_group_independent_of_the_call(eng, nbin, b, f, nchan):
    nsub, npol = 3, 2
    x, ph, w = inputs(nsub, npol, nchan, nbin, seed=3)
    w[1, 2] = 0.0
    full, wfull = host(eng.scrunch_subints(x, w, ph, f, b))
    again, _ = host(eng.scrunch_subints(x, w, ph, f, b))
    np.testing.assert_array_equal(again, full)
    ng = nchan // f
    for s, g in ((0, 0), (1, 0), (2, ng - 1)):
        sl = slice(g * f, (g + 1) * f)
        alone, walone = host(eng.scrunch_subints(x[s:s + 1, :, sl], w[s:s + 1, sl],
                                                 ph[s:s + 1, sl], f, b))
        np.testing.assert_array_equal(alone[0, :, 0], full[s, :, g])
        assert walone[0, 0] == wfull[s, g]
    # one subint's units per chunk: per unit the slices' partial spectra and the
    # spectrum, the weights and phases, W and the profile, and 256 bytes of
    # alignment for each of the six arrays
    nslice = (f + SLICE - 1) // SLICE
    per_unit = (nslice + 1) * (nbin // 2 + 1) * 16 + 2 * f * 8 + 8 + nbin * 8 + 1536
    limit = eng.workspace_limit()
    eng.set_workspace_limit(npol * ng * per_unit + 64)
    try:
        chunked, wchunked = host(eng.scrunch_subints(x, w, ph, f, b))
    finally:
        eng.set_workspace_limit(limit)
    np.testing.assert_array_equal(chunked, full)
    np.testing.assert_array_equal(wchunked, wfull)


def test_raw_under_a_workspace_limit(eng):
    from pulseportraiture_amd.engine import RawSubints
    nbin, f, b, nchan = 2048, 4, 2, 8
    (raw, scl, offs), ph, w = raw_inputs(eng, 3, 2, nchan, nbin, seed=5)
    rs = RawSubints(raw, scl, offs, pmode=0)
    full, _ = host(eng.scrunch_subints(rs, w, ph, f, b, all_pols=True))
    per_unit = 2 * (nbin // 2 + 1) * 16 + 2 * f * 8 + 8 + nbin * 8 + 1536
    limit = eng.workspace_limit()
    eng.set_workspace_limit(3 * per_unit + 64)  # three of a subint's four units: chunks straddle
    try:
        chunked, _ = host(eng.scrunch_subints(rs, w, ph, f, b, all_pols=True))
    finally:
        eng.set_workspace_limit(limit)
    np.testing.assert_array_equal(chunked, full)


def test_refusals(eng):
    import torch
    from pulseportraiture_amd import _lib
    from pulseportraiture_amd.engine import PPFitError, RawSubints
    x, ph, w = inputs(2, 1, 8, 64)
    for f, b, code in ((3, 1, -1), (5, 1, -1), (1, 3, -1), (1, 5, -1), (0, 1, -1), (1, 0, -1),
                       (1, 8, -3)):  # 64 / 8 = 8 bins
        with pytest.raises(PPFitError, match="error %d" % code):
            eng.scrunch_subints(x, w, ph, f, b)
    with pytest.raises(PPFitError, match="error -3"):
        eng.scrunch_subints(np.zeros((1, 1, 2, 8200)), np.ones((1, 2)), np.zeros((1, 2)), 1, 2)
    (raw, scl, offs), rph, rw = raw_inputs(eng, 2, 2, 8, 64)
    with pytest.raises(PPFitError, match="error -1"):
        eng.scrunch_subints(RawSubints(raw, scl, offs, pmode=1), rw, rph, 3, 1)
    with pytest.raises(PPFitError):
        eng.scrunch_subints(RawSubints(raw, scl, offs, pmode=1), rw, rph, 1, 1, all_pols=True)
    # the C entry point itself
    lib, ctx = eng.lib, eng.ctx
    t = torch.zeros(2 * 8 * 64, dtype=torch.float64, device=eng.device)
    p = ctypes.c_void_p(t.data_ptr())
    assert lib.ppf_scrunch_subints(ctx, 1, 1, 8, 64, None, None, None, None, 1, 1, None, None) == -1
    assert lib.ppf_scrunch_subints(ctx, 1, 1, 8, 64, None, None, p, p, 1, 1, p, p) == -1  # no data
    for args in ((p, None, None, p, 1, 1, p, p), (p, None, p, None, 1, 1, p, p),
                 (p, None, p, p, 1, 1, None, p), (p, None, p, p, 1, 1, p, None)):
        assert lib.ppf_scrunch_subints(ctx, 1, 1, 8, 64, *args) == -1
    rd = _lib.RawSubintsDesc()
    rd.raw_type, rd.npol, rd.pmode, rd.ipol = _lib.RAW_I16, 1, 0, 0
    rd.raw = rd.scl = rd.offs = p
    assert lib.ppf_scrunch_subints(ctx, 1, 1, 8, 64, p, ctypes.byref(rd), p, p, 1, 1, p, p) == -1
    rd.raw = None
    assert lib.ppf_scrunch_subints(ctx, 1, 1, 8, 64, None, ctypes.byref(rd), p, p, 1, 1, p, p) == -1
    rd.raw = p
    rd.raw_type = _lib.RAW_U8  # unpack first
    assert lib.ppf_scrunch_subints(ctx, 1, 1, 8, 64, None, ctypes.byref(rd), p, p, 1, 1, p, p) == -3
    rd.raw_type, rd.ipol = _lib.RAW_I16, 1  # ipol outside the one stored polarisation
    assert lib.ppf_scrunch_subints(ctx, 1, 1, 8, 64, None, ctypes.byref(rd), p, p, 1, 1, p, p) == -1
    assert lib.ppf_scrunch_subints(ctx, 0, 1, 8, 64, p, None, p, p, 1, 1, p, p) == 0  # nothing to do
    eng.synchronize()


# ---------------------------------------------------------------------------
# file level
# ---------------------------------------------------------------------------
def within_half_step(got, want, scl):
    """test_gpu_ppalign_init.py's: a stored sample is within half its row's
    quantisation step of the value it was made from."""
    eps = np.finfo(np.float64).eps
    return (np.abs(got - want) <= 0.5 * scl[..., None] * (1 + 1e-9) + 4 * eps * np.abs(want)).all()


def stored_steps(name):
    from pulseportraiture_amd import psrfits
    f = psrfits.PSRFITSFile(name)
    scl = f.meta()["scl"]
    f.close()
    return scl


@pytest.fixture(scope="module")
def fake(eng, tmp_path_factory):
    """A dispersed 2 x 16 x 256 fake pulsar with weights 0, 1 and 2."""
    from pulseportraiture_amd import pplib, synth
    d = tmp_path_factory.mktemp("scrunch")
    par = d / "fake.par"
    par.write_text(PAR)
    nsub, nchan, nbin = 2, 16, 256
    w = np.ones((nsub, nchan))
    w[0, 2] = 0.0
    w[0, 5] = 2.0
    w[1, 8:12] = 0.0  # a whole group of four
    out = str(d / "fake.fits")
    pplib.make_fake_pulsar(synth.EXAMPLE_GMODEL, str(par), outfile=out, nsub=nsub, nchan=nchan,
                           nbin=nbin, noise_stds=0.01, dedispersed=False, weights=w, tsub=60.0,
                           seed=11, quiet=True)
    return out, w, str(d)


def test_scrunch_archive(eng, fake):
    import os
    from pulseportraiture_amd import archive, pplib
    name, w, d = fake
    out = os.path.join(d, "fake.f4b2.fits")
    assert pplib.scrunch_archive(name, out, nchan=4, nbin=128, quiet=True) == out
    src = archive.load_data(name, rm_baseline=False, quiet=True)
    assert src.subints.shape == (2, 1, 16, 256) and not src.dmc
    np.testing.assert_array_equal(src.weights, w)
    ref, rfreqs, rw = R.scrunch_bunch(src.subints, src.freqs, src.weights, src.Ps, src.DM,
                                      bool(src.dmc), 4, 128)
    got = archive.load_data(out, rm_baseline=False, quiet=True)
    assert got.subints.shape == (2, 1, 4, 128)
    assert (got.nsub, got.npol, got.nchan, got.nbin) == (2, 1, 4, 128)
    np.testing.assert_array_equal(got.freqs, rfreqs)
    np.testing.assert_array_equal(got.weights, rw)
    assert rw[1, 2] == 0.0 and rw[0, 0] == 3.0 and rw[0, 1] == 5.0
    assert not got.dmc and got.DM == src.DM
    np.testing.assert_array_equal(got.Ps, src.Ps)
    assert [e.as_tuple() for e in got.epochs] == [e.as_tuple() for e in src.epochs]
    assert np.abs(ref).max() > 0.1
    assert within_half_step(got.subints, ref, stored_steps(out))
    assert not got.subints[1, 0, 2].any()
    # the bunch itself, before it is quantised: the restatement at its bound
    b = archive.scrunch(name, nchan=4, nbin=128, rm_baseline=False)
    assert np.abs(b.subints - ref).max() <= 1e-12 * np.abs(ref).max()
    np.testing.assert_array_equal(b.freqs, rfreqs)
    np.testing.assert_array_equal(b.weights, rw)
    assert b.noise_stds.shape == (2, 1, 4) and b.SNRs.shape == (2, 1, 4)
    assert (b.noise_stds[b.weights[:, None] != 0] > 0).all()
    assert [list(c) for c in b.ok_ichans] == [[0, 1, 2, 3], [0, 1, 3]]
    with pytest.raises(ValueError):
        archive.scrunch(name, nchan=5)
    with pytest.raises(ValueError):
        archive.scrunch(name, nbin=100)


class Spy:
    """Records what Engine.scrunch_subints is given."""

    def __init__(self, monkeypatch, eng):
        self.kinds = []
        inner = type(eng).scrunch_subints

        def spy(this, data, *a, **kw):
            self.kinds.append(type(data).__name__)
            return inner(this, data, *a, **kw)
        monkeypatch.setattr(type(eng), "scrunch_subints", spy)


@pytest.mark.parametrize("npol,pscrunch", [(1, False), (4, False), (4, True)])
def test_file_route_reads_the_samples(eng, tmp_path, monkeypatch, npol, pscrunch):
    """archive.scrunch / scrunch_archive of a PSRFITS file that needs no
    processing hand the stored 16-bit samples to the device (RawSubints: no
    fp64 copy of the archive), to the bits of the loaded-fp64 route; a load
    that processes the data (baseline removal, tscrunch) takes the fp64
    route."""
    import os
    from pulseportraiture_amd import archive, pplib, synth
    par = tmp_path / "fake.par"
    par.write_text(PAR)
    name = str(tmp_path / "p.fits")
    w = np.ones((2, 16))
    w[0, 3] = 0.0
    w[1, 4:8] = 0.0
    pplib.make_fake_pulsar(synth.EXAMPLE_GMODEL, str(par), outfile=name, nsub=2, npol=npol,
                           nchan=16, nbin=256, noise_stds=0.01, dedispersed=False, weights=w,
                           tsub=60.0, seed=3, quiet=True)
    spy = Spy(monkeypatch, eng)
    got = archive.scrunch(name, nchan=4, nbin=128, rm_baseline=False, pscrunch=pscrunch)
    assert spy.kinds == ["RawSubints"]
    loaded = archive.load_data(name, rm_baseline=False, pscrunch=pscrunch, host=False, quiet=True)
    ref = archive.scrunch(loaded, nchan=4, nbin=128)
    assert spy.kinds == ["RawSubints", "Tensor"]
    npo = 1 if pscrunch else npol
    assert got.subints.shape == ref.subints.shape == (2, npo, 4, 128)
    assert np.abs(ref.subints).max() > 0.1
    for key in ("subints", "freqs", "weights", "noise_stds", "SNRs", "Ps"):
        np.testing.assert_array_equal(np.asarray(got[key]), np.asarray(ref[key]), err_msg=key)
    assert (got.npol, got.nchan, got.nbin, got.state) == (ref.npol, ref.nchan, ref.nbin, ref.state)
    # the file writer's route is the same one
    del spy.kinds[:]
    out = str(tmp_path / "p.scr.fits")
    pplib.scrunch_archive(name, out, nchan=4, nbin=128, quiet=True)
    assert spy.kinds == ["RawSubints"] and os.path.exists(out)
    # processing requests load fp64 values
    del spy.kinds[:]
    archive.scrunch(name, nchan=4)              # rm_baseline=True
    archive.scrunch(name, nchan=4, tscrunch=True, rm_baseline=False)
    assert spy.kinds == ["Tensor", "Tensor"]


def test_load_data_fscrunch(eng, fake):
    from pulseportraiture_amd import archive
    name, _, _ = fake
    a = archive.load_data(name, fscrunch=True, quiet=True)
    b = archive.scrunch(name, nchan=1)
    assert a.subints.shape == (2, 1, 1, 256) and a.nchan == 1
    for key in ("subints", "freqs", "weights", "noise_stds", "SNRs", "Ps"):
        np.testing.assert_array_equal(np.asarray(a[key]), np.asarray(b[key]), err_msg=key)
    src = archive.load_data(name, quiet=True)  # baseline removed, as both of them load
    ref, rfreqs, rw = R.scrunch_bunch(src.subints, src.freqs, src.weights, src.Ps, src.DM,
                                      bool(src.dmc), 1, 256)
    assert np.abs(a.subints - ref).max() <= 1e-12 * np.abs(ref).max()
    np.testing.assert_array_equal(a.freqs, rfreqs)
    np.testing.assert_array_equal(a.weights, rw)
    # tscrunch first, then every channel into one
    t = archive.scrunch(name, nchan=1, tscrunch=True)
    assert t.subints.shape == (1, 1, 1, 256)
    np.testing.assert_array_equal(t.weights, [[src.weights.sum()]])
