"""The host side of archive writing, no device: the streaming PSRFITS writer
(include/ppfitsw.h) read back by the package's reader and by an independent
numpy parse, the host fake-data helpers against the reference's own
(tests/golden/fake_pulsar.npz, made by make_golden_fake.py), and the numpy
restatement of the device quantiser (synth.quantize_host).  Readability by
PSRCHIVE is not checked (PSRCHIVE is absent): the layout follows the PSRFITS
definition the reader was written from."""
import re

import numpy as np
import pytest

from pulseportraiture_amd.mjd import MJD

BLOCK = 2880
WIDTH = {"A": 1, "I": 2, "J": 4, "E": 4, "D": 8}
EPHEMERIS = "PSR J1234+5678\nRAJ 12:34:00.0\nDECJ 56:78:00.0\nF0 345.67890123456789\nDM 34.56789\n"


@pytest.fixture(scope="module")
def lib():
    from pulseportraiture_amd import build
    build.build_fits()
    from pulseportraiture_amd import psrfits
    return psrfits


def parse_fits(blob):
    """Every HDU of a FITS file as (cards {key: value text}, data bytes),
    from the standard alone (80-character cards, 2880-byte blocks)."""
    hdus, off = [], 0
    while off < len(blob):
        cards, end = {}, False
        while not end:
            block = blob[off:off + BLOCK].decode("ascii")
            assert len(block) == BLOCK
            off += BLOCK
            for c in range(0, BLOCK, 80):
                card = block[c:c + 80]
                if card.startswith("END "):
                    end = True
                    break
                if card[8:10] == "= ":
                    v = card[10:]
                    m = re.match(r"\s*'((?:[^']|'')*)'", v)
                    cards[card[:8].strip()] = m.group(1).rstrip() if m else v.split("/")[0].strip()
        n = 0
        if int(cards["NAXIS"]):
            n = int(cards["NAXIS1"]) * int(cards["NAXIS2"])
        hdus.append((cards, blob[off:off + n]))
        off += (n + BLOCK - 1) // BLOCK * BLOCK
    return hdus


def columns(cards):
    """[(name, repeat, letter, byte offset)] of a binary table header."""
    out, off = [], 0
    for i in range(1, int(cards["TFIELDS"]) + 1):
        m = re.fullmatch(r"(\d+)([A-Z])", cards["TFORM%d" % i])
        rep, t = int(m.group(1)), m.group(2)
        out.append((cards["TTYPE%d" % i], rep, t, off))
        off += rep * WIDTH[t]
    return out, off


@pytest.mark.parametrize("shape", [(3, 1, 5, 64), (2, 4, 3, 100)])
def test_writer_roundtrip(lib, tmp_path, shape):
    nsub, npol, nchan, nbin = shape
    rng = np.random.default_rng(sum(shape))
    raw = rng.integers(-32767, 32768, size=shape).astype(np.int16)
    raw[0, 0, 0, :4] = [-32767, 32767, 0, -1]
    scl = rng.uniform(1e-3, 2.0, size=shape[:3]).astype(np.float32).astype(np.float64)
    offs = rng.normal(size=shape[:3]).astype(np.float32).astype(np.float64)
    freqs = np.tile(np.linspace(1100.0, 1900.0, nchan), (nsub, 1)) + 0.1 * rng.random((nsub, nchan))
    wts = rng.integers(0, 2, size=(nsub, nchan)).astype(np.float64)
    tsub = np.array([10.0, 10.0, 9.5])[:nsub]
    offs_sub = np.array([5.0, 15.0, 24.75])[:nsub]
    period = np.array([0.003, 0.0030001, 0.0030002])[:nsub]
    par_ang = np.array([10.5, 11.0, 11.5])[:nsub]
    path = str(tmp_path / "w.fits")
    state = "Stokes" if npol == 4 else "Intensity"
    w = lib.PSRFITSWriter(path, npol, nchan, nbin, MJD(57300, 43200, 0.25), 1500.0, 800.0,
                          DM=34.56789, dedispersed=True, state=state, telescope="GBT",
                          source="J1234+5678", ra="12:34:00.0", dec="+56:78:00.0",
                          ephemeris=EPHEMERIS)
    for lo, hi in ((0, 1), (1, nsub)):  # two chunks
        w.write(raw[lo:hi], scl[lo:hi], offs[lo:hi], freqs[lo:hi], wts[lo:hi], tsub[lo:hi],
                offs_sub[lo:hi], period[lo:hi], par_ang[lo:hi])
    with pytest.raises(lib.PSRFITSError):  # a wrong shape is refused before the C call
        w.write(raw[:1, :, :, :-1], scl[:1], offs[:1], freqs[:1], wts[:1], tsub[:1], offs_sub[:1],
                period[:1])
    w.close()

    # the package's reader
    f = lib.PSRFITSFile(path)
    I = f.info
    assert (f.nsub, f.npol, f.nchan, f.nbin) == shape
    assert I.raw_type == 2 and I.has_period and I.has_par_ang and I.dedispersed == 1
    assert I.dm == 34.56789 and I.chan_dm == 34.56789
    assert f.text("source") == "J1234+5678" and f.text("telescope") == "GBT"
    assert f.text("obs_mode") == "PSR"
    assert f.text("pol_type") == ("IQUV" if npol == 4 else "AA+BB")
    assert (I.stt_imjd, I.stt_smjd, I.stt_offs) == (57300, 43200, 0.25)
    assert (I.obsfreq, I.obsbw, I.chan_bw) == (1500.0, 800.0, 800.0 / nchan)
    m = f.meta()
    for key, want in (("freqs", freqs), ("weights", wts), ("scl", scl), ("offs", offs),
                      ("tsubint", tsub), ("offs_sub", offs_sub), ("period", period),
                      ("par_ang", par_ang)):
        np.testing.assert_array_equal(m[key], want, err_msg=key)
    np.testing.assert_array_equal(f.raw(), raw)
    assert f.polyco() is None
    f.close()

    # an independent parse
    blob = open(path, "rb").read()
    assert len(blob) % BLOCK == 0
    hdus = parse_fits(blob)
    prim = hdus[0][0]
    assert prim["SIMPLE"] == "T" and prim["FITSTYPE"] == "PSRFITS" and prim["OBS_MODE"] == "PSR"
    assert prim["HDRVER"] and prim["RA"] == "12:34:00.0" and prim["DEC"] == "+56:78:00.0"
    by_name = {c["EXTNAME"]: (c, d) for c, d in hdus[1:]}
    assert set(by_name) == {"HISTORY", "PSRPARAM", "SUBINT"}
    for c, d in by_name.values():
        assert c["XTENSION"] == "BINTABLE"
        assert int(c["NAXIS1"]) == columns(c)[1]
        assert len(d) == int(c["NAXIS1"]) * int(c["NAXIS2"])
    c, d = by_name["PSRPARAM"]
    lines = [d[i:i + 128].decode().rstrip() for i in range(0, len(d), 128)]
    assert lines == EPHEMERIS.splitlines()
    c, d = by_name["HISTORY"]
    cols, row = columns(c)
    last = d[-row:]
    get = {n: (t, o) for n, _, t, o in cols}
    assert int.from_bytes(last[get["DEDISP"][1]:][:2], "big", signed=True) == 1
    assert int.from_bytes(last[get["NSUB"][1]:][:4], "big", signed=True) == nsub
    c, d = by_name["SUBINT"]
    assert int(c["NAXIS2"]) == nsub
    assert (int(c["NPOL"]), int(c["NCHAN"]), int(c["NBIN"])) == (npol, nchan, nbin)
    assert float(c["DM"]) == 34.56789 and float(c["CHAN_BW"]) == 800.0 / nchan
    cols, row = columns(c)
    name, rep, t, o = cols[-1]
    assert (name, rep, t) == ("DATA", npol * nchan * nbin, "I")
    assert c["TDIM%d" % len(cols)] == "(%d,%d,%d)" % (nbin, nchan, npol)
    rows = np.frombuffer(d, dtype=np.uint8).reshape(nsub, row)
    data = rows[:, o:o + 2 * rep].copy().view(">i2").reshape(shape)  # big-endian on disk
    np.testing.assert_array_equal(data, raw)
    got = {n: rows[:, o:o + r * WIDTH[t]].copy().view(">f%d" % WIDTH[t]) for n, r, t, o in cols[:-1]}
    np.testing.assert_array_equal(got["DAT_SCL"].reshape(shape[:3]), scl)
    np.testing.assert_array_equal(got["DAT_FREQ"], freqs)
    np.testing.assert_array_equal(got["OFFS_SUB"][:, 0], offs_sub)


def test_writer_errors(lib, tmp_path):
    with pytest.raises(lib.PSRFITSError):
        lib.PSRFITSWriter(str(tmp_path / "no" / "dir.fits"), 1, 2, 16, MJD(50000.0), 1500.0, 800.0)
    w = lib.PSRFITSWriter(str(tmp_path / "e.fits"), 1, 2, 16, MJD(50000.0), 1500.0, 800.0)
    z = np.zeros((1, 1, 2, 16), np.int16)
    one = np.ones((1, 1, 2))
    w.write(z, one, one, np.ones((1, 2)), np.ones((1, 2)), [1.0], [0.5], [0.01])
    w.nsub = 5  # out of order
    with pytest.raises(lib.PSRFITSError, match="in order"):
        w.write(z, one, one, np.ones((1, 2)), np.ones((1, 2)), [1.0], [1.5], [0.01])
    w.close(check=False)


def test_fake_helpers_match_reference(golden):
    """add_DM_nu and add_scintillation against the reference's own, stage by
    stage on the golden 8 x 64 portrait, to 1e-12 of the portrait's maximum."""
    from pulseportraiture_amd import pplib
    g = golden("fake_pulsar.npz")
    tol = 1e-12 * np.abs(g["port"]).max()
    dmnu = pplib.add_DM_nu(g["model"], -float(g["phase"]), -float(g["dDM"]), float(g["P"]),
                           g["freqs"], list(g["xs"]), list(g["Cs"]), np.inf)
    assert np.abs(dmnu - g["dmnu"]).max() <= tol
    port = pplib.add_scintillation(g["scat"], list(g["scint"]))
    assert np.abs(port - g["port"]).max() <= tol
    # defaults: one nu**-2 term is rotate_portrait's dispersion law
    k = np.arange(33)
    rot = 0.01 + pplib.Dconst * 1e-3 / float(g["P"]) * (g["freqs"] ** -2.0 - 1500.0 ** -2.0)
    want = np.fft.irfft(np.fft.rfft(g["model"], axis=1) * np.exp(2j * np.pi * rot[:, None] * k), 64)
    got = pplib.add_DM_nu(g["model"], 0.01, 1e-3, float(g["P"]), g["freqs"], nu_ref=1500.0)
    assert np.abs(got - want).max() <= tol
    assert pplib.add_scintillation(g["scat"], None, random=False) is not None
    rng = np.random.default_rng(3)
    a = pplib.add_scintillation(g["scat"], nsin=3, rng=rng)
    assert a.shape == g["scat"].shape and np.isfinite(a).all()


def edge_rows(nbin):
    """Rows on which a quantiser can go wrong (also the device test's)."""
    rng = np.random.default_rng(nbin)
    j = np.arange(nbin)
    rows = [np.full(nbin, 3.25),                       # constant
            np.zeros(nbin),                            # all zero
            np.full(nbin, 0.1),                        # constant, not a float32
            1000.0 + rng.random(nbin),                 # DC 1000, range 1
            -5.0 - 3.0 * rng.random(nbin),             # negative only
            rng.normal(size=nbin),
            1e-3 * rng.normal(size=nbin) + 1e6,        # large offset, small range
            1e30 * rng.normal(size=nbin),
            1e-30 * rng.normal(size=nbin),
            np.where(j == 0, 9.0, np.sin(j)),          # extreme in bin 0
            np.where(j == nbin - 1, -9.0, np.sin(j)),  # extreme in the last bin
            np.where(j == (3 * nbin) // 4 + 1, 50.0, rng.random(nbin)),  # maximum in a later wave's slice
            np.where(j == nbin // 2, -50.0, rng.random(nbin))]
    return np.array(rows)


@pytest.mark.parametrize("nbin", [16, 64, 100, 2048])
def test_host_quantiser_bound(nbin):
    """|raw| <= 32767 and |raw scl + offs - x| <= scl / 2 (1 + 1e-9) + 4 eps |x|:
    half a step of the rounding, plus the fp64 rounding of x - offs and of the
    quotient; scl and offs are float32 values."""
    from pulseportraiture_amd.synth import quantize_host
    x = edge_rows(nbin)
    raw, scl, offs = quantize_host(x)
    assert raw.dtype == np.int16 and np.abs(raw.astype(np.int64)).max() <= 32767
    np.testing.assert_array_equal(scl, scl.astype(np.float32).astype(np.float64))
    np.testing.assert_array_equal(offs, offs.astype(np.float32).astype(np.float64))
    assert (scl > 0).all()
    eps = np.finfo(np.float64).eps
    err = np.abs(raw * scl[:, None] + offs[:, None] - x)
    assert (err <= 0.5 * scl[:, None] * (1 + 1e-9) + 4 * eps * np.abs(x)).all()
    # constant rows: scl 1, offs float32(value), raw 0
    np.testing.assert_array_equal(scl[:3], 1.0)
    np.testing.assert_array_equal(offs[:3], np.float32([3.25, 0.0, 0.1]).astype(np.float64))
    assert not raw[:3].any()
    # the full range is used: the larger extreme reaches +-32767
    assert (np.abs(raw[3:].astype(np.int64)).max(axis=1) == 32767).all()
    with pytest.raises(ValueError):
        quantize_host(np.array([[0.0, np.nan]]))
