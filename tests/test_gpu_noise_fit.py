"""get_noise(method="fit") on the device: Engine.noise_fit_rows / find_kc_rows
/ noise_rows(frac) and the pplib functions over them, against the reference's
fixtures (tests/golden/noise_fit.npz, tests/golden/make_golden_noise_fit.py),
and the default_noise_method switch through load_data and the fit wrappers.

kc is compared on `separated` rows only (the two best per-a minima differ by
more than 1e-9, or tie exactly on the b = 0 plane): all 60 fixture rows are.
Noise is held to 1e-9 relative where kc agrees: the tail power of a
transformed row carries about eps log2(nbin) (peak S/N) of rounding, at most
3e-12 at S/N 1000 and nbin 2048, so three orders of margin.  Measured on an
MI355X: the largest relative noise difference over the fixture rows is
1.6e-13 (nbin 16; 2.4e-14 at nbin 250, at most 2.2e-15 at the powers of two),
the fact 1.1 and fact 2 columns alike, and no kc differs.
"""
import os

import numpy as np
import pytest

from tests import noise_fit_reference as R
from tests.conftest import GOLDEN
from tests.psrfits_writer import quantize, write_psrfits

pytestmark = pytest.mark.gpu

NBINS = (16, 64, 250, 256, 2048)  # 16 and 250: the any-nbin kernel
TOL = 1e-9
NS = R.NS


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from pulseportraiture_amd.engine import get_engine
    return get_engine(0)


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "noise_fit.npz"), allow_pickle=False)


@pytest.fixture
def fit_method():
    """default_noise_method = "fit" for one test, restored after it."""
    from pulseportraiture_amd import pplib
    old = pplib.default_noise_method
    pplib.default_noise_method = "fit"
    yield pplib
    pplib.default_noise_method = old


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)) / np.abs(np.asarray(b))


@pytest.mark.parametrize("nbin", NBINS)
def test_noise_fit_rows_vs_reference(gpu, fx, nbin):
    rows, sep = fx["rows_%d" % nbin], fx["separated_%d" % nbin]
    noise, kc, idx = [t.cpu().numpy() for t in gpu.noise_fit_rows(rows, full=True)]
    ref_kc, ref_idx = fx["kc_%d" % nbin], fx["idx_%d" % nbin]
    print("nbin", nbin, "kc", kc.tolist(), "ref", ref_kc.tolist())
    assert sep.sum() >= 0.9 * len(sep)
    assert np.array_equal(kc[sep], ref_kc[sep])
    same = kc == ref_kc
    err = _rel(noise[same], fx["noise_chans_%d" % nbin][same])
    print("max relative noise difference", err.max())
    assert err.max() <= TOL
    # only the winning a reaches the result; on separated rows it is the reference's
    assert np.array_equal(idx[sep] // (NS * NS), ref_idx[sep] // (NS * NS))
    # rows with no slope tie exactly on the b = 0 plane: the lowest index (ia = 0) wins
    flat = (ref_idx // NS) % NS == 0
    if nbin != 64:
        assert flat.any()
    assert np.all(idx[flat] // NS == 0)
    noise2 = gpu.noise_fit_rows(rows, fact=2.0).cpu().numpy()
    err2 = _rel(noise2[same], fx["noise_fact2_%d" % nbin][same])
    print("max relative noise difference, fact 2", err2.max())
    assert err2.max() <= TOL
    assert np.array_equal(gpu.noise_fit_rows(rows).cpu().numpy(), noise)  # full=False


def test_find_kc_rows_half_tri_and_weights(gpu, fx):
    from pulseportraiture_amd import pplib
    for i in range(int(fx["n_spectra"])):
        p, e = fx["ht_pows_%d" % i], fx["w_errs_%d" % i]
        for errs, fn, pre in ((None, "half_tri", "ht"), (e, "exp_dc", "w"), (e, "half_tri", "w_ht")):
            ref_idx = int(fx[pre + "_idx_%d" % i])
            assert R.separated(fx[pre + "_per_a_%d" % i], ref_idx), (i, pre)
            kc, idx = [int(t.cpu().numpy()) for t in gpu.find_kc_rows(p, errs=errs, fn=fn)]
            assert kc == int(fx[pre + "_kc_%d" % i]), (i, pre)
            assert idx // (NS * NS) == ref_idx // (NS * NS), (i, pre)
            got = pplib.find_kc(p, errs=1.0 if errs is None else errs, fn=fn)
            assert type(got) is int and got == kc
        # a scalar errs changes no minimum
        assert pplib.find_kc(p, errs=3.0) == pplib.find_kc(p)
    # several spectra in one call (the 2-D extension), and through get_noise_fit's spectrum
    rows = fx["rows_256"]
    pows = np.array([R.power_spectrum(r) for r in rows])
    kcs = pplib.find_kc(pows)
    assert kcs.shape == (len(rows),) and np.array_equal(kcs, fx["kc_256"])
    # floor(a) of the last half_tri grid value, 19 * ((n - 1) / 19) + 1 with each
    # operation rounded, is n - 1 at n = 54, 88 and 232 and n at the others: a
    # descending line over the whole spectrum wins there
    for n, want_kc in ((54, 53), (88, 87), (100, 100), (129, 129), (232, 231), (8193, 8193)):
        line = 10.0 ** np.linspace(3.0, 0.0, n)
        kc, idx = [int(t.cpu().numpy()) for t in gpu.find_kc_rows(line, fn="half_tri")]
        want = R.find_kc(line, fn="half_tri", how="factorised", full=True)
        assert R.separated(want[2], want[1]) and want[0] == want_kc
        assert idx // (NS * NS) == want[1] // (NS * NS) == NS - 1 and kc == want_kc, (n, kc)


@pytest.mark.parametrize("nbin", (64, 250))
def test_zero_power_rows(gpu, fx, nbin):
    """A zero power is log10 = -inf: the objective is NaN at flat index 0, which
    numpy.argmin returns; a = 1/n never decays to 0.005, so kc = NH - 1 and
    k_crit = fact kc is clamped to int(0.99 NH)."""
    NH = nbin // 2 + 1
    # integer samples with a zero sum: the DC power is exactly zero on the device too
    rng = np.random.default_rng(nbin)
    row = np.rint(8.0 * rng.standard_normal(nbin) + 200.0 * np.exp(
        -0.5 * ((np.arange(nbin) - nbin / 2) / 3.0) ** 2))
    row[0] -= row.sum()
    assert row.sum() == 0.0
    both = np.stack([np.zeros(nbin), row])
    noise, kc, idx = [t.cpu().numpy() for t in gpu.noise_fit_rows(both, full=True)]
    assert kc.tolist() == [NH - 1, NH - 1] and idx.tolist() == [0, 0]
    assert noise[0] == 0.0
    pows = R.power_spectrum(row)
    want, k_crit = R.noise_from_kc(pows, NH - 1)
    assert k_crit == int(0.99 * NH)
    assert abs(noise[1] - want) <= TOL * want
    if nbin == 64:
        assert int(fx["zero_kc"]) == NH - 1 and float(fx["zero_noise"]) == 0.0
    zdc = fx["zero_dc_pows"]
    kc, idx = [int(t.cpu().numpy()) for t in gpu.find_kc_rows(zdc)]
    assert (kc, idx) == (len(zdc) - 1, 0) and kc == int(fx["zero_dc_kc"])
    # a negative or NaN power goes the same way
    for v in (-1.0, np.nan, np.inf):
        bad = zdc.copy()
        bad[5] = v
        assert [int(t.cpu().numpy()) for t in gpu.find_kc_rows(bad)] == [len(zdc) - 1, 0]


@pytest.mark.parametrize("nbin", (250, 256, 2048))
def test_rows_do_not_depend_on_the_call(gpu, fx, nbin):
    """A row's noise, kc and index are bitwise the same alone, inside a 37-row
    call and across two calls."""
    rows = fx["rows_%d" % nbin]
    big = np.tile(rows, (4, 1))[:37]
    a = [t.cpu().numpy() for t in gpu.noise_fit_rows(big, full=True)]
    b = [t.cpu().numpy() for t in gpu.noise_fit_rows(big, full=True)]
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    for r in (0, 5, 11, 36):
        one = [t.cpu().numpy() for t in gpu.noise_fit_rows(big[r:r + 1], full=True)]
        for x, y in zip(one, a):
            assert x[0] == y[r] and x.dtype == y.dtype
    assert a[0].dtype == np.float64 and a[1].dtype == np.int32 and a[2].dtype == np.int32


def test_pplib_functions_vs_reference(gpu, fx):
    from pulseportraiture_amd import pplib
    for nbin in NBINS:
        rows = fx["rows_%d" % nbin]
        same = np.array_equal(gpu.noise_fit_rows(rows, full=True)[1].cpu().numpy(),
                              fx["kc_%d" % nbin])
        assert same
        got = pplib.get_noise_fit(rows, chans=True)
        assert got.shape == (len(rows),) and _rel(got, fx["noise_chans_%d" % nbin]).max() <= TOL
        assert np.array_equal(pplib.get_noise(rows, method="fit", chans=True), got)
        one = pplib.get_noise(rows[3], method="fit")
        assert type(one) is float and abs(one - fx["noise_%d" % nbin][3]) <= TOL * one
        for frac in (2, 8):
            ps = pplib.get_noise_PS(rows, frac=frac, chans=True)
            assert _rel(ps, fx["ps%d_%d" % (frac, nbin)]).max() <= TOL, (nbin, frac)
        assert np.array_equal(pplib.get_noise_PS(rows, frac=4, chans=True),
                              pplib.get_noise_PS(rows, chans=True))
        assert np.array_equal(gpu.noise_rows(rows, frac=4.0).cpu().numpy(),
                              gpu.noise_rows(rows).cpu().numpy())
    port = fx["port"]
    for got, key in ((pplib.get_noise_fit(port), "port_noise_fit"),
                     (pplib.get_noise_PS(port, frac=2), "port_noise_ps2"),
                     (pplib.get_noise_PS(port, frac=8), "port_noise_ps8")):
        assert type(got) is float and abs(got - float(fx[key])) <= TOL * got, key
    assert _rel(pplib.get_noise_fit(port, chans=True), fx["port_noise_fit_chans"]).max() <= TOL
    for i in range(int(fx["n_snr"])):
        prof = fx["snr_prof_%d" % i]
        assert abs(pplib.get_SNR(prof) - float(fx["snr_%d" % i])) <= TOL * abs(float(fx["snr_%d" % i]))
        assert abs(pplib.get_SNR(prof, fudge=1.0) - float(fx["snr_fudge1_%d" % i])) <= \
            TOL * abs(float(fx["snr_fudge1_%d" % i]))


def test_argument_checks(gpu, fx):
    from pulseportraiture_amd.engine import PPFitError
    rows = fx["rows_64"]
    for bad in (0.0, -1.0, np.nan):
        with pytest.raises(PPFitError):
            gpu.noise_fit_rows(rows, fact=bad)
    for bad in (1.0, 0.5, np.nan):
        with pytest.raises(PPFitError):
            gpu.noise_rows(rows, frac=bad)
    with pytest.raises(PPFitError):
        gpu.noise_fit_rows(np.ones((2, 8)))
    with pytest.raises(PPFitError):
        gpu.find_kc_rows(np.ones((2, 3)))
    with pytest.raises(PPFitError):
        gpu.find_kc_rows(np.ones((1, 8194)))
    with pytest.raises(ValueError):
        gpu.find_kc_rows(np.ones((2, 16)), fn="triangle")
    with pytest.raises(ValueError):
        gpu.find_kc_rows(np.ones((2, 16)), errs=np.ones(15))


def _archive(path, nsub=3, nchan=8, nbin=64):
    from pulseportraiture_amd import synth
    w = synth.make_workload(nsub, nchan, nbin, seed=21)
    raw, scl, offs = quantize(synth.workload_data_host(w)[:, None])
    write_psrfits(path, raw, scl, offs, np.tile(w.freqs, (nsub, 1)),
                  np.ones((nsub, nchan), np.float32), tsubint=[30.0] * nsub,
                  offs_sub=15.0 + 30.0 * np.arange(nsub), period=[w.P] * nsub)
    return w


def test_default_noise_method_reaches_load_data(gpu, tmp_path, fit_method):
    from pulseportraiture_amd import archive, pplib
    path = str(tmp_path / "nf.fits")
    _archive(path)
    d = archive.load_data(path, rm_baseline=False, quiet=True)
    sub = np.asarray(d.subints)
    assert sub.shape == (3, 1, 8, 64)
    fit = gpu.noise_fit_rows(sub).cpu().numpy()
    assert np.array_equal(np.asarray(d.noise_stds), fit)
    pplib.default_noise_method = "PS"
    d = archive.load_data(path, rm_baseline=False, quiet=True)
    ps = gpu.noise_rows(sub).cpu().numpy()
    assert np.array_equal(np.asarray(d.noise_stds), ps)
    assert not np.array_equal(ps, fit)


def test_default_noise_method_reaches_the_fits(gpu, fit_method):
    from pulseportraiture_amd import pplib, pptoaslib, synth
    w = synth.make_workload(1, 8, 64, seed=22)
    port = synth.workload_data_host(w)[0]
    nu = pplib.guess_fit_freq(w.freqs)
    args = (port, w.model, [0.0, w.DM0, 0.0, 0.0, 0.0], w.P, w.freqs, [nu] * 3, [None] * 3)
    kw = dict(fit_flags=[1, 1, 0, 0, 0], log10_tau=False)
    keys = ("params", "param_errs", "scales", "scale_errs", "chi2", "red_chi2", "snr",
            "channel_snrs", "covariance_matrix")

    def same(a, b):
        return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in keys)

    auto = pptoaslib.fit_portrait_full(*args, None, **kw)
    given = pptoaslib.fit_portrait_full(*args, pplib.get_noise_fit(port, chans=True), **kw)
    assert same(auto, given)
    batch = pptoaslib.fit_portraits_batch(port[None], w.model, args[2], w.P, w.freqs,
                                          nu_fits=[nu] * 3, fit_flags=[1, 1, 0, 0, 0])
    assert np.array_equal(batch["errs"][0], pplib.get_noise_fit(port, chans=True))
    legacy = pplib.fit_portrait(port, w.model, [0.0, w.DM0], w.P, w.freqs, nu, None, None)
    legacy_given = pplib.fit_portrait(port, w.model, [0.0, w.DM0], w.P, w.freqs, nu, None,
                                      pplib.get_noise_fit(port, chans=True))
    for k in ("phase", "phase_err", "DM", "DM_err", "chi2", "snr"):
        assert legacy[k] == legacy_given[k], k
    prof, tmpl = port.mean(axis=0), w.model.mean(axis=0)
    ps_auto = pplib.fit_phase_shift(prof, tmpl)
    ps_given = pplib.fit_phase_shift(prof, tmpl, noise=pplib.get_noise_fit(prof))
    for k in ("phase", "phase_err", "scale", "scale_err", "snr", "red_chi2"):
        assert ps_auto[k] == ps_given[k], k
    # "PS" again: the wrappers leave errs to the fit kernels, as before the switch existed
    pplib.default_noise_method = "PS"
    ps = pptoaslib.fit_portrait_full(*args, None, **kw)
    ps_errs = pptoaslib.fit_portrait_full(*args, pplib.get_noise_PS(port, chans=True), **kw)
    assert not same(ps, auto)
    for k, e in (("phi", "phi_err"), ("DM", "DM_err")):
        assert abs(ps[k] - ps_errs[k]) <= 1e-6 * ps[e], k
    batch = pptoaslib.fit_portraits_batch(port[None], w.model, args[2], w.P, w.freqs,
                                          nu_fits=[nu] * 3, fit_flags=[1, 1, 0, 0, 0])
    np.testing.assert_allclose(batch["errs"][0], pplib.get_noise_PS(port, chans=True), rtol=1e-12)
    ps_shift = pplib.fit_phase_shift(prof, tmpl)
    assert ps_shift["phase_err"] != ps_auto["phase_err"]


def test_default_noise_method_reaches_get_toas(gpu, fit_method):
    """An archive without noise_stds: GetTOAs' fits estimate their own errs, by
    the fitted noise floor under "fit" -- the same TOAs as the archive that
    carries get_noise_fit's noise_stds -- and by "PS" otherwise."""
    from pulseportraiture_amd import archive, pplib, pptoas, synth
    from tests.golden_consts import DM0
    nsub, nchan, nbin = 3, 8, 64
    w = synth.make_workload(nsub, nchan, nbin, seed=23)
    data = synth.workload_data_host(w)
    b = dict(subints=data[:, None], freqs=w.freqs, Ps=np.full(nsub, w.P),
             epochs=[(57100 + k, 0, 0.0) for k in range(nsub)], DM=DM0, nu0=1500.0,
             weights=np.ones((nsub, nchan)))
    archive.register_archive("nf_bare", b)
    archive.register_archive("nf_given", dict(
        b, noise_stds=gpu.noise_fit_rows(data[:, None]).cpu().numpy()))

    def toas(name):
        gt = pptoas.GetTOAs([name], synth.EXAMPLE_GMODEL, quiet=True)
        gt.get_TOAs(quiet=True)
        return [np.asarray(v[0]) for v in (gt.phis, gt.phi_errs, gt.DMs, gt.DM_errs)]

    bare, given = toas("nf_bare"), toas("nf_given")
    for x, y in zip(bare, given):
        assert np.array_equal(x, y)
    pplib.default_noise_method = "PS"
    ps = toas("nf_bare")
    assert not np.array_equal(ps[1], bare[1])
