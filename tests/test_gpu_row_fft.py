"""The mixed-radix row FFT (RowSmooth, csrc/ppfit_rowfft.hpp and
ppfit_smoothfft.hpp): even nbin with nbin / 2 = 2^a 3^b 5^c that are no power
of two from 64 up.

- the row entry points at the smallest lengths at which a pass structure can
  go wrong (one radix only, odd N, fewer points than a wave, exactly one block
  of butterflies, the top of each size class) and at realistic ones, under
  the assertions and bars of test_gpu_generic_nbin.test_row_entry_points_generic,
  plus the row rotations and the noiseless generator against numpy at 1e-12 of
  the row scale;
- option row_fft 1 (this FFT) against 0 (the direct sums and the DFT on the
  matrix cores): two implementations of one definition, within 2e-12 of the
  row scale, twice the single-path bar;
- powers of two are not touched by the option (byte-identical);
- the project's reproducibility contract: a row alone or in a batch, a fit
  alone, in a batch, chunked by a 1-byte workspace limit, with and without
  the data-spectrum cache -- bitwise;
- the fit against the oracle at the bars of test_gpu_generic_nbin, and against
  the reference's own results (tests/golden/generic_nbin.npz) with no subint
  excluded, under either value of the option;
- the wide-channel path (per-channel tables in HBM) fed by the new data pass.
"""
import contextlib
import os

import numpy as np
import pytest

from oracle import ppfit_oracle as O
from pulseportraiture_amd import synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# nbin: why (N = nbin / 2)
NBINS = [
    18,    # N = 9: radix-3 only, fewer points than a wave
    20,    # N = 10: 2 * 5
    24,    # N = 12: 4 * 3
    30,    # N = 15: odd N, no radix-2 pass
    50,    # N = 25
    162,   # N = 81 = 3^4
    250,   # N = 125 = 5^3
    1000,  # a realistic length
    1536,  # N = 768: a radix-3 pass of exactly one block of butterflies
    2560,  # N = 1280: radix-5, one block of butterflies per chunk
    2000, 3000,  # realistic lengths
    7290,  # N = 3645: odd, radices 3 and 5 only, near the top
    8100,  # N = 4050: all radices, the largest class
    8000,  # a realistic length near the top
]
FIT_KEYS = ["params", "param_errs", "nu_out", "cov", "scales", "red_chi2", "snr", "nfev",
            "status", "errs"]


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from pulseportraiture_amd.engine import Engine
    return Engine(0)


@contextlib.contextmanager
def row_fft(eng, value):
    old = eng.get_option("row_fft")
    eng.set_option("row_fft", value)
    try:
        yield
    finally:
        eng.set_option("row_fft", old)


# ---------------------------------------------------------------------------
# the row entry points
# ---------------------------------------------------------------------------
_INPUTS, _REFS = {}, {}


def _inputs(nbin):
    """Six rows of a seeded workload and the arguments of every entry point."""
    if nbin not in _INPUTS:
        w = synth.make_workload(1, 6, nbin, seed=830 + nbin)
        data = synth.workload_data_host(w)[0]
        ph = np.linspace(-0.3, 0.4, 6)
        _INPUTS[nbin] = dict(
            data=data, model=w.model, spec=np.fft.rfft(data, axis=-1), ph=ph,
            tau=np.linspace(0.0, 2e-3, 6), tau_rot=np.linspace(0.0, 3.0, 6),
            sc=np.linspace(0.9, 1.1, 6), errs=np.full(6, 1.5),
            d3=np.stack([data, 0.5 * data[::-1]]), phs=np.stack([ph, -ph]),
            wts=np.array([[1.0] * 6, [0.5, 0.0, 1.0, 2.0, 1.0, 1.0]]))
    return _INPUTS[nbin]


def _refs(nbin):
    """numpy / the oracle, once per length."""
    if nbin not in _REFS:
        a = _inputs(nbin)
        k = np.arange(nbin // 2 + 1)
        data, spec, ph = a["data"], a["spec"], a["ph"]
        rot = np.fft.irfft(spec * np.exp(2j * np.pi * np.outer(ph, k)), n=nbin, axis=-1)
        msc = np.fft.irfft(np.fft.rfft(a["model"], axis=-1) /
                           (1 + 2j * np.pi * np.outer(a["tau"], k)), n=nbin, axis=-1)
        _REFS[nbin] = dict(
            noise=O.get_noise_PS(data, chans=True),
            irfft=np.fft.irfft(spec, n=nbin, axis=-1),
            shift=[O.fit_phase_shift(data[i], a["model"][i]) for i in range(6)],
            chi2=np.sum((rot - a["sc"][:, None] * msc) ** 2, axis=-1) / a["errs"] ** 2 / 100.0,
            accum=np.sum(a["wts"][..., None] * np.fft.rfft(a["d3"], axis=-1) *
                         np.exp(2j * np.pi * a["phs"][..., None] * k), axis=0),
            rotate=rot,
            scatter=np.fft.irfft(spec * np.exp(2j * np.pi * np.outer(ph, k)) /
                                 (1 + 2j * np.pi * np.outer(a["tau_rot"], k)), n=nbin, axis=-1),
            synth=np.fft.irfft(np.fft.rfft(a["model"], axis=-1) *
                               np.exp(2j * np.pi * a["phs"][..., None] * k), n=nbin, axis=-1))
    return _REFS[nbin]


def _row_outputs(eng, nbin):
    import torch
    a = _inputs(nbin)
    out = dict(
        noise=eng.noise_rows(a["data"]).cpu().numpy(),
        irfft=eng.irfft_rows(a["spec"], nbin).cpu().numpy(),
        shift=eng.phase_shift_batch(a["data"], a["model"], model_idx=np.arange(6)).cpu().numpy(),
        chi2=eng.resid_chi2_rows(a["data"], a["ph"], a["model"], a["sc"], a["errs"], 100.0,
                                 tau=a["tau"]).cpu().numpy(),
        rotate=eng.rotate_rows(a["data"], a["ph"]).cpu().numpy(),
        scatter=eng.scatter_rotate_rows(a["data"], a["ph"], a["tau_rot"]).cpu().numpy(),
        synth=eng.synth(a["model"], a["phs"], 0.0, 4321).cpu().numpy())
    acc = torch.zeros(6, nbin // 2 + 1, 2, dtype=torch.float64, device=eng.device)
    eng.rotate_accumulate(a["d3"], a["phs"], a["wts"], acc)
    torch.cuda.synchronize()
    got = acc.cpu().numpy()
    out["accum"] = got[..., 0] + 1j * got[..., 1]
    return out


@pytest.mark.parametrize("nbin", NBINS)
def test_row_entry_points_smooth(eng, nbin):
    assert eng.get_option("row_fft") == 1
    assert eng.row_transform(nbin) == "smooth"
    a, ref, got = _inputs(nbin), _refs(nbin), _row_outputs(eng, nbin)
    np.testing.assert_allclose(got["noise"], ref["noise"], rtol=1e-10)
    np.testing.assert_allclose(got["irfft"], ref["irfft"], rtol=0,
                               atol=1e-12 * np.abs(a["data"]).max())
    for i, r in enumerate(ref["shift"]):
        d = abs(got["shift"][i, 0] - r.phase)
        assert min(d, 1.0 - d) <= 1e-3 * r.phase_err, i
        np.testing.assert_allclose(got["shift"][i, 1:], [r.phase_err, r.scale, r.scale_err, r.snr,
                                                         r.red_chi2], rtol=1e-6)
    np.testing.assert_allclose(got["chi2"], ref["chi2"], rtol=1e-9)
    np.testing.assert_allclose(got["accum"], ref["accum"], rtol=0,
                               atol=1e-12 * np.abs(ref["accum"]).max())
    for name in ("rotate", "scatter", "synth"):
        np.testing.assert_allclose(got[name], ref[name], rtol=0,
                                   atol=1e-12 * np.abs(ref[name]).max(), err_msg=name)


@pytest.mark.parametrize("nbin", NBINS)
def test_two_implementations(eng, nbin):
    """row_fft 1 against row_fft 0: within twice the single-path bars."""
    new = _row_outputs(eng, nbin)
    with row_fft(eng, 0):
        assert eng.row_transform(nbin) == "direct"
        old = _row_outputs(eng, nbin)
    assert eng.row_transform(nbin) == "smooth"
    for name in ("irfft", "rotate", "scatter", "synth", "accum"):
        scale = np.abs(old[name]).max(axis=-1, keepdims=True)
        assert np.all(np.abs(new[name] - old[name]) <= 2e-12 * scale), name
    np.testing.assert_allclose(new["noise"], old["noise"], rtol=2e-10)
    np.testing.assert_allclose(new["chi2"], old["chi2"], rtol=2e-9)
    np.testing.assert_allclose(new["shift"][:, 1:], old["shift"][:, 1:], rtol=2e-6)
    d = np.abs(new["shift"][:, 0] - old["shift"][:, 0])
    assert np.all(np.minimum(d, 1.0 - d) <= 2e-3 * old["shift"][:, 1])


def _fit(eng, w, data, flags=(1, 1, 0, 0, 0), **kw):
    nu = O.guess_fit_freq(w.freqs)
    out = eng.fit_batch(data, w.model, w.freqs, w.P, [0.0, w.DM0, 0, 0, 0], list(flags),
                        nu_fit=[nu] * 3, guess=True, **kw)
    return {k: out[k].cpu().numpy() for k in FIT_KEYS}


def _same(a, b):
    for k in FIT_KEYS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


@pytest.mark.parametrize("nbin", [64, 2048])
def test_powers_of_two_untouched(eng, nbin):
    """Byte-identical row outputs and phi + DM fit under row_fft 0 and 1."""
    assert eng.row_transform(nbin) == "pow2"
    w = synth.make_workload(3, 8, nbin, seed=840 + nbin)
    data = synth.workload_data_host(w)
    rows, fit = _row_outputs(eng, nbin), _fit(eng, w, data)
    with row_fft(eng, 0):
        assert eng.row_transform(nbin) == "pow2"
        rows0, fit0 = _row_outputs(eng, nbin), _fit(eng, w, data)
    for k in rows:
        np.testing.assert_array_equal(rows[k], rows0[k], err_msg=k)
    _same(fit, fit0)


# ---------------------------------------------------------------------------
# reproducibility
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nbin", [1000, 1536])
def test_rows_alone_and_in_a_batch_bitwise(eng, nbin):
    import torch
    a = _inputs(nbin)
    NH = nbin // 2 + 1

    def spectra(rows):  # rfft of each row, through ppalign's rotate-and-sum
        n = len(rows)
        acc = torch.zeros(n, NH, 2, dtype=torch.float64, device=eng.device)
        eng.rotate_accumulate(rows[None], np.zeros((1, n)), np.ones((1, n)), acc)
        torch.cuda.synchronize()
        return acc.cpu().numpy()

    def run():
        return (spectra(a["data"]), eng.rotate_rows(a["data"], a["ph"]).cpu().numpy(),
                eng.scatter_rotate_rows(a["data"], a["ph"], a["tau_rot"]).cpu().numpy())

    spec, rot, sca = run()
    for i in (0, 3, 5):
        np.testing.assert_array_equal(spectra(a["data"][i:i + 1])[0], spec[i])
        np.testing.assert_array_equal(
            eng.rotate_rows(a["data"][i:i + 1], a["ph"][i:i + 1]).cpu().numpy()[0], rot[i])
    try:
        eng.set_workspace_limit(1)
        chunked = run()
    finally:
        eng.set_workspace_limit(32 << 30)
    for x, y in zip(chunked, (spec, rot, sca)):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("nbin", [1000, 1536])
def test_fit_alone_batch_and_chunked_bitwise(eng, nbin):
    nsub, nchan = 4, 8
    w = synth.make_workload(nsub, nchan, nbin, seed=850 + nbin)
    data = synth.workload_data_host(w)
    ref = _fit(eng, w, data)
    for i in (0, 2):
        one = _fit(eng, w, data[i:i + 1])
        for k in FIT_KEYS:
            np.testing.assert_array_equal(one[k][0], ref[k][i], err_msg=k)
    try:
        eng.set_workspace_limit(1)
        chunked = _fit(eng, w, data)
    finally:
        eng.set_workspace_limit(32 << 30)
    _same(chunked, ref)


def test_spec_cache_bitwise(eng):
    """STORE then USE at nbin 1000: the fit without the cache, bitwise."""
    nsub, nchan, nbin = 4, 8, 1000
    w = synth.make_workload(nsub, nchan, nbin, seed=860)
    data = synth.workload_data_host(w)
    ref = _fit(eng, w, data)
    cache = eng.spec_cache(nsub, nchan, nbin)
    _same(_fit(eng, w, data, spec_cache=cache), ref)
    assert cache.stored
    _same(_fit(eng, w, data, spec_cache=cache), ref)


# ---------------------------------------------------------------------------
# the fit against the oracle (test_gpu_generic_nbin._vs_oracle's bars)
# ---------------------------------------------------------------------------
def _gap(p, ref, flags):
    """Largest |device - oracle| / sigma over the fitted parameters."""
    g = abs(p[0] - ref.phi) / ref.phi_err
    for i, nm in enumerate(["DM", "GM", "tau", "alpha"], start=1):
        if flags[i]:
            g = max(g, abs(p[i] - getattr(ref, nm)) / getattr(ref, nm + "_err"))
    return g


def _same_status(rc, ref_rc, method):
    if method == "TNC" and {rc, ref_rc} <= {1, 4}:
        return True  # FCONVERGED / LSFAIL at the rounding floor
    return rc == ref_rc


def _vs_oracle(eng, nsub, nchan, nbin, seed, flags, method="trust-ncg", **kw):
    assert eng.row_transform(nbin) == "smooth"
    w = synth.make_workload(nsub, nchan, nbin, seed=seed, **kw)
    data = synth.workload_data_host(w)
    nu = O.guess_fit_freq(w.freqs)
    init = np.tile([0.0, w.DM0, 0.0, 0.0, 0.0], (nsub, 1))
    log10_tau = False
    gt = None
    if flags[3]:
        tg = 2e-3 * (nu / w.nu_ref) ** w.alpha
        init[:, 3], init[:, 4] = np.log10(tg), w.alpha
        gt = np.full(nsub, tg)
        log10_tau = True
    out = eng.fit_batch(data, w.model, w.freqs, w.P, init, flags, nu_fit=[nu] * 3, guess=True,
                        guess_tau=gt, log10_tau=log10_tau, method=method)
    out = {k: v.cpu().numpy() for k, v in out.items() if not k.startswith("_")}
    n_alt = 0
    for i in range(nsub):
        errs = O.get_noise_PS(data[i], chans=True)
        np.testing.assert_allclose(out["errs"][i], errs, rtol=1e-10)
        init = list(out["init_used"][i])

        def oracle(perm=None, init=init):
            p = np.arange(nchan) if perm is None else perm
            return O.fit_portrait_full(data[i][p], w.model[p], init, w.P, w.freqs[p], [nu] * 3,
                                       [None] * 3, errs[p], list(flags), log10_tau=log10_tau,
                                       method=method)

        ref = oracle()
        rc, p = int(out["status"][i]), out["params"][i]
        if _gap(p, ref, flags) > 1e-3 or not _same_status(rc, ref.return_code, method):
            # the oracle's own end points under a reordering of its channel
            # sums or a one-ulp restart
            rng = np.random.default_rng(seed + i)
            alts = [oracle(perm=rng.permutation(nchan)) for _ in range(8)]
            alts += [oracle(init=[np.nextafter(init[0], s)] + init[1:]) for s in (-1, 1)]
            ok = [a for a in alts if _gap(p, a, flags) <= 1e-3 and
                  _same_status(rc, a.return_code, method)]
            assert ok, (i, rc, ref.return_code, _gap(p, ref, flags),
                        [(_gap(p, a, flags), a.return_code) for a in alts])
            n_alt += 1
        np.testing.assert_allclose(out["param_errs"][i][0], ref.phi_err, rtol=1e-4)
        np.testing.assert_allclose(out["red_chi2"][i], ref.red_chi2, rtol=1e-6)
    assert n_alt <= max(1, nsub // 3), n_alt
    return out


@pytest.mark.parametrize("nbin,nchan", [(1000, 32), (1536, 32), (96, 32), (30, 16), (8100, 8)])
def test_fit_phase_dm(eng, nbin, nchan):
    _vs_oracle(eng, 4, nchan, nbin, 870 + nbin, [1, 1, 0, 0, 0])


def test_fit_gm(eng):
    _vs_oracle(eng, 3, 32, 768, 881, [1, 1, 1, 0, 0], gm=2e-6)


def test_fit_scattering(eng):
    _vs_oracle(eng, 3, 64, 1000, 882, [1, 1, 0, 1, 1], tau=2e-3)


@pytest.mark.parametrize("method", ["TNC", "Newton-CG"])
def test_fit_methods(eng, method):
    _vs_oracle(eng, 3, 24, 1000, 883, [1, 1, 0, 0, 0], method=method)


# ---------------------------------------------------------------------------
# the reference's own fits (tests/golden/generic_nbin.npz)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("value", [1, 0])
@pytest.mark.parametrize("case", [0, 1])
def test_fixture(eng, case, value):
    z = np.load(os.path.join(GOLDEN, "generic_nbin.npz"))
    g = lambda k: z["c%d_%s" % (case, k)]  # noqa: E731
    nbin = int(g("nbin"))
    with row_fft(eng, value):
        assert eng.row_transform(nbin) == ("smooth" if value else "direct")
        out = eng.fit_batch(g("data"), g("model"), g("freqs"), float(g("P")), g("init"),
                            [1, 1, 0, 0, 0], nu_fit=np.repeat(g("nu_fit")[:, None], 3, axis=1),
                            errs=g("errs"))
        out = {k: out[k].cpu().numpy() for k in FIT_KEYS}
    for i in range(2):  # every subint: none excluded
        p, e = out["params"][i], out["param_errs"][i]
        assert abs(p[0] - g("phi")[i]) <= 1e-3 * g("phi_err")[i], i
        assert abs(p[1] - g("DM")[i]) <= 1e-3 * g("DM_err")[i], i
        np.testing.assert_allclose(e[0], g("phi_err")[i], rtol=1e-4)
        np.testing.assert_allclose(e[1], g("DM_err")[i], rtol=1e-4)
        np.testing.assert_allclose(out["red_chi2"][i], g("red_chi2")[i], rtol=1e-6)
        assert int(out["status"][i]) == int(g("return_code")[i]), i


# ---------------------------------------------------------------------------
# the wide-channel path
# ---------------------------------------------------------------------------
@contextlib.contextmanager
def hbm_tables(eng, value):
    eng.set_option("hbm_tables", value)
    try:
        yield
    finally:
        eng.set_option("hbm_tables", 0)


def test_wide_channels(eng):
    """2,112 channels x nbin 96 (above PPF_LDS_NCHAN: the per-channel tables
    in HBM whatever the option says) against the oracle, and 40 channels,
    where both table layouts apply, bitwise the same under hbm_tables 0 / 1:
    the new data pass feeds both."""
    _vs_oracle(eng, 1, 2112, 96, 890, [1, 1, 0, 0, 0])
    w = synth.make_workload(1, 2112, 96, seed=890)
    data = synth.workload_data_host(w)
    a = _fit(eng, w, data)
    with hbm_tables(eng, 1):
        _same(_fit(eng, w, data), a)
    w = synth.make_workload(3, 40, 96, seed=891)
    data = synth.workload_data_host(w)
    a = _fit(eng, w, data)
    with hbm_tables(eng, 1):
        _same(_fit(eng, w, data), a)
