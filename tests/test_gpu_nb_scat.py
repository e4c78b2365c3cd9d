"""A phase and a scattering time per channel on the device:
Engine.phase_tau_batch (ppf_phase_tau_batch, ppfit_nbscat.hip) and
GetTOAs.get_narrowband_TOAs(fit_scat=True).

References: the reference's own per-channel fits (tests/golden/nb_scat.npz,
make_golden_nb_scat.py; at the odd lengths 999 and 2049 nb_scat_odd.npz,
make_golden_nb_scat_odd.py) and, for shapes the fixtures do not hold, the CPU
oracle run the same way (tests/nb_scat_cases.py; pinned to the fixtures by
tests/test_nb_scat_golden_cpu.py).

Bars, per fitted channel: |dphi| <= 1e-3 phi_err and |dtau| <= 1e-3 tau_err
(the project's bar; the reference's end point moves by at most 1.8e-5 sigma
between starts), errors and covariance to rtol 1e-6, |dscale| <= 1e-3
scale_err, snr to rtol 1e-5, red_chi2 to rtol 1e-7 (f is stationary in both
parameters, so the bars above move it at second order), status equal.  nfev
is printed, not compared.
"""
import os
import shutil

import numpy as np
import pytest

from tests import nb_scat_cases as NB
from tests.golden_consts import DM0

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from pulseportraiture_amd.engine import get_engine
    return get_engine(0)


def run(eng, data, model, noise, tau0, log10_tau, model_idx=None):
    out, status, nfev = eng.phase_tau_batch(data, model, noise=noise, tau0=tau0,
                                            log10_tau=log10_tau, model_idx=model_idx)
    return out.cpu().numpy(), status.cpu().numpy(), nfev.cpu().numpy()


def check_rows(tag, out, status, nfev, ref):
    """The module's bars; ref: a dict of per-row arrays (fixture or oracle)."""
    d = out[:, 0] - ref["phi"]
    dphi = np.abs(d - np.round(d)) / ref["phi_err"]  # phases are modulo one turn
    dtau = np.abs(out[:, 2] - ref["tau"]) / ref["tau_err"]
    dsc = np.abs(out[:, 4] - ref["scale"]) / ref["scale_err"]
    print("%s: |dphi| %.3g |dtau| %.3g |dscale| %.3g sigma; rel errs %.3g %.3g cov %.3g "
          "snr %.3g red_chi2 %.3g; nfev device %s reference %s" % (
              tag, dphi.max(), dtau.max(), dsc.max(),
              np.abs(out[:, 1] / ref["phi_err"] - 1).max(),
              np.abs(out[:, 3] / ref["tau_err"] - 1).max(),
              np.abs(out[:, 8] / ref["cov"][:, 0, 1] - 1).max(),
              np.abs(out[:, 6] / ref["snr"] - 1).max(),
              np.abs(out[:, 7] / ref["red_chi2"] - 1).max(), list(nfev),
              list(np.asarray(ref["nfeval"]).astype(int))))
    assert np.array_equal(status, np.asarray(ref["return_code"]).astype(int)), (tag, status)
    assert dphi.max() <= 1e-3 and dtau.max() <= 1e-3, (tag, dphi, dtau)
    assert dsc.max() <= 1e-3, (tag, dsc)
    np.testing.assert_allclose(out[:, 1], ref["phi_err"], rtol=1e-6, err_msg=tag)
    np.testing.assert_allclose(out[:, 3], ref["tau_err"], rtol=1e-6, err_msg=tag)
    np.testing.assert_allclose(out[:, 5], ref["scale_err"], rtol=1e-6, err_msg=tag)
    np.testing.assert_allclose(out[:, 8], ref["cov"][:, 0, 1], rtol=1e-6, err_msg=tag)
    np.testing.assert_allclose(out[:, 6], ref["snr"], rtol=1e-5, err_msg=tag)
    np.testing.assert_allclose(out[:, 7], ref["red_chi2"], rtol=1e-7, err_msg=tag)


def kernel_start_phase(data, model, tau, nbin):
    """The starting phase k_nbscat documents (header of ppfit_nbscat.hip): the
    largest cross-correlation between the profile and the template scattered
    at the starting tau, both limited to their first min(nbin / 2, 128)
    harmonics, over the G = min(nbin, 256) phases -0.5 + g / G; the lowest g
    on a tie (argmax)."""
    G, K = min(nbin, 256), min(nbin // 2, 128)
    from oracle import ppfit_oracle as O
    B = O.scattering_portrait_FT(np.array([tau]), nbin)[0]
    Y = (np.fft.rfft(data) * np.conj(np.fft.rfft(model) * B))[1:K + 1]
    ph = -0.5 + np.arange(G) / G
    corr = (Y[None] * np.exp(2j * np.pi * np.outer(ph, np.arange(1, K + 1)))).real.sum(axis=1)
    return float(ph[np.argmax(corr)])


def oracle_rows(data, model, freqs, sigma, P, tau0, log10_tau, start=NB.xcorr_phase):
    """Per-row oracle fits from the bin-resolution cross-correlation start
    (or, with start=kernel_start_phase, from the device's own)."""
    rows = []
    for n in range(len(data)):
        nbin = data.shape[-1]
        ph0 = start(data[n], model[n], NB.start_tau(float(tau0[n]), nbin), nbin)
        rows.append(NB.oracle_channel(data[n], model[n], float(freqs[n]),
                                      None if sigma is None else float(sigma[n]), P, ph0,
                                      float(tau0[n]), log10_tau))
    return {k: np.array([r[k] for r in rows]) for k in rows[0]}


def fixture_case(eng, ic, name):
    c = NB.case(ic, name)
    out, status, nfev = run(eng, c["data"], c["model"], c["errs"], c["tau0"], c["log10"],
                            np.arange(len(c["freqs"])))
    check_rows("case %d nbin %d log10 %d" % (ic, c["nbin"], c["log10"]), out, status, nfev, c)


@pytest.mark.parametrize("ic", NB.scattered_cases())
def test_fixture_scattered_cases(eng, ic):
    fixture_case(eng, ic, NB.MAIN)


@pytest.mark.parametrize("ic", NB.scattered_cases(NB.ODD))
def test_fixture_odd_length_cases(eng, ic):
    """The reference's own fits at nbin 999 (log10 tau, k_nbscat<8>) and 2049
    (linear tau, k_nbscat<16>, the generic-length transform): no Nyquist term,
    errs_FT = sigma sqrt(nbin / 2) with a half-integer, dof = nbin - 3."""
    assert NB.case(ic, NB.ODD)["nbin"] % 2 == 1
    fixture_case(eng, ic, NB.ODD)


@pytest.mark.parametrize("ic", NB.unscattered_cases())
def test_fixture_unscattered_case(eng, ic):
    """No scattering in the data: the reference's log10 tau ends near -8 with
    an error near 1e5, so only the phase and the status are held."""
    c = NB.case(ic)
    out, status, nfev = run(eng, c["data"], c["model"], c["errs"], c["tau0"], c["log10"],
                            np.arange(len(c["freqs"])))
    dphi = np.abs(out[:, 0] - c["phi"]) / c["phi_err"]
    print("unscattered case %d: |dphi| %.3g sigma, status %s, log10 tau %s, nfev device %s "
          "reference %s" % (ic, dphi.max(), list(status), list(np.round(out[:, 2], 2)),
                            list(nfev), list(c["nfeval"])))
    assert np.all(np.isin(status, [0, 1, 2, 3])), status
    assert np.all(np.isfinite(out[:, 0]))
    assert dphi.max() <= 1e-3, dphi


def linear_256_case():
    for ic in NB.scattered_cases():
        c = NB.case(ic)
        if c["nbin"] == 256 and not c["log10"]:
            return c
    raise AssertionError("fixture lacks the (256, linear) case")


def test_zero_start_linear(eng):
    """tau0 = 0 starts at 1 / nbin with linear tau too: the same end point."""
    c = linear_256_case()
    n = len(c["freqs"])
    out, status, nfev = run(eng, c["data"], c["model"], c["errs"], np.zeros(n), False,
                            np.arange(n))
    check_rows("tau0 = 0, linear", out, status, nfev, c)


def test_zero_start_log10(eng):
    """The same data fitted in log10 tau from tau0 = 0, against the oracle
    started there; the end point is the linear fit's."""
    c = linear_256_case()
    n = len(c["freqs"])
    out, status, nfev = run(eng, c["data"], c["model"], c["errs"], np.zeros(n), True,
                            np.arange(n))
    ref = oracle_rows(c["data"], c["model"], c["freqs"], c["errs"], c["P"], np.zeros(n), True)
    check_rows("tau0 = 0, log10", out, status, nfev, ref)
    assert np.all(np.abs(10 ** out[:, 2] - c["tau"]) <= 1e-3 * c["tau_err"])
    assert np.all(np.abs(out[:, 0] - c["phi"]) <= 1e-3 * c["phi_err"])


def test_batch_independence(eng):
    """Rows fitted alone, in a call of five and inside a call of 37 are
    bitwise the same (one wave per row, four rows per workgroup: 1, 5 and 37
    all leave a workgroup partly empty)."""
    c = NB.case(NB.scattered_cases()[1])
    nch = len(c["freqs"])
    idx = np.arange(37) % nch
    args = lambda sel: (c["data"][idx[sel]], c["model"], c["errs"][idx[sel]],  # noqa: E731
                        c["tau0"][idx[sel]], c["log10"], idx[sel])
    big = run(eng, *args(np.arange(37)))
    pick = np.array([0, 7, 16, 21, 36])
    five = run(eng, *args(pick))
    for a, b in zip(five, big):
        assert np.array_equal(a, b[pick])
    for j in (3, 36):
        one = run(eng, *args(np.array([j])))
        for a, b in zip(one, big):
            assert np.array_equal(a, b[[j]])
    # rows that repeat a channel repeat its result
    assert np.array_equal(big[0][0], big[0][nch])


def gaussian_channel(nbin, width, tau, phi, sigma, seed, nrow=1):
    """nrow noisy copies of a Gaussian template scattered by tau [rot] and
    rotated by -phi, with the template."""
    from oracle import ppfit_oracle as O
    x = O.get_bin_centers(nbin)
    tmpl = np.exp(-0.5 * ((x - 0.4) / width) ** 2) + 0.4 * np.exp(-0.5 * ((x - 0.55) / width) ** 2)
    B = O.scattering_portrait_FT(np.array([tau]), nbin)[0]
    k = np.arange(nbin // 2 + 1)
    clean = np.fft.irfft(np.fft.rfft(tmpl) * B * np.exp(-2j * np.pi * k * phi), nbin)
    rng = np.random.default_rng(seed)
    return tmpl, clean[None] + rng.normal(0.0, sigma, (nrow, nbin))


@pytest.mark.parametrize("nbin,width,tau,sigma", [(16, 0.08, 0.08, 0.01),
                                                  (8192, 0.004, 0.003, 0.05)])
def test_smallest_and_largest_nbin(eng, nbin, width, tau, sigma):
    """nbin 16 (the generic-length transform, one register slot) and 8192
    (rows re-read from memory in every evaluation) against the oracle."""
    tmpl, data = gaussian_channel(nbin, width, tau, 0.137, sigma, 16 + nbin)
    tau0 = np.array([0.6 * tau])
    noise = np.array([sigma])
    ref = oracle_rows(data, tmpl[None], [1400.0], noise, 0.003, tau0, True)
    assert ref["snr"][0] >= 15.0, ref["snr"]
    out, status, nfev = run(eng, data, tmpl, noise, tau0, True)
    check_rows("nbin %d" % nbin, out, status, nfev, ref)


# nbin, with nh = nbin // 2 and the register slots ppf_phase_tau_batch picks for
# it (ppfit_capi.hip: nj = 1, 2, 4, 8, 16 for nh <= 64, 128, 256, 512, 1024,
# else 0 = rows re-read from memory).  A change of that dispatch changes this
# column: look again at which lengths sit on its seams.
SEAM_NBINS = [
    130,   # nh 65,   2 slots: one harmonic in the second slot
    258,   # nh 129,  4 slots: third slot nearly empty, fourth empty
    514,   # nh 257,  8 slots: first length of k_nbscat<8>
    999,   # nh 499,  8 slots: odd, ragged
    1024,  # nh 512,  8 slots: all eight full
    1026,  # nh 513,  16 slots: nine of sixteen used
    2049,  # nh 1024, 16 slots: odd, all sixteen full, generic transform
    2050,  # nh 1025, 0: first length of the memory path
    3000,  # nh 1500, 0: ragged tail (23 x 64 + 28)
    4096,  # nh 2048, 0: power-of-two transform on the memory path
    8191,  # nh 4095, 0: largest odd
]
# (nbin, log10_tau, noise given) at which the oracle starts from the kernel's
# own starting phase (test_slot_and_length_seams)
SEAM_KERNEL_START = {(2049, True, True)}


@pytest.mark.parametrize("given", [True, False], ids=["noise_given", "noise_device"])
@pytest.mark.parametrize("log10_tau", [True, False], ids=["log10", "linear"])
@pytest.mark.parametrize("nbin", SEAM_NBINS)
def test_slot_and_length_seams(eng, nbin, log10_tau, given):
    """Every instantiation of k_nbscat, with full, partly filled and empty
    slots, odd lengths and the memory path's first, ragged and longest
    lengths, against the oracle (two rows a case; the noise given, or NaN and
    estimated on the device, the oracle then with sigma=None).

    The device starts from its coarse grid and the oracle from xcorr_phase.
    At (2049, log10 tau, noise given) the oracle's own end point moves by
    3.6e-6 sigma in phi and 4.5e-6 sigma in tau between those two starts (the
    solver stops where rounding makes the predicted reduction non-positive),
    and cov(phi, t), the small off-diagonal term, by 1.07e-6 of itself, past
    its 1e-6 bar; the device differed from the xcorr-started oracle by exactly
    those amounts, with equal status.  There the oracle starts from the
    kernel's documented start (kernel_start_phase) and the bars are unchanged;
    every other case keeps the xcorr start."""
    width = max(0.004, 4.0 / nbin)
    tau, sigma = 0.75 * width, 0.05
    tmpl, data = gaussian_channel(nbin, width, tau, 0.137, sigma, 16 + nbin, nrow=2)
    tau0 = np.full(2, 0.6 * tau)
    start = kernel_start_phase if (nbin, log10_tau, given) in SEAM_KERNEL_START \
        else NB.xcorr_phase
    ref = oracle_rows(data, np.stack([tmpl] * 2), [1400.0] * 2, [sigma] * 2 if given else None,
                      0.003, tau0, log10_tau, start)
    assert ref["snr"].min() >= 15.0, ref["snr"]
    noise = np.array([sigma] * 2) if given else np.full(2, np.nan)
    out, status, nfev = run(eng, data, tmpl, noise, tau0, log10_tau)
    check_rows("seam nbin %d log10 %d given %d" % (nbin, log10_tau, given), out, status, nfev,
               ref)


@pytest.mark.parametrize("log10_tau", [True, False], ids=["log10", "linear"])
@pytest.mark.parametrize("nbin", [130, 258, 999, 2049, 3000])  # 2, 4, 8, 16 and 0 slots
def test_upper_slots_carry_signal(eng, nbin, log10_tau):
    """The seam cases' templates (width >= 0.004 rot) have no power above
    harmonic ~150, so their upper slots hold noise only and bear on red_chi2
    alone.  Here the template is half a bin wide and tau is two bins: |M_k| at
    nbin / 4 is above 0.1 |M_1|, every slot's X_k, m_k and phasor bear on phi,
    tau and their errors.  The coarse starting grid is then many bins from
    the peak; the oracle starts from the kernel's documented start, and its
    end point from xcorr_phase is the same to 4.8e-6 sigma."""
    width, tau, sigma = 0.5 / nbin, 2.0 / nbin, 0.02
    tmpl, data = gaussian_channel(nbin, width, tau, 0.137, sigma, 77 + nbin, nrow=2)
    M = np.abs(np.fft.rfft(tmpl))
    assert M[nbin // 4] >= 0.1 * M[1]
    tau0 = np.full(2, 0.6 * tau)
    ref = oracle_rows(data, np.stack([tmpl] * 2), [1400.0] * 2, [sigma] * 2, 0.003, tau0,
                      log10_tau, kernel_start_phase)
    assert ref["snr"].min() >= 15.0, ref["snr"]
    out, status, nfev = run(eng, data, tmpl, np.array([sigma] * 2), tau0, log10_tau)
    check_rows("sharp nbin %d log10 %d" % (nbin, log10_tau), out, status, nfev, ref)


def test_more_than_one_chunk(eng):
    """ppf_phase_tau_batch cuts its rows into chunks of the workspace limit
    and offsets model_idx, noise, tau0, out, status and nfev by the chunk's
    first row: 11 rows of the (256, linear) fixture case in one chunk, in
    chunks of one and in chunks of 3, 3, 3, 2 are bitwise the same.  Every
    per-row input differs from row to row, model_idx is not monotonic, and the
    noise is given for some rows and NaN (estimated on the device) for others."""
    c = linear_256_case()
    nch, nbin = len(c["freqs"]), c["nbin"]
    idx = (5 * np.arange(11)) % nch  # 0 5 10 15 4 9 14 3 8 13 2
    assert len(set(idx)) == 11 and np.any(np.diff(idx) < 0)
    noise = c["errs"][idx].copy()
    est = np.array([1, 4, 6, 9])
    noise[est] = np.nan
    tau0 = c["tau0"][idx]
    assert len(set(tau0)) == 11 and len(set(c["errs"][idx])) == 11
    args = (c["data"][idx], c["model"], noise, tau0, False, idx)
    per_row = (nbin // 2 + 1) * 16  # ppf_phase_tau_batch: one double2 spectrum a row
    limit = eng.workspace_limit()
    try:
        whole = run(eng, *args)
        eng.set_workspace_limit(1)  # max(1, ...): every row its own chunk
        ones = run(eng, *args)
        eng.set_workspace_limit(3 * per_row + per_row // 2)  # chunks of 3, 3, 3, 2
        threes = run(eng, *args)
    finally:
        eng.set_workspace_limit(limit)
    for name, a, b, d in zip(("out", "status", "nfev"), whole, ones, threes):
        assert np.array_equal(a, b), name
        assert np.array_equal(a, d), name
    # the rows whose noise was given are the fixture's
    giv = np.setdiff1d(np.arange(11), est)
    check_rows("chunked rows, noise given", whole[0][giv], whole[1][giv], whole[2][giv],
               {k: c[k][idx[giv]] for k in ("phi", "phi_err", "tau", "tau_err", "scale",
                                            "scale_err", "snr", "red_chi2", "cov",
                                            "return_code", "nfeval")})


def test_shared_model_rows_and_device_noise(eng):
    """model_idx shared between rows, and NaN noise estimated on the device
    (get_noise_PS of the row)."""
    nbin = 128
    t0, d0 = gaussian_channel(nbin, 0.03, 0.02, -0.21, 0.02, 5, nrow=3)
    t1, d1 = gaussian_channel(nbin, 0.05, 0.03, 0.33, 0.02, 6, nrow=2)
    data = np.concatenate([d0[:2], d1, d0[2:]])
    models = np.stack([t0, t1])
    midx = np.array([0, 0, 1, 1, 0], dtype=np.int32)
    tau0 = np.array([0.015, 0.015, 0.02, 0.02, 0.015])
    ref = oracle_rows(data, models[midx], [1400.0] * 5, None, 0.003, tau0, False)
    assert ref["snr"].min() >= 15.0, ref["snr"]
    out, status, nfev = run(eng, data, models, np.full(5, np.nan), tau0, False, midx)
    check_rows("shared model rows, device noise", out, status, nfev, ref)
    none = run(eng, data, models, None, tau0, False, midx)
    assert np.array_equal(none[0], out)


@pytest.mark.parametrize("nbin", [8, 16384])
def test_nbin_outside_range_is_refused(eng, nbin):
    from pulseportraiture_amd.engine import PPFitError
    with pytest.raises(PPFitError, match="nbin"):
        eng.phase_tau_batch(np.zeros((2, nbin)), np.zeros((1, nbin)))


# --------------------------------------------------------------------------
# End to end: GetTOAs.get_narrowband_TOAs on a 2 x 16 x 256 archive
# --------------------------------------------------------------------------
E2E = dict(name="nbscat.fits", nsub=2, nchan=16, nbin=256, seed=8118, tau=2e-2, sigma=0.1,
           zero_chan=5, scat_guess=(4e-5, 1500.0, -4.0))


def register_e2e_archive():
    """As tests/test_gpu_configs.register_synth_archive, with the noise level
    given (every channel at S/N >= 15) and one zero-weight channel."""
    from pulseportraiture_amd import archive, synth
    from pulseportraiture_amd.mjd import MJD
    e = E2E
    nsub, nchan = e["nsub"], e["nchan"]
    w = synth.make_workload(nsub, nchan, e["nbin"], seed=e["seed"], tau=e["tau"],
                            sigma=e["sigma"])
    data = synth.workload_data_host(w)
    wts = np.ones((nsub, nchan))
    wts[:, e["zero_chan"]] = 0.0
    b = dict(subints=data[:, None], freqs=np.tile(w.freqs, (nsub, 1)), weights=wts,
             SNRs=np.ones((nsub, 1, nchan)), Ps=np.full(nsub, w.P),
             doppler_factors=np.full(nsub, 1.00002),
             epochs=[MJD(57300.0 + 0.001 * i) + 10.0 for i in range(nsub)], DM=DM0,
             backend="syn_be", frontend="syn_rx", backend_delay=2.0e-6, telescope="GBT",
             telescope_code="1", bw=800.0, nu0=1500.0, subtimes=[30.0] * nsub, prof_SNR=100.0)
    archive.register_archive(e["name"], b)
    return w, data


@pytest.fixture(scope="module")
def e2e(eng, tmp_path_factory):
    from pulseportraiture_amd import synth
    w, data = register_e2e_archive()
    d = tmp_path_factory.mktemp("nbscat")
    gmodel = os.path.join(d, "example.gmodel")
    shutil.copy(synth.EXAMPLE_GMODEL, gmodel)
    # the archive holds no noise levels: the driver leaves them to the device
    # (get_noise_PS of each row), the oracle takes the same estimate
    return dict(w=w, data=data, gmodel=gmodel, oracle={})


def e2e_oracle(e2e, log10_tau):
    """Per-channel oracle fits of the archive, computed once per parameterisation."""
    if log10_tau not in e2e["oracle"]:
        w = e2e["w"]
        ts, tref, al = E2E["scat_guess"]
        ref = {}
        for s in range(E2E["nsub"]):
            tau0 = (ts / w.P) * (w.freqs / tref) ** al
            ref[s] = oracle_rows(e2e["data"][s], w.model, w.freqs, None, w.P, tau0, log10_tau)
        e2e["oracle"][log10_tau] = ref
    return e2e["oracle"][log10_tau]


@pytest.mark.parametrize("log10_tau", [True, False])
def test_get_narrowband_toas_fit_scat(eng, e2e, log10_tau):
    from pulseportraiture_amd import pptoas
    from tests._compare import tim_lines
    from tests.test_gpu_drivers import parse_tim
    e, w = E2E, e2e["w"]
    gt = pptoas.GetTOAs([e["name"]], e2e["gmodel"], quiet=True)
    gt.get_narrowband_TOAs(fit_scat=True, log10_tau=log10_tau, scat_guess=e["scat_guess"],
                           quiet=True)
    ref = e2e_oracle(e2e, log10_tau)
    assert gt.nfit == 2 and gt.fit_flags == [1, 1]
    assert gt.covariances[0].shape == (e["nsub"], e["nchan"], 2, 2)
    fitted = np.ones(e["nchan"], dtype=bool)
    fitted[e["zero_chan"]] = False
    lines = tim_lines(gt)
    assert len(lines) == e["nsub"] * fitted.sum()
    for s in range(e["nsub"]):
        r = {k: v[fitted] for k, v in ref[s].items()}
        assert r["snr"].min() >= 15.0, r["snr"]
        # the zero-weight channel is left out
        for arr in (gt.phis, gt.phi_errs, gt.taus, gt.tau_errs, gt.scales, gt.nfevals):
            assert arr[0][s, e["zero_chan"]] == 0
        assert np.all(gt.taus[0][s, fitted] != 0.0)
        out = np.stack([gt.phis[0][s], gt.phi_errs[0][s], gt.taus[0][s], gt.tau_errs[0][s],
                        gt.scales[0][s], gt.scale_errs[0][s], gt.channel_snrs[0][s],
                        np.full(e["nchan"], np.nan), gt.covariances[0][s, :, 0, 1]], axis=1)
        # channel_red_chi2s holds the last channel's value for the whole row
        # (the reference's quirk, pptoas.py:1011)
        out[fitted, 7] = r["red_chi2"]
        np.testing.assert_allclose(gt.channel_red_chi2s[0][s], r["red_chi2"][-1], rtol=1e-7)
        check_rows("e2e subint %d log10 %d" % (s, log10_tau), out[fitted], gt.rcs[0][s, fitted],
                   gt.nfevals[0][s, fitted], r)
        np.testing.assert_allclose(gt.covariances[0][s, fitted, 0, 0], r["cov"][:, 0, 0],
                                   rtol=2e-6)
        np.testing.assert_allclose(gt.covariances[0][s, fitted, 1, 1], r["cov"][:, 1, 1],
                                   rtol=2e-6)
        # .tim flags: %.3f text of the oracle's values, moved by at most the bars
        chans = np.where(fitted)[0]
        for j, n in enumerate(chans):
            head, f = parse_tim(lines[s * len(chans) + j])
            assert int(f["subint"]) == s and int(f["chan"]) == n
            tau, terr = r["tau"][j], r["tau_err"][j]
            assert abs(float(f["scat_ref_freq"]) - w.freqs[n]) <= 1.1e-3
            if log10_tau:
                assert set(f) >= {"scat_time", "log10_scat_time", "log10_scat_time_err"}
                assert "scat_time_err" not in f
                st = 10 ** tau * w.P * 1e6
                assert abs(float(f["scat_time"]) - st) <= 1.1e-3 + st * np.log(10) * 1e-3 * terr
                assert abs(float(f["log10_scat_time"]) - (tau + np.log10(w.P))) <= \
                    1.1e-3 + 1e-3 * terr
                assert abs(float(f["log10_scat_time_err"]) - terr) <= 1.1e-3
            else:
                assert set(f) >= {"scat_time", "scat_time_err"}
                assert "log10_scat_time" not in f
                assert abs(float(f["scat_time"]) - tau * w.P * 1e6) <= \
                    1.1e-3 + 1e-3 * terr * w.P * 1e6
                assert abs(float(f["scat_time_err"]) - terr * w.P * 1e6) <= \
                    1.1e-3 + 1e-6 * terr * w.P * 1e6


def test_fit_scat_false_is_the_phase_shift_path(eng, e2e):
    """fit_scat=False gives what phase_shift_batch gives on the same rows
    (bitwise), tau = 0, no scattering flags."""
    from pulseportraiture_amd import pptoas
    from tests._compare import tim_lines
    from tests.test_gpu_drivers import parse_tim
    e, w = E2E, e2e["w"]
    gt = pptoas.GetTOAs([e["name"]], e2e["gmodel"], quiet=True)
    gt.get_narrowband_TOAs(quiet=True)
    assert gt.nfit == 1 and gt.fit_flags == [1, 0]
    fitted = np.ones(e["nchan"], dtype=bool)
    fitted[e["zero_chan"]] = False
    # the template as get_narrowband_TOAs builds it: the .gmodel with its TAU
    models = gt.templates.portraits(w.freqs[None], e["nbin"], np.array([w.P]))[0]
    for s in range(e["nsub"]):
        out = eng.phase_shift_batch(e2e["data"][s][fitted], models,
                                    noise=np.full(fitted.sum(), np.nan), Ns=100,
                                    bounds=(-0.5, 0.5),
                                    model_idx=np.where(fitted)[0]).cpu().numpy()
        assert np.array_equal(gt.phis[0][s, fitted], out[:, 0])
        assert np.array_equal(gt.phi_errs[0][s, fitted], out[:, 1])
        assert np.array_equal(gt.scales[0][s, fitted], out[:, 2])
        assert np.array_equal(gt.channel_snrs[0][s, fitted], out[:, 4])
    assert not np.any(gt.taus[0]) and not np.any(gt.rcs[0]) and not np.any(gt.nfevals[0])
    assert gt.covariances[0].shape == (e["nsub"], e["nchan"], 1, 1)
    for line in tim_lines(gt):
        assert not any(k.startswith(("scat", "log10_scat")) for k in parse_tim(line)[1])


def test_fit_scat_needs_trust_ncg(eng, e2e):
    from pulseportraiture_amd import pptoas
    gt = pptoas.GetTOAs([E2E["name"]], e2e["gmodel"], quiet=True)
    with pytest.raises(NotImplementedError, match="trust-ncg"):
        gt.get_narrowband_TOAs(fit_scat=True, method="TNC", quiet=True)
