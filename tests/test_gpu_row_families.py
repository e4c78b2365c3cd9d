"""The row entry points at lengths of both transform families.

Every rfft-based row kernel is one body instantiated for the LDS FFT (nbin a
power of two from 64 up) and for direct sums (every other nbin in [16,
8192]).  test_row_entry_points_generic (test_gpu_generic_nbin.py) holds
noise_rows, irfft_rows, phase_shift_batch, resid_chi2_rows and
rotate_accumulate to numpy / the oracle on ROW_NBINS; these tests do the same
for the entry points it does not reach, each at the tolerance of the existing
test of that entry point.
"""
import numpy as np
import pytest

from oracle import ppfit_oracle as O
from pulseportraiture_amd import synth
from tests import noise_fit_reference as R
from tests.test_gpu_generic_nbin import ROW_NBINS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from pulseportraiture_amd.engine import Engine
    return Engine(0)


@pytest.mark.parametrize("nbin", ROW_NBINS)
def test_rotate_rows_both_families(eng, nbin):
    """rotate_rows in place and scatter_rotate_rows with tau != 0 against
    numpy (test_rotate_rows_generic's tolerance)."""
    import torch
    rng = np.random.default_rng(nbin)
    rows = rng.standard_normal((5, nbin))
    ph = rng.uniform(-0.5, 0.5, 5)
    tau = rng.uniform(0.1, 3.0, 5)
    k = np.arange(nbin // 2 + 1)
    ref = np.fft.irfft(np.fft.rfft(rows) * np.exp(2j * np.pi * np.outer(ph, k)), n=nbin)
    buf = torch.tensor(rows, dtype=torch.float64, device=eng.device)
    out = eng.rotate_rows(buf, ph, inplace=True)
    torch.cuda.synchronize()
    assert out.data_ptr() == buf.data_ptr()
    np.testing.assert_allclose(buf.cpu().numpy(), ref, rtol=0, atol=1e-12 * np.abs(ref).max())
    got = eng.scatter_rotate_rows(rows, ph, tau).cpu().numpy()
    spec = np.fft.rfft(rows) * np.exp(2j * np.pi * np.outer(ph, k)) / (1 + 2j * np.pi * np.outer(tau, k))
    ref = np.fft.irfft(spec, n=nbin)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12 * np.abs(ref).max())


@pytest.mark.parametrize("nbin", ROW_NBINS)
def test_noise_fit_rows_both_families(eng, nbin):
    """noise_fit_rows against the CPU reference of get_noise(method="fit"),
    as test_noise_fit_rows_vs_reference: kc and the winning a on the rows whose
    winner is safe from rounding, the noise to 1e-9 where kc agrees."""
    w = synth.make_workload(1, 5, nbin, seed=770 + nbin)
    rows = synth.workload_data_host(w)[0]
    noise, kc, idx = [t.cpu().numpy() for t in eng.noise_fit_rows(rows, full=True)]
    ref = [R.find_kc(R.power_spectrum(r), full=True) for r in rows]
    ref_kc = np.array([r[0] for r in ref])
    ref_idx = np.array([r[1] for r in ref])
    sep = np.array([R.separated(r[2], r[1]) for r in ref])
    print("nbin", nbin, "kc", kc.tolist(), "ref", ref_kc.tolist(), "separated", sep.tolist())
    assert np.array_equal(kc[sep], ref_kc[sep])
    assert np.array_equal(idx[sep] // (R.NS * R.NS), ref_idx[sep] // (R.NS * R.NS))
    same = kc == ref_kc
    for fact in (1.1, 2.0):
        got = noise if fact == 1.1 else eng.noise_fit_rows(rows, fact=fact).cpu().numpy()
        want = np.array([R.noise_from_kc(R.power_spectrum(r), c, fact)[0]
                         for r, c in zip(rows, ref_kc)])
        err = np.abs(got[same] - want[same]) / np.abs(want[same])
        print("fact", fact, "max relative noise difference", err.max() if same.any() else None)
        assert np.all(err <= 1e-9)


@pytest.mark.parametrize("nbin", ROW_NBINS)
def test_synth_and_fake_both_families(eng, nbin):
    """synth and fake_subints(packed=False): noise-free against numpy's irfft
    of the rotated template spectrum, with noise against synth.noise_block
    (test_synth_generic's and test_fake_subints' tolerance)."""
    nchan, nsub, seed, sub0 = 4, 2, 12345, 7
    rng = np.random.default_rng(3 + nbin)
    model = rng.normal(0, 1, (nchan, nbin))
    ph = rng.uniform(-2, 2, (nsub, nchan))
    k = np.arange(nbin // 2 + 1)
    rot = np.fft.irfft(np.fft.rfft(model, axis=-1)[None] * np.exp(2j * np.pi * ph[..., None] * k),
                       n=nbin, axis=-1)
    np.testing.assert_allclose(eng.synth(model, ph, 0.0, seed, sub0=sub0).cpu().numpy(), rot,
                               atol=1e-11)
    np.testing.assert_allclose(eng.synth(model, ph, 1.5, seed, sub0=sub0).cpu().numpy(),
                               rot + synth.noise_block(nsub, nchan, nbin, 1.5, seed, sub0),
                               atol=1e-11)
    amp = rng.uniform(0.5, 1.5, (nsub, nchan))
    sigma = rng.uniform(0.5, 1.5, nchan)
    sigma[1] = 0.0
    got = eng.fake_subints(model, ph, amp, 0.0, seed, sub0=sub0).cpu().numpy()
    np.testing.assert_allclose(got[:, 0], rot * amp[..., None], atol=1e-11)
    got = eng.fake_subints(model, ph, amp, sigma, seed, sub0=sub0, npol=2).cpu().numpy()
    z = synth.noise_block(nsub, 2 * nchan, nbin, 1.0, seed, sub0).reshape(nsub, 2, nchan, nbin)
    np.testing.assert_allclose(got, (rot * amp[..., None])[:, None] + z * sigma[None, None, :, None],
                               atol=1e-11)


@pytest.mark.parametrize("nbin", ROW_NBINS)
def test_phase_shift_model_idx_both_families(eng, nbin):
    """The template spectra through phase_shift_batch with a model_idx that
    repeats rows and skips others (test_row_entry_points_generic's bounds)."""
    w = synth.make_workload(1, 6, nbin, seed=780 + nbin)
    data = synth.workload_data_host(w)[0]
    midx = np.array([0, 2, 2, 5, 0, 3])  # rows 1 and 4 are never used
    out = eng.phase_shift_batch(data, w.model, model_idx=midx).cpu().numpy()
    for i in range(6):
        ref = O.fit_phase_shift(data[i], w.model[midx[i]])
        d = abs(out[i, 0] - ref.phase)
        assert min(d, 1.0 - d) <= 1e-3 * ref.phase_err, i
        np.testing.assert_allclose(out[i, 1:], [ref.phase_err, ref.scale, ref.scale_err, ref.snr,
                                                ref.red_chi2], rtol=1e-6)
