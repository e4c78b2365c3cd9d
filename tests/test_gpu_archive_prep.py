"""The kernels every profile passes before a fit (k_unpack, k_tscrunch,
k_remove_baseline, k_profile_snr) against tests/archive_prep_reference.py:
exact references that share no summation order with the device, with error
bounds derived there from (n - 1) u sum|terms|.  The inputs are those of
tests/archive_prep_cases.py; tests/test_archive_prep_cpu.py proves on the CPU
that each random one is separated (window and crossing margins of at least
1e-9, no row left out), so windows and edges are compared for equality here
and no row is ever skipped.

ppf_profile_snr returns the S/N alone: its window and edges are held through
it (another window or edge moves the S/N by orders of magnitude more than the
bound; the CPU file shows this for the oracle's restatement).

The NaN tests come last: they need the guarded arg-min (include/ppfit.h: a
NaN sum never wins, no ordered sum gives window 0)."""
import numpy as np
import pytest

from tests import archive_prep_cases as K
from tests import archive_prep_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from pulseportraiture_amd.engine import get_engine
    return get_engine(0)


def _remove(gpu, d, w, ntot, duty=K.DUTY):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(d), device=gpu.device).contiguous()
    win = gpu.remove_baseline(t, w, ntot=ntot, duty=duty).cpu().numpy()
    return t.cpu().numpy(), win


def _snr(gpu, x, width, thr=0.1):
    nbin = np.shape(x)[-1]
    duty = (width + 0.5) / nbin  # int(duty nbin) == width
    assert max(1, int(duty * nbin)) == width
    return gpu.profile_snr(x, duty=duty, threshold=thr).cpu().numpy()


# ---------------------------------------------------------------------------
# remove_baseline
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.BASELINE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_remove_baseline_vs_exact(gpu, case):
    """Windows equal, values within (width + 3) u max|row| of the exact result
    (remove_baseline_bound; the parent's bar was 1e-11 max|data|); a wrapping
    window, an unweighted subint (window 0), an unweighted channel with a 1e6
    offset, non-unit weights; a subint alone equals itself in the batch."""
    nbin, npol, ntot, nchan = case
    wd = K.width_of(nbin)
    d, w = K.baseline_case(*case)
    _, starts, _ = R.remove_baseline_exact(d, w, ntot, wd)
    got, win = _remove(gpu, d, w, ntot)
    np.testing.assert_array_equal(win, starts)
    err = R.remove_baseline_error(got, d, starts, wd)
    bound = R.remove_baseline_bound(d, wd)
    print(case, "max err / bound", (err / bound).max())
    assert (err <= bound).all()
    for s in range(3):
        one, w1 = _remove(gpu, d[s:s + 1], w[s:s + 1], ntot)
        assert w1[0] == starts[s]
        np.testing.assert_array_equal(one[0], got[s])


def test_remove_baseline_full_width(gpu):
    """duty 1.0, width = nbin: integer rows tie exactly (window 0); on random
    rows every window holds the whole row, so the values are held to the
    bound whatever start the rounding of equal sums picks."""
    d, w, _ = K.tie_subints(512)
    got, win = _remove(gpu, d, w, 2, duty=1.0)
    np.testing.assert_array_equal(win, 0)
    assert (R.remove_baseline_error(got, d, win, 512) <= R.remove_baseline_bound(d, 512)).all()
    d, w = K.baseline_case(100, 4, 2, 3)
    got, win = _remove(gpu, d, w, 2, duty=1.0)
    assert ((win >= 0) & (win < 100)).all() and win[1] == 0
    assert (R.remove_baseline_error(got, d, win, 100) <= R.remove_baseline_bound(d, 100)).all()


@pytest.mark.parametrize("nbin", K.TIE_NBINS)
def test_exact_ties_first_window(gpu, nbin):
    """Integer rows whose smallest window sum is shared: the first start wins
    between adjacent lanes, across waves (+64), at a thread's second stride
    (+256) and against a wrapping window, in k_remove_baseline (total of two
    channels with weights 1 and 2, two polarisations) and in k_profile_snr.
    ppf_profile_snr returns no window, so there the rows are K.tie_snr_rows
    and the S/N has to be the first window's: tied windows inside one dip
    (adjacent; +64 at nbin 512 and 1000, whose widths pass 64) hold the same
    bins and edges and give the same S/N whichever is taken; separate dips
    (+64 at nbin 400, width 60, and +256, each in one lane; the wrapping dip
    against another lane's) do not."""
    wd = K.width_of(nbin)
    d, w, want = K.tie_subints(nbin)
    got, win = _remove(gpu, d, w, 2)
    np.testing.assert_array_equal(win, want)
    assert (R.remove_baseline_error(got, d, want, wd) <= R.remove_baseline_bound(d, wd)).all()
    # k_profile_snr returns no window: make the S/N tell the tied windows apart
    x = K.tie_snr_rows(nbin)
    ex = R.profile_snr_exact(x, wd, 0.1)
    np.testing.assert_array_equal(ex["window"], want)
    snr = _snr(gpu, x, wd)
    assert (ex["snr"][1:] > 0).all()
    assert (np.abs(snr - ex["snr"]) <= K.INTEGER_SNR_ULPS * R.U * ex["snr"]).all()


# ---------------------------------------------------------------------------
# profile_snr
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nbin,thr", K.SNR_CASES)
def test_profile_snr_vs_exact(gpu, nbin, thr):
    """S/N within the per-row bound of profile_snr_exact (below 1e-12 |snr| on
    every row, checked on the CPU); width 1 gives exactly 0; a row alone
    equals itself in the batch."""
    x = K.snr_rows(nbin, thr)
    wd = K.width_of(nbin)
    ex = R.profile_snr_exact(x, wd, thr)
    got = _snr(gpu, x, wd, thr)
    if wd == 1:
        np.testing.assert_array_equal(got, 0.0)
    else:
        print(nbin, thr, "max err / bound", (np.abs(got - ex["snr"]) / ex["bound"]).max())
        assert (np.abs(got - ex["snr"]) <= ex["bound"]).all()
    for r in (0, len(x) - 1):
        assert _snr(gpu, x[r:r + 1], wd, thr)[0] == got[r]


@pytest.mark.parametrize("nbin", K.SNR_NBINS)
def test_profile_snr_integer_rows_all_thresholds(gpu, nbin):
    """Thresholds 0.0, 0.1 and 0.49 on rows whose sums are exact on the
    device: at 0.0 the upper crossing is the exact tie c = C at the last bin
    before the window, which only exact sums decide."""
    x = K.integer_snr_rows(nbin)
    wd = K.width_of(nbin)
    for thr in K.SNR_THRESHOLDS:
        ex = R.profile_snr_exact(x, wd, thr)
        got = _snr(gpu, x, wd, thr)
        if wd == 1:
            np.testing.assert_array_equal(got, 0.0)
        else:
            assert (np.abs(got - ex["snr"]) <= K.INTEGER_SNR_ULPS * R.U * ex["snr"]).all(), thr


def test_profile_snr_zero_total(gpu):
    """C > 0 is required: 0, 10, 0, 10, ... with an even width has a positive
    variance and C exactly 0, so the S/N is 0.  (A negative C cannot be built
    from finite data: m is the smallest window mean, never above the row's.)"""
    z = K.zero_total_row()
    assert _snr(gpu, z[None], 10)[0] == 0.0


# ---------------------------------------------------------------------------
# tscrunch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.TSCRUNCH_CASES, ids=lambda c: "x".join(map(str, c)))
def test_tscrunch_vs_exact(gpu, case):
    """Values within (nsub + 2) u sum|w d| / sum w (tscrunch_bound); wsum the
    in-order sum of the weights; an unweighted channel gives exactly 0 and
    wsum 0; NaN samples under a zero weight are skipped, not multiplied by 0."""
    npol, nsub, nbin = case
    d, w = K.tscrunch_case(*case)
    want, wsum = R.tscrunch_exact(d, w)
    out, ws = gpu.tscrunch(d, w)
    out, ws = out.cpu().numpy()[0], ws.cpu().numpy()[0]
    run = np.zeros(4)
    for s in range(nsub):
        run = run + w[s]
    np.testing.assert_array_equal(ws, run)
    np.testing.assert_array_equal(ws, wsum)
    assert np.isfinite(out).all()
    assert (out[:, 1] == 0.0).all() and ws[1] == 0.0
    bound = R.tscrunch_bound(d, w)
    live = bound > 0
    print(case, "max err / bound", (np.abs(out - want)[live] / bound[live]).max() if live.any()
          else 0.0)
    assert (np.abs(out - want) <= bound).all()
    if nsub > 1:  # the NaN subint's channel: the average over the other subints
        o2, _ = gpu.tscrunch(d[1:, :, 2:3], w[1:, 2:3])
        np.testing.assert_array_equal(out[:, 2:3], o2.cpu().numpy()[0])


# ---------------------------------------------------------------------------
# unpack
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nbin", [1, 255, 256, 257])
@pytest.mark.parametrize("dtype", ["uint8", "int16", "float32"])
def test_unpack_bitwise(gpu, dtype, nbin):
    """With float32-valued DAT_SCL and DAT_OFFS raw * scl has at most 48
    significant bits: the device's one fma equals numpy's raw * scl + offs bit
    for bit.  npol 4 (pmode 1 takes the second of four polarisations), the
    sample types' extremes, nbin around one block."""
    import torch
    raw, scl, offs = K.unpack_case(dtype, nbin)
    if dtype != "float32":
        info = np.iinfo(dtype)
        assert (raw == info.min).any() and (raw == info.max).any()
    phys = raw.astype(np.float64) * scl[..., None] + offs[..., None]
    dev = gpu.device
    for pmode in (0, 1, 2):
        out = gpu.unpack_subints(torch.as_tensor(raw, device=dev), torch.as_tensor(scl, device=dev),
                                 torch.as_tensor(offs, device=dev), pmode).cpu().numpy()
        want = phys if pmode == 0 else (phys[:, :1] + phys[:, 1:2] if pmode == 1 else phys[:, :1])
        np.testing.assert_array_equal(out, want)


# ---------------------------------------------------------------------------
# load_data: coherence data, pscrunch=False, rm_baseline=True (ntot = 2)
# ---------------------------------------------------------------------------
def test_load_data_coherence_rm_baseline(gpu, tmp_path):
    """A coherence PSRFITS file loaded with pscrunch=False, rm_baseline=True
    equals remove_baseline_exact(ntot=2) of the same file loaded without the
    baseline step.  (A PSRFITS source reports its POL_TYPE, AABBCRCI, as the
    state; load_data once took only the name Coherence for AA + BB and found
    this file's window on AA alone.)"""
    from pulseportraiture_amd import archive
    from tests.test_gpu_psrfits import _coherence_archive
    path = str(tmp_path / "c.fits")
    _, raw, scl, offs, wts = _coherence_archive(path, **K.E2E_SHAPE)
    d0 = archive.load_data(path, pscrunch=False, rm_baseline=False, quiet=True)
    d1 = archive.load_data(path, pscrunch=False, rm_baseline=True, quiet=True)
    sub = np.asarray(d0.subints)
    phys = raw.astype(np.float64) * scl[..., None].astype(np.float64) + \
        offs[..., None].astype(np.float64)
    np.testing.assert_array_equal(sub, phys)  # what the CPU file checked the margins of
    assert sub.shape[1] == 4 and d1.baseline_removed
    wd = K.width_of(sub.shape[-1])
    _, starts, _ = R.remove_baseline_exact(sub, d0.weights, 2, wd)
    err = R.remove_baseline_error(np.asarray(d1.subints), sub, starts, wd)
    assert (err <= R.remove_baseline_bound(sub, wd)).all()
    # the same values registered in memory under PSRCHIVE's name of the state
    reg = {k: d0[k] for k in ["freqs", "weights", "Ps", "epochs", "DM", "dmc", "backend",
                              "frontend", "backend_delay", "telescope", "telescope_code", "bw",
                              "nu0", "subtimes", "source"]}
    reg.update(subints=sub, state="Coherence", baseline_removed=False)
    archive.register_archive("prep_coherence", reg)
    try:
        d2 = archive.load_data("prep_coherence", rm_baseline=True, quiet=True)
    finally:
        archive.unregister_archive("prep_coherence")
    np.testing.assert_array_equal(np.asarray(d2.subints), np.asarray(d1.subints))


# ---------------------------------------------------------------------------
# NaN: last, on the guarded arg-min only
# ---------------------------------------------------------------------------
def test_nan_channel_remove_baseline(gpu):
    """One weighted channel of the total is all NaN in subint 0: every window
    sum is NaN, the window is 0, the subint's other rows are de-meaned over
    it, the NaN rows stay NaN, the other subints are untouched bitwise."""
    case = (100, 2, 2, 3)
    d, w = K.baseline_case(*case)
    clean, _ = _remove(gpu, d, w, 2)
    d[0, 1, 2] = np.nan
    _, starts, _ = R.remove_baseline_exact(d, w, 2, 15)
    assert starts[0] == 0
    got, win = _remove(gpu, d, w, 2)
    np.testing.assert_array_equal(win, starts)
    assert np.isnan(got[0, 1, 2]).all()
    np.testing.assert_array_equal(got[1:], clean[1:])
    keep = np.ones((2, 3), bool)
    keep[1, 2] = False
    fin = np.where(np.isnan(d), 0.0, d)
    err = R.remove_baseline_error(np.where(np.isnan(got), 0.0, got), fin, starts, 15)
    assert (err[0][keep] <= R.remove_baseline_bound(fin, 15)[0][keep]).all()
    # the same channel NaN under a zero weight: the finite rows get the window
    # and the baseline they would get without it
    d2, w2 = K.baseline_case(*case)
    ref, rwin = _remove(gpu, d2, w2, 2)
    d2[2, :, 1] = np.nan  # channel 1 of subint 2 has weight 0
    got2, win2 = _remove(gpu, d2, w2, 2)
    np.testing.assert_array_equal(win2, rwin)
    assert np.isnan(got2[2, :, 1]).all()
    ok = ~np.isnan(d2)
    np.testing.assert_array_equal(got2[ok], ref[ok])


def test_nan_rows_profile_snr(gpu):
    """An all-NaN row beside finite rows gives 0 and leaves the others as
    they are alone; a row with a few NaN bins keeps a finite window and
    gives 0 (C is NaN)."""
    x = K.snr_rows(100)[:3].copy()
    alone = np.array([_snr(gpu, x[r:r + 1], 15)[0] for r in range(3)])
    x[1] = np.nan
    x[2, 40:43] = np.nan
    got = _snr(gpu, x, 15)
    assert got[0] == alone[0] and got[1] == 0.0 and got[2] == 0.0
    assert not np.isnan(got).any()
