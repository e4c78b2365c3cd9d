"""ppalign.add_archives, palign_phases and pplib.scrunched_profile restated in
host numpy, for the tests to import.  The phase fits and the S/N are the
oracle's fit_phase_shift and profile_snr; every rotation is an explicit
irfft(rfft(x) e^{2 pi i k phase}, n = nbin) (the oracle's rotate_data returns
nbin - 1 samples of an odd-length row and is not used)."""
import numpy as np

from oracle import ppfit_oracle as O


def rotate(x, phase):
    """rotate_rows: x [..., nbin], phase [...] (or a scalar)."""
    x = np.asarray(x, dtype=np.float64)
    nbin = x.shape[-1]
    k = np.arange(nbin // 2 + 1)
    ph = np.asarray(phase, dtype=np.float64)[..., None]
    return np.fft.irfft(np.fft.rfft(x, axis=-1) * np.exp(2j * np.pi * ph * k), n=nbin, axis=-1)


def fscrunch(x, phase, w):
    """rotate_fscrunch: x [nunit, nchan, nbin], phase and w [nunit, nchan]."""
    return (np.asarray(w)[..., None] * rotate(x, phase)).sum(axis=1)


def palign_phases(x, dedisp, w):
    """(phases [nunit], reference unit, phase_errs [nunit]) of the two rounds
    (ppalign.palign_phases); phase_errs are those of the second round's fits."""
    x = np.asarray(x, dtype=np.float64)
    nunit, nchan, nbin = x.shape
    p = fscrunch(x, dedisp, w)
    ustar = int(np.argmax(O.profile_snr(p)))
    ph1 = np.array([O.fit_phase_shift(p[u], p[ustar], Ns=nbin).phase for u in range(nunit)])
    r = rotate(p, ph1).sum(axis=0)
    fits = [O.fit_phase_shift(p[u], r, Ns=nbin) for u in range(nunit)]
    ph2 = np.array([f.phase for f in fits])
    return ph2 - ph2[ustar], ustar, np.array([f.phase_err for f in fits])


def add_units(x, w, phases):
    """out[c] = sum_u w[u, c] rotate(x[u, :, c], phases[u]) / sum_u w[u, c]
    where that sum is positive, zeros elsewhere: x [nunit, npol, nchan, nbin],
    w [nunit, nchan].  Returns (portrait [npol, nchan, nbin], weights [nchan]
    of 1 or 0)."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    rot = rotate(x, np.asarray(phases)[:, None, None])
    tot = (w[:, None, :, None] * rot).sum(axis=0)
    tw = w.sum(axis=0)
    good = tw > 0
    out = np.zeros_like(tot)
    out[:, good] = tot[:, good] / tw[good][None, :, None]
    return out, np.where(good, 1.0, 0.0)


def scrunched_profile(subints, dedisp, w):
    """The T-, P- and F-scrunched profile (pplib.scrunched_profile): subints
    [nsub, nchan, nbin] total intensity, dedisp and w [nsub, nchan]."""
    w = np.asarray(w, dtype=np.float64)
    return fscrunch(subints, dedisp, w).sum(axis=0) / w.sum()
