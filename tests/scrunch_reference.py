"""Numpy restatement of ppf_scrunch_subints and archive.scrunch (the stand-ins
for pam -f / -b), written from their definition alone (include/ppfit.h):

    W               = sum_{n in g} w[s][n]
    y               = irfft(sum_{n in g, w != 0} w[s][n] rfft(x[s][p][n]) e^{2 pi i k phase[s][n]},
                            nbin) / W
    out[s][p][g][j] = (1/b) sum_{i < b} y[j b + i]
    wout[s][g]      = W

for every subint s, polarisation p and group g of f adjacent channels; a group
with W = 0 gives zeros and weight 0, and a sample under weight 0 is never
read.  Sums over the channels of a group run in channel order, so W and the
group frequencies are the very doubles the package forms."""
import numpy as np

DCONST = 0.000241 ** -1  # the reference's dispersion constant [MHz**2 cm**3 pc**-1 s]


def scrunch(x, w, phase, f=1, b=1):
    """x [nsub, npol, nchan, nbin], w and phase [nsub, nchan] ->
    (out [nsub, npol, nchan / f, nbin / b], wout [nsub, nchan / f])."""
    x, w, phase = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64), \
        np.asarray(phase, dtype=np.float64)
    nsub, npol, nchan, nbin = x.shape
    assert nchan % f == 0 and nbin % b == 0
    ng, nbo = nchan // f, nbin // b
    k = np.arange(nbin // 2 + 1)
    out = np.zeros((nsub, npol, ng, nbo))
    wout = np.zeros((nsub, ng))
    for s in range(nsub):
        for g in range(ng):
            chans = range(g * f, (g + 1) * f)
            W = 0.0
            for n in chans:
                W += w[s, n]
            wout[s, g] = W
            if W == 0.0:
                continue
            for p in range(npol):
                spec = np.zeros(len(k), dtype=np.complex128)
                for n in chans:
                    if w[s, n] != 0.0:
                        spec += w[s, n] * np.fft.rfft(x[s, p, n]) * \
                            np.exp(2j * np.pi * k * phase[s, n])
                y = np.fft.irfft(spec, n=nbin) / W
                out[s, p, g] = y.reshape(nbo, b).sum(axis=1) / b
    return out, wout


def group_freqs(freqs, w, f):
    """sum_n w nu / sum_n w per subint and group, the plain mean of the
    group's frequencies where its weights are all 0; [nsub, nchan / f]."""
    freqs, w = np.asarray(freqs, dtype=np.float64), np.asarray(w, dtype=np.float64)
    nsub, nchan = w.shape
    ng = nchan // f
    out = np.zeros((nsub, ng))
    for s in range(nsub):
        for g in range(ng):
            W = Wnu = 0.0
            for n in range(g * f, (g + 1) * f):
                W += w[s, n]
                Wnu += w[s, n] * freqs[s, n]
            out[s, g] = Wnu / W if W != 0.0 else freqs[s, g * f:(g + 1) * f].mean()
    return out


def group_phases(freqs, w, Ps, DM, f, dedispersed):
    """The rotation [nsub, nchan] archive.scrunch gives each channel: none for
    an archive stored dedispersed, else the dispersion delay between the
    channel and its group's own frequency, in turns."""
    freqs = np.asarray(freqs, dtype=np.float64)
    if dedispersed:
        return np.zeros_like(freqs)
    ref = np.repeat(group_freqs(freqs, w, f), f, axis=1)
    return DCONST * DM * (freqs ** -2.0 - ref ** -2.0) / np.asarray(Ps, dtype=np.float64)[:, None]


def scrunch_bunch(subints, freqs, w, Ps, DM, dedispersed, nchan, nbin):
    """archive.scrunch of stored values: (subints, freqs, weights)."""
    _, _, nchan_in, nbin_in = np.shape(subints)
    f, b = nchan_in // nchan, nbin_in // nbin
    out, wout = scrunch(subints, w, group_phases(freqs, w, Ps, DM, f, dedispersed), f, b)
    return out, group_freqs(freqs, w, f), wout
