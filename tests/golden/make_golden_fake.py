#!/usr/bin/env python3
"""The reference's fake-data helpers on one small portrait (fake_pulsar.npz).

TEST INFRASTRUCTURE ONLY -- run in the build container, never on the GPU box
and never by the product.  The reference is loaded through the SURVEY.md
§8(c) shim exactly as in make_golden.py; only numbers are written.

make_fake_pulsar itself needs PSRCHIVE, but the functions it applies to the
model are pure numpy (pplib.py:3345-3370): read_model, add_DM_nu (xs [-2, -4],
Cs [1, 0.1]), the scattering of scattering_times / scattering_portrait_FT and
add_scintillation.  They run here in that order on a noise-free 8 x 64
portrait of examples/example.gmodel, and every stage is kept.

add_scintillation's explicit-parameter branch divides len(params) / 3 for a
range(), which Python 3 refuses, so it runs with its random parameters from a
seeded numpy state; the same draws (uniform, chisquare, uniform per sinusoid,
pplib.py:1170-1171) are repeated from that seed and stored as the explicit
parameters the package is given.

Usage:  python tests/golden/make_golden_fake.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import make_golden as MG  # noqa: E402

NCHAN, NBIN = 8, 64
PHASE, DDM = 0.03, 2e-3
XS, CS = [-2.0, -4.0], [1.0, 0.1]
SCINT_SEED, NSIN, AMAX, WMAX = 7, 2, 1.0, 3.0
T_SCAT, ALPHA, NU0 = 2e-5, -4.0, 1500.0  # [s] at nu0


def main():
    _, pplib, _, _, _ = MG.load_reference()
    freqs = MG.channel_freqs(NCHAN)
    phases = pplib.get_bin_centers(NBIN)
    P = MG.P0
    _, _, model = pplib.read_model(MG.GMODEL, phases, freqs, P, quiet=True)
    dmnu = pplib.add_DM_nu(model, -PHASE, -DDM, P, freqs, XS, CS, np.inf)
    taus = pplib.scattering_times(T_SCAT / P, ALPHA, freqs, NU0)
    scat = np.fft.irfft(pplib.scattering_portrait_FT(taus, NBIN) * np.fft.rfft(dmnu, axis=-1),
                        axis=-1)
    np.random.seed(SCINT_SEED)
    port = pplib.add_scintillation(scat, None, True, NSIN, AMAX, WMAX)
    np.random.seed(SCINT_SEED)
    scint = []  # (amp, cycles, phase) per sinusoid, as drawn above
    for _ in range(NSIN):
        scint += [np.random.uniform(0, AMAX), np.random.chisquare(WMAX), np.random.uniform(0, 1)]
    out = os.path.join(HERE, "fake_pulsar.npz")
    np.savez(out, freqs=freqs, P=P, model=model, phase=PHASE, dDM=DDM, xs=XS, Cs=CS,
             scint=scint, t_scat=T_SCAT, alpha=ALPHA, nu0=NU0, dmnu=dmnu, scat=scat, port=port)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
