#!/usr/bin/env python3
"""Generate the wide (more than 2,048 channels) ppspline fixture from the
reference PulsePortraiture source.

TEST INFRASTRUCTURE ONLY, run in the build container like
make_golden_ppspline.py, whose loader, input, stub and runner it imports: the
reference's make_spline_model (smooth=False, try_nlevels=0) on a 2,112-channel
portrait.  The candidate shapes are walked in order and the first for which
the reference keeps at least one eigenvector (ncomp >= 1) is the fixture.

Only numbers are written (no reference text), and not the input portrait:
make_input regenerates it from its seeds, which
tests/test_ppspline_wide_golden_cpu.py pins.
  ppspline_wide.npz   SNRs, noise_stds, pca_weights, mean_prof, eigval,
                      eigvec10, basis (= eigvec[:, ieig]), proj_port, t, c and
                      modelx at every 32nd channel
  ppspline_wide.json  the kept case, ieig / ncomp / ier / k

Usage:  python tests/golden/make_golden_ppspline_wide.py
"""
import json
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402
from make_golden_ppspline import load_ppspline, make_input, make_stub, run, spline_arrays  # noqa: E402

# (nchan, nbin, sigma), tried in this order
CANDIDATES = [(2112, 64, 0.002), (2112, 128, 0.002), (2112, 256, 0.002)]
CHAN_STEP = 32  # modelx is stored at channels 0, 32, 64, ...


def main():
    tmp, pplib, _, _, _ = make_golden.load_reference()
    ppspline = load_ppspline(tmp)
    tried = []
    for nchan, nbin, sigma in CANDIDATES:
        freqs, port = make_input(nchan, nbin, sigma)
        stub, inp = make_stub(pplib, freqs, port)
        run(ppspline, stub)
        tried.append(dict(nchan=nchan, nbin=nbin, sigma=sigma, ncomp=int(stub.ncomp)))
        print("%dx%d" % (nchan, nbin), "ieig", list(stub.ieig), "ier", stub.ier)
        if stub.ncomp >= 1:
            break
    else:
        raise SystemExit("no candidate gives ncomp >= 1: %r" % tried)
    t, c, k = spline_arrays(stub)
    ieig = [int(i) for i in stub.ieig]
    arrs = dict(SNRs=inp["SNRs"], noise_stds=inp["noise_stds"],
                pca_weights=stub.SNRsxs / stub.SNRsxs.sum(), mean_prof=stub.mean_prof,
                eigval=stub.eigval, eigvec10=stub.eigvec[:, :10].T.copy(),
                basis=np.ascontiguousarray(stub.eigvec[:, ieig]),
                proj_port=np.asarray(stub.proj_port), t=t, c=c,
                modelx_sub=stub.modelx[::CHAN_STEP].copy())
    assert np.array_equal(stub.model, stub.modelx)  # no channel is zapped
    meta = dict(nchan=nchan, nbin=nbin, sigma=sigma, tried=tried, ieig=ieig, ncomp=int(stub.ncomp),
                k=k, ier=int(stub.ier), fp=float(stub.fp), chan_step=CHAN_STEP,
                datafile=stub.datafile, source=stub.source, model_name=stub.model_name)
    make_golden.save("ppspline_wide.npz", **arrs)
    with open(os.path.join(HERE, "ppspline_wide.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    size = sum(os.path.getsize(os.path.join(HERE, n))
               for n in ("ppspline_wide.npz", "ppspline_wide.json"))
    assert size < 1000000, size
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
