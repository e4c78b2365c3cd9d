#!/usr/bin/env python3
"""Generate the ppspline fixtures from the reference PulsePortraiture source.

TEST INFRASTRUCTURE ONLY, run in the build container like make_golden.py,
whose shim (load_reference) it reuses: the reference's ppspline.py goes
through the same lib2to3 step into the shim's scratch directory, and its
DataPortrait.make_spline_model / write_model run unbound on a stub `self`
holding the attributes they read (port, portx, freqs, freqsxs, SNRsxs,
noise_stdsxs, bw, masks, datafile, source).  smooth=False and try_nlevels=0:
PyWavelets is not installed, and try_nlevels=0 makes smart_smooth return its
input.

Only numbers are written (no reference text):
  ppspline.npz           inputs, the reference's pca, projections and splines
  ppspline_models.npz    reconst_port and modelx of the default cases
  ppspline_variants.npz  the variants' splines and models
  ppspline.json          shapes, ieig / ncomp / ier / k per case and variant
(three .npz files so that each stays under the repository's file-size limit).

Usage:  python tests/golden/make_golden_ppspline.py
"""
import contextlib
import io
import json
import os
import shutil
import subprocess
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import make_golden  # noqa: E402

# (nchan, nbin, sigma)
CASES = [(32, 256, 0.002), (20, 250, 0.002), (24, 128, 0.002), (16, 64, 0.002), (48, 512, 0.01)]
VARIANT_SHAPES = [(32, 256), (20, 250)]
# name -> (make_spline_model keywords, zapped channels, negative bandwidth)
VARIANTS = {"ncomp2_k5_s0": (dict(max_ncomp=2, k=5, sfac=0), (), False),
            "nbreak3": (dict(max_nbreak=3), (), False),
            "zap_negbw": (dict(), (3, 11), True)}
MODEL_FILE_CASE = (48, 512)


def load_ppspline(tmp):
    shutil.copy(os.path.join(make_golden.REF, "ppspline.py"), tmp)
    subprocess.check_call([sys.executable, "-m", "lib2to3", "-w", "-n", "ppspline.py"], cwd=tmp,
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with contextlib.redirect_stdout(io.StringIO()):
        import ppspline
    return ppspline


def make_input(nchan, nbin, sigma):
    from pulseportraiture_amd import synth
    w = synth.make_workload(1, nchan, nbin, seed=3)
    port = w.model + sigma * np.random.default_rng(5).standard_normal((nchan, nbin))
    return w.freqs, port


def make_stub(pplib, freqs, port, zap=(), negbw=False):
    """The attributes make_spline_model reads, as DataPortrait sets them
    (pplib.py:307-327) for one subint."""
    nchan, nbin = port.shape
    bw = 800.0
    if negbw:
        freqs, port, bw = freqs[::-1].copy(), port[::-1].copy(), -bw
    weights = np.ones(nchan)
    weights[list(zap)] = 0.0
    ok = np.flatnonzero(weights)
    noise = np.array([pplib.get_noise(p) for p in port])
    snrs = np.abs(port).max(axis=1) / noise
    masks = np.einsum("j,k->jk", weights, np.ones(nbin))[None, None]
    s = types.SimpleNamespace()
    s.port = masks[0, 0] * port
    s.portx = s.port[ok]
    s.freqs = freqs[None]
    s.freqsxs = [freqs[ok]]
    s.SNRsxs = snrs[ok]
    s.noise_stdsxs = noise[ok]
    s.bw = bw
    s.masks = masks
    s.datafile = "ppspline_%dx%d.fits" % (nchan, nbin)
    s.source = "J0000+0000"
    inputs = dict(freqs=freqs, port=port, weights=weights, SNRs=snrs, noise_stds=noise, bw=bw)
    return s, inputs


def run(ppspline, stub, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        ppspline.DataPortrait.make_spline_model(stub, smooth=False, quiet=True, try_nlevels=0, **kw)
    return stub


def spline_arrays(stub):
    t, c, k = stub.tck
    c = np.array(c, dtype=np.float64).reshape(stub.ncomp, -1) if stub.ncomp else np.zeros((0, 0))
    return np.asarray(t, dtype=np.float64), c, int(k)


def main():
    tmp, pplib, _, _, _ = make_golden.load_reference()
    ppspline = load_ppspline(tmp)
    base, models, var, meta = {}, {}, {}, {"cases": {}, "variants": {}}
    for nchan, nbin, sigma in CASES:
        key = "%dx%d" % (nchan, nbin)
        freqs, port = make_input(nchan, nbin, sigma)
        stub, inp = make_stub(pplib, freqs, port)
        run(ppspline, stub)
        w = stub.SNRsxs / stub.SNRsxs.sum()
        # the eigenvectors of the PCA alone, as find_significant_eigvec marks them
        with contextlib.redirect_stdout(io.StringIO()):
            ieig_pca = pplib.find_significant_eigvec(stub.eigvec, check_max=10, return_max=10,
                                                     snr_cutoff=150.0, return_smooth=False,
                                                     rchi2_tol=0.1, try_nlevels=0)
        t, c, k = spline_arrays(stub)
        for name, v in inp.items():
            base["%s_%s" % (name, key)] = np.asarray(v)
        base["pca_weights_" + key] = w
        base["mean_prof_" + key] = stub.mean_prof
        base["eigval_" + key] = stub.eigval
        base["eigvec10_" + key] = stub.eigvec[:, :10].T.copy()  # rows
        base["proj_port_" + key] = np.asarray(stub.proj_port)
        base["t_" + key], base["c_" + key] = t, c
        models["reconst_port_" + key] = stub.reconst_port
        models["modelx_" + key] = stub.modelx  # (= model: no channel is zapped)
        assert np.array_equal(stub.model, stub.modelx)
        meta["cases"][key] = dict(nchan=nchan, nbin=nbin, sigma=sigma,
                                  ieig=[int(i) for i in stub.ieig],
                                  ieig_pca=[int(i) for i in ieig_pca], ncomp=int(stub.ncomp), k=k,
                                  ier=None if stub.ier is None else int(stub.ier),
                                  fp=None if stub.fp is None else float(stub.fp),
                                  datafile=stub.datafile, source=stub.source,
                                  model_name=stub.model_name)
        print(key, "ieig", list(stub.ieig), "ieig(pca)", list(ieig_pca), "ier", stub.ier)
        if (nchan, nbin) == MODEL_FILE_CASE:
            path = os.path.join(tmp, "ref_model.spl")
            with contextlib.redirect_stdout(io.StringIO()):
                ppspline.DataPortrait.write_model(stub, path, quiet=True)
            base["model_file_" + key] = np.frombuffer(open(path, "rb").read(), dtype=np.uint8)
        if (nchan, nbin) in VARIANT_SHAPES:
            for vname, (kw, zap, negbw) in VARIANTS.items():
                vstub, vin = make_stub(pplib, freqs, port, zap, negbw)
                run(ppspline, vstub, **kw)
                vk = "%s_%s" % (vname, key)
                t, c, k = spline_arrays(vstub)
                var["t_" + vk], var["c_" + vk] = t, c
                var["modelx_" + vk] = vstub.modelx
                if zap:
                    var["model_" + vk] = vstub.model
                meta["variants"][vk] = dict(case=key, kwargs=kw, zap=list(zap), negbw=negbw,
                                            ieig=[int(i) for i in vstub.ieig],
                                            ncomp=int(vstub.ncomp), k=k, ier=int(vstub.ier))
                print(vk, "ieig", list(vstub.ieig), "nknot", len(t), "ier", vstub.ier)
    for name, arrs in (("ppspline.npz", base), ("ppspline_models.npz", models),
                       ("ppspline_variants.npz", var)):
        make_golden.save(name, **arrs)
        assert os.path.getsize(os.path.join(HERE, name)) < (1 << 20), name
    with open(os.path.join(HERE, "ppspline.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
