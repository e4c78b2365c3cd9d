#!/usr/bin/env python3
"""Byte-for-byte A/B of two libppfit builds over every entry point.

  ab_entry_points.py run OUT.npz      (GPU; library from PPF_LIB)
  ab_entry_points.py cmp A.npz B.npz

`run` calls every Engine method that reaches a ppf_* entry point, on seeded
inputs at the smallest shapes that still take every host path: 11 items of 4
channels (the fit: 8) at nbin 64, the smallest FFT instantiation, and nbin
100, the direct sums (Gaussian fits, joins and the bank at 64 only).  Each
call runs at the default workspace limit and at a limit of 1 byte, where
every chunked site processes one item per chunk.  Stored per call: the
output bytes, or the error text of a call that raises, and, with timing on,
the launch-bracket count of every kernel id the call changed.  `cmp` fails
unless every stored entry is equal.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NITEM, NCHAN, NCHAN_FIT = 11, 4, 8
# fit results that every fitted subint writes in full
FIT_KEYS = ["params", "param_errs", "nu_out", "cov", "scales", "scale_errs", "channel_snrs",
            "chi2", "red_chi2", "snr", "nfev", "status", "errs"]


def _profile(nbin, loc, wid):
    ph = (np.arange(nbin) + 0.5) / nbin
    d = (ph - loc + 0.5) % 1.0 - 0.5
    return np.exp(-0.5 * (d / (wid / 2.3548200450309493)) ** 2)


def _inputs(nbin, nchan, rng):
    freqs = np.linspace(1200.0, 1600.0, nchan)
    model = np.stack([(1.0 + 0.1 * c) * _profile(nbin, 0.5, 0.05 + 0.004 * c) +
                      0.4 * _profile(nbin, 0.62, 0.03) for c in range(nchan)])
    phase = rng.uniform(-0.2, 0.2, (NITEM, nchan))
    shift = np.exp(2j * np.pi * np.arange(nbin // 2 + 1) * phase[..., None])
    data = np.fft.irfft(np.fft.rfft(model)[None] * shift, nbin, axis=-1)
    data = data + 0.02 * rng.standard_normal(data.shape)
    return freqs, model, phase, data


def _flatten(prefix, out, store):
    import torch
    if out is None:
        return
    if isinstance(out, torch.Tensor):
        store[prefix] = out.detach().cpu().numpy()
    elif isinstance(out, dict):
        for k, v in out.items():
            if not k.startswith("_"):
                _flatten(prefix + "/" + k, v, store)
    elif isinstance(out, (tuple, list)):
        for i, v in enumerate(out):
            _flatten("%s/%d" % (prefix, i), v, store)


def calls(eng, nbin, rng):
    """(name, callable) of every entry point at nbin."""
    import torch
    dev = eng.device
    freqs, model, phase, data = _inputs(nbin, NCHAN, rng)
    nh = nbin // 2 + 1
    rows = data.reshape(-1, nbin)           # 44 rows
    rows11 = np.ascontiguousarray(data[:, 0, :])
    row_phase = phase.reshape(-1)
    tau = np.full(rows.shape[0], 0.01)
    weight = rng.uniform(0.5, 1.5, (NITEM, NCHAN))
    midx = (np.arange(rows.shape[0]) % NCHAN).astype(np.int32)
    sub4 = torch.as_tensor(data[:, None], device=dev).contiguous()  # [11, 1, 4, nbin]
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
    c = []
    add = lambda name, fn: c.append(("%s@%d" % (name, nbin), fn))

    add("rotate_rows", lambda: eng.rotate_rows(rows, row_phase))
    add("scatter_rotate_rows", lambda: eng.scatter_rotate_rows(rows, row_phase, tau))
    add("irfft_rows", lambda: eng.irfft_rows(np.fft.rfft(rows, axis=-1), nbin))
    add("noise_rows", lambda: eng.noise_rows(rows))
    add("noise_rows_frac", lambda: eng.noise_rows(rows, frac=3))
    add("noise_fit_rows", lambda: eng.noise_fit_rows(rows, full=True))
    pows = np.abs(np.fft.rfft(rows, axis=-1)) ** 2
    add("find_kc_rows_exp", lambda: eng.find_kc_rows(pows, fn="exp_dc"))
    add("find_kc_rows_tri", lambda: eng.find_kc_rows(pows, errs=np.ones(nh), fn="half_tri"))
    add("resid_chi2_rows", lambda: eng.resid_chi2_rows(
        rows, row_phase, model, np.ones(rows.shape[0]), np.full(rows.shape[0], 0.02), nbin - 2.0,
        tau=tau, model_row=midx))
    add("phase_shift_batch", lambda: eng.phase_shift_batch(rows, model, model_idx=midx))
    add("phase_tau_batch", lambda: eng.phase_tau_batch(rows11, model, model_idx=midx[:NITEM] * 0))
    add("synth", lambda: eng.synth(model, phase, 0.02, 7))
    add("fake_subints", lambda: eng.fake_subints(model, phase, 1.0, 0.02, 7))
    add("fake_subints_packed", lambda: eng.fake_subints(model, phase, 1.0, 0.02, 7, packed=True))
    add("pack_subints", lambda: eng.pack_subints(sub4))

    def unpack():
        raw, scl, offs = eng.pack_subints(sub4)
        return eng.unpack_subints(raw, scl, offs)
    add("unpack_subints", unpack)

    def accumulate():
        acc = torch.zeros((NCHAN, nh, 2), dtype=torch.float64, device=dev)
        keep = eng.rotate_accumulate(t(data), phase, weight, acc)
        torch.cuda.synchronize()
        del keep
        return acc
    add("rotate_accumulate", accumulate)
    add("rotate_fscrunch", lambda: eng.rotate_fscrunch(t(data), phase, weight))
    gpar = [0.0, 0.0, 0.5, 0.0, 0.05, 0.0, 1.0, -0.5, 0.62, 0.0, 0.03, 0.0, 0.4, 0.0]
    add("gaussian_portraits", lambda: eng.gaussian_portraits("000", gpar, 4.0, nbin, freqs, 1400.0))
    spar = list(gpar)
    spar[1] = 1.5
    add("gaussian_portraits_scat",
        lambda: eng.gaussian_portraits("000", spar, 4.0, nbin, freqs, 1400.0))
    eig = np.stack([_profile(nbin, 0.4, 0.1), _profile(nbin, 0.7, 0.2)], 1)
    tck = (np.array([1200.0] * 4 + [1600.0] * 4), rng.standard_normal((2, 4)), 3)
    add("spline_portraits", lambda: eng.spline_portraits(model[0], eig, tck, freqs))
    add("spline_portraits_resample",
        lambda: eng.spline_portraits(model[0], eig, tck, freqs, nbin=164 - nbin))
    irf = dict(DM=30.0, P=0.005, wids=(0.01, 0.02), irf_types=("rect", "gauss"))
    add("instrumental_response_rows",
        lambda: eng.instrumental_response_rows(model, freqs, **irf))
    add("response_table", lambda: eng.response_table(nbin, freqs, **irf))
    add("tscrunch", lambda: eng.tscrunch(sub4, weight))

    def baseline():
        d = sub4.clone()
        win = eng.remove_baseline(d, weight)
        return d, win
    add("remove_baseline", baseline)
    add("profile_snr", lambda: eng.profile_snr(rows))
    for method in ("rows", "gram"):
        add("pca_" + method, lambda method=method: eng.pca_portraits(
            t(data), weight, ncomp=2, method=method))

    def project():
        mean, _, vec, _ = eng.pca_portraits(t(data), weight, ncomp=2, method="rows")
        return eng.pca_project(t(data), mean, vec, reconstruct=True)
    add("pca_project", project)
    nlev = (np.arange(NITEM) % 2 + 1).astype(np.int32)
    fact = np.linspace(0.5, 2.0, NITEM)
    add("wavelet_smooth_rows", lambda: eng.wavelet_smooth_rows(rows11, nlev, fact))
    add("wavelet_objective_rows", lambda: eng.wavelet_objective_rows(rows11, nlev, fact, "soft"))
    add("smart_smooth_rows", lambda: eng.smart_smooth_rows(rows11, 2, table=True))
    return c


def gauss_calls(eng, rng):
    """The Gaussian-component entry points (nbin 64): 2 components, 2 join groups."""
    nbin = 64
    freqs, model, phase, data = _inputs(nbin, NCHAN, rng)
    data = np.broadcast_to(model, data.shape) + 0.02 * rng.standard_normal(data.shape)
    errs = np.full(NCHAN, 0.02)
    par = np.array([0.0, 0.0, 0.5, 0.0, 0.06, 0.0, 1.1, 0.0, 0.62, 0.0, 0.03, 0.0, 0.4, 0.0, 0.0])
    flags = np.array([1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 0])
    jpar = np.concatenate([par[:-1], [0.0, 0.0, 0.01, 0.0], par[-1:]])
    jflags = np.concatenate([flags[:-1], [0, 0, 1, 0], flags[-1:]])
    join_of = np.array([0, 0, 1, 1], dtype=np.int32)
    dm_coef = 4.148808e3 * (freqs ** -2 - 1400.0 ** -2) / 0.005
    g = (data, freqs, errs)
    c = [("gauss_eval@64", lambda: eng.gauss_eval(*g, par, "000", 1400.0)),
         ("gauss_fit@64", lambda: eng.gauss_fit(*g, par, flags, "000", 1400.0, max_nfev=40)),
         ("gauss_eval_join@64", lambda: eng.gauss_eval_join(
             *g, jpar, "000", 1400.0, join_of, dm_coef, 2)),
         ("gauss_fit_join@64", lambda: eng.gauss_fit_join(
             *g, jpar, jflags, "000", 1400.0, join_of, dm_coef, 2, max_nfev=40))]
    resid = data[:, 0, :] - 0.9 * model[0]
    widths = [0.01, 0.02, 0.04, 0.08, 0.16]
    c.append(("gauss_bank@64", lambda: eng.gauss_bank(resid, 0.02, 0.01, widths, full=True)))
    return c


def fit_calls(eng, nbin, rng):
    """ppf_fit_portrait_batch: phase + DM with a guess, the scattering fit by
    trust-ncg, TNC and Newton-CG, the piece pipeline, the tables in HBM and the
    data-spectrum cache with ppf_rotate_accumulate_spec."""
    import torch
    freqs, model, phase, data = _inputs(nbin, NCHAN_FIT, rng)
    nu = [1400.0] * 3
    P = 0.005
    kw = dict(nu_fit=nu, guess=True, guess_Ns=100)

    def fit(flags, init=(0.0, 0.0, 0.0, 0.0, 0.0), **extra):
        out = eng.fit_batch(data, model, freqs, P, list(init), flags, **dict(kw, **extra))
        torch.cuda.synchronize()
        return {k: out[k] for k in FIT_KEYS}

    def piped():
        eng.set_pipeline(2)
        try:
            return fit([1, 1, 0, 0, 0])
        finally:
            eng.set_pipeline(0)

    def wide():
        eng.set_option("hbm_tables", 1)
        try:
            return fit([1, 1, 0, 0, 0])
        finally:
            eng.set_option("hbm_tables", 0)

    def cached():
        cache = eng.spec_cache(NITEM, NCHAN_FIT, nbin)
        first = fit([1, 1, 0, 0, 0], spec_cache=cache)
        again = fit([1, 1, 0, 0, 0], spec_cache=cache)
        acc = torch.zeros((NCHAN_FIT, nbin // 2 + 1, 2), dtype=torch.float64, device=eng.device)
        keep = eng.rotate_accumulate_spec(cache, phase, np.ones_like(phase), acc)
        torch.cuda.synchronize()
        del keep
        return first, again, acc

    scat = dict(init=(0.0, 0.0, 0.0, -2.0, -4.0), log10_tau=True, guess_tau=0.01)
    c = [("fit_phase_dm", lambda: fit([1, 1, 0, 0, 0])),
         ("fit_scat", lambda: fit([1, 1, 0, 1, 0], **scat)),
         ("fit_tnc", lambda: fit([1, 1, 0, 0, 0], method="TNC")),
         ("fit_newton_cg", lambda: fit([1, 1, 0, 0, 0], method="Newton-CG")),
         ("fit_exact", lambda: fit([1, 1, 0, 0, 0], exact=True)),
         ("fit_pipeline", piped), ("fit_hbm_tables", wide), ("fit_spec_cache", cached)]
    return [("%s@%d" % (n, nbin), f) for n, f in c]


def run(out_path):
    import torch
    from pulseportraiture_amd import _lib
    from pulseportraiture_amd.engine import Engine, PPFitError
    eng = Engine(0)
    default_limit = eng.workspace_limit()
    eng.set_timing(True)
    store = {"selftest": np.array(eng.selftest())}
    todo, misuse = [], []
    for nbin in (64, 100):
        rng = np.random.default_rng(20240917 + nbin)
        todo += calls(eng, nbin, rng) + fit_calls(eng, nbin, rng)
    todo += gauss_calls(eng, np.random.default_rng(20240917))
    launches = lambda: np.array([eng.kernel_time(k)[1] for k in _lib.KERNEL_IDS])
    for name, fn in todo:
        for tag, limit in (("default", default_limit), ("limit1", 1)):
            key = "%s/%s" % (name, tag)
            eng.set_workspace_limit(limit)
            before = launches()
            try:
                out = fn()
                torch.cuda.synchronize()
                _flatten(key, out, store)
            except PPFitError as e:
                store[key + "/error"] = np.array(str(e))
                print("%s raised: %s" % (key, e), flush=True)
            except (TypeError, ValueError, IndexError, KeyError, AttributeError) as e:
                misuse.append(key)  # the tool's own call is wrong: no entry point was reached
                print("%s: %s: %s" % (key, type(e).__name__, e), flush=True)
            store[key + "/launches"] = launches() - before
    eng.set_workspace_limit(default_limit)
    np.savez(out_path, **store)
    nerr = sum(k.endswith("/error") for k in store)
    print("saved %s: %d entries of %d calls, %d raised" % (out_path, len(store), len(todo), nerr),
          flush=True)
    if misuse:
        sys.exit("calls that reached no entry point: %s" % ", ".join(misuse))


def cmp(a, b):
    A, B = np.load(a), np.load(b)
    bad = sorted(set(A.files) ^ set(B.files))
    for k in bad:
        print("only in one: %s" % k)
    nerr = 0
    for k in sorted(set(A.files) & set(B.files)):
        x, y = A[k], B[k]
        nerr += k.endswith("/error")
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            bad.append(k)
            print("differs: %s" % k)
    print("%d entries, %d error texts, %d differ" % (len(A.files), nerr, len(bad)))
    print("BITWISE_EQUAL" if not bad else "DIFFER")
    return not bad


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        sys.exit(0 if cmp(sys.argv[2], sys.argv[3]) else 1)
