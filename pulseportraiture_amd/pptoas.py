"""pptoas drop-in: wideband TOAs/DMs with the fits batched on the GPU.

``GetTOAs(datafiles, modelfile).get_TOAs(...)`` reproduces pptoas.py:81-738:
per archive it builds the per-subint templates, then hands every ok subint
to one ``ppf_fit_portrait_batch`` call (guess, fit and post-fit on device),
and assembles TOA records, Doppler-corrected DMs, flags and the DeltaDM mean
on the host.  Archives come from ``archive.load_data`` (PSRCHIVE is out of
scope; see archive.py).
"""
import gc
import time

import numpy as np

from . import archive as _arch
from . import pplib as _pplib
from .engine import FitPipeline, RawSubints, get_engine
from .mjd import MJD, add_days_parts, epoch_parts
from .pplib import (DataBunch, F0_fact, phase_transform, gen_gaussian_portraits_device,
                    guess_fit_freq, scattering_alpha, scattering_times, weighted_mean, write_TOAs,
                    _noise_rows, _fit_errs)
from .pptoaslib import phase_shifts, report_failure
from .templates import TemplateSource, chan_bw, row_keys
from .toas import TOA, TOABlock, TOAList, FlagColumn, MJDArray  # noqa: F401

max_nfile = 999
rm_baseline = bool(F0_fact)  # pptoas.py:25-29


def _dist_info():
    """(rank, world) of an initialised torch.distributed group, else (0, 1)."""
    try:
        import torch.distributed as dist
    except ImportError:
        return 0, 1
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def _gather_objects(obj, rank, world, to_all=False, dst=0):
    """Every rank's obj, in rank order, on dst (None elsewhere) or on every
    rank (to_all) -- dist.gather_object / all_gather_object without their
    per-object pickles of the payload: obj is pickled with protocol 5, so its
    numpy arrays (a shard's columns: ~3.7 KB per subint at 128 channels)
    leave the pickle stream as out-of-band buffers; each rank's message is
    one flat byte tensor [stream | buffer 0 | buffer 1 | ...] (64-byte
    aligned pieces) moved by tensor collectives -- CPU tensors under gloo,
    device tensors under nccl (RCCL over xGMI) -- and rebuilt on the
    receiving rank with the arrays as views of the received bytes."""
    import pickle
    import torch
    import torch.distributed as dist
    bufs = []
    head = pickle.dumps(obj, protocol=5, buffer_callback=bufs.append)
    views = [b.raw() for b in bufs]
    sizes = [len(head)] + [v.nbytes for v in views]
    offs = np.zeros(len(sizes) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([(n + 63) // 64 * 64 for n in sizes])
    flat = np.empty(int(offs[-1]), dtype=np.uint8)
    flat[:len(head)] = np.frombuffer(head, dtype=np.uint8)
    for v, o in zip(views, offs[1:-1]):
        flat[o:o + v.nbytes] = np.frombuffer(v, dtype=np.uint8)
    del head, bufs, views
    dev = torch.device("cuda", torch.cuda.current_device()) \
        if dist.get_backend() == "nccl" else torch.device("cpu")
    meta = torch.tensor([len(flat), len(sizes)], dtype=torch.int64, device=dev)
    metas = [torch.empty_like(meta) for _ in range(world)]
    dist.all_gather(metas, meta)
    metas = torch.stack(metas).cpu().numpy()
    ltot, lcnt = int(metas[:, 0].max()), int(metas[:, 1].max())
    sz = torch.zeros(lcnt, dtype=torch.int64, device=dev)
    sz[:len(sizes)] = torch.as_tensor(sizes, dtype=torch.int64)
    szs = [torch.empty_like(sz) for _ in range(world)]
    dist.all_gather(szs, sz)
    msg = torch.zeros(ltot, dtype=torch.uint8, device=dev)
    msg[:len(flat)] = torch.from_numpy(flat).to(dev)
    del flat
    if to_all:
        got = [torch.empty_like(msg) for _ in range(world)]
        dist.all_gather(got, msg)
    else:
        got = [torch.empty_like(msg) for _ in range(world)] if rank == dst else None
        dist.gather(msg, got, dst=dst)
        if rank != dst:
            return None
    out = []
    for r in range(world):
        a = got[r].cpu().numpy()
        n = int(metas[r, 1])
        s = szs[r][:n].cpu().numpy()
        o = np.zeros(n + 1, dtype=np.int64)
        o[1:] = np.cumsum((s + 63) // 64 * 64)
        out.append(pickle.loads(a[:s[0]].tobytes(),
                                buffers=[a[o[i]:o[i] + s[i]] for i in range(1, n)]))
        got[r] = None
    return out


_POOL = None


def _pool():
    """The host-thread pool of _par_concat / _par_map (None: one thread)."""
    global _POOL
    from .toas import _host_threads
    nt = min(4, _host_threads())
    if nt < 2:
        return None
    if _POOL is None:
        from concurrent.futures import ThreadPoolExecutor
        _POOL = ThreadPoolExecutor(max_workers=nt, thread_name_prefix="pptoas")
    return _POOL


def _par_map(fn, items):
    """[fn(x) for x in items], the calls on host threads."""
    pool = _pool()
    if pool is None:
        return [fn(x) for x in items]
    return [f.result() for f in [pool.submit(fn, x) for x in items]]


def _par_concat(parts):
    """{key: np.concatenate(pieces)} with the pieces copied into place on a
    few host threads (np.copyto releases the GIL); the same arrays as
    np.concatenate's."""
    pool = _pool()
    if pool is None:
        return {k: np.concatenate(v) for k, v in parts.items()}
    out, jobs = {}, []
    for k, v in parts.items():
        a = np.empty((sum(len(x) for x in v),) + v[0].shape[1:],
                     dtype=np.result_type(*[x.dtype for x in v]))
        o = 0
        for x in v:
            jobs.append(pool.submit(np.copyto, a[o:o + len(x)], x))
            o += len(x)
        out[k] = a
    for j in jobs:
        j.result()
    return out


def _gc_paused(fn):
    """Run fn with Python's cyclic collector paused: get_TOAs makes few
    containers, but a full collection of the caller's heap (a torch process
    holds ~10^5 objects) landing inside the call costs more than the call.
    The young generations are still collected after every fitted piece
    (_collect), so garbage does not accumulate over a long call."""
    import functools

    @functools.wraps(fn)
    def run(*a, **k):
        on = gc.isenabled()
        gc.disable()
        try:
            return fn(*a, **k)
        finally:
            if on:
                gc.enable()
    return run


def fit_pipeline(keys):
    """The batched-fit pipeline get_TOAs submits its pieces to
    (engine.FitPipeline on this process's device).  The CPU tests replace it
    at this boundary with pptoaslib.SyncPipeline over a stand-in fit."""
    return FitPipeline(get_engine(), keys=keys)


def _shard_range(n, rank, world):
    """Contiguous [lo, hi) of n units for rank; sizes differ by at most one."""
    base, extra = divmod(n, world)
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


_LIST_ATTRS = ["obs", "doppler_fs", "nu0s", "nu_fits", "nu_refs", "ok_idatafiles", "ok_isubs",
               "epochs", "MJDs", "Ps", "phis", "phi_errs", "TOAs", "TOA_errs", "DM0s", "DMs",
               "DM_errs", "DeltaDM_means", "DeltaDM_errs", "GMs", "GM_errs", "taus",
               "tau_errs", "alphas", "alpha_errs", "scales", "scale_errs", "snrs",
               "channel_snrs", "profile_fluxes", "profile_flux_errs", "fluxes", "flux_errs",
               "flux_freqs", "red_chi2s", "channel_red_chi2s", "covariances", "nfevals",
               "rcs", "fit_durations", "order", "TOA_list", "zap_channels"]
# what get_channel_fits leaves, by fit kind: one [nsub] entry per fitted archive
_CHANFIT_ATTRS = {
    "nb": ["nb_DMs", "nb_DM_errs", "nb_offsets", "nb_offset_errs", "nb_nu_refs",
           "nb_nu_ref_errs", "nb_red_chi2s"],
    "scat": ["scat_amps", "scat_amp_errs", "scat_indices", "scat_index_errs", "scat_nu_refs",
             "scat_red_chi2s"],
    "spect": ["spect_As", "spect_A_errs", "spect_indices", "spect_index_errs",
              "spect_red_chi2s"]}


class GetTOAs:
    """Measure TOAs and DMs from wideband data (pptoas.py:75-738).

    Under an initialised torch.distributed group the fits are sharded over
    the ranks (get_TOAs); ``gather_to`` says which ranks then hold the
    results: "root" (default) -- rank 0 receives every rank's result arrays
    and assembles all TOAs, the other ranks keep none (write from rank 0);
    "all" -- every rank assembles the same TOAs.  ``read_bytes_max`` bounds
    the bytes of one subint-range read of an archive that materialises its
    data (PSRFITS, .npz): a rank's shard is read and fitted in pieces of at
    most that size (registered in-memory archives are views, read whole).
    ``raw_samples = True`` lets the fits of a PSRFITS archive read its 16-bit
    samples themselves (engine.RawSubints): no fp64 copy of a read piece is
    made, the pieces are sized by the samples' bytes, and the TOAs are those
    of the default path.  It applies when nothing has to process the data
    first (no dedispersion, baseline removal or tscrunch) and the noise is
    the fit's own (pplib.default_noise_method "PS"); otherwise the default
    path runs.  load_data's SNRs (Profile::snr()) still need fp64 profiles:
    they are taken from one scratch tensor of at most ``raw_snr_bytes``
    (default 1 GiB), refilled piece by piece."""
    gather_to = "root"
    read_bytes_max = 8 << 30
    raw_samples = False
    raw_snr_bytes = 1 << 30
    read_raw_pieces = 0  # read pieces whose fits took the samples (diagnostic)
    # device-resident subints of one call are fitted in pieces of these
    # fractions (at least pipeline_min_subints in all), each piece's TOA
    # records built while the next runs; pipeline_depth fits in flight
    pipeline_fracs = (0.7, 0.3)
    pipeline_min_subints = 4096
    pipeline_depth = 1

    def __init__(self, datafiles, modelfile, quiet=False):
        if isinstance(datafiles, (list, tuple)):
            self.datafiles = list(datafiles)
        elif _arch.file_is_type(datafiles, "ASCII"):
            self.datafiles = [ln.strip() for ln in open(datafiles).readlines() if ln.strip()]
        else:
            self.datafiles = [datafiles]
        if len(self.datafiles) > max_nfile:
            raise SystemExit("Too many archives.  See/change max_nfile(=%d)." % max_nfile)
        self.is_FITS_model = _arch.file_is_type(modelfile, "FITS")
        self.modelfile = modelfile
        self._templates = None
        for a in _LIST_ATTRS + sum(_CHANFIT_ATTRS.values(), []):
            setattr(self, a, [])
        self.TOA_list = TOAList()
        self.instrumental_response_dict = self.ird = {"DM": 0.0, "wids": [], "irf_types": []}
        self.quiet = quiet

    @property
    def templates(self):
        """The TemplateSource of modelfile (templates.py), parsed on first use.
        It builds Gaussian portraits with this module's gen_gaussian_portraits_
        device: like fit_pipeline, the boundary where the CPU tests put the
        host restatement in place of the device."""
        if self._templates is None:
            self._templates = TemplateSource(self.modelfile, self.is_FITS_model,
                                             gen_gaussian_portraits_device)
        return self._templates

    def _irf_active(self):
        return bool(getattr(self, "add_instrumental_response", False)) and \
            bool(self.ird["DM"] or len(self.ird["wids"]))

    # -- per-subint templates (policy here, mechanism in templates.py) -------
    def _models(self, data, fit_scat, uniform_freqs=False):
        """get_TOAs' templates (pptoas.py:323-393) and each subint's index into
        them, or None on an archive template's nbin/nchan mismatch: the model
        with the subint's own P, unscattered under fit_scat, one per distinct
        frequency row (and P when TAU is in bins of P); then the response
        with that P and the chan_bw of the ok channels, at every channel
        (masked ones are not fitted), one per distinct (template, frequency
        row, chan_bw, P when ird["DM"])."""
        src = self.templates
        ok = np.asarray(data.ok_isubs)
        idx = np.zeros(data.nsub, dtype=np.int32)
        if src.kind == "fits":
            md, model = src.fits(data.nchan)
            if md.nbin != data.nbin or md.nchan != data.nchan:  # pptoas.py:329-338
                return None
            models = np.asarray(model)[None]
        else:
            self.model_name = src.name
            tau_P = False
            if src.kind == "gmodel":
                self.ngauss = src.ngauss
                if fit_scat:
                    self.model_code, self.model_nu_ref = src.code, src.nu_ref
                    self.gparams, self.alpha = np.copy(src.gparams), src.alpha
                tau_P = src.gparams[1] != 0 and not fit_scat
            if uniform_freqs and not tau_P:
                first, inv = np.zeros(1, dtype=np.int64), np.zeros(len(ok), dtype=np.int64)
            else:
                keyrows = data.freqs[ok]
                if tau_P:
                    keyrows = np.concatenate([keyrows, data.Ps[ok][:, None]], axis=1)
                first, inv = row_keys(keyrows)
            idx[ok] = inv
            models = src.portraits(data.freqs[ok[first]], len(data.phases), data.Ps[ok[first]],
                                   scattered=not fit_scat)
        if self._irf_active():
            ird, P = self.ird, data.Ps[ok]
            cbw = np.array([chan_bw(data.freqs[i, data.ok_ichans[i]]) for i in ok])
            first, inv = row_keys(np.column_stack([idx[ok], data.freqs[ok], cbw,
                                                   P if ird["DM"] else 0 * P]))
            models = np.stack([src.respond(models[idx[ok[j]]], data.freqs[ok[j]], P[j], cbw[j],
                                           ird) for j in first])
            idx[ok] = inv
        return models, idx

    @staticmethod
    def _channel_rows(data, isubs, skip_channels=None):
        """Every ok channel of subints isubs, in (isub, ok channel) order: the
        data rows [n, nbin], their load_data noise (nan where the archive has
        none) and the subint and channel index of each; skip_channels
        ([nchan] bool) drops those channels."""
        chans = [np.asarray(data.ok_ichans[i], dtype=np.int64) for i in isubs]
        isub = np.repeat(np.asarray(isubs, dtype=np.int64), [len(c) for c in chans])
        ichan = np.concatenate(chans) if chans else np.zeros(0, dtype=np.int64)
        if skip_channels is not None:
            keep = ~skip_channels[ichan]
            isub, ichan = isub[keep], ichan[keep]
        ns = data.get("noise_stds")
        noise = np.full(len(isub), np.nan) if ns is None else np.asarray(ns)[isub, 0, ichan]
        return np.asarray(data.subints)[isub, 0, ichan], noise, isub, ichan

    def _open(self, datafile, tscrunch, quiet, rm_base=None):
        """open_archive as get_TOAs loads (pptoas.py:250-264): no
        dedispersion; a dedispersed archive (dmc = 1) is reopened with
        dededisperse=True."""
        rb = rm_baseline if rm_base is None else rm_base
        a = _arch.open_archive(datafile, dedisperse=False, dededisperse=False, tscrunch=tscrunch,
                               pscrunch=True, rm_baseline=rb, quiet=quiet)
        if a.meta.dmc:
            if not quiet:
                print("%s is dedispersed (dmc = 1).  Reloading it." % datafile)
            a = _arch.open_archive(datafile, dedisperse=False, dededisperse=True,
                                   tscrunch=tscrunch, pscrunch=True, rm_baseline=rb,
                                   quiet=quiet)
        return a

    def _load(self, datafile, tscrunch, quiet, rm_base):
        """load_data as the reference's drivers call it (pptoas.py:808-820,
        1329-1344): reloaded with dededisperse=True when dmc = 1."""
        a = self._open(datafile, tscrunch, quiet, rm_base)
        b = DataBunch(**dict(a.meta))
        sub = a.read()
        if b.get("snr_deferred"):  # load_data's SNRs (pplib.py:2762-2770)
            b.SNRs = a.snrs(sub)
            b.snr_deferred = False
        b.subints = _arch.host_array(sub)
        return b

    @_gc_paused
    def get_TOAs(self, datafile=None, tscrunch=False, nu_refs=None, DM0=None, bary=True,
                 fit_DM=True, fit_GM=False, fit_scat=False, log10_tau=True, scat_guess=None,
                 fix_alpha=False, print_phase=False, print_flux=False, print_parangle=False,
                 add_instrumental_response=False, addtnl_toa_flags={}, method="trust-ncg",
                 bounds=None, nu_fits=None, show_plot=False, quiet=None):
        """pptoas.py:150-738 with the subint loop batched on the device.

        Every archive is opened for its metadata first (no DATA read); the
        (archive, subint) units in get_TOAs order are split into contiguous
        shards, one per rank of an initialised torch.distributed group, and a
        rank reads only the subint range of its shard (pptoas.py:246,343 is the
        loop being sharded).  Fits are submitted per archive and flag set, a
        large one in pieces (``pipeline_fracs``), through ``fit_pipeline``
        (engine.FitPipeline): the device fits piece i + 1 while the host turns
        piece i's results into records and text.  Every rank turns its own
        shard's results into columns -- the per-subint arrays and a TOABlock
        of its TOA records, with the .tim text already formatted when there
        is more than one rank -- and only those finished columns travel: to
        rank 0 (``gather_to`` "root", default), which concatenates them in
        unit order into the per-archive lists and TOA_list, or to every rank
        ("all").  With "root" the other ranks add nothing to their lists
        (their shard's blocks stay in ``shard_blocks``)."""
        if quiet is None:
            quiet = self.quiet
        warning = "You are using an experimental functionality of pptoas!"
        self.nfit = 1 + int(fit_DM) + int(fit_GM) + 2 * int(fit_scat) - int(fix_alpha)
        self.fit_phi, self.fit_DM, self.fit_GM = True, fit_DM, fit_GM
        self.fit_tau = self.fit_alpha = fit_scat
        if fit_scat:
            self.fit_alpha = not fix_alpha
        self.fit_flags = [int(self.fit_phi), int(self.fit_DM), int(self.fit_GM),
                          int(self.fit_tau), int(self.fit_alpha)]
        self.log10_tau = log10_tau
        if not fit_scat:
            self.log10_tau = log10_tau = False
        if (self.fit_GM or fit_scat) and not quiet:
            print(warning)
        self.scat_guess = scat_guess
        self.DM0, self.bary = DM0, bary
        self.tscrunch = tscrunch
        self.add_instrumental_response = add_instrumental_response
        self._fit_flags_prev = None  # the reference's loop-carried fit_flags
        start = time.time()
        self.phase_s = tm = {}  # wall time per phase of this call (diagnostic)
        clock = time.perf_counter

        def mark(k, t0):
            tm[k] = tm.get(k, 0.0) + clock() - t0
            return clock()
        t = clock()
        datafiles = self.datafiles if datafile is None else [datafile]
        # 1. metadata of every archive (all ranks; no DATA read)
        jobs = []
        n_ok0 = len(self.ok_idatafiles)
        for iarch, datafile in enumerate(datafiles):
            try:
                t = clock()
                arch = self._open(datafile, tscrunch, quiet)
                meta = arch.meta
                t = mark("open", t)
                if not len(meta.ok_isubs):
                    if not quiet:
                        print("No subints to fit for %s.  Skipping it." % datafile)
                    continue
                self.ok_idatafiles.append(iarch)
            except RuntimeError:
                if not quiet:
                    print("Cannot load_data(%s).  Skipping it." % datafile)
                continue
            name = datafile if isinstance(datafile, str) else meta.filename
            job = self._prepare(name, meta, nu_refs, nu_fits, fit_scat, method, bounds, quiet)
            t = mark("prepare", t)
            if job is not None:
                job.arch = arch
                jobs.append(job)
        # 2. shard the units, read and fit this rank's subints, and turn the
        # results into columns (arrays + TOA records) on this rank
        rank, world = _dist_info()
        counts = [len(j.ok_isubs) for j in jobs]
        lo, hi = _shard_range(int(sum(counts)), rank, world)
        shards, durations, off = {}, {}, 0
        pipe = None
        pend = {}  # piece id -> [ij, a0, nsubs, groups left, result arrays]
        for ij, job in enumerate(jobs):
            a0, a1 = max(lo, off) - off, min(hi, off + counts[ij]) - off
            off += counts[ij]
            if a1 <= a0:
                continue
            if pipe is None:
                pipe = fit_pipeline(_RESULT_KEYS)
            t = clock()
            pa0 = a0
            for rsubs in self._read_pieces(job, job.ok_isubs[a0:a1]):
                s_lo, sub, errs = self._read(job, rsubs, fit_scat)
                t = mark("read", t)
                for subs in self._pipe_split(rsubs, sub):
                    self._submit(pipe, pend, (ij, pa0), job, subs, s_lo, sub, errs, fit_scat,
                                 method)
                    pa0 += len(subs)
                    t = mark("submit", t)
                    while len(pipe) > self.pipeline_depth:
                        self._collect(pipe, pend, jobs, shards, durations,
                                      (print_phase, print_flux, print_parangle,
                                       addtnl_toa_flags), mark)
                        t = clock()
        while pipe is not None and len(pipe):
            self._collect(pipe, pend, jobs, shards, durations,
                          (print_phase, print_flux, print_parangle, addtnl_toa_flags), mark)
        self.shard_blocks = [sh.block for ij in sorted(shards) for sh in shards[ij]]
        # 3. gather the finished columns: to rank 0 (gather_to "root") or to
        # every rank ("all")
        t = clock()
        if world > 1:
            got = _gather_objects((shards, durations), rank, world,
                                  to_all=self.gather_to == "all")
            if got is None:  # gather_to "root": the results live on rank 0
                del self.ok_idatafiles[n_ok0:]
                return
            shards, spans = {}, {}
            for s_r, d_r in got:
                for ij, v in s_r.items():
                    shards.setdefault(ij, []).extend(v)
                for ij, sp in d_r.items():  # summed over the ranks fitting the archive
                    spans[ij] = spans.get(ij, 0.0) + sp[1] - sp[0]
        else:
            spans = {ij: sp[1] - sp[0] for ij, sp in durations.items()}
        t = mark("gather", t)
        for ij, job in enumerate(jobs):
            self._finish(job, sorted(shards[ij], key=lambda v: v.a0), spans.get(ij, 0.0), quiet)
        mark("finish", t)
        tot = time.time() - start
        if not quiet and len(self.ok_isubs):
            n = np.array([len(x) for x in self.ok_isubs]).sum()
            print("--------------------------")
            print("Total time: %.2f sec, ~%.4f sec/TOA" % (tot, tot / n))

    def get_narrowband_TOAs(self, datafile=None, tscrunch=False, fit_scat=False,
                            log10_tau=True, scat_guess=None, print_phase=False,
                            print_flux=False, print_parangle=False,
                            add_instrumental_response=False, addtnl_toa_flags={},
                            method="trust-ncg", bounds=None, show_plot=False, quiet=None):
        """Narrowband TOAs: one FFTFIT per channel (pptoas.py:740-1125).

        Every (subint, channel) profile of every archive goes to the device in
        one ppf_phase_shift_batch call (brute force on linspace(-0.5, 0.5,
        100) + Nelder-Mead, pplib.py:2054-2100, with the load_data noise as
        err); TOAs, flags and the per-archive arrays follow the reference.

        fit_scat=True fits a phase and a scattering time per channel instead,
        which the reference announces but leaves commented out
        (pptoas.py:752-753, 982-988): pptoaslib.fit_portrait_full on each
        channel as a one-channel portrait with fit_flags [1, 0, 0, 1, 0] and
        nu_fits = nu_outs = the channel's frequency, all in one
        ppf_phase_tau_batch call (one wave per profile, trust-ncg; any other
        method raises NotImplementedError).  A .gmodel template is built
        unscattered (pptoas.py:896-911).  The starting tau is scat_guess =
        (tau [s], nu_ref, alpha) or else the .gmodel's TAU, scaled to each
        channel's own frequency -- a deliberate departure from the reference's
        set-up, which computes one value per subint at the fit frequency --
        and 1 / nbin where that is 0, for log10 and linear tau alike; the
        starting phase is the cross-correlation peak with the template
        scattered at it (ppfit_nbscat.hip).  nfit is 2 and fit_flags [1, 1]
        (one channel cannot constrain alpha); taus / tau_errs [nsub, nchan]
        hold the fitted parameter (log10 tau or tau, in rotations at the
        channel's frequency), covariances is [nsub, nchan, 2, 2], nfevals and
        rcs are scipy's.  TOAs carry scat_time [us], (log10_)scat_time(_err)
        and scat_ref_freq = the channel's frequency as get_TOAs writes them,
        without a Doppler factor (this method applies none).
        fit_scat=False is the reference's behaviour (tau = 0).  Reference
        quirks kept: channel_red_chi2s[isub] is set to the last channel's
        reduced chi2 for the whole row (pptoas.py:1011); channels whose
        template-archive weight is 0 are skipped (pptoas.py:966).  Where the
        reference cannot run -- a .gmodel template (model_data undefined,
        pptoas.py:966), isub > 0 of a tscrunched template, print_phase
        (results.phi, :1048) and print_flux (fluxes undefined, :1052) -- this
        build uses the template's single weight row, prints the fitted phase
        and prints the per-channel flux estimate.
        """
        if quiet is None:
            quiet = self.quiet
        fit_scat = bool(fit_scat)
        if fit_scat and method != "trust-ncg":
            raise NotImplementedError(
                "get_narrowband_TOAs(fit_scat=True) fits with method='trust-ncg' only, not %r"
                % (method,))
        self.nfit = 1 + int(fit_scat)
        self.fit_phi, self.fit_tau = True, fit_scat
        self.fit_flags = [int(self.fit_phi), int(self.fit_tau)]
        self.log10_tau = log10_tau if fit_scat else False
        if not quiet:
            print("You are using an experimental functionality of pptoas!")
        self.scat_guess = scat_guess
        self.tscrunch = tscrunch
        self.add_instrumental_response = add_instrumental_response
        start = time.time()
        datafiles = self.datafiles if datafile is None else [datafile]
        for iarch, datafile in enumerate(datafiles):
            try:
                data = self._load(datafile, tscrunch, quiet, rm_baseline)
                if not len(data.ok_isubs):
                    if not quiet:
                        print("No subints to fit for %s.  Skipping it." % datafile)
                    continue
                self.ok_idatafiles.append(iarch)
            except RuntimeError:
                if not quiet:
                    print("Cannot load_data(%s).  Skipping it." % datafile)
                continue
            name = datafile if isinstance(datafile, str) else data.filename
            nsub, nchan, nbin = data.nsub, data.nchan, data.nbin
            obs = DataBunch(telescope=data.telescope, backend=data.backend,
                            frontend=data.frontend)
            MJDs = np.array([data.epochs[i].in_days() for i in range(nsub)], dtype=np.double)
            # the model at freqs[isub] with TAU in bins of Ps[isub] (pptoas.py:888-915):
            # one template per distinct (frequency row, P)
            src = self.templates
            ok = np.asarray(data.ok_isubs)
            midx = np.zeros(nsub, dtype=np.int64)
            skip = None
            if src.kind == "fits":
                md, model = src.fits(nchan)
                if md.nbin != nbin:
                    if not quiet:
                        print("Model nbin %d != data nbin %d for %s; skipping it." % (
                            md.nbin, nbin, name))
                    continue
                if md.nchan not in (1, nchan):
                    if not quiet:
                        print("Model nchan %d != data nchan %d for %s; skipping it." % (
                            md.nchan, nchan, name))
                    continue
                skip = np.asarray(md.weights)[0] == 0  # pptoas.py:966
                models = np.asarray(model)[None]
            else:
                if fit_scat and src.kind == "gmodel":
                    self.model_code, self.model_nu_ref = src.code, src.nu_ref
                    self.gparams, self.alpha = np.copy(src.gparams), src.alpha
                first, midx[ok] = row_keys(np.column_stack([data.freqs[ok], data.Ps[ok]]))
                models = src.portraits(data.freqs[ok[first]], nbin, data.Ps[ok[first]],
                                       scattered=not fit_scat)
            if self._irf_active():
                # modelx convolved per subint, with its P and the chan_bw of
                # its ok channels (pptoas.py:920-926)
                models = np.stack([src.respond(
                    models[midx[i]], data.freqs[i], data.Ps[i],
                    chan_bw(data.freqs[i, data.ok_ichans[i]]), self.ird) for i in ok])
                midx[ok] = np.arange(len(ok))
            rows, noise, isub, ichan = self._channel_rows(data, ok, skip)
            mrows = (midx[isub] * nchan + ichan).astype(np.int32)
            where = list(zip(isub.tolist(), ichan.tolist()))
            t0 = time.time()
            out = np.zeros((0, 6))
            tau_out = np.zeros((0, 3))  # t, t_err, cov(phi, t) per row under fit_scat
            rc_out, nfev_out = np.zeros(0, dtype=int), np.zeros(0, dtype=int)
            if len(rows) and fit_scat:
                # the starting tau [rot] at each channel's own frequency
                nu, P_row = data.freqs[isub, ichan], data.Ps[isub]
                if scat_guess is not None:
                    ts, tref, alpha_g = scat_guess
                    tau0 = (ts / P_row) * (nu / tref) ** alpha_g
                elif src.kind == "gmodel":
                    tau0 = (self.gparams[1] / P_row) * (nu / self.model_nu_ref) ** self.alpha
                else:
                    tau0 = np.zeros(len(rows))
                res, rc_d, nfev_d = get_engine().phase_tau_batch(
                    rows, models.reshape(-1, nbin), noise=noise, tau0=tau0,
                    log10_tau=self.log10_tau, model_idx=mrows)
                res = res.cpu().numpy()
                out, tau_out = res[:, [0, 1, 4, 5, 6, 7]], res[:, [2, 3, 8]]
                rc_out, nfev_out = rc_d.cpu().numpy(), nfev_d.cpu().numpy()
            elif len(rows):
                out = get_engine().phase_shift_batch(
                    rows, models.reshape(-1, nbin), noise=noise, Ns=100, bounds=(-0.5, 0.5),
                    model_idx=mrows).cpu().numpy()
            fit_duration = time.time() - t0
            z = lambda *sh: np.zeros(sh, dtype=np.float64)
            phis, phi_errs = z(nsub, nchan), z(nsub, nchan)
            TOAs = np.zeros([nsub, nchan], dtype="object")
            TOA_errs = np.zeros([nsub, nchan], dtype="object")
            taus, tau_errs = z(nsub, nchan), z(nsub, nchan)
            scales, scale_errs, channel_snrs = z(nsub, nchan), z(nsub, nchan), z(nsub, nchan)
            pfl, pfle = z(nsub, nchan), z(nsub, nchan)
            channel_red_chi2s = z(nsub, nchan)
            covariances = z(nsub, nchan, self.nfit, self.nfit)
            nfevals = np.zeros([nsub, nchan], dtype="int")
            rcs = np.zeros([nsub, nchan], dtype="int")
            for j, ((isub, ichan), (phase, phase_err, scale, scale_err, snr, red_chi2)) in \
                    enumerate(zip(where, out)):
                P = data.Ps[isub]
                toa = data.epochs[isub] + MJD(((phase * P) + data.backend_delay) / (3600 * 24.))
                toa_err = phase_err * P * 1e6
                if print_flux:
                    m = models[mrows[j] // nchan][ichan]
                    pfl[isub, ichan] = m.mean() * scale
                    pfle[isub, ichan] = abs(m.mean()) * scale_err
                phis[isub, ichan], phi_errs[isub, ichan] = phase, phase_err
                TOAs[isub, ichan], TOA_errs[isub, ichan] = toa, toa_err
                scales[isub, ichan], scale_errs[isub, ichan] = scale, scale_err
                channel_snrs[isub, ichan] = snr
                channel_red_chi2s[isub] = red_chi2  # the whole row (pptoas.py:1011)
                flags = {"be": data.backend, "fe": data.frontend,
                         "f": data.frontend + "_" + data.backend, "nbin": nbin,
                         "bw": abs(data.bw) / nchan, "subint": isub, "chan": ichan,
                         "tobs": data.subtimes[isub], "tmplt": self.modelfile, "snr": snr,
                         "gof": red_chi2}
                if print_phase:
                    flags["phs"] = phase
                    flags["phs_err"] = phase_err
                if print_flux:
                    flags["flux"] = pfl[isub, ichan]
                    flags["flux_err"] = pfle[isub, ichan]
                if print_parangle:
                    flags["par_angle"] = data.parallactic_angles[isub]
                if fit_scat:
                    tau, tau_err, cov_pt = tau_out[j]
                    taus[isub, ichan], tau_errs[isub, ichan] = tau, tau_err
                    covariances[isub, ichan] = [[phase_err ** 2, cov_pt], [cov_pt, tau_err ** 2]]
                    nfevals[isub, ichan], rcs[isub, ichan] = nfev_out[j], rc_out[j]
                    if self.log10_tau:
                        flags["scat_time"] = 10 ** tau * P * 1e6
                        flags["log10_scat_time"] = tau + np.log10(P)
                        flags["log10_scat_time_err"] = tau_err
                    else:
                        flags["scat_time"] = tau * P * 1e6
                        flags["scat_time_err"] = tau_err * P * 1e6
                    flags["scat_ref_freq"] = data.freqs[isub, ichan]
                for k, v in addtnl_toa_flags.items():
                    flags[k] = v
                self.TOA_list.append(TOA(name, data.freqs[isub, ichan], toa, toa_err,
                                         data.telescope, data.telescope_code, None, None,
                                         flags))
            for attr, val in [("order", name), ("obs", obs), ("doppler_fs", data.doppler_factors),
                              ("ok_isubs", np.asarray(data.ok_isubs)), ("epochs", data.epochs),
                              ("MJDs", MJDs), ("Ps", data.Ps), ("phis", phis),
                              ("phi_errs", phi_errs), ("TOAs", TOAs), ("TOA_errs", TOA_errs),
                              ("taus", taus), ("tau_errs", tau_errs), ("scales", scales),
                              ("scale_errs", scale_errs), ("channel_snrs", channel_snrs),
                              ("profile_fluxes", pfl), ("profile_flux_errs", pfle),
                              ("covariances", covariances),
                              ("channel_red_chi2s", channel_red_chi2s), ("nfevals", nfevals),
                              ("rcs", rcs), ("fit_durations", fit_duration)]:
                getattr(self, attr).append(val)
            if not quiet:
                print("--------------------------")
                print(name)
                print("~%.4f sec/TOA" % (fit_duration / max(len(self.TOA_list), 1)))
        if not quiet and len(self.ok_isubs):
            tot = time.time() - start
            print("--------------------------")
            print("Total time: %.2f sec, ~%.4f sec/TOA" % (tot, tot / max(len(self.TOA_list), 1)))

    # -- fits across the channels of what the drivers left --------------------
    def get_channel_fits(self, nu_ref=None, quiet=None):
        """One measurement per subint from the per-channel values the last
        driver call left, every subint of every fitted archive in one device
        call per kind of fit (pplib.fit_DMs_to_freq_resids, pplib.fit_powlaws):

        - after get_narrowband_TOAs: a DM, an offset [s] and the crossing
          frequency from phis * P with phi_errs * P, over the channels with
          phi_errs > 0 (fit_DM_to_freq_resids) -> nb_DMs, nb_DM_errs,
          nb_offsets, nb_offset_errs, nb_nu_refs, nb_nu_ref_errs, nb_red_chi2s;
        - if that call had fit_scat=True: a power law through the linear
          scattering times [s] (under log10_tau, tau = 10**t P with sigma =
          ln 10 tau t_err), over the channels whose error is finite and > 0,
          from [median tau, pplib.scattering_alpha] -> scat_amps,
          scat_amp_errs, scat_indices, scat_index_errs, scat_nu_refs,
          scat_red_chi2s;
        - after either driver with print_flux=True: a power law through
          profile_fluxes with profile_flux_errs, over the channels with error
          > 0, from [mean flux, 0] -> spect_As, spect_A_errs, spect_indices,
          spect_index_errs, spect_red_chi2s.

        Each list gets one [nsub] entry per fitted archive (the lists are
        rebuilt by every call); subints that were not fitted, and rows with
        fewer than 3 usable channels, are NaN.  nu_ref defaults to each
        archive's nu0.  The lists of a kind that does not apply stay empty; an
        archive left by the other driver than the last gets NaN entries.  The
        drivers' own attributes are not touched."""
        if quiet is None:
            quiet = self.quiet
        narch = len(self.order)
        if not narch:
            raise RuntimeError("get_channel_fits: no fitted archive; run get_TOAs or "
                               "get_narrowband_TOAs first")
        narrow = np.ndim(self.phis[-1]) == 2
        scat = narrow and bool(getattr(self, "fit_tau", False))
        flux = any(np.any(np.asarray(e) > 0.0) for e in self.profile_flux_errs)
        for names in _CHANFIT_ATTRS.values():
            for a in names:
                setattr(self, a, [])
        # the rows: every fitted subint of every archive, padded to the widest
        freqs, nu_refs, nsubs = [], [], []
        for name in self.order:
            meta = self._open(name, getattr(self, "tscrunch", False), True).meta
            freqs.append(np.asarray(meta.freqs, dtype=np.float64))
            nu_refs.append(float(meta.nu0) if nu_ref is None else float(nu_ref))
            nsubs.append(len(freqs[-1]))
        same = [np.ndim(self.phis[i]) == (2 if narrow else 1) for i in range(narch)]
        where = [(i, int(isub)) for i in range(narch) if same[i] for isub in self.ok_isubs[i]]
        nmax = max(f.shape[1] for f in freqs)

        def rows(per_chan, fill):
            out = np.full((len(where), nmax), fill, dtype=np.float64)
            for j, (i, isub) in enumerate(where):
                v = np.asarray(per_chan[i], dtype=np.float64)[isub]
                out[j, :len(v)] = v
            return out

        F = rows(freqs, 1.0)
        P = np.array([self.Ps[i][isub] for i, isub in where], dtype=np.float64)[:, None]
        nu = np.array([nu_refs[i] for i, _ in where], dtype=np.float64)

        def spread(kind, columns):
            for a, col in zip(_CHANFIT_ATTRS[kind], columns):
                vals = [np.full(n, np.nan) for n in nsubs]
                for j, (i, isub) in enumerate(where):
                    vals[i][isub] = col[j]
                getattr(self, a).extend(vals)

        def used_errs(e):
            with np.errstate(invalid="ignore"):
                return np.where(np.isfinite(e) & (e > 0.0), e, 0.0)

        def first_guess(y, e, stat):
            g = np.full(len(y), np.nan)
            for j in range(len(y)):
                if (e[j] > 0.0).any():
                    g[j] = stat(y[j][e[j] > 0.0])
            return g

        with np.errstate(all="ignore"):
            if narrow and len(where):
                e = used_errs(rows(self.phi_errs, 0.0) * P)
                r = _pplib.fit_DMs_to_freq_resids(F, rows(self.phis, 0.0) * P, e)
                spread("nb", [r.DM, r.DM_err, r.offset, r.offset_err, r.nu_ref, r.nu_ref_err,
                              r.red_chi2])
            if scat and len(where):
                t, te = rows(self.taus, 0.0), rows(self.tau_errs, 0.0)
                if self.log10_tau:
                    tau = 10.0 ** t * P
                    sig = np.log(10.0) * tau * te
                else:
                    tau, sig = t * P, te * P
                sig = used_errs(sig)
                init = np.column_stack([first_guess(tau, sig, np.median),
                                        np.full(len(where), _pplib.scattering_alpha)])
                r = _pplib.fit_powlaws(tau, init, sig, F, nu)
                spread("scat", [r.amp, r.amp_err, r.alpha, r.alpha_err, r.nu_ref,
                                r.chi2 / r.dof])
            if flux and len(where):
                y = rows(self.profile_fluxes, 0.0)
                e = used_errs(rows(self.profile_flux_errs, 0.0))
                init = np.column_stack([first_guess(y, e, np.mean), np.zeros(len(where))])
                r = _pplib.fit_powlaws(y, init, e, F, nu)
                spread("spect", [r.amp, r.amp_err, r.alpha, r.alpha_err, r.chi2 / r.dof])
        if not quiet:
            def med(v):
                v = v[np.isfinite(v)]
                return np.median(v) if len(v) else np.nan

            for i, name in enumerate(self.order):
                parts = []
                if self.nb_DMs:
                    parts.append("median narrowband DM = %.6f" % med(self.nb_DMs[i]))
                if self.scat_indices:
                    parts.append("median scattering index = %.3f" % med(self.scat_indices[i]))
                if self.spect_indices:
                    parts.append("median spectral index = %.3f" % med(self.spect_indices[i]))
                print("%s: %s" % (name, "; ".join(parts) if parts else "no channel fits"))

    # -- fitted portraits, residuals and channel zapping --------------------
    def _fitted_rows(self, datafile, isubs, quiet):
        """Inputs of show_fit (pptoas.py:1324-1402) for the subints isubs of
        one fitted archive, as device rows: for every ok channel of every
        subint, the data row, its rotate_portrait_full phase, its template
        row (de-duplicated templates + row index), the fitted scale, the
        scattering time [rot] and the channel noise."""
        ok_files = list(np.array(self.datafiles)[self.ok_idatafiles])
        ifile = ok_files.index(datafile)
        # rm_baseline=True as in show_fit; archives reach this build already
        # loaded (PSRCHIVE's baseline removal is out of scope, archive.py)
        data = self._load(datafile, getattr(self, "tscrunch", False), quiet, True)
        nsub, nchan, nbin = data.nsub, data.nchan, data.nbin
        isubs = np.asarray(isubs, dtype=np.int64)
        # show_fit's template (pptoas.py:1356-1388): unscattered where the
        # fitted tau != 0 (the fit's tau scatters it), else the model with TAU
        # in bins of data.Ps.mean(); one per distinct (frequency row, tau != 0)
        src = self.templates
        midx = np.zeros(nsub, dtype=np.int64)
        models = np.zeros((0, nchan, nbin))
        if src.kind == "fits":
            models = np.asarray(src.fits(nchan)[1], dtype=np.float64)[None]
        elif len(isubs):
            scat = np.asarray(self.taus[ifile])[isubs] != 0.0
            first, midx[isubs] = row_keys(np.column_stack([data.freqs[isubs], scat]))
            f, scat = data.freqs[isubs[first]], scat[first]
            models = np.empty((len(first), nchan, nbin))
            if scat.any():
                models[scat] = src.portraits(f[scat], nbin, scattered=False)
            if not scat.all():
                models[~scat] = src.portraits(f[~scat], nbin, data.Ps.mean())
        if self._irf_active() and len(isubs):
            # the subint's P and the full freqs row (pptoas.py:1382-1388), so
            # chan_bw is |freqs[1] - freqs[0]| over all channels
            models = np.stack([src.respond(models[midx[i]], data.freqs[i], data.Ps[i],
                                           chan_bw(data.freqs[i]), self.ird) for i in isubs])
            midx[isubs] = np.arange(len(isubs))
        phase, tau_ch = np.zeros((nsub, nchan)), np.zeros((nsub, nchan))
        for isub in isubs:
            DM = self.DMs[ifile][isub]
            GM = self.GMs[ifile][isub]
            if self.bary:  # pptoas.py:1348-1350, whatever was fitted
                DM /= self.doppler_fs[ifile][isub]
                GM /= self.doppler_fs[ifile][isub] ** 3
            freqs = data.freqs[isub]
            nu_ref_DM, nu_ref_GM, nu_ref_tau = self.nu_refs[ifile][isub]
            phase[isub] = phase_shifts(self.phis[ifile][isub], DM, GM, freqs, nu_ref_DM,
                                       nu_ref_GM, data.Ps[isub])
            tau = self.taus[ifile][isub]
            if tau != 0.0:
                tau_ch[isub] = scattering_times(10 ** tau if self.log10_tau else tau,
                                                self.alphas[ifile][isub], freqs, nu_ref_tau)
        rows, noise, isub, ichan = self._channel_rows(data, isubs)
        return DataBunch(data=data, ifile=ifile, rows=rows, phase=phase[isub, ichan],
                         models=models.reshape(-1, nbin),
                         model_row=(midx[isub] * nchan + ichan).astype(np.int32),
                         scale=np.asarray(self.scales[ifile])[isub, ichan],
                         tau=tau_ch[isub, ichan], noise=noise,
                         where=list(zip(isub.tolist(), ichan.tolist())))

    def show_fit(self, datafile=None, isub=0, rotate=0.0, show=True, return_fit=False,
                 savefig=False, quiet=None):
        """Fitted portrait and scaled template of one subint (pptoas.py:1310-1412):
        the data rotated by the fitted phi/DM/GM (rotate_portrait_full) and
        the (scattered) template times the fitted channel scales, formed on
        the device.  Plotting (show_residual_plot) is out of scope: show only
        prints a note."""
        if quiet is None:
            quiet = self.quiet
        if datafile is None:
            datafile = self.datafiles[0]
        eng = get_engine()
        fr = self._fitted_rows(datafile, [isub], quiet)
        data = fr.data
        nchan, nbin = data.nchan, data.nbin
        ok = np.asarray(data.ok_ichans[isub])
        port = np.zeros((nchan, nbin))
        model_scaled = np.zeros((nchan, nbin))
        if len(ok):
            port[ok] = eng.scatter_rotate_rows(fr.rows, fr.phase + rotate).cpu().numpy()
            ms = eng.scatter_rotate_rows(fr.models[fr.model_row], np.full(len(ok), rotate),
                                         fr.tau).cpu().numpy()
            model_scaled[ok] = fr.scale[:, None] * ms
        # channels outside ok_ichans stay 0: masked data (port *= masks) and
        # a zero fitted scale
        port *= np.asarray(data.masks[isub, 0])
        if show and not quiet:
            print("show_fit: plotting is not part of this build; use return_fit=True")
        if return_fit:
            ns = data.get("noise_stds")
            noise = ns[isub, 0] if ns is not None else \
                _noise_rows(eng, np.asarray(data.subints)[isub, 0]).cpu().numpy()
            return port, model_scaled, data.ok_ichans[isub], data.freqs[isub], noise

    def get_channels_to_zap(self, SNR_threshold=8.0, rchi2_threshold=1.3, iterate=True,
                            show=False):
        """Flag channels by reduced chi2 and S/N (pptoas.py:1201-1278); needs
        get_TOAs first.  Every ok channel of every ok subint of an archive
        goes to the device in one ppf_resid_chi2_rows call (rotation,
        scattering, scaling and the chi2 sum fused per channel); the
        thresholds and the iterated S/N cut run on the host as there."""
        eng = get_engine()
        for iarch, ok_idatafile in enumerate(self.ok_idatafiles):
            datafile = self.datafiles[ok_idatafile]
            ok_isubs = list(self.ok_isubs[iarch])
            fr = self._fitted_rows(datafile, ok_isubs, True)
            data = fr.data
            chi2 = np.zeros(0)
            if len(fr.where):
                noise = fr.noise
                if np.isnan(noise).any():  # load_data's get_noise on the device
                    est = _noise_rows(eng, fr.rows).cpu().numpy()
                    noise = np.where(np.isnan(noise), est, noise)
                chi2 = eng.resid_chi2_rows(fr.rows, fr.phase, fr.models, fr.scale, noise,
                                           data.nbin - 2, tau=fr.tau,
                                           model_row=fr.model_row).cpu().numpy()
            per_sub = {}
            for (isub, ichan), c in zip(fr.where, chi2):
                per_sub.setdefault(isub, []).append(c)
            channel_red_chi2s, zap_channels = [], []
            for isub in ok_isubs:
                ok_ichans = list(data.ok_ichans[isub])
                red_chi2s = list(per_sub.get(int(isub), []))
                channel_snrs = self.channel_snrs[iarch][isub]
                thr = (SNR_threshold ** 2.0 / len(ok_ichans)) ** 0.5
                bad = []
                for ok_ichan, c in zip(ok_ichans, red_chi2s):
                    if c > rchi2_threshold or np.isnan(c):
                        bad.append(ok_ichan)
                    elif SNR_threshold and channel_snrs[ok_ichan] < thr:
                        bad.append(ok_ichan)
                channel_red_chi2s.append(red_chi2s)
                zap_channels.append(bad)
                if iterate and SNR_threshold and len(bad):
                    old_len = len(bad)
                    added_new = True
                    while added_new and (len(ok_ichans) - len(bad)):
                        thr = (SNR_threshold ** 2.0 / (len(ok_ichans) - len(bad))) ** 0.5
                        for ok_ichan in ok_ichans:
                            if ok_ichan in bad:
                                continue
                            if channel_snrs[ok_ichan] < thr:
                                bad.append(ok_ichan)
                        added_new = bool(len(bad) - old_len)
                        old_len = len(bad)
                if show and len(bad):
                    print("%s, subint: %d  bad chans: %s" % (datafile, isub, bad))
            self.channel_red_chi2s.append(channel_red_chi2s)
            self.zap_channels.append(zap_channels)

    def _prepare(self, datafile, data, nu_ref_tuple, nu_fit_tuple, fit_scat, method, bounds,
                 quiet):
        """Per-archive set-up of pptoas.py:246-484 on the metadata, as arrays:
        templates, reference frequencies, initial parameters and the
        per-subint fit flags."""
        nsub, nchan, nbin = data.nsub, data.nchan, data.nbin
        obs = DataBunch(telescope=data.telescope, backend=data.backend, frontend=data.frontend)
        DM_stored = data.DM
        DM0 = DM_stored if self.DM0 is None else self.DM0
        ep = data.get("epoch_parts") or epoch_parts(data.epochs)
        MJDs = ep[0] + (ep[1] + ep[2]) / 86400.0  # MJD.in_days elementwise
        ok_isubs = np.asarray(data.ok_isubs)
        wn = np.asarray(data.weights) != 0.0
        mask = wn.astype(np.uint8)
        # per-channel rows every ok subint shares (one row to the device,
        # one template key, one guess_fit_freq)
        dense = len(ok_isubs) == nsub

        def okrows(a):
            return a if dense else a[ok_isubs]

        def rows_equal(a):
            a = okrows(a)
            return bool(len(ok_isubs)) and bool((a == a[0]).all())
        # freqs and weights compared on two host threads (numpy releases the
        # GIL); equal weight rows make the mask rows equal too
        ru = _par_map(rows_equal, [data.freqs, data.weights])
        uniform = {"freqs": ru[0], "weights": ru[1], "mask": ru[1] or rows_equal(mask)}
        mm = self._models(data, fit_scat, uniform["freqs"])
        if mm is None:
            if not quiet:
                print("Model nbin/nchan mismatch for %s; skipping it." % datafile)
            return None
        models, midx = mm
        nchx = np.count_nonzero(wn, axis=1)
        allok = nchx == nchan
        # the tobs flag's values: typed when the durations are numbers
        tobs = np.asarray(data.subtimes)
        if tobs.dtype.kind not in "fiu":
            tobs = np.asarray(data.subtimes, dtype=object)
        # reference frequencies (pptoas.py:396-415)
        nu_fits_a = np.zeros((nsub, 3))
        nu_refs_a = np.full((nsub, 3), np.nan)
        if nu_ref_tuple is not None:
            nu_refs_a[ok_isubs] = [nu_ref_tuple[0], nu_ref_tuple[0], nu_ref_tuple[-1]]
            if self.bary and nu_ref_tuple[-1]:
                nu_refs_a[ok_isubs, 2] /= np.asarray(data.doppler_factors)[ok_isubs]
        # initial guesses (pptoas.py:420-456; phi from the device guess)
        init = np.zeros((nsub, 5))
        guess_tau = np.zeros(nsub)
        init[ok_isubs, 1] = DM_stored
        self._nu_fit_and_tau(data, ok_isubs, wn, allok, nu_fit_tuple, fit_scat, nu_fits_a, init,
                             guess_tau, uniform["freqs"])
        # per-subint fit flags (pptoas.py:474-484): get_TOAs keeps one
        # fit_flags list across subints and archives, and a 2-channel subint
        # (fit_DM and fit_GM) zeroes GM in the *previous* subint's list --
        # phase-only after a 1-channel subint, and an UnboundLocalError when no
        # subint came before it.
        ff_all = np.zeros((nsub, 5), dtype=np.int64)
        special = (nchx[ok_isubs] == 1) | ((nchx[ok_isubs] == 2) & bool(self.fit_DM and self.fit_GM))
        if not special.any():
            ff_all[ok_isubs] = self.fit_flags
            self._fit_flags_prev = list(self.fit_flags)
        else:
            for isub in ok_isubs:
                n = nchx[isub]
                if n == 1:
                    ff = [1, 0, 0, 0, 0]
                elif n == 2 and self.fit_DM and self.fit_GM:
                    if self._fit_flags_prev is None:
                        raise UnboundLocalError(
                            "local variable 'fit_flags' referenced before assignment")
                    ff = list(self._fit_flags_prev)
                    ff[2] = 0
                else:
                    ff = list(self.fit_flags)
                self._fit_flags_prev = ff
                ff_all[isub] = ff
        if bounds is None and method == "TNC":
            # get_TOAs' default TNC bounds (pptoas.py:458-467)
            bounds = [(None, None), (None, None), (None, None),
                      (np.log10((10 * nbin) ** -1), None) if self.log10_tau else (0.0, None),
                      (-10.0, 10.0)]
        return _Job(name=datafile, data=data, obs=obs, DM0=DM0, MJDs=MJDs, epoch_parts=ep,
                    ok_isubs=ok_isubs, models=models, midx=midx, mask=mask, wn=wn,
                    nchx=nchx, nu_fits_a=nu_fits_a, nu_refs_a=nu_refs_a, init=init,
                    guess_tau=guess_tau, ff=ff_all, bounds=bounds, allok=allok,
                    nu_fit_tuple=nu_fit_tuple, uniform=uniform, tobs=tobs)

    def _nu_fit_and_tau(self, data, isubs, wn, allok, nu_fit_tuple, fit_scat, nu_fits_a, init,
                        guess_tau, uniform_freqs=False):
        """nu_fit (guess_fit_freq with the channel S/Ns, pptoas.py:396-415)
        and the scattering guess at nu_fit_tau (pptoas.py:420-440) of subints
        isubs, into nu_fits_a / init / guess_tau."""
        if not len(isubs):
            return
        nbin = data.nbin
        if nu_fit_tuple is None:
            nu_fits_a[isubs] = self._guess_fit_freqs(data, isubs, wn, allok,
                                                     uniform_freqs)[:, None]
        else:
            nu_fits_a[isubs] = [nu_fit_tuple[0], nu_fit_tuple[0], nu_fit_tuple[-1]]
        if fit_scat:
            P = data.Ps[isubs]
            nu_fit_tau = nu_fits_a[isubs, 2]
            if self.scat_guess is not None:
                ts, tref, alpha_g = self.scat_guess
                tau_g = (ts / P) * (nu_fit_tau / tref) ** alpha_g
            else:
                alpha_g = self.alpha if hasattr(self, "alpha") else scattering_alpha
                tau_g = (self.gparams[1] / P) * (nu_fit_tau / self.model_nu_ref) ** alpha_g \
                    if hasattr(self, "gparams") else np.zeros(len(isubs))
            tau_g = np.asarray(tau_g, dtype=np.float64) * np.ones(len(isubs))
            guess_tau[isubs] = tau_g
            if self.log10_tau:
                tau_g = np.log10(np.where(tau_g == 0.0, nbin ** -1, tau_g))
            init[isubs, 3] = tau_g
            init[isubs, 4] = alpha_g

    @staticmethod
    def _guess_fit_freqs(data, ok_isubs, wn, allok, uniform_freqs=False):
        """guess_fit_freq(freqsx, SNRsx) of every ok subint (pptoas.py:401,
        pplib.py:2618-2632): once when every such subint has the same
        frequencies, all channels on and the same S/Ns; whole rows at once
        where every channel is on (numpy's row sums are its 1-D sums), the
        compressed rows otherwise."""
        dense = len(ok_isubs) == data.nsub
        f = data.freqs if dense else data.freqs[ok_isubs]
        snr = np.asarray(data.SNRs)[:, 0] if dense else np.asarray(data.SNRs)[ok_isubs, 0]
        alla = bool(allok.all()) if dense else bool(allok[ok_isubs].all())
        if alla and uniform_freqs and (snr == snr[0]).all():
            return np.full(len(ok_isubs), guess_fit_freq(f[0], snr[0]))  # one distinct row
        if uniform_freqs:
            # one frequency row: its terms once, broadcast over the S/N rows
            # (the same elementwise operations on the same values)
            f0 = np.asarray(f[0], dtype=np.float64)
            nu0 = (f0.min() + f0.max()) * 0.5
            f2 = f0 ** -2
            out = nu0 + np.sum((f0 - nu0) * snr * f2, axis=1) / np.sum(snr * f2, axis=1)
        else:
            nu0 = (f.min(axis=1) + f.max(axis=1)) * 0.5
            f2 = f ** -2
            out = nu0 + np.sum((f - nu0[:, None]) * snr * f2, axis=1) / np.sum(snr * f2, axis=1)
        for j in np.flatnonzero(~allok[ok_isubs]):
            isub = ok_isubs[j]
            ok = wn[isub]
            out[j] = guess_fit_freq(data.freqs[isub, ok], np.asarray(data.SNRs)[isub, 0, ok])
        return out

    def _read_pieces(self, job, subs):
        """Split subs (ascending subint indices) into runs whose subint range
        reads at most read_bytes_max bytes (one run for views of registered
        archives)."""
        data = job.data
        if not getattr(job.arch, "owns_reads", True):
            return [subs]
        per = 8 * int(data.npol) * int(data.nchan) * int(data.nbin)
        if len(subs):  # raw samples: the bytes one subint of them holds
            one = self._read_raw(job, int(subs[0]), int(subs[0]) + 1)
            per = one.nbytes if one is not None else per
        span = max(1, int(self.read_bytes_max) // per)
        out, i = [], 0
        while i < len(subs):
            j = int(np.searchsorted(subs, subs[i] + span, side="left"))
            out.append(subs[i:j])
            i = j
        return out

    def _read_raw(self, job, lo, hi):
        """Subints lo:hi as RawSubints when raw_samples applies, else None."""
        from . import pplib
        if not self.raw_samples or pplib.default_noise_method != "PS":
            return None
        read_raw = getattr(job.arch, "read_raw", None)
        return None if read_raw is None else read_raw(lo, hi)

    def _raw_snrs(self, rs):
        """profile_snr of every profile of rs (all polarisations kept by its
        pscrunch mode), [n, npo, nchan] numpy: the values are unpacked into
        one scratch tensor of at most raw_snr_bytes, a piece at a time."""
        import torch
        eng = get_engine()
        n, npol, nchan, nbin = rs.raw.shape
        npo = 1 if rs.pmode else int(npol)
        step = max(1, min(n, int(self.raw_snr_bytes) // (8 * npo * int(nchan) * int(nbin))))
        scratch = torch.empty((step, npo, nchan, nbin), dtype=torch.float64, device=eng.device)
        out = np.empty((n, npo, nchan))
        for a in range(0, n, step):
            b = min(n, a + step)
            piece = eng.unpack_subints(rs.raw[a:b], rs.scl[a:b], rs.offs[a:b], rs.pmode,
                                       out=scratch[:b - a])
            out[a:b] = eng.profile_snr(piece).cpu().numpy()  # waits: the scratch is free again
        return out

    def _read(self, job, subs, fit_scat):
        """Read the subint range of subs (one read piece): (first subint,
        [n, nchan, nbin] numpy or device view -- or the piece's RawSubints
        under raw_samples --, noise rows or None).  A PSRFITS archive's
        deferred SNRs (Profile::snr(), pplib.py:2762-2770) come from the data
        just read, then those subints' nu_fit and scattering guess."""
        data = job.data
        s_lo, s_hi = int(subs[0]), int(subs[-1]) + 1
        rs = self._read_raw(job, s_lo, s_hi)
        if rs is not None:
            self.read_raw_pieces += 1
            full, sub = None, rs
        else:
            full = job.arch.read(s_lo, s_hi)  # [s_hi - s_lo, npol, nchan, nbin], numpy or device
            sub = full[:, 0]
        if data.get("snr_deferred"):
            data.SNRs[s_lo:s_hi] = self._raw_snrs(rs) if rs is not None else \
                get_engine().profile_snr(full).cpu().numpy()
            self._nu_fit_and_tau(data, subs, job.wn, job.allok, job.nu_fit_tuple, fit_scat,
                                 job.nu_fits_a, job.init, job.guess_tau, job.uniform["freqs"])
        ns = data.get("noise_stds")
        return s_lo, sub, None if ns is None else np.asarray(ns)[:, 0]

    def _pipe_split(self, subs, sub):
        """Pipeline pieces of one read piece: host-resident subints in pieces
        of at most STREAM_CHUNK_BYTES (their copies overlap the fits), device-
        resident ones in shrinking fractions (pipeline_fracs) so that the
        host work after the last piece is small."""
        n = len(subs)
        if (_arch._is_tensor(sub) or isinstance(sub, RawSubints)) and sub.device.type != "cpu":
            if n < self.pipeline_min_subints:
                return [subs]
            cuts = np.cumsum([0.0] + list(self.pipeline_fracs))
            cuts = np.unique(np.round(cuts / cuts[-1] * n).astype(int))
        else:
            from .pptoaslib import STREAM_CHUNK_BYTES
            per = 8 * int(np.prod(sub.shape[1:]))
            step = max(1, STREAM_CHUNK_BYTES // per)
            cuts = np.unique(np.append(np.arange(0, n, step), n))
        return [subs[i:j] for i, j in zip(cuts[:-1], cuts[1:]) if j > i]

    def _submit(self, pipe, pend, key, job, subs, s_lo, sub, errs, fit_scat, method):
        """Launch the fits of subints subs (one device call per fit-flag
        group) into the pipeline; piece key = (archive index, a0)."""
        data = job.data
        ffs = job.ff[subs]
        groups = [np.arange(len(subs))] if (ffs == ffs[0]).all() else \
            [np.flatnonzero((ffs == r).all(axis=1)) for r in np.unique(ffs, axis=0)]
        pend[key] = [len(groups), len(subs), None, time.time()]
        for g in groups:
            s = subs[g]
            rel = s - s_lo
            if len(rel) == rel[-1] - rel[0] + 1:  # contiguous: a view
                d = sub[int(rel[0]):int(rel[-1]) + 1]
            else:
                d = sub[rel] if not _arch._is_tensor(sub) else sub[_arch_index(rel, sub)]
            # errs None: the device estimates get_noise_PS per channel, as
            # load_data's noise_stds (pplib.py:2744-2748), or _fit_errs does by
            # another default_noise_method; per-channel rows shared by every
            # subint go as one row
            pipe.submit((key, g, _take(job.nu_fits_a, s)),
                        d, job.models, job.row("freqs", s), _take(data.Ps, s),
                        _take(job.init, s), list(ffs[g[0]]),
                        nu_fit=_take(job.nu_fits_a, s), nu_out=_take(job.nu_refs_a, s),
                        errs=_fit_errs(None, d, None) if errs is None
                        else _take(errs, s),
                        log10_tau=self.log10_tau, option=0, is_toa=True,
                        chan_mask=job.row("mask", s), weights=job.row("weights", s),
                        model_idx=_take(job.midx, s), guess=True, guess_Ns=100,
                        guess_wrap=True, guess_nu=None,
                        guess_tau=_take(job.guess_tau, s) if fit_scat else None,
                        method=method, bounds=job.bounds)

    def _collect(self, pipe, pend, jobs, shards, durations, toa_args, mark):
        """Collect the oldest fit in the pipeline; when its piece is complete,
        turn it into columns on this rank (_shard; its .tim text formatted
        now, while later pieces still run on the device)."""
        t = time.perf_counter()
        (key, g, nu_fit), res = pipe.collect()
        t = mark("wait", t)
        p = pend[key]
        keep = {k: res[k] for k in _RESULT_KEYS if k in res}
        keep["nu_fit"] = nu_fit  # the assembling rank's nu_fits
        if p[0] == 1 and p[2] is None:
            out = keep
        else:
            if p[2] is None:
                p[2] = {k: np.zeros((p[1],) + v.shape[1:], dtype=v.dtype) for k, v in keep.items()}
            for k, v in keep.items():
                p[2][k][g] = v
            out = p[2]
        p[0] -= 1
        if p[0]:
            return
        del pend[key]
        ij, a0 = key
        # the archive's fit wall time on this rank: first submit to last
        # collect (its pieces overlap on the device, so no per-piece sum)
        t0, t1 = durations.get(ij, (p[3], p[3]))
        durations[ij] = (min(t0, p[3]), max(t1, time.time()))
        sh = self._shard(jobs[ij], a0, out, *toa_args)
        t = mark("shard", t)
        sh.block.preformat()  # the .tim text of these records
        mark("preformat", t)
        shards.setdefault(ij, []).append(sh)
        # the collector is paused over get_TOAs (_gc_paused): free this
        # piece's cyclic garbage from the young generations, so a long call
        # (a 125k-subint shard in many pieces) does not pile it up, without
        # a full collection of the caller's heap inside the call
        if not gc.isenabled():
            gc.collect(1)

    def _shard(self, job, a0, res, print_phase, print_flux, print_parangle, addtnl_toa_flags):
        """Columns of ok subints job.ok_isubs[a0:a0 + n] from their device
        results (pptoas.py:522-661), on the rank that fitted them: the
        per-subint values in ok order and a TOABlock of their TOA records
        (flags in the reference's insertion order, pptoas.py:606-661, then
        addtnl_toa_flags)."""
        data, datafile = job.data, job.name
        nchan = data.nchan
        p, e = res["params"], res["param_errs"]
        n = len(p)
        ok = job.ok_isubs[a0:a0 + n]
        status, nfev = res["status"].astype(np.int64), res["nfev"].astype(np.int64)
        for j in np.flatnonzero(~np.isin(status, (0, 1, 2, 4))):
            report_failure(int(status[j]), "%s_%d" % (datafile, ok[j]))
        ff = job.ff[ok]
        P = data.Ps[ok]
        phi, phi_err = p[:, 0], e[:, 0]
        DM, DM_err, GM, GM_err = p[:, 1].copy(), e[:, 1], p[:, 2].copy(), e[:, 2]
        mjd = add_days_parts(tuple(x[ok] for x in job.epoch_parts),
                             ((phi * P) + data.backend_delay) / (3600 * 24.))
        TOA_err = phi_err * P * 1e6
        if self.bary:
            df = np.asarray(data.doppler_factors, dtype=np.float64)[ok]
            DM = np.where(ff[:, 1] != 0, DM * df, DM)
            GM = np.where(ff[:, 2] != 0, GM * df ** 3, GM)
        else:
            df = np.ones(n)
        wn = _take(job.wn, ok)
        wall = bool(wn.all())
        sc = res["scales"] if wall else np.where(wn, res["scales"], 0.0)
        sce = res["scale_errs"] if wall else np.where(wn, res["scale_errs"], 0.0)
        chs = res["channel_snrs"] if wall else np.where(wn, res["channel_snrs"], 0.0)
        nuo = res["nu_out"]
        nf = ff.sum(axis=1)
        cov = res["cov"]
        full = nf == self.nfit
        if full.all():
            covs = np.ascontiguousarray(cov[:, :self.nfit, :self.nfit])
        else:
            covs = np.zeros((n, self.nfit, self.nfit))
            covs[full] = cov[full][:, :self.nfit, :self.nfit]
            for j in np.flatnonzero(~full):
                cm = cov[j][:nf[j], :nf[j]]
                try:  # the reference's assignment, broadcasting a 1x1 block
                    covs[j] = cm
                except ValueError:
                    w = np.where(ff[j])[0]
                    for ii, ifit in enumerate(w):
                        for jj, jfit in enumerate(w):
                            covs[j][ifit, jfit] = cm[ii, jj]
        if wall and job.uniform["freqs"]:  # every row the same: its extremes
            f0 = data.freqs[ok[0]]
            fmax, fmin = np.full(n, f0.max()), np.full(n, f0.min())
        else:
            fo = _take(data.freqs, ok)
            fmax = (fo if wall else np.where(wn, fo, -np.inf)).max(axis=1)
            fmin = (fo if wall else np.where(wn, fo, np.inf)).min(axis=1)
        flux = None
        if print_flux:
            # scattering keeps each row's mean, so the scattered model's
            # channel means are the template's (pptoas.py:553-575)
            pfl, pfle = np.zeros((n, nchan)), np.zeros((n, nchan))
            fluxes, flux_errs, flux_freqs = np.zeros(n), np.zeros(n), np.zeros(n)
            for j, isub in enumerate(ok):
                okc = wn[j]
                means = job.models[job.midx[isub]][okc].mean(axis=1)
                pfl[j, okc] = means * sc[j][okc]
                pfle[j, okc] = abs(means) * sce[j][okc]
                fluxes[j], flux_errs[j] = weighted_mean(pfl[j, okc], pfle[j, okc])
                flux_freqs[j] = weighted_mean(data.freqs[isub, okc], pfle[j, okc])[0]
            flux = (pfl, pfle, fluxes, flux_errs, flux_freqs)
        # TOA records as columns; a flag some rows lack carries a presence mask
        cols = []

        def col(key, vals, present=None):
            if present is not None:
                if not present.any():
                    return
                if present.all():
                    present = None
            cols.append(FlagColumn.of(key, vals, n, present))

        gp = ff[:, 2] != 0
        if gp.any():
            col("gm", GM, gp)
            col("gm_err", GM_err, gp)
        tp = ff[:, 3] != 0
        if tp.any():
            if self.log10_tau:
                col("scat_time", 10 ** p[:, 3] * P / df * 1e6, tp)
                col("log10_scat_time", p[:, 3] + np.log10(P / df), tp)
                col("log10_scat_time_err", e[:, 3], tp)
            else:
                col("scat_time", p[:, 3] * P / df * 1e6, tp)
                col("scat_time_err", e[:, 3] * P / df * 1e6, tp)
            col("scat_ref_freq", nuo[:, 2] * df, tp)
            col("scat_ind", p[:, 4], tp)
        col("scat_ind_err", e[:, 4], ff[:, 4] != 0)
        const = FlagColumn
        cols += [const("be", "const", data.backend), const("fe", "const", data.frontend),
                 const("f", "const", data.frontend + "_" + data.backend),
                 const("nbin", "const", data.nbin), const("nch", "const", nchan)]
        col("nchx", job.nchx[ok])
        col("bw", fmax - fmin)
        cols.append(const("chbw", "const", abs(data.bw) / nchan))
        col("subint", ok)
        col("tobs", _take(job.tobs, ok))
        col("fratio", fmax / fmin)
        cols.append(const("tmplt", "const", self.modelfile))
        col("snr", res["snr"])
        col("phi_DM_cov", cov[:, 0, 1],
            ~np.isnan(job.nu_refs_a[ok, 0]) & (ff[:, 0] != 0) & (ff[:, 1] != 0))
        col("gof", res["red_chi2"])
        if print_phase:
            col("phs", phi)
            col("phs_err", phi_err)
        if print_flux:
            col("flux", flux[2])
            col("flux_err", flux[3])
            col("flux_ref_freq", flux[4])
        if print_parangle:
            col("par_angle", np.asarray(data.parallactic_angles)[ok])
        dp = ff[:, 1] != 0
        block = TOABlock(datafile, data.telescope, data.telescope_code, nuo[:, 0], mjd, TOA_err,
                         dm=DM if dp.any() else None, dme=DM_err if dp.any() else None,
                         dm_present=None if dp.all() else dp, cols=cols)
        block.add_flags(list(addtnl_toa_flags.items()))
        return DataBunch(a0=a0, n=n, phi=phi, phi_err=phi_err, DM=DM, DM_err=DM_err, GM=GM,
                         GM_err=GM_err, tau=p[:, 3], tau_err=e[:, 3], alpha=p[:, 4],
                         alpha_err=e[:, 4], nfev=nfev, status=status, scales=sc, scale_errs=sce,
                         chsnrs=chs, snr=res["snr"], red_chi2=res["red_chi2"], covs=covs,
                         nu_out=nuo, nu_fit=res["nu_fit"], mjd=mjd, TOA_err=TOA_err, flux=flux,
                         block=block)

    def _finish(self, job, shards, fit_duration, quiet):
        """The per-archive lists of pptoas.py:662-720 (and the DeltaDM mean,
        :664-681) from the shards' columns, concatenated in unit order; the
        shards' TOABlocks join TOA_list."""
        data, datafile = job.data, job.name
        nsub, nchan = data.nsub, data.nchan
        ok = job.ok_isubs
        nok = len(ok)
        if len(shards) == 1:
            def cat(k):
                return shards[0][k]
        else:
            # the per-channel columns (most of the bytes) joined on host
            # threads: a fresh [nsub, nchan] array's first-touch page faults
            # and copies are most of _finish's time
            big = _par_concat({k: [sh[k] for sh in shards]
                               for k in ("scales", "scale_errs", "chsnrs")})

            def cat(k):
                return big[k] if k in big else np.concatenate([sh[k] for sh in shards])
        dense = nok == nsub  # ok_isubs is then every subint, in order

        def spread(v, tail=(), dtype=np.float64):
            if dense:
                return np.ascontiguousarray(v, dtype=dtype)
            out = np.zeros((nsub,) + tail, dtype=dtype)
            out[ok] = v
            return out

        phis, phi_errs = spread(cat("phi")), spread(cat("phi_err"))
        DMs, DM_errs = spread(cat("DM")), spread(cat("DM_err"))
        GMs, GM_errs = spread(cat("GM")), spread(cat("GM_err"))
        taus, tau_errs = spread(cat("tau")), spread(cat("tau_err"))
        alphas, alpha_errs = spread(cat("alpha")), spread(cat("alpha_err"))
        nfevals, rcs = spread(cat("nfev"), dtype="int"), spread(cat("status"), dtype="int")
        scales = spread(cat("scales"), (nchan,))
        scale_errs = spread(cat("scale_errs"), (nchan,))
        chsnrs = spread(cat("chsnrs"), (nchan,))
        snrs, red_chi2s = spread(cat("snr")), spread(cat("red_chi2"))
        covs = spread(cat("covs"), (self.nfit, self.nfit))
        if shards[0].flux is not None:
            fl = [np.concatenate([sh.flux[i] for sh in shards]) for i in range(5)]
            pfl, pfle = spread(fl[0], (nchan,)), spread(fl[1], (nchan,))
            fluxes, flux_errs, flux_freqs = spread(fl[2]), spread(fl[3]), spread(fl[4])
        else:
            pfl, pfle = np.zeros((nsub, nchan)), np.zeros((nsub, nchan))
            fluxes, flux_errs, flux_freqs = np.zeros(nsub), np.zeros(nsub), np.zeros(nsub)
        mjd = [shards[0].mjd[i] if len(shards) == 1 else
               np.concatenate([sh.mjd[i] for sh in shards]) for i in range(3)]
        if dense:
            TOAs = MJDArray(*mjd)
        else:
            parts = []
            for i, dt in enumerate((np.int64, np.int64, np.float64)):
                a = np.zeros(nsub, dtype=dt)
                a[ok] = mjd[i]
                parts.append(a)
            valid = np.zeros(nsub, dtype=bool)
            valid[ok] = True
            TOAs = MJDArray(*parts, valid=valid)
        if dense:
            TOA_errs = cat("TOA_err").astype(object)
            job.nu_fits_a[:] = cat("nu_fit")
        else:
            TOA_errs = np.zeros(nsub, dtype="object")
            TOA_errs[ok] = cat("TOA_err")
            job.nu_fits_a[ok] = cat("nu_fit")  # (computed by whichever rank read the subint)
        # the reference's list(np.zeros([nsub, 3])) with ok rows filled
        # (pptoas.py:283-284, 406, 527-530) as one [nsub, 3] array: indexed
        # by subint it gives the same rows
        nu_fits = job.nu_fits_a
        nu_refs = np.zeros((nsub, 3))
        nu_refs[ok] = cat("nu_out")
        for sh in shards:
            self.TOA_list.add_block(sh.block)
        # DeltaDM weighted mean per archive (pptoas.py:664-681)
        DeltaDMs = DMs - job.DM0
        dd, de = (DeltaDMs, DM_errs) if dense else (DeltaDMs[ok], DM_errs[ok])
        w = de ** -2 if np.all(de) else np.ones(nok)
        mean, wsum = np.average(dd, weights=w, returned=True)
        var = wsum ** -1
        if nok > 1:
            var *= np.sum(((dd - mean) ** 2) * w) / (len(dd) - 1)
        for attr, val in [("order", datafile), ("obs", job.obs),
                          ("doppler_fs", data.doppler_factors), ("nu0s", data.nu0),
                          ("nu_fits", nu_fits), ("nu_refs", nu_refs), ("ok_isubs", ok),
                          ("epochs", data.epochs), ("MJDs", job.MJDs), ("Ps", data.Ps),
                          ("phis", phis), ("phi_errs", phi_errs), ("TOAs", TOAs),
                          ("TOA_errs", TOA_errs), ("DM0s", job.DM0), ("DMs", DMs),
                          ("DM_errs", DM_errs), ("DeltaDM_means", mean),
                          ("DeltaDM_errs", var ** 0.5), ("GMs", GMs), ("GM_errs", GM_errs),
                          ("taus", taus), ("tau_errs", tau_errs), ("alphas", alphas),
                          ("alpha_errs", alpha_errs), ("scales", scales),
                          ("scale_errs", scale_errs), ("snrs", snrs),
                          ("channel_snrs", chsnrs), ("profile_fluxes", pfl),
                          ("profile_flux_errs", pfle), ("fluxes", fluxes),
                          ("flux_errs", flux_errs), ("flux_freqs", flux_freqs),
                          ("covariances", covs), ("red_chi2s", red_chi2s),
                          ("nfevals", nfevals), ("rcs", rcs),
                          ("fit_durations", fit_duration)]:
            getattr(self, attr).append(val)
        if not quiet:
            print("--------------------------")
            print(datafile)
            print("~%.4f sec/TOA" % (fit_duration / nok))
            print("Med. TOA error is %.3f us" % (np.median(phi_errs[ok]) *
                                                 data.Ps.mean() * 1e6))


class _Job(DataBunch):
    """One archive's get_TOAs set-up (GetTOAs._prepare)."""

    def row(self, key, s):
        """Per-subint [nsub, nchan] input key ("freqs", "weights", "mask")
        for subints s: one shared [nchan] row when every subint's is the
        same.  The shared row is the first ok subint's: `uniform` compares
        the ok subints' rows only, and a zapped subint 0 is not one of them."""
        a = self.mask if key == "mask" else self.data[key]
        if self.uniform[key]:
            return a[int(self.ok_isubs[0])]
        return _take(a, s)


def _take(a, s):
    """a[s]: a view when s is an ascending run of consecutive indices."""
    s = np.asarray(s)
    if len(s) and s[-1] - s[0] + 1 == len(s) and (len(s) < 3 or s[1] == s[0] + 1):
        return a[int(s[0]):int(s[-1]) + 1]
    return a[s]


_RESULT_KEYS = ["params", "param_errs", "nu_out", "cov", "scales", "scale_errs",
                "channel_snrs", "chi2", "red_chi2", "snr", "nfev", "status"]


def _arch_index(rel, t):
    import torch
    return torch.as_tensor(rel, device=t.device, dtype=torch.long)
