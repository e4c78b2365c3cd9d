"""ppspline drop-in: B-spline portrait models from a PCA of an averaged portrait.

For an nchan x nbin portrait of aligned profiles (ppalign's output) the model
is a B-spline representation of the curve the nchan profiles trace in the
space of a few eigenprofiles (ppspline.py:1-20).  The PCA runs on the device
(ppf_pca_portraits, batched over portraits; ppf_pca_gram_portraits above
2,048 unzapped channels), as do the projections
(ppf_pca_project) and the model portraits (ppf_spline_portraits); the curve
fit is one scipy.interpolate.splprep call per model on nchan x <= 10 numbers
(FITPACK, third-party to the reference too).

Wavelet smoothing of the eigenvectors and the mean profile, the reference's
default, is opt-in as smooth="swt": the undecimated db8 transform built from
its definition on the device (pplib.smart_smooth, ppf_smart_smooth_rows;
DESIGN.md section 9), every vector and mean profile of a make_spline_models
call in one device call.  smooth=True stays refused: it would promise
PyWavelets' output, which is not available to pin against.  Without smoothing
(the default here) the reference's S/N test lets noise eigenvectors through at
large nbin, so callers should pass smooth="swt" or set max_ncomp
(INTEGRATION.md).

A metafile (an ASCII list of archives, one per receiver) gives the
reference's concatenated portrait (pplib.py:163-299) with its join attributes,
which ppgauss fits; make_spline_model takes it as it is.

Not here: plotting and the command line.
"""
import pickle

import numpy as np

from . import archive as _arch
from . import pplib
from .pplib import (get_noise, gen_spline_portrait, find_significant_eigvec, smart_smooth,
                    wavelet_smooth)

_NO_SMOOTH = ("smooth=True: " + pplib._NO_SMOOTH)


def spline_smoothing(nprof, SNRs, noise_stds, sfac=1.0):
    """The smoothing condition s handed to splprep (ppspline.py:136-138)."""
    SNRs = np.asarray(SNRs, dtype=np.float64)
    return sfac * nprof * np.sum((SNRs * np.asarray(noise_stds)) ** 2) / sum(SNRs) ** 2


def fit_spline_curve(proj_port, weights, freqs, s, bw=1.0, k=3, max_nbreak=None, quiet=True,
                     splprep=None):
    """The B-spline curve traced by the projected profiles, parameterized by
    frequency (ppspline.py:139-155): splprep over the rows in increasing
    frequency (reversed when bw < 0), refitted with at most max_nbreak
    breakpoints (nest = max_nbreak + 2 k; s = inf at two) if the first fit
    has more.  Returns (tck, u), fp, ier, msg.  splprep: the fitting
    function (default scipy.interpolate.splprep)."""
    if splprep is None:
        from scipy.interpolate import splprep
    flip = -1 if bw < 0 else 1  # u in splprep has to be increasing
    x = list(np.asarray(proj_port)[::flip].T)
    w, u = np.asarray(weights)[::flip], np.asarray(freqs)[::flip]
    nu_lo, nu_hi = np.min(freqs), np.max(freqs)
    (tck, u_out), fp, ier, msg = splprep(x, w=w, u=u, ub=nu_lo, ue=nu_hi, k=k, task=0, s=s,
                                         t=None, full_output=1, nest=None, per=0,
                                         quiet=int(quiet))
    if max_nbreak is not None and len(np.unique(tck[0])) > max_nbreak:
        if max_nbreak < 2:
            print("max_nbreak not >= 2; setting max_nbreak = 2...")
            max_nbreak = 2
        if max_nbreak == 2:
            s = np.inf
        (tck, u_out), fp, ier, msg = splprep(x, w=w, u=u, ub=nu_lo, ue=nu_hi, k=k, task=0, s=s,
                                             t=None, full_output=1, nest=max_nbreak + (k * 2),
                                             per=0, quiet=int(quiet))
    return (tck, u_out), fp, ier, msg


JOIN_HEADER = ("# archive name" + " " * 32 + "-phase offset & err [rot]" + " " * 2 +
               "-delta-DM & err [cm**-3 pc]\n")


def join_parameter_line(datafile, phase, phase_err, dm, dm_err):
    """One line of a .join file (pplib.py:516-519)."""
    return (datafile + " " * abs(45 - len(datafile)) + "% .10f" % phase + " " * 1 +
            "%.10f" % phase_err + " " * 2 + "% .6f" % dm + " " * 1 + "%.6f" % dm_err + "\n")


def read_joinfile(joinfile, datafiles, join_params):
    """join_params with the phases and DMs of a .join file's last
    len(datafiles) lines, matched by archive name (pplib.py:282-297): the
    columns are name, phase, phase error, DM, DM error, or (old files) name,
    phase, DM."""
    join_params = np.array(join_params, dtype=np.float64)
    with open(joinfile, "r") as jf:
        lines = [line.split() for line in jf.readlines()[-len(datafiles):]]
    try:
        for line in lines:
            ijoin = datafiles.index(line[0])
            join_params[ijoin * 2] = np.double(line[1])
            join_params[ijoin * 2 + 1] = np.double(line[3] if len(line) > 3 else line[2])
    except (ValueError, IndexError):
        print("Bad join file.")
    return join_params


class DataPortrait(object):
    """The data to which a model is fitted (pplib.py:139-327): a PSRFITS
    file, an .npz, or a registered / dict archive, loaded dedispersed,
    tscrunched and pscrunched -- or a metafile, an ASCII list of such
    archives (one per receiver), whose rows are concatenated and sorted by
    frequency.  port is the masked portrait, portx its unzapped channels;
    likewise freqs / freqsxs, noise_stds / noise_stdsxs and SNRs / SNRsxs.

    For a metafile join_ichans / join_ichanxs hold each archive's rows of
    port / portx, join_params its phase [rot] and DM offsets (the first
    archive's phase 0 and fixed, the others' from fit_phase_shift against the
    first's profile; every DM 0 and free) or those of joinfile, and
    all_join_params = [join_ichanxs, join_params, join_fit_flags] is what
    pplib.fit_gaussian_portrait takes."""

    def __init__(self, datafile, quiet=False, joinfile=None):
        self.joinfile = joinfile
        if _arch.file_is_type(datafile, "ASCII"):
            self._load_metafile(datafile, quiet)
            return
        if joinfile is not None:
            raise NotImplementedError("joinfile: only with a metafile (one archive has nothing "
                                      "to join)")
        self.njoin = 0
        self.join_params, self.join_ichans, self.all_join_params = [], [], []
        self.data = _arch.load_data(datafile, dedisperse=True, dededisperse=False, tscrunch=True,
                                    pscrunch=True, fscrunch=False, flux_prof=True,
                                    refresh_arch=True, return_arch=True, quiet=quiet)
        self.datafile = datafile if isinstance(datafile, str) else self.data.filename
        self.datafiles = [self.datafile]
        for key in self.data.keys():
            setattr(self, key, self.data[key])
        if self.source is None:
            self.source = "noname"
        self.subints = _arch.host_array(self.subints)
        self.weights = np.asarray(self.weights, dtype=np.float64)
        self.masks = np.asarray(self.masks)
        self.port = (self.masks * self.subints)[0, 0]
        if self.noise_stds is None:
            self.noise_stds = get_noise(self.subints[0, 0], chans=True)[None, None]
        self.noise_stds = np.array(self.noise_stds, dtype=np.float64)
        self.SNRs = np.array(self.SNRs, dtype=np.float64)
        ok = self.ok_ichans[0]
        self.portx = self.port[ok]
        self.flux_prof = self.port.mean(axis=1)
        self.flux_profx = self.flux_prof[ok]
        self.freqsxs = [self.freqs[0, ok]]
        self.noise_stdsxs = self.noise_stds[0, 0, ok]
        self.SNRsxs = self.SNRs[0, 0, ok]
        self.norm_values = np.ones(len(self.port))

    def _load_metafile(self, metafile, quiet):
        """The concatenated portrait of a metafile's archives (pplib.py:163-299)."""
        with open(metafile, "r") as mf:
            self.datafiles = [line.strip() for line in mf.readlines() if line.strip()]
        self.metafile = self.datafile = metafile
        self.njoin = len(self.datafiles)
        for datafile in self.datafiles:
            if not _arch.file_is_type(datafile, "FITS"):
                raise NotImplementedError(
                    "metafile %s lists %s, which is not a registered, .npz or PSRFITS archive: "
                    "archives in other PSRCHIVE formats are not supported" % (metafile, datafile))
        join_params, join_fit_flags = [], []
        join_nchans, join_nchanxs = [0], [0]
        cols = {key: [] for key in ("freqs", "freqsxs", "masks", "port", "portx", "noise_stds",
                                    "noise_stdsxs", "SNRs", "SNRsxs", "weights", "weightsxs")}
        Ps, lofreq, hifreq = 0.0, np.inf, 0.0
        for ifile, datafile in enumerate(self.datafiles):
            data = _arch.load_data(datafile, dedisperse=True, tscrunch=True, pscrunch=True,
                                   fscrunch=False, flux_prof=True, return_arch=True, quiet=quiet)
            sub = _arch.host_array(data.subints)[0, 0]
            ok = np.asarray(data.ok_ichans[0])
            weights = np.asarray(data.weights, dtype=np.float64)[0]
            masks = np.asarray(data.masks)[0, 0]
            noise = get_noise(sub, chans=True) if data.noise_stds is None else \
                np.asarray(data.noise_stds, dtype=np.float64)[0, 0]
            SNRs = np.asarray(data.SNRs, dtype=np.float64)[0, 0]
            # the archive's fscrunched profile (weighted, as PSRCHIVE scrunches)
            prof = np.average(sub[ok], axis=0, weights=weights[ok])
            if ifile == 0:
                self.nbin, self.phases, self.source = data.nbin, data.phases, data.source
                refprof = prof
                join_params += [0.0, 0.0]
                join_fit_flags += [0, 1]
            else:
                if data.nbin != self.nbin:
                    raise ValueError("%s: %s has %d phase bins and %s has %d; a joint portrait "
                                     "needs one nbin" % (metafile, datafile, data.nbin,
                                                         self.datafiles[0], self.nbin))
                phi = -pplib.fit_phase_shift(prof, refprof, Ns=self.nbin).phase
                join_params += [phi, 0.0]
                join_fit_flags += [1, 1]
            join_nchans.append(join_nchans[-1] + data.nchan)
            join_nchanxs.append(join_nchanxs[-1] + len(ok))
            Ps += np.mean(data.Ps)
            half = abs(data.bw) / (2 * data.nchan)
            lofreq = min(lofreq, data.freqs.min() - half)
            hifreq = max(hifreq, data.freqs.max() + half)
            cols["freqs"].extend(data.freqs[0])
            cols["freqsxs"].extend(data.freqs[0, ok])
            cols["masks"].extend(masks)
            cols["port"].extend(sub * masks)
            cols["portx"].extend(sub[ok])
            cols["noise_stds"].extend(noise)
            cols["noise_stdsxs"].extend(noise[ok])
            cols["SNRs"].extend(SNRs)
            cols["SNRsxs"].extend(SNRs[ok])
            cols["weights"].extend(weights)
            cols["weightsxs"].extend(weights[ok])
        if self.source is None:
            self.source = "noname"
        self.Ps = [Ps / self.njoin]
        self.lofreq, self.hifreq = lofreq, hifreq
        self.bw = hifreq - lofreq
        freqs, freqsxs = np.array(cols["freqs"]), np.array(cols["freqsxs"])
        self.nu0 = freqs.mean()
        self.isort, self.isortx = np.argsort(freqs), np.argsort(freqsxs)
        self.join_nchans, self.join_nchanxs = join_nchans, join_nchanxs
        self.join_ichans = [np.flatnonzero((self.isort >= join_nchans[i]) *
                                           (self.isort < join_nchans[i + 1]))
                            for i in range(self.njoin)]
        self.join_ichanxs = [np.flatnonzero((self.isortx >= join_nchanxs[i]) *
                                            (self.isortx < join_nchanxs[i + 1]))
                             for i in range(self.njoin)]
        self.masks = np.array(cols["masks"])[self.isort][None, None]
        self.port = np.array(cols["port"])[self.isort]
        self.portx = np.array(cols["portx"])[self.isortx]
        self.flux_prof = self.port.mean(axis=1)
        self.flux_profx = self.portx.mean(axis=1)
        self.noise_stds = np.array(cols["noise_stds"])[self.isort][None, None]
        self.noise_stdsxs = np.array(cols["noise_stdsxs"])[self.isortx]
        self.SNRs = np.array(cols["SNRs"])[self.isort][None, None]
        self.SNRsxs = np.array(cols["SNRsxs"])[self.isortx]
        self.weights = np.array(cols["weights"])[self.isort][None]
        self.weightsxs = np.array(cols["weightsxs"])[self.isortx][None]
        self.freqs = freqs[self.isort][None]
        self.freqsxs = [freqsxs[self.isortx]]
        self.nchan = len(self.port)
        self.nchanx = len(self.portx)
        self.ok_ichans = [np.flatnonzero(self.weights[0] > 0.0)]
        self.norm_values = np.ones(self.nchan)
        self.join_params = np.array(join_params)
        self.join_param_errs = np.zeros(len(join_params))
        self.join_fit_flags = np.array(join_fit_flags)
        if self.joinfile:
            self.join_params = read_joinfile(self.joinfile, self.datafiles, self.join_params)
        self.all_join_params = [self.join_ichanxs, self.join_params, self.join_fit_flags]

    def apply_joinfile(self, nu_ref, undo=False):
        """Rotate port and portx by minus the join parameters about nu_ref
        [MHz], the fitted model's reference frequency (pplib.py:329-355);
        undo=True rotates the other way.

        A rotation drops the imaginary part it gives the Nyquist harmonic, so
        rotating back does not return the rows it started from (noise has
        power there).  undo=True therefore puts back the arrays the last
        apply_joinfile(nu_ref) rotated, when port and portx are still the
        arrays it left and the join parameters are the same; otherwise it
        rotates, as the reference does."""
        sign = 1.0 if undo else -1.0
        key = (float(nu_ref), tuple(float(v) for v in self.join_params))
        last = getattr(self, "_joinfile_applied", None)
        self._joinfile_applied = None
        if undo and last is not None and last[0] == key and self.port is last[3] \
                and self.portx is last[4]:
            self.port, self.portx = last[1], last[2]
            return
        before = (self.port, self.portx)
        self.port = pplib.rotate_join_rows(self.port, self.join_ichans, self.join_params,
                                           self.Ps[0], self.freqs[0], nu_ref, sign)
        self.portx = pplib.rotate_join_rows(self.portx, self.join_ichanxs, self.join_params,
                                            self.Ps[0], self.freqsxs[0], nu_ref, sign)
        if not undo:
            self._joinfile_applied = (key,) + before + (self.port, self.portx)

    def write_join_parameters(self):
        """Append the join parameters to joinfile, or to <model_name>.join
        (pplib.py:486-521).  As there, the parameters are the opposite of the
        rotation that aligns the data: use a negative with rotate_data; the
        DMs are offsets, not Doppler corrected."""
        joinfile = self.joinfile if self.joinfile is not None else self.model_name + ".join"
        with open(joinfile, "a") as jf:
            jf.write(JOIN_HEADER)
            for ifile, datafile in enumerate(self.datafiles):
                jf.write(join_parameter_line(datafile, self.join_params[ifile * 2],
                                             self.join_param_errs[::2][ifile],
                                             self.join_params[ifile * 2 + 1],
                                             self.join_param_errs[1::2][ifile]))

    def normalize_portrait(self, method="rms"):
        """Normalize each channel's profile (pplib.py:357-382)."""
        if method not in ("mean", "max", "prof", "rms", "abs"):
            print("Unknown method for normalize_portrait(...), '%s'." % method)
            return
        if method == "prof":
            weights = self.weights[0]
            weightsx = self.weights[self.weights > 0]
        else:
            weights = weightsx = None
        self.unnorm_noise_stds = np.copy(self.noise_stds)
        self.port, self.norm_values = pplib.normalize_portrait(self.port, method, weights=weights,
                                                               return_norms=True)
        self.noise_stds[0, 0] = get_noise(self.port, chans=True)
        self.flux_prof = self.port.mean(axis=1)
        self.unnorm_noise_stdsxs = np.copy(self.noise_stdsxs)
        self.portx = pplib.normalize_portrait(self.portx, method, weights=weightsx,
                                              return_norms=False)
        self.noise_stdsxs = get_noise(self.portx, chans=True)
        self.flux_profx = self.portx.mean(axis=1)

    def unnormalize_portrait(self):
        """Undo normalize_portrait (pplib.py:384-398)."""
        if hasattr(self, "unnorm_noise_stds"):
            self.port = (self.norm_values * self.port.transpose()).transpose()
            self.noise_stds = np.copy(self.unnorm_noise_stds)
            del self.unnorm_noise_stds
            self.flux_prof = self.port.mean(axis=1)
            self.portx = (self.norm_values[self.ok_ichans[0]] * self.portx.transpose()).transpose()
            self.noise_stdsxs = np.copy(self.unnorm_noise_stdsxs)
            del self.unnorm_noise_stdsxs
            self.flux_profx = self.portx.mean(axis=1)
            self.norm_values = np.ones(len(self.port))

    def smooth_portrait(self, smart=False, **kwargs):
        """Wavelet-smooth the portrait and its unzapped channels
        (pplib.py:400-424): wavelet_smooth(**kwargs), or with smart
        smart_smooth over min(8, log2 nbin) levels; the noise levels and flux
        profiles are refreshed."""
        if smart:
            def smooth(port):
                return smart_smooth(port, try_nlevels=min(8, int(np.log2(self.nbin))), **kwargs)
        else:
            def smooth(port):
                return wavelet_smooth(port, **kwargs)
        self.port = smooth(self.port)
        self.noise_stds[0, 0] = get_noise(self.port, chans=True)
        self.flux_prof = self.port.mean(axis=1)
        self.portx = smooth(self.portx)
        self.noise_stdsxs = get_noise(self.portx, chans=True)
        self.flux_profx = self.portx.mean(axis=1)

    def fit_flux_profile(self, channel_errs=None, nu_ref=None, guessA=1.0, guessalpha=0.0,
                         plot=False, savefig=False, quiet=False):
        """Fit a power law to the phase-averaged flux spectrum of the unzapped
        channels, flux_profx over freqsxs[0] (pplib.py:426-484), on the
        device (pplib.fit_powlaw).  channel_errs defaults to ones, nu_ref to
        nu0.  Sets flux_fit (fit_powlaw's DataBunch), spect_A, spect_A_err,
        spect_A_ref, spect_index and spect_index_err.  plot defaults to False,
        unlike the reference: plotting is not part of this build."""
        if nu_ref is None:
            nu_ref = self.nu0
        freqs = np.asarray(self.freqsxs[0], dtype=np.float64)
        if channel_errs is None:
            channel_errs = np.ones(len(freqs))
        fp = pplib.fit_powlaw(self.flux_profx, np.array([guessA, guessalpha]), channel_errs,
                              freqs, nu_ref)
        if not quiet:
            print("")
            print("Flux-density power-law fit")
            print("----------------------------------")
            print("residual mean = %.2f" % fp.residuals.mean())
            print("residual std. = %.2f" % fp.residuals.std())
            print("reduced chi-squared = %.2f" % (fp.chi2 / fp.dof))
            print("A = %.3f +/- %.3f (flux at %.2f MHz)" % (fp.amp, fp.amp_err, fp.nu_ref))
            print("alpha = %.3f +/- %.3f" % (fp.alpha, fp.alpha_err))
        if plot or savefig:
            print("fit_flux_profile: plotting is not part of this build; the fit is in flux_fit")
        self.flux_fit = fp
        self.spect_A = fp.amp
        self.spect_A_err = fp.amp_err
        self.spect_A_ref = fp.nu_ref
        self.spect_index = fp.alpha
        self.spect_index_err = fp.alpha_err

    def pca_weights(self):
        """The PCA (and spline) weights of the unzapped channels (ppspline.py:69)."""
        return self.SNRsxs / np.sum(self.SNRsxs)

    def make_spline_model(self, max_ncomp=10, smooth=False, snr_cutoff=150.0, rchi2_tol=0.1, k=3,
                          sfac=1.0, max_nbreak=None, model_name=None, quiet=False, **kwargs):
        """Make a model based on PCA and B-spline interpolation
        (ppspline.py:34-204; the arguments are the reference's).

        smooth defaults to False, unlike the reference.  smooth="swt" smooths
        the eigenvectors and the mean profile with pplib.smart_smooth (the
        project's from-definition db8 transform) as the reference's
        smooth=True does with PyWavelets: the significance test, the
        projections, the model and write_model use the smoothed arrays, kept
        as self.smooth_eigvec and self.smooth_mean_prof.  smooth=True raises
        NotImplementedError.  **kwargs go to find_significant_eigvec (and,
        under smooth="swt", on to smart_smooth for the eigenvectors)."""
        make_spline_models([self], max_ncomp=max_ncomp, smooth=smooth, snr_cutoff=snr_cutoff,
                           rchi2_tol=rchi2_tol, k=k, sfac=sfac, max_nbreak=max_nbreak,
                           model_names=[model_name], quiet=quiet, **kwargs)

    def _finish_model(self, mean_prof, eigval, eigvec, max_ncomp, snr_cutoff, rchi2_tol, k, sfac,
                      max_nbreak, model_name, quiet, kwargs, smoothed=None):
        """make_spline_model after the PCA (ppspline.py:83-204); eigvec
        [nbin, r] column vectors.  smoothed (smooth="swt"): the smart_smooth
        of the leading eigenvectors, as rows, and of the mean profile."""
        port = self.portx
        pca_weights = self.pca_weights()
        freqs = self.freqsxs[0]
        return_max = 10 if max_ncomp is None else min(max_ncomp, 10)
        for attr in ("smooth_eigvec", "smooth_mean_prof"):  # of an earlier model
            if hasattr(self, attr):
                delattr(self, attr)
        if smoothed is None:
            ieig = find_significant_eigvec(eigvec, check_max=10, return_max=return_max,
                                           snr_cutoff=snr_cutoff, return_smooth=False,
                                           rchi2_tol=rchi2_tol, **kwargs)
            model_vec, model_mean = eigvec, mean_prof
        else:
            smooth_cols = np.zeros(eigvec.shape)
            smooth_cols[:, :len(smoothed[0])] = smoothed[0].T
            ieig, model_vec = find_significant_eigvec(
                eigvec, check_max=10, return_max=return_max, snr_cutoff=snr_cutoff,
                return_smooth=True, rchi2_tol=rchi2_tol, smooth="swt", smooth_eigvec=smooth_cols,
                **kwargs)
            model_mean = smoothed[1]
        ncomp = len(ieig)
        nfull = len(self.freqs[0])
        if ncomp == 0:  # a model with the constant average portrait
            proj_port = port[:, :0]
            modelx = reconst_port = np.tile(model_mean, (len(freqs), 1))
            model = np.tile(model_mean, (nfull, 1))
            (tck, u) = [np.array([]), np.array([]), 0], np.array([])
            fp, ier, msg = None, None, None
        else:
            # (the projections are about the unsmoothed mean profile, as in
            # the reference)
            basis = np.ascontiguousarray(model_vec[:, ieig])
            proj, rec = pplib._engine().pca_project(port, mean_prof,
                                                    np.ascontiguousarray(basis.T),
                                                    reconstruct=True)
            proj_port, reconst_port = proj.cpu().numpy(), rec.cpu().numpy()
            s = spline_smoothing(len(proj_port), self.SNRsxs, self.noise_stdsxs, sfac)
            (tck, u), fp, ier, msg = fit_spline_curve(proj_port, pca_weights, freqs, s, self.bw,
                                                      k, max_nbreak, quiet)
            if ier > 1:
                print("Something went wrong in si.splprep for %s:\n%s" % (self.source, msg))
            # both portraits in one device call
            both = gen_spline_portrait(model_mean, np.concatenate([freqs, self.freqs[0]]), basis,
                                       tck)
            modelx, model = both[:len(freqs)], both[len(freqs):]
        self.ieig, self.ncomp = ieig, ncomp
        self.eigvec, self.eigval, self.mean_prof = eigvec, eigval, mean_prof
        if smoothed is not None:
            self.smooth_mean_prof, self.smooth_eigvec = model_mean, model_vec
        self.proj_port, self.reconst_port = proj_port, reconst_port
        self.tck, self.u, self.fp, self.ier, self.msg = tck, u, fp, ier, msg
        self.model_name = self.datafile + ".spl" if model_name is None else model_name
        self.model, self.modelx = model, modelx
        self.model_masked = self.model * self.masks[0, 0]
        if not quiet:
            if proj_port.sum():
                print("B-spline interpolation model %s uses %d basis profile components and %d "
                      "breakpoints (%d B-splines with k=%d)." % (
                          self.model_name, ncomp, len(np.unique(self.tck[0])),
                          len(self.tck[0]) - self.tck[2] - 1, self.tck[2]))
            else:
                print("B-spline interpolation model %s uses 0 basis profile components; it "
                      "returns the average profile." % self.model_name)

    def write_model(self, outfile, quiet=False):
        """Write the model as the reference's pickle (ppspline.py:206-230):
        [model_name, source, datafile, mean_prof, eigvec[:, ieig], tck] -- the
        smoothed mean profile and eigenvectors when the model was made with
        smooth="swt" -- in protocol 2 so that the Python-2 reference reads it
        too."""
        if hasattr(self, "smooth_eigvec"):
            eigvec, mean_prof = self.smooth_eigvec, self.smooth_mean_prof
        else:
            eigvec, mean_prof = self.eigvec, self.mean_prof
        basis = eigvec[:, self.ieig] if len(self.ieig) else eigvec[:, []]
        blob = pickle.dumps([self.model_name, self.source, self.datafile, mean_prof,
                             np.ascontiguousarray(basis), self.tck], protocol=2)
        # numpy 2 names its array constructor numpy._core.multiarray, which a
        # Python-2 numpy does not have; numpy.core.multiarray resolves in
        # both.  (Protocol 2 writes a global as the text "c<module>\n<name>\n",
        # so the substitution cannot touch a length field.)
        blob = blob.replace(b"cnumpy._core.multiarray\n", b"cnumpy.core.multiarray\n")
        with open(outfile, "wb") as of:
            of.write(blob)
        if not quiet:
            print("Wrote modelfile %s." % outfile)


def make_spline_models(portraits, max_ncomp=10, smooth=False, snr_cutoff=150.0, rchi2_tol=0.1,
                       k=3, sfac=1.0, max_nbreak=None, model_names=None, quiet=False, **kwargs):
    """make_spline_model for a list of DataPortraits whose condensed
    portraits share one shape (pulsars x receivers): one batched PCA call,
    then (smooth="swt") one smart_smooth call for every portrait's leading
    eigenvectors and mean profile, then the host steps per portrait.  The
    results are those of the one-by-one calls, exactly."""
    if smooth and smooth != "swt":
        raise NotImplementedError(_NO_SMOOTH)
    portraits = list(portraits)
    if not portraits:
        return portraits
    shape = portraits[0].portx.shape
    for dp in portraits:
        if dp.portx.shape != shape:
            raise ValueError("make_spline_models: portraits of %s and %s unzapped channels x bins; "
                             "one shape per call" % (shape, dp.portx.shape))
    if model_names is None:
        model_names = [None] * len(portraits)
    if not quiet:
        print("Performing principal component analysis on data with %d dimensions and %d "
              "measurements..." % (shape[1], shape[0]))
    mean, eigval, eigvec, info = pplib._engine().pca_portraits(
        np.stack([dp.portx for dp in portraits]),
        np.stack([dp.pca_weights() for dp in portraits]))
    mean, eigval, info = mean.cpu().numpy(), eigval.cpu().numpy(), info.cpu().numpy()
    eigvec = eigvec.cpu().numpy()
    nbin = shape[1]
    if smooth and nbin % 2 != 0:
        print("nbin = %d is odd; cannot wavelet_smooth.\n" % nbin)
        smooth = False
    elif smooth and nbin & (nbin - 1):
        print("nbin = %d is not a power of two; can only try wavelet_smooth to one level; "
              "recommend resampling to a power-of-two number of phase bins.\n" % nbin)
    smoothed = [None] * len(portraits)
    if smooth:
        # the keywords find_significant_eigvec hands on to smart_smooth; the
        # mean profiles get rchi2_tol alone (ppspline.py:101-102)
        sm_kw = {key: val for key, val in kwargs.items()
                 if key not in ("check_crossings", "check_acorr", "noise", "smooth_eigvec")}
        ncheck = min(10, eigvec.shape[1])
        vecs = eigvec[:, :ncheck].reshape(-1, nbin)
        if any(key in sm_kw for key in ("try_nlevels", "threshtype")):
            svecs = smart_smooth(vecs, rchi2_tol=rchi2_tol, **sm_kw)
            smean = smart_smooth(mean, rchi2_tol=rchi2_tol)
        else:  # the same search for both: one device call
            both = smart_smooth(np.concatenate([vecs, mean]), rchi2_tol=rchi2_tol, **sm_kw)
            svecs, smean = both[:len(vecs)], both[len(vecs):]
        svecs = svecs.reshape(len(portraits), ncheck, nbin)
        smoothed = [(svecs[i], smean[i]) for i in range(len(portraits))]
    for i, dp in enumerate(portraits):
        if not info[i, 1]:
            print("PCA of %s did not converge in %d sweeps." % (dp.datafile, info[i, 0]))
        dp.pca_info = info[i]
        dp._finish_model(mean[i], eigval[i], np.ascontiguousarray(eigvec[i].T), max_ncomp,
                         snr_cutoff, rchi2_tol, k, sfac, max_nbreak, model_names[i], quiet, kwargs,
                         smoothed[i])
    return portraits
