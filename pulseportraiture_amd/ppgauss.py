"""ppgauss drop-in: Gaussian-component portrait models fitted on the device.

A model is a sum of Gaussian components whose location, width and amplitude
evolve with frequency (power law or linear), optionally scattered
(ppgauss.py:1-20); it is written as the .gmodel text file pplib.read_model
reads.  The fits -- lmfit's leastsq in the reference, one core and no
Jacobian -- run as one batched Levenberg-Marquardt call with an analytic
Jacobian (ppf_gauss_fit_batch, ppfit_gauss.hip).

The interactive GaussianSelector is replaced by an automatic search
(max_ngauss > 0: pplib.auto_gaussian_profiles, a matched-filter pursuit on
the device); auto_gauss and init_params remain.

A metafile portrait (several receivers' archives; ppspline.DataPortrait) is
fitted jointly: a phase and a DM offset per archive alongside the components
(ppf_gauss_fit_join_batch), written to <model_name>.join after every fit.

Not here: residplot and the command line.
"""
import time

import numpy as np

from . import pplib
from . import ppspline
from .pplib import (default_model, scattering_alpha, gaussian_profile, get_noise,
                    fit_phase_shift, fit_portrait, fit_gaussian_profile, fit_gaussian_portraits,
                    guess_fit_freq, read_model, rotate_data, auto_gaussian_profiles)

_NO_SELECTOR = ("the interactive GaussianSelector is not supported: give max_ngauss (the "
                "automatic component search), auto_gauss (one component, fitted "
                "automatically) or init_params")


class DataPortrait(ppspline.DataPortrait):
    """ppspline's DataPortrait (pplib.py:139-327) with the Gaussian-component
    model builder (ppgauss.py:25-372)."""

    def __init__(self, datafile, quiet=False, joinfile=None):
        super(DataPortrait, self).__init__(datafile, quiet=quiet, joinfile=joinfile)
        self.nchan, self.nbin = self.port.shape
        self.nchanx = len(self.portx)
        self.phases = pplib.get_bin_centers(self.nbin)
        if getattr(self, "nu0", None) is None:
            self.nu0 = float(np.mean(self.freqs[0]))
        self.init_params = []

    # -- the initial profile fit ------------------------------------------
    def fit_profile(self, profile, tau=0.0, fixscat=True, auto_gauss=0.0, profile_fit_flags=None,
                    show=False, init_params=None, max_ngauss=0):
        """Fit Gaussian components to a profile (ppgauss.py:27-53) without
        the GUI: auto_gauss != 0 is the initial width [rot] of one component
        placed by fit_phase_shift (ppgauss.py:419, 442-459); init_params (DC,
        tau [bin], then loc, wid, amp per component) seeds several; with
        neither, max_ngauss > 0 searches for up to that many components
        (pplib.auto_gaussian_profiles)."""
        profile = np.asarray(profile, dtype=np.float64)
        fit_scattering = not fixscat
        if init_params is None and not auto_gauss:
            if not max_ngauss:
                raise NotImplementedError(_NO_SELECTOR)
            self._take_search(auto_gaussian_profiles(
                [profile], None, max_ngauss, self._search_tau(tau, fixscat), fit_scattering)[0])
            return
        if init_params is None:
            if fit_scattering and tau == 0.0:
                tau = 0.1  # (ppgauss.py:415-416)
            errs = get_noise(profile)
            dc = sorted(profile)[len(profile) // 10 + 1]
            amp, wid = profile.max(), auto_gauss
            first = amp * gaussian_profile(len(profile), 0.5, wid)
            loc = 0.5 + fit_phase_shift(profile, first, errs).phase
            init_params = [dc, tau, loc, wid, amp]
        else:
            init_params = list(np.asarray(init_params, dtype=np.float64))
            errs = get_noise(profile)
            if fit_scattering and init_params[1] == 0.0:
                init_params[1] = 0.1
        fgp = fit_gaussian_profile(profile, init_params, np.zeros(len(profile)) + errs,
                                   profile_fit_flags, fit_scattering, quiet=True)
        self.profile_fit = fgp
        self.init_params = fgp.fitted_params
        self.init_param_errs = fgp.fit_errs
        self.ngauss = (len(self.init_params) - 2) // 3

    @staticmethod
    def _search_tau(tau, fixscat):
        return 0.1 if (not fixscat and tau == 0.0) else tau  # (ppgauss.py:415-416)

    def _take_search(self, found):
        """The automatic search's result as the profile fit."""
        if not found.ngauss:
            raise RuntimeError("%s: the automatic component search found no significant "
                               "component in the reference profile" % self.datafile)
        self.profile_fit = found
        self.init_params = found.fitted_params
        self.init_param_errs = found.fit_errs
        self.ngauss = found.ngauss

    def _ref_profile(self, ref_prof):
        """The profile of the channels around nu_ref (ppgauss.py:120-141)."""
        self.nu_ref, self.bw_ref = ref_prof
        if self.nu_ref is None:
            self.nu_ref = self.nu0
        if self.bw_ref is None:
            self.bw_ref = abs(self.bw)
        f = self.freqs[0]
        ok = np.flatnonzero((self.nu_ref - self.bw_ref / 2 < f) *
                            (self.nu_ref + self.bw_ref / 2 > f) *
                            self.masks[0, 0].mean(axis=1))
        return np.take(self.port, ok, axis=0).mean(axis=0)  # unweighted

    # -- the model ----------------------------------------------------------
    def _start_model(self, modelfile, ref_prof, tau, fixloc, fixwid, fixamp, fixscat, fixalpha,
                     scattering_index, model_code, fiducial_gaussian, auto_gauss, model_name,
                     init_params, max_ngauss=0):
        """The starting parameters and flags (ppgauss.py:99-159)."""
        if modelfile:
            (self.model_name, self.model_code, self.nu_ref, self.ngauss, self.init_model_params,
             self.fit_flags, self.scattering_index, self.fitalpha) = read_model(modelfile)
            self.fixalpha = not self.fitalpha
            if model_name is not None:
                self.model_name = model_name
            self.init_model_params = np.array(self.init_model_params, dtype=np.float64)
            self.init_model_params[1] *= self.nbin / self.Ps[0]  # TAU [s] -> [bin]
            return
        self.model_code = model_code
        self.scattering_index = scattering_index
        self.fixalpha = fixalpha
        self.fitalpha = int(not self.fixalpha)
        self.model_name = self.source if model_name is None else model_name
        if init_params is not None or not len(self.init_params):
            profile = self._ref_profile(ref_prof)
            self.fit_profile(profile, tau=tau, fixscat=fixscat, auto_gauss=auto_gauss,
                             profile_fit_flags=None, show=False, init_params=init_params,
                             max_ngauss=max_ngauss)
        ip = np.asarray(self.init_params, dtype=np.float64)
        comps = np.zeros((self.ngauss, 6))  # slopes and spectral indices start at 0
        comps[:, 0], comps[:, 2], comps[:, 4] = ip[2::3], ip[3::3], ip[4::3]
        self.init_model_params = np.concatenate([ip[:2], comps.ravel()])
        self.fit_flags = np.ones(len(self.init_model_params))
        self.fit_flags[1] *= not fixscat
        self.fit_flags[3::6] *= not fixloc
        self.fit_flags[5::6] *= not fixwid
        self.fit_flags[7::6] *= not fixamp
        if fiducial_gaussian:
            self.fit_flags[3::6] = 1
            self.fit_flags[3::6][0] = 0

    def make_gaussian_model(self, modelfile=None, ref_prof=(None, None), tau=0.0, fixloc=False,
                            fixwid=False, fixamp=False, fixscat=True, fixalpha=True,
                            scattering_index=scattering_alpha, model_code=default_model, niter=0,
                            fiducial_gaussian=False, auto_gauss=0.0, writemodel=False,
                            outfile=None, writeerrfile=False, errfile=None, model_name=None,
                            residplot=None, quiet=False, init_params=None, max_ngauss=0):
        """Fit a Gaussian-component model with independently evolving
        components (ppgauss.py:55-238; the arguments are the reference's;
        in place of the GUI, init_params seeds the profile fit or
        max_ngauss > 0 searches for its components)."""
        make_gaussian_models(
            [self], modelfiles=[modelfile], ref_prof=ref_prof, tau=tau, fixloc=fixloc,
            fixwid=fixwid, fixamp=fixamp, fixscat=fixscat, fixalpha=fixalpha,
            scattering_index=scattering_index, model_code=model_code, niter=niter,
            fiducial_gaussian=fiducial_gaussian, auto_gauss=auto_gauss, writemodel=writemodel,
            outfiles=[outfile], writeerrfile=writeerrfile, errfiles=[errfile],
            model_names=[model_name], residplot=residplot, quiet=quiet, init_params=[init_params],
            max_ngauss=max_ngauss)

    def _fit_inputs(self):
        """fit_gaussian_portrait's arguments of model_iteration (ppgauss.py:246-250)."""
        return (self.model_code, self.portx, self.model_params, self.scattering_index,
                self.noise_stdsxs, self.fit_flags, not self.fixalpha, self.freqsxs[0], self.nu_ref,
                self.all_join_params, self.Ps[0])

    def _take_fit(self, fgp, duration):
        """model_iteration after the fit (ppgauss.py:251-275)."""
        self.fitted_params, self.fit_errs, self.chi2, self.dof = (
            fgp.fitted_params, fgp.fit_errs, fgp.chi2, fgp.dof)
        self.scattering_index, self.scattering_index_err = (fgp.scattering_index,
                                                            fgp.scattering_index_err)
        self.fgp = fgp
        if self.njoin:
            self.model_params = self.fitted_params[:-self.njoin * 2]
            self.model_param_errs = self.fit_errs[:-self.njoin * 2]
            self.join_params = self.fitted_params[-self.njoin * 2:]
            self.join_param_errs = self.fit_errs[-self.njoin * 2:]
            self.all_join_params[1] = self.join_params
            self.write_join_parameters()
        else:
            self.model_params = self.fitted_params[:]
            self.model_param_errs = self.fit_errs[:]
        self.model = pplib.gen_gaussian_portraits_device(
            self.model_code, self.fitted_params, self.scattering_index, self.nbin, self.freqs[0],
            self.nu_ref, self.join_ichans, self.Ps[0])
        self.model_masked = self.model * self.masks[0, 0]
        self.modelx = np.compress(self.masks[0, 0].mean(axis=1), self.model, axis=0)
        self.duration = duration
        self.total_time += duration

    def model_iteration(self, quiet=False):
        """Iterate over a model fit (ppgauss.py:240-276)."""
        while True:
            _fit_batch([self], quiet)
            yield

    def check_convergence(self, efac=1.0, quiet=False):
        """Whether the phase and DM of the data, as measured by the fitted
        model, are within their errors times efac (ppgauss.py:278-334).  As
        there: 1, or a falsy value (0 when the phase is outside, None when
        only the DM is)."""
        if self.njoin:  # both without the fitted join rotations
            portx, modelx = (pplib.rotate_join_rows(rows, self.join_ichanxs, self.join_params,
                                                    self.Ps[0], self.freqsxs[0], self.nu_ref, -1.0)
                             for rows in (self.portx, self.modelx))
        else:
            portx, modelx = np.copy(self.portx), np.copy(self.modelx)
        phase_guess = fit_phase_shift(portx.mean(axis=0), modelx.mean(axis=0)).phase % 1
        if phase_guess >= 0.5:
            phase_guess -= 1.0
        fp = fit_portrait(portx, modelx, np.array([phase_guess, 0.0]), self.Ps[0], self.freqsxs[0],
                          self.nu_fit, None, None, bounds=[(None, None), (None, None)], id=None,
                          quiet=True)
        self.fp_results = fp
        self.phi, self.phierr, self.DM, self.DMerr, self.red_chi2 = (
            fp.phase, fp.phase_err, fp.DM, fp.DM_err, fp.red_chi2)
        if not quiet:
            print("Iter %d:" % (self.itern - self.niter))
            print(" duration of %.2f min" % (self.duration / 60.))
            print(" phase offset of %.2e +/- %.2e [rot]" % (self.phi, self.phierr))
            print(" DM of %.6e +/- %.2e [cm**-3 pc]" % (self.DM, self.DMerr))
            print(" red. chi**2 of %.2f." % self.red_chi2)
        if min(abs(self.phi), abs(1 - self.phi)) < abs(self.phierr) * efac:
            if abs(self.DM) < abs(self.DMerr) * efac:
                if not quiet:
                    print("\nIteration converged.\n")
                return 1
            return None
        return 0

    def write_model(self, outfile=None, append=False, quiet=False):
        """Write the model parameters to file (ppgauss.py:336-354): loc >= 1
        wrapped, tau in seconds."""
        if outfile is None:
            outfile = self.datafile + ".gmodel"
        model_params = np.copy(self.model_params)
        model_params[2::6] = np.where(model_params[2::6] >= 1.0, model_params[2::6] % 1,
                                      model_params[2::6])
        model_params[1] *= self.Ps[0] / self.nbin
        pplib.write_model(outfile, self.model_name, self.model_code, self.nu_ref, model_params,
                          self.fit_flags, self.scattering_index, self.fitalpha, append=append,
                          quiet=quiet)

    def write_errfile(self, errfile=None, append=False, quiet=False):
        """Write the parameter uncertainties to file (ppgauss.py:356-372)."""
        if errfile is None:
            errfile = self.datafile + ".gmodel_errs"
        errs = np.copy(self.model_param_errs)
        errs[1] *= self.Ps[0] / self.nbin
        pplib.write_model(errfile, self.model_name + "_errors", self.model_code, self.nu_ref, errs,
                          self.fit_flags, self.scattering_index_err, self.fitalpha, append=append,
                          quiet=quiet)


def _fit_batch(dps, quiet):
    """One model_iteration step of every portrait, in one device call."""
    start = time.time()
    args = [dp._fit_inputs() for dp in dps]
    cols = list(zip(*args))
    joined = dps[0].njoin > 0
    fgps = fit_gaussian_portraits(cols[0], cols[1], cols[2], cols[3], cols[4], cols[5], cols[6],
                                  dps[0].phases, cols[7], cols[8],
                                  join_params=cols[9] if joined else [],
                                  Ps=cols[10] if joined else None, quiet=quiet)
    duration = (time.time() - start) / len(dps)
    for dp, fgp in zip(dps, fgps):
        dp._take_fit(fgp, duration)


def make_gaussian_models(portraits, modelfiles=None, ref_prof=(None, None), tau=0.0, fixloc=False,
                         fixwid=False, fixamp=False, fixscat=True, fixalpha=True,
                         scattering_index=scattering_alpha, model_code=default_model, niter=0,
                         fiducial_gaussian=False, auto_gauss=0.0, writemodel=False, outfiles=None,
                         writeerrfile=False, errfiles=None, model_names=None, residplot=None,
                         quiet=False, init_params=None, max_ngauss=0):
    """make_gaussian_model for a list of DataPortraits whose unzapped
    portraits share one shape, component count and number of joined archives
    (metafile portraits): each iteration's portrait
    fits run in one ppf_gauss_fit_batch call, and with max_ngauss > 0 the
    reference profiles of all portraits that need the component search go
    through one pplib.auto_gaussian_profiles call.  The results are those of
    the one-by-one calls, exactly.  modelfiles, outfiles, errfiles,
    model_names and init_params are lists (None: the default for every
    portrait)."""
    if residplot:
        raise NotImplementedError("residplot (plotting) is not supported")
    dps = list(portraits)
    if not dps:
        return dps
    n = len(dps)
    modelfiles, outfiles, errfiles, model_names, init_params = (
        [None] * n if v is None else list(v)
        for v in (modelfiles, outfiles, errfiles, model_names, init_params))
    search = [i for i, dp in enumerate(dps)
              if not modelfiles[i] and init_params[i] is None and not len(dp.init_params)
              and not auto_gauss and max_ngauss]
    if search:
        found = auto_gaussian_profiles([dps[i]._ref_profile(ref_prof) for i in search], None,
                                       max_ngauss, DataPortrait._search_tau(tau, fixscat),
                                       not fixscat)
        for i, f in zip(search, found):
            dps[i]._take_search(f)
    for i, dp in enumerate(dps):
        if modelfiles[i]:
            if outfiles[i] is None:
                outfiles[i] = modelfiles[i]
        if errfiles[i] is None and outfiles[i] is not None:
            errfiles[i] = outfiles[i] + "_errs"
        dp._start_model(modelfiles[i], ref_prof, tau, fixloc, fixwid, fixamp, fixscat, fixalpha,
                        scattering_index, model_code, fiducial_gaussian, auto_gauss,
                        model_names[i], init_params[i], max_ngauss)
        dp.nu_fit = guess_fit_freq(dp.freqsxs[0], dp.SNRsxs)
        dp.niter = dp.itern = max(int(niter), 0)
        dp.model_params = np.copy(dp.init_model_params)
        dp.total_time = 0.0
        dp.start = time.time()
    shape = (dps[0].portx.shape, dps[0].ngauss, dps[0].njoin)
    for dp in dps:
        if (dp.portx.shape, dp.ngauss, dp.njoin) != shape:
            raise ValueError("make_gaussian_models: portraits of %s and %s (unzapped channels x "
                             "bins, components, joined archives); one shape per call"
                             % (shape, (dp.portx.shape, dp.ngauss, dp.njoin)))

    def finish(batch):
        for dp in batch:
            dp.cnvrgnc = dp.check_convergence(efac=1.0, quiet=quiet)
            i = dps.index(dp)
            if writemodel:
                dp.write_model(outfile=outfiles[i], quiet=quiet)
            if writeerrfile:
                dp.write_errfile(errfile=errfiles[i], quiet=quiet)

    if not quiet:
        print("Fitting Gaussian model portrait...")
    _fit_batch(dps, quiet)
    finish(dps)
    while True:
        todo = [dp for dp in dps if dp.niter and not dp.cnvrgnc]
        if not todo:
            break
        for dp in todo:
            if not quiet:
                print("\n...iteration %d..." % (dp.itern - dp.niter + 1))
            if dp.njoin:  # the join parameters carry the alignment (ppgauss.py:191)
                continue
            dp.port = rotate_data(dp.port, dp.phi, dp.DM, dp.Ps[0], dp.freqs[0], dp.nu_fit)
            dp.portx = rotate_data(dp.portx, dp.phi, dp.DM, dp.Ps[0], dp.freqsxs[0], dp.nu_fit)
        _fit_batch(todo, quiet)
        for dp in todo:
            dp.niter -= 1
        finish(todo)
    for dp in dps:
        if dp.njoin:  # data and model without the fitted join rotations (ppgauss.py:206-224)
            args = (dp.join_params, dp.Ps[0])
            dp.port = pplib.rotate_join_rows(dp.port, dp.join_ichans, *args, dp.freqs[0],
                                             dp.nu_ref, -1.0)
            dp.portx = pplib.rotate_join_rows(dp.portx, dp.join_ichanxs, *args, dp.freqsxs[0],
                                              dp.nu_ref, -1.0)
            dp.model = pplib.rotate_join_rows(dp.model, dp.join_ichans, *args, dp.freqs[0],
                                              dp.nu_ref, -1.0)
            dp.model_masked = dp.model * dp.masks[0, 0]
            dp.modelx = np.compress(dp.masks[0, 0].mean(axis=1), dp.model, axis=0)
    if not quiet:
        for dp in dps:
            print("")
            print("Residuals mean: %.2e" % (dp.portx - dp.modelx).mean())
            print("Residuals std:  %.2e" % (dp.portx - dp.modelx).std())
            print("Data std:       %.2e\n" % np.median(dp.noise_stdsxs))
            print("Total fit time: %.2f min" % (dp.total_time / 60.0))
            print("Total time:     %.2f min\n" % ((time.time() - dp.start) / 60.0))
    return dps
