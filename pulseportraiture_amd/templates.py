"""The one place GetTOAs' template portraits come from.

TemplateSource parses the model file once (archive template, .gmodel or
ppspline model) and builds portraits for rows of channel frequencies on the
device.  The drivers in pptoas.py differ only in policy, each after a line of
the reference:

driver                P (TAU * nbin / P)     response: P, chan_bw      scattered                  one template per
--------------------  ---------------------  ------------------------  -------------------------  ---------------------------
get_TOAs              the subint's           the subint's P; |f[1] -   no under fit_scat (TAU 0,  frequency row (+ P when
 (pptoas.py:351-393)  (:355-358)             f[0]| of its ok channels  index 0.0, :368-374),      TAU != 0); with the response
                                             (:387-393)                else yes                   also chan_bw (+ P when DM)
get_narrowband_TOAs   the subint's           the subint's P; ok        no under fit_scat          (frequency row, P); with the
 (pptoas.py:888-926)  (:892-895)             channels (:920-926)       (:896-911), else yes       response the subint
show_fit, get_        data.Ps.mean()         the subint's P; |f[1] -   no where the fitted tau    (frequency row, fitted
 channels_to_zap      (:1369-1371)           f[0]| of all channels     != 0 (:1372-1378), else    tau != 0); with the
 (pptoas.py:1356-88)                         (:1382-1388)              yes                        response the subint

An archive template (pptoas.py:323-338, 859-880, 1356-1366) is one portrait
for every subint; a ppspline model (:375-378, 912-915, 1379-1381) has no TAU.
"""
import numpy as np

from . import archive as _arch
from .engine import get_engine
from .pplib import gen_gaussian_portraits_device, load_spline_model_file, read_model


def row_keys(rows):
    """First-appearance index of every distinct row, and each row's index
    into those (np.unique on the rows, renumbered in order of appearance)."""
    rows = np.ascontiguousarray(rows)
    if (rows == rows[0]).all():
        return np.zeros(1, dtype=np.int64), np.zeros(len(rows), dtype=np.int64)
    v = rows.view(np.dtype((np.void, rows.dtype.itemsize * rows.shape[1]))).ravel()
    _, first, inv = np.unique(v, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    return first[order], rank[inv.ravel()]


def chan_bw(freqs):
    """instrumental_response_port_FT's |freqs[1] - freqs[0]| (pptoaslib.py:174);
    0 for one channel, where the reference's raises IndexError."""
    return abs(freqs[1] - freqs[0]) if len(freqs) > 1 else 0.0


class TemplateSource:
    """A model file, parsed once: kind is "fits", "gmodel" (with read_model's
    name, code, nu_ref, ngauss, gparams, alpha) or "spline" (with name and
    spline = [mean_prof, eigvec, tck]).  gaussian builds the Gaussian portraits
    (a driver passes the builder its own module holds)."""

    def __init__(self, modelfile, is_FITS_model, gaussian=gen_gaussian_portraits_device):
        self.modelfile, self._gaussian = modelfile, gaussian
        self._fits = None
        if is_FITS_model:
            self.kind, self.name = "fits", modelfile
            return
        try:
            (self.name, self.code, self.nu_ref, self.ngauss, self.gparams, _, self.alpha,
             _) = read_model(modelfile, quiet=True)
            self.kind = "gmodel"
        except UnboundLocalError:  # not a .gmodel: a ppspline model (pptoas.py:375-378)
            self.name, _, _, *self.spline = load_spline_model_file(modelfile)
            self.kind = "spline"

    def fits(self, nchan=None):
        """(load_data bunch, portrait) of the archive template (pptoas.py:323-338):
        tscrunched, baseline removed, masked; one channel is tiled to nchan."""
        if self._fits is None:
            md = _arch.load_data(self.modelfile, dedisperse=False, dededisperse=False,
                                 tscrunch=True, pscrunch=True, rm_baseline=True, quiet=True)
            self._fits = md, np.asarray((md.masks * md.subints)[0, 0])
        md, model = self._fits
        if md.nchan == 1 and nchan is not None:
            model = np.tile(model[0], nchan).reshape(nchan, md.nbin)
        return md, model

    def portraits(self, freq_rows, nbin, P=None, scattered=True):
        """The model at every row of freq_rows as numpy [nrow, nchan, nbin]:
        read_model's TAU * nbin / P (pplib.py:2936-2942), P a scalar or one
        per row, in one batched device build per distinct P; scattered=False:
        TAU = 0 and scattering index 0.0.  A spline model: one build."""
        f = np.atleast_2d(freq_rows)
        if self.kind == "spline":
            return get_engine().spline_portraits(*self.spline, f, nbin).cpu().numpy()
        params, alpha = np.array(self.gparams, dtype=float), self.alpha
        if not scattered:
            params[1], alpha = 0.0, 0.0
        if params[1] == 0.0:
            return self._gaussian(self.code, params, alpha, nbin, f, self.nu_ref)
        P = np.broadcast_to(np.asarray(P, dtype=np.float64), len(f))
        out = np.empty(f.shape + (nbin,))
        for p in np.unique(P):
            sel = np.flatnonzero(P == p)
            pp = np.copy(params)
            pp[1] *= nbin / p
            out[sel] = self._gaussian(self.code, pp, alpha, nbin, f[sel], self.nu_ref)
        return out

    @staticmethod
    def respond(model, freqs, P, cbw, ird):
        """model [nchan, nbin] convolved with instrumental_response_port_FT(nbin,
        freqs, DM, P, wids, irf_types) (pptoas.py:387-393), on the device."""
        return get_engine().instrumental_response_rows(
            np.asarray(model, dtype=np.float64), freqs, ird["DM"], P, ird["wids"],
            ird["irf_types"], chan_bw=cbw).cpu().numpy()
