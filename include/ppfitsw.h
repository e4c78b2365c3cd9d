/* ppfitsw.h -- streaming fold-mode PSRFITS writer (libppfits.so, host only).
 *
 * The counterpart of ppfits.h for pplib.write_archive / unload_new_archive /
 * make_fake_pulsar (pplib.py:3039-3384) and ppalign's averaged archive
 * (ppalign.py:227-243), which the reference unloads through PSRCHIVE.  The
 * file follows the PSRFITS definition (the layout ppfits.h reads): a primary
 * header, a HISTORY table whose one row carries DEDISP, a PSRPARAM table with
 * the ephemeris text, and the SUBINT table with 16-bit samples
 * (DATA * DAT_SCL + DAT_OFFS, as ppf_pack_subints of ppfit.h quantises them).
 * There is no POLYCO table: the constant folding period goes into the SUBINT
 * PERIOD column.
 *
 * Subints are appended in chunks, in order, so a producer can make the next
 * chunk while this one is written; ppfw_close fills in the row counts and
 * pads the file.  Samples arrive in native byte order and are swapped to
 * FITS's big-endian order on the copy into the row buffer.
 *
 * Every function returns 0 or a negative PPFITS_ERR_* (ppfits.h);
 * ppfw_error() holds the reason.
 */
#ifndef PPFITSW_H
#define PPFITSW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ppfw_file ppfw_file;

typedef struct {
  int32_t npol, nchan, nbin;
  int32_t dedispersed;        /* HISTORY DEDISP: the data are DM corrected      */
  int32_t stt_imjd;           /* start MJD, integer day                         */
  int32_t stt_smjd;           /* start second of the day                        */
  double stt_offs;            /* start fractional second                        */
  double obsfreq, obsbw;      /* centre frequency, bandwidth [MHz]              */
  double dm;                  /* SUBINT DM and primary CHAN_DM [cm**-3 pc]      */
  double be_delay;            /* primary BE_DELAY [s]                           */
  char telescope[32], frontend[32], backend[32], source[32];
  char pol_type[16];          /* SUBINT POL_TYPE: AA+BB, IQUV, AABBCRCI         */
  char ra[32], dec[32];       /* hh:mm:ss.sss, +dd:mm:ss.sss                    */
} ppfw_desc;

/* Create path (truncated if it exists) and write everything up to the first
 * SUBINT row.  ephemeris: the parameter file's text (NULL or "": an empty
 * PSRPARAM table), one PSRPARAM row per line.  *out is set even on failure
 * (read the error, then ppfw_close).                                          */
int ppfw_create(const char* path, const ppfw_desc* desc, const char* ephemeris, ppfw_file** out);

/* Append subints [isub0, isub0 + n); isub0 must be the number written so far
 * (PPFITS_ERR_RANGE otherwise).  Host arrays, C order:
 *   raw [n][npol][nchan][nbin] int16, native byte order;
 *   scl, offs [n][npol][nchan] (stored as float32: pass float32-exact values);
 *   freqs, wts [n][nchan] (DAT_FREQ as D, DAT_WTS as E);
 *   tsubint, offs_sub, period, par_ang [n] (par_ang NULL: zeros).            */
int ppfw_write_subints(ppfw_file* f, int32_t isub0, int32_t n, const int16_t* raw,
                       const double* scl, const double* offs, const double* freqs,
                       const double* wts, const double* tsubint, const double* offs_sub,
                       const double* period, const double* par_ang);

/* Fix NAXIS2 of SUBINT and NSUB of HISTORY, pad to 2880 bytes, close and
 * free f.  Returns the first error of the file's life, if any.              */
int ppfw_close(ppfw_file* f);

const char* ppfw_error(const ppfw_file* f);

/* Set DAT_WTS[isub[i]][ichan[i]] = wts[i], i < n, of the existing fold-mode
 * PSRFITS file at path, in place: the stand-in for `paz -m`.  Only the bytes
 * of those cells change (each is written in the column's own type, E or D);
 * the header, the history, the polyco and every sample stay as they were.
 * Any fold-mode file ppfits.h reads can be patched, this writer's own
 * included.  Everything is checked before the first byte is written:
 *   PPFITS_ERR_FORMAT  not FITS, OBS_MODE other than PSR / CAL, no SUBINT
 *                      table or DAT_WTS column, or a SUBINT HDU that carries
 *                      CHECKSUM / DATASUM -- such a file is REFUSED, not
 *                      re-summed (this writer emits neither keyword);
 *   PPFITS_ERR_RANGE   a subint or channel outside the table;
 * and the file is then untouched.  err (may be NULL) receives the reason,
 * at most errlen bytes with the terminator.                                 */
int ppfw_patch_weights(const char* path, int32_t n, const int32_t* isub, const int32_t* ichan,
                       const double* wts, char* err, size_t errlen);

#ifdef __cplusplus
}
#endif

#endif /* PPFITSW_H */
