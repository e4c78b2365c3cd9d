"""ppzap drop-in: flag bad channels (ppzap.py:18-95).

Two algorithms, as in the reference:
- ``GetTOAs.get_channels_to_zap`` (pptoas.py:1201-1278) after ``get_TOAs``:
  per-channel reduced chi2 of the fitted portrait (one fused device call per
  archive, ppf_resid_chi2_rows) plus the iterated S/N cut;
- ``get_zap_channels`` (ppzap.py:18-48): the iterated median + nstd * std cut
  on the channel noise levels -- nchan numbers per subint, host arithmetic.

``print_paz_cmds`` writes the PSRCHIVE ``paz`` commands (ppzap.py:50-95);
``apply_zap_channels`` and ``run_paz_cmds`` carry them out on PSRFITS files
without PSRCHIVE (DAT_WTS patched in place, psrfits.patch_weights) -- a
defined stand-in for paz, not pinned against it.
The command-line front end is out of scope.
"""
import re
import shutil
import sys

import numpy as np


def get_zap_channels(data, nstd=3):
    """Channels whose noise is more than nstd standard deviations above the
    subint median, removed and re-tested until none is flagged
    (ppzap.py:18-48).  ``data`` needs ok_isubs, ok_ichans and noise_stds."""
    zap_channels = []
    noise_stds = np.asarray(data.noise_stds)
    for isub in data.ok_isubs:
        ichans = list(np.copy(data.ok_ichans[isub]))
        zap_ichans = []
        while len(ichans):
            ns = noise_stds[isub, 0, ichans]
            median = np.median(ns)
            std = np.std(ns)
            bad = list(np.where(ns > median + nstd * std)[0])
            if not len(bad):
                break
            flagged = list(np.array(ichans)[bad])
            zap_ichans.extend(flagged)
            for ichan in flagged:
                ichans.pop(ichans.index(ichan))
        zap_ichans.sort()
        zap_channels.append(zap_ichans)
    return zap_channels


def print_paz_cmds(datafiles, zap_list, all_subs=False, modify=True, outfile=None,
                   quiet=False):
    """Print (or append to outfile) the paz commands that zap zap_list[iarch][isub]
    (ppzap.py:50-95).  Returns the lines written."""
    if not len(datafiles) or not len(zap_list):
        if not quiet:
            print("Nothing to zap.")
            return None
    lines = _paz_lines(datafiles, zap_list, all_subs, modify)
    out = open(outfile, "a") if outfile is not None else sys.stdout
    try:
        for line in lines:
            out.write(line + "\n")
    finally:
        if outfile is not None:
            out.close()
    if outfile is not None and not quiet:
        print("Wrote %s." % outfile)
    return lines


def _paz_plan(datafiles, zap_list, all_subs, modify):
    """What print_paz_cmds' lines do, in their order, as operations: ("copy",
    F) for `paz -e zap F`, ("zap", F, C, S) for `paz -m -I -z C -w S F` and
    ("zap", F, C, None) for `paz -m -z C F` (ppzap.py:50-95; with all_subs a
    line equal to the one before it is not repeated)."""
    ops = []
    paz_outfile = None
    for iarch, datafile in enumerate(datafiles):
        count = sum(len(z) for z in zap_list[iarch])
        if count:
            if modify:
                paz_outfile = datafile
            else:
                paz_outfile = _zap_name(datafile)
                ops.append(("copy", datafile))
        last = None
        for isub, bad_ichans in enumerate(zap_list[iarch]):
            for bad_ichan in bad_ichans:
                if not all_subs:
                    ops.append(("zap", paz_outfile, int(bad_ichan), isub))
                else:
                    op = ("zap", paz_outfile, int(bad_ichan), None)
                    if op != last:
                        ops.append(op)
                    last = op
    return ops


def _paz_lines(datafiles, zap_list, all_subs, modify):
    """The command lines of print_paz_cmds."""
    lines = []
    for op in _paz_plan(datafiles, zap_list, all_subs, modify):
        if op[0] == "copy":
            lines.append("paz -e zap %s" % op[1])
        elif op[3] is not None:
            lines.append("paz -m -I -z %d -w %d %s" % (op[2], op[3], op[1]))
        else:
            lines.append("paz -m -z %d %s" % (op[2], op[1]))
    return lines


def _zap_name(datafile):
    """The file `paz -e zap datafile` writes: the extension replaced by zap,
    or .zap appended (print_paz_cmds' rule: everything after the last "." of
    the name as given, directories included)."""
    ii = datafile[::-1].find(".")
    return datafile + ".zap" if ii < 0 else datafile[:-ii] + "zap"


_PAZ_FORMS = (
    (re.compile(r"paz\s+-e\s+zap\s+(\S+)"), lambda m: ("copy", m.group(1))),
    (re.compile(r"paz\s+-m\s+-I\s+-z\s+(\d+)\s+-w\s+(\d+)\s+(\S+)"),
     lambda m: ("zap", m.group(3), int(m.group(1)), int(m.group(2)))),
    (re.compile(r"paz\s+-m\s+-z\s+(\d+)\s+(\S+)"),
     lambda m: ("zap", m.group(2), int(m.group(1)), None)),
)


def _parse_paz(line):
    for rx, make in _PAZ_FORMS:
        m = rx.fullmatch(line.strip())
        if m:
            return make(m)
    raise ValueError("run_paz_cmds: not one of `paz -e zap F`, `paz -m -I -z C -w S F`, "
                     "`paz -m -z C F`: %r" % line)


def _run_paz(ops, quiet):
    """Carry out parsed commands in order.  Consecutive zaps of a file become
    one psrfits.patch_weights call (every cell checked before the file is
    touched); a copy first flushes the zaps pending on its source."""
    from . import psrfits
    pending, written = {}, []

    def flush(name):
        cells = pending.pop(name, [])
        if not cells:
            return
        f = psrfits.PSRFITSFile(name)
        nsub = f.nsub
        f.close()
        isubs, ichans = [], []
        for ichan, isub in cells:
            for s in (range(nsub) if isub is None else (isub,)):
                isubs.append(s)
                ichans.append(ichan)
        psrfits.patch_weights(name, isubs, ichans, 0.0)
        if not quiet:
            print("Zapped %d profiles of %s." % (len(set(zip(isubs, ichans))), name))

    for op in ops:  # before anything is written
        if op[0] == "copy" and op[1].endswith("."):  # the rule would name the copy "zap"
            raise ValueError("%r ends in '.': no extension to replace by zap" % op[1])
    for op in ops:
        if op[0] == "copy":
            flush(op[1])
            dst = _zap_name(op[1])
            pending.pop(dst, None)  # overwritten
            shutil.copyfile(op[1], dst)
            name = dst
        else:
            name = op[1]
            pending.setdefault(name, []).append((op[2], op[3]))
        if name not in written:
            written.append(name)
    for name in list(pending):
        flush(name)
    return written


def run_paz_cmds(lines_or_path, quiet=True):
    """Carry out saved print_paz_cmds output without PSRCHIVE: a list of
    lines, or the path of a command file.  Exactly three forms are taken,

        paz -e zap F             copy F to its name with the extension zap
        paz -m -I -z C -w S F    weight 0 for channel C of subint S, in place
        paz -m -z C F            weight 0 for channel C of every subint

    (blank lines skipped; F holds no whitespace, as in a shell command without
    quotes).  Any other line raises ValueError naming it, and
    nothing is applied before the whole input has parsed.  Only DAT_WTS
    cells change (psrfits.patch_weights).  Returns the files written."""
    if isinstance(lines_or_path, str):
        with open(lines_or_path) as f:
            lines = f.read().splitlines()
    else:
        lines = list(lines_or_path)
    ops = [_parse_paz(line) for line in lines if line.strip()]
    return _run_paz(ops, quiet)


def apply_zap_channels(datafiles, zap_list, all_subs=False, modify=False, quiet=False):
    """Do what the lines of print_paz_cmds(datafiles, zap_list, all_subs,
    modify) would do under PSRCHIVE: with modify=False copy each archive
    that has something flagged to the name with the extension zap (an
    archive with nothing flagged is not copied), then set DAT_WTS to 0 for
    every flagged (subint, channel) -- with all_subs, for the channel in
    every subint -- in the copy, or with modify=True in the file itself.
    Nothing else of the file changes.  The operations are those the lines
    stand for, made by the same code (_paz_plan), not the lines parsed back:
    a name may hold anything, whitespace included.  A name ending in "."
    is a ValueError.  Returns the names written."""
    if not len(datafiles) or not len(zap_list):
        if not quiet:
            print("Nothing to zap.")
        return []
    return _run_paz(_paz_plan(datafiles, zap_list, all_subs, modify), quiet)
