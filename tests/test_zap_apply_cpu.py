"""Zap lists applied without PSRCHIVE, no device: ppfw_patch_weights
(include/ppfitsw.h) and ppzap.apply_zap_channels / run_paz_cmds on a 3-subint
x 8-channel x 64-bin file written by the package's own writer.

- a patch changes only the bytes of the DAT_WTS cells named (byte-for-byte
  comparison, the cells located by an independent parse of the file), the
  reader returns the new weights, patching twice leaves the same file, and
  what is refused -- an index outside the table, a file that is not fold
  mode, a SUBINT checksum -- leaves the file untouched;
- run_paz_cmds(print_paz_cmds(...)) writes the files apply_zap_channels
  writes, for all_subs and modify both ways and with an archive that has
  nothing flagged (not copied); an unknown command raises before anything is
  written;
- tools/patch_weights_check.cpp, a stand-alone program around the new entry
  point, builds with -fsanitize=address,undefined and runs clean."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from pulseportraiture_amd.mjd import MJD
from tests.test_psrfits_write_cpu import columns, parse_fits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSUB, NPOL, NCHAN, NBIN = 3, 1, 8, 64


@pytest.fixture(scope="module")
def lib():
    from pulseportraiture_amd import build
    build.build_fits()
    from pulseportraiture_amd import psrfits
    return psrfits


def write_file(lib, path, nsub=NSUB, seed=0):
    rng = np.random.default_rng(seed)
    shape = (nsub, NPOL, NCHAN, NBIN)
    raw = rng.integers(-32767, 32768, size=shape).astype(np.int16)
    scl = rng.uniform(1e-3, 2.0, size=shape[:3]).astype(np.float32).astype(np.float64)
    offs = rng.normal(size=shape[:3]).astype(np.float32).astype(np.float64)
    freqs = np.tile(np.linspace(1100.0, 1900.0, NCHAN), (nsub, 1))
    wts = rng.uniform(0.5, 2.0, size=(nsub, NCHAN)).astype(np.float32).astype(np.float64)
    w = lib.PSRFITSWriter(str(path), NPOL, NCHAN, NBIN, MJD(57300, 43200, 0.25), 1500.0, 800.0,
                          DM=12.5, state="Intensity", ephemeris="PSR J0000+0000\nF0 100.0\nDM 12.5\n")
    w.write(raw, scl, offs, freqs, wts, np.full(nsub, 10.0), 5.0 + 10.0 * np.arange(nsub),
            np.full(nsub, 0.01))
    w.close()
    return str(path), wts


@pytest.fixture()
def fits(lib, tmp_path):
    return write_file(lib, tmp_path / "a.fits")


def wts_cells(blob):
    """Byte range (start, width) of DAT_WTS[isub][ichan] for every cell, from
    an independent parse of the file."""
    assert [h[0].get("EXTNAME") for h in parse_fits(blob)][-1] == "SUBINT"
    pos, cells = 0, {}
    while pos < len(blob):
        cards = {}
        end = False
        while not end:
            block = blob[pos:pos + 2880].decode("ascii")
            pos += 2880
            for c in range(0, 2880, 80):
                card = block[c:c + 80]
                if card.startswith("END "):
                    end = True
                    break
                if card[8:10] == "= ":
                    v = card[10:]
                    cards[card[:8].strip()] = v.split("/")[0].strip().strip("'").strip()
        n = int(cards["NAXIS1"]) * int(cards["NAXIS2"]) if int(cards["NAXIS"]) else 0
        if cards.get("EXTNAME") == "SUBINT":
            cols, row = columns(cards)
            name, rep, t, coff = [c for c in cols if c[0] == "DAT_WTS"][0]
            assert t == "E" and rep == NCHAN
            for s in range(int(cards["NAXIS2"])):
                for c in range(rep):
                    cells[(s, c)] = (pos + s * row + coff + 4 * c, 4)
        pos += (n + 2879) // 2880 * 2880
    return cells


def changed_bytes(a, b):
    assert len(a) == len(b)
    return set(np.flatnonzero(np.frombuffer(a, np.uint8) != np.frombuffer(b, np.uint8)).tolist())


def read_weights(lib, path):
    f = lib.PSRFITSFile(path)
    w = f.meta()["weights"]
    f.close()
    return w


def test_patch_changes_only_the_cells(lib, fits):
    path, wts = fits
    before = open(path, "rb").read()
    cells = wts_cells(before)
    assert len(cells) == NSUB * NCHAN
    named = [(0, 1), (2, 7), (1, 3)]
    lib.patch_weights(path, [s for s, _ in named], [c for _, c in named], [0.0, 0.0, 0.25])
    after = open(path, "rb").read()
    allowed = set()
    for key in named:
        a, n = cells[key]
        allowed.update(range(a, a + n))
    diff = changed_bytes(before, after)
    assert diff and diff <= allowed
    # every named cell did change (none of the original weights is 0 or 0.25)
    for key in named:
        a, n = cells[key]
        assert diff & set(range(a, a + n))
    want = wts.copy()
    want[0, 1] = want[2, 7] = 0.0
    want[1, 3] = 0.25
    np.testing.assert_array_equal(read_weights(lib, path), want)
    # the same patch again: the same file
    lib.patch_weights(path, [s for s, _ in named], [c for _, c in named], [0.0, 0.0, 0.25])
    assert open(path, "rb").read() == after
    # one value broadcast over several cells
    lib.patch_weights(path, [0, 1, 2], 5, 0.0)
    want[:, 5] = 0.0
    np.testing.assert_array_equal(read_weights(lib, path), want)


@pytest.mark.parametrize("isub,ichan", [(NSUB, 0), (0, NCHAN), (-1, 0), (0, -1), ([0, NSUB], [1, 1])])
def test_out_of_range_leaves_the_file(lib, fits, isub, ichan):
    path, _ = fits
    before = open(path, "rb").read()
    with pytest.raises(lib.PSRFITSError, match="outside"):
        lib.patch_weights(path, isub, ichan, 0.0)
    assert open(path, "rb").read() == before


def test_not_fold_mode_and_checksum_refused(lib, fits, tmp_path):
    path, _ = fits
    blob = open(path, "rb").read()
    # a search-mode primary header
    i = blob.index(b"OBS_MODE= 'PSR     '")
    search = str(tmp_path / "search.fits")
    open(search, "wb").write(blob[:i] + b"OBS_MODE= 'SEARCH  '" + blob[i + 20:])
    # a SUBINT header that carries a checksum (the card replaces a spare one)
    j = blob.index(b"INT_UNIT= ")
    summed = str(tmp_path / "summed.fits")
    open(summed, "wb").write(blob[:j] + b"DATASUM = '0       '".ljust(80) + blob[j + 80:])
    not_fits = str(tmp_path / "text.fits")
    open(not_fits, "wb").write(b"x" * 5760)
    for name, why in ((search, "fold mode"), (summed, "DATASUM"), (not_fits, "FITS")):
        before = open(name, "rb").read()
        with pytest.raises(lib.PSRFITSError, match=why):
            lib.patch_weights(name, 0, 0, 0.0)
        assert open(name, "rb").read() == before
    with pytest.raises(lib.PSRFITSError):
        lib.patch_weights(str(tmp_path / "missing.fits"), 0, 0, 0.0)


# ---------------------------------------------------------------------------
# ppzap.apply_zap_channels / run_paz_cmds
# ---------------------------------------------------------------------------
ZAPS = [[[1, 4], [], [4, 6]],  # archive 0: per subint
        [[], [], []],          # archive 1: nothing flagged
        [[0], [0], [7]]]       # archive 2


def three_archives(lib, d):
    os.makedirs(str(d))
    names = []
    for i in range(3):
        names.append(write_file(lib, d / ("arch%d.fits" % i), seed=i)[0])
    return names


def tree(d):
    return {n: open(os.path.join(str(d), n), "rb").read() for n in sorted(os.listdir(str(d)))}


def expected_weights(w, zaps, all_subs):
    w = w.copy()
    for isub, chans in enumerate(zaps):
        for c in chans:
            if all_subs:
                w[:, c] = 0.0
            else:
                w[isub, c] = 0.0
    return w


@pytest.mark.parametrize("modify", [False, True])
@pytest.mark.parametrize("all_subs", [False, True])
def test_apply_equals_running_the_printed_commands(lib, tmp_path, all_subs, modify):
    from pulseportraiture_amd import ppzap
    a = three_archives(lib, tmp_path / "a")
    b = three_archives(lib, tmp_path / "b")
    originals = tree(tmp_path / "a")
    assert originals == tree(tmp_path / "b")
    w0 = [read_weights(lib, n) for n in a]

    written = ppzap.apply_zap_channels(a, ZAPS, all_subs=all_subs, modify=modify, quiet=True)
    cmds = str(tmp_path / "cmds.txt")
    lines = ppzap.print_paz_cmds(b, ZAPS, all_subs=all_subs, modify=modify, outfile=cmds,
                                 quiet=True)
    assert lines
    ran = ppzap.run_paz_cmds(cmds)
    got_a, got_b = tree(tmp_path / "a"), tree(tmp_path / "b")
    assert got_a == got_b
    assert [os.path.basename(n) for n in written] == [os.path.basename(n) for n in ran]

    if modify:
        assert sorted(got_a) == ["arch0.fits", "arch1.fits", "arch2.fits"]
        assert [os.path.basename(n) for n in written] == ["arch0.fits", "arch2.fits"]
        out = {0: a[0], 2: a[2]}
    else:
        # the archive with nothing flagged is not copied; the inputs are untouched
        assert sorted(got_a) == ["arch0.fits", "arch0.zap", "arch1.fits", "arch2.fits", "arch2.zap"]
        for n in ("arch0.fits", "arch1.fits", "arch2.fits"):
            assert got_a[n] == originals[n]
        assert [os.path.basename(n) for n in written] == ["arch0.zap", "arch2.zap"]
        out = {0: a[0][:-4] + "zap", 2: a[2][:-4] + "zap"}
    assert got_a["arch1.fits"] == originals["arch1.fits"]
    for i, name in out.items():
        np.testing.assert_array_equal(read_weights(lib, name),
                                      expected_weights(w0[i], ZAPS[i], all_subs))
        # nothing but DAT_WTS bytes differs from the input
        cells = wts_cells(originals["arch%d.fits" % i])
        allowed = set()
        for a0, n in cells.values():
            allowed.update(range(a0, a0 + n))
        assert changed_bytes(originals["arch%d.fits" % i], open(name, "rb").read()) <= allowed
    # the lines themselves, as a list
    c = three_archives(lib, tmp_path / "c")
    lines_c = ppzap._paz_lines(c, ZAPS, all_subs, modify)
    ppzap.run_paz_cmds(lines_c)
    assert tree(tmp_path / "c") == got_a


def test_extension_rule(lib, tmp_path, monkeypatch):
    """print_paz_cmds' rule, kept as it is: the text after the last "." of
    the name as given (directories included) is replaced by "zap", and a name
    with no "." at all gets ".zap" appended.  Names relative to the working
    directory, so that no directory of the temporary path takes part."""
    from pulseportraiture_amd import ppzap
    assert "." not in "noext" and ppzap._zap_name("noext") == "noext.zap"
    assert ppzap._zap_name("a.b/noext") == "a.zap"  # the reference's rule, dots in directories too
    assert ppzap._zap_name("dir/x.y.fits") == "dir/x.y.zap"
    _, w = write_file(lib, tmp_path / "noext")
    monkeypatch.chdir(tmp_path)
    lines = ppzap._paz_lines(["noext"], [[[2], [], []]], False, False)
    assert lines == ["paz -e zap noext", "paz -m -I -z 2 -w 0 noext.zap"]
    out = ppzap.apply_zap_channels(["noext"], [[[2], [], []]], quiet=True)
    assert out == ["noext.zap"]
    want = w.copy()
    want[0, 2] = 0.0
    np.testing.assert_array_equal(read_weights(lib, "noext.zap"), want)
    assert ppzap.apply_zap_channels([], [], quiet=True) == []


def test_names_with_whitespace_and_trailing_dot(lib, tmp_path, monkeypatch):
    """apply_zap_channels never goes through text: a name with a blank in it
    works (a command file cannot carry one unquoted: run_paz_cmds refuses the
    line).  A name ending in "." has no extension to replace -- the rule would
    call the copy "zap" -- and is refused before anything is written."""
    from pulseportraiture_amd import ppzap
    monkeypatch.chdir(tmp_path)
    _, w = write_file(lib, tmp_path / "my archive.fits")
    out = ppzap.apply_zap_channels(["my archive.fits"], [[[], [3], []]], all_subs=True, quiet=True)
    assert out == ["my archive.zap"]
    want = w.copy()
    want[:, 3] = 0.0
    np.testing.assert_array_equal(read_weights(lib, "my archive.zap"), want)
    with pytest.raises(ValueError):
        ppzap.run_paz_cmds(ppzap._paz_lines(["my archive.fits"], [[[], [3], []]], True, False))
    write_file(lib, tmp_path / "ok.fits")
    write_file(lib, tmp_path / "dot.")
    before = tree(tmp_path)
    with pytest.raises(ValueError, match="ends in"):
        ppzap.apply_zap_channels(["ok.fits", "dot."], [[[1], [], []], [[1], [], []]], quiet=True)
    with pytest.raises(ValueError, match="ends in"):
        ppzap.run_paz_cmds(["paz -e zap ok.fits", "paz -e zap dot."])
    assert tree(tmp_path) == before


@pytest.mark.parametrize("bad", ["paz -r -m arch0.fits", "paz -m -z x arch0.fits",
                                 "psrzap arch0.fits", "paz -m -I -z 1 arch0.fits",
                                 "paz -e zzz arch0.fits"])
def test_unknown_command_raises_before_anything_is_written(lib, tmp_path, bad):
    from pulseportraiture_amd import ppzap
    names = three_archives(lib, tmp_path / "a")
    before = tree(tmp_path / "a")
    lines = ["paz -e zap %s" % names[0], "paz -m -z 3 %s" % names[1], bad.replace("arch0.fits", names[0])]
    with pytest.raises(ValueError) as e:
        ppzap.run_paz_cmds(lines)
    assert lines[2] in str(e.value)
    assert tree(tmp_path / "a") == before
    # a bad index is refused by the patch itself, and that file stays as it was
    with pytest.raises(lib.PSRFITSError):
        ppzap.run_paz_cmds(["paz -m -z %d %s" % (NCHAN, names[1])])
    assert tree(tmp_path / "a") == before


def test_standalone_program_under_sanitizers(lib, fits, tmp_path):
    """tools/patch_weights_check.cpp with the reader and the writer, all
    compiled with -fsanitize=address,undefined (the runtimes linked into the
    program itself); any report fails the run."""
    path, _ = fits
    cxx = os.environ.get("CXX", "g++")
    csrc = os.path.join(ROOT, "pulseportraiture_amd", "csrc")
    exe = str(tmp_path / "patch_weights_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",
                           '-DPPF_SRC_HASH="check"', "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "patch_weights_check.cpp"),
                           os.path.join(csrc, "psrfits.cpp"),
                           os.path.join(csrc, "psrfits_write.cpp"), "-o", exe])
    work = str(tmp_path / "copy.fits")
    shutil.copyfile(path, work)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe, work], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "ok" and "ERROR" not in out.stderr
    assert open(work, "rb").read() == open(path, "rb").read()
