"""ppalign's driver without a device: main's option table (the reference's
letters, destinations and defaults, ppalign.py:247-312), run's choice of the
starting template with the device functions replaced by recorders, the
aliases, and the binding of ppf_rotate_fscrunch."""
import os
import re

import numpy as np
import pytest

from tests.conftest import ROOT

# (option strings, dest, default, takes a value) as the reference's OptionParser has them
REFERENCE_OPTIONS = [
    (("-M", "--metafile"), "metafile", None, True),
    (("-I", "--init"), "initial_guess", None, True),
    (("-g", "--width"), "fwhm", None, True),
    (("-D", "--no_DM"), "fit_dm", True, False),
    (("-T", "--tscr"), "tscrunch", False, False),
    (("-p", "--poln"), "pscrunch", True, False),
    (("-C", "--cutoff"), "SNR_cutoff", 0.0, True),
    (("-o", "--outfile"), "outfile", None, True),
    (("-P", "--palign"), "palign", False, False),
    (("-N", "--norm"), "norm", None, True),
    (("-s", "--smooth"), "smooth", False, False),
    (("-r", "--rot"), "rot_phase", 0.0, True),
    (("--place",), "place", None, True),
    (("--niter",), "niter", 1, True),
    (("--verbose",), "quiet", True, False),
]


def test_option_table():
    from pulseportraiture_amd import ppalign
    parser = ppalign._parser()
    acts = {a.dest: a for a in parser._actions if a.dest != "help"}
    assert sorted(acts) == sorted(o[1] for o in REFERENCE_OPTIONS)
    for strings, dest, default, valued in REFERENCE_OPTIONS:
        a = acts[dest]
        assert tuple(a.option_strings) == strings, dest
        assert a.default == default and type(a.default) is type(default), dest
        assert (a.nargs != 0) == valued, dest
        if not valued:  # a flag stores the opposite of its default
            assert a.const is (not default), dest
    o = parser.parse_args(["-M", "m", "-D", "-T", "-p", "-P", "-s", "--verbose"])
    assert (o.fit_dm, o.tscrunch, o.pscrunch, o.palign, o.smooth, o.quiet) == \
        (False, True, False, True, True, False)


class Recorder:
    def __init__(self, monkeypatch, nchan_of=None, nbin=64):
        from pulseportraiture_amd import ppalign, pplib
        self.calls = []
        self.nchan_of = nchan_of or {}
        self.nbin = nbin
        monkeypatch.setattr(ppalign, "add_archives", self.rec("add"))
        monkeypatch.setattr(pplib, "make_constant_portrait", self.rec("const"))
        monkeypatch.setattr(ppalign, "align_archives", self.rec("align", ret="PORT"))
        monkeypatch.setattr(ppalign, "smooth_archive", self.rec("smooth"))
        monkeypatch.setattr(ppalign._arch, "open_archive", self.open_archive)

    def rec(self, name, ret=None):
        def f(*a, **kw):
            if name in ("add", "const"):  # the guess must be writable here
                out = a[1]
                assert os.path.exists(out) and os.path.getsize(out) == 0
                open(out, "w").write(name)
            self.calls.append((name, a, kw))
            return ret
        return f

    def open_archive(self, name, **kw):
        from pulseportraiture_amd.pplib import DataBunch
        return DataBunch(meta=DataBunch(nchan=self.nchan_of.get(name, 4), nbin=self.nbin))


@pytest.fixture()
def meta(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    m = tmp_path / "files.meta"
    m.write_text("first.fits\nsecond.fits\n")
    return str(m)


def tmp_files(path):
    return [f for f in os.listdir(path) if f.startswith("ppalign.")]


def test_run_adds_archives_without_a_guess(meta, tmp_path, monkeypatch):
    from pulseportraiture_amd import ppalign
    r = Recorder(monkeypatch)
    assert ppalign.run(meta, palign=True, pscrunch=False, fit_dm=False, niter=3) == "PORT"
    (n0, a0, k0), (n1, a1, k1) = r.calls
    assert n0 == "add" and a0[0] == meta and k0["palign"] is True and k0["pscrunch"] is False
    tmp = a0[1]
    assert os.path.basename(tmp).startswith("ppalign.") and tmp.endswith(".tmp.fits")
    assert os.path.realpath(os.path.dirname(tmp)) == os.path.realpath(str(tmp_path))
    assert n1 == "align" and a1 == (meta,) and k1["initial_guess"] == tmp
    assert k1 == dict(initial_guess=tmp, fit_dm=False, tscrunch=False, pscrunch=False,
                      SNR_cutoff=0.0, outfile=None, norm=None, rot_phase=0.0, place=None, niter=3,
                      quiet=True)
    assert tmp_files(tmp_path) == []


def test_run_constant_gaussian(meta, tmp_path, monkeypatch):
    from pulseportraiture_amd import ppalign
    from pulseportraiture_amd.pplib import gaussian_profile
    r = Recorder(monkeypatch, nbin=128)
    ppalign.run(meta, initial_guess="given.fits", fwhm="0.05", smooth=True)  # -g overrides -I
    (n0, a0, k0), (n1, a1, k1), (n2, a2, k2) = r.calls
    assert n0 == "const" and a0[0] == "first.fits"
    np.testing.assert_array_equal(k0["profile"], gaussian_profile(128, 0.5, 0.05))
    assert (k0["DM"], k0["dmc"], k0["weights"]) == (0.0, False, None)
    assert n1 == "align" and k1["initial_guess"] == a0[1]
    assert n2 == "smooth" and a2 == (meta + ".algnd.fits",)
    assert tmp_files(tmp_path) == []


def test_run_given_guess(meta, tmp_path, monkeypatch):
    from pulseportraiture_amd import ppalign
    r = Recorder(monkeypatch, nchan_of={"one.fits": 1})
    ppalign.run(meta, initial_guess="many.fits", outfile="o.fits", smooth=True)
    assert [c[0] for c in r.calls] == ["align", "smooth"]
    assert r.calls[0][2]["initial_guess"] == "many.fits" and r.calls[1][1] == ("o.fits",)
    del r.calls[:]
    ppalign.run(meta, initial_guess="one.fits")
    (n0, a0, k0), (n1, a1, k1) = r.calls
    assert n0 == "const" and a0[0] == "first.fits" and k0["profile"] is None
    assert n1 == "align" and k1["initial_guess"] == a0[1] != "one.fits"
    assert tmp_files(tmp_path) == []


def test_run_removes_the_guess_on_error(meta, tmp_path, monkeypatch):
    from pulseportraiture_amd import ppalign
    Recorder(monkeypatch)

    def boom(*a, **kw):
        assert os.path.exists(kw["initial_guess"])
        raise RuntimeError("boom")
    monkeypatch.setattr(ppalign, "align_archives", boom)
    with pytest.raises(RuntimeError, match="boom"):
        ppalign.run(meta)
    assert tmp_files(tmp_path) == []


def test_main_calls_run(meta, monkeypatch, capsys):
    from pulseportraiture_amd import ppalign
    seen = []
    monkeypatch.setattr(ppalign, "run", lambda *a, **kw: seen.append((a, kw)))
    assert ppalign.main(["-M", meta, "-g", "0.1", "-C", "5", "-r", "0.25", "--place", "0.3",
                         "--niter", "2", "-N", "prof", "-o", "out.fits"]) == 0
    (a, kw), = seen
    assert a == (meta,)
    assert kw == dict(initial_guess=None, fwhm="0.1", fit_dm=True, tscrunch=False, pscrunch=True,
                      SNR_cutoff=5.0, outfile="out.fits", palign=False, norm="prof", smooth=False,
                      rot_phase=0.0, place=0.3, niter=2, quiet=True)  # --place overrides --rot
    ppalign.main(["-M", meta, "-r", "0.25"])
    assert seen[1][1]["rot_phase"] == 0.25 and seen[1][1]["place"] is None
    # no metafile, or no iterations: the help, nothing run
    assert ppalign.main([]) == 0 and ppalign.main(["-M", meta, "--niter", "0"]) == 0
    assert len(seen) == 2 and "--palign" in capsys.readouterr().out


def test_module_entry_point():
    src = open(os.path.join(ROOT, "pulseportraiture_amd", "ppalign.py")).read()
    assert re.search(r'if __name__ == "__main__":\n\s+import sys\n\s+sys.exit\(main\(\)\)', src)


def test_aliases_and_signatures():
    import inspect
    from pulseportraiture_amd import ppalign, pplib
    assert ppalign.psradd_archives is ppalign.add_archives
    assert ppalign.psrsmooth_archive is ppalign.smooth_archive

    def sig(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(ppalign.add_archives) == [("metafile", E), ("outfile", E), ("palign", False),
                                         ("tscrunch", True), ("pscrunch", True), ("quiet", False)]
    assert sig(ppalign.smooth_archive) == [("archive", E), ("outfile", None), ("smart", True),
                                           ("quiet", False), ("kwargs", E)]
    assert sig(pplib.make_constant_portrait) == [
        ("archive", E), ("outfile", E), ("profile", None), ("DM", 0.0), ("dmc", False),
        ("weights", None), ("quiet", False)]
    assert sig(ppalign.run) == [
        ("metafile", E), ("initial_guess", None), ("fwhm", None), ("fit_dm", True),
        ("tscrunch", False), ("pscrunch", True), ("SNR_cutoff", 0.0), ("outfile", None),
        ("palign", False), ("norm", None), ("smooth", False), ("rot_phase", 0.0), ("place", None),
        ("niter", 1), ("quiet", True)]
    for f in (ppalign.add_archives, ppalign.smooth_archive):
        assert "not pinned" in " ".join(f.__doc__.split()).lower()


def test_binding():
    from pulseportraiture_amd import _lib, build, engine
    txt = open(os.path.join(ROOT, "include", "ppfit.h")).read()
    assert re.search(r"^int ppf_rotate_fscrunch\(ppf_ctx\* ctx, int32_t nunit, int32_t nchan,\s+"
                     r"int32_t nbin,\s+const double\* data, const double\* phase,\s+"
                     r"const double\* weight,\s+double\* prof\);", txt, re.M)
    assert "ppf_rotate_fscrunch" in _lib.EXPORTS and len(_lib.EXPORTS["ppf_rotate_fscrunch"][0]) == 8
    kid = int(re.search(r"#define PPF_K_FSCRUNCH (\d+)", txt).group(1))
    assert _lib.KERNEL_IDS["fscrunch"] == kid
    assert int(re.search(r"#define PPF_NUM_KERNELS (\d+)", txt).group(1)) == \
        len(_lib.KERNEL_IDS) == kid + 1
    assert "ppfit_fscrunch.hip" in build.DEPS
    assert hasattr(engine.Engine.rotate_fscrunch, "__wrapped__")  # runs on the engine's stream
    assert re.search(r"#define PPF_VERSION 1\b", txt)
