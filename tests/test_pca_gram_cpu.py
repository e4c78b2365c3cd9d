"""Host-side wiring of the Gram-path PCA (ppfit_gram.hip): the header, the
ctypes table, the translation unit and the build's dependency list name it,
and the built library exports it."""
import ctypes
import os
import re

from pulseportraiture_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gram_entry_is_declared_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "ppfit.h")).read()
    for name in ("ppf_pca_gram_portraits", "ppf_get_pca_gram_times"):
        assert re.search(r"\bint %s\(ppf_ctx\* ctx" % name, hdr), name
        assert name in _lib.EXPORTS
    # the same argument list as the sister entry
    assert _lib.EXPORTS["ppf_pca_gram_portraits"] == _lib.EXPORTS["ppf_pca_portraits"]
    assert "ppfit_gram.hip" in build.DEPS
    unit = open(os.path.join(build.CSRC, "ppfit_lib.hip")).read()
    assert unit.index('"ppfit_pca.hip"') < unit.index('"ppfit_gram.hip"') < unit.index('"ppfit_capi.hip"')
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, "ppf_pca_gram_portraits") and hasattr(lib, "ppf_get_pca_gram_times")
