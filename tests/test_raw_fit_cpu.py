"""The raw-sample fit's interface without a device: the header's declaration
of ppf_fit_portrait_batch_raw and ppf_raw_subints against the ctypes
binding, and engine.RawSubints on CPU tensors (construction checks, shape,
views, gathers)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.conftest import ROOT


def _header():
    return open(os.path.join(ROOT, "include", "ppfit.h")).read()


def test_header_declares_raw_fit():
    txt = _header()
    assert re.search(r"^int\s+ppf_fit_portrait_batch_raw\s*\(\s*ppf_ctx\*\s*\w+,\s*const ppf_fit_desc\*"
                     r"\s*\w+,\s*const ppf_raw_subints\*\s*\w+,\s*const ppf_fit_result\*\s*\w+\)",
                     txt, re.M | re.S)
    assert re.search(r"\}\s*ppf_raw_subints\s*;", txt)
    assert re.search(r"#define PPF_VERSION 1\b", txt)


def test_ctypes_struct_matches_header():
    """Field names, order and C types of ppf_raw_subints, parsed from the
    header, against _lib.RawSubintsDesc; the entry point's binding."""
    from pulseportraiture_amd import _lib
    body = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\}\s*ppf_raw_subints\s*;",
                     _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            m = re.match(r"(.*?)(\w+)$", decl, re.S)
            fields.append((m.group(2), " ".join(m.group(1).split())))
    assert [n for n, _ in fields] == ["raw_type", "npol", "pmode", "ipol", "raw", "scl", "offs"]
    assert [n for n, _ in _lib.RawSubintsDesc._fields_] == [n for n, _ in fields]
    for (name, ctype), (_, pyt) in zip(fields, _lib.RawSubintsDesc._fields_):
        assert pyt is (ctypes.c_int32 if ctype == "int32_t" else ctypes.c_void_p), name
        assert ctype == "int32_t" or ctype.endswith("*"), name
    # the layout a C compiler gives it: four int32, then three pointers
    assert _lib.RawSubintsDesc.raw.offset == 16
    assert ctypes.sizeof(_lib.RawSubintsDesc) == 16 + 3 * ctypes.sizeof(ctypes.c_void_p)
    args, res = _lib.EXPORTS["ppf_fit_portrait_batch_raw"]
    assert res is ctypes.c_int and len(args) == 4
    assert args[2]._type_ is _lib.RawSubintsDesc and args[1]._type_ is _lib.FitDesc
    # ppf_fit_desc is not grown by the feature: still ends with the cache rows
    assert _lib.FitDesc._fields_[-1][0] == "spec_R" and len(_lib.FitDesc._fields_) == 32
    hdr = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\}\s*ppf_fit_desc\s*;",
                    _header(), re.S).group(1)
    assert "raw" not in re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def _parts(nsub=5, npol=2, nchan=3, nbin=64, dtype=torch.int16):
    g = torch.Generator().manual_seed(3)
    raw = torch.randint(-100, 100, (nsub, npol, nchan, nbin), generator=g).to(dtype)
    scl = torch.rand((nsub, npol, nchan), generator=g, dtype=torch.float64) + 0.5
    offs = torch.randn((nsub, npol, nchan), generator=g, dtype=torch.float64)
    return raw, scl, offs


def test_raw_subints_shape_and_views():
    from pulseportraiture_amd.engine import RawSubints
    raw, scl, offs = _parts()
    rs = RawSubints(raw, scl, offs, pmode=1)
    assert rs.shape == (5, 3, 64) and len(rs) == 5
    assert rs.device.type == "cpu" and not rs.is_pinned()
    assert rs.nbytes == raw.numel() * 2 + 2 * scl.numel() * 8
    v = rs[1:4]
    assert v.shape == (3, 3, 64) and (v.pmode, v.ipol) == (1, 0)
    assert v.raw.data_ptr() == raw[1:4].data_ptr()  # views, not copies
    assert v.scl.data_ptr() == scl[1:4].data_ptr() and v.offs.data_ptr() == offs[1:4].data_ptr()
    raw[2, 0, 0, 0] = 77
    assert int(v.raw[1, 0, 0, 0]) == 77
    assert rs.to("cpu") is rs
    # numpy arrays are taken as they are (shared memory)
    rn = RawSubints(raw.numpy(), scl.numpy(), offs.numpy(), pmode=0, ipol=1)
    assert rn.raw.data_ptr() == raw.data_ptr() and rn.ipol == 1
    for dt in (torch.uint8, torch.float32):
        assert RawSubints(raw.to(dt), scl, offs).raw.dtype == dt


@pytest.mark.parametrize("idx", [[3, 0, 3], np.array([4, 1]), torch.tensor([2])])
def test_raw_subints_gather(idx):
    from pulseportraiture_amd.engine import RawSubints
    raw, scl, offs = _parts()
    g = RawSubints(raw, scl, offs, pmode=2)[idx]
    ix = [int(i) for i in idx]
    assert g.shape == (len(ix), 3, 64) and g.pmode == 2
    assert torch.equal(g.raw, raw[ix]) and torch.equal(g.scl, scl[ix])
    assert torch.equal(g.offs, offs[ix])
    assert g.raw.data_ptr() != raw.data_ptr()  # a gather copies


def test_raw_subints_refusals():
    from pulseportraiture_amd.engine import RawSubints
    raw, scl, offs = _parts()
    with pytest.raises(ValueError):
        RawSubints(raw[0], scl[0], offs[0])  # not [nsub, npol, nchan, nbin]
    with pytest.raises(ValueError):
        RawSubints(raw, scl[:, :1], offs)
    with pytest.raises(ValueError):
        RawSubints(raw, scl, offs[:4])
    with pytest.raises(TypeError):
        RawSubints(raw.to(torch.int32), scl, offs)
    with pytest.raises(TypeError):
        RawSubints(raw.to(torch.float64), scl, offs)
    with pytest.raises(TypeError):
        RawSubints(raw, scl.to(torch.float32), offs)
    with pytest.raises(TypeError):
        RawSubints(raw.tolist(), scl, offs)
    for pmode in (-1, 3):
        with pytest.raises(ValueError):
            RawSubints(raw, scl, offs, pmode=pmode)
    for ipol in (-1, 2):
        with pytest.raises(ValueError):
            RawSubints(raw, scl, offs, ipol=ipol)
    with pytest.raises(ValueError):
        RawSubints(raw[:, :1], scl[:, :1], offs[:, :1], pmode=1)  # AA + BB of one polarisation
    rs = RawSubints(raw, scl, offs)
    with pytest.raises(IndexError):
        rs[::2]
    with pytest.raises(IndexError):
        rs[[[0, 1]]]


def test_get_toas_raw_samples_default_off():
    from pulseportraiture_amd import pptoas
    assert pptoas.GetTOAs.raw_samples is False
    assert pptoas.GetTOAs.raw_snr_bytes == 1 << 30
