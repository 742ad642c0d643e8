"""The Python binding (diffsplitting_amd/_lib.py) without a GPU: every entry of SIGNATURES against its prototype in
include/dsx.h, what the call path refuses and what it passes through (against a recording stand-in for the C function),
and a search of the package for hand-built pointers."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest
import torch

from diffsplitting_amd import _lib
from diffsplitting_amd._lib import Dev, DsxError, Handle, Host, Stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HANDLES = {"dsx_model", "dsx_exec", "dsx_tileplan", "dsx_lpips", "dsx_resize_plan", "dsx_tiff"}
# C scalar -> (bytes, class): signed, unsigned, floating
SCALARS = {"int": (4, "i"), "int64_t": (8, "i"), "unsigned": (4, "u"), "uint32_t": (4, "u"), "uint64_t": (8, "u"),
           "size_t": (8, "u"), "float": (4, "f"), "double": (8, "f"), "int32_t": (4, "i"), "uint8_t": (1, "u"),
           "uint16_t": (2, "u"), "unsigned long long": (8, "u")}


def _prototypes():
    """name -> (return type, [parameter text]) of every function include/dsx.h declares; comments stripped."""
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "dsx.h")).read(), flags=re.S)
    hdr = "\n".join(ln for ln in hdr.splitlines() if not ln.lstrip().startswith("#"))     # macros are not prototypes
    protos = {}
    for m in re.finditer(r"^([A-Za-z_][\w \*]*?)\s*\b(dsx_\w+)\s*\(([^()]*)\)\s*;", hdr, flags=re.M):
        params = [" ".join(p.split()) for p in m.group(3).split(",")]
        protos[m.group(2)] = (" ".join(m.group(1).split()), [] if params == ["void"] else params)
    # nothing that looks like a call or a declaration of a dsx_ function may escape the prototype pattern
    assert set(re.findall(r"\b(dsx_[a-z0-9_]+)\s*\(", hdr)) == set(protos)
    return protos


def _split(param):
    """'const float* x_dev' -> (base type, pointer depth, name, sized array?); `T x[4]` is a pointer to T"""
    m = re.fullmatch(r"(?:const )?([\w ]+?)\s*((?:\*\s*(?:const\s*)?)*)(\w+)(\[\d+\])?", param)
    assert m, param
    sized = m.group(4) is not None
    return m.group(1), m.group(2).count("*") + sized, m.group(3), sized


def _scalar_class(ctype):
    return C.sizeof(ctype), {"f": "f", "d": "f"}.get(ctype._type_, "i" if ctype._type_.islower() else "u")


def _is_ctypes_pointer(t):
    return isinstance(t, type) and issubclass(t, C._Pointer)


def test_every_entry_agrees_with_its_prototype():
    protos = _prototypes()
    assert len(protos) >= 91 and set(protos) == set(_lib.SIGNATURES)
    for name, (ret, params) in protos.items():
        res, kinds = _lib.SIGNATURES[name]
        where = f"{name} returns {ret}"
        if ret == "void":
            assert res is None, where
        elif ret == "const char*":
            assert res is C.c_char_p, where
        else:
            assert _scalar_class(res) == SCALARS[ret], where
        assert len(kinds) == len(params), f"{name}: {len(params)} parameters declared, {len(kinds)} in the table"
        for i, (param, kind) in enumerate(zip(params, kinds)):
            base, depth, pname, sized = _split(param)
            where = f"{name} parameter {i} ({param}) is {kind!r}"
            if depth == 0:
                assert not isinstance(kind, _lib._Kind) and not _is_ctypes_pointer(kind) and kind is not C.c_char_p, where
                assert _scalar_class(kind) == SCALARS[base], where
                continue
            assert isinstance(kind, _lib._Kind) or _is_ctypes_pointer(kind) or kind is C.c_char_p, where
            if pname == "stream":
                assert kind == Stream and base == "void" and depth == 1, where
            elif base in HANDLES:
                assert kind == Handle if depth == 1 else kind is C.POINTER(C.c_void_p), where
            elif pname.endswith("_dev"):
                assert kind == Dev(base) and depth == 1, where
            elif pname.endswith("_host") or pname.startswith("host_") or sized:
                assert kind == Host or _is_ctypes_pointer(kind), where
            else:                                           # no suffix: the table is the statement, but never device
                assert not (isinstance(kind, _lib._Kind) and kind.name == "Dev"), where
            assert kind != Stream or pname == "stream", where
            assert kind != Handle or base in HANDLES, where
            # the element type, wherever the table states one
            if isinstance(kind, _lib._Kind) and kind.name == "Dev":
                assert kind.elem == base and base in _lib.DEV_DTYPES, where
            elif kind is C.c_char_p:
                assert base == "char" and depth == 1, where
            elif _is_ctypes_pointer(kind) and depth == 1 and not base.startswith("dsx_"):
                assert _scalar_class(kind._type_) == SCALARS[base], where
            elif _is_ctypes_pointer(kind) and depth == 1:
                assert issubclass(kind._type_, C.Structure), where
            elif _is_ctypes_pointer(kind):
                assert kind is C.POINTER(C.c_void_p) and depth == 2, where
    # the C functions carry plain ctypes types
    assert _lib._cdll.dsx_randn.argtypes == [C.c_void_p, C.c_int64, C.c_uint64, C.c_uint64, C.c_void_p]


def test_kinds_compare_by_meaning():
    assert Dev("float") == Dev("float") and Dev("float") != Dev("double") and Host != Handle and Dev("void") != Host
    assert len({Dev("float"), Dev("float"), Stream}) == 2
    assert torch.float32 in _lib.DEV_DTYPES["float"] and torch.float64 in _lib.DEV_DTYPES["double"]
    assert torch.int16 in _lib.DEV_DTYPES["uint16_t"] and torch.int64 in _lib.DEV_DTYPES["uint64_t"]
    assert set(_lib.DEV_DTYPES["uint8_t"]) == {torch.uint8, torch.int8} and _lib.DEV_DTYPES["void"] is None
    assert torch.float32 not in _lib.DEV_DTYPES["uint64_t"] and torch.int32 not in _lib.DEV_DTYPES["uint16_t"]


class Recorder:
    """Stands in for a C function: keeps the arguments of every call and returns ``value``."""

    def __init__(self, value=0):
        self.calls, self.value = [], value

    def __call__(self, *args):
        self.calls.append(args)
        return self.value


KINDS = [Handle, Dev("float"), C.c_int, Host, Dev("void"), Stream]


def test_tensors_that_must_not_reach_a_kernel_are_refused_before_the_call():
    rec = Recorder()
    f = _lib.bind("dsx_fake", rec, KINDS)
    good = torch.zeros(8)
    for bad, word in ((good, "cpu"),                                        # not on the device
                      (torch.zeros(4, 4).t(), "strided"),                   # not contiguous
                      (torch.zeros(8, dtype=torch.float64), "float64")):    # not the element type
        with pytest.raises(DsxError, match=rf"dsx_fake: argument 1 .*{word}"):
            f(None, bad, 3, None, None, None)
    with pytest.raises(DsxError, match="dsx_fake: argument 4"):             # void takes any element type, on the device
        f(None, None, 3, None, torch.zeros(8, dtype=torch.int16), None)
    # host slots: memory as it lies, on the host (a CUDA tensor: tests/test_gpu_binding.py)
    with pytest.raises(DsxError, match="dsx_fake: argument 3 takes host memory"):
        f(None, None, 3, torch.zeros(8, device="meta"), None, None)
    for strided in (np.zeros((4, 4))[:, 1], torch.zeros(4, 4)[:, 1]):
        with pytest.raises(DsxError, match="dsx_fake: argument 3 takes host memory"):
            f(None, None, 3, strided, None, None)
    with pytest.raises(TypeError, match="dsx_fake takes 6 arguments, got 5"):
        f(None, None, 3, None, None)
    assert rec.calls == []


def test_the_device_rule():
    d0, d1 = torch.device("cuda", 0), torch.device("cuda", 1)
    assert _lib.common_device("dsx_fake", []) is None
    assert _lib.common_device("dsx_fake", [d1]) == d1 and _lib.common_device("dsx_fake", [d0, d0, d0]) == d0
    for devices in ([d0, d1], [d1, d1, d0]):
        with pytest.raises(DsxError, match=r"dsx_fake: tensors on cuda:\d and on cuda:\d"):
            _lib.common_device("dsx_fake", devices)


@pytest.mark.parametrize("value", [0, 7, -1, -3, None, 2.5])
def test_addresses_and_the_return_value_pass_through(value):
    rec = Recorder(value)
    f = _lib.bind("dsx_fake", rec, KINDS)
    h, p, s = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x3000)
    buf = (C.c_float * 4)()
    assert f(h, p, 3, buf, 0x4000, s) is value
    assert f(None, None, 3, None, None, None) is value                     # no tensor: None stays the NULL stream
    assert f(0x10, 0x20, C.c_int(3), 0x30, p, 0x40) is value
    assert len(rec.calls) == 3
    for got, want in zip(rec.calls[0], (h, p, 3, buf, 0x4000, s)):
        assert got is want
    assert rec.calls[1] == (None, None, 3, None, None, None)
    assert rec.calls[2][:2] == (0x10, 0x20) and rec.calls[2][3:] == (0x30, p, 0x40)


def test_host_memory_arrives_as_its_address():
    rec = Recorder()
    f = _lib.bind("dsx_fake", rec, KINDS)
    a, t = np.arange(6, dtype=np.float32).reshape(2, 3), torch.arange(6.0)
    f(None, None, 0, a, None, None)
    f(None, None, 0, t, None, None)
    assert rec.calls[0][3] == a.ctypes.data and rec.calls[1][3] == t.data_ptr()
    ptrs = _lib.host_pointers([t, t[2:]])
    assert list(ptrs) == [t.data_ptr(), t.data_ptr() + 8]
    with pytest.raises(DsxError, match="host memory"):
        _lib.host_pointers([t[::2]])


def test_an_entry_with_nothing_to_convert_is_the_function_itself():
    rec = Recorder()
    assert _lib.bind("dsx_fake", rec, [Handle, C.c_int, C.POINTER(C.c_int64)]) is rec
    assert _lib.lib.dsx_abi_version() == 2 and _lib.lib.dsx_loss_blocks(1, 8, 8) >= 1


def test_the_real_library_keeps_its_status_and_message():
    """A negative status comes back as it is (``check`` stays with the caller), through the bound call."""
    rc = _lib.lib.dsx_randn_samples(None, 0, 0, 0, None, 0, None)
    assert rc < 0 and _lib.lib.dsx_last_error()
    with pytest.raises(DsxError, match=f"libdsx status {rc}"):
        _lib.check(rc)


def test_no_wrapper_builds_a_pointer_or_a_stream_by_hand():
    pkg = os.path.join(ROOT, "diffsplitting_amd")
    found = []
    for path in sorted(glob.glob(os.path.join(pkg, "**", "*.py"), recursive=True)):
        rel = os.path.relpath(path, pkg)
        if rel == "_lib.py":
            continue
        for n, line in enumerate(open(path), 1):
            if ".data_ptr()" in line or ".cuda_stream" in line:
                found.append((rel, n, line.strip()))
    # the one exception: UNet's parameter fingerprint, which is no call argument
    assert [f[0] for f in found] == [os.path.join("model", "engine_unet.py")], found
    assert "t._version" in found[0][2]
