"""The C ABI: libdynamo_hip.so builds for gfx950 on a GPU-less host, loads, and exports every symbol that
include/dynamo_hip.h declares; the ctypes mirror agrees with the header.  No compute calls (no GPU here)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def so():
    from hipops import lib
    lib.build()
    return ctypes.CDLL(lib.LIB_PATH)


def header_text():
    """include/dynamo_hip.h with its comments stripped."""
    txt = open(os.path.join(ROOT, "include", "dynamo_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def header_symbols():
    return sorted(set(re.findall(r"\b(dd_[a-z0-9_]+)\s*\(", header_text())))


C_KINDS = {("long", "long"): "long long", ("size_t",): "size_t", ("double",): "double", ("float",): "float", ("int",): "int", ("int32_t",): "int"}


def c_kind(decl, named):
    """Kind of a return type (named=False) or of one parameter, whose name (when it has one) is dropped."""
    if "*" in decl:
        return "pointer"
    words = tuple(w for w in decl.split() if w != "const")
    if named and words not in C_KINDS:
        words = words[:-1]
    assert words in C_KINDS, "cannot classify %r" % decl
    return C_KINDS[words]


def header_prototypes():
    """{name: (return kind, [parameter kinds])} of every statement of the header outside its struct definitions; a statement that
    is no dd_* prototype, or a type this does not know, fails the test."""
    txt = re.sub(r"^\s*#.*$", "", header_text(), flags=re.M)
    txt = re.sub(r"typedef\s+struct\s+\w+\s*\{.*?\}\s*\w+\s*;", "", txt, flags=re.S)
    txt = txt.replace('extern "C" {', "")
    assert txt.rstrip().endswith("}"), txt[-40:]
    protos = {}
    for stmt in txt.rstrip()[:-1].split(";"):
        stmt = " ".join(stmt.split())
        if not stmt:
            continue
        m = re.fullmatch(r"(.+?)\b(dd_[a-z0-9_]+) ?\((.*)\)", stmt)
        assert m, "not a dd_* prototype: %r" % stmt
        ret, name, params = m.groups()
        assert name not in protos, name
        params = [] if params.strip() == "void" else params.split(",")
        protos[name] = (c_kind(ret, False), [c_kind(q, True) for q in params])
    return protos


def ctypes_kind(t):
    if t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer)):
        return "pointer"
    kinds = {ctypes.c_longlong: "long long", ctypes.c_size_t: "size_t", ctypes.c_double: "double", ctypes.c_float: "float",
             ctypes.c_int: "int", ctypes.c_int32: "int"}
    assert t in kinds, "cannot classify %r" % t
    return kinds[t]


def test_every_declared_symbol_is_exported(so):
    from hipops import abi
    declared = header_symbols()
    assert len(declared) >= 20
    for name in declared:
        assert hasattr(so, name), "libdynamo_hip.so does not export " + name
    assert sorted(abi.EXPORTED) == declared, (sorted(set(declared) ^ set(abi.EXPORTED)))


def test_signature_table_matches_the_prototypes():
    """Every prototype of the header against abi.SIGNATURES: the same set of names, and per entry point the same number of
    arguments and the same kind (pointer, long long, size_t, double, float, int) for each of them and for the return value.
    No exceptions."""
    from hipops import abi
    protos = header_prototypes()
    assert len(protos) >= 20 and sorted(protos) == header_symbols()
    assert set(abi.SIGNATURES) == set(protos), sorted(set(abi.SIGNATURES) ^ set(protos))
    assert abi.EXPORTED == tuple(abi.SIGNATURES)
    for name, (ret, params) in protos.items():
        res, args = abi.SIGNATURES[name]
        assert (ctypes_kind(res), [ctypes_kind(a) for a in args]) == (ret, params), name


def test_constants_match_the_header():
    """Every `#define DD_<NAME> <integer>` against abi.DD_<NAME> (DD_VIS_<KIND>: abi.DD_VIS_KINDS[kind]); one without a mirror fails."""
    from hipops import abi
    txt = header_text()
    names = re.findall(r"^\s*#\s*define\s+(DD_\w+)", txt, flags=re.M)
    defines = dict(re.findall(r"^\s*#\s*define\s+(DD_\w+)[ \t]+(-?\d+)[ \t]*$", txt, flags=re.M))
    assert len(names) >= 20 and sorted(names) == sorted(defines), sorted(set(names) ^ set(defines))
    for name, value in defines.items():
        if hasattr(abi, name):
            mirror = getattr(abi, name)
        else:
            assert name.startswith("DD_VIS_") and name[7:].lower() in abi.DD_VIS_KINDS, "hipops/abi.py has no mirror of " + name
            mirror = abi.DD_VIS_KINDS[name[7:].lower()]
        assert mirror == int(value), (name, mirror, value)
    assert len(abi.DD_VIS_KINDS) == sum(1 for n in defines if n.startswith("DD_VIS_") and not hasattr(abi, n))


def test_declare_reports_a_missing_symbol(so):
    """A library that lacks entry points (a stale build): declare() names each of them and nothing else, and no longer passes over
    them; the whole library declares every name of the table."""
    from hipops import abi
    gone = ("dd_photo_loss_part", "dd_abi_version")

    class Stale:
        def __getattr__(self, name):
            if name in gone:
                raise AttributeError(name)
            return getattr(so, name)
    with pytest.raises(AttributeError) as err:
        abi.declare(Stale())
    assert sorted(re.findall(r"dd_\w+", str(err.value))) == sorted(gone)
    assert abi.declare(so) == abi.EXPORTED
    for name, (res, args) in abi.SIGNATURES.items():
        assert getattr(so, name).restype is res and getattr(so, name).argtypes == args, name


def test_abi_version_and_error_strings(so):
    from hipops import abi
    abi.declare(so)
    assert so.dd_abi_version() == abi.DD_ABI_VERSION
    assert so.dd_error_string(0) == b"success"


def test_struct_layout_matches_header():
    """sizeof/offsetof computed by the C compiler vs the ctypes mirror."""
    import subprocess
    import tempfile
    from hipops import abi
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "dynamo_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(DDPhotoScale), sizeof(DDPhotoArgs), offsetof(DDPhotoArgs, scale),
         offsetof(DDPhotoScale, out_delta), offsetof(DDPhotoArgs, target), sizeof(DDAssembleArgs), offsetof(DDAssembleArgs, term_of));
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(DDRegSmooth), sizeof(DDRegScale), sizeof(DDRegArgs), offsetof(DDRegScale, w_sparsity),
         offsetof(DDRegScale, w_ground), offsetof(DDRegArgs, scale));
  printf("%zu %zu %zu %zu\n", sizeof(DDJpegHeader), offsetof(DDJpegHeader, qt), offsetof(DDJpegHeader, bits), offsetof(DDJpegHeader, vals));
  return 0;
}'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "l.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "l")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    want = [ctypes.sizeof(abi.DDPhotoScale), ctypes.sizeof(abi.DDPhotoArgs), abi.DDPhotoArgs.scale.offset,
            abi.DDPhotoScale.out_delta.offset, abi.DDPhotoArgs.target.offset, ctypes.sizeof(abi.DDAssembleArgs),
            abi.DDAssembleArgs.term_of.offset,
            ctypes.sizeof(abi.DDRegSmooth), ctypes.sizeof(abi.DDRegScale), ctypes.sizeof(abi.DDRegArgs), abi.DDRegScale.w_sparsity.offset,
            abi.DDRegScale.w_ground.offset, abi.DDRegArgs.scale.offset,
            ctypes.sizeof(abi.DDJpegHeader), abi.DDJpegHeader.qt.offset, abi.DDJpegHeader.bits.offset, abi.DDJpegHeader.vals.offset]
    assert got == want, (got, want)


def test_loss_path_refuses_cpu_tensors():
    import torch
    import tools
    from hipops.lib import DynamoHipError
    with pytest.raises(DynamoHipError):
        tools.SSIM()(torch.rand(1, 3, 8, 8), torch.rand(1, 3, 8, 8))
    with pytest.raises(DynamoHipError):
        tools.disp_to_depth(torch.rand(1, 1, 8, 8), 0.1, 100.0)
