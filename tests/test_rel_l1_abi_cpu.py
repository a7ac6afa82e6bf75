"""CPU: the entry points that are declared beside their source (mikudance_amd/csrc/*.h named in _lib.EXTENSION_SIGNATURES) instead of in
include/mdance_hip.h: header, binding table and shared library agree, symbol for symbol and argument for argument (no compute).  What
tests/test_abi.py holds for include/*.h, for these."""
import ctypes
import os
import re

from mikudance_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mikudance_amd", "csrc")
KIND = {"P": ctypes.c_void_p, "int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "size_t": ctypes.c_size_t}


def _prototypes(header):
    """{symbol: (result kind, [argument kinds])} of the md_* prototypes in a header, comments removed."""
    text = open(os.path.join(CSRC, header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    out = {}
    for res, name, args in re.findall(r"\b(int|size_t)\s+(md_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        out[name] = (res, ["P" if "*" in a else a.split()[-2] for a in args.split(",")])
    return out


def test_extension_headers_tables_and_library_agree():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert "rel_l1.h" in _lib.EXTENSION_SIGNATURES
    seen = set()
    for header, table in _lib.EXTENSION_SIGNATURES.items():
        protos = _prototypes(header)
        assert set(protos) == set(table) and protos, (header, set(protos) ^ set(table))
        for name, (res, args) in protos.items():
            assert hasattr(lib, name), f"{name} declared in csrc/{header} but not exported"
            assert table[name] == (KIND[res], [KIND[a] for a in args]), name
            assert name not in _lib.SIGNATURES and name not in seen       # one table per symbol
            seen.add(name)
        assert header in open(os.path.join(CSRC, "Makefile")).read()       # the object is rebuilt when its header changes
    assert set(_lib.EXTENSION_SIGNATURES["rel_l1.h"]) == {"md_rel_l1_f16", "md_rel_l1_workspace_bytes"}
    typed = _lib.load()
    for table in _lib.EXTENSION_SIGNATURES.values():
        for name, (res, args) in table.items():
            fn = getattr(typed, name)
            assert fn.restype is res and fn.argtypes == args, name
    assert typed.md_rel_l1_workspace_bytes(1, 8) == 8 and typed.md_rel_l1_workspace_bytes(0, 8) == 0
    assert typed.md_rel_l1_workspace_bytes(1 << 20, 320) == 2048 * 8       # the cap on the grid: at most 16 KiB
