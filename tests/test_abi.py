"""CPU-only: the C-ABI library is present, loads, and exports every symbol include/mh_pmvo.h declares."""
import ctypes
import os
import re

from conftest import ROOT


def declared_symbols(headers=("mh_pmvo.h", "mh_pmvo_lab.h")):
    out = set()
    for h in headers:
        hdr = open(os.path.join(ROOT, "include", h)).read()
        hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
        out |= set(re.findall(r"\b(mh_[a-z_0-9]+)\s*\(", hdr))
    return sorted(out)


def declared_prototypes(headers=("mh_pmvo.h", "mh_pmvo_lab.h")):
    """{name: (return type, [parameter types])} of every prototype, each type reduced to its class: "pointer", "char*"
    (const char *), "void" or the scalar type's own name."""
    def kind(decl, named):
        decl = " ".join(decl.replace("*", " * ").split())
        if "*" in decl:
            return "char*" if decl.startswith("const char *") and decl.count("*") == 1 else "pointer"
        words = [w for w in decl.split() if w != "const"]
        if named and len(words) > 1:
            words = words[:-1]       # the parameter's name
        return " ".join(words)

    return {name: (kind(ret, False), [kind(q, True) for q in params])
            for name, (ret, params) in declared_parameters(headers).items()}


def declared_parameters(headers=("mh_pmvo.h", "mh_pmvo_lab.h")):
    """{name: (return declaration, [parameter declarations])} of every prototype, as written (comments removed, blanks
    folded): what tells a `const float *` from a `float *`"""
    out = {}
    for h in headers:
        hdr = open(os.path.join(ROOT, "include", h)).read()
        hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
        hdr = re.sub(r"^\s*#.*$", "", hdr, flags=re.M)
        for ret, name, params in re.findall(r"([^;{}()]*?)\b(mh_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", hdr):
            params = [] if params.strip() in ("", "void") else [" ".join(q.split()) for q in params.split(",")]
            assert name not in out, name
            out[name] = (" ".join(ret.split()), params)
    return out


def bound_kind(t):
    """the class of a ctypes type in the terms of declared_prototypes"""
    if t is None:
        return "void"
    if t is ctypes.c_char_p:
        return "char*"
    if t is ctypes.c_void_p or issubclass(t, ctypes._Pointer):
        return "pointer"
    return {ctypes.c_int: "int", ctypes.c_float: "float", ctypes.c_double: "double", ctypes.c_longlong: "long long",
            ctypes.c_size_t: "size_t"}[t]


def test_lab_switches_are_not_in_the_supported_header():
    """include/mh_pmvo.h is what an integrator binds; the A/B forms and cross-check kernels live in mh_pmvo_lab.h"""
    main, lab = set(declared_symbols(("mh_pmvo.h",))), set(declared_symbols(("mh_pmvo_lab.h",)))
    assert lab == {"mh_ctx_set_lab_option", "mh_debug_key_stats"} and not (main & lab)
    doc = open(os.path.join(ROOT, "include", "mh_pmvo.h")).read()
    for key in ("search_variant", "search_body", "taps_tile", "tap_codes"):
        assert '"%s"' % key not in doc, key


def test_header_declares_the_bound_entry_points():
    from monohair_amd import _lib

    assert set(_lib.EXPORTS) == set(declared_symbols())
    # ... with the types the headers give them: the ctypes table is a hand-written copy of the prototypes
    protos = declared_prototypes()
    assert sorted(protos) == declared_symbols()
    bound = {name: (bound_kind(res), [bound_kind(a) for a in args]) for name, (res, args) in _lib._SIGS.items()}
    assert {n: (protos[n], bound[n]) for n in protos if protos[n] != bound[n]} == {}


def test_library_loads_and_exports_everything():
    from monohair_amd import _lib

    assert os.path.exists(_lib.LIB_PATH), "build with __graft_entry__.build()"
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared_symbols():
        assert hasattr(L, name), name
    assert _lib.lib().mh_version() >= 100


def test_product_never_imports_the_oracle():
    """The oracle is test infrastructure: nothing under monohair_amd/ (or PMVO.py) may import it."""
    bad = []
    for base, _, files in os.walk(os.path.join(ROOT, "monohair_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(base, f)).read()
                if re.search(r"^\s*(import|from)\s+oracle\b", src, flags=re.M):
                    bad.append(os.path.join(base, f))
    assert not bad, bad


def test_no_gpu_means_loud_failure():
    import pytest
    import torch

    from monohair_amd import _lib, pmvo

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_lib.MhError):
        pmvo.PMVO({}, {}, {}, {}, {}, device="cuda:0", image_size=[8, 8])


def test_integration_doc_names_every_entry_point():
    """INTEGRATION.md maps each C entry point to the reference code it replaces: keep it complete."""
    from monohair_amd import _lib

    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert [n for n in _lib.EXPORTS if n not in doc] == []
