"""The argument lists of the ctypes binding are held to the header: every prototype of include/ec_amd.h is parsed and
``_lib.SIGNATURES`` has to agree with it in argument count and, argument by argument and for the return value, in class --
pointer or handle; ``int``, ``long``, ``size_t``, ``uint64_t``; ``float``; and where the binding uses a typed pointer
(``POINTER(c_float)``, ``POINTER(c_int)``, ``POINTER(c_size_t)``, ``POINTER(c_void_p)``) the pointee.  tests/test_cabi_symbols.py
checks the names; a miscounted ``[c_void_p] * 4`` would otherwise shift every later argument of a call silently."""
import ctypes as C
import os
import re

SCALARS = {"int": C.c_int, "long": C.c_long, "size_t": C.c_size_t, "uint64_t": C.c_uint64, "float": C.c_float}
TYPED_POINTERS = {"float": C.POINTER(C.c_float), "int": C.POINTER(C.c_int), "size_t": C.POINTER(C.c_size_t)}
HANDLE_TYPES = ("ec_stream_t", "ec_event_t")


def prototypes(repo_root):
    """{name: (return type, [parameter types])} as written in the header, qualifiers and parameter names dropped"""
    txt = open(os.path.join(repo_root, "include", "ec_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    txt = re.sub(r"//[^\n]*", " ", txt)
    txt = re.sub(r"^\s*#[^\n]*", " ", txt, flags=re.M)
    txt = re.sub(r"\b(typedef\s+struct|enum)\s*\{[^}]*\}[^;]*;", " ", txt)
    txt = re.sub(r'extern\s+"C"\s*\{', " ", txt)
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(ec_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt):
        assert name not in out, name
        params = [p.strip() for p in params.split(",")] if params.strip() not in ("", "void") else []
        out[name] = (_type(ret, False), [_type(p, True) for p in params])
    return out


def _type(decl, named):
    """`const float* masks` -> `float*`; `ec_policy_t** out` -> `ec_policy_t**`; `int T` -> `int`"""
    decl = re.sub(r"\b(const|struct|unsigned)\b", " ", decl).replace("*", " * ")
    words = decl.split()
    stars = words.count("*")
    words = [w for w in words if w != "*"]
    if named and len(words) > 1:
        words = words[:-1]                      # the parameter's name
    assert len(words) == 1, decl
    return words[0] + "*" * stars


def _agrees(ctype, htype):
    """does the binding's type belong to the class of the header's?"""
    if htype == "void":
        return ctype is None
    if htype in HANDLE_TYPES:
        return ctype is C.c_void_p
    if htype.endswith("*"):
        base, stars = htype.rstrip("*"), htype.count("*")
        if ctype is C.c_void_p:
            return True
        if ctype is C.c_char_p:
            return base == "char" and stars == 1
        if stars == 2:
            return ctype is C.POINTER(C.c_void_p)
        return ctype is TYPED_POINTERS.get(base)
    return ctype is SCALARS.get(htype)


def test_parser_reads_the_header(repo_root):
    protos = prototypes(repo_root)
    assert protos["ec_version"] == ("int", []) and protos["ec_strerror"] == ("char*", ["int"])
    assert protos["ec_policy_param_offset"] == ("int", ["ec_policy_t*", "int", "size_t*", "size_t*"])
    assert protos["ec_policy_create"] == ("int", ["ec_policy_t**", "ec_policy_cfg*"])
    assert protos["ec_policy_destroy"][0] == "void" and protos["ec_rn50_plan_hash"][0] == "uint64_t"
    assert protos["ec_policy_act_ex"][1][-2:] == ["float", "ec_stream_t"] and len(protos["ec_policy_act_ex"][1]) == 26
    assert protos["ec_gae"][1][-4:] == ["float", "float", "float", "ec_stream_t"]


def test_signatures_agree_with_the_header(repo_root):
    from embodied_clip_amd import _lib
    protos = prototypes(repo_root)
    assert sorted(protos) == sorted(_lib.SIGNATURES)
    bad = []
    for name, (res, args) in _lib.SIGNATURES.items():
        hres, hargs = protos[name]
        if len(args) != len(hargs):
            bad.append((name, "count", len(args), len(hargs)))
            continue
        if not _agrees(res, hres):
            bad.append((name, "return", res, hres))
        bad += [(name, i, a, h) for i, (a, h) in enumerate(zip(args, hargs)) if not _agrees(a, h)]
    assert not bad, bad
