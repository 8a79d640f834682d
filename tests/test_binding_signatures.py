"""The ctypes signatures of diff_gaussian_rasterization._C against include/gsr.h (no GPU needed).

_C._load spells every entry point's `argtypes` as an anonymous list; a slipped position would
compile, load and hand the GPU the wrong pointer.  Every `gsr_*` prototype of the header is parsed
here and compared, position by position, with what the binding declares."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "bool": ctypes.c_bool, "size_t": ctypes.c_size_t,
           "unsigned": ctypes.c_uint, "long": ctypes.c_long}
POINTER_TYPEDEFS = ("gsr_stream_t", "gsr_resize_fn")


def _prototypes():
    """{name: (return type, [parameter type, ...])} of every gsr_* function the header declares; a
    parameter type is its declaration without `const` and without the parameter's name."""
    with open(os.path.join(ROOT, "include", "gsr.h")) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s]*?[\w*])\s*\b(gsr_\w+)\s*\(([^()]*)\)\s*;", text):
        ret = " ".join(ret.replace("const", " ").split())
        types = []
        for p in params.split(","):
            p = " ".join(p.replace("const", " ").split())
            if p in ("void", ""):
                continue
            m = re.fullmatch(r"(.*?)\s*\b\w+", p)  # drop the parameter's name
            types.append(m.group(1).replace(" ", ""))
        protos[name] = (ret.replace(" ", ""), types)
    return protos


def _is_pointer(ct):
    return ct is ctypes.c_void_p or (isinstance(ct, type) and issubclass(ct, ctypes._Pointer))


def test_argtypes_match_header():
    from diff_gaussian_rasterization import _C
    protos = _prototypes()
    checked, bad = 0, []
    for name, (ret, types) in sorted(protos.items()):
        fn = getattr(_C.lib, name, None)
        if fn is None or fn.argtypes is None:
            continue
        checked += 1
        if len(fn.argtypes) != len(types):
            bad.append(f"{name}: {len(fn.argtypes)} argtypes, header has {len(types)} parameters")
            continue
        for k, (ct, t) in enumerate(zip(fn.argtypes, types)):
            if "*" in t or t in POINTER_TYPEDEFS:
                ok = _is_pointer(ct)
            else:
                ok = t in SCALARS and ct is SCALARS[t]
            if not ok:
                bad.append(f"{name}: parameter {k} is `{t}` in the header, {ct.__name__} in the binding")
        want = {"size_t": ctypes.c_size_t, "char*": ctypes.c_char_p}.get(ret)
        if want is not None and fn.restype is not want:
            bad.append(f"{name}: returns {ret}, restype is {fn.restype}")
    assert not bad, "\n".join(bad)
    assert len(protos) >= 50, f"parsed only {len(protos)} prototypes from gsr.h"
    assert checked >= 40, f"only {checked} bound functions were checked"
