"""ctypes binding of libcatseg_hip.so, derived from its C headers (include/catseg_hip*.h).

The library is the product: there is no fallback.  Loading fails loudly when the
shared object is missing, and `require_gpu()` fails when no HIP device is
visible, so nothing on the path can silently run elsewhere.

The headers are the one definition of the ABI: `parse_abi` reads them once at import and
makes every struct class, enum constant, argument list and return type from them (the product
headers, the tuning header, and the function-only headers catseg_hip.h includes).  A
declaration it does not understand is an error, never a skipped entry.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CATSEG_HIP_LIB", os.path.join(_HERE, "libcatseg_hip.so"))
INCLUDE_DIR = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include")
PRODUCT_HEADERS = ("catseg_hip.h", "catseg_hip_train.h")
TUNING_HEADER = "catseg_hip_tuning.h"          # diagnostics entry, not part of the product ABI
# product entries declared in headers of their own, which catseg_hip.h includes (the outline simplifier)
INCLUDED_HEADERS = ("catseg_hip_simplify.h",)
# later function-only headers catseg_hip.h includes, a group of their own (the boundary-aware evaluation)
EXTENSION_HEADERS = ("catseg_hip_boundary.h",)
# and a third such group (the label-map renderer)
RENDER_HEADERS = ("catseg_hip_render.h",)
# and a fourth (the confidence outputs: top-k label maps and calibration counters)
CONFIDENCE_HEADERS = ("catseg_hip_confidence.h",)
# and a fifth (the majority filter and the mode overviews of label maps)
MODE_HEADERS = ("catseg_hip_mode.h",)

BIG = 1 << 62

_SCALARS = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "uint8_t": C.c_uint8, "int16_t": C.c_int16,
            "float": C.c_float, "double": C.c_double}
# catseg_hip_train.h says of each: "an array of these lives in DEVICE memory".  The host fills them as
# bytes and passes a device address, so a pointer to one is a plain c_void_p, not POINTER(cls).
DEVICE_ARRAY_STRUCTS = ("CatsegAdamWTensor", "CatsegTrainImageDesc")

_NAME = r"(\w+)\s*(?:\[(\d+)\])?"
_DECL = re.compile(r"(.+?)\s*\b" + _NAME)
_STRUCT = re.compile(r"typedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;")
_ENUM = re.compile(r"enum\s*\{([^{}]*)\}\s*;")
_PROTO = re.compile(r"(.+?)\b(catseg_\w+)\s*\(([^()]*)\)", re.S)


def _ctype(spec, structs, decl, ret=False):
    words = spec.replace("*", " * ").split()
    base = [w for w in words if w not in ("const", "*")]
    stars, name = words.count("*"), base[0] if len(base) == 1 else None
    if stars == 0 and name in _SCALARS:
        return _SCALARS[name]
    if stars == 0 and name in structs:
        return structs[name]
    if stars == 0 and name == "void" and ret:
        return None
    if stars == 1 and name == "char":
        return C.c_char_p
    if stars == 1 and (name in _SCALARS or name == "void"):
        return C.c_void_p
    if stars == 1 and name in structs:
        return C.c_void_p if name in DEVICE_ARRAY_STRUCTS else C.POINTER(structs[name])
    raise RuntimeError(f"type {spec!r} is outside the vocabulary of the ABI headers in `{decl}`")


def _declarators(text, structs, decl):
    """`type a, b[4]` -> [(a, ctype), (b, ctype * 4)]."""
    first, *more = [" ".join(p.split()) for p in text.split(",")]
    m = _DECL.fullmatch(first)
    rest = [re.fullmatch(_NAME, p) for p in more]
    if not m or not all(rest) or ("*" in m.group(1) and rest):
        raise RuntimeError(f"cannot parse `{text.strip()}` in `{decl}`")
    t = _ctype(m.group(1), structs, decl)
    return [(n, t * int(dim) if dim else t) for n, dim in [m.groups()[1:]] + [r.groups() for r in rest]]


def parse_abi(text, structs=None):
    """Parse the text of one ABI header.  `structs`: the {C name: class} of the headers it includes.
    Returns (structs, enums, protos): {C name: ctypes.Structure class}, {name: int} and
    {name: (restype, argtypes)}.  Raises RuntimeError naming the declaration it cannot map."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"#ifdef __cplusplus.*?#endif", " ", text, flags=re.S)      # extern "C" { ... }
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    structs, enums, protos = dict(structs or {}), {}, {}
    for body, name in _STRUCT.findall(text):
        decl = f"struct {name}"
        fields = [f for part in body.split(";") if part.strip() for f in _declarators(part, structs, decl)]
        structs[name] = type(name.replace("Catseg", "", 1), (C.Structure,), {"_fields_": fields})
    for body in _ENUM.findall(text):
        for item in body.split(","):
            m = re.fullmatch(r"\s*(\w+)\s*=\s*(-?\d+)\s*", item)
            if not m:
                raise RuntimeError(f"cannot parse `{item.strip()}` in `enum {{{' '.join(body.split())}}}`")
            enums[m.group(1)] = int(m.group(2))
    for chunk in _ENUM.sub(" ", _STRUCT.sub(" ", text)).split(";"):
        decl = " ".join(chunk.split())
        if not decl:
            continue
        m = _PROTO.fullmatch(chunk.strip())
        if not m:
            raise RuntimeError(f"cannot parse `{decl}`")
        params = m.group(3).strip()
        args = [] if params in ("", "void") else [_declarators(p, structs, decl)[0][1] for p in params.split(",")]
        protos[m.group(2)] = (_ctype(m.group(1), structs, decl, ret=True), args)
    n = len(re.findall(r"catseg_\w+\s*\(", text))
    if len(protos) != n:
        raise RuntimeError(f"{n} `catseg_*(` in the header text, {len(protos)} prototypes parsed: one was "
                           "skipped or declared twice")
    return structs, enums, protos


def _read_headers():
    structs, enums, protos, exported = {}, {}, {}, ()
    for h in PRODUCT_HEADERS + (TUNING_HEADER,):
        path = os.path.join(INCLUDE_DIR, h)
        if not os.path.exists(path):
            raise RuntimeError(f"{h} not found at {path}: the ctypes binding of libcatseg_hip.so is made from the "
                               "headers in include/ and has no other definition")
        try:
            structs, e, p = parse_abi(open(path).read(), structs)
        except RuntimeError as err:
            raise RuntimeError(f"{path}: {err}") from None
        enums.update(e)
        protos.update(p)
        if h in PRODUCT_HEADERS:
            exported = tuple(protos)
    # the one host out-parameter of the ABI: `int* value`, filled through byref()
    protos["catseg_tuning_get"][1][1] = C.POINTER(C.c_int)
    return structs, enums, protos, exported


def _read_included_headers(structs, headers=INCLUDED_HEADERS):
    protos = {}
    for h in headers:
        path = os.path.join(INCLUDE_DIR, h)
        if not os.path.exists(path):
            raise RuntimeError(f"{h} not found at {path}: catseg_hip.h includes it")
        try:
            more, enums, p = parse_abi(open(path).read(), structs)
        except RuntimeError as err:
            raise RuntimeError(f"{path}: {err}") from None
        if len(more) != len(structs) or enums or set(p) & set(protos):
            raise RuntimeError(f"{path}: an included header declares functions only, each once")
        protos.update(p)
    return protos


_STRUCTS, _ENUMS, _PROTOS, EXPORTED = _read_headers()
_INCLUDED_PROTOS = _read_included_headers(_STRUCTS)
if set(_INCLUDED_PROTOS) & set(_PROTOS):
    raise RuntimeError(f"declared twice: {sorted(set(_INCLUDED_PROTOS) & set(_PROTOS))}")
EXPORTED_INCLUDED = tuple(_INCLUDED_PROTOS)
_EXTENSION_PROTOS = _read_included_headers(_STRUCTS, EXTENSION_HEADERS)
if set(_EXTENSION_PROTOS) & (set(_PROTOS) | set(_INCLUDED_PROTOS)):
    raise RuntimeError(f"declared twice: {sorted(set(_EXTENSION_PROTOS) & (set(_PROTOS) | set(_INCLUDED_PROTOS)))}")
EXPORTED_EXTENSIONS = tuple(_EXTENSION_PROTOS)
_RENDER_PROTOS = _read_included_headers(_STRUCTS, RENDER_HEADERS)
if set(_RENDER_PROTOS) & (set(_PROTOS) | set(_INCLUDED_PROTOS) | set(_EXTENSION_PROTOS)):
    raise RuntimeError("declared twice: "
                       f"{sorted(set(_RENDER_PROTOS) & (set(_PROTOS) | set(_INCLUDED_PROTOS) | set(_EXTENSION_PROTOS)))}")
EXPORTED_RENDER = tuple(_RENDER_PROTOS)
_CONFIDENCE_PROTOS = _read_included_headers(_STRUCTS, CONFIDENCE_HEADERS)
_EARLIER = set(_PROTOS) | set(_INCLUDED_PROTOS) | set(_EXTENSION_PROTOS) | set(_RENDER_PROTOS)
if set(_CONFIDENCE_PROTOS) & _EARLIER:
    raise RuntimeError(f"declared twice: {sorted(set(_CONFIDENCE_PROTOS) & _EARLIER)}")
EXPORTED_CONFIDENCE = tuple(_CONFIDENCE_PROTOS)
_MODE_PROTOS = _read_included_headers(_STRUCTS, MODE_HEADERS)
if set(_MODE_PROTOS) & (_EARLIER | set(_CONFIDENCE_PROTOS)):
    raise RuntimeError(f"declared twice: {sorted(set(_MODE_PROTOS) & (_EARLIER | set(_CONFIDENCE_PROTOS)))}")
EXPORTED_MODE = tuple(_MODE_PROTOS)
# the struct classes under their header names without the prefix: RowMap, GemmArgs, RowsEpi, AdamWTensor, ...
globals().update({cls.__name__: cls for cls in _STRUCTS.values()})
F32, BF16, FP8 = (_ENUMS["CATSEG_" + n] for n in ("F32", "BF16", "FP8"))
ACT_NONE, ACT_RELU, ACT_GELU, ACT_QUICKGELU, ACT_SIGMOID = (
    _ENUMS["CATSEG_ACT_" + n] for n in ("NONE", "RELU", "GELU", "QUICKGELU", "SIGMOID"))


def rowmap(d1=1, m1=BIG, s1=1, d2=1, m2=1, s2=0, off=0) -> RowMap:  # noqa: F821
    return RowMap(d1, m1, s1, d2, m2, s2, off)  # noqa: F821


IDENTITY = rowmap()

_lib = None


def load() -> C.CDLL:
    """Load libcatseg_hip.so (raises if it is missing — there is no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"libcatseg_hip.so not found at {LIB_PATH}: build it with "
            "`make -C cat-seg_amd/csrc` (or __graft_entry__.build()); the CAT-Seg HIP path has no fallback")
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in {**_PROTOS, **_INCLUDED_PROTOS, **_EXTENSION_PROTOS, **_RENDER_PROTOS,
                                      **_CONFIDENCE_PROTOS, **_MODE_PROTOS}.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = argtypes, restype
    _lib = lib
    return lib


def call(name: str, *args) -> None:
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        msg = lib.catseg_last_error().decode(errors="replace")
        raise RuntimeError(f"{name} failed ({rc}): {msg}")


def tune(name: str, value: int) -> None:
    """Force an A/B knob (include/catseg_hip_tuning.h; tests / tools only): process-wide, read at
    launch.  Raises on an unknown name."""
    call("catseg_tuning_set", name.encode(), int(value))


def tuning(name: str) -> int:
    v = C.c_int(0)
    call("catseg_tuning_get", name.encode(), C.byref(v))
    return v.value


def tuning_knobs():
    return load().catseg_tuning_list().decode().split(",")


def require_gpu():
    import torch

    if not torch.cuda.is_available():
        raise RuntimeError("the CAT-Seg HIP path needs a visible MI355X (torch.cuda.is_available() is False)")
    load()
