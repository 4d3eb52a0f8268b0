"""The ctypes binding (cat_seg/_lib.py) is made from include/catseg_hip*.h at import.  These tests hold it
to the headers and to the compiler: every prototype bound, every struct laid out as the host compiler lays
it out, the signatures most likely to trip a parser pinned literally, and the parser refusing whatever it
does not understand instead of skipping it."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from cat_seg import _lib as L
from cat_seg.data import train_input as TI

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
HEADERS = ("catseg_hip.h", "catseg_hip_train.h", "catseg_hip_tuning.h")
vp, i32, i64, f32 = C.c_void_p, C.c_int, C.c_int64, C.c_float


def _declared(header):
    """The names a header declares, found without the binding's parser."""
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(INCLUDE, header)).read(), flags=re.S)
    return re.findall(r"\b(catseg_\w+)\s*\(", text)


def test_every_prototype_is_bound_and_nothing_else():
    product = _declared(HEADERS[0]) + _declared(HEADERS[1])
    tuning = _declared(HEADERS[2])
    assert len(product) == len(set(product)) and len(L.EXPORTED) == len(set(L.EXPORTED))
    assert set(L.EXPORTED) == set(product)
    assert set(tuning) == {"catseg_tuning_set", "catseg_tuning_get", "catseg_tuning_list"}
    assert not set(tuning) & set(L.EXPORTED)
    assert set(L._PROTOS) == set(product) | set(tuning)
    assert len(L._PROTOS) == 116 and len(L._STRUCTS) == 18
    lib = L.load()
    for name, (restype, argtypes) in L._PROTOS.items():
        fn = getattr(lib, name)                      # present in the .so
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    # the public struct names are the header's without the prefix
    for cname, cls in L._STRUCTS.items():
        assert cname.startswith("Catseg") and getattr(L, cname[len("Catseg"):]) is cls


def _host_compiler():
    for cc in ("c++", "g++", "clang++"):
        if shutil.which(cc):
            return [cc]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return [hipcc, "-x", "c++"] if os.path.exists(hipcc) else None


@pytest.fixture(scope="module")
def compiled_layout(tmp_path_factory):
    """{"CatsegX": sizeof, "CatsegX.field": (offsetof, sizeof)} as the host compiler sees the three headers."""
    cc = _host_compiler()
    if cc is None:
        pytest.skip("no host C++ compiler (c++, g++, clang++ or hipcc) on this machine")
    lines = ["#include <cstddef>", "#include <cstdio>"] + [f'#include "{h}"' for h in HEADERS] + ["int main() {"]
    for cname, cls in L._STRUCTS.items():
        lines.append(f'  std::printf("{cname} %zu\\n", sizeof({cname}));')
        for field, _ in cls._fields_:
            lines.append(f'  std::printf("{cname}.{field} %zu %zu\\n", offsetof({cname}, {field}), '
                         f"sizeof((({cname}*)0)->{field}));")
    lines += ["  return 0;", "}"]
    d = tmp_path_factory.mktemp("abi_layout")
    src, exe = d / "layout.cpp", d / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(cc + ["-std=c++11", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    table = {}
    for line in out.splitlines():
        key, *nums = line.split()
        table[key] = int(nums[0]) if len(nums) == 1 else (int(nums[0]), int(nums[1]))
    return table


def test_struct_layout_matches_the_compiler(compiled_layout):
    assert len(L._STRUCTS) == 18
    n_fields = 0
    for cname, cls in L._STRUCTS.items():
        assert C.sizeof(cls) == compiled_layout[cname], cname
        for field, _ in cls._fields_:
            d = getattr(cls, field)
            assert (d.offset, d.size) == compiled_layout[f"{cname}.{field}"], f"{cname}.{field}"
            n_fields += 1
    assert n_fields + len(L._STRUCTS) == len(compiled_layout)
    # the numpy view of the training descriptors is the same struct
    assert TI.DESC_DTYPE.itemsize == compiled_layout["CatsegTrainImageDesc"] == 128
    assert TI.DESC_WORDS == 32
    assert TI.DESC_DTYPE.names == tuple(f for f, _ in L.TrainImageDesc._fields_) and len(TI.DESC_DTYPE.names) == 27
    for field in TI.DESC_DTYPE.names:
        dt, off = TI.DESC_DTYPE.fields[field][:2]
        assert (off, dt.itemsize) == compiled_layout[f"CatsegTrainImageDesc.{field}"], field
    assert TI.DESC_DTYPE.fields["crop"][0].shape == (4,)
    assert C.sizeof(L.AdamWTensor) == compiled_layout["CatsegAdamWTensor"] == 56


PINNED = {
    "catseg_tiled_blend": (i32, [vp] + [i32] * 16 + [vp] * 5),
    "catseg_train_crop_select": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, C.c_double, vp, vp, vp]),
    "catseg_layernorm": (i32, [vp, i64, L.RowMap, i32, vp, i64, i32, vp, vp, i64, i64, f32, vp]),
    "catseg_rows_mlp": (i32, [vp, i64, i64, vp, vp, f32, vp, vp, i64, i32, vp, C.POINTER(L.RowsEpi), i32, vp]),
    "catseg_label_regions_write": (i32, [vp, i64, i64, i64, i32, vp, i64, vp, i64, vp, i64, vp, vp, vp, vp, vp, i64, vp]),
    "catseg_adamw_step": (i32, [vp, vp, i64, f32, f32, f32, f32, vp, vp, i64, vp]),
    "catseg_train_augment": (i32, [vp, vp, vp, vp, i32, i32, i64, vp, vp, vp]),
    "catseg_last_error": (C.c_char_p, []),
    "catseg_label_runs_workspace": (i64, [i64, i64]),
    "catseg_conv3x3_workspace": (i64, [C.POINTER(L.ConvArgs)]),
    "catseg_abi_version": (i32, []),
    "catseg_tuning_set": (i32, [C.c_char_p, i32]),
    "catseg_tuning_get": (i32, [C.c_char_p, C.POINTER(C.c_int)]),
    "catseg_tuning_list": (C.c_char_p, []),
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_signature(name):
    restype, argtypes = PINNED[name]
    assert L._PROTOS[name][0] is restype
    assert L._PROTOS[name][1] == argtypes            # ctypes caches POINTER(cls): == is identity per entry
    fn = getattr(L.load(), name)
    assert fn.restype is restype and list(fn.argtypes) == argtypes


def test_constants_come_from_the_header_enums():
    assert (L.F32, L.BF16, L.FP8) == (0, 1, 2)
    assert (L.ACT_NONE, L.ACT_RELU, L.ACT_GELU, L.ACT_QUICKGELU, L.ACT_SIGMOID) == (0, 1, 2, 3, 4)
    assert L._ENUMS["CATSEG_ERR_ARG"] == -1 and L._ENUMS["CATSEG_ERR_HIP"] == -2
    assert bytes(L.IDENTITY) == bytes(L.RowMap(1, 1 << 62, 1, 1, 1, 0, 0))


GOOD = """
/* a comment with catseg_ghost( in it */
enum { CATSEG_A = 0, CATSEG_B = -3 };
typedef struct { int64_t n, m; const float* p; int32_t box[4]; } CatsegThing;
int catseg_one(const CatsegThing* t, CatsegThing by_value, const uint8_t* bytes,
               double d, void* stream);
int64_t catseg_two(void);
"""

REFUSED = {
    "unknown type": ("int catseg_bad(const half* x, void* stream);", "catseg_bad"),
    "unknown scalar": ("int catseg_bad(unsigned n);", "catseg_bad"),
    "pointer to pointer": ("int catseg_bad(float** rows);", "catseg_bad"),
    "unnamed parameter": ("int catseg_bad(int, void* stream);", "catseg_bad"),
    "function pointer": ("int catseg_bad(int (*cb)(int), void* stream);", "catseg_bad"),
    "missing semicolon": ("int catseg_bad(int a)\nint catseg_worse(int b);", "catseg_bad"),
    "inline body": ("static inline int catseg_bad(int a) { return a; }", "catseg_bad"),
    "unknown return": ("size_t catseg_bad(int a);", "catseg_bad"),
    "declared twice": ("int catseg_bad(int a);\nint catseg_bad(int a);", "declared twice"),
    "struct field of unknown type": ("typedef struct { int64_t n; half* p; } CatsegBad;", "CatsegBad"),
    "struct field, two pointers in one list": ("typedef struct { float* a, b; } CatsegBad;", "CatsegBad"),
    "named struct": ("typedef struct CatsegBad { int n; } CatsegBad;\nint catseg_ok(int a);", "CatsegBad"),
    "enum without a value": ("enum { CATSEG_BAD };", "CATSEG_BAD"),
}


def test_parser_reads_the_vocabulary():
    structs, enums, protos = L.parse_abi(GOOD)
    T = structs["CatsegThing"]
    assert T.__name__ == "Thing"
    assert [(n, t) for n, t in T._fields_] == [("n", i64), ("m", i64), ("p", vp), ("box", i32 * 4)]
    assert enums == {"CATSEG_A": 0, "CATSEG_B": -3}
    assert protos == {"catseg_one": (i32, [C.POINTER(T), T, vp, C.c_double, vp]), "catseg_two": (i64, [])}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_parser_refuses_what_it_does_not_understand(case):
    text, names = REFUSED[case]
    with pytest.raises(RuntimeError, match=re.escape(names)):
        L.parse_abi(GOOD + text)


def test_missing_header_is_a_loud_error(monkeypatch, tmp_path):
    monkeypatch.setattr(L, "INCLUDE_DIR", str(tmp_path))
    with pytest.raises(RuntimeError, match="catseg_hip.h not found"):
        L._read_headers()
