"""Host half of the connected-region / sieve feature: the numpy / scipy restatement (tests/regions_ref.py), which
the GPU tests hold the kernels to, against hand-written answers on maps of at most 5 x 5; the config keys and the
refused combinations of MODEL.CATSEG_HIP.REGIONS; the C ABI entries and their host-side argument checks; and the
kernels' index / union / key logic (csrc/label_regions_logic.h) run sequentially on the host against a flood fill
(tools/label_regions_host.cpp)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import regions_ref as R
from cat_seg import _lib as L
from cat_seg import build_model

from conftest import ROOT
from test_boundary_cpu import tiny_cfg


def test_diagonal_pair_is_one_region_under_8_and_two_under_4():
    m = np.array([[1, 0],
                  [0, 1]])
    ids8, t8 = R.regions(m, 8)
    assert ids8.tolist() == [[0, 1], [1, 0]]
    assert t8["label"].tolist() == [1, 0] and t8["area"].tolist() == [2, 2]
    assert t8["bbox"].tolist() == [[0, 0, 2, 2], [0, 0, 2, 2]] and t8["first"].tolist() == [0, 1]
    ids4, t4 = R.regions(m, 4)
    assert ids4.tolist() == [[0, 1], [2, 3]]
    assert t4["label"].tolist() == [1, 0, 0, 1] and t4["area"].tolist() == [1, 1, 1, 1]
    assert t4["bbox"].tolist() == [[0, 0, 1, 1], [1, 0, 2, 1], [0, 1, 1, 2], [1, 1, 2, 2]]
    assert t4["first"].tolist() == [0, 1, 2, 3]


def test_ring_with_a_hole_is_numbered_by_the_rings_first_pixel():
    m = np.array([[0, 0, 0, 0, 0],
                  [0, 5, 5, 5, 0],
                  [0, 5, 0, 5, 0],
                  [0, 5, 5, 5, 0],
                  [0, 0, 0, 0, 0]])
    for conn in (4, 8):
        ids, t = R.regions(m, conn)
        assert ids.tolist() == [[0, 0, 0, 0, 0], [0, 1, 1, 1, 0], [0, 1, 2, 1, 0], [0, 1, 1, 1, 0], [0, 0, 0, 0, 0]]
        assert t["label"].tolist() == [0, 5, 0] and t["area"].tolist() == [16, 8, 1]
        assert t["first"].tolist() == [0, 6, 12]
        assert t["bbox"].tolist() == [[0, 0, 5, 5], [1, 1, 4, 4], [2, 2, 3, 3]]
    assert ids.dtype == np.int32 and all(v.dtype == np.int32 for v in t.values())


def test_fold_joins_labels_at_and_above_the_clamp():
    m = np.array([[20, 21, 3]])
    assert R.regions(m, 4)[0].tolist() == [[0, 1, 2]]
    ids, t = R.regions(m, 4, clamp_pred=20)
    assert ids.tolist() == [[0, 0, 1]] and t["label"].tolist() == [20, 3]


def test_score_sum_is_fixed_point_with_ties_to_even():
    m = np.array([[1, 1, 2]])
    s = np.array([[0.5 / 65536, 1.5 / 65536, 1.0]], np.float32)
    _, t = R.regions(m, 4, score=s)
    assert t["score_q16"].tolist() == [0 + 2, 65536] and t["score_q16"].dtype == np.int64
    assert t["score"].dtype == np.float32 and t["score"].tolist() == [np.float32(2 / 65536 / 2), 1.0]


# regions (conn 4): 0 = the 1s (area 3), 1 = the single 9, 2 = the 2s (area 3); the 9 touches both large regions
TIE = np.array([[1, 9, 2],
                [1, 0, 2],
                [1, 0, 2]])
# every region has area 1 or 2: with min_area 3 nothing is large and nothing moves
ONLY_SMALL = np.array([[1, 2, 2],
                       [3, 4, 4]])


def test_sieve_tie_goes_to_the_lower_region_number():
    ids, t = R.regions(TIE, 4)
    assert ids.tolist() == [[0, 1, 2], [0, 3, 2], [0, 3, 2]] and t["area"].tolist() == [3, 1, 3, 2]
    out = R.sieve(TIE, 3, 4)
    # the 9 (area 1) touches regions 0 and 2, both of area 3: region 0 wins; the 0s (area 2) likewise
    assert out.tolist() == [[1, 1, 2], [1, 1, 2], [1, 1, 2]]
    # min_area 2: only the 9 is small; the 0s (area 2) are large but smaller than the tied 3s
    assert R.sieve(TIE, 2, 4).tolist() == [[1, 1, 2], [1, 0, 2], [1, 0, 2]]
    # the largest area wins before the region number does
    m = np.array([[1, 9, 2, 2],
                  [1, 0, 2, 2]])
    assert R.sieve(m, 2, 4).tolist() == [[1, 2, 2, 2], [1, 2, 2, 2]]
    assert out.dtype == np.int32


def test_sieve_keeps_a_small_region_with_only_small_neighbours():
    assert R.sieve(ONLY_SMALL, 3, 4).tolist() == ONLY_SMALL.tolist()
    assert R.sieve(ONLY_SMALL, 3, 8).tolist() == ONLY_SMALL.tolist()
    # one pass, not iterated: the 7 touches only the ring of 8s, which is small, and stays, though the ring moves
    m = np.array([[1, 1, 1, 1, 1],
                  [1, 8, 8, 8, 1],
                  [1, 8, 7, 8, 1],
                  [1, 8, 8, 8, 1],
                  [1, 1, 1, 1, 1]])
    for conn in (4, 8):
        assert R.regions(m, conn)[1]["area"].tolist() == [16, 8, 1]
        out = R.sieve(m, 9, conn)
        assert out[2, 2] == 7 and (out == 1).sum() == 24


def test_sieve_min_area_1_is_the_identity():
    rng = np.random.default_rng(0)
    m = rng.integers(-3, 4, (5, 5))
    for conn in (4, 8):
        assert np.array_equal(R.sieve(m, 1, conn), m)
        assert np.array_equal(R.sieve(m, 26, conn), m)          # nothing is large


def test_sieve_under_8_sees_diagonal_neighbours():
    m = np.array([[1, 1, 0],
                  [1, 1, 0],
                  [0, 0, 9]])
    # under 4 the 0s are two regions of area 2, which take the 1s' label, and the 9 touches only them and stays;
    # under 8 the 0s join into one region of area 4 and the 9 also touches the 1s (area 4, the lower number)
    assert R.sieve(m, 3, 4).tolist() == [[1, 1, 1], [1, 1, 1], [1, 1, 9]]
    assert R.sieve(m, 3, 8).tolist() == [[1, 1, 0], [1, 1, 0], [0, 0, 1]]


def test_config_keys_and_defaults():
    cfg = tiny_cfg()
    node = cfg.MODEL.CATSEG_HIP.REGIONS
    assert node.ENABLED is False and node.CONNECTIVITY == 8 and node.MIN_AREA == 0
    cfg = tiny_cfg(**{"MODEL.CATSEG_HIP.REGIONS.ENABLED": "True", "MODEL.CATSEG_HIP.REGIONS.CONNECTIVITY": "4",
                      "MODEL.CATSEG_HIP.REGIONS.MIN_AREA": "6", "MODEL.CATSEG_HIP.OUTPUT": "labels"})
    m = build_model(cfg)
    assert m.regions is True and m.regions_connectivity == 4 and m.regions_min_area == 6
    m = build_model(tiny_cfg())
    assert m.regions is False


@pytest.mark.parametrize("over", [
    {"MODEL.CATSEG_HIP.REGIONS.ENABLED": "True"},                                          # OUTPUT "probs"
    {"MODEL.CATSEG_HIP.REGIONS.ENABLED": "True", "MODEL.CATSEG_HIP.OUTPUT": "labels",
     "MODEL.CATSEG_HIP.REGIONS.CONNECTIVITY": "6"},
    {"MODEL.CATSEG_HIP.REGIONS.ENABLED": "True", "MODEL.CATSEG_HIP.OUTPUT": "labels",
     "MODEL.CATSEG_HIP.REGIONS.MIN_AREA": "-1"},
])
def test_refused_combinations_raise_at_construction(over):
    with pytest.raises(ValueError, match="REGIONS"):
        build_model(tiny_cfg(**over))


NEW = ("catseg_label_regions_workspace", "catseg_label_regions_count", "catseg_label_regions_write",
       "catseg_sieve_labels")


def test_header_and_lib_carry_the_symbols():
    declared = set(re.findall(r"\b(catseg_\w+)\s*\(", open(os.path.join(ROOT, "include", "catseg_hip.h")).read()))
    lib = L.load()
    for s in NEW:
        assert s in declared and s in L.EXPORTED and hasattr(lib, s), s


def test_workspace_and_argument_checks_without_gpu():
    """The host-side checks return before anything is launched: bad arguments are refused without a device."""
    lib = L.load()
    ws = lib.catseg_label_regions_workspace
    assert ws(0, 5, 0) == 0 and ws(5, -1, 1) == 0
    assert ws(1 << 16, 1 << 15, 0) == 0 and ws(1 << 16, 1 << 15, 1) == 0        # H * W == 2^31
    # 70 x 100: 7000 pixels, 110 segments of 64 -> 112 padded, one scan block
    assert ws(70, 100, 0) == 4 * (4 + 7000 + 3 * 112 + 1)
    assert ws(70, 100, 1) == 4 * (4 + 4 * 7000)
    nb, ns = ws(8, 8, 0), ws(8, 8, 1)
    p = 1 << 20                                     # an aligned non-null address, never dereferenced on these paths
    count = lambda *a: lib.catseg_label_regions_count(*a)
    assert count(None, 8, 8, 8, -1, 8, p, nb, None) == -1
    assert count(p, 8, 8, 7, -1, 8, p, nb, None) == -1                  # ld < W
    assert count(p, 8, 8, 8, -1, 6, p, nb, None) == -1                  # connectivity 6
    assert count(p, 8, 8, 8, -1, 8, p, nb - 4, None) == -1              # workspace too small
    assert count(p, 8, 8, 8, -1, 8, p + 4, nb, None) == -1              # workspace misaligned
    assert count(p, 1 << 16, 1 << 15, 1 << 15, -1, 8, p, nb, None) == -1
    assert b"2^31" in lib.catseg_last_error()
    write = lambda *a: lib.catseg_label_regions_write(*a)
    assert write(p, 8, 8, 8, -1, None, 0, p, nb, None, 8, p, p, p, p, None, 4, None) == -1     # no region_ids
    assert write(p, 8, 8, 8, -1, None, 0, p, nb, p, 7, p, p, p, p, None, 4, None) == -1        # ld_ids < W
    assert write(p, 8, 8, 8, -1, None, 0, p, nb, p, 8, p, p, p, p, None, -1, None) == -1       # capacity < 0
    assert write(p, 8, 8, 8, -1, None, 0, p, nb, p, 8, p, None, p, p, None, 4, None) == -1     # a null column
    assert write(p, 8, 8, 8, -1, p, 8, p, nb, p, 8, p, p, p, p, None, 4, None) == -1           # score without score_q16
    assert write(p, 8, 8, 8, -1, p, 7, p, nb, p, 8, p, p, p, p, p, 4, None) == -1              # ld_score < W
    sieve = lambda *a: lib.catseg_sieve_labels(*a)
    q = p + (1 << 16)
    assert sieve(p, 8, 8, 8, -1, 8, 0, q, 8, p, ns, None) == -1         # min_area 0
    assert b"min_area" in lib.catseg_last_error()
    assert sieve(p, 8, 8, 8, -1, 6, 2, q, 8, p, ns, None) == -1         # connectivity 6
    assert sieve(p, 8, 8, 7, -1, 8, 2, q, 8, p, ns, None) == -1         # ld < W
    assert sieve(p, 8, 8, 8, -1, 8, 2, q, 7, p, ns, None) == -1         # ld_out < W
    assert sieve(p, 8, 8, 8, -1, 8, 2, p + 64, 8, p, ns, None) == -1    # out overlaps labels
    assert sieve(p, 8, 8, 8, -1, 8, 2, q, 8, p, nb, None) == -1         # the count workspace is too small for the sieve
    assert sieve(p, 1 << 16, 1 << 15, 1 << 15, -1, 8, 2, q, 1 << 15, p, ns, None) == -1


def test_kernel_logic_on_the_host_against_a_flood_fill(tmp_path):
    """tools/label_regions_host.cpp: the per-pixel functions the kernels call, phase by phase in shuffled pixel
    orders, on the GPU tests' shapes and patterns; labelling against a flood fill, the sieve's keys against a
    direct search."""
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "label_regions_host")
    subprocess.run([cxx, "-std=c++17", "-O2", "-I", os.path.join(ROOT, "cat-seg_amd", "csrc"),
                    os.path.join(ROOT, "tools", "label_regions_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().startswith("ok"), r.stdout[-2000:]
