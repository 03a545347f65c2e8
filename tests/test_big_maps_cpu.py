"""Host only (no launch): what build_header (csrc/oc_level_host.h) makes of maps around the 64-cell
boundary, read back through the C ABI (oc_level_spec_source -- the text of the specialised header).

  planes128 -- the STRUCTURE field that selects the two-word tile bit-planes in cell_type() and in
    env_step's navigation -- is 1 above 64 cells and 0 at 64 (8 x 8, the largest one-word map);
  the three bit-planes (nonfloor, cell_lo, cell_hi) of every map here equal the parsed cell grid bit
    for bit, and a Cutboard / Delivery tile at dense cells 63 and 64 lands in word 0 bit 63 and word 1
    bit 0;
  blobs above 128 cells or wider / taller than 16 are refused by build_header ("level dimensions out
    of range") and by compile_level ("too large").  (129 = 3 x 43 has no factorisation within 16 x 16:
    the smallest refused cell count a 16 x 16 grid can hold is 130 = 13 x 10.)"""
import re

import numpy as np
import pytest

import big_maps as bm

W_WORD, H_WORD = 2, 3           # include/oc_level.h: OC_LV_W, OC_LV_H


def _field(text, name):
    m = re.search(r"^  (.*),  // %s$" % name, text, re.M)
    assert m, name
    return [int(v.rstrip("ul"), 16) for v in re.findall(r"0x[0-9a-f]+u(?:ll)?", m.group(1))]


def _planes(lv, geometry=True):
    from gym_comm_amd import specialize
    text = specialize.spec_header_text(lv.blob, geometry)
    return {k: _field(text, k) for k in ("nonfloor", "cell_lo", "cell_hi", "planes128", "closed_border")}


@pytest.mark.parametrize("name", sorted(bm.MAPS))
def test_planes128_is_set_above_64_cells_and_the_planes_hold_the_grid(name):
    lv = bm.level(name, 2)
    nc = lv.width * lv.height
    p = _planes(lv)
    assert p["planes128"] == [1 if nc > 64 else 0] and p["closed_border"] == [1]
    # the structure library's header carries the same two fields and none of the map
    s = _planes(lv, geometry=False)
    assert s["planes128"] == p["planes128"] and s["closed_border"] == [1]
    assert s["nonfloor"] == s["cell_lo"] == s["cell_hi"] == [0, 0]
    cells = np.asarray(lv.cells).reshape(-1)          # [y][x] -> dense y * W + x
    assert cells.size == nc
    for c in range(128):
        t = int(cells[c]) if c < nc else 0
        got = [(p[k][c >> 6] >> (c & 63)) & 1 for k in ("nonfloor", "cell_lo", "cell_hi")]
        assert got == [int(t != 0), t & 1, t >> 1], (name, c)
    if nc <= 64:
        assert p["nonfloor"][1] == p["cell_lo"][1] == p["cell_hi"][1] == 0


def test_the_64_cell_map_is_the_largest_one_word_map():
    assert bm.level("control_8x8", 2).width * bm.level("control_8x8", 2).height == 64
    assert max(lv.width * lv.height for lv in (bm.level(n, 2) for n in bm.MAPS)) == 128


@pytest.mark.parametrize("at63,at64", [("/", "*"), ("*", "/")])
def test_tiles_at_dense_cells_63_and_64_straddle_the_two_words(at63, at64):
    """8 x 9: dense cell 63 is (7, 7) on the east wall, cell 64 is (0, 8), the south-west corner."""
    from gym_comm_amd import compiler, levels
    rows = ["-t----l-", "/      -", "*      -"] + ["-      -"] * 3 + ["-      p", "-      " + at63, at64 + "------p"]
    lv = compiler.compile_level(levels.parse_level_text("straddle", "\n".join(rows) + "\n\nSalad\n\n2 1\n5 5"), 2, 100)
    assert (lv.width, lv.height) == (8, 9)
    kind = {"/": levels.CUTBOARD, "*": levels.DELIVERY}
    assert lv.cells[7][7] == kind[at63] and lv.cells[8][0] == kind[at64]
    p = _planes(lv)
    assert p["planes128"] == [1]
    for word, bit, t in ((0, 63, kind[at63]), (1, 0, kind[at64])):
        assert (p["nonfloor"][word] >> bit) & 1 == 1
        assert (p["cell_lo"][word] >> bit) & 1 == t & 1
        assert (p["cell_hi"][word] >> bit) & 1 == t >> 1 == 1


@pytest.mark.parametrize("w,h", [(13, 10), (10, 13), (17, 7), (7, 17), (43, 3)],
                         ids=["130-cells", "130-cells-tall", "17-wide", "17-tall", "129-cells"])
def test_blobs_above_the_limits_are_refused_by_build_header(w, h):
    from gym_comm_amd import _lib, specialize
    blob = bm.level("wide_16x8", 2).blob.copy()
    blob[W_WORD], blob[H_WORD] = w, h
    for geometry in (True, False):
        with pytest.raises(_lib.OcError, match="level dimensions out of range"):
            specialize.spec_header_text(blob, geometry)
    with pytest.raises(_lib.OcError, match="level dimensions out of range"):
        _lib.subtask_info(blob)


@pytest.mark.parametrize("w,h", [(13, 10), (17, 7), (7, 17)])
def test_compile_level_refuses_them_too(w, h):
    from gym_comm_amd import compiler, levels
    rows = ["-" * w] + ["-" + " " * (w - 2) + "-"] * (h - 2) + ["*" + "-" * (w - 1)]
    rows[0] = "-tp" + "-" * (w - 3)
    spec = levels.parse_level_text("over", "\n".join(rows) + "\n\nSimpleTomato\n\n1 1\n2 2")
    with pytest.raises(ValueError, match="too large"):
        compiler.compile_level(spec, 2, 100)


def test_a_map_set_refuses_to_mix_one_word_and_two_word_maps():
    """planes128 is a STRUCTURE field: the structure library of the 16 x 8 map was compiled for two-word
    planes, so the 8 x 8 map of the same recipe, items and border is not of its structure -- in either
    order, and whichever of the two libraries is asked.  (Refusals happen before any device work.)"""
    import ctypes
    from gym_comm_amd import specialize
    big, small = bm.level("wide_16x8", 2), bm.level("control_8x8", 2)
    assert specialize.spec_key(big.blob, False) != specialize.spec_key(small.blob, False)
    i32p = ctypes.POINTER(ctypes.c_int32)
    for own, other in ((big, small), (small, big)):
        path = specialize.ensure(own.blob, geometry=False, compile=False)
        assert path, "build() makes the structure library of every level tests/spec_levels.py lists"
        _, L = specialize.load_for(own.blob, "structure")
        assert L.oc_is_specialized() == 1
        blobs = [np.ascontiguousarray(m.blob, dtype=np.int32) for m in (own, other)]
        ptrs = (i32p * 2)(*[b.ctypes.data_as(i32p) for b in blobs])
        sizes = np.array([b.size for b in blobs], np.int32)
        h = ctypes.c_void_p()
        rc = L.oc_mapset_create(ptrs, sizes.ctypes.data_as(i32p), 2, ctypes.byref(h))
        msg = L._oc_last_error().decode()
        assert rc == -1 and not h.value and "blob 1" in msg and "structure" in msg, msg
