"""The map grid without a GPU: the structs' layout against the header, the exported symbols, the library's defaults, the Python
options, strings typed out by hand, what the entry points refuse before they ask for a device, the cases' own assertions on the
restatement (tests/grid_ref.py), the restatement against itself with one rule changed at a time, and csrc/smh_grid.h compiled into a
stand-alone program (tests/grid_rule_check.cpp, with -fsanitize=address,undefined where the host compiler links it) whose indices,
digits and strings equal the restatement's."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import grid_cases as GC
import grid_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "squad-mortar-helper_amd", "csrc")
SYMBOLS = ("smhv_grid_defaults", "smhv_grid_ref_text", "smhv_batch_grid", "smhv_batch_read_grid", "smhv_batch_grid_ptr", "smhv_grid_map",
           "smhv_batch_grid_refs", "smhv_batch_read_grid_refs", "smhv_batch_grid_refs_ptr", "smhv_grid_refs")
# the rule changed -> the family whose cases must notice
MUTANTS = {"ceil": "ceil", "top123": "top123", "per_level": "per_level", "trunc": "trunc", "finest": "ceil", "window": "window"}


def test_struct_layouts_and_constants_against_the_header(built, tmp_path):
    from squad_mortar_helper_amd import _lib as L
    fields = {"smhv_grid_options": (L.GridOptionsStruct, 80), "smhv_grid_result": (L.GridResult, 64), "smhv_grid_planes": (L.GridPlanes, 16),
              "smhv_grid_ref": (L.GridRef, 48), "smhv_grid_refs_result": (L.GridRefsResult, 3088)}
    body = "".join('  Z(%s);\n' % t + "".join('  O(%s, %s);\n' % (t, f) for f, _ in cls._fields_) for t, (cls, _) in fields.items())
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smh_vision_hip.h"\n'
                   '#define O(t, f) printf(#t "." #f " %zu\\n", offsetof(t, f))\n'
                   '#define Z(t) printf(#t " %zu\\n", sizeof(t))\n'
                   'int main(void) {\n' + body +
                   '  printf("consts %u %u %u %u %u %u %u %u %u %u\\n", SMHV_GRID_PAINT, SMHV_GRID_BYTES, SMHV_GRID_CELLS, SMHV_GRID_HAS_CELL, SMHV_GRID_LABEL,\n'
                   '         SMHV_GRID_NONE, SMHV_GRID_SCALES, SMHV_GRID_HEIGHTMAP, SMHV_GRID_MAX_COLS, SMHV_GRID_MAX_ROWS);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(ln.rsplit(" ", 1) if not ln.startswith("consts") else ("consts", ln[7:]) for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    for t, (cls, size) in fields.items():
        assert int(got[t]) == C.sizeof(cls) == size, t               # the sizes the header states
        for f, _ in cls._fields_:
            assert int(got["%s.%s" % (t, f)]) == getattr(cls, f).offset, (t, f)
    assert L.GridRef.text.offset == 32 and L.GridRef.valid.offset == 27 and L.GridRefsResult.ref.offset == 16 and L.GridOptionsStruct.line.offset == 56
    assert [int(v) for v in got["consts"].split()] == [L.GRID_PAINT, L.GRID_BYTES, L.GRID_CELLS, L.GRID_HAS_CELL, L.GRID_LABEL, L.GRID_NONE, L.GRID_SCALES,
                                                        L.GRID_HEIGHTMAP, G.MAX_COLS, G.MAX_ROWS] == [1, 2, 4, 1, 16, 0, 1, 2, 702, 999]
    assert (G.PAINT, G.BYTES, G.CELLS, G.HAS_CELL, G.LABEL, G.NONE, G.SCALES, G.HEIGHTMAP) == (1, 2, 4, 1, 16, 0, 1, 2)


def test_symbols_defaults_and_the_python_options(built):
    import squad_mortar_helper_amd as smh
    L = smh._lib
    lib = L.load()
    for name in SYMBOLS:
        assert getattr(lib, name) is not None, name
    o = L.GridOptionsStruct()
    C.memset(C.byref(o), 0xA5, C.sizeof(o))
    assert lib.smhv_grid_defaults(C.byref(o)) == 0 and lib.smhv_grid_defaults(None) == L.E_INVALID
    got = dict(cell_m=o.cell_m, levels=o.levels, origin_m=tuple(o.origin_m), min_px=o.min_px, label_min_px=o.label_min_px,
               line=tuple(tuple(k) for k in o.line), label=tuple(o.label))
    assert got == G.DEFAULTS and (o.size, o.flags, o.reserved0, o.reserved) == (80, L.GRID_PAINT, 0, 0)
    assert bytes(smh.GridOptions().struct()) == bytes(o)
    p = smh.GridOptions(cell_m=100, levels=3, origin_m=(1.5, -2), min_px=0, label_min_px=7, paint=False, bytes=True, cells=True, line=GC.LINE, label=GC.LABEL).struct()
    assert (p.flags, p.cell_m, p.levels, tuple(p.origin_m), p.min_px, p.label_min_px) == (L.GRID_BYTES | L.GRID_CELLS, 100.0, 3, (1.5, -2.0), 0.0, 7.0)
    assert tuple(tuple(k) for k in p.line) == GC.LINE and tuple(p.label) == GC.LABEL


def test_strings_typed_out_by_hand(built):
    import squad_mortar_helper_amd as smh
    L = smh._lib
    lib = L.load()
    want = {(0, 1, ()): "A1", (1, 4, (7, 3)): "B4-7-3", (25, 9, ()): "Z9", (26, 10, (5,)): "AA10-5", (27, 99, ()): "AB99", (51, 100, ()): "AZ100",
            (52, 1, ()): "BA1", (700, 998, (1, 2, 3)): "ZY998-1-2-3", (701, 999, (9, 9, 9)): "ZZ999-9-9-9", (18, 12, (1, 9)): "S12-1-9"}
    for (col, row1, digits), text in want.items():
        assert smh.grid_ref_text(col, row1, digits) == text == G.ref_text(col, row1, digits), (col, row1, digits)
    assert max(len(t) for t in want.values()) == 11
    out = C.create_string_buffer(b"\x55" * 16, 16)
    d = (C.c_uint8 * 3)(7, 3, 1)
    assert lib.smhv_grid_ref_text(1, 4, d, 2, out) == 0 and out.raw == b"B4-7-3" + bytes(10)          # NUL-padded to 16
    assert lib.smhv_grid_ref_text(0, 1, None, 0, out) == 0 and out.raw == b"A1" + bytes(14)
    for col, row1, digits, levels in ((702, 1, d, 0), (0, 0, d, 0), (0, 1000, d, 0), (0, 1, d, 4), (0, 1, None, 1), (0, 1, (C.c_uint8 * 3)(0, 1, 1), 1),
                                      (0, 1, (C.c_uint8 * 3)(1, 10, 1), 2)):
        assert lib.smhv_grid_ref_text(col, row1, digits, levels, out) == L.E_INVALID, (col, row1, levels)
    assert lib.smhv_grid_ref_text(0, 1, d, 0, None) == L.E_INVALID
    assert [G.letters(c) for c in (0, 25, 26, 51, 52, 701)] == ["A", "Z", "AA", "AZ", "BA", "ZZ"]


def test_null_handles_are_refused_before_a_device_is_asked(built):
    import squad_mortar_helper_amd as smh
    L = smh._lib
    lib = L.load()
    o = smh.GridOptions().struct()
    assert lib.smhv_batch_grid(None, 0, 1, None, None, C.byref(o), None, None) == L.E_INVALID
    assert lib.smhv_batch_grid_refs(None, 0, 1, None, None, C.byref(o), None) == L.E_INVALID
    assert lib.smhv_grid_map(None, None, None, C.byref(o), None, None, None, None, None, None) == L.E_INVALID
    assert lib.smhv_grid_refs(None, None, 0, None, None, None, None, C.byref(o), None) == L.E_INVALID
    assert lib.smhv_batch_read_grid(None, 0, 1, None) == L.E_INVALID and lib.smhv_batch_grid_ptr(None, None) == L.E_INVALID
    assert lib.smhv_batch_read_grid_refs(None, 0, 1, None) == L.E_INVALID and lib.smhv_batch_grid_refs_ptr(None, None) == L.E_INVALID


@pytest.mark.parametrize("case", GC.all_cases(), ids=lambda c: c.name)
def test_every_case_contains_what_it_is_for(built, case):
    r, refs = GC.checked(case)
    s = G.summary(r)
    b = r["bytes"]
    assert s["n_cell"] >= sum(s["n_line"]) and s["n_cell"] >= s["n_label"]
    assert not (b[(b & G.HAS_CELL) == 0]).any() and not r["cells"][(b & G.HAS_CELL) == 0].any()
    assert len(refs[1]) == 2 * len(case.lines)


def _same(a, b, ra, rb):
    return np.array_equal(a["bytes"], b["bytes"]) and np.array_equal(a["cells"], b["cells"]) and ra == rb


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_a_changed_rule_is_noticed_by_its_family(built, mutant):
    cases = GC.family(MUTANTS[mutant])
    assert cases
    for c in cases:
        assert not _same(GC.restate(c), GC.restate(c, mutant), GC.restate_refs(c), GC.restate_refs(c, mutant)), (mutant, c.name)


def test_the_families_cover_the_issue(built):
    names = [c.name for c in GC.all_cases()]
    assert {c.family for c in GC.all_cases()} >= set(MUTANTS.values()) | {"letters", "ld", "labels", "source", "ends"}
    assert sum(n.startswith("min_px") for n in names) == 12 and sum(n.startswith("label_min_px") for n in names) == 3
    assert {GC.restate(c)["ld"] for c in GC.family("ld")} == {-1, 0, 1, 2, 3}


def _job(c):
    """A case as a job of grid_rule_check -> (bytes in, [the expected records]) or None when the frame has no grid."""
    source, ax, ay = G.frame(c.viewport, c.minimap, c.hm, c.fit, c.mpx, c.opt)
    if source == G.NONE:
        return None
    ow, oh = c.window
    sw, sh, tx, ty = (np.float32(v) for v in (c.viewport or (1.0, 1.0, 0.0, 0.0)))
    pts = [(np.float32(min(i, ow)) + np.float32(0.5), np.float32(min(i, oh)) + np.float32(0.5), min(i, ow), min(i, oh)) for i in range(max(ow, oh) + 1)]
    with np.errstate(all="ignore"):
        for x0, y0, x1, y1 in c.lines:
            for x, y in ((x0, y0), (x1, y1)):
                pts.append((np.float32(np.float32(x * sw) + tx), np.float32(np.float32(y * sh) + ty), -2 ** 31, -2 ** 31))
    H, W = c.hm[0].shape if c.hm else (0, 0)
    blob = struct.pack("<6d6f2I4I", float(c.mpx) if c.mpx is not None else 0.0, c.opt["origin_m"][0], c.opt["origin_m"][1], c.opt["cell_m"], c.opt["min_px"],
                       c.opt["label_min_px"], ax["r0"], ay["r0"], ax["r1"], ay["r1"], sw, sh, W, H, int(source == G.SCALES), c.opt["levels"], c.opt["label"][3], len(pts))
    blob += b"".join(struct.pack("<2f2i", *p) for p in pts)
    ld = G.drawn_levels(ax, ay, c.opt)
    want = [struct.pack("<iI", ld, int(G.labels_drawn(ax, ay, ld, c.opt)))]
    ex, ey = G.entries(ax, np.arange(ow + 2).astype(np.float32) + np.float32(0.5)), G.entries(ay, np.arange(oh + 2).astype(np.float32) + np.float32(0.5))
    first = (G._first(ax, ow + 1, ex["idx"][0], None), G._first(ay, oh + 1, ey["idx"][0], None))
    L = c.opt["levels"]
    cross = [G._cross([i[:-1] for i in e["idx"]], [i[1:] for i in e["idx"]], e["has"][:-1] & e["has"][1:], ld, None) for e in (ex, ey)]
    for x, y, X, Y in pts:
        p = G.point_ref(ax, ay, x, y)
        rec = struct.pack("<ddII3BBI16s", p["x_m"], p["y_m"], p["col"], p["row1"], *p["digit"], p["valid"], 0, p["text"])
        e = (G.entries(ax, [x]), G.entries(ay, [y]))
        flags = sum((int(e[k]["inn"][0]) | int(e[k]["has"][0]) << 1) << (2 * k) for k in range(2))
        pix = X != -2 ** 31
        fs = [int(first[k][P]) if pix and e[k]["has"][0] else 0 for k, P in ((0, X), (1, Y))]
        cr = [int(cross[k][P]) if pix and e[k]["has"][0] else 4 for k, P in ((0, X), (1, Y))]
        want.append(rec + struct.pack("<2iI2i2II", int(e[0]["idx"][L][0]), int(e[1]["idx"][L][0]), flags, fs[0], fs[1], cr[0], cr[1], 0))
    return blob, want


def test_the_header_as_a_stand_alone_program(built, tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "grid_rule_check")
    base = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "grid_rule_check.cpp"), "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    if san.returncode != 0:                                    # (a host without the sanitizers' runtimes: the plain program)
        subprocess.run(base, check=True, capture_output=True, text=True)
    jobs = [(c, _job(c)) for c in GC.all_cases()]
    jobs = [(c, j) for c, j in jobs if j is not None]
    assert len(jobs) >= 30
    (tmp_path / "in.bin").write_bytes(struct.pack("<I", len(jobs)) + b"".join(j[0] for _, j in jobs))
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok: %d jobs" % len(jobs)), (r.returncode, r.stdout[-400:], r.stderr[-3000:])
    got = (tmp_path / "out.bin").read_bytes()
    at = 0
    for c, (_, want) in jobs:
        for i, w in enumerate(want):
            assert got[at:at + len(w)] == w, (c.name, i, got[at:at + len(w)].hex(), w.hex())
            at += len(w)
    assert at == len(got)
