"""Scale labels: text, without a GPU: the structs' layout against a C program compiled from the header; every case's expectation
(tests/label_text_cases.py) on the restatement (tests/label_text_ref.py); copies of the restatement with one rule changed, each of
which some case notices; the host helpers smhv_glyph_templates_from_label and smhv_glyph_templates_check against the restatement
and every invalid template form; and csrc/smh_glyph_rule.h compiled into a stand-alone program (tests/glyph_rule_check.cpp, with
-fsanitize=address,undefined where the host compiler links it) whose records equal the restatement's byte for byte."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import label_text_cases as LC
import label_text_ref as LT
import scale_label_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "squad-mortar-helper_amd", "csrc")


@pytest.fixture(scope="module")
def smh(built):
    import squad_mortar_helper_amd
    return squad_mortar_helper_amd


@pytest.fixture(scope="module")
def frames(built):
    """[(case, want, the restatement's frame)]"""
    return [(c, LC.want_of(c), LT.read_frame(LC.want_of(c), c["atlas"])) for c in LC.cases()]


def test_struct_layouts_and_constants_against_the_header(smh, tmp_path):
    from squad_mortar_helper_amd import _lib as L
    fields = {"smhv_glyph_template": (L.GlyphTemplate, ["code", "w", "h", "reserved", "rows"]),
              "smhv_glyph_atlas_options": (L.GlyphAtlasOptions, ["accept_num", "accept_den"]),
              "smhv_label_text_entry": (L.LabelTextEntry, ["text", "n_glyphs", "flags", "meters", "reserved", "best", "second", "tmpl"]),
              "smhv_label_text_frame": (L.LabelTextFrame, ["n", "has", "mpx", "anchors", "reserved", "label"])}
    body = "".join("  Z(%s);\n" % t + "".join("  O(%s, %s);\n" % (t, f) for f in fs) for t, (_, fs) in fields.items())
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "smh_vision_hip.h"\n'
                   '#define O(t, f) printf(#t "." #f " %zu\\n", offsetof(t, f))\n'
                   '#define Z(t) printf(#t " %zu\\n", sizeof(t))\n'
                   'int main(void) {\n' + body +
                   '  printf("consts %u %u %u\\n", SMHV_LABEL_MAX_GLYPHS, SMHV_ATLAS_MAX_TEMPLATES, SMHV_LABEL_TEXT_TOO_MANY);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(ln.rsplit(" ", 1) if not ln.startswith("consts") else ("consts", ln[7:]) for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    for t, (cls, fs) in fields.items():
        assert int(got[t]) == C.sizeof(cls), t
        for f in fs:
            assert int(got["%s.%s" % (t, f)]) == getattr(cls, f).offset, (t, f)
    assert (int(got["smhv_glyph_template"]), int(got["smhv_label_text_entry"]), int(got["smhv_label_text_frame"])) == (132, LT.ENTRY_BYTES, LT.REC_BYTES)
    assert got["consts"].split() == [str(v) for v in (L.LABEL_MAX_GLYPHS, L.ATLAS_MAX_TEMPLATES, L.LABEL_TEXT_TOO_MANY)]
    assert (LT.MAX_GLYPHS, LT.MAX_TEMPLATES, LT.TOO_MANY, LT.MAX_LABELS, LT.MAX_SCALES) == (L.LABEL_MAX_GLYPHS, L.ATLAS_MAX_TEMPLATES, L.LABEL_TEXT_TOO_MANY,
                                                                                           L.MAX_SCALE_LABELS, L.MAX_SCALES)


def test_every_expectation_on_the_restatement(frames):
    names = [c["name"] for c, _, _ in frames]
    assert len(set(names)) == len(names) >= 45
    for c, want, fr in frames:
        if "boxes" in c["expect"]:                             # the painted labels are the words the scale-label rule finds
            assert [lb[:4] for lb in want["labels"]] == c["expect"]["boxes"], c["name"]
        LC.check_expect(c, fr)
        assert len(LT.pack_frame(fr)) == LT.REC_BYTES
    closed = next(fr for c, _, fr in frames if c["name"] == "frame_closed")
    over = next((want, fr) for c, want, fr in frames if c["name"] == "frame_runs_overflow")
    assert LT.pack_frame(closed) == bytes(LT.REC_BYTES) == LT.pack_frame(over[1]) and over[0]["header"][4] == 1
    # the ladder case's mean does depend on the order of its sum
    lad = next(fr for c, _, fr in frames if c["name"] == "frame_ladder_order")
    want = next(w for c, w, _ in frames if c["name"] == "frame_ladder_order")
    r = [float(m) / float(lb[6] - lb[4]) for m, lb in zip((100, 300, 900), want["labels"])]
    assert lad["mpx"] == ((r[0] + r[1]) + r[2]) / 3.0 != ((r[2] + r[1]) + r[0]) / 3.0


def test_text_to_meters_is_the_label_filter_of_the_scales_branch(smh):
    texts = ["33m", "100m", "2700m", "4294967295m", "4294967296m", "m", "0m", "007m", "+5m", "300", "3m0m", "30m0", "+m", "++5m", "+0m", "5+m", "?00m", "3?m",
             "99999999999999m", "mm", "m5m", "5mm", "", "0", "12m3m", "-5m", " 5m", "5 m"]
    for t in texts:
        hits = smh.parse_ocr_labels([dict(text=t, left=0, right=10, bottom=5)])[0]
        assert LT.meters_of(t) == (hits[0][0] if hits else 0), t
    assert [LT.meters_of(t) for t in texts[:12]] == [33, 100, 2700, 4294967295, 0, 0, 0, 7, 5, 0, 0, 30]


def test_the_frame_rule_is_the_host_function(smh, frames):
    """anchors_of against smhv_scale_labels_anchors (the header's one text of the rule, run on the host) and parse_ocr_labels."""
    from squad_mortar_helper_amd import _lib as L
    some = 0
    for c, want, fr in frames:
        if not fr["n"]:
            continue
        labels = [L.ScaleLabel(*lb) for lb in want["labels"]]
        an, mpx = smh.scale_labels_anchors(labels, [lb["meters"] for lb in fr["labels"]])
        assert (an.n, an.scales_start_y, [tuple(an.scales[k]) for k in range(an.n)]) == (len(fr["scales"]), fr["start_y"], fr["scales"]), c["name"]
        assert (mpx is not None) == bool(fr["has"]) and (mpx or 0.0) == fr["mpx"], c["name"]
        scales, start_y = smh.parse_ocr_labels(smh.scale_label_hits(labels, [lb["text"] for lb in fr["labels"]]))
        assert (scales, start_y or 0) == (fr["scales"], fr["start_y"]), c["name"]
        some += bool(fr["has"])
    assert some >= 25


@pytest.mark.parametrize("field,value", [("shifts", False), ("tie_low", False), ("accept_on", "glyph"), ("find", "find"), ("brk", False)])
def test_a_changed_rule_is_noticed(frames, field, value):
    rule = LT.RULE._replace(**{field: value})
    differing = [c["name"] for c, want, fr in frames if LT.pack_frame(LT.read_frame(want, c["atlas"], rule)) != LT.pack_frame(fr)]
    assert differing, field


def _same_templates(got, want):
    assert len(got) == len(want)
    for t, (code, b) in zip(got, want):
        assert (chr(t.code), t.w, t.h, t.reserved, list(t.rows)) == (code, b.shape[1], b.shape[0], 0, LT.template_rows(b))


def test_learning_helper_against_the_restatement(smh, frames):
    from squad_mortar_helper_amd import _lib as L
    done = 0
    for c, want, fr in frames:
        truth = c["expect"].get("truth") or c["expect"].get("texts")
        if not fr["n"] or c["name"] in ("glyphs_17", "run_of_33_columns") or c["name"].startswith(("shift_two", "accept_", "strip_glorious_by")):
            continue
        for cell, box, text, lb in zip(want["crops"], want["labels"], truth, fr["labels"]):
            text = text.replace("?", "x")                      # ('?' is no code: any other character will do for a glyph nobody reads)
            if len(text) != lb["n_glyphs"]:
                continue
            _same_templates(smh.glyph_templates_from_label(cell, box, text), LT.learn(cell, box, text))
            smh.glyph_templates_check(smh.glyph_templates_from_label(cell, box, text))
            done += 1
    assert done >= 40
    # the atlas of a strip, learned label by label and without duplicates, is the restatement's
    want = LC.want_of(LC.by_name("strip_glorious_by_albasrah_png"))
    texts = SC.STRIPS["glorious_png"]["texts"]
    got = smh.glyphs.learn_templates(zip(want["crops"], want["labels"], texts))
    _same_templates(got, LC.strip_atlas("glorious_png").templates)
    assert sorted({chr(t.code) for t in got}) == ["0", "1", "3", "9", "m"]
    # what the helper refuses: a wrong glyph count, a glyph wider than 32 columns, a character that is no code
    cell, box = want["crops"][0], want["labels"][0]
    wide = LC.want_of(LC.by_name("run_of_33_columns"))
    many = LC.want_of(LC.by_name("glyphs_17"))
    for args in ((cell, box, "100"), (cell, box, "100mm"), (cell, box, ""), (cell, box, "10?m"), (cell, box, "10 m"), (cell, box, "10\x7fm"), (cell, box, "10\xe9m"),
                 (wide["crops"][0], wide["labels"][0], "Wm"), (many["crops"][0], many["labels"][0], "0" * 17), (cell, (0, 0, 129, 10), "100m"),
                 (cell, (0, 0, 10, 33), "100m"), (cell, (5, 0, 5, 10), "100m")):
        with pytest.raises(smh.VisionError) as ei:
            smh.glyph_templates_from_label(*args)
        assert ei.value.code == L.E_INVALID, args[2]
    assert LT.learn(cell, box, "100") is None and LT.learn(cell, box, "10?m") is None and LT.learn(wide["crops"][0], wide["labels"][0], "Wm") is None


def test_templates_check_refuses_every_invalid_form(smh):
    from squad_mortar_helper_amd import _lib as L
    good = LC.lib_templates(LC.FONT12)
    smh.glyph_templates_check(good)
    smh.glyph_templates_check(good + good[:8])                   # 32 templates, codes shared

    def variant(**kw):
        t = L.GlyphTemplate()
        C.memmove(C.addressof(t), C.addressof(good[0]), C.sizeof(t))     # '0' at scale 1: 5 x 7
        for k, v in kw.items():
            if k == "rows":
                for y, r in v.items():
                    t.rows[y] = r
            else:
                setattr(t, k, v)
        return t
    bad = dict(code_space=variant(code=0x20), code_del=variant(code=0x7F), code_question=variant(code=ord("?")), code_high=variant(code=0xE9), code_0=variant(code=0),
               w_0=variant(w=0), w_33=variant(w=33), h_0=variant(h=0), h_33=variant(h=33), reserved=variant(reserved=1),
               empty_first_row=variant(rows={0: 0}), empty_last_row=variant(rows={6: 0}), empty_first_column=variant(rows={y: good[0].rows[y] & ~1 for y in range(7)}),
               empty_last_column=variant(rows={y: good[0].rows[y] & ~16 for y in range(7)}), bit_right_of_the_box=variant(rows={3: good[0].rows[3] | 32}),
               bit_below_the_box=variant(rows={7: 1}), bit_in_the_last_row=variant(rows={31: 1}), narrower_than_its_bits=variant(w=4), lower_than_its_bits=variant(h=6))
    for name, t in bad.items():
        for lst in ([t], good[:3] + [t]):
            with pytest.raises(smh.VisionError) as ei:
                smh.glyph_templates_check(lst)
            assert ei.value.code == L.E_INVALID, name
    for lst in ([], good + good[:9]):
        with pytest.raises(smh.VisionError) as ei:
            smh.glyph_templates_check(lst)
        assert ei.value.code == L.E_INVALID
    full = variant(w=32, h=32, rows={y: 0xFFFFFFFF for y in range(32)})      # the largest template there is
    smh.glyph_templates_check([full, variant(w=1, h=1, rows={0: 1, 1: 0, 2: 0, 3: 0, 4: 0, 5: 0, 6: 0})])


def test_the_header_as_a_stand_alone_program(frames, tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "glyph_rule_check")
    base = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "glyph_rule_check.cpp"), "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    if san.returncode != 0:                                    # (a host without the sanitizers' runtimes: the plain program)
        subprocess.run(base, check=True, capture_output=True, text=True)
    blob = struct.pack("<I", len(frames))
    for c, want, _ in frames:
        tpl = LC.lib_templates(c["atlas"])
        rec, cells = LC.label_frame_bytes(want)
        blob += struct.pack("<4I", len(tpl), c["atlas"].num, c["atlas"].den, 0) + b"".join(bytes(t) for t in tpl) + rec + cells
    (tmp_path / "in.bin").write_bytes(blob)
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok: %d frames" % len(frames)), (r.returncode, r.stdout[-400:], r.stderr[-3000:])
    got = (tmp_path / "out.bin").read_bytes()
    assert len(got) == LT.REC_BYTES * len(frames)
    for i, (c, _, fr) in enumerate(frames):
        assert got[i * LT.REC_BYTES:(i + 1) * LT.REC_BYTES] == LT.pack_frame(fr), c["name"]
