"""Person labels without a GPU: ``hrn_label_layout`` / ``hrn_label_covers`` -- the text the kernels compile, csrc/draw_labels_math.h --
against the numpy restatement of the definition (tests/label_ref.py) over whole small canvases, the glyphs against the header's
table bit for bit, the percent arithmetic against the same two float32 operations in numpy, the declarations, every refusal with
its message, and the same cases walked by a stand-alone C++ program under AddressSanitizer and UBSan (a child process of its own;
nothing is preloaded into Python)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import label_ref
from conftest import load_pkg
from draw_ref import grid

H, W = 64, 96          # the window every case is compared on
F32 = np.float32
IDS = [0, 7, 10, 99, 100, 2147483647, -1]
SCORES = [np.nan, -0.5, 0.0, np.nextafter(F32(0.005), F32(-1)), F32(0.005), np.nextafter(F32(0.005), F32(1)), 0.995, 1.0, 7.0]
SCALES = [1, 2, 3, 16]
THICKNESSES = [0, 1, 2, 16]
# the header's table, typed again: rows top to bottom, bit 4 = the leftmost column
TABLE = """
0: 0E 11 13 15 19 11 0E    5: 1F 10 1E 01 01 11 0E
1: 04 0C 04 04 04 04 0E    6: 06 08 10 1E 11 11 0E
2: 0E 11 01 02 04 08 1F    7: 1F 01 02 04 08 08 08
3: 1F 02 04 02 01 11 0E    8: 0E 11 11 0E 11 11 0E
4: 02 06 0A 12 1F 02 02    9: 0E 11 11 0F 01 02 0C
"""


def case(box, pid=None, score=None, s=1, T=2, window=(0, 0)):
    return dict(box=tuple(int(v) for v in box), pid=pid, score=score, s=s, T=T, window=window)


def cases():
    out = [case((20, 30, 80, 60), pid=i) for i in IDS]
    out += [case((20, 30, 80, 60), pid=7, score=v) for v in SCORES] + [case((20, 30, 80, 60), score=v) for v in SCORES]
    out += [case((5, 5 + 9 * s, 90, 60), pid=10, score=0.5, s=s, T=T) for s in SCALES for T in THICKNESSES]
    out += [case((20, 30, 80, 60))]                                                        # neither id nor score: outline only
    out += [case((20, 30, 80, 60), pid=-1), case((20, 30, 80, 60), pid=-1, score=0.25)]    # a negative id prints nothing
    out += [case((30, 20, 33, 50), pid=3, T=2), case((30, 20, 60, 22), T=16), case((30, 20, 31, 21), T=1)]   # narrower than 2 T: filled
    for s in SCALES:                                                                       # the plate inside (y1 = 9 s - 1) and above (9 s)
        out += [case((10, 9 * s - 1, 70, 9 * s + 40), pid=42, s=s), case((10, 9 * s, 70, 9 * s + 40), pid=42, s=s)]
    out += [case((-8192, -8192, 16383, 16383), pid=1, T=16), case((-8192, 10, 40, 16383), pid=1, score=1.0),
            case((-8193, 10, 40, 50), pid=1), case((10, -8193, 40, 50), pid=1), case((10, 10, 16384, 50), pid=1), case((10, 10, 40, 16384), pid=1),
            case((40, 10, 40, 50), pid=1), case((10, 50, 40, 50), pid=1), case((41, 10, 40, 50), pid=1), case((0, 0, 0, 0), pid=1, score=0.9)]
    # 14 cells at the largest scale, 1360 pixels wide: the window moved along it; and a window off the canvas's origin
    out += [case((0, 200, 1500, 400), pid=2147483647, score=1.0, s=16, window=(x, 56 + 20 * k)) for k, x in enumerate((0, 90, 700, 1290))]
    out += [case((-50, -40, 30, 20), pid=5, score=0.3, s=2, window=(-60, -50)), case((16300, 16300, 16383, 16383), pid=8, window=(16290, 16280))]
    return out


def ref_classes(c):
    """(H, W) of 0 / 1 / 2 from the restatement's masks, painted in primitive order"""
    px, py = grid(H, W)
    px, py = px + c["window"][0], py + c["window"][1]
    cls = np.zeros((H, W), np.int64)
    for mask, kind in label_ref.person_primitives(px, py, c["box"], c["pid"], c["score"], c["s"], c["T"]):
        cls[mask] = kind
    return cls


def lib_classes(post, lib, rec, window):
    fn = lib.hrn_label_covers
    ref = ctypes.byref(rec)
    return np.asarray([[fn(ref, window[0] + x, window[1] + y) for x in range(W)] for y in range(H)], np.int64)


def test_layout_and_covers_equal_the_restatement():
    post, lib = load_pkg("postproc"), load_pkg("_lib").load()
    seen = set()
    for c in cases():
        rec = post.label_layout(c["box"], c["pid"], c["score"], c["s"], c["T"])
        assert rec.colour == 0 and rec.text_colour == 0
        drawn = label_ref.is_drawn(c["box"])
        assert rec.drawn == int(drawn), c
        if not drawn:
            assert bytes(rec) == bytes(64), c                                       # every other field is 0
        else:
            row = label_ref.cells(c["pid"], c["score"])
            assert (rec.x1, rec.y1, rec.x2, rec.y2, rec.thickness, rec.scale, rec.ncells) == c["box"] + (c["T"], c["s"], len(row)), c
            packed = rec.cells_lo | (rec.cells_hi << 32)
            assert [(packed >> (4 * k)) & 15 for k in range(len(row))] == [15 if d is None else d for d in row] and packed >> (4 * len(row)) == 0, c
            want = label_ref.plate_rect(c["box"], len(row), c["s"]) if row else (0, 0, 0, 0)
            assert (rec.left, rec.top, rec.width, rec.height) == want, c
        got, want = lib_classes(post, lib, rec, c["window"]), ref_classes(c)
        np.testing.assert_array_equal(got, want, err_msg=str(c))
        seen |= set(np.unique(want).tolist())
    assert seen == {0, 1, 2}
    assert post.label_covers(post.label_layout((2, 20, 40, 50), 8), 4, 12) == 2 and post.label_covers(post.label_layout((2, 20, 40, 50), 8), 2, 11) == 1


def test_glyphs_are_the_table_bit_for_bit():
    post = load_pkg("postproc")
    table = {int(d): [int(b, 16) for b in row.split()] for d, row in re.findall(r"(\d): ((?:[0-9A-F]{2} ?){7})", TABLE)}
    assert sorted(table) == list(range(10)) and table == label_ref.GLYPHS
    for d in range(10):
        rec = post.label_layout((3, 20, 60, 50), d, None, 1, 0)                 # plate at (3, 11), the glyph's dots from (4, 12)
        assert (rec.left, rec.top, rec.width, rec.height, rec.ncells) == (3, 11, 7, 9, 1)
        rows = [sum((post.label_covers(rec, 4 + col, 12 + r) == 2) << (4 - col) for col in range(5)) for r in range(7)]
        assert rows == table[d], (d, [hex(v) for v in rows])
        frame = [[post.label_covers(rec, 3 + x, 11 + y) for x in range(7)] for y in range(9)]
        assert frame[0] == [1] * 7 and frame[8] == [1] * 7 and all(r[0] == 1 and r[6] == 1 for r in frame)     # the plate's margin


def test_percent_is_two_float32_operations():
    post = load_pkg("postproc")
    more = [0.004999, 0.015, 0.125, 0.135, 0.5, 0.994999, 0.99499995, 0.99999994, np.inf, -np.inf, -0.0, 1e-30, 0.095, 0.105]
    neighbours = [np.nextafter(F32(k / 200), F32(side)) for k in range(1, 200, 2) for side in (-1, 2)] + [F32(k / 200) for k in range(1, 200, 2)]
    for v in SCORES + more + neighbours:
        rec = post.label_layout((10, 30, 60, 60), None, v, 1, 0)
        p = None if np.isnan(F32(v)) else int(F32(F32(min(max(F32(v), F32(0)), F32(1))) * F32(100.0)) + F32(0.5))      # each result rounded to float32
        assert p == label_ref.percent(v)
        if p is None:
            assert rec.ncells == 0 and rec.width == 0
            continue
        assert 0 <= p <= 100
        packed = rec.cells_lo | (rec.cells_hi << 32)
        assert "".join(str((packed >> (4 * k)) & 15) for k in range(rec.ncells)) == str(p), (float(v), p)
    assert [label_ref.percent(v) for v in SCORES] == [None, 0, 0, 0, 1, 1, 100, 100, 100]      # 0.005f * 100 rounds to 0.5f, its lower neighbour's product stays below


def test_symbols_are_declared_and_exported():
    lib = load_pkg("_lib")
    names = {"hrn_label_layout", "hrn_label_covers", "hrn_draw_labels_dev", "hrn_label_last_error"}
    assert names <= set(lib.header_symbols()) and names <= set(lib.SYMBOLS)
    assert set(lib.header_symbols()) == set(lib.SYMBOLS)
    assert os.path.exists(os.path.join(lib.CSRC, "draw_labels_math.h")) and "draw.hip" in lib.SOURCES
    L = lib.load()
    for name in names:
        assert hasattr(L, name)
    text = open(os.path.join(lib.INCLUDE, "hrnet_mi355.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    fields = re.search(r"typedef struct \{([^}]*)\} hrn_label_record;", bare).group(1)
    assert re.findall(r"(\w+)\s*[,;]", fields) == [f[0] for f in lib.LabelRecordC._fields_]
    assert ctypes.sizeof(lib.LabelRecordC) == 64
    for row in TABLE.strip().splitlines():                  # the definition stands where the contract is
        assert row.strip() in text
    assert L.hrn_draw_labels_dev(None, None, 0, None, None, None, 1, 0, None, None, None, 1, 0, 2, None) == 1   # no handle
    draw = open(os.path.join(lib.CSRC, "draw.hip")).read()
    assert "label_raster_kernel" in draw and "label_build_kernel" in draw and '#include "draw_labels_math.h"' in draw


def test_host_refusals():
    lib = load_pkg("_lib")
    post, L = load_pkg("postproc"), lib.load()
    box = np.asarray([1, 2, 30, 40], np.int32)
    rec = lib.LabelRecordC()
    refused = [((None, 1, 3, 0, 0.0, 1, 2, ctypes.byref(rec)), "null box / record"), ((box.ctypes.data, 1, 3, 0, 0.0, 1, 2, None), "null box / record"),
               ((box.ctypes.data, 1, 3, 0, 0.0, 0, 2, ctypes.byref(rec)), "scale must be in [1, 16]"),
               ((box.ctypes.data, 1, 3, 0, 0.0, 17, 2, ctypes.byref(rec)), "scale must be in [1, 16]"),
               ((box.ctypes.data, 1, 3, 0, 0.0, 1, -1, ctypes.byref(rec)), "thickness must be in [0, 16]"),
               ((box.ctypes.data, 1, 3, 0, 0.0, 1, 17, ctypes.byref(rec)), "thickness must be in [0, 16]")]
    for args, text in refused:
        assert L.hrn_label_layout(*args) == 7 and L.hrn_label_last_error().decode() == text, text
    assert L.hrn_label_layout(box.ctypes.data, 1, 3, 0, 0.0, 16, 16, ctypes.byref(rec)) == 0 and L.hrn_label_last_error() == b""
    assert L.hrn_label_covers(None, 0, 0) == 7 and L.hrn_label_last_error() == b"null record"
    for field, value in (("scale", 0), ("scale", 17), ("thickness", 17), ("ncells", 15), ("ncells", -1)):
        bad = post.label_layout(box, 3)
        setattr(bad, field, value)
        assert L.hrn_label_covers(ctypes.byref(bad), 0, 0) == 7 and b"not one hrn_label_layout wrote" in L.hrn_label_last_error(), field
        with pytest.raises(ValueError, match="not one hrn_label_layout wrote"):
            post.label_covers(bad, 0, 0)
    with pytest.raises(ValueError, match=r"scale must be in \[1, 16\]"):
        post.label_layout(box, 3, scale=0)
    with pytest.raises(ValueError, match="x1, y1, x2, y2"):
        post.label_layout([1, 2, 3], 3)


def test_draw_labels_refusals_need_no_gpu():
    """a plan-only handle (device = -1): every argument error is reported as such, and a good call as 'plan-only'"""
    pkg, lib = load_pkg(), load_pkg("_lib")
    net = pkg.NativeHRNet(32, 17, (64, 64), "fp32", max_batch=2, device=-1)
    L, h = net._lib, net._h

    def bgr(**change):
        e = lib.CanvasC()
        e.y, e.height, e.width, e.pitch_y, e.format = 4096, 120, 160, 480, 0      # never touched: nothing is launched
        for k, v in change.items():
            setattr(e, k, v)
        return e

    def yuv(fmt=1, **change):
        e = lib.CanvasC()
        e.y, e.u, e.v = 4096, 8192, (12288 if fmt == 2 else None)
        e.height, e.width, e.pitch_y, e.pitch_c, e.format = 120, 160, 192, 192 if fmt == 1 else 96, fmt
        for k, v in change.items():
            setattr(e, k, v)
        return e

    def table_of(*entries):
        t = (lib.CanvasC * len(entries))()
        for k, e in enumerate(entries):
            ctypes.memmove(ctypes.addressof(t[k]), ctypes.addressof(e), ctypes.sizeof(e))
        return t

    colours = np.arange(12, dtype=np.uint8).reshape(4, 3)
    good = dict(table=table_of(bgr(), lib.CanvasC()), nframes=2, boxes=4096, ids=8192, scores=12288, stride=5, n=2, idx=np.zeros(2, np.int32),
                colors=colours, text=colours, Cb=4, scale=0, T=2)

    def call(**change):
        a = dict(good, **change)
        p = lambda v: None if v is None else (v.ctypes.data if isinstance(v, np.ndarray) else v)   # noqa: E731
        rc = L.hrn_draw_labels_dev(h, a["table"], a["nframes"], a["boxes"], a["ids"], a["scores"], a["stride"], a["n"], p(a["idx"]),
                                   p(a["colors"]), p(a["text"]), a["Cb"], a["scale"], a["T"], None)
        return rc, L.hrn_last_error(h).decode()

    for change in (dict(), dict(ids=None), dict(scores=None, stride=0), dict(ids=None, scores=None), dict(nframes=1, idx=None), dict(n=0),
                   dict(n=0, boxes=None), dict(scale=16, T=16), dict(scale=1, T=0), dict(stride=1), dict(table=table_of(yuv(1), lib.CanvasC())),
                   dict(table=table_of(yuv(2), yuv(1, y=16384)), idx=np.asarray([0, 1], np.int32))):
        rc, err = call(**change)
        assert rc == 7 and "plan-only" in err, (change.keys(), err)
    refused = [
        (dict(n=-1), "n is negative"), (dict(Cb=0), "Cb must be at least 1"), (dict(Cb=-3), "Cb must be at least 1"),
        (dict(scale=-1), "scale must be in [0, 16]"), (dict(scale=17), "scale must be in [0, 16]"),
        (dict(T=-1), "thickness must be in [0, 16]"), (dict(T=17), "thickness must be in [0, 16]"),
        (dict(stride=0), "score_stride must be at least 1"), (dict(stride=-5), "score_stride must be at least 1"),
        (dict(table=None), "null canvases / boxes / colours"), (dict(boxes=None), "null canvases"), (dict(colors=None), "null canvases"),
        (dict(text=None), "null canvases"), (dict(nframes=0), "null canvases"),
        (dict(idx=None), "without frame_index there must be one frame"),
        (dict(idx=np.asarray([0, 2], np.int32)), "frame_index 2 of person 1 is outside [0, 2)"),
        (dict(idx=np.asarray([-1, 0], np.int32)), "frame_index -1 of person 0 is outside [0, 2)"),
        (dict(idx=np.asarray([0, 1], np.int32)), "canvas 1, which person 1 is drawn on, is null"),
    ]
    for change, text in refused:
        rc, err = call(**change)
        assert rc == 7 and err.startswith("hrn_draw_labels_dev: ") and text in err, (list(change), err)
    faults = [
        (bgr(y=None), "is null"), (bgr(height=0), "non-positive width or height"), (bgr(height=8193), "side above 8192"),
        (bgr(pitch_y=479), "pitch below three times its width"), (bgr(format=3), "unknown format"),
        (yuv(1, height=121), "odd width or height"), (yuv(1, pitch_y=158), "pitch_y below its width"), (yuv(1, pitch_c=158), "pitch_c below its width"),
        (yuv(2, pitch_c=79), "pitch_c below half its width"), (yuv(2, v=None), "null plane"),
    ]
    for entry, text in faults:
        first = yuv(1) if entry.format in (1, 2) else bgr()
        rc, err = call(table=table_of(first, entry), idx=np.asarray([0, 1], np.int32))
        assert rc == 7 and "canvas 1, which person 1 is drawn on, " in err and text in err, (text, err)
        rc, err = call(table=table_of(first, entry))                      # ... while nobody referring to it is fine
        assert rc == 7 and "plan-only" in err, (text, err)
    rc, err = call(table=table_of(bgr(), bgr(height=60)), idx=np.asarray([0, 1], np.int32))
    assert rc == 7 and "canvases 0 and 1 name the same buffer" in err and "must not overlap" in err, err
    rc, err = call(table=table_of(bgr(), yuv(1)), idx=np.asarray([0, 1], np.int32))
    assert rc == 7 and "mixes formats" in err and "all BGR or all YUV" in err, err
    net.close()


def sanitizer_compiler(tmp_path):
    """a host C++ compiler that links a program with -fsanitize=address,undefined: (command with those flags, None), or (None, why not)"""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    tried = []
    for cc in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(cc) or (cc if os.path.exists(cc) else None)
        if not path:
            continue
        for runtime in (["-static-libasan", "-static-libubsan"], []):      # (GCC links its runtimes shared by default; Clang statically)
            cmd = [path, "-fsanitize=address,undefined"] + runtime
            r = subprocess.run(cmd + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True)
            if r.returncode == 0 and subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0:
                return cmd, None
        tried.append("%s: %s" % (path, (r.stderr or "the probe did not run").strip().splitlines()[-1:]))
    return None, "; ".join(tried) or "no C++ compiler found"


def test_the_walk_under_sanitizers(tmp_path):
    """tests/labels_walk.cpp: the header alone, compiled for the host with AddressSanitizer and UBSan, over the cases above"""
    lib = load_pkg("_lib")
    cc, why = sanitizer_compiler(tmp_path)
    assert cc, "no host compiler links -fsanitize=address,undefined here: " + str(why)
    exe = tmp_path / "labels_walk"
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "labels_walk.cpp")
    subprocess.run(cc + ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fno-sanitize-recover=all",
                         "-I", lib.CSRC, "-o", str(exe), src], check=True)
    all_cases = cases()
    lines = []
    for c in all_cases:
        score = F32(0 if c["score"] is None else c["score"])
        lines.append("%d %d %d %d %d %d %d %d %d %d %d %d" % (c["box"] + (c["pid"] is not None, c["pid"] or 0, c["score"] is not None,
                                                               int(score.view(np.uint32)), c["s"], c["T"]) + tuple(c["window"])))
    (tmp_path / "cases.txt").write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe), str(tmp_path / "cases.txt")], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    out = r.stdout.split("\n")[:-1]
    assert len(out) == len(all_cases)
    for c, line in zip(all_cases, out):
        cls = ref_classes(c)
        h = 1469598103934665603
        for v in cls.reshape(-1).tolist():
            h = ((h ^ v) * 1099511628211) & (2 ** 64 - 1)
        drawn = label_ref.is_drawn(c["box"])
        want = (int(drawn), len(label_ref.cells(c["pid"], c["score"])) if drawn else 0, int((cls == 1).sum()), int((cls == 2).sum()), h)
        assert tuple(int(v) for v in line.split()) == want, (c, line)
