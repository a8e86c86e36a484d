"""BGR -> 4:2:0 YCbCr without a GPU: the table and the host form (``hrn_yuv_forward_coefficients``, ``hrn_bgr_to_yuv_blocks``) against
the numpy restatement (tests/bgr2yuv_ref.py) bit for bit over all 2^24 colours, the six conditions of the definition measured on the
restatement, csrc/yuv_fwd.h alone under AddressSanitizer and UBSan, every refusal of ``hrn_bgr_to_yuv_frames`` on a plan-only
handle, the declarations, ``bgr_to_yuv``'s argument errors."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import bgr2yuv_ref as ref
import yuv10_ref
import yuv_ref
from conftest import load_pkg

NEW = {"hrn_yuv_forward_coefficients", "hrn_bgr_to_yuv_blocks", "hrn_bgr_to_yuv_frames"}
TABLES = [(m, r) for m in ("bt601", "bt709") for r in ("limited", "full")]
# the values of the definition's text, (R, G, B) per row
STATED = {
    ("bt601", "limited"): (16, 269262, 528618, 102662, -155423, -305128, 460551, 460551, -385654, -74897),
    ("bt601", "full"): (0, 313524, 615514, 119538, -176932, -347356, 524288, 524288, -439026, -85262),
    ("bt709", "limited"): (16, 191455, 644067, 65019, -105533, -355018, 460551, 460551, -418321, -42230),
    ("bt709", "full"): (0, 222927, 749942, 75707, -120138, -404150, 524288, 524288, -476214, -48074),
}


def lib_blocks(L, matrix, range_, depth, bgr):
    bgr = np.ascontiguousarray(bgr, np.uint8).reshape(-1, 4, 3)
    out = np.empty((len(bgr), 6), np.uint16)
    rc = L.hrn_bgr_to_yuv_blocks(ref.MATRICES[matrix], ref.RANGES[range_], depth, bgr.ctypes.data, len(bgr), out.ctypes.data)
    assert rc == 0
    return out


def test_symbols_and_sources():
    lib = load_pkg("_lib")
    assert NEW <= set(lib.header_symbols()) and NEW <= set(lib.SYMBOLS)
    assert set(lib.header_symbols()) == set(lib.SYMBOLS)
    assert "yuv_out.hip" in lib.SOURCES
    for f in ("yuv_out.hip", "yuv_fwd.h"):
        assert os.path.exists(os.path.join(lib.CSRC, f)), f
    for f in ("yuv_out.hip", "hrnet_mi355.cpp"):   # one text for the host and the device
        assert '#include "yuv_fwd.h"' in open(os.path.join(lib.CSRC, f)).read(), f
    assert os.path.join(lib.CSRC, "yuv_fwd.h") in lib._deps("yuv_out.hip")
    L = lib.load()
    for name in NEW:
        assert hasattr(L, name), name
    pkg = load_pkg()
    assert hasattr(pkg.NativeHRNet, "bgr_to_yuv") and hasattr(pkg.YuvFrame, "empty")
    assert "bgr_to_yuv" in pkg.YuvFrame.__doc__


def test_coefficients_are_the_rule():
    L = load_pkg("_lib").load()
    for key in TABLES:
        out = np.zeros(10, np.int32)
        assert L.hrn_yuv_forward_coefficients(ref.MATRICES[key[0]], ref.RANGES[key[1]], out.ctypes.data) == 0
        got = tuple(int(v) for v in out)
        assert got == ref.table(*key) == STATED[key], (key, got, ref.table(*key))
        y0, cyr, cyg, cyb, cur, cug, cub, cvr, cvg, cvb = got
        assert cur + cug + cub == 0 and cvr + cvg + cvb == 0 and cub == cvr
        assert y0 == (16 if key[1] == "limited" else 0)
        assert abs(cyr + cyg + cyb - round((219 / 255 if key[1] == "limited" else 1) * 2 ** 20)) <= 2   # the luma row: sy, rounded thrice
    out = np.zeros(10, np.int32)
    for matrix, range_ in ((2, 0), (-1, 0), (0, 2), (0, -1), (7, 7)):
        assert L.hrn_yuv_forward_coefficients(matrix, range_, out.ctypes.data) == 7
    assert L.hrn_yuv_forward_coefficients(0, 0, None) == 7 and not out.any()
    px = np.zeros((1, 4, 3), np.uint8)
    res = np.zeros((1, 6), np.uint16)
    for args in ((2, 0, 8), (0, 2, 8), (0, 0, 9), (0, 0, 0), (0, 0, 16)):
        assert L.hrn_bgr_to_yuv_blocks(*args, px.ctypes.data, 1, res.ctypes.data) == 7
    assert L.hrn_bgr_to_yuv_blocks(0, 0, 8, px.ctypes.data, -1, res.ctypes.data) == 7
    assert L.hrn_bgr_to_yuv_blocks(0, 0, 8, None, 1, res.ctypes.data) == 7 and L.hrn_bgr_to_yuv_blocks(0, 0, 8, px.ctypes.data, 1, None) == 7
    assert L.hrn_bgr_to_yuv_blocks(0, 0, 8, None, 0, None) == 0


@pytest.mark.parametrize("key", TABLES, ids=["%s-%s" % k for k in TABLES])
def test_all_colours_and_the_six_conditions(key):
    """all 2^24 uniform blocks, in 16 chunks: the host form equals the restatement bit for bit at both depths, and the
    restatement meets the six conditions of the definition with exactly its bounds.  Measured (colours off the float64 formula):
    530, 46 343, 2 373, 31 524.  Condition 3 as measured: no clip engages in limited range; in full range exactly two values are
    clipped at 8 bits (pure blue's U and pure red's V, 256 -> 255) and none at 10 -- that is what is asserted"""
    matrix, range_ = key
    L = load_pkg("_lib").load()
    t = ref.table(matrix, range_)
    limited = range_ == "limited"
    inverse = yuv_ref.TABLES[key]
    differ = 0                                   # colours on which Y, U or V is not the float64 formula's
    clipped = 0                                  # (colour, depth) pairs on which a clip changes a value
    worst8, worst10, worst_f, worst_s = np.zeros(3, int), np.zeros(3, int), 0, 0
    lo8, hi8, lo10, hi10 = np.full(3, 1 << 20), np.full(3, -1), np.full(3, 1 << 20), np.full(3, -1)
    gr = np.arange(1 << 16, dtype=np.uint32)
    for chunk in range(16):
        b = np.repeat(np.arange(16 * chunk, 16 * chunk + 16, dtype=np.uint8), 1 << 16)
        g, r = np.tile((gr >> 8).astype(np.uint8), 16), np.tile((gr & 255).astype(np.uint8), 16)
        colours = np.stack([b, g, r], 1)
        uniform = np.ascontiguousarray(np.repeat(colours[:, None, :], 4, 1))
        per_depth = {}
        for depth in (8, 10):
            want = ref.blocks(uniform, t, depth)
            got = lib_blocks(L, matrix, range_, depth, uniform)
            assert np.array_equal(got, want), (key, depth, chunk, np.flatnonzero((got != want).any(1))[:4])
            # 1. four equal pixels convert as one pixel does: every term of the chroma sum is 4 x the pixel's
            shift = 20 if depth == 8 else 18
            half = 1 << (shift - 1)
            for col, row in ((4, t[4:7]), (5, t[7:10])):
                one = (row[0] * r.astype(np.int64) + row[1] * g.astype(np.int64) + row[2] * b.astype(np.int64) + (128 << 20) + half) >> shift
                assert np.array_equal(want[:, col], np.clip(one, 0, (1 << depth) - 1))
            assert (want[:, :4] == want[:, :1]).all()
            # 3. no clip engages: the values BEFORE the clip are in range
            raw = np.stack([ref.luma_raw(t, depth, r, g, b), ref.chroma_raw(t[4:7], depth, 4 * r.astype(np.int64), 4 * g.astype(np.int64), 4 * b.astype(np.int64)),
                            ref.chroma_raw(t[7:10], depth, 4 * r.astype(np.int64), 4 * g.astype(np.int64), 4 * b.astype(np.int64))], 1)
            clipped += int((raw != want[:, [0, 4, 5]]).any(1).sum())
            lo, hi = (lo8, hi8) if depth == 8 else (lo10, hi10)
            np.minimum(lo, raw.min(0), out=lo), np.maximum(hi, raw.max(0), out=hi)
            per_depth[depth] = want[:, [0, 4, 5]].astype(np.int64)
        s8, s10 = per_depth[8], per_depth[10]
        # 2. against the float64 formula of hrn_yuv_from_bgr
        fy, fu, fv = ref.float_formula(matrix, range_, r, g, b)
        d = np.abs(s8 - np.stack([fy, fu, fv], 1).astype(np.int64))
        worst_f = max(worst_f, int(d.max()))
        differ += int((d.max(1) > 0).sum())
        # 4. / 5. back through the EXISTING inverse (the restatements hrn_yuv_to_bgr is pinned to)
        back8 = np.stack(yuv_ref.convert(s8[:, 0].astype(np.uint8), s8[:, 1].astype(np.uint8), s8[:, 2].astype(np.uint8), inverse), 1)
        back10 = np.stack(yuv10_ref.convert10(s10[:, 0], s10[:, 1], s10[:, 2], inverse), 1)
        worst8 = np.maximum(worst8, np.abs(back8.astype(np.int64) - colours).max(0))
        worst10 = np.maximum(worst10, np.abs(back10.astype(np.int64) - colours).max(0))
        # 6. the 10-bit sample is the 8-bit one at four times the resolution
        worst_s = max(worst_s, int(np.abs(s10 - 4 * s8).max()))
    print("%s %s: %d colours differ from the float64 formula (by at most %d); round trip (B, G, R) 8-bit %s, 10-bit %s; |s10 - 4 s8| <= %d; "
          "before the clips 8-bit %s..%s, 10-bit %s..%s, %d values clipped"
          % (matrix, range_, differ, worst_f, worst8, worst10, worst_s, lo8, hi8, lo10, hi10, clipped))
    assert worst_f <= 1 and differ < (1 << 16)
    # 3. the clips.  Limited range: none engages, at either depth.  Full range: none at 10 bits and none on luma, but at 8 bits
    # pure blue gives U = 256 and pure red V = 256 before the clip (128 + 127.5, rounded up: the sum is exactly 2^30) -- the float64
    # formula does the same -- so exactly these two values are clipped, by one level; nothing else is, and nothing goes below 0
    if limited:
        assert clipped == 0
        assert tuple(lo8) == (16, 16, 16) and tuple(hi8) == (235, 240, 240)
        assert tuple(lo10) == (64, 64, 64) and tuple(hi10) == (940, 960, 960)
    else:
        assert clipped == 2
        assert tuple(lo8) == (0, 1, 1) and tuple(hi8) == (255, 256, 256)
        assert tuple(lo10) == (0, 2, 2) and tuple(hi10) == (1020, 1022, 1022)
    assert all(w <= bound for w, bound in zip(worst8, (2, 1, 1) if limited else (1, 1, 1))), worst8          # 4. (B, G, R)
    assert all(w <= bound for w, bound in zip(worst10, (1, 0, 0) if key == ("bt601", "limited") else (0, 0, 0))), worst10   # 5.
    assert worst_s <= 2                                                                                           # 6.


@pytest.mark.parametrize("depth", [8, 10])
def test_non_uniform_blocks_equal_the_restatement(depth):
    """seeded blocks of four different pixels, and blocks of extreme pixels: the chroma SUM is exercised"""
    L = load_pkg("_lib").load()
    rng = np.random.default_rng(depth)
    noise = rng.integers(0, 256, (300000, 4, 3), dtype=np.uint8)
    corners = rng.choice(np.asarray([0, 1, 254, 255], np.uint8), (20000, 4, 3))
    bgr = np.concatenate([noise, corners])
    for key in TABLES:
        got, want = lib_blocks(L, *key, depth, bgr), ref.blocks(bgr, ref.table(*key), depth)
        assert np.array_equal(got, want), (key, np.flatnonzero((got != want).any(1))[:4])
        assert int(want.max()) <= (255 if depth == 8 else 1023)


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


def test_the_extreme_blocks_under_sanitizers(tmp_path):
    """tests/bgr2yuv_walk.cpp: csrc/yuv_fwd.h alone, compiled for the host with AddressSanitizer and UBSan (signed overflow ends
    the program): a clean exit over the extreme blocks says every sum fits int32; its lines equal the restatement"""
    lib = load_pkg("_lib")
    cc, why = sanitizer_compiler(tmp_path)
    assert cc, "no host compiler links -fsanitize=address,undefined here: " + str(why)
    exe = tmp_path / "bgr2yuv_walk"
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bgr2yuv_walk.cpp")
    subprocess.run(cc + ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fno-sanitize-recover=all", "-I", lib.CSRC, "-o", str(exe), src], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = [[int(v) for v in line.split()] for line in r.stdout.split("\n")[:-1]]
    assert len(lines) == 4 * 2 * 8
    names_m, names_r = {v: k for k, v in ref.MATRICES.items()}, {v: k for k, v in ref.RANGES.items()}
    seen = set()
    for line in lines:
        matrix, range_, depth = names_m[line[0]], names_r[line[1]], line[2]
        bgr = np.asarray(line[3:15], np.uint8).reshape(1, 4, 3)
        assert line[15:] == [int(v) for v in ref.blocks(bgr, ref.table(matrix, range_), depth)[0]], line
        seen.add((matrix, range_, depth, tuple(line[3:6])))
    assert len(seen) >= 4 * 2 * 6   # black, white and the rows' extremes are different blocks
    # the largest sum of all, reached: full range, a chroma row's maximiser -- exactly 2^30 before the shift
    t = ref.table("bt601", "full")
    assert t[6] * 1020 + (128 << 22) + (1 << 21) == 1 << 30


def canvas(lib, fmt=0, h=120, w=160, y=4096, pitch=None, **change):
    """an hrn_canvas of fake addresses (nothing is launched on a plan-only handle): BGR (fmt 0) or a YUV layout, packed unless `pitch`"""
    e = lib.CanvasC()
    e.format, e.height, e.width = fmt, h, w
    if fmt == 0:
        e.y, e.pitch_y = y, 3 * w if pitch is None else pitch
    else:
        wide, planar = fmt in (5, 6), fmt in (2, 6)
        pitch = (2 * w if wide else w) if pitch is None else pitch
        e.y, e.u, e.pitch_y = y, (y or 4096) + pitch * h, pitch
        e.pitch_c = pitch // 2 if planar else pitch
        if planar:
            e.v = e.u + e.pitch_c * (h // 2)
    for k, v in change.items():
        setattr(e, k, v)
    return e


def table_of(lib, *entries):
    t = (lib.CanvasC * len(entries))()
    for k, e in enumerate(entries):
        t[k] = e
    return t


def test_frames_refusals_need_no_gpu():
    """a plan-only handle (device = -1): every argument error is reported as such, before 'plan-only'; a good call as 'plan-only'"""
    pkg, lib = load_pkg(), load_pkg("_lib")
    net = pkg.NativeHRNet(32, 17, (64, 64), "fp32", max_batch=2, device=-1)
    L, h = net._lib, net._h

    def call(src, dst, n=None):
        rc = L.hrn_bgr_to_yuv_frames(h, None if src is None else table_of(lib, *src), None if dst is None else table_of(lib, *dst),
                                     (len(src) if src is not None else len(dst)) if n is None else n, None)
        return rc, L.hrn_last_error(h).decode()

    C = lambda *a, **k: canvas(lib, *a, **k)   # noqa: E731
    far = 1 << 24
    good = [([C()], [C(f, y=far)]) for f in (1, 2, 4, 5, 6)]
    good += [([C()], [C(1, y=far, matrix=1, range=1)]), ([C(pitch=487)], [C(2, y=far, pitch=166)]), ([C(h=2, w=2)], [C(5, 2, 2, far)]),
             ([C(h=8192, w=8192)], [C(6, 8192, 8192, far)]), ([C(y=4097, pitch=481)], [C(1, y=far + 1, pitch=163)]),
             ([C(), C(h=40, w=56, y=8192)], [C(1, y=far), C(6, 40, 56, 2 * far, matrix=1)]),   # sizes, layouts and tables may differ by frame
             ([C(y=4097)], [C(5, y=far, pitch=322)])]
    for src, dst in good:
        rc, err = call(src, dst)
        assert rc == 7 and "plan-only" in err, err
    rc, err = call([], [], n=0)
    assert rc == 7 and "plan-only" in err, err
    assert L.hrn_bgr_to_yuv_frames(h, None, None, 0, None) == 7 and "plan-only" in L.hrn_last_error(h).decode()
    refused = [
        (([C()], [C(1, y=far)], -1), "nframes is negative"),
        ((None, [C(1, y=far)], 1), "null frame tables"), (([C()], None, 1), "null frame tables"),
        (([C(1)], [C(1, y=far)]), "frame 0: the source is not an HRN_PIX_BGR frame"), (([C(5)], [C(5, y=far)]), "the source is not an HRN_PIX_BGR"),
        (([C(), C(2, y=8192)], [C(1, y=far), C(2, y=2 * far)]), "frame 1: the source is not"),
        (([C()], [C(y=far)]), "the destination has an unknown format"), (([C()], [C(1, y=far, format=3)]), "the destination has an unknown format"),
        (([C()], [C(1, y=far, format=7)]), "unknown format (HRN_PIX_NV12, HRN_PIX_I420, HRN_PIX_NV21, HRN_PIX_P010 or HRN_PIX_I010)"),
        (([C()], [C(1, y=far, format=-1)]), "unknown format"),
        (([C()], [C(1, y=far, matrix=2)]), "the destination has an unknown matrix (HRN_YUV_BT601 or HRN_YUV_BT709)"),
        (([C()], [C(2, y=far, matrix=-1)]), "unknown matrix"),
        (([C()], [C(1, y=far, range=2)]), "the destination has an unknown range (HRN_YUV_LIMITED or HRN_YUV_FULL)"),
        (([C()], [C(6, y=far, range=-1)]), "unknown range"),
        (([C(y=None)], [C(1, y=far)]), "the source has a null plane"), (([C()], [C(1, y=far, u=None)]), "the destination has a null plane"),
        (([C()], [C(1, y=None)]), "the destination has a null plane"), (([C()], [C(2, y=far, v=None)]), "the destination has a null plane"),
        (([C()], [C(6, y=far, v=None)]), "null plane"),
        (([C(h=0)], [C(1, h=0, y=far)]), "the source has a non-positive width or height"), (([C(w=-4)], [C(1, w=-4, y=far)]), "non-positive"),
        (([C(h=121)], [C(1, h=121, y=far)]), "the source has an odd width or height"), (([C(w=161)], [C(2, w=161, y=far)]), "odd width or height"),
        (([C()], [C(1, h=121, y=far)]), "the destination has an odd width or height"),
        (([C(w=8194)], [C(1, w=8194, y=far)]), "the source has a side above 8192"), (([C(h=8194)], [C(5, h=8194, y=far)]), "a side above 8192"),
        (([C()], [C(1, h=122, y=far)]), "frame 0: the destination is 122 x 160, the source is 120 x 160"),
        (([C()], [C(5, w=158, y=far)]), "the destination is 120 x 158, the source is 120 x 160"),
        (([C(pitch=479)], [C(1, y=far)]), "the source has pitch_y below its row's bytes"),
        (([C()], [C(1, y=far, pitch=159)]), "the destination has pitch_y below its row's bytes"),
        (([C()], [C(1, y=far, pitch_c=158)]), "the destination has pitch_c below its chroma row's bytes"),
        (([C()], [C(2, y=far, pitch_c=79)]), "pitch_c below"), (([C()], [C(5, y=far, pitch=318)]), "pitch_y below"),
        (([C()], [C(5, y=far, pitch_c=318)]), "pitch_c below"), (([C()], [C(6, y=far, pitch_c=158)]), "pitch_c below"),
        (([C(h=2, w=2, pitch=1 << 30)], [C(1, 2, 2, far)]), "the source has a plane with pitch * rows >= 2^31"),
        (([C(h=2, w=2)], [C(1, 2, 2, far, pitch=1 << 30)]), "the destination has a plane with pitch * rows >= 2^31"),
        (([C()], [C(5, y=far + 1)]), "the destination has an odd plane address or pitch on a 10-bit frame"),
        (([C()], [C(5, y=far, pitch=323)]), "odd plane address or pitch on a 10-bit frame"),
        (([C()], [C(6, y=far, pitch_c=161)]), "odd plane address or pitch"), (([C()], [C(6, y=far, v=far + 77777)]), "odd plane address or pitch"),
        (([C(y=far)], [C(1, y=far)]), "the source of frame 0 is the destination of frame 0"),
        (([C(), C(y=far)], [C(1, y=far), C(1, y=2 * far)]), "the source of frame 1 is the destination of frame 0"),
        (([C(), C(y=8192)], [C(1, y=far), C(2, y=far)]), "frames 0 and 1 name the same destination"),
        (([C(), C(y=8192)], [C(1, y=far), C(1, y=2 * far, range=5)]), "frame 1: the destination has an unknown range"),
    ]
    for args, text in refused:
        rc, err = call(*args)
        assert rc == 7 and err.startswith("hrn_bgr_to_yuv_frames: ") and text in err and "plan-only" not in err, (text, err)
    net.close()


def test_python_argument_errors():
    """what ``bgr_to_yuv`` and ``YuvFrame.empty`` tell themselves, before anything reaches the library (a plan-only engine: no GPU)"""
    pkg = load_pkg()
    Y = pkg.YuvFrame
    f = Y.empty(4, 6, "p010", "bt709", "full")
    assert (f.height, f.width, f.pitch, f.format, f.matrix, f.range, f.nbytes, f.data.numel()) == (4, 6, 12, "p010", "bt709", "full", 72, 72)
    assert Y.empty(4, 6).nbytes == 36 and Y.empty(2, 2, "nv12", chroma_order="vu").chroma_order == "vu"
    for kw in (dict(format="nv21"), dict(format="bgr"), dict(matrix="bt2020"), dict(range="tv"), dict(chroma_order="vu", format="i420"),
               dict(chroma_order="xy")):
        with pytest.raises(ValueError):
            Y.empty(4, 6, **kw)
    for hw in ((3, 6), (4, 5), (0, 6), (4, -2)):
        with pytest.raises(ValueError):
            Y.empty(*hw)
    import inspect
    sig = inspect.signature(pkg.NativeHRNet.bgr_to_yuv)
    assert list(sig.parameters) == ["self", "frames", "format", "matrix", "range", "chroma_order", "out"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == ["nv12", "bt601", "limited", "uv", None]
    assert not hasattr(pkg.SimpleHRNet, "bgr_to_yuv")
    import torch
    net = pkg.NativeHRNet(32, 17, (64, 64), "fp32", max_batch=2, device=-1)
    frame = np.zeros((4, 6, 3), np.uint8)
    bad = [dict(frames=frame, format="nv21"), dict(frames=frame, format="yuv420p"), dict(frames=frame, matrix="bt2020"),
           dict(frames=frame, range="pc"), dict(frames=frame, chroma_order="vu", format="p010"), dict(frames=[], format="nv21"),
           dict(frames=Y.empty(4, 6)), dict(frames=[frame, Y.empty(4, 6)]), dict(frames=[frame, None]),
           dict(frames=np.zeros((5, 6, 3), np.uint8)), dict(frames=np.zeros((2, 4, 7, 3), np.uint8)), dict(frames=np.zeros((4, 6), np.uint8)),
           dict(frames=np.zeros((4, 6, 4), np.uint8)), dict(frames=torch.zeros((0, 6, 3), dtype=torch.uint8)),
           dict(frames=frame, out=torch.zeros(36, dtype=torch.uint8)), dict(frames=frame, out=[Y.empty(4, 6), Y.empty(4, 6)]),
           dict(frames=[frame, frame], out=Y.empty(4, 6)), dict(frames=frame, out=Y.empty(6, 4)), dict(frames=frame, out=[None])]
    for kw in bad:
        with pytest.raises(ValueError):
            net.bgr_to_yuv(**kw)
    net.close()
