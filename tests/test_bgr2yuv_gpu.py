"""BGR -> 4:2:0 YCbCr on the GPU: ``hrn_bgr_to_yuv_frames`` / ``NativeHRNet.bgr_to_yuv`` against the numpy restatement
(tests/bgr2yuv_ref.py), byte for byte over WHOLE destination buffers pre-filled with a sentinel, margins before and after included
(a write into pitch padding or beside a plane shows).  Every comparison is equality; the round trip has the definition's bounds.

Shapes: a tile is 256 x 8 pixels and a thread owns 2 rows x 4 pixels, so 2 x 2 (one 2-pixel group), 4 x 6 (a whole group and a
2-pixel tail), 38 x 70 (five tile rows, the last of 6 rows), 66 x 130, 8 x 260 and 20 x 518 (two and three tiles per row, the last
of 4 and of 6 pixels) meet every edge."""
import numpy as np
import pytest
import torch

import bgr2yuv_ref as ref
from conftest import load_pkg, state_dict_np

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
MARGIN = 64
FORMATS = ["nv12", "nv21", "i420", "p010", "i010"]
TABLES = [(m, r) for m in ("bt601", "bt709") for r in ("limited", "full")]
_NET = []


def engine():
    if not _NET:
        _NET.append(load_pkg().NativeHRNet(32, 17, (64, 64), "fp32", max_batch=2, device=0).load_state_dict(state_dict_np(32, 0)))
    return _NET[0]


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


class Job:
    """one frame of a raw call: the BGR pixels `bgr` in a source buffer at byte `src_off`, rows `src_pitch` apart; the destination
    planes in a sentinel-filled buffer, Y at MARGIN + `dst_off`, rows `pitch_y` apart (default packed, or packed + `pad`)"""

    def __init__(self, bgr, fmt, matrix="bt601", range_="limited", pad=0, src_pad=0, src_off=0, dst_off=0, pitch_y=None):
        self.bgr, self.fmt, self.matrix, self.range_ = bgr, fmt, matrix, range_
        h, w = bgr.shape[:2]
        sb = 2 if fmt in ref.TEN_BIT else 1
        planar = fmt in ref.PLANAR
        self.h, self.w = h, w
        self.src_pitch, self.src_off = 3 * w + src_pad, src_off
        self.pitch_y = (w * sb + pad) if pitch_y is None else pitch_y
        self.pitch_c = (w * sb // 2 if planar else w * sb) + pad
        self.y_off = MARGIN + dst_off
        self.u_off = self.y_off + self.pitch_y * h
        self.v_off = self.u_off + self.pitch_c * (h // 2) if planar else None
        self.end = (self.v_off if planar else self.u_off) + self.pitch_c * (h // 2) + MARGIN
        src = noise(src_off + self.src_pitch * h + 8, 99)       # (what lies between the rows is noise, and stays)
        for i in range(h):
            src[src_off + i * self.src_pitch:src_off + i * self.src_pitch + 3 * w] = bgr[i].reshape(-1)
        self.src = src
        self.want = ref.write_frame(np.full(self.end, SENTINEL, np.uint8), bgr, fmt, matrix, range_, self.y_off, self.pitch_y, self.u_off,
                                    self.pitch_c, self.v_off)


def run(jobs):
    """ONE hrn_bgr_to_yuv_frames call for all jobs; every destination buffer whole, as numpy; the sources are checked unchanged"""
    net, lib = engine(), load_pkg("_lib")
    n = len(jobs)
    s_table, d_table = (lib.CanvasC * max(n, 1))(), (lib.CanvasC * max(n, 1))()
    srcs = [torch.from_numpy(j.src).cuda() for j in jobs]
    dsts = [torch.full((j.end,), SENTINEL, dtype=torch.uint8, device="cuda") for j in jobs]
    for k, j in enumerate(jobs):
        s, d = s_table[k], d_table[k]
        s.y, s.height, s.width, s.pitch_y, s.format = srcs[k].data_ptr() + j.src_off, j.h, j.w, j.src_pitch, 0
        base = dsts[k].data_ptr()
        d.y, d.u, d.v = base + j.y_off, base + j.u_off, None if j.v_off is None else base + j.v_off
        d.height, d.width, d.pitch_y, d.pitch_c = j.h, j.w, j.pitch_y, j.pitch_c
        d.format, d.matrix, d.range = ref.LAYOUTS[j.fmt], ref.MATRICES[j.matrix], ref.RANGES[j.range_]
    net._launch("hrn_bgr_to_yuv_frames", s_table, d_table, n)
    torch.cuda.synchronize()
    for k, j in enumerate(jobs):
        np.testing.assert_array_equal(srcs[k].cpu().numpy(), j.src, err_msg="source %d was written" % k)
    return [d.cpu().numpy() for d in dsts]


def check(jobs):
    got = run(jobs)
    for k, (j, g) in enumerate(zip(jobs, got)):
        bad = np.flatnonzero(g != j.want)
        assert len(bad) == 0, "frame %d (%s %d x %d, %s %s): %d bytes differ, first at %d (Y from %d, chroma from %d): %d != %d" % (
            k, j.fmt, j.h, j.w, j.matrix, j.range_, len(bad), bad[0], j.y_off, j.u_off, g[bad[0]], j.want[bad[0]])
    return got


@pytest.mark.parametrize("fmt", FORMATS)
def test_small_and_many_tile_frames(fmt):
    """one call per size (the frame in the kernel arguments), then all sizes in one call (the table)"""
    sizes = [(2, 2), (4, 6), (8, 260), (20, 518), (10, 256), (2, 4)]
    jobs = [Job(noise((h, w, 3), 10 * h + w), fmt) for h, w in sizes]
    alone = [check([j])[0] for j in jobs]
    together = check(jobs)
    for a, b in zip(alone, together):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("fmt", FORMATS)
def test_pitched_destination_and_source_view(fmt):
    """38 x 70: destination rows 3 bytes (8 bit) / 6 bytes (10 bit) beyond their samples, Y and chroma alike, and a source view of
    rows 5 bytes beyond their pixels: bases and rows misaligned, the padding keeps the sentinel"""
    pad = 6 if fmt in ref.TEN_BIT else 3
    bgr = noise((38, 70, 3), 1)
    check([Job(bgr, fmt, pad=pad, src_pad=5)])
    check([Job(bgr, fmt, pad=pad, src_pad=0), Job(bgr, fmt, pad=0, src_pad=5), Job(bgr, fmt, pad=2 * pad, src_pad=9)])


@pytest.mark.parametrize("fmt", FORMATS)
def test_byte_path_equals_the_aligned_call(fmt):
    """66 x 130 with pitches that are multiples of 4, so the aligned call runs on dwords; the same frame with the source one byte
    and the destination one byte (two: 10 bit) off: the byte path, and the same bytes"""
    sb = 2 if fmt in ref.TEN_BIT else 1
    bgr = noise((66, 130, 3), 2)
    aligned = Job(bgr, fmt, pad=2 * sb, src_pad=2)        # 8 bit: Y 132, chroma 132 / 67; source 392 -- (I420's chroma rows are 67: its 16-bit path)
    off = Job(bgr, fmt, pad=2 * sb, src_pad=2, src_off=1, dst_off=sb)
    assert aligned.pitch_y % 4 == 0 and aligned.src_pitch % 4 == 0 and aligned.y_off % 4 == 0 and off.y_off % 4 == sb
    a, b = check([aligned, off])
    np.testing.assert_array_equal(a[aligned.y_off:aligned.end - MARGIN], b[off.y_off:off.end - MARGIN])
    # everything a multiple of 4, the chroma rows of the planar layouts included: every dword path
    wide = Job(noise((66, 136, 3), 3), fmt)
    assert wide.pitch_c % 4 == 0
    check([wide])


@pytest.mark.parametrize("matrix,range_", TABLES, ids=["%s-%s" % t for t in TABLES])
def test_every_layout_and_table(matrix, range_):
    """all five layouts at 38 x 70, packed (8 bit: rows of 70 and 35 bytes, the byte paths) and with rows that are multiples of 4
    (the dword paths with a 2-pixel tail group), in one call"""
    bgr = noise((38, 70, 3), 5)
    bgr[:4, :8] = np.asarray([[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255]], np.uint8)
    jobs = [Job(bgr, fmt, matrix, range_) for fmt in FORMATS]
    jobs += [Job(bgr, fmt, matrix, range_, pad=4 if fmt in ref.TEN_BIT else 2, src_pad=2) for fmt in FORMATS]
    check(jobs)


def test_five_frames_in_one_call_equal_five_calls():
    pkg, net = load_pkg(), engine()
    specs = [("nv12", "uv", 38, 70, "bt601", "limited"), ("nv12", "vu", 2, 2, "bt709", "full"), ("i420", "uv", 66, 130, "bt709", "limited"),
             ("p010", "uv", 4, 6, "bt601", "full"), ("i010", "uv", 20, 518, "bt709", "full")]
    frames = [noise((h, w, 3), k) for k, (_, _, h, w, _, _) in enumerate(specs)]
    outs = [pkg.YuvFrame.empty(h, w, f, m, r, order, net.torch_device) for f, order, h, w, m, r in specs]
    back = net.bgr_to_yuv(frames, out=outs)
    assert len(back) == 5 and all(a is b for a, b in zip(back, outs))
    for frame, out, (f, order, h, w, m, r) in zip(frames, outs, specs):
        alone = net.bgr_to_yuv(frame, f, m, r, order)
        assert isinstance(alone, pkg.YuvFrame) and alone.data.is_cuda
        assert (alone.height, alone.width, alone.format, alone.matrix, alone.range, alone.chroma_order) == (h, w, f, m, r, order)
        assert alone.pitch == w * alone.sample_bytes
        want = ref.packed(frame, "nv21" if order == "vu" else f, m, r)
        np.testing.assert_array_equal(alone.data.cpu().numpy(), want)
        np.testing.assert_array_equal(out.data.cpu().numpy(), want)


def test_no_frames():
    net = engine()
    assert net.bgr_to_yuv([]) == [] and net.bgr_to_yuv(np.zeros((0, 4, 4, 3), np.uint8), "p010") == []
    assert run([]) == []
    assert net._lib.hrn_bgr_to_yuv_frames(net._h, None, None, 0, None) == 0


@pytest.mark.parametrize("matrix,range_", TABLES, ids=["%s-%s" % t for t in TABLES])
def test_round_trip_through_yuv_to_bgr(matrix, range_):
    """a 64 x 64 frame of uniform 2x2 blocks in seeded colours, there and back: within 2 levels in B and 1 in G and R (limited) or
    1 in all three (full) through the 8-bit layouts; exact through the 10-bit ones, but B within 1 for BT.601 limited"""
    net = engine()
    colours = noise((32, 32, 3), 7)
    colours[0, :8] = np.asarray([[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255]], np.uint8)
    frame = np.repeat(np.repeat(colours, 2, 0), 2, 1)
    limited = range_ == "limited"
    for fmt, order in (("nv12", "uv"), ("nv12", "vu"), ("i420", "uv"), ("p010", "uv"), ("i010", "uv")):
        back = net.yuv_to_bgr(net.bgr_to_yuv(frame, fmt, matrix, range_, order)).cpu().numpy()
        worst = np.abs(back.astype(int) - frame.astype(int)).reshape(-1, 3).max(0)
        if fmt in ref.TEN_BIT:
            bound = (1, 0, 0) if (matrix, range_) == ("bt601", "limited") else (0, 0, 0)
        else:
            bound = (2, 1, 1) if limited else (1, 1, 1)
        print("%s %s %s %s: round trip off by (B, G, R) %s, bound %s" % (fmt, order, matrix, range_, worst, bound))
        assert all(w <= b for w, b in zip(worst, bound)), (fmt, worst, bound)


@pytest.mark.parametrize("fmt,order", [("nv12", "uv"), ("nv12", "vu"), ("i420", "uv"), ("p010", "uv"), ("i010", "uv")])
def test_converting_and_turning_by_180_degrees_commute(fmt, order):
    """180 degrees maps 2x2 blocks onto 2x2 blocks and the sum of four is order-free: bit for bit"""
    net = engine()
    frame = noise((38, 70, 3), 11)
    a = net.rotate_frames(net.bgr_to_yuv(frame, fmt, "bt709", "limited", order), 1)
    b = net.bgr_to_yuv(net.rotate_frames(frame, 1), fmt, "bt709", "limited", order)
    assert (a.height, a.width, a.format, a.chroma_order) == (b.height, b.width, b.format, b.chroma_order) == (38, 70, fmt, order)
    assert torch.equal(a.data, b.data)
    np.testing.assert_array_equal(b.data.cpu().numpy(), ref.packed(frame[::-1, ::-1], "nv21" if order == "vu" else fmt, "bt709", "limited"))


def test_python_shapes():
    pkg, net = load_pkg(), engine()
    dev = net.torch_device
    stack = noise((3, 8, 12, 3), 13)
    out = net.bgr_to_yuv(stack, "i420", "bt709", "full")
    assert isinstance(out, list) and len(out) == 3 and all(isinstance(f, pkg.YuvFrame) and f.device == dev for f in out)
    for f, frame in zip(out, stack):
        np.testing.assert_array_equal(f.data.cpu().numpy(), ref.packed(frame, "i420", "bt709", "full"))
    # a resident stack, a resident frame, a strided view of a resident frame, a sequence of host frames: the same bytes
    resident = torch.from_numpy(stack).cuda()
    assert all(torch.equal(a.data, b.data) for a, b in zip(net.bgr_to_yuv(resident, "i420", "bt709", "full"), out))
    assert torch.equal(net.bgr_to_yuv(resident[1], "i420", "bt709", "full").data, out[1].data)
    big = torch.from_numpy(noise((16, 24, 3), 14)).cuda()
    view = big[4:12, 6:18]
    assert not view.is_contiguous()
    np.testing.assert_array_equal(net.bgr_to_yuv(view, "p010").data.cpu().numpy(), ref.packed(view.cpu().numpy(), "p010"))
    assert torch.equal(net.bgr_to_yuv(list(stack), "i420", "bt709", "full")[2].data, out[2].data)
    # out=: the caller's objects come back, a single one for a single frame; a pitched one keeps its padding; its layout is ITS OWN
    h, w, pitch = 8, 12, 20
    mine = pkg.YuvFrame(torch.full((pitch * h * 3 // 2,), SENTINEL, dtype=torch.uint8, device=dev), h, w, "nv12", "bt601", "full", pitch,
                        chroma_order="vu")
    assert net.bgr_to_yuv(stack[0], "i010", "bt709", "limited", out=mine) is mine
    want = ref.write_frame(np.full(pitch * h * 3 // 2, SENTINEL, np.uint8), stack[0], "nv21", "bt601", "full", 0, pitch, pitch * h, pitch)
    np.testing.assert_array_equal(mine.data.cpu().numpy(), want)
    outs = [pkg.YuvFrame.empty(8, 12, "p010", device=dev) for _ in range(3)]
    back = net.bgr_to_yuv(stack, out=outs)
    assert isinstance(back, list) and all(a is b for a, b in zip(back, outs))
    np.testing.assert_array_equal(outs[2].data.cpu().numpy(), ref.packed(stack[2], "p010"))
    # refusals that need the device: a destination elsewhere, a destination that is the source
    with pytest.raises(ValueError, match="engine's device"):
        net.bgr_to_yuv(stack[0], out=pkg.YuvFrame.empty(8, 12))
    same = torch.zeros((8 * 12 * 3,), dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="in-place conversion is not offered"):
        net.bgr_to_yuv(same.view(8, 12, 3), out=pkg.YuvFrame(same, 8, 12, "nv12"))
    torch.cuda.synchronize()
    assert not bool(same.any())
