"""The face mosaic on the GPU: ``NativeHRNet.mosaic`` against the host form of the same definition (``postproc.mosaic``:
hrn_mosaic_host, which tests/test_mosaic_host.py holds to the numpy restatement) -- whole buffers, byte for byte and status for
status, on frames of random bytes with sentinel bytes around and between the rows, so that a stray write shows.  Tiny frames,
designed joints: no pass of the network is needed."""
import numpy as np
import pytest
import torch

import mosaic_cases
from conftest import load_pkg
from mosaic_cases import BOXES, CELLS, F32, HEAD, noise

pytestmark = pytest.mark.gpu

# (format, height, width, pitch, byte offset of the frame in its buffer)
LAYOUTS = {
    "bgr, base and pitch multiples of 4": ("bgr", 70, 90, 272, 0),
    "bgr, an odd offset and pitch 3 W + 5": ("bgr", 70, 90, 275, 1),
    "nv12, aligned": ("nv12", 66, 94, 96, 0),
    "nv12, an odd offset and pitch": ("nv12", 66, 94, 99, 1),
    "i420, aligned": ("i420", 66, 94, 96, 0),
    "i420, an odd offset, chroma rows of 49 bytes": ("i420", 66, 94, 98, 1),
}
TAIL = 64       # sentinel bytes behind the frame


@pytest.fixture(scope="module")
def net():
    n = load_pkg().NativeHRNet(32, 17, (64, 96), "fp32", max_batch=4, device=0)
    yield n
    n.close()


class Canvas:
    """one noise buffer twice, on the host and on the device, and the same frame in both: `host_frame` for postproc.mosaic,
    `frame` for NativeHRNet.mosaic"""

    def __init__(self, layout, seed):
        pkg = load_pkg()
        self.fmt, self.h, self.w, self.pitch, self.offset = fmt, h, w, pitch, offset = layout
        size = h * pitch if fmt == "bgr" else h * pitch * 3 // 2
        self.before = noise(offset + size + TAIL, seed)
        self.host = self.before.copy()
        self.dev = torch.from_numpy(self.before.copy()).cuda()
        if fmt == "bgr":
            self.host_frame = np.lib.stride_tricks.as_strided(self.host[offset:], (h, w, 3), (pitch, 3, 1))
            self.frame = torch.as_strided(self.dev, (h, w, 3), (pitch, 3, 1), offset)
        else:
            self.host_frame = pkg.YuvFrame(self.host[offset:offset + size], h, w, fmt, "bt601", "limited", pitch)
            self.frame = pkg.YuvFrame(self.dev[offset:offset + size], h, w, fmt, "bt601", "limited", pitch)
            assert np.shares_memory(self.host_frame.data.numpy(), self.host) and self.frame.data.data_ptr() == self.dev.data_ptr() + offset

    def download(self):
        return self.dev.cpu().numpy()


def on_device(x, dtype):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype)).cuda()


def check(net, layout, seed, device_inputs=True, with_status=True, **kw):
    """the engine and the host form on the same bytes; returns (buffer before, buffer after, status), the two having been held equal"""
    post = load_pkg("postproc")
    c = Canvas(layout, seed)
    _, want_status = post.mosaic(c.host_frame, return_status=True, **kw)
    given = dict(kw)
    if device_inputs:
        given["pts"], given["boxes"] = on_device(kw.get("pts"), F32), on_device(kw.get("boxes"), np.int32)
    out = net.mosaic(c.frame, return_status=with_status, **given)
    status = None
    if with_status:
        out, status = out
        assert status.is_cuda and status.dtype == torch.int32
        np.testing.assert_array_equal(status.cpu().numpy(), want_status, err_msg=str((layout, sorted(kw))))
    assert out is c.frame or (c.fmt == "bgr" and out.data_ptr() == c.frame.data_ptr())      # in place: the same object, or the same view
    got = c.download()
    np.testing.assert_array_equal(got, c.host, err_msg=str((layout, {k: v for k, v in kw.items() if k not in ("pts", "boxes")})))
    return c.before, got, want_status


def crowd(h, w, seed):
    designed = [p for name, p in mosaic_cases.people() if "the ends of the range" not in name]
    return np.concatenate([np.stack(designed), mosaic_cases.scattered(25, h, w, seed)])


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_every_layout_and_cell_equals_the_host_form(net, name):
    layout = LAYOUTS[name]
    pts = crowd(layout[1], layout[2], 1)
    seen = set()
    for k, cell in enumerate(CELLS + (None,)):
        before, after, status = check(net, layout, k, pts=pts, joints=HEAD, cell=cell)
        assert (before != after).any()
        seen |= set(status.tolist())
    assert seen == {0, 1, 2}
    check(net, layout, 7, pts=pts, joints=HEAD, cell=8, with_status=False)                     # status_dev NULL
    check(net, layout, 8, pts=pts, joints=None, cell=16, scale=(3, 2), min_half=3, confidence_threshold=0.05)
    check(net, layout, 9, pts=pts, joints=(2, 2, 0), cell=4, scale=(64, 1), device_inputs=False)    # host pts are uploaded
    everything = mosaic_cases.all_people()                  # the two people whose region is the whole canvas: every cell, partial ones included
    before, after, _ = check(net, layout, 10, pts=everything, joints=HEAD, cell=32)
    tail = layout[4] + (layout[1] * layout[3] if layout[0] == "bgr" else layout[1] * layout[3] * 3 // 2)
    np.testing.assert_array_equal(after[tail:], before[tail:])
    np.testing.assert_array_equal(after[:layout[4]], before[:layout[4]])


def test_a_second_identical_call_changes_nothing_and_the_order_does_not_matter(net):
    layout = LAYOUTS["bgr, an odd offset and pitch 3 W + 5"]
    pts = crowd(70, 90, 2)
    c = Canvas(layout, 3)
    net.mosaic(c.frame, pts=on_device(pts, F32), joints=HEAD, cell=8)
    first = c.download()
    net.mosaic(c.frame, pts=on_device(pts, F32), joints=HEAD, cell=8)
    np.testing.assert_array_equal(c.download(), first)
    d = Canvas(layout, 3)
    order = np.random.default_rng(0).permutation(len(pts))
    net.mosaic(d.frame, pts=on_device(pts[order], F32), joints=HEAD, cell=8)
    np.testing.assert_array_equal(d.download(), first)
    assert (first != c.before).any()


def test_two_canvases_of_different_sizes_and_one_nobody_is_on(net):
    post = load_pkg("postproc")
    sizes = [(70, 90), None, (40, 50), (1030, 1100)]
    frame_index = np.asarray([2, 0, 3, 0, 2, 2, 0, 3, 0], np.int32)
    pts = mosaic_cases.scattered(len(frame_index), 40, 50, seed=4)
    for cell in (None, 16):                                 # None: 8 on the small canvases, 16 on the large one
        before = [None if s is None else noise(s + (3,), 20 + k) for k, s in enumerate(sizes)]
        host = [None if b is None else b.copy() for b in before]
        devs = [None if b is None else torch.from_numpy(b.copy()).cuda() for b in before]
        _, want_status = post.mosaic(host, pts=pts, joints=HEAD, frame_index=frame_index, cell=cell, return_status=True)
        out, status = net.mosaic(devs, pts=on_device(pts, F32), joints=HEAD, frame_index=frame_index, cell=cell, return_status=True)
        assert out[1] is None and all(o is d for o, d in zip(out, devs))
        np.testing.assert_array_equal(status.cpu().numpy(), want_status)
        for f in (0, 2, 3):
            np.testing.assert_array_equal(devs[f].cpu().numpy(), host[f], err_msg="frame %d" % f)
            assert (host[f] != before[f]).any()
    with pytest.raises(RuntimeError, match="is null"):
        net.mosaic(devs, pts=pts[:1], joints=HEAD, frame_index=[1])
    with pytest.raises(ValueError, match="frame_index"):
        net.mosaic(devs, pts=pts, joints=HEAD)


@pytest.mark.parametrize("name", ["bgr, an odd offset and pitch 3 W + 5", "nv12, aligned"])
def test_more_people_than_one_cull_chunk(net, name):
    """300 people whose regions all meet tile (0, 0): two chunks of the cull; then only people of the second chunk have a region"""
    layout = LAYOUTS[name]
    pts = mosaic_cases.scattered(300, 70, 90, seed=5, spread=(26, 26))
    for cell in (2, 8, 32):
        _, _, status = check(net, layout, 11, pts=pts, joints=HEAD, cell=cell, min_half=2)
        assert (status == 0).all()
    quiet = pts.copy()
    quiet[:256, :, 2] = 0.0                                 # the first chunk: nobody live
    quiet[256:, :, 1] += 2.0
    before, after, status = check(net, layout, 12, pts=quiet, joints=HEAD, cell=4, min_half=1, scale=(1, 64))
    assert (status[:256] == 1).all() and (status[256:] == 0).all() and (before != after).any()
    lone = quiet.copy()
    lone[256:299, :, 2] = 0.0                               # ... and of the second chunk only its last person
    before, after, status = check(net, layout, 13, pts=lone, joints=HEAD, cell=4, min_half=1, scale=(1, 64))
    assert status.tolist() == [1] * 299 + [0] and (before != after).any()


def test_a_region_that_straddles_four_tiles_and_a_tile_nobody_touches(net):
    layout = LAYOUTS["bgr, base and pitch multiples of 4"]
    h, w, pitch = layout[1:4]
    one = mosaic_cases.person({0: (31, 31), 1: (34, 29), 2: (29, 29)})[None]        # X 29..34, Y 29..31: R = 5, the square (26, 25, 38, 36)
    for cell in CELLS:
        before, after, status = check(net, layout, 14, pts=one, joints=HEAD, cell=cell)
        assert status.tolist() == [0]
        rows_before, rows_after = before[:h * pitch].reshape(h, pitch), after[:h * pitch].reshape(h, pitch)
        changed = np.zeros((h, w), bool)
        changed[:, :] = (rows_before[:, :3 * w] != rows_after[:, :3 * w]).reshape(h, w, 3).any(2)
        for ty in (0, 1):
            for tx in (0, 1):
                assert changed[32 * ty:32 * ty + 32, 32 * tx:32 * tx + 32].any(), (cell, ty, tx)       # all four tiles took part
        lo, hi = lambda v: v // cell * cell, lambda v: -(-v // cell) * cell        # noqa: E731
        outside = np.ones((h, w), bool)
        outside[lo(25):hi(36), lo(26):hi(38)] = False
        assert not changed[outside].any()                   # the cells the square touches, and no other
        assert not changed[64:].any() and not changed[:, 64:].any()          # the tiles nobody touches keep their bytes
    # the same through boxes, on an NV12 frame
    box = np.asarray([[26, 25, 38, 36]], np.int32)
    for cell in (2, 32):
        check(net, LAYOUTS["nv12, an odd offset and pitch"], 15, boxes=box, cell=cell)


@pytest.mark.parametrize("name", ["bgr, an odd offset and pitch 3 W + 5", "nv12, an odd offset and pitch", "i420, aligned"])
def test_boxes_from_device_memory_and_from_numpy(net, name):
    layout = LAYOUTS[name]
    rng = np.random.default_rng(6)
    x1, y1 = rng.integers(-10, 90, 70), rng.integers(-10, 70, 70)
    boxes = np.concatenate([BOXES, np.stack([x1, y1, x1 + rng.integers(-2, 30, 70), y1 + rng.integers(-2, 30, 70)], 1).astype(np.int32)])
    for cell in (4, 16, None):
        _, a, status = check(net, layout, 16, boxes=boxes, cell=cell, device_inputs=True)
        _, b, _ = check(net, layout, 16, boxes=boxes, cell=cell, device_inputs=False)
        np.testing.assert_array_equal(a, b)
        assert set(status.tolist()) == {0, 1, 2}
    check(net, layout, 17, boxes=boxes[:65], cell=8, with_status=False)     # 65 people: a second block of the build launch, one thread used


def test_nobody_and_refusals(net):
    before = noise((46, 70, 3), 2)
    dev = torch.from_numpy(before.copy()).cuda()
    assert net.mosaic(dev, pts=np.zeros((0, 17, 3), F32), joints=HEAD) is dev               # n == 0: nothing is launched
    out, status = net.mosaic(dev, boxes=np.zeros((0, 4), np.int32), return_status=True)
    assert out is dev and tuple(status.shape) == (0,)
    pts = mosaic_cases.all_people()[:3]
    for kw, text in ((dict(cell=3), "cell must be 0, 2, 4, 8, 16 or 32"), (dict(min_half=4097), "min_half must be in"), (dict(scale=(65, 1)), "scale_num and scale_den"),
                     (dict(joints=[17]), "indices in"), (dict(joints=[]), "1 to 256 indices")):
        with pytest.raises((ValueError, RuntimeError), match=text):
            net.mosaic(dev, pts=pts, **kw)
    with pytest.raises(ValueError, match="exactly one of them"):
        net.mosaic(dev, pts=pts, boxes=BOXES[:3])
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dev.cpu().numpy(), before)
    host = net.mosaic(before.copy(), pts=pts, joints=HEAD, cell=8)          # a host frame is uploaded; the device copy is returned
    want = load_pkg("postproc").mosaic(before.copy(), pts=pts, joints=HEAD, cell=8)
    assert host.is_cuda
    np.testing.assert_array_equal(host.cpu().numpy(), want)
