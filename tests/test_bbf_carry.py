"""The fused BasicBlock pass of the 48-channel branch (conv3x3_lds.inc: bbf_run) on blocks that walk many consecutive tiles: every tile
after a block's first one carries conv1's halo rows over from the tile before it instead of recomputing them.  Bit for bit against the
two separate launches (HRN_BBF=0), in both 16-bit formats, at all nine row pitches the pass runs at (wp = 9, 17, ..., 73: the carry
arithmetic -- the carried units, the X-unit rows, the fragment deal -- is a function of the pitch), over calls that cross image boundaries
and end on a ragged last tile; and the plan that makes the sliding tiles the common case at the headline batch."""
import numpy as np
import pytest
import torch

import plan_census as C
from conftest import load_pkg, state_dict_np

pkg = load_pkg()


def _fused_block_tiles(net, n):
    """tiles per fused block, over every grouped launch of a call of n crops (hrnet_mi355.cpp: group_blocks)"""
    blocks, members = np.zeros((40000, 6), np.int32), np.zeros(64, np.int32)
    group, tiles = 0, []
    while True:
        nb = net._lib.hrn_plan_block_map(net._h, group, n, group & 1, blocks.ctypes.data, len(blocks), members.ctypes.data, len(members))
        if nb < 0:
            break
        tiles += [int(t) for _, _, t, _, _, flags in blocks[:nb] if flags & 1]
        group += 1
    return np.asarray(tiles)


# long fused blocks even on small calls: with these values a block of a small launch holds 4096 / 2 / 64 = 32 tiles of 512 pixels when
# the tensor has as many (no cap of the kernel: plan_census.VARIANTS["long"] gives 48)
LONG_BLOCKS = {"HRN_BBF_MIN_TILES": "1", "HRN_BBF_TPB_DIV": "1", "HRN_HALF_STAGES": "4096"}


def test_long_block_switches_make_sliding_tiles_on_small_calls(monkeypatch):
    """(the GPU test below relies on it) the switches it sets give fused blocks of many tiles at its call sizes"""
    for k, v in LONG_BLOCKS.items():
        monkeypatch.setenv(k, v)
    net = pkg.NativeHRNet(48, 17, (384, 288), "bf16", max_batch=7, device=-1)
    t = _fused_block_tiles(net, 7)
    net.close()
    assert len(t) > 0 and t.max() >= 8 and t.sum() > 2 * len(t)


def test_default_fused_blocks_walk_several_tiles_at_batch_256(monkeypatch):
    """The default plan at the headline shape: the fused blocks are long enough that most tiles slide (only a block's first
    tile recomputes conv1's halo rows)."""
    for k in ("HRN_BBF_TPB_DIV", "HRN_HALF_STAGES", "HRN_BBF_MIN_TILES", "HRN_BBF", "HRN_LONG_FACTOR", "HRN_LONG_SHARE"):
        monkeypatch.delenv(k, raising=False)
    net = pkg.NativeHRNet(48, 17, (384, 288), "bf16", max_batch=256, device=-1)
    t = _fused_block_tiles(net, 256)
    net.close()
    assert len(t) > 0 and t.mean() >= 2.5
    assert (t.sum() - len(t)) / t.sum() >= 0.6   # sliding tiles / all fused tiles


PITCH_WIDTHS = list(range(32, 289, 32))       # wp = w / 4 + 1 = 9, 17, ..., 73: every pitch conv3x3_lds_bbf_ok admits


def _pitch_case(h, w):
    """(h, w, n, max_batch) of the smallest call whose branch 0 has at least five 512-pixel tiles: one fused block of five or six tiles,
    four of them sliding, across n >= 2 images, the last one short (an image is (h / 4 + 1) * (w / 4 + 1) flat rows, an odd number)"""
    n = max(2, 4 * 512 // ((h // 4 + 1) * (w // 4 + 1)) + 2)
    return (h, w, n, n)


PITCH_CASES = [_pitch_case(h, w) for w in PITCH_WIDTHS for h in (32, 64)]


def test_pitch_cases_slide_at_all_nine_pitches(monkeypatch):
    """(the GPU test below relies on it) on plan-only handles: each pitch case has fused blocks of five or more tiles at its pitch,
    ending on a ragged tile, and the nine pitches are exactly the ones any legal resolution slides at"""
    for k, v in LONG_BLOCKS.items():
        monkeypatch.setenv(k, v)
    pitches = set()
    for h, w, n, mb in PITCH_CASES:
        net = pkg.NativeHRNet(48, 17, (h, w), "bf16", max_batch=mb, device=-1)
        t, walk = _fused_block_tiles(net, n), C.walk_of(net, n)
        net.close()
        wp = w // 4 + 1
        assert len(t) > 0 and t.max() >= 5 and ("slide", wp) in walk, (h, w, n)
        assert n >= 2 and (n * (h // 4 + 1) * wp) % 512 != 0
        assert any(k[0] == "walk" and k[6] == "fused" and k[7] == 3 and k[9] == "ragged" for k in walk), (h, w, n)
        pitches.add(wp)
    assert sorted(pitches) == list(range(9, 74, 8))
    monkeypatch.undo()
    net = pkg.NativeHRNet(48, 17, (32, 320), "bf16", max_batch=64, device=-1)      # wp = 81: the fused pass is not planned
    assert not any(i.algo == 2 for i in net.conv_infos())
    net.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("h,w,n,mb", [(384, 288, 7, 7), (384, 288, 9, 5), (256, 192, 9, 9), (64, 64, 13, 13)] + PITCH_CASES)
def test_sliding_fused_tiles_are_bit_identical(monkeypatch, dtype, h, w, n, mb):
    """Fused blocks of many tiles (32 with LONG_BLOCKS where the tensor holds as many; most of them sliding) against HRN_BBF=0:
    heat-maps and joints, bit for bit."""
    assert torch.cuda.is_available(), "GPU tests need a GPU: the HIP path has no CPU fallback"
    crops = torch.from_numpy(pkg.synth_crops(n, h, w, seed=61)).cuda()
    boxes = pkg.synth_boxes(n, seed=62)
    for k, v in LONG_BLOCKS.items():
        monkeypatch.setenv(k, v)
    outs = []
    for on in (True, False):
        monkeypatch.delenv("HRN_BBF", raising=False)
        if not on:
            monkeypatch.setenv("HRN_BBF", "0")
        net = pkg.NativeHRNet(48, 17, (h, w), dtype, max_batch=mb, device=0)
        net.load_state_dict(state_dict_np(48, 5))
        tiles = _fused_block_tiles(net, mb)
        hm, pts = net.predict_crops(crops, boxes, return_heatmaps=True)
        outs.append((hm.cpu().numpy(), pts.cpu().numpy(), tiles))
        net.close()
    assert len(outs[0][2]) > 0 and outs[0][2].max() >= 4   # the fused pass ran, with sliding tiles
    assert len(outs[1][2]) == 0
    assert np.isfinite(outs[0][0]).all() and np.abs(outs[0][0]).max() > 0
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
