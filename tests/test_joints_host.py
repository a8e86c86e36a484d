"""Heads with more than 32 joints, host side (plan-only handles, no GPU): the create-time bound, the grouped weight image of the
head, and the symbols.  The GPU side is tests/test_joints_gpu.py."""
import re
import os

import numpy as np
import pytest

from conftest import ROOT, load_pkg


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def header_bound():
    text = open(os.path.join(ROOT, "include", "hrnet_mi355.h")).read()
    m = re.search(r"^#define\s+HRN_MAX_JOINTS\s+(\d+)\s*$", text, re.M)
    assert m, "include/hrnet_mi355.h does not define HRN_MAX_JOINTS"
    return int(m.group(1))


MODELS = [("HRNet", 32), ("HRNet", 48), ("PoseResNet", 50)]


@pytest.mark.parametrize("model,c", MODELS)
def test_create_accepts_up_to_the_bound(pkg, model, c):
    bound = header_bound()
    assert bound >= 160
    for J in (33, 64, 65, 133, bound):
        net = pkg.NativeHRNet(c, J, (64, 64), "bf16", max_batch=2, device=-1, model_name=model)
        assert net.nof_joints == J and net.weight_blob_bytes() > 0
        net.close()
    with pytest.raises(ValueError, match=r"HRN_MAX_JOINTS = %d" % bound):
        pkg.NativeHRNet(c, bound + 1, (64, 64), "bf16", max_batch=2, device=-1, model_name=model)
    with pytest.raises(ValueError, match="HRN_MAX_JOINTS"):
        pkg.NativeHRNet(c, 0, (64, 64), "bf16", max_batch=2, device=-1, model_name=model)


def align256(x):
    return (x + 255) // 256 * 256


def head_tail(net, J, head_c):
    """(offset of the fp32 [J][c] weights, of the biases, of the MFMA image, bytes of one group's image): final_layer is the
    tail of the blob (include/hrnet_mi355.h)"""
    group_bytes = 2 * ((head_c + 31) // 32) * 1024
    wp = net.weight_blob_bytes() - (J + 31) // 32 * group_bytes
    b = wp - align256(4 * J)
    return b - align256(4 * J * head_c), b, wp, group_bytes


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("model,c,head_c", [("HRNet", 32, 32), ("HRNet", 48, 48), ("PoseResNet", 50, 256)])
def test_group_image_is_the_image_of_a_head_of_those_joints(pkg, dtype, model, c, head_c):
    J = 133
    sd = pkg.synth_state_dict(c, J, 4, model=model)
    full = pkg.NativeHRNet(c, J, (64, 64), dtype, max_batch=1, device=-1, model_name=model).load_state_dict(sd)
    w_off, b_off, wp_off, gb = head_tail(full, J, head_c)
    fw = full.read_blob(w_off, 4 * J * head_c).view(np.float32).reshape(J, head_c)
    fb = full.read_blob(b_off, 4 * J).view(np.float32)
    np.testing.assert_array_equal(fw, np.asarray(sd["final_layer.weight"], np.float32).reshape(J, head_c))
    np.testing.assert_array_equal(fb, np.asarray(sd["final_layer.bias"], np.float32))
    body = full.read_blob(0, w_off)
    for g in range((J + 31) // 32):
        rows = slice(32 * g, min(32 * g + 32, J))
        jg = rows.stop - rows.start
        part = dict(sd)
        part["final_layer.weight"] = np.ascontiguousarray(sd["final_layer.weight"][rows])
        part["final_layer.bias"] = np.ascontiguousarray(sd["final_layer.bias"][rows])
        small = pkg.NativeHRNet(c, jg, (64, 64), dtype, max_batch=1, device=-1, model_name=model).load_state_dict(part)
        sw, sb, swp, sgb = head_tail(small, jg, head_c)
        assert sgb == gb and small.weight_blob_bytes() - swp == gb            # one group: the two-fragment image of old
        assert sw == w_off                                                     # everything in front of the head is laid out alike
        np.testing.assert_array_equal(small.read_blob(0, sw), body)
        np.testing.assert_array_equal(small.read_blob(swp, gb), full.read_blob(wp_off + g * gb, gb))
        np.testing.assert_array_equal(small.read_blob(sw, 4 * jg * head_c).view(np.float32).reshape(jg, head_c), fw[rows])
        np.testing.assert_array_equal(small.read_blob(sb, 4 * jg).view(np.float32), fb[rows])
        if jg < 32:   # the last group: 5 rows, the other 27 of its two fragments zero
            img = full.read_blob(wp_off + g * gb, gb).view(np.uint16).reshape(2, -1, 64, 8)
            lanes_of_row = np.arange(64) % 16
            assert not img[0][:, lanes_of_row >= jg].any() and not img[1].any()
            assert img[0][:, lanes_of_row < jg].any()
        small.close()
    full.close()


def test_j17_blob_and_launches_are_those_of_one_group(pkg):
    """J <= 32 is one group: the head's image stays two fragments, and the blob of a 17- and of a 32-joint model differ by the
    fp32 rows alone"""
    a = pkg.NativeHRNet(48, 17, (128, 96), "bf16", max_batch=2, device=-1)
    b = pkg.NativeHRNet(48, 32, (128, 96), "bf16", max_batch=2, device=-1)
    c = pkg.NativeHRNet(48, 33, (128, 96), "bf16", max_batch=2, device=-1)
    assert b.weight_blob_bytes() - a.weight_blob_bytes() == align256(4 * 32 * 48) - align256(4 * 17 * 48)
    assert c.weight_blob_bytes() - b.weight_blob_bytes() == align256(4 * 33 * 48) - align256(4 * 32 * 48) + 2 * 2 * 1024
    assert a.launches_per_pass() == b.launches_per_pass() == c.launches_per_pass()
    for net in (a, b, c):
        net.close()


def test_fp16_overflow_is_checked_in_every_group(pkg):
    sd = dict(pkg.synth_state_dict(32, 133, 1))
    w = np.array(sd["final_layer.weight"], np.float32)
    w[130].flat[3] = 7e4            # a row of the last group
    sd["final_layer.weight"] = w
    with pytest.raises(KeyError, match="65504"):
        pkg.NativeHRNet(32, 133, (64, 64), "fp16", max_batch=1, device=-1).load_state_dict(sd)
    pkg.NativeHRNet(32, 133, (64, 64), "bf16", max_batch=1, device=-1).load_state_dict(sd).close()


def test_symbols(pkg):
    lib = load_pkg("_lib")
    assert header_bound() == 256
    handle = lib.load()
    for name in lib.header_symbols():
        assert hasattr(handle, name), name
    assert set(lib.header_symbols()) == set(lib.SYMBOLS)
