"""The fp16 arithmetic mode on a CPU-only box: a plan-only fp16 handle has exactly the bf16 handle's plan (same kernels, tiles,
offsets, block maps), its packed weights are torch's fp16 rounding of the folded weights (subnormals kept, out-of-range weights
refused), the Python layer accepts the fp16 spellings, and the fp16 translation units of the hand-scheduled kernels keep the
invariants their bf16 twins are held to (tests/test_build_invariants.py)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import load_pkg, state_dict_np

pkg = load_pkg()
native = load_pkg("native")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simple-hrnet_amd", "csrc")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"

INFO_FIELDS = ["name", "cin", "cout", "ksize", "stride", "relu", "has_residual", "in_h", "in_w", "out_h", "out_w", "kpad", "nr",
               "algo", "ks", "w_offset", "w_bytes", "b_offset", "flops"]


def _net(model, c, res, dtype, mb):
    return pkg.NativeHRNet(c, 17, res, dtype, max_batch=mb, device=-1, model_name=model)


def test_plan_only_handle_in_fp16():
    net = _net("HRNet", 32, (64, 64), "fp16", 2)
    assert net.dtype == "fp16" and len(net.conv_infos()) > 0
    net.close()


def _maps(net, n):
    """every block map the plan has for a call of n crops: LDS-staged groups, generic groups, stride-2 groups (+ the fused stem)"""
    lib, out = net._lib, []
    blocks, members = np.zeros((60000, 3), np.int32), np.zeros(256, np.int32)
    group = 0
    while True:
        nb = lib.hrn_plan_block_map(net._h, group, n, group & 1, blocks.ctypes.data, len(blocks), members.ctypes.data, len(members))
        if nb < 0:
            break
        out.append(("block", group, blocks[:nb].copy(), members.copy()))
        group += 1
    px, group = ctypes.c_int32(0), 0
    while True:
        nb = lib.hrn_plan_direct_map(net._h, group, n, blocks.ctypes.data, len(blocks), members.ctypes.data, len(members),
                                     ctypes.byref(px))
        if nb < 0:
            break
        out.append(("direct", group, blocks[:nb].copy(), members.copy(), px.value))
        group += 1
    for group in range(-1, 64):
        b = (ctypes.c_int32 * (3 * 65536))()
        parts = (ctypes.c_int32 * (5 * 256))()
        act = ctypes.c_int32()
        r = lib.hrn_plan_s2_map(net._h, group, n, b, 65536, parts, 256, ctypes.byref(act))
        if r < 0:
            if group >= 0:
                break
            continue
        nb, npart = r & 0xfffff, r >> 20
        out.append(("s2", group, np.array(b[:3 * nb]), np.array(parts[:5 * npart]), act.value))
    return out


@pytest.mark.parametrize("model,c,res,mb", [("HRNet", 48, (384, 288), 256), ("HRNet", 32, (256, 192), 32),
                                            ("PoseResNet", 50, (256, 192), 32)])
def test_fp16_plan_equals_bf16_plan(model, c, res, mb):
    a, b = _net(model, c, res, "bf16", mb), _net(model, c, res, "fp16", mb)
    ia, ib = a.conv_infos(), b.conv_infos()
    assert len(ia) == len(ib) > 0
    for x, y in zip(ia, ib):
        assert [getattr(x, f) for f in INFO_FIELDS] == [getattr(y, f) for f in INFO_FIELDS], x.name
    assert a.weight_blob_bytes() == b.weight_blob_bytes()
    assert a.launches_per_pass() == b.launches_per_pass()
    for n in (1, 7, mb):
        ma, mb_ = _maps(a, n), _maps(b, n)
        assert len(ma) == len(mb_) > 0
        for x, y in zip(ma, mb_):
            assert x[0] == y[0] and x[1] == y[1]
            for u, v in zip(x[2:], y[2:]):
                assert np.array_equal(np.asarray(u), np.asarray(v)), (x[0], x[1], n)
    a.close()
    b.close()


# ---- fold and pack ---------------------------------------------------------------------------------------------------------
def _f16(raw):
    return raw.view(np.float16).astype(np.float32)


def _unpack(net, info):
    """fp32 values of a convolution's 16-bit image, as an (cout, 9 * cin or kpad) matrix (the generic
    fragment-major image; algo 1 / 2 / 3: the slice-major image of the LDS-staged kernel and its 96-cout form)"""
    raw = net.read_blob(info.w_offset, info.w_bytes)
    vals = _f16(raw)
    if info.algo in (1, 2, 3):   # (2: a member of a fused BasicBlock -- the same image)
        ks, nrb = info.ks, info.nr
        slices, ntiles, nch = info.cin // ks, info.cout // (16 * nrb), (9 * ks + 31) // 32
        vals = vals.reshape(ntiles, slices, nch, nrb, 64, 8)
        out = np.zeros((info.cout, 9 * info.cin), np.float32)
        for t in range(ntiles):
            for s in range(slices):
                for c in range(nch):
                    for j in range(nrb):
                        for lane in range(64):
                            li, g = lane & 15, lane >> 4
                            co = t * 16 * nrb + (li >> 2) * 4 * nrb + j * 4 + (li & 3)
                            if info.algo == 3:
                                co = t * 96 + (j >> 1) * 32 + (li >> 2) * 8 + (j & 1) * 4 + (li & 3)
                            for e in range(8):
                                kl = 32 * c + 8 * g + e
                                if kl < 9 * ks:
                                    out[co, (kl // ks) * info.cin + s * ks + kl % ks] = vals[t, s, c, j, lane, e]
                                else:
                                    assert vals[t, s, c, j, lane, e] == 0
        return out
    kchunks = info.kpad // 32
    vals = vals.reshape(info.cout // 16, kchunks, 64, 8)
    out = np.zeros((info.cout, info.kpad), np.float32)
    for f in range(info.cout // 16):
        ng, j = divmod(f, info.nr)
        for lane in range(64):
            li, g = lane & 15, lane >> 4
            co = ng * 16 * info.nr + (li >> 2) * 4 * info.nr + j * 4 + (li & 3)
            for k in range(kchunks):
                out[co, k * 32 + g * 8:k * 32 + (g + 1) * 8] = vals[f, k, lane]
    return out


def _folded(sd, conv, bn):
    w = sd[conv + ".weight"].astype(np.float64)
    scale = sd[bn + ".weight"].astype(np.float64) / np.sqrt(sd[bn + ".running_var"].astype(np.float64) + 1e-5)
    cout, cin, kh, kw = w.shape
    return (w * scale[:, None, None, None]).transpose(0, 2, 3, 1).reshape(cout, kh * kw * cin).astype(np.float32)


CASES = [("conv2", "bn2"), ("layer1.0.conv1", "layer1.0.bn1"), ("transition1.0.0", "transition1.0.1"),
         ("stage2.0.branches.0.0.conv1", "stage2.0.branches.0.0.bn1"),
         ("stage3.1.branches.1.3.conv2", "stage3.1.branches.1.3.bn2"),
         ("stage4.0.fuse_layers.3.0.2.0", "stage4.0.fuse_layers.3.0.2.1"),
         ("stage4.2.fuse_layers.0.3.0", "stage4.2.fuse_layers.0.3.1")]


def _check_pack(sd, c=48, res=(64, 64)):
    net = _net("HRNet", c, res, "fp16", 1).load_state_dict(sd)
    infos = {i.name.decode(): i for i in net.conv_infos()}
    n_sub = 0
    for conv, bn in CASES:
        info = infos[conv]
        want = torch.from_numpy(_folded(sd, conv, bn)).to(torch.float16)
        n_sub += int(((want != 0) & (want.abs() < 2.0 ** -14)).sum())
        got = torch.from_numpy(_unpack(net, info)).to(torch.float16)   # (exact: every fp16 value is an fp32 value)
        assert torch.equal(got[:, :want.shape[1]].view(torch.int16), want.view(torch.int16)), conv
        assert not got[:, want.shape[1]:].any()
    net.close()
    return n_sub


def test_fold_and_pack_is_torch_fp16_rounding():
    _check_pack(state_dict_np(48))


def test_fold_and_pack_keeps_fp16_subnormals():
    sd = dict(state_dict_np(48))
    for k in list(sd):
        if k.endswith(".weight") and sd[k].ndim == 4:
            sd[k] = sd[k] * np.float32(2.0 ** -12)   # folded weights around 1e-5 .. 1e-4: many below 2^-14
    assert _check_pack(sd) > 1000


def test_out_of_range_weight_is_refused():
    sd = dict(state_dict_np(32))
    w = sd["stage2.0.branches.0.0.conv1.weight"].copy()
    w[0, 0, 0, 0] = 1e6
    sd["stage2.0.branches.0.0.conv1.weight"] = w
    net = _net("HRNet", 32, (64, 64), "fp16", 1)
    with pytest.raises(KeyError, match="65504"):
        net.load_state_dict(sd)
    net.close()
    pkg.NativeHRNet(32, 17, (64, 64), "bf16", max_batch=1, device=-1).load_state_dict(sd).close()   # bf16 has the range


# ---- Python layer ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alias", ["fp16", "f16", "float16", "half", torch.float16])
def test_dtype_aliases(alias):
    assert native.DTYPES[alias] == 2
    net = pkg.NativeHRNet(32, 17, (64, 64), alias, max_batch=1, device=-1)
    assert net.dtype == "fp16"
    net.close()


def test_bad_dtype_message_names_all_three():
    with pytest.raises(ValueError) as e:
        pkg.NativeHRNet(32, 17, (64, 64), "int8", device=-1)
    assert all(d in str(e.value) for d in ("bf16", "fp16", "fp32"))


def test_simple_hrnet_constructs_in_fp16(monkeypatch):
    sh = load_pkg("simple_hrnet")
    made = []

    class Probe:
        def __init__(self, c, nof_joints, resolution, dtype, **kw):
            made.append(dtype)
            self.real = pkg.NativeHRNet(c, nof_joints, resolution, dtype, max_batch=kw.get("max_batch", 1), device=-1)
            self.dtype = self.real.dtype

        def load_state_dict(self, sd):
            self.real.load_state_dict(sd)
            return self

    monkeypatch.setattr(sh, "NativeHRNet", Probe)
    monkeypatch.setattr(sh, "resolve_devices", lambda device: [0])
    model = sh.SimpleHRNet(32, 17, state_dict_np(32), resolution=(64, 64), multiperson=False, dtype="fp16", device="cuda:0")
    assert made == ["fp16"] and model.model.dtype == "fp16"
    model.model.real.close()


# ---- the fp16 translation units ------------------------------------------------------------------------------------------------
def _hipcc():
    h = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(h) or not os.path.exists(OBJDUMP):
        pytest.skip("no hipcc / llvm-objdump")
    return h


_CACHE = {}


def _compile(source, tmp):
    """-> ({kernel: resource usage}, {kernel: [instruction]}) of the gfx950 device code of `source`"""
    if source in _CACHE:
        return _CACHE[source]
    obj = os.path.join(tmp, source + ".o")
    out = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "--no-gpu-bundle-output",
                          "-c", os.path.join(CSRC, source), "-o", obj, "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    use, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            use[name] = {}
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            use[name][m.group(1).strip()] = int(m.group(2))
    text = subprocess.run([OBJDUMP, "-d", obj], capture_output=True, text=True, timeout=300).stdout
    asm, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = asm.setdefault(m.group(1), [])
            continue
        if cur is not None and "//" in line and line[:1] in " \t":
            ins, _, tail = line.partition("//")
            m = re.match(r"\s*([0-9A-F]+):", tail)
            if m and ins.strip():
                cur.append((int(m.group(1), 16), re.sub(r"\s+", " ", ins).strip()))
    _CACHE[source] = (use, asm)
    return use, asm


def _twin(name):
    """the bf16 kernel's symbol for an fp16 one: the element-format template argument is the last one, 2 -> 1"""
    return re.sub(r"Li2EEEv", "Li1EEEv", name)


def _mfma(ins, fmt):
    return sum(t.startswith("v_mfma_f32_16x16x32_" + fmt + " ") for _, t in ins)


@pytest.mark.parametrize("pair,pattern,count", [(("conv3x3_lds.hip", "conv3x3_lds_f16.hip"), "conv3x3_lds_kernel", 4),
                                                (("bottleneck_chain.hip", "bottleneck_chain_f16.hip"), "bottleneck_chain_kernel", 4),
                                                (("conv_s2.hip", "conv_s2_f16.hip"), "conv_s2_slab_kernel", 1)])
def test_fp16_kernels_mirror_their_bf16_twins(pair, pattern, count, tmp_path):
    use16, asm16 = _compile(pair[1], str(tmp_path))
    _, asmbf = _compile(pair[0], str(tmp_path))
    k16 = {k: v for k, v in asm16.items() if pattern in k}
    assert len(k16) == count
    for name, ins in k16.items():
        u = use16[name]
        assert u["ScratchSize"] == 0 and u.get("VGPRs Spill", 0) == 0, (name, u)
        assert u["VGPRs"] <= 256 and u["Occupancy"] >= 2 or pattern == "bottleneck_chain_kernel", (name, u)
        twin = asmbf[_twin(name)]
        n = _mfma(ins, "f16")
        print("%s: %d fp16 MFMAs (bf16 twin %d)" % (name[:60], n, _mfma(twin, "bf16")))
        assert n > 0 and n == _mfma(twin, "bf16") and _mfma(ins, "bf16") == 0 and not any("bf16" in t for _, t in ins)
        assert not any("cvt_pkrtz" in t for _, t in ins)
        if pattern == "conv_s2_slab_kernel":
            ops = [t.split()[0] for _, t in ins]
            assert ops.count("global_store_dwordx4") == 6 and ops.count("global_store_dwordx2") == 2


def test_fp16_basicblock_kernel_keeps_the_hand_scheduled_invariants(tmp_path):
    """test_build_invariants.py's counted-wait table, s100 / s101 and M0 rules on the fp16 <48, 3> kernel"""
    _, asm = _compile("conv3x3_lds_f16.hip", str(tmp_path))
    (ins,) = [v for k, v in asm.items() if "conv3x3_lds_kernelILi48ELi3ELi2E" in k]
    sites = [i for i, (_, t) in enumerate(ins) if t.startswith("s_getpc_b64 s[100:101]")]
    assert len(sites) >= 2
    for i in sites:
        a = ins[i][0] + 4
        head = [t.split()[0] for _, t in ins[i + 1:i + 6]]
        assert head == ["s_lshl_b32", "s_add_u32", "s_add_u32", "s_addc_u32", "s_setpc_b64"], head
        assert ins[i + 1][1].endswith(", 3") and ins[i + 2][1].endswith(", 20")
        ends = set()
        for k in range(24):
            (aw, tw), (ab, tb) = ins[i + 6 + 2 * k], ins[i + 7 + 2 * k]
            assert aw == a + 20 + 8 * k and tw == "s_waitcnt vmcnt(%d)" % k, (k, hex(aw), tw)
            assert ab == aw + 4 and tb.startswith("s_branch "), (k, tb)
            ends.add(ab + 4 + 4 * int(tb.split()[1]))
        assert ends == {a + 20 + 8 * 24}, ends
    allowed = ("s_getpc_b64 s[100:101]", "s_add_u32 s100, s100,", "s_addc_u32 s101, s101, 0", "s_setpc_b64 s[100:101]")
    for _, t in ins:
        if re.search(r"\bs10[01]\b|s\[100:101\]|s\[100:10[2-9]\]|s\[9[6-9]:10[0-9]\]", t):
            assert t.startswith(allowed), t
    m0_readers = ("global_load_lds", "buffer_load", "ds_gws", "s_sendmsg", "s_movrel", "v_movrel", "v_interp", "ds_add_gs", "ds_sub_gs",
                  "ds_read_addtid", "ds_write_addtid", "s_ttrace")
    n_dma = 0
    for i, (_, t) in enumerate(ins):
        op = t.split()[0]
        operands = t.replace(",", " ").split()[1:]
        if "m0" in operands:
            assert op.startswith("s_") and operands[0] == "m0" and "m0" not in operands[1:], t
        if op.startswith(m0_readers):
            assert op.startswith("global_load_lds"), t
            n_dma += 1
            prev = [x for _, x in ins[max(0, i - 48):i]]
            assert any(re.match(r"s_\w+ m0,", x) for x in prev), (t, prev[-4:])
    assert n_dma > 20


def test_no_round_toward_zero_conversion_anywhere(tmp_path):
    for src in ("kernels.hip", "stem_fused.hip", "conv3x3_lds_f16.hip", "conv_s2_f16.hip", "bottleneck_chain_f16.hip"):
        _, asm = _compile(src, str(tmp_path))
        assert not any("cvt_pkrtz" in t for ins in asm.values() for _, t in ins), src
    _, asm = _compile("kernels.hip", str(tmp_path))
    for kind in ("stem_mfma_kernel", "stem7_mfma_kernel", "head_mfma_kernel"):
        (ins,) = [v for k, v in asm.items() if kind + "ILi2E" in k]
        assert _mfma(ins, "f16") > 0 and _mfma(ins, "bf16") == 0, kind
