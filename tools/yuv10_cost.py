"""NV21 and 10-bit (P010 / I010) input, measured: writes DIR/yuv10.txt (and prints it).  Nothing here is gated in advance except (c).

  (a) yuv_to_bgr of a resident 1920x1080 frame for nv12, nv21, p010 and i010, beside the bytes each must move (1.5 or 3 B/px read,
      3 B/px written) as a share of the 8 TB/s HBM peak and of the 6.3 TB/s a copy reaches on MI355X.  The entry is called
      through the C ABI into one preallocated output, so a call's host side is a ctypes call and a launch; a 2x2 frame gives the
      floor of that.  (A 1080p frame and its output fit the 256 MB Infinity Cache: the share says how far the call is from the
      HBM rate, not that HBM was the source.)
  (b) the YUV crop pre-path (preprocess_frame) for 8 people on that frame at 256x192, the same four formats.
  (c) the 8-bit regression check: NV12 yuv_to_bgr and the NV12 pre-path on the PARENT commit's library (--parent-lib, a built
      libhrnet_mi355.so of the parent) and on this tree's, in this process, alternating; one of them is measured twice (a second
      engine on this tree's library) and the difference between those two is the spread.  "No slowdown" = this - parent <= spread.

Device events around windows of at least a second each (the calls per window are calibrated per candidate), after a warm-up;
the candidates of a block take turns, round by round, in a rotated order; medians of the windows.

usage: python tools/yuv10_cost.py --out DIR [--parent-lib PATH] [--rounds R] [--window SECONDS]"""
import ctypes
import importlib
import os
import statistics
import sys

import costlib
from costlib import ROOT, window

ap = costlib.parser(__doc__, "yuv10.txt", rounds=5)
ap.add_argument("--parent-lib", help="libhrnet_mi355.so built from the parent commit: (c) is NOT MEASURED without it")
ap.add_argument("--window", type=float, default=1.0, help="seconds per window, at least")
args = ap.parse_args()
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np   # noqa: E402
import torch         # noqa: E402

import yuv10_ref     # noqa: E402  (the packers, and a YuvFrame by layout name)

pkg = importlib.import_module("simple-hrnet_amd")
L = importlib.import_module("simple-hrnet_amd._lib")
H, W, HF, WF, PEOPLE = 256, 192, 1080, 1920, 8
HBM_PEAK, HBM_COPY = 8.0e12, 6.3e12      # MI355X: spec, and what a float4 copy reaches
FORMATS = ("nv12", "nv21", "p010", "i010")

def engine(lib_path=None):
    """an engine on this tree's library, or on the library at `lib_path` (bound through the package's own symbol table)"""
    if lib_path is None:
        return pkg.NativeHRNet(32, 17, (H, W), "bf16", max_batch=PEOPLE, device=0)    # the pre-path needs no weights
    other = ctypes.CDLL(os.path.abspath(lib_path))
    for name, (res, argtypes) in L.SYMBOLS.items():
        fn = getattr(other, name)
        fn.restype, fn.argtypes = res, argtypes
    mine = L.load()
    L._lib = other
    try:
        return pkg.NativeHRNet(32, 17, (H, W), "bf16", max_batch=PEOPLE, device=0)
    finally:
        L._lib = mine


def frame_of(fmt, height=HF, width=WF, seed=11):
    rng = np.random.default_rng(seed)
    if fmt in ("nv12", "i420"):
        data = rng.integers(0, 256, height * width * 3 // 2, dtype=np.uint8)
    else:
        data = yuv10_ref.pack(*yuv10_ref.random_samples(rng, height, width, fmt), fmt, junk=rng)
    return yuv10_ref.frame(pkg, data, height, width, fmt, "bt709", "limited").to("cuda:0")   # (nv21: "nv12" with chroma_order="vu")


def boxes():
    rng = np.random.default_rng(5)
    dets = np.zeros((PEOPLE, 4), np.float32)
    for i in range(PEOPLE):
        bh = rng.integers(300, 900)
        bw = int(bh * rng.uniform(0.3, 0.6))
        x1, y1 = rng.uniform(0, WF - bw), rng.uniform(0, HF - bh)
        dets[i] = (x1, y1, x1 + bw, y1 + bh)
    return dets


def to_bgr_call(net, frame, out):
    """hrn_yuv_to_bgr of `frame` into `out` through the C ABI: no tensor is allocated, no device context entered"""
    entry = L.YuvFrameC()
    frame._fill(entry)
    fn, h, ref, ptr, stream = net._lib.hrn_yuv_to_bgr, net._h, ctypes.byref(entry), out.data_ptr(), net._stream()

    def call():
        if fn(h, ref, ptr, stream) != 0:
            raise RuntimeError(net._lib.hrn_last_error(h).decode())
    call.keep = (entry, frame, out)
    return call


def calibrated(cands):
    """ms per call of every candidate: args.rounds windows of at least args.window seconds each, interleaved in a rotated order"""
    reps = {}
    for k, fn in cands.items():                # warm-up (staging ring, scratch, clocks), then the calls a window needs
        window(fn, 200)
        per_call = window(fn, 2000)
        reps[k] = max(2000, int(args.window * 1e3 / per_call) + 1)
    samples = {k: [] for k in cands}
    for r in range(args.rounds):
        for k in costlib.rotated(cands, r):
            samples[k].append(window(cands[k], reps[k]))
    return samples, reps


report = costlib.Report(args.out, "yuv10.txt", "%9.3f us  (min %.3f .. max %.3f)", scale=1e3)
say, fmt_ms = report.say, report.fmt
say("NV21 / P010 / I010 input -- tools/yuv10_cost.py; %d windows of >= %.1f s per candidate, interleaved, device events, medians"
    % (args.rounds, args.window))
say("device: %s" % torch.cuda.get_device_name(0))
net = engine()
frames = {f: frame_of(f) for f in FORMATS}
out = torch.empty((HF, WF, 3), dtype=torch.uint8, device="cuda:0")
dets = boxes()
want = {f: net.yuv_to_bgr(frames[f]) for f in FORMATS}

# ---- (a)
tiny, tiny_out = frame_of("nv12", 2, 2), torch.empty((2, 2, 3), dtype=torch.uint8, device="cuda:0")
cands = {f: to_bgr_call(net, frames[f], out) for f in FORMATS}
cands["floor"] = to_bgr_call(net, tiny, tiny_out)
s, reps = calibrated(cands)
say()
say("(a) hrn_yuv_to_bgr of a resident %dx%d frame, BT.709 limited, one preallocated output" % (WF, HF))
say("    a 2x2 frame (the call's own floor: ctypes + launch)      %s" % fmt_ms(s["floor"]))
for f in FORMATS:
    nbytes = frames[f].nbytes + HF * WF * 3
    ms = statistics.median(s[f])
    rate = nbytes / (ms * 1e-3)
    say("    %-5s %5.2f MB in + %.2f MB out = %5.2f MB   %s   %6.2f TB/s = %4.1f %% of 8.0 TB/s peak, %4.1f %% of the 6.3 TB/s copy rate   [%d calls per window]"
        % (f, frames[f].nbytes / 1e6, HF * WF * 3 / 1e6, nbytes / 1e6, fmt_ms(s[f]), rate / 1e12, 100 * rate / HBM_PEAK, 100 * rate / HBM_COPY, reps[f]))
nv12_ms = statistics.median(s["nv12"])
say("    against nv12: " + ", ".join("%s x %.2f" % (f, statistics.median(s[f]) / nv12_ms) for f in FORMATS[1:]) +
    "   (a 10-bit frame is twice the bytes read: up to x 2 is its bandwidth)")

# ---- (b)
say()
crops = {f: net.preprocess_frame(frames[f], dets)[0] for f in FORMATS}
same = all(torch.equal(crops[f], net.preprocess_frame(want[f], dets)[0]) for f in FORMATS)
s, reps = calibrated({f: (lambda f=f: net.preprocess_frame(frames[f], dets)) for f in FORMATS})
say("(b) preprocess_frame, %d people of that frame, %dx%d crops, through the Python entry (crops equal the BGR path's bit for bit: %s)"
    % (PEOPLE, H, W, "yes" if same else "NO"))
for f in FORMATS:
    say("    %-5s %s   [%d calls per window]" % (f, fmt_ms(s[f]), reps[f]))
nv12_ms = statistics.median(s["nv12"])
say("    against nv12: " + ", ".join("%s x %.2f" % (f, statistics.median(s[f]) / nv12_ms) for f in FORMATS[1:]))

# ---- (c)
say()
if not args.parent_lib:
    say("(c) NV12 on the parent commit's library against this tree's: NOT MEASURED (no --parent-lib)")
else:
    parent, again = engine(args.parent_lib), engine()
    arms = {"parent": parent, "this": net, "this again": again}
    equal = all(torch.equal(e.yuv_to_bgr(frames["nv12"]), want["nv12"]) and torch.equal(e.preprocess_frame(frames["nv12"], dets)[0], crops["nv12"])
                for e in arms.values())
    say("(c) the 8-bit regression check: NV12 on the parent commit's library and on this tree's, one process, alternating windows")
    say("    (the parent's results equal this tree's bit for bit: %s; 'this again' = a second engine on this tree's library: the spread)" % ("yes" if equal else "NO"))
    outs = {k: torch.empty_like(out) for k in arms}
    verdicts = []
    for what, cands in (("hrn_yuv_to_bgr, 1080p NV12", {k: to_bgr_call(e, frames["nv12"], outs[k]) for k, e in arms.items()}),
                        ("preprocess_frame, %d people, NV12" % PEOPLE, {k: (lambda e=e: e.preprocess_frame(frames["nv12"], dets)) for k, e in arms.items()})):
        s, reps = calibrated(cands)
        say("    %s" % what)
        for k in arms:
            say("      %-10s %s   [%d calls per window]" % (k, fmt_ms(s[k]), reps[k]))
        med = {k: 1e3 * statistics.median(s[k]) for k in arms}
        spread, diff = abs(med["this"] - med["this again"]), med["this"] - med["parent"]
        verdict = "no slowdown beyond the spread" if diff <= spread else "SLOWER beyond the spread"
        verdicts.append(verdict)
        say("      this - parent = %+.3f us; spread (this against this again) = %.3f us -> %s" % (diff, spread, verdict))
    parent.close(), again.close()
net.close()
