"""Joints over time on the GPU, measured: writes DIR/temporal_filter.txt (and prints it).  No time is fixed in advance; everything
is reported as seen.

  (a) NativeHRNet.filter_poses on RESIDENT joints, state and match, against the round trip it replaces: download of pts, state and
      match, postproc.filter_poses on the host, upload of the filtered joints, the prediction and the new state (pinned buffers on
      both ways) -- at 8, 64 and 256 people with J = 17 and at 64 people with J = 133.  Beside each timing of the call: the floor of
      moving its bytes once at 6.15 TB/s (12 read + 24 + 4 gathered + 12 + 12 + 24 + 4 written per joint, 4 per person), and a bare
      kernel-sized launch for scale (torch's copy of the same joints).
  (b) --ab-root DIR: predict_frame (8 people, HRNet-W32 256x192 bf16) in THIS tree against the checkout at DIR (the parent commit,
      built): costlib.ab, the protocol of tools/README.md.  Without --ab-root: NOT MEASURED.
  HIP events around back-to-back calls, host side included, interleaved (round r runs the candidates in a rotated order), medians
  with the spread of the samples beside them.

usage: python tools/temporal_cost.py --out DIR [--rounds R] [--reps K] [--ab-root DIR]"""
import importlib
import statistics
import sys

import costlib
from costlib import timed

args = costlib.parser(__doc__, "temporal_filter.txt", rounds=9, reps=50, ab="predict_frame").parse_args()
sys.path.insert(0, costlib.ROOT)
import numpy as np   # noqa: E402
import torch         # noqa: E402

HBM = 6.15e12   # bytes per second: the floor printed beside the timings
pkg = importlib.import_module("simple-hrnet_amd")
report = costlib.Report(args.out, "temporal_filter.txt", "%9.4f ms  (min %.4f .. max %.4f)")
say, fmt = report.say, report.fmt

say("joints over time -- tools/temporal_cost.py; %d samples of %d calls per candidate, interleaved, HIP events, host side included, medians"
    % (args.rounds, args.reps))
say("device: %s" % torch.cuda.get_device_name(0))
net = pkg.NativeHRNet(32, 17, (64, 64), "bf16", max_batch=1, device=0)   # the filter needs no weights
pp = pkg.postproc
say()
say("(a) filter_poses on resident tensors against the round trip it replaces (pts, state, match down; postproc.filter_poses; filtered")
say("    joints, prediction and state up; pinned buffers), one stream of people matched one to one")
lost = []
for n, J in ((8, 17), (64, 17), (256, 17), (64, 133)):
    rng = np.random.default_rng(n + J)
    before = np.concatenate([rng.uniform(0, 1000, (n, J, 2)), rng.uniform(0.5, 1.0, (n, J, 1))], 2).astype(np.float32)
    now = before.copy()
    now[:, :, :2] += rng.normal(0, 2, (n, J, 2)).astype(np.float32)
    match = rng.permutation(n).astype(np.int32)
    now = np.ascontiguousarray(now[match])                   # person i of this frame is person match[i] of the previous one
    _, _, state = pp.filter_poses(before)
    want = pp.filter_poses(now, state, match)
    d_pts, d_match = torch.from_numpy(now).cuda(), torch.from_numpy(match).cuda()
    d_state = tuple(torch.from_numpy(s).cuda() for s in state)
    got = net.filter_poses(d_pts, d_state, d_match)
    assert np.array_equal(got[0].cpu().numpy().view(np.uint32), want[0].view(np.uint32)) and \
        np.array_equal(got[2][0].cpu().numpy().view(np.uint32), want[2][0].view(np.uint32)), "the device call disagrees with the host form"
    pins = [torch.empty(t.shape, dtype=t.dtype).pin_memory() for t in (d_pts, d_state[0], d_state[1], d_match)]
    ups = [torch.empty(s, dtype=t).pin_memory() for s, t in (((n, J, 3), torch.float32), ((n, J, 3), torch.float32), ((n, J, 6), torch.float32),
                                                             ((n, J), torch.int32))]

    def round_trip():
        for pin, t in zip(pins, (d_pts, d_state[0], d_state[1], d_match)):
            pin.copy_(t, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        out, pred, (values, age) = pp.filter_poses(pins[0].numpy(), (pins[1].numpy(), pins[2].numpy()), pins[3].numpy())
        for up, a in zip(ups, (out, pred, values, age)):
            up.copy_(torch.from_numpy(a))
        return [up.cuda(non_blocking=True) for up in ups]

    s = timed({"device": lambda: net.filter_poses(d_pts, d_state, d_match), "round trip": round_trip, "torch copy": lambda: d_pts.clone()},
              args.rounds, args.reps)
    ours, theirs = statistics.median(s["device"]), statistics.median(s["round trip"])
    moved = n * J * (12 + 24 + 4 + 12 + 12 + 24 + 4) + n * 4
    floor = moved / HBM * 1e3
    say("    %3d people, J = %3d" % (n, J))
    say("        filter_poses on the device   %s   bytes floor %.6f ms (%.1f KB at 6.15 TB/s): %.0f x the floor -- launch-bound"
        % (fmt(s["device"]), floor, moved / 1e3, ours / floor))
    say("        round trip through the host  %s   device / round trip = %.3f%s"
        % (fmt(s["round trip"]), ours / theirs, "" if ours <= theirs else "   <-- the device call LOSES here"))
    say("        one torch copy of the joints %s   (a bare launch from Python, for scale)" % fmt(s["torch copy"]))
    if ours > theirs:
        lost.append("%d x %d" % (n, J))
say("    the device call %s" % ("won at every size" if not lost else "LOST at " + ", ".join(lost)))
net.close()

say()
runs = costlib.ab(report, "(b)", ["predict"], args.ab_root, args.ab_pairs, args.rounds, max(args.reps // 2, 2))   # (a pass is no small call)
say()
say("Not claimed: that filtered joints or predicted boxes improve accuracy or tracking on a trained network (no weights, no video here).")
sys.exit(runs is None)
