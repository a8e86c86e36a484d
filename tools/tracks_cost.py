"""The person track table on the GPU, measured: writes DIR/track_table.txt (and prints it).  No number here is a gate: what one
update of the table costs beside associate_people on the same people, beside the host round trip it replaces, and with half the
table lost (the matrix is then twice as wide) are results to record.

  (a) NativeHRNet.track_people (one launch, demo parameters, max_lost 5, coast on) at 8, 64 and 256 people per stream with J = 17
      and at 64 with J = 133, every row a jittered copy of a seen track, against
        - NativeHRNet.associate_people on the same people (previous frame = the tracks);
        - the host round trip: download pts and boxes, postproc.track_people on a host table, upload ids, pts and boxes;
        - the same update on a table twice as full, the other half lost.
      HIP events around back-to-back calls, host side included, interleaved (round r runs the candidates in a rotated order),
      medians.  Every call starts from the same table and the frame's own boxes and joints (refresh copies, timed on their own).
  (b) --ab-root DIR: predict_frame (8 people, HRNet-W32 256x192 bf16) and bench.py in THIS tree against the checkout at DIR (the
      parent commit, built): costlib.ab, the protocol of tools/README.md.  Without --ab-root: NOT MEASURED.

usage: python tools/tracks_cost.py --out DIR [--rounds R] [--reps K] [--ab-root DIR]"""
import importlib
import statistics
import sys

import costlib
from costlib import people_of, timed

args = costlib.parser(__doc__, "track_table.txt", rounds=9, reps=20, ab="predict_frame and bench.py").parse_args()
sys.path.insert(0, costlib.ROOT)
import numpy as np   # noqa: E402
import torch         # noqa: E402

pkg = importlib.import_module("simple-hrnet_amd")
report = costlib.Report(args.out, "track_table.txt")
say, fmt = report.say, report.fmt

say("person track table -- tools/tracks_cost.py; %d samples of %d calls per candidate, interleaved, HIP events, host side included, medians"
    % (args.rounds, args.reps))
say("device: %s" % torch.cuda.get_device_name(0))
net = pkg.NativeHRNet(32, 17, (64, 64), "bf16", max_batch=1, device=0)   # the table needs no weights
pp = pkg.postproc
alpha, thr, smooth, max_lost, coast, va = 0.2, 0.4, 0.1, 5, True, 0.5    # scripts/live-demo.py:122 and the table's own three

say()
say("(a) track_people, demo parameters (pose_alpha %.1f, threshold %.1f, smoothing %.1f), max_lost %d, coast on; every row a jittered copy"
    % (alpha, thr, smooth, max_lost))
say("    of a seen track in shuffled order; C = 256.  host round trip = download pts + boxes, postproc.track_people, upload ids + pts + boxes")
for count, joints in ((8, 17), (64, 17), (256, 17), (64, 133)):
    prev_pts, prev_boxes = people_of(count, joints, count)
    order = np.random.default_rng(count).permutation(count)
    cur_pts, cur_boxes = people_of(count, joints, count + 1, jitter=3.0, base=prev_pts[order])

    def table_of(lost):
        """the `count` tracks seen in the previous update, then `lost` more that have been lost for two updates"""
        t = pp.new_track_table(1, 256, joints)
        t["slot_id"][0, :count], t["slot_row"][0, :count], t["slot_hits"][0, :count] = np.arange(count), np.arange(count), 3
        t["slot_boxes"][0, :count], t["slot_pts"][0, :count] = prev_boxes, prev_pts
        if lost:
            g_pts, g_boxes = people_of(lost, joints, 7 * count)
            t["slot_id"][0, count:count + lost], t["slot_lost"][0, count:count + lost] = np.arange(count, count + lost), 2
            t["slot_hits"][0, count:count + lost] = 3
            t["slot_boxes"][0, count:count + lost], t["slot_pts"][0, count:count + lost] = g_boxes, g_pts
        t["next_id"][0] = count + lost
        return t

    half = min(count, 256 - count)            # (at 256 per stream the table is full of seen tracks: nobody can be lost beside them)
    tables = {"seen": table_of(0), "half lost": table_of(half)}
    master = {k: {n: torch.from_numpy(v).cuda() for n, v in t.items()} for k, t in tables.items()}
    work = {k: {n: v.clone() for n, v in t.items()} for k, t in master.items()}
    dev = [torch.from_numpy(v).cuda() for v in (cur_boxes, cur_pts, prev_boxes, prev_pts, np.arange(count, dtype=np.int32))]
    work_boxes, work_pts = dev[0].clone(), dev[1].clone()
    next_id = torch.tensor([count], dtype=torch.int32, device="cuda")
    pin_boxes, pin_pts = torch.empty_like(dev[0], device="cpu").pin_memory(), torch.empty_like(dev[1], device="cpu").pin_memory()
    host_master = tables["seen"]
    host_work = {n: v.copy() for n, v in host_master.items()}

    def refresh(which):
        work_boxes.copy_(dev[0]), work_pts.copy_(dev[1])
        if which:
            for n, v in master[which].items():
                work[which][n].copy_(v)

    def table_call(which):
        refresh(which)
        return net.track_people(work_boxes, work_pts, work[which], alpha, thr, smooth, max_lost, coast, va)

    def assoc_call():
        refresh(None)
        return net.associate_people(work_boxes, work_pts, dev[2], dev[3], dev[4], next_id, alpha, thr, smooth)

    def host_call():
        pin_boxes.copy_(dev[0], non_blocking=True), pin_pts.copy_(dev[1], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        for n, v in host_master.items():
            host_work[n][...] = v
        b, p, ids, _, _, _ = pp.track_people(pin_boxes.numpy(), pin_pts.numpy(), host_work, alpha, thr, smooth, max_lost, coast, va)
        work_boxes.copy_(torch.from_numpy(b), non_blocking=True), work_pts.copy_(torch.from_numpy(p), non_blocking=True)
        return torch.from_numpy(ids).cuda(non_blocking=True)

    matched = int((table_call("seen")[3] >= 0).sum()), int((table_call("half lost")[3] >= 0).sum())
    reps = args.reps if count < 256 else max(2, args.reps // 4)
    s = timed({"table": lambda: table_call("seen"), "wide": lambda: table_call("half lost"), "assoc": assoc_call, "host": host_call,
               "refresh table": lambda: refresh("seen"), "refresh rows": lambda: refresh(None)}, args.rounds, reps)
    med = {k: statistics.median(v) for k, v in s.items()}
    say("    %3d people, J = %d (%d / %d matched)" % (count, joints, matched[0], matched[1]))
    say("        track_people                         %s" % fmt(s["table"]))
    say("        track_people, %3d more tracks lost    %s   (%d columns)" % (half, fmt(s["wide"]), count + half))
    say("        associate_people on the same people  %s" % fmt(s["assoc"]))
    say("        host round trip                      %s" % fmt(s["host"]))
    say("        refresh copies: table + rows         %s   (in both track_people lines; not part of a video loop)" % fmt(s["refresh table"]))
    say("        refresh copies: rows only            %s   (in the associate_people line)" % fmt(s["refresh rows"]))
    say("        less their refresh copies: track_people %.4f ms, associate_people %.4f ms -> %.2f x; track_people / host round trip = %.3f"
        % (med["table"] - med["refresh table"], med["assoc"] - med["refresh rows"],
           (med["table"] - med["refresh table"]) / max(med["assoc"] - med["refresh rows"], 1e-9), med["table"] / med["host"]))
net.close()

say()
runs = costlib.ab(report, "(b)", ["predict"], args.ab_root, args.ab_pairs, args.rounds, args.reps, bench=True)
say()
say("Not claimed: how well these ids hold on a trained network -- no trained weights and no video exist where this was measured.")
sys.exit(runs is None)
