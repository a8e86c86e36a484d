"""Cost of a head with more than 32 joints on the headline shape (HRNet-W48, 384x288, one micro-batch of 256 crops, bf16).
Three measurements, each from child processes of this one (one GPU process at a time, every child under its own time limit; the
first child that fails ends the run):

  1. the whole pass at J = 17, this library against a tagged variant built from the parent commit (HRN_LIB_TAG, see
     tools/build_variant.py): costlib.ab, the protocol of tools/README.md; every child takes `--rounds` samples of `--reps` passes.
  2. the head launch alone, `rocprofv3 --kernel-trace --stats`, one traced child per (J, heat-maps written or not): J = 17 and
     J = 133.  Against 5 x the J = 17 launch (the naive form: one launch per joint group) and against the floor of its bytes at
     the project's measured 6.15 TB/s (input read once + 4 * J * h * w per crop where maps are written).
  3. the pass at J = 133 against J = 17 in ONE process, refine None and "dark", rotated order.

usage: python tools/head_joints_cost.py --out DIR [--parent-tag parent] [--rounds R] [--reps K]   -> DIR/head_joints.txt; a missing
variant library skips measurement 1 and says so."""
import importlib
import json
import os
import statistics
import sys

import costlib

sys.path.insert(0, costlib.ROOT)
C, H, W, N = 48, 384, 288, 256
HBM_BPS = 6.15e12          # the project's measured streaming rate (profiles/README.md)
GROUP = 32


def engine(pkg, J):
    return pkg.NativeHRNet(C, J, (H, W), "bf16", max_batch=N, device=0).load_state_dict(pkg.synth_state_dict(C, J, 0))


def inputs(pkg):
    import torch
    crops = torch.randn((N, 3, H, W), generator=torch.Generator(device="cuda").manual_seed(1234), device="cuda")
    return crops, torch.from_numpy(pkg.synth_boxes(N)).cuda()


def child_pass17(args):
    """median ms per pass of predict_crops at J = 17 with whatever library HRN_LIB_TAG selects"""
    pkg = importlib.import_module("simple-hrnet_amd")
    net = engine(pkg, 17)
    crops, boxes = inputs(pkg)
    s = costlib.timed({"pass17": lambda: net.predict_crops(crops, boxes)}, args.rounds, args.reps, warmup=4)
    print(json.dumps({"pass17": statistics.median(s["pass17"]), "blob_bytes": net.weight_blob_bytes(), "launches": net.launches_per_pass()}))
    net.close()


def child_trace(args):
    """a few passes of one (J, maps) configuration, to be run under rocprofv3"""
    import torch
    pkg = importlib.import_module("simple-hrnet_amd")
    net = engine(pkg, args.joints)
    crops, boxes = inputs(pkg)
    for _ in range(2 + args.reps):
        net.predict_crops(crops, boxes, return_heatmaps=bool(args.maps))
    torch.cuda.synchronize()
    net.close()


def child_pass133(args):
    pkg = importlib.import_module("simple-hrnet_amd")
    nets = {17: engine(pkg, 17), 133: engine(pkg, 133)}
    crops, boxes = inputs(pkg)
    samples = costlib.timed({"%d %s" % (J, mode): (lambda J=J, mode=mode: nets[J].predict_crops(crops, boxes, refine=mode))
                             for J in (17, 133) for mode in (None, "dark")}, args.rounds, args.reps)
    print(json.dumps({"ms": {k: [round(s, 4) for s in v] for k, v in samples.items()}}))
    for net in nets.values():
        net.close()


def main():
    ap = costlib.parser(__doc__, "head_joints.txt", rounds=5, reps=10, out_required=False)
    ap.add_argument("--parent-tag", default="parent")
    ap.add_argument("--child", choices=["pass17", "trace", "pass133"])
    ap.add_argument("--joints", type=int, default=17)
    ap.add_argument("--maps", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        return {"pass17": child_pass17, "trace": child_trace, "pass133": child_pass133}[args.child](args)
    if not args.out:
        ap.error("--out DIR is required")
    me = [sys.executable, os.path.abspath(__file__), "--rounds", str(args.rounds), "--reps", str(args.reps)]
    report = costlib.Report(args.out, "head_joints.txt")   # (every finished line is kept at once: a later child that fails loses nothing)
    say = report.say
    say("head with more than 32 joints: HRNet-W48 384x288, one micro-batch of 256 crops, bf16 (tools/head_joints_cost.py)")
    say("samples: %d per child, %d passes each, HIP events" % (args.rounds, args.reps))
    say()

    lib_mod = importlib.import_module("simple-hrnet_amd._lib")
    variant = lib_mod.LIB_PATH.replace(".so", "_%s.so" % args.parent_tag)

    # ---- 1. the whole pass at J = 17, this library against the parent's
    if os.path.exists(variant):
        def pass17_argv(root):   # (the parent's side is the variant library, selected by its tag; the checkout is this one on both sides)
            tag = [] if root == costlib.ROOT else ["HRN_LIB_TAG=" + args.parent_tag]
            return ["env", "-u", "HRN_LIB_TAG"] + tag + me + ["--child", "pass17"]

        runs = costlib.ab(report, "1.", ["pass17"], variant, 3, args.rounds, args.reps, argv_of=pass17_argv,
                          titles={"pass17": ("the whole pass at J = 17", "ms per pass of 256 crops, the median of each child's samples")})
        if runs is None:
            raise SystemExit(1)
        say("   weight blob bytes / launches per pass: this %d / %d, parent %d / %d"
            % tuple(runs[side][key][0] for side in ("this tree", "parent") for key in ("blob_bytes", "launches")))
    else:
        say("1. not measured: no variant library %s (build the parent commit's library under that name)" % os.path.basename(variant))
    say()

    # ---- 2. the head launch alone, rocprofv3 --kernel-trace --stats, one run per configuration
    head = {}
    for J in (17, 133):
        for maps in (0, 1):
            d = os.path.join(args.out, "trace_j%d_maps%d" % (J, maps))
            costlib.traced(me + ["--child", "trace", "--joints", str(J), "--maps", str(maps)], d, timeout=300)
            # head_kernel / head_mfma_kernel (J <= 32), head_groups_kernel / head_mfma_groups_kernel
            head[(J, maps)] = costlib.kernel_stats(d, ("hrn::head_",))["hrn::head_"]
    hw = (H // 4) * (W // 4)
    in_bytes = N * hw * C * 2
    say("2. the head launch alone (rocprofv3 --kernel-trace --stats, a run of its own per row; us: average [min, max] over the calls)")
    for (J, maps), (calls, avg, lo, hi) in sorted(head.items()):
        floor = (in_bytes + (4 * J * hw * N if maps else 0)) / HBM_BPS * 1e6
        say("   J = %3d, heat-maps %-7s: %8.1f us [%.1f, %.1f] over %d calls; floor of its bytes at 6.15 TB/s %6.1f us (%.2f x the floor)" %
            (J, "written" if maps else "off", avg / 1e3, lo / 1e3, hi / 1e3, calls, floor, avg / 1e3 / floor))
    groups = (133 + GROUP - 1) // GROUP
    for maps in (0, 1):
        naive, got = groups * head[(17, maps)][1] / 1e3, head[(133, maps)][1] / 1e3
        spread = groups * (head[(17, maps)][3] - head[(17, maps)][2]) / 1e3
        say("   heat-maps %-7s: naive form = %d x the J = 17 launch = %.1f us (+- %.1f us of its spread); the grouped launch takes %.1f us = %.2f x" %
            ("written" if maps else "off", groups, naive, spread, got, got / naive))
    say()

    # ---- 3. the pass at J = 133 against J = 17, one process
    res, failure = costlib.run_child(me + ["--child", "pass133"], 420)
    if failure:
        raise SystemExit("child pass133 ended with %s: nothing more is started on the GPU" % failure)
    r = res["ms"]
    med = {k: statistics.median(v) for k, v in r.items()}
    say("3. the pass at J = 133 against J = 17, one process, rotated order (ms per pass of 256 crops; crops/s)")
    for k in sorted(r, key=lambda s: (s.split()[1], int(s.split()[0]))):
        say("   J = %3s refine %-5s: median %.4f ms [%.4f, %.4f]  %8.1f crops/s" % (k.split()[0], k.split()[1], med[k], min(r[k]), max(r[k]), N / med[k] * 1e3))
    for mode in ("None", "dark"):
        say("   refine %-5s: J = 133 costs %+.4f ms per pass over J = 17 (%.2f %%)" %
            (mode, med["133 " + mode] - med["17 " + mode], 100 * (med["133 " + mode] / med["17 " + mode] - 1)))
    say("   DARK over plain at J = 133: %+.4f ms (the scratch heat-map write of 256 x 133 maps and the window reads)" % (med["133 dark"] - med["133 None"]))


if __name__ == "__main__":
    main()
