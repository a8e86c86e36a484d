"""Cost of a head with more than 32 joints on the headline shape (HRNet-W48, 384x288, one micro-batch of 256 crops, bf16).
Three measurements, each from child processes of this one (one GPU process at a time, every child under its own time limit; the
first child that fails ends the run):

  1. the whole pass at J = 17, this library against a tagged variant built from the parent commit (HRN_LIB_TAG, see
     tools/build_variant.py): children alternate A, B, A, B, ...; every child takes `--rounds` samples of `--reps` passes.  The two
     must agree within the spread of the parent's own samples.
  2. the head launch alone, `rocprofv3 --kernel-trace --stats`, one traced child per (J, heat-maps written or not): J = 17 and
     J = 133.  Against 5 x the J = 17 launch (the naive form: one launch per joint group) and against the floor of its bytes at
     the project's measured 6.15 TB/s (input read once + 4 * J * h * w per crop where maps are written).
  3. the pass at J = 133 against J = 17 in ONE process, refine None and "dark", rotated order.

usage: python tools/head_joints_cost.py --out DIR [--parent-tag parent] [--rounds R] [--reps K]   -> DIR/head_joints.txt (+ the raw
child outputs); a missing variant library skips measurement 1 and says so."""
import argparse, csv, glob, importlib, json, os, statistics, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
C, H, W, N = 48, 384, 288, 256
HBM_BPS = 6.15e12          # the project's measured streaming rate (profiles/README.md)
GROUP = 32


def engine(pkg, J):
    return pkg.NativeHRNet(C, J, (H, W), "bf16", max_batch=N, device=0).load_state_dict(pkg.synth_state_dict(C, J, 0))


def inputs(pkg):
    import torch
    crops = torch.randn((N, 3, H, W), generator=torch.Generator(device="cuda").manual_seed(1234), device="cuda")
    return crops, torch.from_numpy(pkg.synth_boxes(N)).cuda()


def timed(fn, reps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def child_pass17(args):
    """ms per pass of predict_crops at J = 17 with whatever library HRN_LIB_TAG selects"""
    import torch
    pkg = importlib.import_module("simple-hrnet_amd")
    net = engine(pkg, 17)
    crops, boxes = inputs(pkg)
    for _ in range(4):
        net.predict_crops(crops, boxes)
    torch.cuda.synchronize()
    samples = [timed(lambda: net.predict_crops(crops, boxes), args.reps) for _ in range(args.rounds)]
    print(json.dumps({"tag": os.environ.get("HRN_LIB_TAG", ""), "blob_bytes": net.weight_blob_bytes(), "launches": net.launches_per_pass(),
                      "ms": [round(s, 4) for s in samples]}))
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
    import torch
    pkg = importlib.import_module("simple-hrnet_amd")
    nets = {17: engine(pkg, 17), 133: engine(pkg, 133)}
    crops, boxes = inputs(pkg)
    cases = [(J, mode) for J in (17, 133) for mode in (None, "dark")]
    for J, mode in cases:
        for _ in range(3):
            nets[J].predict_crops(crops, boxes, refine=mode)
    torch.cuda.synchronize()
    samples = {"%d %s" % k: [] for k in cases}
    for r in range(args.rounds):
        for J, mode in cases[r % 4:] + cases[:r % 4]:
            samples["%d %s" % (J, mode)].append(timed(lambda: nets[J].predict_crops(crops, boxes, refine=mode), args.reps))
    print(json.dumps({"ms": {k: [round(s, 4) for s in v] for k, v in samples.items()}}))
    for net in nets.values():
        net.close()


def run(cmd, log, env=None, limit=300):
    """one child under its own time limit; its stdout goes to `log`; returns the last line of it"""
    with open(log, "w") as f:
        rc = subprocess.call(["timeout", "-k", "10", str(limit)] + cmd, stdout=f, stderr=subprocess.STDOUT, env=env, cwd=ROOT,
                             stdin=subprocess.DEVNULL)
    if rc != 0:
        raise SystemExit("child failed with exit code %d (see %s): nothing more is started on the GPU" % (rc, log))
    lines = [x for x in open(log).read().splitlines() if x.strip()]
    return lines[-1] if lines else ""


def head_stats(stats_dir):
    """(calls, average ns, min ns, max ns) of the head kernel in a rocprofv3 --stats directory"""
    for path in glob.glob(os.path.join(stats_dir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            if "hrn::head_" in row["Name"]:   # head_kernel / head_mfma_kernel (J <= 32), head_groups_kernel / head_mfma_groups_kernel
                return int(row["Calls"]), float(row["AverageNs"]), float(row["MinNs"]), float(row["MaxNs"])
    raise SystemExit("no head kernel in the statistics under " + stats_dir)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--parent-tag", default="parent")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10, help="passes per timed sample")
    ap.add_argument("--child", choices=["pass17", "trace", "pass133"])
    ap.add_argument("--joints", type=int, default=17)
    ap.add_argument("--maps", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        return {"pass17": child_pass17, "trace": child_trace, "pass133": child_pass133}[args.child](args)
    if not args.out:
        ap.error("--out DIR is required")
    os.makedirs(args.out, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__), "--rounds", str(args.rounds), "--reps", str(args.reps)]
    report = ["head with more than 32 joints: HRNet-W48 384x288, one micro-batch of 256 crops, bf16 (tools/head_joints_cost.py)",
              "samples: %d per child, %d passes each, HIP events" % (args.rounds, args.reps), ""]
    done = [0]

    def flush():   # every finished measurement is printed and kept at once: a later child that fails loses nothing
        print("\n".join(report[done[0]:]), flush=True)
        done[0] = len(report)
        open(os.path.join(args.out, "head_joints.txt"), "w").write("\n".join(report) + "\n")

    lib_mod = importlib.import_module("simple-hrnet_amd._lib")
    variant = lib_mod.LIB_PATH.replace(".so", "_%s.so" % args.parent_tag)

    # ---- 1. the whole pass at J = 17, this library against the parent's
    if os.path.exists(variant):
        ms = {"this": [], "parent": []}
        meta = {}
        for k in range(6):                               # this, parent, this, parent, ...
            who = "parent" if k & 1 else "this"
            env = dict(os.environ)
            env.pop("HRN_LIB_TAG", None)
            if who == "parent":
                env["HRN_LIB_TAG"] = args.parent_tag
            r = json.loads(run(me + ["--child", "pass17"], os.path.join(args.out, "pass17_%d_%s.log" % (k, who)), env))
            ms[who] += r["ms"]
            meta[who] = (r["blob_bytes"], r["launches"])
        med = {k: statistics.median(v) for k, v in ms.items()}
        report += ["1. whole pass at J = 17, three children each, alternating (ms per pass of 256 crops)",
                   "   this branch: median %.4f  (min %.4f, max %.4f)   %.1f crops/s" % (med["this"], min(ms["this"]), max(ms["this"]), N / med["this"] * 1e3),
                   "   parent     : median %.4f  (min %.4f, max %.4f)   %.1f crops/s" % (med["parent"], min(ms["parent"]), max(ms["parent"]), N / med["parent"] * 1e3),
                   "   difference of the medians %+.4f ms; spread of the parent's own samples %.4f ms -> %s" %
                   (med["this"] - med["parent"], max(ms["parent"]) - min(ms["parent"]),
                    "within it" if min(ms["parent"]) <= med["this"] <= max(ms["parent"]) else "OUTSIDE it"),
                   "   weight blob bytes / launches per pass: this %d / %d, parent %d / %d" % (meta["this"] + meta["parent"]), ""]
    else:
        report += ["1. not measured: no variant library %s (build the parent commit's library under that name)" % os.path.basename(variant), ""]

    flush()

    # ---- 2. the head launch alone, rocprofv3 --kernel-trace --stats, one run per configuration
    head = {}
    for J in (17, 133):
        for maps in (0, 1):
            d = os.path.join(args.out, "trace_j%d_maps%d" % (J, maps))
            run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "t", "--output-format", "csv", "--"] + me +
                ["--child", "trace", "--joints", str(J), "--maps", str(maps)], os.path.join(args.out, "trace_j%d_maps%d.log" % (J, maps)))
            head[(J, maps)] = head_stats(d)
    hw = (H // 4) * (W // 4)
    in_bytes = N * hw * C * 2
    report.append("2. the head launch alone (rocprofv3 --kernel-trace --stats, a run of its own per row; us: average [min, max] over the calls)")
    for (J, maps), (calls, avg, lo, hi) in sorted(head.items()):
        floor = (in_bytes + (4 * J * hw * N if maps else 0)) / HBM_BPS * 1e6
        report.append("   J = %3d, heat-maps %-7s: %8.1f us [%.1f, %.1f] over %d calls; floor of its bytes at 6.15 TB/s %6.1f us (%.2f x the floor)" %
                      (J, "written" if maps else "off", avg / 1e3, lo / 1e3, hi / 1e3, calls, floor, avg / 1e3 / floor))
    groups = (133 + GROUP - 1) // GROUP
    for maps in (0, 1):
        naive, got = groups * head[(17, maps)][1] / 1e3, head[(133, maps)][1] / 1e3
        spread = groups * (head[(17, maps)][3] - head[(17, maps)][2]) / 1e3
        report.append("   heat-maps %-7s: naive form = %d x the J = 17 launch = %.1f us (+- %.1f us of its spread); the grouped launch takes %.1f us = %.2f x" %
                      ("written" if maps else "off", groups, naive, spread, got, got / naive))
    report.append("")
    flush()

    # ---- 3. the pass at J = 133 against J = 17, one process
    r = json.loads(run(me + ["--child", "pass133"], os.path.join(args.out, "pass133.log"), limit=420))["ms"]
    med = {k: statistics.median(v) for k, v in r.items()}
    report.append("3. the pass at J = 133 against J = 17, one process, rotated order (ms per pass of 256 crops; crops/s)")
    for k in sorted(r, key=lambda s: (s.split()[1], int(s.split()[0]))):
        report.append("   J = %3s refine %-5s: median %.4f ms [%.4f, %.4f]  %8.1f crops/s" % (k.split()[0], k.split()[1], med[k], min(r[k]), max(r[k]), N / med[k] * 1e3))
    for mode in ("None", "dark"):
        report.append("   refine %-5s: J = 133 costs %+.4f ms per pass over J = 17 (%.2f %%)" %
                      (mode, med["133 " + mode] - med["17 " + mode], 100 * (med["133 " + mode] / med["17 " + mode] - 1)))
    report.append("   DARK over plain at J = 133: %+.4f ms (the scratch heat-map write of 256 x 133 maps and the window reads)" % (med["133 dark"] - med["133 None"]))
    flush()


if __name__ == "__main__":
    main()
