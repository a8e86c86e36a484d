"""What the tools/*_cost.py scripts share: the timing loop, the report, the arguments, the people, the child workloads of the
"this tree against the parent commit" section, that section itself, and the traced child.  tools/README.md states the protocol.
Importing this module does not import torch.

usage: python tools/costlib.py --child NAME[,NAME...] --root DIR [--rounds R] [--reps K]     (one JSON line: name -> median ms)
NAME is one of WORKLOADS; DIR is the checkout whose package is timed -- the script is always this tree's."""
import argparse
import csv
import glob
import importlib
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BENCH = ("--gpus", "1", "--steps", "30", "--warmup", "5")
SIDES = ("parent", "this tree")


# ---- timing
def window(fn, reps):
    """HIP-event ms per call of `reps` back-to-back calls"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def rotated(names, r):
    """the order of round r: every candidate takes every place in turn"""
    names = list(names)
    return names[r % len(names):] + names[:r % len(names)]


def timed(cands, rounds, reps=1, warmup=3):
    """{name: [ms per call, ...]}: `warmup` calls of every candidate, then `rounds` windows of `reps` calls each, interleaved"""
    import torch
    for fn in cands.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in cands}
    for r in range(rounds):
        for k in rotated(cands, r):
            samples[k].append(window(cands[k], reps))
    return samples


# ---- report
class Report:
    """say() prints a line and appends it to DIR/NAME at once, so a run killed at its time limit leaves what it measured"""

    def __init__(self, out_dir, name, form="%8.4f ms  (min %.4f .. max %.4f)", scale=1.0):
        os.makedirs(out_dir, exist_ok=True)
        self.path, self.form, self.scale = os.path.join(out_dir, name), form, scale
        open(self.path, "w").close()

    def say(self, text=""):
        print(text, flush=True)
        with open(self.path, "a") as f:
            f.write(text + "\n")

    def fmt(self, samples):
        return self.form % (self.scale * statistics.median(samples), self.scale * min(samples), self.scale * max(samples))


# ---- arguments
def parser(doc, report_name, rounds=9, reps=None, ab=None, out_required=True):
    """--out and --rounds; --reps where the tool has calls per sample; --ab-root / --ab-pairs where it has an A/B of `ab`"""
    ap = argparse.ArgumentParser(description=doc, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", required=out_required, help="directory %s is written to" % report_name)
    ap.add_argument("--rounds", type=int, default=rounds, help="timed samples per candidate")
    if reps is not None:
        ap.add_argument("--reps", type=int, default=reps, help="calls per timed sample")
    if ab is not None:
        ap.add_argument("--ab-root", help="checkout of the parent commit, built: %s there against here" % ab)
        ap.add_argument("--ab-pairs", type=int, default=3, help="child processes of this tree in the A/B (the parent runs once more)")
    return ap


# ---- people
def people_of(count, joints=17, seed=0, frame_hw=(1080, 1920), jitter=0.0, base=None):
    """`count` people of plausible size spread over the frame, or `base` jittered by `jitter` pixels: ((count, joints, 3) float32
    (y, x, confidence 0.9), (count, 4) int32 boxes around the joints)"""
    import numpy as np
    rng = np.random.default_rng(seed)
    hf, wf = frame_hw
    if base is None:
        pts = np.empty((count, joints, 3), np.float32)
        for i in range(count):
            bh = rng.uniform(300, 900)
            bw = bh * rng.uniform(0.3, 0.6)
            x1, y1 = rng.uniform(0, wf - bw), rng.uniform(0, hf - bh)
            pts[i, :, 0] = rng.uniform(y1, y1 + bh, joints)
            pts[i, :, 1] = rng.uniform(x1, x1 + bw, joints)
        pts[..., 2] = 0.9
    else:
        pts = base.copy()
        pts[..., :2] += rng.normal(0, jitter, pts[..., :2].shape).astype(np.float32)
    boxes = np.stack([pts[..., 1].min(1), pts[..., 0].min(1), pts[..., 1].max(1), pts[..., 0].max(1)], 1)
    return pts, np.round(boxes).astype(np.int32)


def prepath_boxes(count):
    """the boxes of bench.py's `prepath` block on its 1080p frame (the frame is drawn first there, so the boxes are the same)"""
    import numpy as np
    hf, wf = 1080, 1920
    rng = np.random.default_rng(5)
    rng.integers(0, 256, (hf, wf, 3), dtype=np.uint8)
    dets = np.zeros((count, 4), np.float32)
    for i in range(count):
        bh = rng.integers(300, 900)
        bw = int(bh * rng.uniform(0.3, 0.6))
        x1, y1 = rng.uniform(0, wf - bw), rng.uniform(0, hf - bh)
        dets[i] = (x1, y1, x1 + bw, y1 + bh)
    return dets


# ---- child workloads: what the A/B children time, each on a 1080p BGR frame resident in HBM
WORKLOADS = {
    "predict": ("predict_frame", "predict_frame, 8 people of a 1080p frame, HRNet-W32 256x192 bf16"),
    "predict_w48": ("predict_frame", "predict_frame, 8 people of a 1080p frame, HRNet-W48 384x288 bf16"),
    "draw8": ("draw_poses", "draw_poses, 8 people, COCO skeleton, 1080p BGR"),
    "draw64": ("draw_poses", "draw_poses, 64 people, COCO skeleton, 1080p BGR"),
    "draw8_ids": ("draw_poses with host ids", "draw_poses, host ids, 8 people, COCO skeleton, 1080p BGR"),
    "prepath_bgr": ("BGR preprocess_frame", "preprocess_frame, 16 people of a 1080p BGR frame, 384x288 crops"),
}


def coco_skeleton():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "coco_skeleton.json")))["coco_skeleton"]


def _workload(name, pkg, frame):
    """(engine, call) of one WORKLOADS entry"""
    import numpy as np
    import torch

    def engine(channels, res, batch, weights):
        net = pkg.NativeHRNet(channels, 17, res, "bf16", max_batch=batch, device=0)
        return net.load_state_dict(pkg.synth_state_dict(channels, 17, 0)) if weights else net

    if name in ("predict", "predict_w48"):
        net = engine(32, (256, 192), 8, True) if name == "predict" else engine(48, (384, 288), 8, True)
        dets = people_of(8, seed=1)[1].astype(np.float32)
        return net, lambda: net.predict_frame(frame, dets)
    if name in ("draw8", "draw64", "draw8_ids"):
        net, count, skeleton = engine(32, (64, 64), 1, False), 64 if name == "draw64" else 8, coco_skeleton()
        pts = torch.from_numpy(people_of(count, seed=count)[0]).cuda()
        kw = {"person_ids": np.arange(8, dtype=np.int32)} if name == "draw8_ids" else {}
        return net, lambda: net.draw_poses(frame, pts, skeleton, **kw)
    if name == "prepath_bgr":
        net, dets = engine(32, (384, 288), 32, False), prepath_boxes(16)
        return net, lambda: net.preprocess_frame(frame, dets)
    raise SystemExit("unknown child workload %r: one of %s" % (name, ", ".join(WORKLOADS)))


def child_main(names, root, rounds, reps):
    sys.path.insert(0, os.path.abspath(root))
    import numpy as np
    import torch
    pkg = importlib.import_module("simple-hrnet_amd")
    frame = torch.from_numpy(np.random.default_rng(6).integers(0, 256, (1080, 1920, 3), dtype=np.uint8)).cuda()
    loads = {name: _workload(name, pkg, frame) for name in names}
    s = timed({name: fn for name, (_, fn) in loads.items()}, rounds, reps, warmup=5)
    for net, _ in loads.values():
        net.close()
    print(json.dumps({k: statistics.median(v) for k, v in s.items()}))


# ---- the A/B: this tree against the parent commit
def ab_order(pairs):
    """fresh children alternately, the parent first and last: the parent's own runs give the spread"""
    if pairs < 1:
        raise ValueError("--ab-pairs must be at least 1: the spread is taken between the parent's own runs")
    return [SIDES[0]] + [SIDES[1], SIDES[0]] * pairs


def verdict(parent, tree, larger_is_better=False):
    """(diff, spread, words): median(this tree) - median(parent) against max - min of the parent's own runs"""
    diff, spread = statistics.median(tree) - statistics.median(parent), max(parent) - min(parent)
    if abs(diff) <= spread:
        return diff, spread, "unchanged"
    return diff, spread, ("SLOWER" if (diff > 0) != larger_is_better else "faster") + " beyond the spread"


def last_json(text):
    """the last line of a child's output that holds a JSON object"""
    return json.loads([ln for ln in text.splitlines() if ln.lstrip().startswith("{")][-1])


def run_child(argv, limit, cwd=None):
    """one fresh process, stdin closed, under its own time limit: (its JSON result, None) or (None, what went wrong)"""
    try:
        done = subprocess.run(argv, cwd=cwd, stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        return None, "time limit (%d s)" % limit
    if done.returncode != 0:
        return None, "exit status %d" % done.returncode
    return last_json(done.stdout), None


def ab(report, label, names, ab_root, pairs, rounds, reps, bench=False, argv_of=None, titles=WORKLOADS, limit=300):
    """The section `label` of a report: the children `names` (and bench.py) in this tree against the checkout at `ab_root`.
    `argv_of(root)` gives a child's command (default: this file's --child mode).  Returns {side: {key: [value per run]}} -- empty
    when there is no `ab_root` -- or None when a child failed: no further child is started then, and the caller exits non-zero."""
    say = report.say
    what = " and ".join(dict.fromkeys([titles[n][0] for n in names] + ["bench.py"] * bench))
    if not ab_root:
        say("%s %s, this tree against the parent commit: NOT MEASURED (no --ab-root)" % (label, what))
        return {}
    order = ab_order(pairs)
    roots = dict(zip(SIDES, (os.path.abspath(ab_root), ROOT)))
    argv_of = argv_of or (lambda root: [sys.executable, os.path.abspath(__file__), "--child", ",".join(names), "--root", root,
                                        "--rounds", str(rounds), "--reps", str(reps)])
    say("%s %s: this tree against the parent commit, fresh processes one at a time on the same box, alternately, the parent" % (label, what))
    say("    first and last (%d runs against %d); the spread is the one between the parent's own runs" % (pairs + 1, pairs))
    runs = {side: {} for side in SIDES}
    for side in order:
        jobs = [(argv_of(roots[side]), None, limit)]
        if bench:
            jobs.append(([sys.executable, os.path.join(roots[side], "bench.py")] + list(BENCH), roots[side], 2 * limit))
        for argv, cwd, seconds in jobs:
            res, failure = run_child(argv, seconds, cwd)
            if failure:
                say("    A/B NOT COMPLETED: the child `%s` of %s (%s) ended with %s; no further child is started"
                    % (" ".join(argv[1:]), side, roots[side], failure))
                return None
            if cwd:    # bench.py's result line: its value under whichever name it has
                res = {"bench": float(next(res[key] for key in ("value", "images_per_sec", "throughput", "crops_per_sec") if key in res))}
            for key, value in res.items():
                runs[side].setdefault(key, []).append(value)
    for name in list(names) + ["bench"] * bench:
        unit = "" if name == "bench" else " ms"
        say("    %s" % ("bench.py %s, its value (larger is better)" % " ".join(BENCH) if name == "bench" else titles[name][1]))
        for side in SIDES:
            say("        %-10s runs %s%s -> median %.4f%s"
                % (side, ", ".join("%.4f" % v for v in runs[side][name]), unit, statistics.median(runs[side][name]), unit))
        diff, spread, words = verdict(runs[SIDES[0]][name], runs[SIDES[1]][name], larger_is_better=name == "bench")
        say("        difference %+.4f%s; spread between the parent's own runs %.4f%s -> %s" % (diff, unit, spread, unit, words))
    return runs


# ---- traced children
def traced(argv, out_dir, timeout=600):
    """`argv` under rocprofv3 --kernel-trace --stats (kernel tracing only; the program after `--`), csv under `out_dir`.  A child
    that fails or reaches its time limit ends the tool: nothing more is started on the GPU after it."""
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out_dir, "-o", "t", "--output-format", "csv", "--"] + list(argv)
    try:
        rc = subprocess.run(cmd, timeout=timeout, stdin=subprocess.DEVNULL, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode
    except subprocess.TimeoutExpired:
        rc = "time limit (%d s)" % timeout
    if rc != 0:
        raise SystemExit("traced child `%s` ended with %s: nothing more is started on the GPU" % (" ".join(argv), rc))


def kernel_stats(stats_dir, names):
    """name -> (calls, average ns, min ns, max ns) of the kernels whose name holds one of `names`, from a --stats directory"""
    found = {}
    for path in glob.glob(os.path.join(stats_dir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            for name in names:
                if name in row["Name"]:
                    found[name] = (int(row["Calls"]), float(row["AverageNs"]), float(row["MinNs"]), float(row["MaxNs"]))
    return found


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--child", required=True, help="workloads to time, comma-separated: " + ", ".join(WORKLOADS))
    ap.add_argument("--root", required=True, help="the checkout whose package is timed")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    child_main(args.child.split(","), args.root, args.rounds, args.reps)
