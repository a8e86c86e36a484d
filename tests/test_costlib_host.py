"""tools/costlib.py without a GPU: the rotation, the order of the A/B children, its verdict rule, what it does when a child fails,
the write-through report and the JSON contract of the child mode.  The stand-in children are plain `python -c` programs."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import costlib  # noqa: E402


def test_import_does_not_import_torch():
    import subprocess
    code = "import sys; sys.path.insert(0, %r); import costlib; sys.exit('torch' in sys.modules)" % os.path.dirname(costlib.__file__)
    assert subprocess.run([sys.executable, "-c", code]).returncode == 0


@pytest.mark.parametrize("names", [["a"], ["a", "b"], ["a", "b", "c", "d", "e"]])
def test_rotated(names):
    for r in range(7):
        order = costlib.rotated(names, r)
        assert sorted(order) == sorted(names)
        assert order[0] == names[r % len(names)]                                        # every candidate leads in turn
        assert all(order[i + 1] == names[(names.index(order[i]) + 1) % len(names)] for i in range(len(names) - 1))
    assert costlib.rotated(dict.fromkeys(names), 1) == costlib.rotated(names, 1)         # (a dict of candidates gives its keys)


def test_ab_order():
    assert costlib.ab_order(1) == ["parent", "this tree", "parent"]
    assert costlib.ab_order(3) == ["parent", "this tree", "parent", "this tree", "parent", "this tree", "parent"]
    for pairs in (0, -1):
        with pytest.raises(ValueError):
            costlib.ab_order(pairs)


def test_verdict():
    parent = [10.0, 10.5, 10.25]                      # median 10.25, spread 0.5
    assert costlib.verdict(parent, [10.5, 10.5]) == (0.25, 0.5, "unchanged")            # strictly inside
    assert costlib.verdict(parent, [10.75]) == (0.5, 0.5, "unchanged")                  # exactly the spread
    assert costlib.verdict(parent, [9.75]) == (-0.5, 0.5, "unchanged")
    assert costlib.verdict(parent, [11.0, 11.0])[2] == "SLOWER beyond the spread"
    assert costlib.verdict(parent, [9.5])[2] == "faster beyond the spread"
    # the bench arm: larger is better, so the words swap (and only the words)
    assert costlib.verdict(parent, [11.0], larger_is_better=True) == (0.75, 0.5, "faster beyond the spread")
    assert costlib.verdict(parent, [9.5], larger_is_better=True) == (-0.75, 0.5, "SLOWER beyond the spread")
    assert costlib.verdict(parent, [10.75], larger_is_better=True)[2] == "unchanged"
    assert costlib.verdict([7.0, 7.0], [7.0])[2] == "unchanged" and costlib.verdict([7.0, 7.0], [7.001])[2] == "SLOWER beyond the spread"


def counting_child(tmp_path, body):
    """argv builder of a stand-in child: it appends the root it was given to a counter file, then runs `body`"""
    counter = tmp_path / "started"
    code = "import sys, time\nopen(%r, 'a').write(sys.argv[1] + '\\n')\nparent = sys.argv[1] == %r\n%s" % (str(counter), str(tmp_path / "parent"), body)
    return (lambda root: [sys.executable, "-c", code, root]), (lambda: counter.read_text().splitlines() if counter.exists() else [])


def test_ab_runs_children_alternately_and_reports(tmp_path):
    # the child's value depends on its root alone: 5.0 in the parent, 5.25 here; the parent's own runs do not differ -> spread 0
    argv_of, started = counting_child(tmp_path, "print('noise'); print('{\"predict\": %s}' % (5.0 if parent else 5.25))")
    parent = tmp_path / "parent"
    parent.mkdir()
    report = costlib.Report(str(tmp_path), "r.txt")
    runs = costlib.ab(report, "(c)", ["predict"], str(parent), 2, 1, 1, argv_of=argv_of)
    assert runs == {"parent": {"predict": [5.0, 5.0, 5.0]}, "this tree": {"predict": [5.25, 5.25]}}
    assert started() == [str(parent), costlib.ROOT, str(parent), costlib.ROOT, str(parent)]
    text = open(report.path).read()
    assert "parent     runs 5.0000, 5.0000, 5.0000 ms -> median 5.0000 ms" in text
    assert "this tree  runs 5.2500, 5.2500 ms -> median 5.2500 ms" in text
    assert "difference +0.2500 ms; spread between the parent's own runs 0.0000 ms -> SLOWER beyond the spread" in text


def test_ab_without_root_and_with_no_pairs(tmp_path):
    argv_of, started = counting_child(tmp_path, "print('{\"predict\": 1.0}')")
    report = costlib.Report(str(tmp_path), "r.txt")
    assert costlib.ab(report, "(c)", ["predict"], None, 3, 1, 1, argv_of=argv_of) == {}
    assert open(report.path).read() == "(c) predict_frame, this tree against the parent commit: NOT MEASURED (no --ab-root)\n"
    with pytest.raises(ValueError):
        costlib.ab(report, "(c)", ["predict"], str(tmp_path), 0, 1, 1, argv_of=argv_of)
    assert started() == []


@pytest.mark.parametrize("body, limit, status", [("sys.exit(3)", 30, "exit status 3"), ("time.sleep(30)", 1, "time limit")])
def test_ab_stops_at_the_first_failed_child(tmp_path, body, limit, status):
    # the parent's children are well; the first child of this tree fails: the second of five started, and the last one
    argv_of, started = counting_child(tmp_path, "if parent:\n    print('{\"predict\": 1.0}')\nelse:\n    " + body)
    parent = tmp_path / "parent"
    parent.mkdir()
    report = costlib.Report(str(tmp_path), "r.txt")
    report.say("measured before the A/B")
    assert costlib.ab(report, "(c)", ["predict"], str(parent), 2, 1, 1, argv_of=argv_of, limit=limit) is None
    assert started() == [str(parent), costlib.ROOT]
    text = open(report.path).read()
    assert text.startswith("measured before the A/B\n")
    last = text.splitlines()[-1]
    assert "this tree" in last and costlib.ROOT in last and status in last and "no further child is started" in last


def test_report_writes_through(tmp_path):
    report = costlib.Report(str(tmp_path / "deep" / "dir"), "r.txt", "%6.1f us [%.1f, %.1f]", scale=1e3)
    assert open(report.path).read() == ""
    said = []
    for text in ("first", "", "third  %s" % report.fmt([0.002, 0.001, 0.004])):
        report.say(text)
        said.append(text)
        assert open(report.path).read() == "\n".join(said) + "\n"
    assert said[-1] == "third     2.0 us [1.0, 4.0]"
    assert costlib.Report(str(tmp_path), "d.txt").fmt([1.0, 3.0, 2.0]) == "  2.0000 ms  (min 1.0000 .. max 3.0000)"


def test_child_json_contract(tmp_path):
    # one JSON object of name -> median ms, on the last line that holds one; other lines before it do not count
    res, failure = costlib.run_child([sys.executable, "-c", "print('warming up'); print('{\"old\": 1}'); print('{\"predict\": 1.5, \"draw8\": 0.25}')"], 30)
    assert failure is None and res == {"predict": 1.5, "draw8": 0.25}
    assert costlib.last_json('x\n{"a": 1}\n\ntrailing words\n') == {"a": 1}
    res, failure = costlib.run_child([sys.executable, "-c", "import sys; print(sys.stdin.read() == '', end=''); print(); print('{}')"], 30)
    assert failure is None and res == {}                                                # (stdin is closed: the read returns at once)


def test_people_of():
    import numpy as np
    pts, boxes = costlib.people_of(64, joints=133, seed=3)
    assert pts.shape == (64, 133, 3) and pts.dtype == np.float32 and boxes.shape == (64, 4) and boxes.dtype == np.int32
    assert (pts[..., 2] == np.float32(0.9)).all()
    assert (boxes[:, 0] >= 0).all() and (boxes[:, 1] >= 0).all() and (boxes[:, 2] <= 1920).all() and (boxes[:, 3] <= 1080).all()
    heights, widths = boxes[:, 3] - boxes[:, 1], boxes[:, 2] - boxes[:, 0]
    assert heights.max() <= 900 and heights.min() > 250 and (widths <= 0.6 * 900).all()   # (133 joints nearly fill a 300..900 box)
    again, _ = costlib.people_of(64, joints=133, seed=3)
    assert np.array_equal(pts, again)
    moved, moved_boxes = costlib.people_of(64, joints=133, seed=4, jitter=3.0, base=pts)
    assert moved.shape == pts.shape and not np.array_equal(moved, pts) and np.abs(moved[..., :2] - pts[..., :2]).max() < 20
    assert np.array_equal(moved[..., 2], pts[..., 2]) and np.abs(moved_boxes - boxes).max() < 20
