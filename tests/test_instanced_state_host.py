"""What CudaInstancedBVH reports after every call (tests/host/instanced_state_host_test.cpp, compiled here against libntrace_amd.so; DESIGN.md
6af).  The GPU test walks the class through every single event from four base states and every ordered pair of events from the widened
and from the motion state.  Its output -- outcome or refusal text, every public predicate, count and buffer size, the hashes of each
trace's records -- in compact()'s lossless short form equals tests/golden/instanced_state_walk.txt line for line: that file was recorded
from the class as it stood before its freshness flags were derived from one table of writes
(tests/golden/make_instanced_state_walk.py), and a change to it is a deliberate edit.  The CPU test exhausts the pure state object
(ntrace_amd/host/InstancedState.hpp) over all product subsets times all writes."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "instanced_state_host_test.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "instanced_state_walk.txt")


def compile_driver(root, out):
    """The driver of this checkout against the headers and the library of the checkout at `root`."""
    lib = os.path.join(root, "ntrace_amd")
    inc = ["-I" + os.path.join(root, "include"), "-I" + os.path.join(root, "ntrace_amd", "csrc"), "-I" + os.path.join(root, "ntrace_amd", "host")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off"] + inc + [SRC, "-o", out, "-L" + lib, "-lntrace_amd",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return out


def run_walk(exe):
    """-> the walk's lines; the last one is the driver's own summary."""
    out = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert lines and lines[-1].startswith("instanced_state_host_test gpu: done, "), lines[-3:]
    return lines[:-1]


def compact(lines):
    """The walk's lines with nothing lost, in a form that can be read whole: every distinct outcome, state and trace or flags result once,
    under a number; one line per set-up call and per single event; and per base state and first event one row: the first event's
    outcome.state.result, then one such cell per second event, in the order of the `events` line.  The walk is deterministic, so a first
    event comes out the same ahead of each of its 27 second events; where it does not, a line of its own says so, which no recorded
    file holds."""
    tables = {"outcome": {}, "state": {}, "result": {"": 0}}
    events, single, rows, odd = [], [], {}, []
    for line in lines:
        head, outcome, rest = line.split(" | ", 2)
        _, where, event = head.split(" ")
        state, result = re.fullmatch(r"(.* bytes=\S+) ?(.*)", rest).groups()
        cell = ".".join(str(tables[k].setdefault(text, len(tables[k]))) for k, text in (("outcome", outcome), ("state", state), ("result", result)))
        if event not in events:
            events.append(event)
        if ">" in where:
            rows.setdefault(where.split(">")[0], []).append((event, cell))
        else:
            single.append("%s %s %s" % (where, event, cell))
    head = ["events " + " ".join(events)] + ["%s %d %s" % (kind, k, text) for kind, table in tables.items() for text, k in table.items()]
    pairs = []
    for where, calls in rows.items():   # where: base:first; calls: first, second, first, second, ...
        first = where.split(":")[1]
        odd += ["%s came out as %s %s ahead of second event %d" % (where, event, cell, k)
                for k, (event, cell) in enumerate(calls[0::2]) if (event, cell) != (first, calls[0][1])]
        if [event for event, _ in calls[1::2]] != events:
            odd.append("%s: the second events are not the `events` line" % where)
        pairs.append("%s %s : %s" % (where, calls[0][1], " ".join(cell for _, cell in calls[1::2])))
    return head + single + pairs + odd


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "ntrace_amd", "csrc")])
    return compile_driver(ROOT, str(tmp_path_factory.mktemp("instanced_state_host") / "instanced_state_host_test"))


def test_the_table_of_writes_over_all_product_subsets_cpu(exe):
    out = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "instanced_state_host_test cpu: ok" in out.stdout


@pytest.mark.gpu
def test_the_walk_equals_the_recorded_one_line_for_line_gpu(exe):
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    got = compact(run_walk(exe))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, "line %d:\n  now      %s\n  recorded %s" % (k + 1, g, w)
    assert len(got) == len(want), got[len(want):] + want[len(got):]
