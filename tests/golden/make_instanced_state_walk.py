"""Generates tests/golden/instanced_state_walk.txt: the output of tests/host/instanced_state_host_test.cpp's walk over CudaInstancedBVH --
after every call the outcome or the refusal's text, every public predicate, count and buffer size, and the hashes of each trace's
records -- in the lossless short form of test_instanced_state_host.compact: the distinct outcomes, states and results under numbers, a
line per single event, a row of 27 cells per first event of a pair.  The file freezes which call makes what stale, which call is
refused with which words and which launch a traceBatch takes: it was written from the class as it stood before its nine freshness flags
were derived from one table of writes (InstancedState.hpp), and a change to it is a deliberate, visible edit, never a
side effect of a refactor.  Needs a device.
Re-run: python tests/golden/make_instanced_state_walk.py [root of a built checkout of the commit whose behaviour is the rule; default:
this one].  The driver is always this checkout's; it uses the public API only.

Before it writes, the script asserts on the log that every event ran with outcome `ok` at least once, and that every fail() text of that
checkout's CudaInstancedBVH.cpp occurred at least once, but for these, which valid arguments in any order of calls do not reach:
  the arguments themselves are refused   Incorrect BVH layout; not a Compact tree's buffers; no meshes; bad mesh buffers; no BLASes
                                         selected; BLAS index outside (of a selection); no instances; without instanceNode; a transform
                                         or index buffer is smaller; no kernel name; no motion key; the motion key's buffer is smaller
  a pool of 4 GB                         the pool is full
  the library has to fail                every "CudaInstancedBVH: %s" of ntr_last_error, "instance %d: %s" (a singular transform) and
                                         "the world's trace: %s".  With them the two places that mark the TLAS lost after a failed
                                         ntr_tlas_refit / ntr_tlas_motion_refit are kept by reading, not by this walk
  calls that are no event of the walk    no BLASes to measure (measureBLASes reads only); no instance status (getInstanceStatus);
                                         setRayTimes' buffer holds fewer (the walk sets no per-ray times)
No pair of events is left out: the whole walk takes a few seconds.
"""
import os
import re
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE)]

import test_instanced_state_host as t  # noqa: E402

# the texts of the docstring's list: whole format strings, and parts that no reachable text holds
UNREACHABLE = ("CudaInstancedBVH: no instances", "CudaInstancedBVH: no motion key", "CudaInstancedBVH: %s", "CudaInstancedBVH: instance %d: %s",
               "CudaInstancedBVH: BLAS index %d outside [0, %d)")
UNREACHABLE_PARTS = ("Incorrect BVH layout!", "not a Compact tree's buffers", "the pool is full", "no meshes", "bad mesh buffers", "no BLASes selected",
                     "without instanceNode", "a transform or index buffer is smaller", "no kernel name", "the motion key's buffer is smaller",
                     "the world's trace: %s", "no instance status", "setRayTimes' buffer")
FORMATS = {"%d": r"-?\d+", "%s": r".*"}


def fail_texts(cpp):
    """Every fail() format string of the file, adjacent literals joined."""
    with open(cpp) as f:
        src = f.read()
    texts = set()
    for m in re.finditer(r'\bfail\(\s*((?:"(?:[^"\\]|\\.)*"\s*)+)', src):
        texts.add("".join(re.findall(r'"((?:[^"\\]|\\.)*)"', m.group(1))))
    return sorted(texts)


def reachable(text):
    return text not in UNREACHABLE and not any(part in text for part in UNREACHABLE_PARTS)


if __name__ == "__main__":
    root = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else t.ROOT
    with tempfile.TemporaryDirectory() as tmp:
        exe = t.compile_driver(root, os.path.join(tmp, "instanced_state_host_test"))
        start = time.time()
        lines = t.run_walk(exe)
        seconds = time.time() - start
    outcomes = {}
    for line in lines:
        head, outcome, _ = line.split(" | ", 2)
        outcomes.setdefault(head.split(" ")[2], set()).add(outcome)
    never_ok = sorted(e for e, o in outcomes.items() if "ok" not in o)
    assert not never_ok and len(outcomes) == 27, (never_ok, len(outcomes))
    refusals = set().union(*outcomes.values()) - {"ok"}
    texts = fail_texts(os.path.join(root, "ntrace_amd", "host", "CudaInstancedBVH.cpp"))
    want = [x for x in texts if reachable(x)]
    for text in want:
        pattern = re.escape(text)
        for f, r in FORMATS.items():
            pattern = pattern.replace(re.escape(f), r)
        # `no BLASes to %s`: optimizeBLASes' word is reached; measureBLASes is no event
        assert any(re.fullmatch(pattern, r) for r in refusals), "never refused with: " + text
    with open(t.GOLDEN, "w") as f:
        f.write("\n".join(t.compact(lines)) + "\n")
    print("instanced_state_walk: %d calls, %d distinct refusals, every one of the %d reachable fail() texts of %d occurred; the walk took %.1f s"
          % (len(lines), len(refusals), len(want), len(texts), seconds))
