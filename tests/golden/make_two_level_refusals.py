"""Generates tests/golden/two_level_refusals.json: for each of the 13 entry points of the two-level trace, the code and the full
ntr_last_error text of every faulty call that tests/test_two_level_refusals_cpu.py makes (the cases are that module's).  The file
freezes what the entry points refuse, with which words and in which order: it was written from the library as it stood before their
host launch was stated once (trace_instanced_launch.h), and a change to it is a deliberate, visible edit, never a side effect of a
refactor.  Needs no device.  Re-run: python tests/golden/make_two_level_refusals.py [path of a libntrace_amd.so built from the commit
whose behaviour is the rule; default: the product library]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import ntrace_amd as nt  # noqa: E402
import test_two_level_refusals_cpu as t  # noqa: E402

if __name__ == "__main__":
    nt.use_library(os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else None)
    golden = {name: t.record(name) for name in t.ENTRY_POINTS}
    for name, rec in golden.items():
        for label, value in rec.items():   # every faulty call was refused before any device work; zero rays are NTR_OK and zeroed
            codes = [v[0] for v in value] if isinstance(value[0], list) else value[:1]
            assert (value == [0, True]) if label == t.ZERO_RAYS else all(c == -1 for c in codes), (name, label, value)
    with open(t.GOLDEN, "w") as f:
        json.dump(golden, f, indent=1, sort_keys=True)
        f.write("\n")
    print("two_level_refusals: %d entry points, %d cases" % (len(golden), sum(len(r) for r in golden.values())))
