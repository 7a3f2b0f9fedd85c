"""Generates tests/golden/refit_refusals.json: for each of the five in-place refit entry points (ntr_tlas_refit, ntr_tlas_motion_refit,
ntr_tlas_wide_refit, ntr_bvh_refit_batch, ntr_pool_wide_refit), the code, the full ntr_last_error text and the zeroed result struct of
every faulty call that tests/test_refit_refusals_cpu.py makes, in the blocking and in the asynchronous form (the cases are that
module's).  The file freezes what the entry points refuse, with which words and in which order: it was written from the library as it
stood before their host protocol and the shared argument checks were stated once (refit_launch.h, tlas_refit_parts.h), and a change to
it is a deliberate, visible edit, never a side effect of a refactor.  Needs no device.  Re-run: python tests/golden/make_refit_refusals.py
[path of a libntrace_amd.so built from the commit whose behaviour is the rule; default: the product library]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import ntrace_amd as nt  # noqa: E402
import test_refit_refusals_cpu as t  # noqa: E402

if __name__ == "__main__":
    nt.use_library(os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else None)
    golden = {name: t.record(name) for name in t.CHECKS}
    for name, rec in golden.items():
        for label, value in rec.items():   # every faulty call was refused before any device work
            assert t.refused_on_the_host(value), (name, label, value)
    with open(t.GOLDEN, "w") as f:
        json.dump(golden, f, indent=1, sort_keys=True)
        f.write("\n")
    print("refit_refusals: %d entry points, %d cases" % (len(golden), sum(len(r) for r in golden.values())))
