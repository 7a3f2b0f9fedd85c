"""What the 13 entry points of the two-level trace refuse, and in which order, without a device: every call below starts from a good call
on fake, never dereferenced pointers and must return the code and the full ntr_last_error text that tests/golden/two_level_refusals.json
records (written by tests/golden/make_two_level_refusals.py from the library as it was before the host launch was stated once,
DESIGN.md 6y).  Single faults: the REFUSED lists of test_instanced_fast_capi_cpu.py and test_instanced_wide_fast_capi_cpu.py, as far as
an entry point has the argument, and a null seed where the seed is not optional.  Double faults: two neighbouring checks fail at once, and
the text says which comes first.  numRays == 0 returns NTR_OK whatever else is passed and zeroes every out-argument."""
import ctypes as C
import inspect
import json
import os

import ntrace_amd as nt
import test_instanced_fast_capi_cpu as binary
import test_instanced_wide_fast_capi_cpu as wide

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "two_level_refusals.json")
FAKE = binary.FAKE
# the wrapper of each entry point (the C name is "ntr_" + it) and the table of its layout
ENTRY_POINTS = dict([(n, binary) for n in ("trace_instanced", "trace_instanced_masked", "trace_instanced_stats", "trace_instanced_seeded",
                                           "trace_instanced_seeded_stats", "trace_instanced_fast", "trace_instanced_fast_stats")] +
                    [(n, wide) for n in ("trace_instanced_wide", "trace_instanced_wide_stats", "trace_instanced_wide_seeded",
                                         "trace_instanced_wide_seeded_stats", "trace_instanced_wide_fast", "trace_instanced_wide_fast_stats")])
ZERO_RAYS = "num_rays=0, every other argument zero"
# the checks in their order, one fault for each: (binary layout, wide layout)
BAD_VIS = dict(vis=nt.InstanceVisibility(FAKE + 2, 0))
CHAIN = [(dict(num_rays=-1),) * 2, (dict(d_rays=0),) * 2, (dict(num_instances=0),) * 2, (dict(root_link=~5),) * 2,
         (dict(tlas_nodes_bytes=100), dict(wide_tlas_nodes_bytes=192)), (dict(pool_nodes_bytes=700), dict(wide_pool_nodes_bytes=704)),
         (dict(pool_woop_bytes=8),) * 2, (BAD_VIS,) * 2, (dict(d_seed_results=FAKE + 8),) * 2, (dict(d_flags=0),) * 2]
LAST_TOO = dict(d_flags=FAKE + 4)   # the last check fails in two ways


def _label(change):
    def text(v):
        if isinstance(v, nt.InstanceVisibility):
            return "vis(0x%x,0x%x,0x%x)" % (v.d_instanceMasks or 0, v.d_rayMasks or 0, v.rayMask)
        return "0x%x" % v if v > 9 else str(v)
    return " ".join("%s=%s" % (k, text(v)) for k, v in change.items())


def cases(name):
    """-> [(label, keyword arguments)]: the faulty calls of one entry point's wrapper."""
    layout = ENTRY_POINTS[name]
    params = inspect.signature(getattr(nt, name)).parameters
    seeded = "d_seed_results" in params and params["d_seed_results"].default is inspect.Parameter.empty
    good = {k: v for k, v in layout.GOOD.items() if k in params}
    if seeded:
        good.update(d_seed_results=FAKE, seed_instance=5)
    applies = lambda change: all(k in params for k in change)   # noqa: E731
    singles = [c for c in layout.REFUSED if applies(c)] + ([dict(d_seed_results=0)] if seeded else [])
    chain = [c[layout is wide] for c in CHAIN if applies(c[layout is wide])]
    doubles = [dict(a, **b) for a, b in zip(chain, chain[1:])]
    if applies(LAST_TOO):
        doubles.append(dict(chain[-2], **LAST_TOO))
    return [(_label(c), dict(good, **c)) for c in singles + doubles]


def refusal(name, kw):
    try:
        getattr(nt, name)(**kw)
    except nt.NtrError as e:
        return [e.code, str(e)]
    return [0, ""]


def raw_outs(name):
    """-> (the C function, all-zero arguments, the indices of its out-arguments, their buffers filled with 0xFF)."""
    fn = getattr(nt.lib(), "ntr_" + name)
    n = len(fn.argtypes)
    sizes = [4]   # the seconds
    if name.endswith("_stats"):
        sizes = [C.sizeof(nt.InstancedTraceStats)] + ([C.sizeof(nt.InstancedFastStats)] if "fast" in name else [])
    outs = [C.create_string_buffer(b"\xff" * s, s) for s in sizes]
    at = list(range(n - 1 - len(outs), n - 1))   # before the stream, which is last
    return fn, [None if t is C.c_void_p or hasattr(t, "contents") else 0 for t in fn.argtypes], at, outs


def null_stats(name):
    """The stats forms through ctypes: null stats and numRays == -1 at once, for every choice of the null pointers -> [[code, text]]."""
    fn, args, at, outs = raw_outs(name)
    got = []
    for given in ([False], [False, False], [True, False], [False, True]):
        if len(given) == len(outs):
            a = list(args)
            a[0] = -1
            for i, o, g in zip(at, outs, given):
                a[i] = C.cast(o, fn.argtypes[i]) if g else None
            got.append([fn(*a), (nt.lib().ntr_last_error() or b"").decode()])
    return got


def zero_rays(name):
    """numRays == 0 and every other argument zero -> (code, every out-argument is all zero bytes)."""
    fn, args, at, outs = raw_outs(name)
    for i, o in zip(at, outs):
        args[i] = C.cast(o, fn.argtypes[i])
    return fn(*args), all(o.raw == bytes(len(o.raw)) for o in outs)


def record(name):
    """Everything the golden file holds for one entry point: label -> [code, text], a list of those, or [code, outs zeroed]."""
    rec = {label: refusal(name, kw) for label, kw in cases(name)}
    if name.endswith("_stats"):
        rec["null stats, num_rays=-1"] = null_stats(name)
    rec[ZERO_RAYS] = list(zero_rays(name))
    return rec


def test_every_refusal_and_the_order_of_the_checks_are_the_recorded_ones():
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert len(ENTRY_POINTS) == 13 and set(golden) == set(ENTRY_POINTS)
    for name in ENTRY_POINTS:
        got = record(name)
        # at the least the 19 single faults of an entry point without masks, seed and flags, the six pairs of its seven checks, zero rays
        assert len(got) >= 26, (name, len(got))
        for label, value in got.items():
            assert label in golden[name], (name, label)
            assert value == golden[name][label], (name, label, value, golden[name][label])
        assert set(golden[name]) == set(got), (name, sorted(set(golden[name]) - set(got)))


def test_zero_rays_is_ok_whatever_else_is_passed_and_zeroes_the_outs():
    for name in ENTRY_POINTS:
        assert zero_rays(name) == (0, True), name
