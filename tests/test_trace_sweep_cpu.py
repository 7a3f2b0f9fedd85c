"""The definition of the trace-tunable sweep (tests/trace_sweep.py), checked without a device: the pairwise rows cover every pair, the
shape rows reach every launch shape the plan can return, and the factor table and the library know the same tunables.  The rows
themselves are launched by tests/test_trace_sweep_gpu.py."""
import itertools
import os
import re

import pytest

import ntrace_amd as nt
import trace_sweep as ts

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ntrace_amd", "csrc")
BATCHES = (12288 - 27, 8229, 1000)     # the sizes test_trace_sweep_gpu.py traces its shape rows with


@pytest.fixture(autouse=True)
def default_tunables(monkeypatch):
    for k in list(os.environ):
        if k.startswith("NTR_"):
            monkeypatch.delenv(k, raising=False)
    nt.set_tunables()
    yield
    ts.clear()
    nt.set_tunables()


def test_the_table_is_well_formed():
    names = [f[0] for f in ts.FACTORS]
    assert len(set(names)) == len(names)
    for name, values, where, why in ts.FACTORS:
        assert len(values) >= 2 and len(set(values)) == len(values) and all(isinstance(v, int) for v in values), name
        # what bounds the domain: a line of the code that consumes the tunable
        m = re.fullmatch(r"([a-z_]+\.(?:h|hip|cpp)):(\d+)", where)
        assert m and why, (name, where)
        with open(os.path.join(CSRC, m.group(1))) as f:
            lines = f.read().splitlines()
        assert 1 <= int(m.group(2)) <= len(lines) and lines[int(m.group(2)) - 1].strip(), (name, where)
    assert set(ts.PLAN_STEERING) <= set(names) and set(ts.LOOP_FACTORS) <= set(names)
    assert set(ts.FIXED) <= set(ts.EXCLUDED) and not set(ts.EXCLUDED) & set(names)
    assert all(isinstance(r, str) and r for r in ts.EXCLUDED.values())


def test_the_table_and_the_library_know_the_same_tunables():
    """Every name tunables_load_locked reads is a factor or is excluded with a reason, and nothing in the table is unknown to the
    library: a tunable added to ntr_api.cpp fails here until it joins the sweep.  The defaults are the library's, too."""
    with open(os.path.join(CSRC, "ntr_api.cpp")) as f:
        src = f.read()
    read = dict(re.findall(r'env_int\("(NTR_[A-Z0-9_]+)",\s*([^)]+?)\)', src))
    assert len(read) >= 30, "the pattern no longer finds the env_int calls"
    swept = {f[0] for f in ts.FACTORS}
    missing = sorted(set(read) - swept - set(ts.EXCLUDED))
    assert not missing, "tunables the sweep neither varies nor excludes (tests/trace_sweep.py, FACTORS / EXCLUDED): %s" % missing
    unknown = sorted((swept | set(ts.EXCLUDED)) - set(read))
    assert not unknown, "names the library does not read: %s" % unknown
    assert all(n.startswith(("NTR_TRACE_", "NTR_SCHED_")) for n in swept)
    not_trace = sorted(n for n in ts.EXCLUDED if n.startswith(("NTR_TRACE_", "NTR_SCHED_")) and n not in ts.FIXED)
    assert not not_trace, "a trace tunable may only be excluded by fixing it: %s" % not_trace
    for name, default in ts.DEFAULTS.items():
        assert eval(read[name], {"__builtins__": {}}) == default, (name, read[name], default)


def test_pairwise_rows_cover_every_pair():
    rows = ts.pairwise_rows()
    assert rows[0] == ts.DEFAULTS
    for r in rows:
        assert set(r) == set(ts.DEFAULTS) and all(r[n] in ts.DOMAIN[n] for n in r)
    want = ts.all_pairs()
    k = len(ts.FACTORS)
    assert len(want) == sum(len(ts.FACTORS[i][1]) * len(ts.FACTORS[j][1]) for i, j in itertools.combinations(range(k), 2))
    got = set()
    for r in rows:
        got |= ts.pairs_of(r)
    assert got == want, "%d pairs in no row, e.g. %s" % (len(want - got), sorted(want - got)[:3])
    # a covering array of strength 2 needs at least the product of its two largest domains; greedy stays within a small factor of it
    sizes = sorted(len(f[1]) for f in ts.FACTORS)
    assert sizes[-1] * sizes[-2] <= len(rows) <= 2 * sizes[-1] * sizes[-2], len(rows)
    # every row but the first is there for a pair no earlier row holds
    seen = set()
    for i, r in enumerate(rows):
        assert i == 0 or ts.pairs_of(r) - seen, "row %d covers nothing new" % i
        seen |= ts.pairs_of(r)


def test_shape_rows_reach_every_launch_shape_of_the_plan():
    """The keys of shape_rows are exactly those the full product of the plan-steering factors reaches (enumerated here a second time),
    every row's configuration reaches its key, and factors outside PLAN_STEERING move no key."""
    rows = ts.shape_rows(BATCHES)
    keys = [k for k, _ in rows]
    assert len(set(keys)) == len(keys)

    def keys_of(config, kernels=nt.KERNELS):
        ts.apply(config)
        return {ts.shape_key(kernel, ah, n, nt.trace_plan(kernel, n, ah, ts.PLAN_NODES_BYTES, ts.PLAN_WOOP_BYTES, num_cus=ts.PLAN_NUM_CUS))
                for kernel in kernels for ah in (0, 1) for n in BATCHES}

    reached = set()
    for combo in itertools.product(*(ts.DOMAIN[n] for n in ts.PLAN_STEERING)):
        reached |= keys_of(dict(ts.DEFAULTS, **dict(zip(ts.PLAN_STEERING, combo))))
    assert set(keys) == reached, (len(keys), len(reached))
    for key, config in rows:
        assert key in keys_of(config, kernels=(key[0],)), key
        assert set(ts.non_default(config)) <= set(ts.PLAN_STEERING)
    # every kernel name, both hit modes, every size; both sides of the routing, every launch variant a trace launch can have
    assert {k[0] for k in keys} == set(nt.KERNELS) and {k[1] for k in keys} == {0, 1} and {k[2] for k in keys} == set(BATCHES)
    assert {k[4] for k in keys} == {0, 1, 2} and {k[3] for k in keys} == {1, 5, 6, 7} and {k[11] for k in keys} == {0, 1, 5}
    # the pairwise rows, which vary every factor, reach no shape beyond these
    for r in ts.pairwise_rows():
        assert keys_of(r) <= reached, ts.row_id(r)


def test_rows_are_deterministic():
    assert ts.pairwise_rows() == ts.pairwise_rows()
    a, b = ts.shape_rows(BATCHES), ts.shape_rows(BATCHES)
    assert a == b and [ts.row_id(c) for _, c in a] == [ts.row_id(c) for _, c in b]
    # the tree's size in bytes moves grids, never a shape, while it stays above the prediction threshold and below the wide pool's
    assert [k for k, _ in ts.shape_rows(BATCHES, 64 * 5000, 64 * 7001)] == [k for k, _ in a]


def test_apply_sets_a_row_and_clear_restores_the_defaults():
    base = nt.trace_plan("kepler_dynamic_fetch", 1 << 21, False, 1 << 24, 1 << 24).as_dict()
    ts.apply(dict(ts.DEFAULTS, NTR_TRACE_CHUNK=128, NTR_TRACE_POOL_HEADS=8))
    p = nt.trace_plan("kepler_dynamic_fetch", 8229, False, ts.PLAN_NODES_BYTES, ts.PLAN_WOOP_BYTES)
    assert p.chunk == 128 and p.numHeads == 8 and p.predictable and p.useAutoHint      # (the lowered thresholds)
    ts.apply(ts.DEFAULTS)
    p = nt.trace_plan("kepler_dynamic_fetch", 8229, False, ts.PLAN_NODES_BYTES, ts.PLAN_WOOP_BYTES)
    assert p.chunk == 64 and p.numHeads == 128 and p.predictable
    ts.clear()
    assert not any(k.startswith("NTR_") for k in os.environ)
    assert nt.trace_plan("kepler_dynamic_fetch", 1 << 21, False, 1 << 24, 1 << 24).as_dict() == base


def test_values_no_kernel_can_take_are_clamped_when_the_tunables_load():
    """A refill threshold above the wave size would ask a full wave for a refill for ever (csrc/trace_kernels.hip: popcount(live) <
    threshold while the pool holds rays), a persistent grid of no workgroups is no launch, a chunk of no rays never empties the pool:
    tunables_load_locked clamps them, and the plan -- what the launch half binds -- shows the clamped value."""
    nt.set_tunables(NTR_TRACE_FETCH_THRESHOLD=65, NTR_TRACE_MINIPOOL_THRESHOLD=1000, NTR_TRACE_BLOCKS_PER_CU=0, NTR_TRACE_CHUNK=0, NTR_TRACE_ROUTE=0)
    for kernel in nt.KERNELS:
        p = nt.trace_plan(kernel, 1 << 21, False, 1 << 24, 1 << 24, num_cus=256)
        assert max(p.fetchThreshold, p.persistentFetchThreshold, p.perrayFetchThreshold) == 64 and p.chunk == 1, kernel
        if p.variant == 1:
            assert p.persistentBlocks == 256 and p.numBlocksIncoherent == 0 and p.numBlocksDivergent == 0, kernel
    nt.set_tunables(NTR_TRACE_ROUTE=None)
    f = nt.trace_plan("fermi_speculative_while_while", 1 << 21, False, 1 << 24, 1 << 24, num_cus=256)
    assert f.coherentRoute == 1 and f.fetchThreshold == f.perrayFetchThreshold == f.persistentFetchThreshold == 64 and f.persistentBlocks == 256
    # the ends of the domain pass through as they are
    nt.set_tunables(NTR_TRACE_FETCH_THRESHOLD=64, NTR_TRACE_MINIPOOL_THRESHOLD=64, NTR_TRACE_BLOCKS_PER_CU=1, NTR_TRACE_CHUNK=1)
    p = nt.trace_plan("kepler_dynamic_fetch", 1 << 21, False, 1 << 24, 1 << 24, num_cus=256)
    assert (p.persistentFetchThreshold, p.perrayFetchThreshold, p.persistentBlocks, p.chunk) == (64, 64, 256, 1)
    nt.set_tunables(NTR_TRACE_FETCH_THRESHOLD=None, NTR_TRACE_MINIPOOL_THRESHOLD=None, NTR_TRACE_BLOCKS_PER_CU=None, NTR_TRACE_CHUNK=None)
