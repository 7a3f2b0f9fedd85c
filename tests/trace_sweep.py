"""The sweep of the trace tunables: which configurations the suite launches (tests/test_trace_sweep_cpu.py checks this definition without
a device, tests/test_trace_sweep_gpu.py launches every row of it against the oracle).

ntr_trace_bvh promises the oracle's records bit for bit whatever the NTR_TRACE_* / NTR_SCHED_* tunables say.  Two families of rows
test that promise:

* pairwise_rows(): a covering array over FACTORS -- every value of every tunable meets every value of every other one in some row.
  That is what finds two LOOP parameters that do not get on (a forced pool depth with a refill threshold of 64, dynamic fetch from the
  start with splitting at every step, ...);
* shape_rows(): one configuration per LAUNCH SHAPE -- per distinct outcome of plan_trace (csrc/trace_plan.h) in the fields that select
  device code or launch-time behaviour.  A shape is a product of three or more tunables, the kernel name, the hit mode and the batch
  size, so pairs do not reach them all; the full product of the plan-steering tunables, evaluated through ntr_trace_plan on the CPU,
  does.

A tunable's DOMAIN is what the code that consumes it is written to take, found by reading that code (the file:line beside every
entry), never by trying values on a device.  Nothing here is stored: rows and shapes are computed on demand, so they follow the plan.

A new tunable: add its env_int line to csrc/ntr_api.cpp, read its consumer, and enter it in FACTORS (default first, then the other
values worth a launch: both ends of the domain, every value at which the consumer takes another path) or in EXCLUDED with the reason;
if plan_trace reads it and it changes a field of shape_key, name it in PLAN_STEERING as well.  test_trace_sweep_cpu.py fails until
the name is in one of the two lists."""
import itertools
import os
import random

import ntrace_amd as nt

# (name, values -- the default first --, what bounds the domain: file:line under ntrace_amd/csrc/ and the reading of it)
FACTORS = (
    ("NTR_TRACE_UNIFIED", (1, 0), "trace_plan.h:95", "a switch (!= 0): unified-step or while-while loop in the persistent body"),
    ("NTR_TRACE_ROUTE", (1, 0), "trace_plan.h:85", "a switch (!= 0)"),
    ("NTR_TRACE_MINIPOOL", (-1, 0, 1, 4, 16), "trace_kernels.hip:163",
     "< 0 on the device, 0 off, K = 1 the plain body through the mini-pool launch, 2 .. NTR_MINIPOOL_MAX_K = 16 pooled; above: plain body"),
    ("NTR_TRACE_MINIPOOL_WIDE", (-1, 2, 4), "trace_plan.h:42", "2 .. NTR_MINIPOOL_MAX_K is taken, anything else means 'by tree size'"),
    ("NTR_TRACE_MINIPOOL_THRESHOLD", (48, 1, 64), "trace_kernels.hip:111",
     "popcount(live) < threshold leaves the loop for a refill: <= 1 never, 64 = as soon as a lane is free; above 64 a full wave "
     "would never step (clamped to 64, ntr_api.cpp:372)"),
    ("NTR_TRACE_FETCH_THRESHOLD", (-1, 0, 1, 64), "trace_kernels.hip:426",
     "< 0 by body (48 / 24 / 0), 0 whole-wave refills only, 1 .. 64 as the mini-pool's threshold (clamped to 64, ntr_api.cpp:371)"),
    ("NTR_TRACE_CHUNK", (64, 32, 128, 48), "trace_kernels.hip:342",
     ">= 1 (clamped, ntr_api.cpp:367); the buffer-order pool deals whole chunks of any size, a wave takes a chunk above 64 in several "
     "refills; the ordered pool needs chunks that divide 256 and the plan drops it otherwise (trace_plan.h:138)"),
    ("NTR_TRACE_POOL_HEADS", (128, 8, 1024), "trace_plan.h:107", "clamped to 8 .. kPoolHeadsMax = 1024 and rounded down to a multiple of 8"),
    ("NTR_TRACE_BLOCKS_PER_CU", (7, 1), "trace_plan.h:103", ">= 1 (clamped, ntr_api.cpp:373); the grid is capped by the batch"),
    ("NTR_TRACE_BLOCKS_PER_CU_INCOHERENT", (3, 0, 1), "trace_plan.h:110", "0 < n < BLOCKS_PER_CU shrinks the grid, anything else leaves it"),
    ("NTR_TRACE_BLOCKS_PER_CU_DIVERGENT", (4, 0, 1), "trace_plan.h:114", "0 < n < BLOCKS_PER_CU shrinks the grid, anything else leaves it"),
    ("NTR_TRACE_SPLIT_SLICE", (8, 0, 1), "trace_plan.h:62", "<= 0 off, n >= 1 = the lanes are looked at every n steps"),
    ("NTR_TRACE_WHOLE_WAVE", (1, 0), "trace_kernels.hip:358", "a switch (== 0 means dynamic fetch from the start)"),
    ("NTR_TRACE_PREFETCH_AFTER", (8, -1, 0), "trace_kernels.hip:410", "< 0 never, n >= 0 = the dequeue is posted n steps into a chunk"),
    ("NTR_TRACE_LEAF_SWITCH", (-1, 0, 65), "trace_kernels.hip:72",
     "< 0 by hit mode (32 / 24, trace_plan.h:63); popcount(inner) < n: 0 never, 65 whenever a lane waits at a leaf"),
    ("NTR_TRACE_OCTANT", (1, 0), "trace_kernels.hip:199", "a switch"),
    ("NTR_TRACE_FLAT_FETCH", (1, 0), "trace_plan.h:57", "a switch (!= 0): flat or two-descriptor fetch instantiation"),
    ("NTR_TRACE_UNIFORM_PROLOGUE", (1, 0), "trace_plan.h:59", "a switch (!= 0)"),
    ("NTR_TRACE_CERTAIN_STEPS", (1, 0, 2), "ntr_api.cpp:258", "0 off, 1 any-hit launches, >= 2 every launch"),
    ("NTR_TRACE_CERTAIN_DESCENT", (1, 0), "ntr_api.cpp:306", "a switch (!= 0)"),
    ("NTR_TRACE_PREDICT", (1, 0), "trace_plan.h:69", "a switch (!= 0)"),
    ("NTR_TRACE_PREDICT_PERSISTENT", (1, 0), "trace_plan.h:138", "a switch (!= 0)"),
    ("NTR_TRACE_PREDICT_DEPTH", (9, 1), "sched_kernels.hip:347", "clamped to 1 .. NTR_TOP_DEPTH_MAX = 10; read when a BVH's table is (re)built"),
    ("NTR_TRACE_PERSISTENT_HINTS", (1, 0), "trace_plan.h:130", "a switch (!= 0)"),
    ("NTR_TRACE_AUTO_HINT", (1, 0), "trace_plan.h:131", "a switch (!= 0)"),
    ("NTR_SCHED_REFRESH_EVERY", (16, 1), "trace_plan.h:199", "<= 1 every launch refreshes, n = the n-th, 2n-th and every 4n-th"),
    ("NTR_SCHED_CLASSES", (32, 1, 64), "sched_kernels.hip:499", "clamped to 1 .. SCHED_MAX_CLASSES = 64; above 32 the 64-class instantiation"),
)

# thresholds lowered for the whole sweep, so that batches of a few thousand rays in trees of a few thousand nodes reach the dispatch-order
# prediction, the routing by coherence and the automatic hint
FIXED = {"NTR_TRACE_PREDICT_MIN_RAYS": 4096, "NTR_TRACE_AUTO_HINT_MIN_RAYS": 4096, "NTR_TRACE_PREDICT_MIN_NODES": 64}

# names tunables_load_locked reads that the sweep does not vary, each with its reason
EXCLUDED = {
    "NTR_TRACE_PREDICT_MIN_RAYS": "fixed at 4096 for the sweep (FIXED): a size threshold, the plan test pins both sides of it",
    "NTR_TRACE_AUTO_HINT_MIN_RAYS": "fixed at 4096 for the sweep (FIXED): a size threshold, the plan test pins both sides of it",
    "NTR_TRACE_PREDICT_MIN_NODES": "fixed at 64 for the sweep (FIXED): a size threshold, the plan test pins both sides of it",
    "NTR_LBVH_SPLIT": "LBVH build only (lbvh_kernels.hip): no trace launch reads it",
    "NTR_LBVH_AGG_LDS": "LBVH build only: no trace launch reads it",
    "NTR_LBVH_SORT_ITEMS": "LBVH build only: no trace launch reads it",
    "NTR_LBVH_AGG_STAGED": "LBVH build only: no trace launch reads it",
}

# the factors plan_trace turns into another launch shape (shape_key): shape_rows takes their full product
PLAN_STEERING = ("NTR_TRACE_UNIFIED", "NTR_TRACE_ROUTE", "NTR_TRACE_MINIPOOL", "NTR_TRACE_PREDICT", "NTR_TRACE_PREDICT_PERSISTENT",
                 "NTR_TRACE_PERSISTENT_HINTS", "NTR_TRACE_AUTO_HINT", "NTR_TRACE_CHUNK", "NTR_TRACE_FLAT_FETCH")

# the factors a kernel's traversal / refill loop reads (the comb tree of test_unified_loop_gpu.py is traced on rows that change one)
LOOP_FACTORS = ("NTR_TRACE_UNIFIED", "NTR_TRACE_MINIPOOL", "NTR_TRACE_MINIPOOL_THRESHOLD", "NTR_TRACE_FETCH_THRESHOLD", "NTR_TRACE_CHUNK",
                "NTR_TRACE_SPLIT_SLICE", "NTR_TRACE_WHOLE_WAVE", "NTR_TRACE_PREFETCH_AFTER", "NTR_TRACE_LEAF_SWITCH", "NTR_TRACE_OCTANT",
                "NTR_TRACE_FLAT_FETCH", "NTR_TRACE_UNIFORM_PROLOGUE", "NTR_TRACE_CERTAIN_STEPS", "NTR_TRACE_CERTAIN_DESCENT")

DOMAIN = {name: values for name, values, _, _ in FACTORS}
DEFAULTS = {name: values[0] for name, values, _, _ in FACTORS}
PAIRWISE_SEED = 20240607
PAIRWISE_CANDIDATES = 40

# the CPU enumeration's stand-in for the GPU test's tree (nodes of 64 x 3000 bytes) and device
PLAN_NODES_BYTES, PLAN_WOOP_BYTES, PLAN_NUM_CUS = 64 * 3000, 64 * 3000, 256


def non_default(config):
    """{name: value} of the settings of `config` that differ from the defaults, in table order."""
    return {n: config[n] for n in DEFAULTS if n in config and config[n] != DEFAULTS[n]}


def row_id(config):
    """A row's pytest id: its non-default settings, the NTR_ prefix dropped."""
    nd = non_default(config)
    return ",".join("%s=%d" % (n.replace("NTR_TRACE_", "").replace("NTR_", ""), v) for n, v in nd.items()) or "defaults"


def apply(config):
    """Sets the library's tunables to `config` on top of FIXED; every factor the configuration does not name goes back to its default."""
    kv = {n: None for n in DEFAULTS}
    kv.update(FIXED)
    kv.update(non_default(config))
    nt.set_tunables(**kv)


def clear():
    """Every name the sweep touches back to the library's default."""
    nt.set_tunables(**{n: None for n in itertools.chain(DEFAULTS, FIXED)})


def all_pairs():
    """Every ((factor i, value), (factor j, value)), i < j by table position, as indices into FACTORS and its value tuples."""
    out = set()
    for i, j in itertools.combinations(range(len(FACTORS)), 2):
        for a in range(len(FACTORS[i][1])):
            for b in range(len(FACTORS[j][1])):
                out.add((i, a, j, b))
    return out


def pairs_of(config):
    """The pairs of all_pairs() that `config` (a full {name: value}) holds."""
    idx = [FACTORS[i][1].index(config[FACTORS[i][0]]) for i in range(len(FACTORS))]
    return {(i, idx[i], j, idx[j]) for i, j in itertools.combinations(range(len(FACTORS)), 2)}


def pairwise_rows():
    """A covering array of strength 2 over FACTORS, built greedily (row 0 = the defaults; every further row is the best of
    PAIRWISE_CANDIDATES candidates, each grown factor by factor -- in a shuffled order, seeded in code -- taking the value that covers the
    most still-uncovered pairs with the values the candidate already holds).  Deterministic; returns full {name: value} dicts."""
    rng = random.Random(PAIRWISE_SEED)
    k = len(FACTORS)
    uncovered = all_pairs()

    def key(i, a, j, b):
        return (i, a, j, b) if i < j else (j, b, i, a)

    rows = [[0] * k]
    uncovered -= {key(i, 0, j, 0) for i, j in itertools.combinations(range(k), 2)}
    while uncovered:
        best, best_gain = None, -1
        for _ in range(PAIRWISE_CANDIDATES):
            # start from a still-uncovered pair, so that every row makes progress
            i0, a0, j0, b0 = rng.choice(sorted(uncovered))
            cand = {i0: a0, j0: b0}
            order = [f for f in range(k) if f not in cand]
            rng.shuffle(order)
            for f in order:
                gains = []
                for v in range(len(FACTORS[f][1])):
                    gains.append((sum(1 for g, w in cand.items() if key(f, v, g, w) in uncovered), rng.random(), v))
                cand[f] = max(gains)[2]
            row = [cand[f] for f in range(k)]
            gain = sum(1 for i, j in itertools.combinations(range(k), 2) if (i, row[i], j, row[j]) in uncovered)
            if gain > best_gain:
                best, best_gain = row, gain
        rows.append(best)
        uncovered -= {(i, best[i], j, best[j]) for i, j in itertools.combinations(range(k), 2)}
    return [{FACTORS[f][0]: FACTORS[f][1][v] for f, v in enumerate(r)} for r in rows]


def shape_key(kernel, any_hit, num_rays, plan):
    """What of a plan selects device code or launch-time behaviour: the kernel instantiations launched (launchVariant, flatFetch, the
    persistent variant where a persistent side is launched), whether one or two bodies run and who decides (coherentRoute), where the
    mini-pool's K comes from, and which scheduling work surrounds the launch (prediction, ordered pool, automatic hint, coherence probe)."""
    persistent_side = plan.variant == 1 or plan.coherentRoute == 1      # NTR_VARIANT_PERSISTENT (csrc/trace_kernels.h)
    return (kernel, int(bool(any_hit)), int(num_rays), plan.launchVariant, plan.coherentRoute, plan.minipool, plan.poolKFromDevice,
            plan.predictable, plan.persistentOrder, plan.useAutoHint, plan.probeOnRefresh, plan.persistentVariant if persistent_side else 0,
            plan.flatFetch)


def steering_product():
    """Every configuration of the plan-steering factors (the others at their defaults), in enumeration order."""
    for combo in itertools.product(*(DOMAIN[n] for n in PLAN_STEERING)):
        config = dict(DEFAULTS)
        config.update(zip(PLAN_STEERING, combo))
        yield config


def shape_rows(batches, nodes_bytes=PLAN_NODES_BYTES, woop_bytes=PLAN_WOOP_BYTES, num_cus=PLAN_NUM_CUS):
    """One (key, configuration) per launch shape that the full product of the plan-steering factors reaches for a kernel name of
    nt.KERNELS, a hit mode and a batch size of `batches`: the first configuration in enumeration order that reaches it.  Evaluated
    through ntr_trace_plan (no device); leaves the environment and the library's tunables as it found them."""
    seen = {}
    before = {n: os.environ.get(n) for n in itertools.chain(DEFAULTS, FIXED)}
    try:
        for config in steering_product():
            apply(config)
            for kernel in nt.KERNELS:
                for any_hit in (0, 1):
                    for n in batches:
                        key = shape_key(kernel, any_hit, n, nt.trace_plan(kernel, n, any_hit, nodes_bytes, woop_bytes, num_cus=num_cus))
                        if key not in seen:
                            seen[key] = config
    finally:
        nt.set_tunables(**before)
    return list(seen.items())
