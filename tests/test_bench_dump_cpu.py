"""bench.py --dump-outputs without a GPU: dump_outputs() on stand-in result buffers of a 1080p frame (primary batch + 16 AO batches)."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
bench = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bench)


def _records(n, seed):
    rng = np.random.default_rng(seed)
    r = np.zeros((n, 4), dtype=np.int32)
    r[:, 0] = rng.integers(-1, 262267, n)
    for c in (1, 2, 3):
        r[:, c] = rng.random(n, dtype=np.float32).view(np.int32)
    return r


class _Frame:
    def __init__(self, primary, ao):
        self.primary = torch.from_numpy(primary.view(np.uint8).reshape(-1).copy())
        self.batches = [{}] + [{"res_t": torch.from_numpy(a.view(np.uint8).reshape(-1).copy())} for a in ao]

    def own_primary_records(self):
        return self.primary


def test_dump_outputs_1080p_frame(tmp_path):
    prim = _records(1920 * 1080, 1)
    ao = [_records(131072 * 8, 2 + i) for i in range(16)]
    frame = _Frame(prim, ao)
    shapes = bench.dump_outputs(str(tmp_path / "a"), frame, torch)
    bench.dump_outputs(str(tmp_path / "b"), frame, torch)
    assert shapes["primary_id"] == [1920 * 1080] and shapes["ao_id"] == [bench.DUMP_AO_RECORDS]
    total = 0
    for name in shapes:
        a = np.load(str(tmp_path / "a" / (name + ".npy")))
        assert a.dtype in (np.float32, np.float64)
        assert np.array_equal(a.view(np.uint8), np.load(str(tmp_path / "b" / (name + ".npy"))).view(np.uint8))
        total += os.path.getsize(str(tmp_path / "a" / (name + ".npy")))
    assert total <= 64 * 10 ** 6
    # the primary frame whole and bit for bit; id exact as float64
    assert np.array_equal(np.load(str(tmp_path / "a" / "primary_id.npy")), prim[:, 0].astype(np.float64))
    for k, c in (("t", 1), ("u", 2), ("v", 3)):
        assert np.array_equal(np.load(str(tmp_path / "a" / ("primary_%s.npy" % k))).view(np.int32), prim[:, c])
    # the AO sample: records of the concatenated batches at sorted, distinct indices
    all_ao = np.concatenate(ao)
    got = np.load(str(tmp_path / "a" / "ao_t.npy")).view(np.int32)
    ids = np.load(str(tmp_path / "a" / "ao_id.npy"))
    idx = np.sort(np.random.default_rng(bench.DUMP_SAMPLE_SEED).choice(all_ao.shape[0], bench.DUMP_AO_RECORDS, replace=False))
    assert np.array_equal(got, all_ao[idx, 1]) and np.array_equal(ids, all_ao[idx, 0].astype(np.float64))
