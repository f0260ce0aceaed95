"""bench.py --dump-outputs: the sample of the last step's records is fixed by the hit totals, exact in float32 and
within 64 MB, on host tensors shaped like a shard of bench.py's timed step."""
import os

import numpy as np
import torch

import bench


def _shard(n_hits, K=200, seed=0):
    rng = np.random.default_rng(seed)
    cap = max(n_hits) + 16
    hits = [torch.from_numpy(rng.integers(1, 100_001, size=(cap, 3), dtype=np.int32)) for _ in range(2)]
    hsc = [torch.from_numpy(rng.uniform(0.01, 30.0, cap).astype(np.float16).view(np.int16)) for _ in range(2)]
    counts = torch.from_numpy(rng.integers(0, 1 << 40, size=(2, K), dtype=np.int64))
    return {"hits": hits, "hsc": hsc, "counts": counts}


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_sampled_exact_and_repeatable(tmp_path):
    totals = (3_000_000, 2_500_000)          # past DUMP_SAMPLE: the records go as a sample
    sh = _shard(totals)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), sh, totals)
    bench.dump_outputs(str(b), sh, totals)
    got, again = _load(a), _load(b)
    assert set(got) == {"hit_totals", "hit_counts", "hits_fwd", "scores_fwd", "hits_fwd_rows", "hits_rev", "scores_rev", "hits_rev_rows"}
    assert sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a)) <= 64 << 20
    for k in got:
        assert got[k].dtype in (np.float32, np.float64), k
        assert np.array_equal(got[k], again[k]), k
    assert np.array_equal(got["hit_totals"], np.array(totals, dtype=np.float64))
    assert np.array_equal(got["hit_counts"].astype(np.int64), sh["counts"].numpy())
    for rc, tag in enumerate(("fwd", "rev")):
        rows = got[f"hits_{tag}_rows"].astype(np.int64)
        assert 0 < len(rows) <= bench.DUMP_SAMPLE and rows[-1] < totals[rc] and np.all(np.diff(rows) > 0)
        assert np.array_equal(got[f"hits_{tag}"].astype(np.int32), sh["hits"][rc].numpy()[rows])
        assert np.array_equal(got[f"scores_{tag}"], sh["hsc"][rc].numpy()[rows].view(np.float16).astype(np.float32))


def test_dump_outputs_small_step_is_whole(tmp_path):
    totals = (1000, 0)
    sh = _shard((1000, 1))
    bench.dump_outputs(str(tmp_path), sh, totals)
    got = _load(tmp_path)
    assert np.array_equal(got["hits_fwd"].astype(np.int32), sh["hits"][0].numpy()[:1000])
    assert got["hits_rev"].shape == (0, 3) and got["scores_rev"].shape == (0,)
