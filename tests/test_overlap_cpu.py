"""Site occupancy, unique starts and the motif overlap (Jaccard) matrix without a GPU: the restatement in tests/_overlap_ref.py
pins the union_ranges quirk on hand-made dictionaries; post.overlap_ratio / connected_components / fisher_pvec equal it on random
inputs; the new C entry point refuses a NULL context; the Julia shim binds it."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import _overlap_ref as ref  # noqa: E402


# ---- the quirk of union_ranges (_h4_overlap_ratio.jl:48-56), pinned in the restatement -------------------------------------
def test_one_window_is_kept():
    u = ref.get_union_ranges({7: [3]}, 5)
    assert u == {7: [(3, 7)]}
    assert ref.total_active_position(u) == 5


def test_two_disjoint_windows_only_the_first_counts():
    u = ref.get_union_ranges({1: [20, 2]}, 4)
    assert u == {1: [(2, 5)]}
    assert ref.total_active_position(u) == 4


def test_overlapping_windows_lose_the_last_one():
    # 2..6 and 4..8 overlap; the window of the largest start (4) is still never merged in
    assert ref.total_active_position(ref.get_union_ranges({1: [4, 2]}, 5)) == 5
    # three windows: the first two merge, the third (largest start) is dropped
    assert ref.total_active_position(ref.get_union_ranges({1: [1, 3, 30]}, 4)) == 6


def test_duplicated_max_start_is_still_covered():
    # a forward and a reverse-complement hit at the same start: one copy is dropped, the other covers it
    u = ref.get_union_ranges({1: [10, 2, 10]}, 3)
    assert u == {1: [(2, 4), (10, 12)]}
    assert ref.total_active_position(u) == 6


def test_unsorted_positions():
    assert ref.get_union_ranges({4: [9, 1, 5]}, 2) == {4: [(1, 2), (5, 6)]}


def test_uniq_counts_and_overlap_of_hand_made_dicts():
    pos = [{1: [1, 5, 1], 2: [3]}, {1: [2, 40]}, {}]
    lens = [4, 3, 2]
    u, _ = ref.get_uniq_counts(pos, [{}, {}, {}])
    assert list(u) == [3.0, 2.0, 0.0]
    olap, acs, pair = ref.get_overlap_ratio(pos, lens)
    # motif 1: read 1 windows 1..4 twice (duplicate start 1) and 5..8 (largest, once: dropped) -> 1..4; read 2: 3..6 -> 8 positions
    # motif 2: read 1 windows 2..4, 40..42 (dropped) -> 3 positions
    assert list(acs) == [8, 3, 0]
    assert pair[0, 1] == 3 and olap[0, 1] == np.float32(3) / np.float32(8 + 3 - 3)
    assert olap[0, 2] == 0 and np.isnan(olap[2, 2]) == False and olap[2, 2] == 0   # the diagonal stays 0
    # two empty motifs: 0 / 0
    olap2, _, _ = ref.get_overlap_ratio([{}, {}], [3, 3])
    assert np.isnan(olap2[0, 1]) and np.isnan(olap2[1, 0])


# ---- the host parts of the product equal the restatement --------------------------------------------------------------------
def _random_dicts(rng, K, N, L, lens, empty=()):
    pos = []
    for i in range(K):
        d = {}
        if i not in empty:
            for n in rng.choice(np.arange(1, N + 1), size=rng.integers(0, N), replace=False):
                starts = rng.integers(1, L - lens[i] + 2, size=rng.integers(1, 5)).tolist()
                if rng.random() < 0.3:
                    starts.append(starts[0])            # a start on both strands
                d[int(n)] = starts
        pos.append(d)
    return pos


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_overlap_ratio_equals_restatement(pkg, seed):
    rng = np.random.default_rng(seed)
    K, N, L = 12, 30, 40
    lens = rng.integers(3, 12, size=K)
    pos = _random_dicts(rng, K, N, L, lens, empty=(4, 9))
    olap, acs, pair = ref.get_overlap_ratio(pos, lens)
    ov = pair.astype(np.int64)
    np.fill_diagonal(ov, acs)
    got = pkg.post.overlap_ratio(acs, ov)
    assert got.dtype == np.float32
    assert np.isnan(got[4, 9]) and np.isnan(olap[4, 9])
    assert np.array_equal(got.view(np.uint32), olap.view(np.uint32))


@pytest.mark.parametrize("seed,thresh", [(5, 0.2), (6, 0.5), (7, 0.8), (8, 0.05)])
def test_connected_components_equals_restatement(pkg, seed, thresh):
    rng = np.random.default_rng(seed)
    K = 40
    m = rng.random((K, K)).astype(np.float32) ** 3
    m = np.maximum(m, m.T)
    m[rng.integers(0, K, 5), :] = np.nan                    # NaN rows: never above the threshold
    np.fill_diagonal(m, 0)
    want = ref.return_connected_components(m, thresh)
    got = pkg.post.connected_components(m, thresh)
    assert [[j + 1 for j in t] for t in got] == want
    assert sorted(j for t in got for j in t) == list(range(K))


def test_fisher_pvec_equals_restatement(pkg):
    pytest.importorskip("scipy")
    rng = np.random.default_rng(11)
    N, L = 500, 100
    a = rng.integers(0, 3000, size=30)
    b = rng.integers(0, 3000, size=30)
    a[3] = b[3] = 0
    a[7] = 0
    want = ref.fisher_pvec(a, b, N, L)
    got = pkg.post.fisher_pvec(a, b, N, L)
    assert got[3] == 1.0
    assert np.array_equal(got, want)


# ---- the C entry point and the Julia shim ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built(pkg):
    if not os.path.exists(pkg._lib.LIB_PATH):
        from _pkg import load_build

        load_build().build(verbose=False)
    return pkg


def test_occupancy_entry_refuses_a_null_context(built):
    lib = built._lib.lib()
    assert "motifs_hits_occupancy_dev" in built._lib.SIGNATURES
    lens = np.full(3, 5, dtype=np.int64)
    occ = np.zeros(3, dtype=np.int64)
    rc = lib.motifs_hits_occupancy_dev(None, None, 0, None, 0, 0, 10, 50, lens.ctypes.data_as(ctypes.c_void_p), 3, None, 3,
                                       occ.ctypes.data_as(ctypes.c_void_p), None, None)
    assert rc == built._lib.ERR_INVALID
    assert "null context" in lib.motifs_last_error().decode()


def test_julia_shim_binds_occupancy():
    text = open(os.path.join(ROOT, "julia", "MotifsHIP.jl")).read()
    assert re.search(r"ccall\(\(:motifs_hits_occupancy_dev, lib\)", text)
    for fn in ("function hits_occupancy!(", "function get_overlap_ratio(ms", "function get_fisher_p_values(ms, data"):
        assert fn in text, fn
