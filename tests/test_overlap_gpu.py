"""GPU parity of motifs_hits_occupancy_dev (post.occupancy): occupied positions, unique starts and the motif overlap sums are
exact against the literal restatement in tests/_overlap_ref.py, and post.overlap_ratio is bit-equal to its Float32 matrix, on
records from the library's own scan of synth data; hand-made adversarial lists; motif_map windows; read chunks; shards that add
up (two calls, and a 2-rank gloo run on one device); Fisher p-values end to end; and the configs[1] shape."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import _overlap_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu


def scan_records(ctx, pkg, bank, lens, codes, n0=0):
    """Both strands of the library's scan, left on the device: [(hits_t, n), (hits_t, n)]."""
    lib = pkg._lib
    N, L = codes.shape
    raw = torch.from_numpy(np.ascontiguousarray(codes)).cuda()
    dcodes = torch.zeros(lib.Context.codes_bytes(N, L), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.encode_dev(raw.data_ptr(), lib.DATA_CODES_U8, N, L, dcodes.data_ptr())
    out = []
    for rc in (False, True):
        n = ctx.pwm_scan_hits_dev(bank, lens, dcodes.data_ptr(), N, L, rc, None, None, 0, n0=n0)
        hits = torch.zeros((max(n, 1), 3), dtype=torch.int32, device="cuda")
        sc = torch.zeros(max(n, 1), dtype=torch.int16, device="cuda")
        ctx.pwm_scan_hits_dev(bank, lens, dcodes.data_ptr(), N, L, rc, hits.data_ptr(), sc.data_ptr(), n, n0=n0)
        ctx.synchronize()
        out.append((hits, sc, n))
    return out


def upload(rec):
    rec = np.ascontiguousarray(np.asarray(rec, dtype=np.int64).reshape(-1, 3))
    return torch.from_numpy(rec.astype(np.uint32).view(np.int32)).cuda() if len(rec) else None, len(rec)


def host(h, n):
    return h[:n].cpu().numpy().view(np.uint32).astype(np.int64) if n else np.zeros((0, 3), np.int64)


def check_against_restatement(ctx, pkg, strands_np, lens, N, L, n0=0, motif_map=None):
    """Device call on the records strands_np (list of (n, 3) arrays) vs the restatement on the dictionaries they make."""
    post = pkg.post
    K = len(lens)
    dev = [upload(r) for r in strands_np]
    occ, uq, ov = post.occupancy(ctx, dev, lens, N, L, n0=n0, motif_map=motif_map)
    positions = ref.records_to_positions(strands_np, K)
    sel, lens_sel = list(range(K)), lens
    if motif_map is not None:
        sel = [m for m in range(K) if motif_map[m] >= 0]
        sel.sort(key=lambda m: motif_map[m])
        positions = [positions[m] for m in sel]
        lens_sel = np.asarray([lens[m] for m in sel])
    olap, acs, pair = ref.get_overlap_ratio(positions, lens_sel)
    uniq, _ = ref.get_uniq_counts(positions, [{}] * len(positions))
    assert np.array_equal(occ, acs)
    assert np.array_equal(uq.astype(np.float64), uniq)
    assert np.array_equal(np.diag(ov), occ)
    assert np.array_equal(ov, ov.T)
    off = ~np.eye(len(sel), dtype=bool)
    assert (ov[off] < 2 ** 24).all()
    assert np.array_equal(ov[off].astype(np.float32), pair[off])
    got = post.overlap_ratio(occ, ov)
    assert np.array_equal(got.view(np.uint32), olap.view(np.uint32))
    return occ, uq, ov


SHAPES = [(1, 5, 12, 60, 300), (9, 5, 12, 200, 200), (65, 14, 20, 200, 120), (150, 30, 33, 1000, 30), (200, 5, 12, 60, 80)]


@pytest.mark.parametrize("K,lo,hi,L,N", SHAPES)
def test_occupancy_equals_restatement(ctx, pkg, K, lo, hi, L, N):
    sy, post = pkg.synth, pkg.post
    codes = sy.gen_codes(N, L, 900 + K, n_plant=4, k=min(lo, 10), frac=0.5)
    pwms, lens = sy.gen_pwm_bank(K, 901 + K, len_lo=lo, len_hi=hi, alpha=0.35)
    bank = sy.pad_bank(pwms, lens)
    strands = scan_records(ctx, pkg, bank, lens, codes)
    recs = [host(h, n) for h, _, n in strands]
    assert sum(len(r) for r in recs) > 0
    check_against_restatement(ctx, pkg, recs, lens, N, L)
    # ... and after the threshold filter (the records the reference's later steps see)
    filt = []
    for h, sc, n in strands:
        s = sc[:n].cpu().numpy().view(np.float16).astype(np.float32)
        m = host(h, n)[:, 0]
        thr = np.array([np.float16(np.quantile(s[m == k + 1], 0.4)) if (m == k + 1).any() else np.float16(0) for k in range(K)],
                       dtype=np.float16)
        oh, _, kept = post.filter_by_thresh(ctx, h, sc, n, thr)
        ctx.synchronize()
        filt.append(host(oh, kept))
    check_against_restatement(ctx, pkg, filt, lens, N, L)


def _adversarial(rng, K, N, L, lens, n0):
    fwd, rev = [], []
    for n in range(n0 + 1, n0 + N + 1):
        for m in range(1, K + 1):
            if m == 3 or rng.random() < 0.4:                 # motif 3 has no record at all
                continue
            ln = int(lens[m - 1])
            k = int(rng.integers(1, 5))
            starts = rng.integers(1, L - ln + 2, size=k)
            for s in starts:
                (fwd if rng.random() < 0.5 else rev).append((m, n, int(s)))
            if rng.random() < 0.3:                           # forward and reverse hits at the same start (the largest)
                mx = int(starts.max())
                fwd.append((m, n, mx))
                rev.append((m, n, mx))
            if rng.random() < 0.2:                           # a window ending at L
                fwd.append((m, n, L - ln + 1))
    for n in range(n0 + 1, n0 + N + 1, 7):                   # reads with exactly one record of motif 1
        fwd = [r for r in fwd if not (r[0] == 1 and r[1] == n)]
        rev = [r for r in rev if not (r[0] == 1 and r[1] == n)]
        fwd.append((1, n, int(rng.integers(1, L - int(lens[0]) + 2))))
    return np.array(fwd, np.int64).reshape(-1, 3), np.array(rev, np.int64).reshape(-1, 3)


def test_adversarial_lists(ctx, pkg):
    rng = np.random.default_rng(5)
    K, N, L, n0 = 7, 60, 90, 1234
    lens = np.array([4, 9, 6, 33, 1, 12, 90], np.int64)      # a window as long as the read, and one of a single position
    fwd, rev = _adversarial(rng, K, N, L, lens, n0)
    occ, uq, ov = check_against_restatement(ctx, pkg, [fwd, rev], lens, N, L, n0=n0)
    assert occ[2] == 0 and uq[2] == 0
    # the records shuffled, and split differently over the two arrays
    allr = np.concatenate([fwd, rev])
    p = rng.permutation(len(allr))
    o2 = pkg.post.occupancy(ctx, [upload(allr[p[: len(p) // 3]]), upload(allr[p[len(p) // 3:]])], lens, N, L, n0=n0)
    for a, b in zip(o2, (occ, uq, ov)):
        assert np.array_equal(a, b)
    # one array only
    o3 = pkg.post.occupancy(ctx, [upload(allr[p])], lens, N, L, n0=n0)
    assert np.array_equal(o3[2], ov)


@pytest.mark.parametrize("bad", ["past_L", "read_below", "read_above", "l_zero"])
def test_out_of_range_record_is_invalid(ctx, pkg, bad):
    lib = pkg._lib
    lens = np.array([5, 8], np.int64)
    N, L, n0 = 10, 40, 100
    rec = [(1, 101, 1), (2, 110, 33), (1, 105, 36)]
    rec.append({"past_L": (2, 103, 34), "read_below": (1, 100, 3), "read_above": (1, 111, 3), "l_zero": (2, 104, 0)}[bad])
    with pytest.raises(lib.MotifsError) as e:
        pkg.post.occupancy(ctx, [upload(rec)], lens, N, L, n0=n0)
    assert e.value.code == lib.ERR_INVALID
    # the context still works afterwards
    occ, _, _ = pkg.post.occupancy(ctx, [upload(rec[:3])], lens, N, L, n0=n0)
    assert list(occ) == [10, 8]                              # motif 1: reads 101 (1..5) and 105 (36..40); motif 2: 33..40


def test_motif_map_length_window(ctx, pkg):
    sy = pkg.synth
    K, N, L = 40, 150, 120
    codes = sy.gen_codes(N, L, 71, n_plant=3, k=8, frac=0.5)
    pwms, lens = sy.gen_pwm_bank(K, 72, len_lo=5, len_hi=16, alpha=0.35)
    strands = scan_records(ctx, pkg, sy.pad_bank(pwms, lens), lens, codes)
    recs = [host(h, n) for h, _, n in strands]
    # take_out_sub_ms_by_range_indicator!: the motifs with lengths in a window, in their order
    inside = [m for m in range(K) if 8 <= lens[m] <= 12]
    mm = np.full(K, -1, np.int32)
    mm[inside] = np.arange(len(inside), dtype=np.int32)
    occ, _, ov = check_against_restatement(ctx, pkg, recs, lens, N, L, motif_map=mm)
    assert ov.shape == (len(inside), len(inside))


def test_chunks_and_halves_add_up(ctx, pkg):
    sy, post, lib = pkg.synth, pkg.post, pkg._lib
    K, N, L = 70, 400, 150
    codes = sy.gen_codes(N, L, 81, n_plant=3, k=9, frac=0.5)
    pwms, lens = sy.gen_pwm_bank(K, 82, len_lo=6, len_hi=14, alpha=0.35)
    strands = scan_records(ctx, pkg, sy.pad_bank(pwms, lens), lens, codes)
    dev = [(h, n) for h, _, n in strands]
    whole = post.occupancy(ctx, dev, lens, N, L)
    # a workspace bound of a quarter of the reads: Nc = floor(limit / (4 (K + K16 W))) (include/motifs_hip.h) -> 4 chunks
    W, K16 = (L + 31) // 32, (K + 15) // 16 * 16
    per_read = 4 * (K + K16 * W)
    small = lib.Context(0)
    try:
        small.set_workspace_limit(per_read * (N // 4) + per_read // 2)
        assert -(-N // ((per_read * (N // 4) + per_read // 2) // per_read)) >= 3
        chunked = post.occupancy(small, dev, lens, N, L)
    finally:
        small.close()
    for a, b in zip(chunked, whole):
        assert np.array_equal(a, b)
    # two calls over the two halves of the reads add up to one call
    recs = [host(h, n) for h, n in dev]
    h = 173
    lo = post.occupancy(ctx, [upload(r[r[:, 1] <= h]) for r in recs], lens, h, L)
    hi = post.occupancy(ctx, [upload(r[r[:, 1] > h]) for r in recs], lens, N - h, L, n0=h)
    for a, b, c in zip(lo, hi, whole):
        assert np.array_equal(a + b, c)
    # an unused overlap output leaves the others as they are
    o2 = post.occupancy(ctx, dev, lens, N, L, overlap=False)
    assert o2[2] is None and np.array_equal(o2[0], whole[0]) and np.array_equal(o2[1], whole[1])


def _rank_worker(rank, ws, port, ret):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    sys.path.insert(0, ROOT)
    from _pkg import load_pkg

    pkg = load_pkg()
    ctx = pkg._lib.Context(0)
    reducer, _ = pkg.parallel.make_reducer(ctx, prefer_rccl=False)
    sy, post, par = pkg.synth, pkg.post, pkg.parallel
    K, N, L = 30, 300, 100
    codes = sy.gen_codes(N, L, 91, n_plant=3, k=8, frac=0.5)
    pwms, lens = sy.gen_pwm_bank(K, 92, len_lo=6, len_hi=12, alpha=0.35)
    lo, hi = par.shard_range(N, rank, ws)
    strands = scan_records(ctx, pkg, sy.pad_bank(pwms, lens), lens, codes[lo:hi], n0=lo)
    got = post.occupancy(ctx, [(h, n) for h, _, n in strands], lens, hi - lo, L, n0=lo, reducer=reducer)
    ret[f"got{rank}"] = got
    if rank == 0:
        whole = scan_records(ctx, pkg, sy.pad_bank(pwms, lens), lens, codes)
        ret["one"] = post.occupancy(ctx, [(h, n) for h, _, n in whole], lens, N, L)
    ctx.close()
    dist.destroy_process_group()


def test_two_ranks_sum_to_the_single_device_matrices():
    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ret = mp.Manager().dict()
    mp.spawn(_rank_worker, args=(2, port, ret), nprocs=2, join=True)
    ret = dict(ret)
    for r in range(2):
        for a, b in zip(ret[f"got{r}"], ret["one"]):
            assert np.array_equal(a, b)


def test_fisher_end_to_end(ctx, pkg):
    pytest.importorskip("scipy")
    sy, post, sc = pkg.synth, pkg.post, pkg.scan
    K, N, L = 24, 250, 100
    codes = sy.gen_codes(N, L, 101, n_plant=3, k=8, frac=0.6)
    bg = np.ascontiguousarray(np.random.default_rng(102).permuted(codes, axis=1))       # the reads' bases shuffled
    pwms, lens = sy.gen_pwm_bank(K, 103, len_lo=6, len_hi=10, alpha=0.3)
    bank = sy.pad_bank(pwms, lens)
    pos = []
    for c in (codes, bg):
        strands = scan_records(ctx, pkg, bank, lens, c)
        filt = []
        for h, s, n in strands:
            oh, _, kept = post.filter_by_thresh(ctx, h, s, n, np.full(K, np.float16(4.0)))
            ctx.synchronize()
            filt.append(host(oh, kept))
        pos.append(ref.records_to_positions(filt, K))
    assert sum(len(d) for d in pos[0]) > 0
    ms = sc.Motifs(pwms, lens)
    ms.positions, ms.positions_bg = pos
    data = sc.FastaData(sy.codes_to_onehot(codes).reshape(N, 1, 4 * L))
    want = ref.get_fisher_p_values(pos[0], pos[1], lens, N, L)
    got = post.get_fisher_p_values(ms, data, ctx=ctx)
    assert np.array_equal(got, want)
    assert (got < 1).any()
    u, ub = post.get_uniq_counts(ms, ctx=ctx)
    wu, wub = ref.get_uniq_counts(pos[0], pos[1])
    assert np.array_equal(u, wu) and np.array_equal(ub, wub)
    olap, _, _ = ref.get_overlap_ratio(pos[0], lens)
    assert np.array_equal(post.get_overlap_ratio(ms, L, ctx=ctx).view(np.uint32), olap.view(np.uint32))


def test_configs1_shape(ctx, pkg):
    """BASELINE configs[1]: 100 000 reads x 200 bp, 200 PWMs of length 12, both strands (the bench's own scan)."""
    sy, post, lib = pkg.synth, pkg.post, pkg._lib
    N, L, K = 100_000, 200, 200
    seed = sy.SEED_BASE + 2
    pwms, lens = sy.gen_pwm_bank(K, seed, len_lo=12, len_hi=12, alpha=0.3)
    codes = sy.gen_codes(N, L, seed, n_plant=5, k=12)
    strands = scan_records(ctx, pkg, sy.pad_bank(pwms, lens), lens, codes)
    dev = [(h, n) for h, _, n in strands]
    assert sum(n for _, n in dev) > 10_000_000
    occ, uq, ov = post.occupancy(ctx, dev, lens, N, L)
    assert np.array_equal(np.diag(ov), occ)
    assert np.array_equal(ov, ov.T)
    assert (ov <= np.minimum(occ[:, None], occ[None, :])).all()
    assert (uq <= occ).all() and (occ > 0).all()
    # a random 2 000-read subset: exact against the restatement (every motif's totals; the pair sums on a sample of pairs)
    rng = np.random.default_rng(3)
    subset = np.sort(rng.choice(np.arange(1, N + 1), size=2000, replace=False))
    sub_t = torch.from_numpy(subset).cuda()
    part, rest = [], []
    for h, n in dev:
        inside = torch.isin(h[:n, 1].long(), sub_t)
        part.append((h[:n][inside].contiguous(), int(inside.sum())))
        rest.append((h[:n][~inside].contiguous(), int((~inside).sum())))
    so, su, sov = post.occupancy(ctx, part, lens, N, L)
    ro, ru, rov = post.occupancy(ctx, rest, lens, N, L)
    assert np.array_equal(so + ro, occ) and np.array_equal(su + ru, uq) and np.array_equal(sov + rov, ov)
    positions = ref.records_to_positions([host(h, n) for h, n in part], K)
    unions = [ref.get_union_ranges(positions[i], int(lens[i])) for i in range(K)]
    assert np.array_equal(so, [ref.total_active_position(u) for u in unions])
    assert np.array_equal(su.astype(np.float64), ref.get_uniq_counts(positions, [{}] * K)[0])
    for _ in range(200):
        i, j = sorted(rng.choice(K, size=2, replace=False))
        o = 0
        for k in set(unions[i]) & set(unions[j]):
            for ri in unions[i][k]:
                for rj in unions[j][k]:
                    o += ref.num_overlap(ri, rj)
        assert sov[i, j] == o == sov[j, i]
