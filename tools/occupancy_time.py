"""Time motifs_hits_occupancy_dev (site occupancy, unique starts and the motif overlap sums, post.occupancy) on
  * BASELINE configs[1]: the scan's own records of 100 000 reads x 200 bp against 200 PWMs of length 12, both strands;
  * a synthetic K = 2048, N = 25 000, L = 1 000 case (random records, lengths 8-20), with the default workspace bound and with
    a 2 GiB one (read chunks);
and, for comparison, the host path: download the records, then the dictionary restatement (union ranges + the pair loop of
get_overlap_ratio) on a sample of reads, scaled up.  Prints one JSON line per case.
usage: python tools/occupancy_time.py [--reps 10] [--host-sample 40] [--no-big]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from _pkg import load_pkg

VALU_LANE_OPS = 256 * 128 * 2.4e9       # 256 CUs x 4 SIMD-32 x 32 lanes per clock at 2.4 GHz (the 157 TFLOPS FP32 vector peak / 2)


def time_calls(ctx, lib, post, dev, lens, N, L, reps):
    for _ in range(2):
        out = post.occupancy(ctx, dev, lens, N, L)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = post.occupancy(ctx, dev, lens, N, L)          # (the call drains the stream: it reads the range flag back)
        ts.append((time.perf_counter() - t0) * 1e3)
    # the library's share alone: the raw call on preallocated outputs, stage by stage with HIP events
    K = len(lens)
    occ = torch.zeros(K, dtype=torch.int64, device="cuda")
    uq = torch.zeros(K, dtype=torch.int64, device="cuda")
    ov = torch.zeros((K, K), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    (ha, na), (hb, nb) = dev
    raw = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ctx.hits_occupancy_dev(ha.data_ptr(), na, hb.data_ptr(), nb, 0, N, L, lens, None, K, occ.data_ptr(), uq.data_ptr(), ov.data_ptr())
        raw.append((time.perf_counter() - t0) * 1e3)
    slots = (lib.KS_OCC_RECORDS, lib.KS_OCC_ROWS, lib.KS_OCC_OVERLAP)
    ctx.enable_timing(True, slots=slots)
    ctx.reset_timing()
    for _ in range(reps):
        ctx.hits_occupancy_dev(ha.data_ptr(), na, hb.data_ptr(), nb, 0, N, L, lens, None, K, occ.data_ptr(), uq.data_ptr(), ov.data_ptr())
    stages = {name: ctx.kernel_ms(s)[0] / reps for name, s in zip(("records", "rows", "overlap"), slots)}
    ctx.enable_timing(False)
    W = (L + 31) // 32
    bound_ms = K * (K + 1) / 2 * N * W * 2 / VALU_LANE_OPS * 1e3
    return out, {"ms_per_call_post_occupancy": float(np.median(ts)), "ms_per_call_raw": float(np.median(raw)),
                 "stage_ms": stages, "overlap_valu_bound_ms": bound_ms, "overlap_fraction_of_valu_bound": bound_ms / stages["overlap"]}


def host_path(dev, lens, N, sample, seed=0):
    """Download both record arrays; then the dictionary restatement on `sample` reads, scaled to N."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    recs = [h[:n].cpu().numpy() for h, n in dev]
    d2h_ms = (time.perf_counter() - t0) * 1e3
    rec = np.concatenate(recs).view(np.uint32).astype(np.int64)
    rng = np.random.default_rng(seed)
    pick = np.sort(rng.choice(np.arange(1, N + 1), size=sample, replace=False))
    rec = rec[np.isin(rec[:, 1], pick)]
    K = len(lens)
    t0 = time.perf_counter()
    pos = [dict() for _ in range(K)]
    for m, n, l in rec:
        pos[m - 1].setdefault(n, []).append(l)
    unions = []
    for i in range(K):                                   # union_ranges with its quirk, per read
        u = {}
        for n, ls in pos[i].items():
            rs = sorted((l, l + lens[i] - 1) for l in ls)
            out = [rs[0]]
            for r in rs[:-1]:
                if out[-1][1] >= r[0]:
                    out[-1] = (out[-1][0], r[1])
                else:
                    out.append(r)
            u[n] = out
        unions.append(u)
    acs = [sum(b - a + 1 for rs in u.values() for a, b in rs) for u in unions]
    for i in range(K):                                   # the pair loop
        for j in range(i + 1, K):
            o = 0
            for k in unions[i].keys() & unions[j].keys():
                for a1, b1 in unions[i][k]:
                    for a2, b2 in unions[j][k]:
                        o += max(0, min(b1, b2) - max(a1, a2) + 1)
    dict_s = time.perf_counter() - t0
    return {"d2h_ms": d2h_ms, "d2h_bytes": int(sum(r.nbytes for r in recs)), "host_sample_reads": sample,
            "host_dict_s_sample": dict_s, "host_dict_s_scaled": dict_s * N / sample, "acs_sample_sum": int(sum(acs))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-sample", type=int, default=40)
    ap.add_argument("--no-big", action="store_true")
    args = ap.parse_args()
    pkg = load_pkg()
    lib, sy, post = pkg._lib, pkg.synth, pkg.post
    ctx = lib.Context(0)
    ctx.set_stream(0)
    # ---- configs[1] --------------------------------------------------------------------------------------------------
    N, L, K = 100_000, 200, 200
    seed = sy.SEED_BASE + 2
    pwms, lens = sy.gen_pwm_bank(K, seed, len_lo=12, len_hi=12, alpha=0.3)
    bank = sy.pad_bank(pwms, lens)
    codes = sy.gen_codes(N, L, seed, n_plant=5, k=12)
    raw = torch.from_numpy(codes).cuda()
    dcodes = torch.zeros(lib.Context.codes_bytes(N, L), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.encode_dev(raw.data_ptr(), lib.DATA_CODES_U8, N, L, dcodes.data_ptr())
    need = ctx.pwm_scan_hits_both_dev(bank, lens, dcodes.data_ptr(), N, L, None, None, 0)
    cap = max(need)
    hits = [torch.empty((cap, 3), dtype=torch.int32, device="cuda") for _ in range(2)]
    hsc = [torch.empty(cap, dtype=torch.int16, device="cuda") for _ in range(2)]
    got = ctx.pwm_scan_hits_both_dev(bank, lens, dcodes.data_ptr(), N, L, [h.data_ptr() for h in hits], [s.data_ptr() for s in hsc], cap)
    ctx.synchronize()
    dev = [(hits[0], got[0]), (hits[1], got[1])]
    out, res = time_calls(ctx, lib, post, dev, lens, N, L, args.reps)
    res.update({"case": "configs[1]", "N": N, "L": L, "K": K, "records": int(sum(got)),
                "checksum": [int(out[0].sum()), int(out[1].sum()), int(out[2].sum())]})
    res["host"] = host_path(dev, lens, N, args.host_sample)
    print(json.dumps(res), flush=True)
    del hits, hsc, dev
    torch.cuda.empty_cache()
    if args.no_big:
        return
    # ---- K = 2048, N = 25 000, L = 1 000 ----------------------------------------------------------------------------------
    N, L, K = 25_000, 1000, 2048
    g = torch.Generator(device="cuda").manual_seed(7)
    lens = np.random.default_rng(8).integers(8, 21, size=K).astype(np.int64)
    lens_t = torch.from_numpy(lens).cuda()
    dev = []
    for _ in range(2):
        n = 12_000_000
        m = torch.randint(1, K + 1, (n,), device="cuda", generator=g)
        rd = torch.randint(1, N + 1, (n,), device="cuda", generator=g)
        lmax = L - lens_t[m - 1] + 1
        l = (torch.rand(n, device="cuda", generator=g) * lmax).long() + 1
        dev.append((torch.stack([m, rd, l], 1).to(torch.int32).contiguous(), n))
    for limit_gib in (0, 2):
        c2 = lib.Context(0)
        c2.set_stream(0)
        if limit_gib:
            c2.set_workspace_limit(limit_gib << 30)
        W, K16 = (L + 31) // 32, (K + 15) // 16 * 16
        nc = max(1, min(N, ((limit_gib or 8) << 30) // (4 * (K + K16 * W))))
        out, res = time_calls(c2, lib, post, dev, lens, N, L, max(2, args.reps // 3))
        res.update({"case": "K2048_N25000_L1000", "workspace_limit_gib": limit_gib or 8, "chunks": -(-N // nc), "records": 2 * 12_000_000,
                    "checksum": [int(out[0].sum()), int(out[1].sum()), int(out[2].sum())]})
        print(json.dumps(res), flush=True)
        c2.close()


if __name__ == "__main__":
    main()
