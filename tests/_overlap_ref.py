"""Literal restatement of the reference's occupancy / overlap / Fisher helpers over Julia-style dictionaries
({read: [start, ...]} per motif, the shape of ms.positions), line by line, for the tests.  Test infrastructure only: the
product does not import it.  Indices inside the dictionaries are 1-based as in the reference; motif indices returned by
return_connected_components are 1-based as well."""
import numpy as np


def unique_positions(positions_array):                     # _h4_overlap_ratio.jl:1
    out = []
    for p in positions_array:
        if p not in out:
            out.append(p)
    return out


def get_uniq_pos(positions_i):                             # _h4:5-11
    return {k: unique_positions(v) for k, v in positions_i.items()}


def active_counts_position(positions):                     # _h7_fisher.jl:1-12 (Float64 per motif)
    out = np.zeros(len(positions), dtype=np.float64)
    for i, d in enumerate(positions):
        s = 0
        for k in d:
            s += len(d[k])
        out[i] = s
    return out


def get_uniq_counts(positions, positions_bg):              # _h4:13-15
    return (active_counts_position([get_uniq_pos(d) for d in positions]),
            active_counts_position([get_uniq_pos(d) for d in positions_bg]))


def num_overlap(r1, r2):                                   # _h4:19-28; ranges are (first, last), inclusive
    assert r1[0] <= r1[1] and r2[0] <= r2[1], "range is not valid"
    if r1[0] <= r2[0] <= r1[1]:
        return min(r1[1], r2[1]) - r2[0] + 1
    elif r2[0] <= r1[0] <= r2[1]:
        return min(r1[1], r2[1]) - r1[0] + 1
    return 0


def total_active_position(position):                       # _h4:30-38
    c = 0
    for key in position:
        for r in position[key]:
            c += r[1] - r[0] + 1
    return c


def push_ranges(ranges, _ranges_, i):                      # _h4:40-46 (i is 1-based)
    if _ranges_[-1][1] >= ranges[i - 1][0]:
        _ranges_[-1] = (_ranges_[-1][0], ranges[i - 1][1])
    else:
        _ranges_.append(ranges[i - 1])


def union_ranges(ranges):                                  # _h4:48-56
    if len(ranges) == 0:
        return []
    ranges = sorted(ranges, key=lambda x: x[0])
    _ranges_ = [ranges[0]]
    for i in range(1, len(ranges[1:]) + 1):                # eachindex(@view ranges[2:end]) = 1 .. n-1: pushes ranges[i], not ranges[i+1]
        push_ranges(ranges, _ranges_, i)
    return _ranges_


def union_pos(positions_arr_k, len_):                      # _h4:58-61
    return union_ranges([(p, p + len_ - 1) for p in positions_arr_k])


def get_union_ranges(positions_i, len_i):                  # _h4:63-69
    return {k: union_pos(v, len_i) for k, v in positions_i.items()}


def get_total_occupied_positions(position_ranges):        # _h4:71-79
    return total_active_position(position_ranges)


def get_overlap_ratio(positions, lens):                    # _h4:86-117, Float32 accumulation of the pair sum
    K = len(positions)
    union_poses = [get_union_ranges(positions[i], int(lens[i])) for i in range(K)]
    acs = [total_active_position(u) for u in union_poses]
    olap = np.zeros((K, K), dtype=np.float32)
    pair = np.zeros((K, K), dtype=np.float32)              # (the Float32 sums themselves, for the exactness checks)
    for i in range(K):
        for j in range(i + 1, K):
            pos_i, pos_j = union_poses[i], union_poses[j]
            overlap_ij = np.float32(0)
            for k in set(pos_i) & set(pos_j):
                if len(pos_i[k]) == 0:                     # `a || b && continue` is `a || (b && continue)`: an empty
                    pass                                   # pos_i[k] falls through to loops that add nothing
                elif len(pos_j[k]) == 0:
                    continue
                for ri in pos_i[k]:
                    for rj in pos_j[k]:
                        overlap_ij = np.float32(overlap_ij + np.float32(num_overlap(ri, rj)))
            den = np.float32(np.float32(acs[i] + acs[j]) - overlap_ij)
            with np.errstate(divide="ignore", invalid="ignore"):
                olap[i, j] = olap[j, i] = np.float32(overlap_ij / den)
            pair[i, j] = pair[j, i] = overlap_ij
    return olap, np.array(acs, dtype=np.int64), pair


def fisher_pvec(a, b, N, L):                               # _h7:21-36 (activate_sum = N L; N_test when test)
    from scipy.stats import fisher_exact

    s = N * L
    out = np.zeros(len(a), dtype=np.float64)
    for i in range(len(a)):
        ai, bi = int(a[i]), int(b[i])
        c, d = s - ai, s - bi
        if ai == 0 and bi == 0:
            out[i] = 1.0
        else:
            out[i] = fisher_exact([[ai, c], [bi, d]], alternative="greater")[1]
    return out


def get_fisher_p_values(positions, positions_bg, lens, N, L):   # _h7:38-44
    tp = [get_total_occupied_positions(get_union_ranges(d, int(lens[i]))) for i, d in enumerate(positions)]
    tb = [get_total_occupied_positions(get_union_ranges(d, int(lens[i]))) for i, d in enumerate(positions_bg)]
    return fisher_pvec(tp, tb, N, L)


def return_connected_components(olap_ratio, jaccard_thresh=0.8):   # _h8_remove_redundancy.jl:73-104
    A = np.asarray(olap_ratio) > jaccard_thresh
    n = A.shape[0]
    marked = [False] * n
    trees = []
    for i in range(1, n + 1):
        start = i
        queue = []                                         # Deque: pushfirst! at the front, pop! from the back
        if not marked[i - 1]:
            marked[i - 1] = True
            subtree = [start]
            queue.insert(0, start)
            while len(queue) != 0:
                v = queue.pop()
                for j in [x + 1 for x in np.nonzero(A[v - 1, :] > 0)[0]]:
                    if not marked[j - 1]:
                        marked[j - 1] = True
                        subtree.append(j)
                        queue.insert(0, j)
            trees.append(subtree)
    return trees


def records_to_positions(recs, K):
    """(m, n, l) records of any number of arrays, in order -> ms.positions (modify_w_found! pushes in record order)."""
    pos = [dict() for _ in range(K)]
    for r in recs:
        for m, n, l in np.asarray(r, dtype=np.int64).reshape(-1, 3):
            pos[m - 1].setdefault(int(n), []).append(int(l))
    return pos
