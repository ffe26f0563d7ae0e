"""TEST INFRASTRUCTURE: plain numpy model of the clearance per configuration on device-made pairs (hfcl_scene_nearest_self*,
include/hppfcl_amd_nearest_self.h) -- the definition, written on the dense (i, j) matrix of a configuration, not on a list: the
candidates the groups allow, the bound of every candidate (nearest_model.bound), the seed pair, the two lists of pairs, the thresholds,
the two ranked folds and their combination.  The yardstick of tests/test_scene_nearest_self_cpu.py (against the g++ build of
hpp-fcl_amd/csrc/hfcl_nearest_self.hpp and against nearest_model.select on the explicit list) and tests/test_scene_nearest_self_gpu.py."""
import numpy as np

import nearest_model
import pairs_model

NO_PAIR = np.uint64(0xFFFFFFFFFFFFFFFF)
NONE = 0xFFFFFFFF


def allowed(n, groups=None):
    """(n, n) bool: the candidates (i, j), i < j; with groups = (object_group, collides) only those whose groups may pair."""
    cand = np.triu(np.ones((n, n), dtype=bool), 1)
    if groups is not None:
        g = np.asarray(groups[0]).astype(np.int64)
        masks = np.asarray(groups[1], dtype=np.uint64)
        cand &= ((masks[g][:, None] >> g[None, :].astype(np.uint64)) & np.uint64(1)).astype(bool)
    return cand


def explicit_list(n, groups=None):
    """P: every candidate in lexicographic order, uint32 (|P|, 2)."""
    return np.ascontiguousarray(np.argwhere(allowed(n, groups)).astype(np.uint32).reshape(-1, 2))


def no_record(abi, f32):
    r = np.zeros(1, dtype=abi.RESULT_F32_DTYPE if f32 else abi.RESULT_DTYPE)
    r["distance"] = np.inf
    r["status"] = 0x80000000
    if not f32:
        r["normal"] = r["p1"] = r["p2"] = np.nan
        r["b1"] = r["b2"] = -1
    return r[0]


def _listed(mask):
    """(pairs uint32 (k, 2), conf_begin, configuration of every entry) of a (n_conf, n, n) mask, in (c, i, j) order."""
    cij = np.argwhere(mask)
    conf_begin = np.concatenate([[0], np.cumsum(mask.reshape(len(mask), -1).sum(axis=1))]).astype(np.uint64)
    return np.ascontiguousarray(cij[:, 1:].astype(np.uint32).reshape(-1, 2)), conf_begin, cij[:, 0]


def select(abi, boxes, groups, records, upper_bound=np.inf, r=nearest_model.R64):
    """boxes (n_conf, n, 6); records: those of distance() on explicit_list(n, groups), n_conf * |P| of either precision, standing for
    what the narrow phase computes.  Returns a dict: seed (uint64[n_conf], (i << 32) | j), pairs1 / conf_begin1, thr, pairs2 /
    conf_begin2, summary1 / summary2 (the ranked folds), clearance (SCENE_CLEARANCE_DTYPE[n_conf]) and min_records."""
    boxes = np.asarray(boxes, dtype=np.float64)
    n_conf, n = boxes.shape[:2]
    D = np.float64(upper_bound)
    cand = allowed(n, groups)
    P = np.argwhere(cand)
    index = np.full((n, n), -1, dtype=np.int64)
    index[P[:, 0], P[:, 1]] = np.arange(len(P))
    L = nearest_model.bound(boxes[:, :, None, :], boxes[:, None, :, :], r) if n else np.zeros((n_conf, 0, 0))
    flat = np.where(cand[None], L, np.inf).reshape(n_conf, n * n)
    first = flat.argmin(axis=1) if n else np.zeros(n_conf, dtype=np.int64)  # (the first of equal values: the lowest (i, j))
    seed = ((first // max(n, 1)).astype(np.uint64) << np.uint64(32)) | (first % max(n, 1)).astype(np.uint64)
    if not cand.any():
        seed = np.full(n_conf, NO_PAIR, dtype=np.uint64)
    is_seed = np.zeros((n_conf, n * n), dtype=bool)
    if cand.any():
        is_seed[np.arange(n_conf), first] = True
    is_seed = is_seed.reshape(n_conf, n, n)
    pass1 = cand[None] & (np.isneginf(L) | is_seed) & (L <= D)
    out = dict(seed=seed)
    recs, sums, lists = [], [], []
    for l, mask in enumerate((pass1, None)):
        if l == 1:
            thr = np.where(sums[0]["min_distance"] < D, sums[0]["min_distance"], D)
            out["thr"] = thr
            mask = cand[None] & ~pass1 & (L <= thr[:, None, None])
        pairs, cb, conf = _listed(mask)
        rec = records[conf * len(P) + index[pairs[:, 0], pairs[:, 1]]]
        lists.append((pairs, cb))
        recs.append(rec)
        sums.append(pairs_model.fold_ranked(abi, rec, cb))
        out["pairs%d" % (l + 1)], out["conf_begin%d" % (l + 1)], out["summary%d" % (l + 1)] = pairs, cb, sums[l]
    clear = np.zeros(n_conf, dtype=abi.SCENE_CLEARANCE_DTYPE)
    f32 = records.dtype == abi.RESULT_F32_DTYPE
    min_records = np.zeros(n_conf, dtype=records.dtype)
    for c in range(n_conf):
        best = None
        for l in range(2):
            pairs, cb = lists[l]
            lo, hi = int(cb[c]), int(cb[c + 1])
            clear["n_evaluated"][c] += hi - lo
            if hi == lo:
                continue
            s = sums[l][c]
            clear["n_skipped"][c] += s["n_skipped"]
            if s["min_pair"] == NONE:
                continue
            k = lo + int(s["min_pair"])
            this = (float(s["min_distance"]), int(pairs[k, 0]), int(pairs[k, 1]), l, k)
            if best is None or this[:3] < best[:3]:
                best = this
        if best is None:
            clear["min_distance"][c], clear["min_i"][c], clear["min_j"][c] = np.inf, NONE, NONE
            min_records[c] = no_record(abi, f32)
        else:
            clear["min_distance"][c] = sums[best[3]]["min_distance"][c]
            clear["min_i"][c], clear["min_j"][c] = best[1], best[2]
            min_records[c] = recs[best[3]][best[4]]
    out["clearance"], out["min_records"] = clear, min_records
    return out


def check_against_full(abi, sel, P, records, upper_bound=np.inf):
    """What the header promises against distance() on P: wherever the unpruned minimum is <= upper_bound the same bits, the pair
    P[min_pair] and that query's record; elsewhere min_distance > upper_bound.  Returns the number of configurations beyond the bound."""
    full = abi.fold_records(records, len(P), None)
    clear = sel["clearance"]
    near = full["min_distance"] <= upper_bound
    assert clear["min_distance"][near].tobytes() == full["min_distance"][near].tobytes()
    mp = full["min_pair"][near].astype(np.int64)
    assert np.array_equal(clear["min_i"][near], P[mp, 0]) and np.array_equal(clear["min_j"][near], P[mp, 1])
    want = records.reshape(len(full), len(P))[np.flatnonzero(near), mp]
    assert sel["min_records"][near].tobytes() == want.tobytes()
    assert np.all(clear["min_distance"][~near] > upper_bound)
    return int((~near).sum())
