"""TEST INFRASTRUCTURE: plain numpy model of the per-configuration minimum distance with box-bound pruning (hfcl_scene_nearest*,
include/hppfcl_amd_nearest.h) -- the definition: the bound L of a query from its two world boxes, the seeds, the two lists, the thresholds.
The yardstick of tests/test_scene_nearest_cpu.py (against the g++ build of hpp-fcl_amd/csrc/hfcl_nearest.hpp) and
tests/test_scene_nearest_gpu.py."""
import numpy as np

import cull_model

R64 = 2.0 ** -40
R32 = 2.0 ** -18
INFLATION_SLACK = 2e-10


def raw_bound(a, b):
    """(lb, e, M) of boxes a, b (..., 6): the distance between the boxes (0 where they touch), the sum of their diagonals, their largest
    absolute coordinate.  The operation order is the header's."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        g = np.maximum(a[..., :3] - b[..., 3:], b[..., :3] - a[..., 3:])
        g = np.where(g > 0.0, g, 0.0)
        lb = np.sqrt((g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2])
        da, db = a[..., 3:] - a[..., :3], b[..., 3:] - b[..., :3]
        e = (np.sqrt((da[..., 0] * da[..., 0] + da[..., 1] * da[..., 1]) + da[..., 2] * da[..., 2]) +
             np.sqrt((db[..., 0] * db[..., 0] + db[..., 1] * db[..., 1]) + db[..., 2] * db[..., 2]))
        M = np.maximum(np.abs(a).max(axis=-1), np.abs(b).max(axis=-1))
    return lb, e, M


def bound(a, b, r=R64):
    """L(q): lb - (2e-10 * e + r * M); -inf where the boxes touch (closed intervals) or anything is not finite."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    lb, e, M = raw_bound(a, b)
    with np.errstate(invalid="ignore", over="ignore"):
        L = lb - (INFLATION_SLACK * e + np.float64(r) * M)
        apart = ((a[..., :3] - b[..., 3:] > 0.0) | (b[..., :3] - a[..., 3:] > 0.0)).any(axis=-1)
    ok = np.isfinite(a).all(axis=-1) & np.isfinite(b).all(axis=-1) & apart & np.isfinite(L)
    return np.where(ok, L, -np.inf)


def query_bounds(aabbs, pairs, r=R64):
    """L of every query: (n_conf, n_pairs) from the world boxes (n_conf, n_objects, 6) and the (n_pairs, 2) pair list."""
    aabbs = np.asarray(aabbs, dtype=np.float64)
    pairs = np.asarray(pairs).reshape(-1, 2)
    return bound(aabbs[:, pairs[:, 0]], aabbs[:, pairs[:, 1]], r)


def _listed(mask):
    ids = np.flatnonzero(mask.reshape(-1)).astype(np.uint64)
    conf_begin = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.uint64)
    return ids, conf_begin


def select(abi, L, records, upper_bound=np.inf):
    """The two passes on the bounds L (n_conf, n_pairs) with `records` (n_conf * n_pairs, either precision) standing for what the narrow
    phase computes.  Returns a dict: seed (uint32[n_conf]), ids1 / conf_begin1, thr (float64[n_conf]), ids2 / conf_begin2, and summary --
    the fold over the evaluated records."""
    n_conf, n_pairs = L.shape
    D = np.float64(upper_bound)
    seed = L.argmin(axis=1).astype(np.uint32)  # (the first of equal values: the lowest p)
    p = np.arange(n_pairs)[None, :]
    pass1 = (np.isneginf(L) | (p == seed[:, None])) & (L <= D)
    ids1, cb1 = _listed(pass1)
    s1 = cull_model.fold_listed(abi, records[ids1.astype(np.int64)], ids1, n_conf, n_pairs, None)
    thr = np.where(s1["min_distance"] < D, s1["min_distance"], D)
    pass2 = ~pass1 & (L <= thr[:, None])
    ids2, cb2 = _listed(pass2)
    both = np.flatnonzero((pass1 | pass2).reshape(-1))
    summary = cull_model.fold_listed(abi, records[both], both.astype(np.uint64), n_conf, n_pairs, None)
    return dict(seed=seed, ids1=ids1, conf_begin1=cb1, thr=thr, ids2=ids2, conf_begin2=cb2, summary=summary)


def check_against_full(summary, full_summary, upper_bound=np.inf):
    """What the header promises: min_distance / min_pair equal the unculled summary's where its minimum is <= upper_bound, and
    min_distance > upper_bound elsewhere.  Returns the number of configurations beyond the bound."""
    near = full_summary["min_distance"] <= upper_bound
    assert summary["min_distance"][near].tobytes() == full_summary["min_distance"][near].tobytes()
    assert summary["min_pair"][near].tobytes() == full_summary["min_pair"][near].tobytes()
    assert np.all(summary["min_distance"][~near] > upper_bound)
    return int((~near).sum())
