"""TEST INFRASTRUCTURE: plain numpy models of the device cull (hfcl_scene_cull*) and of the fold over its list, the yardsticks of
tests/test_scene_cull_cpu.py (against the g++ build of hpp-fcl_amd/csrc/hfcl_cull.hpp) and tests/test_scene_cull_gpu.py."""
import numpy as np


def cull_queries(aabbs, pairs, inflate=0.0):
    """Host-side restatement of the cull (hfcl_scene_cull*): world boxes (n_conf, n_objects, 6) and the (n_pairs, 2) pair list ->
    (query_ids uint64 ascending, conf_begin uint64[n_conf + 1]).  A query q = c * n_pairs + p survives when the boxes of its two objects,
    each grown by `inflate` on every side, touch (closed intervals; a NaN keeps the pair)."""
    aabbs = np.asarray(aabbs, dtype=np.float64)
    pairs = np.asarray(pairs).reshape(-1, 2)
    n_conf = aabbs.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        lo, hi = aabbs[..., :3] - np.float64(inflate), aabbs[..., 3:] + np.float64(inflate)
        a_lo, a_hi, b_lo, b_hi = lo[:, pairs[:, 0]], hi[:, pairs[:, 0]], lo[:, pairs[:, 1]], hi[:, pairs[:, 1]]
        keep = ~((a_lo > b_hi).any(axis=-1) | (a_hi < b_lo).any(axis=-1))
    ids = np.flatnonzero(keep.reshape(-1)).astype(np.uint64)
    conf_begin = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.uint64) if n_conf else np.zeros(1, dtype=np.uint64)
    return ids, conf_begin


def fold_listed(abi, records, query_ids, n_conf, n_pairs, security_margin=None):
    """fold_records over a list: the records of the queries `query_ids` -> SCENE_SUMMARY_DTYPE[n_conf].  The records are scattered
    into a full (n_conf, n_pairs) table whose other entries do not count (a value no fold takes: NaN, no flags), and folded."""
    full = np.zeros(int(n_conf) * int(n_pairs), dtype=records.dtype)
    full["distance"] = np.nan
    full[np.asarray(query_ids, dtype=np.int64)] = records
    return abi.fold_records(full, n_pairs, security_margin)
