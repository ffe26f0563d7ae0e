"""TEST INFRASTRUCTURE: plain numpy models of the device's self-collision pair lists (hfcl_scene_self_pairs*) and of the fold over such a
list, and the scenes tests/test_scene_pairs_cpu.py and tests/test_scene_pairs_gpu.py share.  The list of a configuration is
np.triu_indices(n, 1) filtered by the rule of cull_model.cull_queries; the fold is cull_model.fold_listed with an entry's rank inside
its configuration as its pair index."""
import numpy as np

import cull_model


def self_pairs(aabbs, inflate=0.0):
    """World boxes (n_conf, n_objects, 6) -> (pairs uint32 (n_listed, 2), conf_begin uint64[n_conf + 1]): for configuration c, then i,
    then j ascending, every (i < j) whose boxes, each grown by `inflate`, touch (closed intervals; a NaN keeps the pair)."""
    aabbs = np.asarray(aabbs, dtype=np.float64)
    n_conf, n = aabbs.shape[:2]
    i, j = np.triu_indices(n, 1)
    tri = np.stack([i, j], axis=1).astype(np.uint32)
    parts, conf_begin = [], np.zeros(n_conf + 1, dtype=np.uint64)
    for c in range(n_conf):  # (one configuration at a time: 37 x 179 700 candidate pairs at once are gigabytes)
        ids, _ = cull_model.cull_queries(aabbs[c:c + 1], tri, inflate)
        parts.append(tri[ids.astype(np.int64)])
        conf_begin[c + 1] = conf_begin[c] + np.uint64(len(ids))
    pairs = np.concatenate(parts) if parts else np.zeros((0, 2), dtype=np.uint32)
    return np.ascontiguousarray(pairs.reshape(-1, 2)), conf_begin


def conf_of(conf_begin):
    """The configuration of every list entry."""
    counts = np.diff(np.asarray(conf_begin).astype(np.int64))
    return np.repeat(np.arange(len(counts)), counts)


def fold_ranked(abi, records, conf_begin, security_margin=None):
    """The fold of hfcl_scene_*_pairs_device: SCENE_SUMMARY_DTYPE[n_conf]; an entry's pair index is its rank k - conf_begin[c]."""
    cb = np.asarray(conf_begin).astype(np.int64)
    n_conf = len(cb) - 1
    counts = np.diff(cb)
    width = max(int(counts.max()) if n_conf else 0, 1)
    c = conf_of(conf_begin)
    rank = np.arange(len(records)) - cb[:-1][c]
    return cull_model.fold_listed(abi, records, c * width + rank, n_conf, width, security_margin)


def expand(obj_shape, table, pairs, conf_begin):
    """The per-pair arrays a caller without scenes builds on the host: (s1, s2, rows1, rows2) of every list entry."""
    c = conf_of(conf_begin)
    i, j = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)
    return obj_shape[i], obj_shape[j], np.ascontiguousarray(table[c, i]), np.ascontiguousarray(table[c, j])


# ---- the scenes -----------------------------------------------------------------------------------------------------------------
SHARE_LO, SHARE_HI = 0.01, 0.30


def mixed_library(pkg, seed=3, nper=4):
    """cfg5's shape mix (Box, Sphere, Capsule, Ellipsoid, Convex32), nper of each."""
    return pkg.workloads._mixed_library(np.random.default_rng(seed), nper)


class PairScene:
    """n_conf configurations of n_objects posed objects of `lib`: configuration 0 has no touching pair (a lattice wider than any
    box), configuration 1 every pair (all objects at the origin), the others between SHARE_LO and SHARE_HI of all pairs -- each drawn
    again, with the model on the host's boxes, until its share is there (n_objects >= 5: below that no such share exists).  n_conf = 1
    is configuration `only` of the three."""

    def __init__(self, pkg, lib, n_objects, n_conf, seed=0, only=None):
        rng = np.random.default_rng([seed, n_objects, n_conf])
        self.lib, self.n, self.n_conf = lib, n_objects, n_conf
        self.obj_shape = rng.integers(0, len(lib), n_objects).astype(np.uint32)
        kinds = [0, 1, 2] if n_conf >= 3 else [only if only is not None else 2]
        kinds = (kinds + [2] * n_conf)[:n_conf]
        self.kinds = kinds
        quat = pkg.workloads.uniform_quaternions(rng, n_conf * n_objects).reshape(n_conf, n_objects, 4)
        T = np.zeros((n_conf, n_objects, 3))
        all_pairs = n_objects * (n_objects - 1) // 2
        side = 7.25  # (n^2 * 30.5 / (2 * 0.08 * n^2 / 2))^(1/3): about 8 % of the pairs for workloads' mix; shapes of this library are smaller
        for c, kind in enumerate(kinds):
            if kind == 0:
                g = int(np.ceil(n_objects ** (1.0 / 3.0)))
                k = np.arange(n_objects)
                T[c] = 6.0 * np.stack([k % g, (k // g) % g, k // (g * g)], axis=1)  # (no shape reaches 2 from its centre; boxes grown by 0.25 stay apart)
            elif kind == 2 and n_objects >= 2:
                for attempt in range(200):
                    T[c] = rng.uniform(-side / 2, side / 2, (n_objects, 3))
                    share = len(self._model(pkg, quat[c:c + 1], T[c:c + 1])[0]) / all_pairs
                    if n_objects < 5 or SHARE_LO <= share <= SHARE_HI:
                        break
                    if attempt % 20 == 19:
                        side *= 0.8 if share < SHARE_LO else 1.25
                else:
                    raise AssertionError("no placement with a share in range")
        self.quat, self.T = quat, T
        self.tf = pkg.geometry.make_pose(quat=quat.reshape(-1, 4), T=T.reshape(-1, 3)).reshape(n_conf, n_objects, 12)
        self.pose = pkg.geometry.pose_f32_from_quat(quat.reshape(-1, 4), T.reshape(-1, 3)).reshape(n_conf, n_objects, 7)
        wide = pkg.geometry.make_pose(quat=self.pose[..., :4].reshape(-1, 4).astype(np.float64),
                                      T=self.pose[..., 4:].reshape(-1, 3).astype(np.float64)).reshape(n_conf, n_objects, 12)
        self.boxes = self._host_boxes(pkg, self.tf)
        self.boxes32 = self._host_boxes(pkg, wide)
        self._lists = {}

    def _host_boxes(self, pkg, tf):
        return np.stack([pkg.engine.world_aabbs(self.lib, self.obj_shape, tf[c]) for c in range(len(tf))]).reshape(len(tf), self.n, 6)

    def _model(self, pkg, quat, T):
        tf = pkg.geometry.make_pose(quat=quat.reshape(-1, 4), T=T.reshape(-1, 3)).reshape(len(quat), self.n, 12)
        return self_pairs(self._host_boxes(pkg, tf), 0.0)

    def expected(self, f32=False, inflate=0.0):
        """The model's (pairs, conf_begin): computed once, shared, not modified."""
        key = (bool(f32), float(inflate))
        if key not in self._lists:
            self._lists[key] = self_pairs(self.boxes32 if f32 else self.boxes, inflate)
        return self._lists[key]

    def check_shares(self):
        """An empty list cannot pass for a correct one: the model's own output has a configuration without a pair, one with every pair,
        and the others in between."""
        pairs, cb = self.expected()
        counts = np.diff(cb.astype(np.int64))
        all_pairs = self.n * (self.n - 1) // 2
        for c, kind in enumerate(self.kinds):
            if kind == 0:
                assert counts[c] == 0, c
            elif kind == 1:
                assert counts[c] == all_pairs, c
            elif self.n >= 5:
                assert SHARE_LO * all_pairs <= counts[c] <= SHARE_HI * all_pairs, (c, counts[c], all_pairs)
        return counts
