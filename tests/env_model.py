"""TEST INFRASTRUCTURE: the numpy model of a scene with a static environment (include/hppfcl_amd_env.h) and the scenes
tests/test_scene_env_cpu.py and tests/test_scene_env_gpu.py share.  The env list is pairs_model.self_pairs / groups_model.self_pairs of the
FULL tables' boxes -- the moving rows of a configuration followed by the environment's -- with every entry i >= n_moving removed and
conf_begin recounted.  The tile boxes are the header's fold, member by member, in numpy; what the sweep skips by them is counted from the
boxes alone, as groups_model.skipped counts what it skips by the groups."""
import numpy as np

import groups_model
import pairs_model

TILE = groups_model.TILE  # hfcl_pairs.hpp: PAIRS_TILE
ROWS = groups_model.ROWS  # hfcl_pairs.hpp: PAIRS_ROWS
SHARE_LO, SHARE_HI = 0.01, 0.30
SHARE_MIN_ALLOWED = 100   # (scenes with fewer allowed pairs have no list between 1 % and 30 % of them worth the name: (1, 1) has one pair)


def filter_moving(pairs, conf_begin, n_moving):
    """A list of the full scene -> the env list: the entries with i < n_moving, conf_begin recounted."""
    keep = pairs[:, 0] < n_moving if len(pairs) else np.zeros(0, dtype=bool)
    conf = pairs_model.conf_of(conf_begin)
    counts = np.bincount(conf[keep], minlength=len(conf_begin) - 1).astype(np.uint64)
    cb = np.concatenate([[np.uint64(0)], np.cumsum(counts, dtype=np.uint64)]).astype(np.uint64)
    return np.ascontiguousarray(pairs[keep].reshape(-1, 2)), cb


def env_pairs(full_boxes, n_moving, inflate=0.0, group=None, words=None):
    """World boxes (n_conf, n_objects, 6) of the full tables -> (pairs uint32 (n_listed, 2), conf_begin uint64[n_conf + 1])."""
    if group is None:
        pairs, cb = pairs_model.self_pairs(full_boxes, inflate)
    else:
        pairs, cb = groups_model.self_pairs(full_boxes, inflate, group, words)
    return filter_moving(pairs, cb, n_moving)


def n_allowed(n_moving, n_env):
    return n_moving * (n_moving - 1) // 2 + n_moving * n_env


# ---- the tile rule ------------------------------------------------------------------------------------------------------------------
def fold_boxes(boxes):
    """(m, 6) boxes -> their box by the header's rule: per coordinate the fold in member order from +inf / -inf, m = x < m ? x : m (max:
    x > M ? x : M), a NaN member coordinate making that coordinate -inf / +inf for good."""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 6)
    m = np.concatenate([np.full(3, np.inf), np.full(3, -np.inf)])
    dead = np.zeros(6, dtype=bool)
    with np.errstate(invalid="ignore"):
        for x in b:
            lower = np.concatenate([x[:3] < m[:3], x[3:] > m[3:]])
            m = np.where(lower, x, m)
            dead |= np.isnan(x)
    return np.where(dead, np.concatenate([np.full(3, -np.inf), np.full(3, np.inf)]), m)


def tile_boxes(env_boxes):
    """(n_env, 6) -> (ceil(n_env / TILE), 6): tile t holds the environment objects [t TILE, (t + 1) TILE)."""
    b = np.asarray(env_boxes, dtype=np.float64).reshape(-1, 6)
    n_tiles = (len(b) + TILE - 1) // TILE
    out = np.zeros((n_tiles, 6))
    # the fold of all tiles at once, member by member (the same sequence of comparisons as fold_boxes)
    m = np.tile(np.concatenate([np.full(3, np.inf), np.full(3, -np.inf)]), (n_tiles, 1))
    dead = np.zeros((n_tiles, 6), dtype=bool)
    with np.errstate(invalid="ignore"):
        for k in range(TILE):
            idx = np.arange(n_tiles) * TILE + k
            live = idx < len(b)
            x = b[np.minimum(idx, len(b) - 1)] if len(b) else np.zeros((0, 6))
            lower = np.concatenate([x[:, :3] < m[:, :3], x[:, 3:] > m[:, 3:]], axis=1) & live[:, None]
            m = np.where(lower, x, m)
            dead |= np.isnan(x) & live[:, None]
    out[:] = np.where(dead, np.concatenate([np.full(3, -np.inf), np.full(3, np.inf)])[None, :], m)
    return out


def grow(boxes, inflate):
    b = np.array(boxes, dtype=np.float64, copy=True)
    b[..., :3] -= inflate
    b[..., 3:] += inflate
    return b


def touch(a, b):
    """cull_boxes_touch: closed intervals, every comparison false on a NaN."""
    with np.errstate(invalid="ignore"):
        return ~((a[..., 0] > b[..., 3]) | (a[..., 1] > b[..., 4]) | (a[..., 2] > b[..., 5]) |
                 (a[..., 3] < b[..., 0]) | (a[..., 4] < b[..., 1]) | (a[..., 5] < b[..., 2]))


def skipped_by_box(full_boxes, n_moving, inflate=0.0):
    """Per configuration: (cells skipped, cells) of the sweep's (row block, environment tile) cells -- a cell is skipped when the tile's
    grown box does not touch the union of the block's rows' grown boxes.  Also returns the mask (n_conf, blocks, tiles)."""
    fb = np.asarray(full_boxes, dtype=np.float64)
    n_conf = fb.shape[0]
    tb = grow(tile_boxes(fb[0, n_moving:]), inflate)  # (the environment is the same in every configuration)
    n_blocks = (n_moving + ROWS - 1) // ROWS
    mask = np.zeros((n_conf, n_blocks, len(tb)), dtype=bool)
    for c in range(n_conf):
        for b in range(n_blocks):
            u = fold_boxes(grow(fb[c, b * ROWS:min((b + 1) * ROWS, n_moving)], inflate))
            mask[c, b] = ~touch(u[None, :], tb)
    return mask.reshape(n_conf, -1).sum(axis=1), n_blocks * len(tb), mask


# ---- the scenes -----------------------------------------------------------------------------------------------------------------
class EnvScene:
    """n_conf configurations of n_moving posed objects of `lib` (cfg5's shape mix) among n_env objects that stand still.  The environment is
    generated as slabs along x, a slab per tile of TILE consecutive objects, with gaps between the slabs that no box bridges: tiles are
    compact.  The moving objects of a row block (ROWS consecutive objects) of configuration c >= 1 sit next to members of slab
    (block + c) % tiles, so every tile is met and every block skips the other slabs; in configuration 0 they sit far from everything.
    The slab's size is drawn
    again, with the model on the host's boxes, until the listing configurations hold between SHARE_LO and SHARE_HI of the allowed pairs
    (scenes with at least SHARE_MIN_ALLOWED of them).  check() asserts what this promises on the model's output."""

    GAP = 12.0  # between slabs: no box of this library reaches 2 from its centre, grown by 0.25, and a moving object sits within `near` of a member

    def __init__(self, pkg, lib, n_moving, n_env, n_conf, seed=0):
        rng = np.random.default_rng([seed, n_moving, n_env, n_conf])
        self.lib, self.n_moving, self.n_env, self.n_conf = lib, n_moving, n_env, n_conf
        self.n = n = n_moving + n_env
        self.obj_shape = rng.integers(0, len(lib), n).astype(np.uint32)
        self.n_tiles = (n_env + TILE - 1) // TILE
        assert n_conf >= 2  # (the tests take n_conf = 1 as the configurations of a three-configuration scene one by one)
        self.kinds = [0] + [1] * (n_conf - 1)
        q_env = pkg.workloads.uniform_quaternions(rng, n_env).reshape(n_env, 4)
        q_mov = pkg.workloads.uniform_quaternions(rng, n_conf * max(n_moving, 1)).reshape(n_conf, max(n_moving, 1), 4)[:, :n_moving]
        side, near = 9.0, 2.0
        allowed = n_allowed(n_moving, n_env)
        for attempt in range(60):
            sub = np.random.default_rng([seed, n_moving, n_env, n_conf, attempt])
            slab = np.arange(n_env) // TILE
            T_env = sub.uniform(0.0, side, (n_env, 3))
            T_env[:, 0] += slab * (side + self.GAP)
            T_mov = np.zeros((n_conf, n_moving, 3))
            for c, kind in enumerate(self.kinds):
                if kind == 0:  # a lattice far below everything: no pair at all
                    k = np.arange(n_moving)
                    g = int(np.ceil(max(n_moving, 1) ** (1.0 / 3.0)))
                    T_mov[c] = 6.0 * np.stack([k % g, (k // g) % g, k // (g * g)], axis=1) - np.array([0.0, 0.0, 1000.0])
                    continue
                block = np.arange(n_moving) // ROWS
                if self.n_tiles:
                    t = (block + c) % self.n_tiles
                    lo, hi = t * TILE, np.minimum((t + 1) * TILE, n_env)
                    member = lo + (sub.random(n_moving) * (hi - lo)).astype(np.int64)
                    T_mov[c] = T_env[member] + sub.uniform(-near, near, (n_moving, 3))
                else:  # no environment: the moving objects among themselves, PairScene's box
                    T_mov[c] = sub.uniform(-3.6, 3.6, (n_moving, 3))
            self.q_env, self.T_env, self.q_mov, self.T_mov = q_env, T_env, q_mov, T_mov
            self._make_tables(pkg)
            self._lists = {}
            pairs, cb = self.expected()
            if n_env and n_moving and set(((pairs[:, 1].astype(np.int64) - n_moving) // TILE)[pairs[:, 1] >= n_moving].tolist()) != set(range(self.n_tiles)):
                near *= 0.7  # (a tile of one member that no moving object's box reached)
                continue
            if allowed < SHARE_MIN_ALLOWED:
                break
            counts = np.diff(cb.astype(np.int64))
            shares = np.array([counts[c] / allowed for c, kind in enumerate(self.kinds) if kind == 1])
            if np.all((shares >= SHARE_LO) & (shares <= SHARE_HI)):
                break
            if shares.min() < SHARE_LO:
                side *= 0.85
            else:
                side *= 1.2
        else:
            raise AssertionError("no environment with every tile met and the shares in range")

    def _make_tables(self, pkg):
        g, n_conf, nm, ne = pkg.geometry, self.n_conf, self.n_moving, self.n_env
        self.moving_tf = g.make_pose(quat=self.q_mov.reshape(-1, 4), T=self.T_mov.reshape(-1, 3)).reshape(n_conf, nm, 12)
        self.env_tf = g.make_pose(quat=self.q_env, T=self.T_env).reshape(ne, 12)
        self.moving_pose = g.pose_f32_from_quat(self.q_mov.reshape(-1, 4), self.T_mov.reshape(-1, 3)).reshape(n_conf, nm, 7)
        self.env_pose = g.pose_f32_from_quat(self.q_env, self.T_env).reshape(ne, 7)
        self.tf = full_table(self.moving_tf, self.env_tf)
        self.pose = full_table(self.moving_pose, self.env_pose)
        wide = g.make_pose(quat=self.pose[..., :4].reshape(-1, 4).astype(np.float64),
                           T=self.pose[..., 4:].reshape(-1, 3).astype(np.float64)).reshape(n_conf, self.n, 12)
        self.boxes = host_boxes(pkg, self.lib, self.obj_shape, self.tf)
        self.boxes32 = host_boxes(pkg, self.lib, self.obj_shape, wide)

    def expected(self, f32=False, inflate=0.0, groups=None):
        """The model's (pairs, conf_begin): computed once, shared, not modified.  groups: None or (name, object_group, words)."""
        key = (bool(f32), float(inflate), None if groups is None else groups[0])
        if key not in self._lists:
            boxes = self.boxes32 if f32 else self.boxes
            self._lists[key] = env_pairs(boxes, self.n_moving, inflate, *(groups[1:] if groups else ()))
        return self._lists[key]

    def check(self):
        """What the scene promises, on the model's output alone."""
        pairs, cb = self.expected()
        counts = np.diff(cb.astype(np.int64))
        allowed = n_allowed(self.n_moving, self.n_env)
        conf = pairs_model.conf_of(cb)
        assert not len(pairs) or pairs[:, 0].max() < self.n_moving
        assert np.all(pairs[:, 0] < pairs[:, 1])
        for c, kind in enumerate(self.kinds):
            if kind == 0:
                assert counts[c] == 0, c
            elif allowed >= SHARE_MIN_ALLOWED:
                assert SHARE_LO * allowed <= counts[c] <= SHARE_HI * allowed, (c, counts[c], allowed)
        if self.n_env and self.n_moving:
            tile_of = (pairs[:, 1].astype(np.int64) - self.n_moving) // TILE
            met = set(tile_of[pairs[:, 1] >= self.n_moving].tolist())
            assert met == set(range(self.n_tiles)), (met, self.n_tiles)  # every environment tile has a listed pair in some configuration
            skipped, cells, _ = skipped_by_box(self.boxes, self.n_moving)
            assert skipped.max() > 0, "no cell is skipped by its box"
            if self.n_tiles > 1:  # ... in a configuration that lists something too
                assert max(skipped[c] for c, kind in enumerate(self.kinds) if kind == 1) > 0
        if self.n_env and self.n_moving >= 2 and allowed >= SHARE_MIN_ALLOWED:
            both = [c for c in range(self.n_conf)
                    if np.any(pairs[conf == c, 1] < self.n_moving) and np.any(pairs[conf == c, 1] >= self.n_moving)]
            assert both, "no configuration lists both kinds of pair"
        return counts


def full_table(moving, env):
    """The full table of a call: moving[c] followed by the environment's rows, for every configuration."""
    n_conf = moving.shape[0]
    return np.ascontiguousarray(np.concatenate([moving, np.broadcast_to(env[None], (n_conf,) + env.shape)], axis=1))


def host_boxes(pkg, lib, obj_shape, tf):
    return np.stack([pkg.engine.world_aabbs(lib, obj_shape, tf[c]) for c in range(len(tf))]).reshape(len(tf), len(obj_shape), 6) \
        if len(obj_shape) else np.zeros((len(tf), 0, 6))


SIZES = [(1, 1), (2, 0), (5, 255), (16, 256), (17, 257), (63, 600), (64, 600), (65, 600), (130, 513)]
CONFS = [1, 3, 37]


def robot_groups(n_moving, n):
    """scene_robot_env's groups for a scene of n_moving <= 63 links: link k is group k, every obstacle group n_moving; allowed are
    link-link but the chain's neighbours and link-obstacle, not obstacle-obstacle."""
    group = np.minimum(np.arange(n), n_moving).astype(np.uint8)
    m = np.ones((n_moving + 1, n_moving + 1), dtype=bool)
    k = np.arange(n_moving)
    m[k, k] = False
    m[k[:-1], k[1:]] = m[k[1:], k[:-1]] = False
    m[n_moving, n_moving] = False
    return group, groups_model.words_of(m)
