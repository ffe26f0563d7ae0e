"""TEST INFRASTRUCTURE: plain numpy model of the clearance of the moving objects among an environment kept on the device
(hfcl_scene_nearest_env*, include/hppfcl_amd_nearest_env.h) and the scenes its tests share.  select() is nearest_self_model.select with
the candidates restricted to i < n_moving, written on the (n_moving, n) part of a configuration's (i, j) matrix.  The pruning of whole
(row block, environment tile) cells is restated in numpy from the header's text -- per-box terms, per-tile terms, the block as one box,
Lt -- so that what a pass drops can be counted from the boxes alone.  NearestEnvScene adds two kinds of configuration to
env_model.EnvScene: "hover" and "graze".  The yardstick of tests/test_scene_nearest_env_cpu.py and tests/test_scene_nearest_env_gpu.py."""
import numpy as np

import env_model
import nearest_model
import nearest_self_model
import pairs_model

NO_PAIR = nearest_self_model.NO_PAIR
NONE = 0xFFFFFFFF
TILE, ROWS = env_model.TILE, env_model.ROWS
COORD_MAX = 2.0 ** 500
HOVER_SHARE = 0.25


# ---- candidates -------------------------------------------------------------------------------------------------------------------------
def candidates(n_moving, n, groups=None):
    """(n_moving, n) bool: (i, j) with i < n_moving, i < j < n, whose groups may pair."""
    return nearest_self_model.allowed(n, groups)[:n_moving]


def explicit_list(n_moving, n, groups=None):
    """P_env: every candidate in lexicographic order, uint32 (|P_env|, 2)."""
    return np.ascontiguousarray(np.argwhere(candidates(n_moving, n, groups)).astype(np.uint32).reshape(-1, 2))


def env_groups(n_moving, n, groups=None):
    """Groups for nearest_self on the FULL table that forbid exactly the environment x environment pairs on top of `groups`: object o
    of group g becomes group 2 g + (o >= n_moving); (a, x) may pair with (b, y) when a may pair with b and not both are environment."""
    if groups is None:
        group, words = np.zeros(n, dtype=np.uint8), np.array([1], dtype=np.uint64)
    else:
        group, words = np.asarray(groups[0], dtype=np.uint8), np.asarray(groups[1], dtype=np.uint64)
    assert len(words) <= 32
    is_env = (np.arange(n) >= n_moving).astype(np.uint8)
    new = np.zeros(2 * len(words), dtype=np.uint64)
    for a in range(len(words)):
        for b in range(len(words)):
            if (int(words[a]) >> b) & 1:
                new[2 * a] |= np.uint64(3 << (2 * b))      # a moving object: with both halves of group b
                new[2 * a + 1] |= np.uint64(1 << (2 * b))  # an environment object: with the moving half only
    return (2 * group + is_env).astype(np.uint8), new


# ---- the selection ----------------------------------------------------------------------------------------------------------------------
def _listed(mask):
    cij = np.argwhere(mask)
    conf_begin = np.concatenate([[0], np.cumsum(mask.reshape(len(mask), -1).sum(axis=1))]).astype(np.uint64)
    return np.ascontiguousarray(cij[:, 1:].astype(np.uint32).reshape(-1, 2)), conf_begin, cij[:, 0]


def select(abi, boxes, n_moving, groups, records, upper_bound=np.inf, r=nearest_model.R64):
    """boxes (n_conf, n, 6) of the FULL tables; records: those of distance() on explicit_list(n_moving, n, groups), n_conf * |P_env| of
    either precision.  Returns the dict of nearest_self_model.select: seed, pairs1 / conf_begin1, thr, pairs2 / conf_begin2,
    summary1 / summary2, clearance, min_records -- and L, the (n_conf, n_moving, n) bounds."""
    boxes = np.asarray(boxes, dtype=np.float64)
    n_conf, n = boxes.shape[:2]
    nm = n_moving
    D = np.float64(upper_bound)
    cand = candidates(nm, n, groups)
    P = np.argwhere(cand)
    index = np.full((max(nm, 1), max(n, 1)), -1, dtype=np.int64)
    index[P[:, 0], P[:, 1]] = np.arange(len(P))
    L = nearest_model.bound(boxes[:, :nm, None, :], boxes[:, None, :, :], r) if nm and n else np.zeros((n_conf, nm, n))
    flat = np.where(cand[None], L, np.inf).reshape(n_conf, nm * n)
    any_cand = bool(cand.any())
    first = flat.argmin(axis=1) if any_cand else np.zeros(n_conf, dtype=np.int64)  # (the first of equal values: the lowest (i, j))
    seed = ((first // max(n, 1)).astype(np.uint64) << np.uint64(32)) | (first % max(n, 1)).astype(np.uint64)
    if not any_cand:
        seed = np.full(n_conf, NO_PAIR, dtype=np.uint64)
    is_seed = np.zeros((n_conf, nm * n), dtype=bool)
    if any_cand:
        is_seed[np.arange(n_conf), first] = True
    is_seed = is_seed.reshape(n_conf, nm, n)
    pass1 = cand[None] & (np.isneginf(L) | is_seed) & (L <= D)
    out = dict(seed=seed, L=L)
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
            min_records[c] = nearest_self_model.no_record(abi, f32)
        else:
            clear["min_distance"][c] = sums[best[3]]["min_distance"][c]
            clear["min_i"][c], clear["min_j"][c] = best[1], best[2]
            min_records[c] = recs[best[3]][best[4]]
    out["clearance"], out["min_records"] = clear, min_records
    return out


# ---- pruning by distance ------------------------------------------------------------------------------------------------------------------
def box_terms(boxes):
    """(m, 6) -> (m, 2): the diagonal, and the largest |coordinate| -- -1 when a coordinate is not finite (nearest_box_terms, packed)."""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 6)
    with np.errstate(invalid="ignore", over="ignore"):
        d = b[:, 3:] - b[:, :3]
        diagonal = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        a = np.abs(b)
        largest = np.where(np.isnan(a), 0.0, a).max(axis=1) if len(b) else np.zeros(0)
    finite = np.isfinite(b).all(axis=1)
    return np.stack([diagonal, np.where(finite, largest, -1.0)], axis=1)


def _fold_max(values):
    """m = x > m ? x : m from 0, in order (a NaN is never the larger)."""
    m = 0.0
    for x in values:
        if x > m:
            m = x
    return m


def tile_terms(env_boxes):
    """(n_env, 6) -> (tiles, 2): the largest member diagonal, the largest member `largest`; -1 in the second when the tile is wild."""
    t = box_terms(env_boxes)
    out = np.zeros(((len(t) + TILE - 1) // TILE, 2))
    for k in range(len(out)):
        m = t[k * TILE:(k + 1) * TILE]
        out[k] = _fold_max(m[:, 0]), (-1.0 if (m[:, 1] < 0).any() else _fold_max(m[:, 1]))
    return out


def tile_bound(rows, tile_box, terms, r=nearest_model.R64):
    """Lt of the block of row boxes `rows` (k, 6) and a tile (its box by env_model.fold_boxes, its terms by tile_terms)."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 6)
    rt = box_terms(rows)
    if terms[1] < 0 or (rt[:, 1] < 0).any():
        return -np.inf
    diagonal, largest = _fold_max(rt[:, 0]), _fold_max(rt[:, 1])
    if not largest <= COORD_MAX or not terms[1] <= COORD_MAX:
        return -np.inf
    u = env_model.fold_boxes(rows)
    if env_model.touch(u, np.asarray(tile_box)):
        return -np.inf
    with np.errstate(over="ignore", invalid="ignore"):
        g = np.maximum(u[:3] - tile_box[3:], tile_box[:3] - u[3:])
        if not (g > 0).any():
            return -np.inf
        g = np.where(g > 0.0, g, 0.0)
        lb = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
        e = np.float64(diagonal) + np.float64(terms[0])
        M = max(largest, terms[1])
        L = lb - (nearest_model.INFLATION_SLACK * e + np.float64(r) * np.float64(M))
    return float(L) if np.isfinite(L) else -np.inf


def dropped_cells(sel, boxes, n_moving, r=nearest_model.R64):
    """Per pass the (n_conf, row blocks, environment tiles) mask of the cells dropped by Lt, and Lt itself: pass 1 drops a cell with a
    finite Lt that does not hold the seed, pass 2 one with Lt > thr[c]."""
    boxes = np.asarray(boxes, dtype=np.float64)
    n_conf, n = boxes.shape[:2]
    env = boxes[0, n_moving:]
    tb, tt = env_model.tile_boxes(env), tile_terms(env)
    n_blocks = (n_moving + ROWS - 1) // ROWS
    Lt = np.full((n_conf, n_blocks, len(tb)), -np.inf)
    drop1, drop2 = np.zeros(Lt.shape, dtype=bool), np.zeros(Lt.shape, dtype=bool)
    for c in range(n_conf):
        si, sj = int(sel["seed"][c] >> np.uint64(32)), int(sel["seed"][c] & np.uint64(0xFFFFFFFF))
        for b in range(n_blocks):
            i0, i1 = b * ROWS, min((b + 1) * ROWS, n_moving)
            for t in range(len(tb)):
                Lt[c, b, t] = tile_bound(boxes[c, i0:i1], tb[t], tt[t], r)
                j0 = n_moving + t * TILE
                here = sel["seed"][c] != NO_PAIR and i0 <= si < i1 and j0 <= sj < min(j0 + TILE, n)
                drop1[c, b, t] = Lt[c, b, t] > -np.inf and not here
                drop2[c, b, t] = Lt[c, b, t] > sel["thr"][c]
    return drop1, drop2, Lt


# ---- the scenes ---------------------------------------------------------------------------------------------------------------------------
class NearestEnvScene:
    """An env_model.EnvScene of three configurations (0: far from everything, 1 and 2: among the members of a slab, boxes and shapes
    touching) and two more kinds of configuration of the same objects:
      "hover": every moving object on a lattice wider than any box, a layer per row block, above the slab the block meets -- every moving
               box is clear of every other box, so pass 1 is exactly the seed and pass 2 does the work;
      "graze": the hover lattice lowered (without an environment: tightened) until some boxes touch but no shapes collide -- found by
               bisection with the oracle's distances of the touching pairs.
    Configurations 0 .. 2 are the EnvScene's, 3 is hover, 4 graze.  records: the oracle's distance() on P_env of the full tables.
    check() asserts what this promises on the model's output."""

    PITCH = 4.1  # no shape of this library reaches 2 from its centre: boxes on a lattice of this pitch never touch

    def __init__(self, pkg, oracle, lib, n_moving, n_env, seed=0, groups=None):
        self.es = es = env_model.EnvScene(pkg, lib, n_moving, n_env, 3, seed)
        self.pkg, self.lib, self.n_moving, self.n_env, self.n = pkg, lib, n_moving, n_env, es.n
        self.obj_shape, self.groups = es.obj_shape, groups
        self.n_conf, self.kinds = 5, ["far", "among", "among", "hover", "graze"]
        self.n_tiles = es.n_tiles
        rng = np.random.default_rng([seed, n_moving, n_env, 77])
        self.q_extra = pkg.workloads.uniform_quaternions(rng, 2 * max(n_moving, 1)).reshape(2, max(n_moving, 1), 4)[:, :n_moving]
        self._oracle = oracle
        T_hover = self._lattice(self.PITCH, 3)
        lo, hi = 0.0, self.PITCH  # (lo: shapes collide or the lattice is degenerate; hi: no boxes touch)
        T_graze = None
        for _ in range(40):
            mid = 0.5 * (lo + hi)
            T = self._lattice(mid, 4)
            state = self._state(T)
            if state == "graze":
                T_graze = T
                break
            lo, hi = (mid, hi) if state == "collide" else (lo, mid)
        self.has_graze = T_graze is not None
        if T_graze is None:  # (no pair at all to graze: a scene of one object)
            assert n_moving + n_env < 2 or n_moving == 0, "no height at which boxes touch and no shapes collide"
            T_graze = self._lattice(self.PITCH, 4)
        g = pkg.geometry
        q = np.concatenate([es.q_mov, self.q_extra])
        T = np.concatenate([es.T_mov, T_hover[None], T_graze[None]])
        self.moving_tf = g.make_pose(quat=q.reshape(-1, 4), T=T.reshape(-1, 3)).reshape(5, n_moving, 12)
        self.moving_pose = g.pose_f32_from_quat(q.reshape(-1, 4), T.reshape(-1, 3)).reshape(5, n_moving, 7)
        self.env_tf, self.env_pose = es.env_tf, es.env_pose
        self.tf = env_model.full_table(self.moving_tf, self.env_tf)
        self.pose = env_model.full_table(self.moving_pose, self.env_pose)
        self.boxes = env_model.host_boxes(pkg, lib, self.obj_shape, self.tf)
        self.P = explicit_list(n_moving, self.n, groups)
        self._records = None
        self._sel = {}

    @property
    def records(self):
        """The oracle's distance() on P_env of the full tables, all five configurations: computed once."""
        if self._records is None:
            self._records = self._distance(self.tf, np.tile(self.P, (5, 1)), np.repeat(np.arange(5), len(self.P)))
        return self._records

    def _lattice(self, h, conf):
        """Row block b in a layer of its own, 4 x 4 objects of pitch PITCH: above slab (b + conf) % tiles -- centred on it (hover) or with
        its first object above the slab's highest member (graze) -- at height h over the highest member's centre plus PITCH b (no
        environment: all blocks in one lattice of pitch h)."""
        nm, es = self.n_moving, self.es
        k = np.arange(nm)
        block, within = k // ROWS, k % ROWS
        if not self.n_env:
            g = int(np.ceil(max(nm, 1) ** (1.0 / 3.0)))
            return h * np.stack([k % g, (k // g) % g, k // (g * g)], axis=1).astype(np.float64)
        T = np.zeros((nm, 3))
        t = (block + conf) % self.n_tiles
        for b in np.unique(block):
            rows = block == b
            members = es.T_env[int(t[rows][0]) * TILE:(int(t[rows][0]) + 1) * TILE]
            if conf == 4:  # graze: the block's first object right above the slab's highest member
                corner = members[members[:, 2].argmax()]
            else:
                corner = 0.5 * (members.min(axis=0) + members.max(axis=0)) - 1.5 * self.PITCH
            T[rows, 0] = corner[0] + self.PITCH * (within[rows] % 4)
            T[rows, 1] = corner[1] + self.PITCH * (within[rows] // 4)
            T[rows, 2] = es.T_env[:, 2].max() + h + self.PITCH * b
        return T

    def _distance(self, tf, pairs, conf):
        lib, shape = self.lib, self.obj_shape
        i, j = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)
        return self._oracle.distance_batch(lib.shapes_array(), lib.vertices_array(), shape[i], shape[j], np.ascontiguousarray(tf[conf, i]),
                                           np.ascontiguousarray(tf[conf, j]), self.pkg.abi.default_distance_request(), n_threads=8)

    def _state(self, T_mov):
        """Of one configuration: "clear" (no candidate's boxes touch), "collide" (some shapes do), "graze" (boxes touch, no shapes collide)."""
        g = self.pkg.geometry
        moving = g.make_pose(quat=self.q_extra[1].reshape(-1, 4), T=T_mov).reshape(1, self.n_moving, 12)
        tf = env_model.full_table(moving, self.es.env_tf)
        boxes = env_model.host_boxes(self.pkg, self.lib, self.obj_shape, tf)
        P = explicit_list(self.n_moving, self.n, self.groups)
        touching = P[env_model.touch(boxes[0, P[:, 0]], boxes[0, P[:, 1]])] if len(P) else P
        if not len(touching):
            return "clear"
        rec = self._distance(tf, touching, np.zeros(len(touching), dtype=np.int64))
        return "collide" if (rec["distance"] <= 0).any() else "graze"

    def select(self, D=np.inf, r=nearest_model.R64):
        """The model's answer with the oracle's records: computed once, shared, not modified."""
        if (D, r) not in self._sel:
            self._sel[(D, r)] = select(self.pkg.abi, self.boxes, self.n_moving, self.groups, self.records, D, r)
        return self._sel[(D, r)]

    def check(self):
        """What the scene promises, on the model's output alone.  Returns (share of the hover configuration's candidates evaluated,
        cells dropped by Lt in pass 1, in pass 2, cells)."""
        sel = self.select()
        n_cand = len(self.P)
        clear = sel["clearance"]
        L = sel["L"]
        cand = candidates(self.n_moving, self.n, self.groups)
        share = float(clear["n_evaluated"][3]) / n_cand if n_cand else 0.0
        if n_cand:
            assert not np.isneginf(L[3][cand]).any()                      # hover: no box touches another
            assert np.diff(sel["conf_begin1"].astype(np.int64))[3] == 1    # ... so pass 1 is exactly the seed
            assert clear["min_distance"][3] > 0
            if n_cand >= env_model.SHARE_MIN_ALLOWED:
                assert share <= HOVER_SHARE, share
        if self.has_graze:
            assert np.isneginf(L[4][cand]).any() and clear["min_distance"][4] > 0  # graze: boxes touch, no shapes collide
        drop1, drop2, _ = dropped_cells(sel, self.boxes, self.n_moving)
        if self.n_env and self.n_moving:
            assert min(clear["min_distance"][1:3]) < 0                   # among: some shapes collide
            conf = pairs_model.conf_of(sel["conf_begin1"])
            p = np.concatenate([sel["pairs1"], sel["pairs2"]])
            met = set(((p[:, 1].astype(np.int64) - self.n_moving) // TILE)[p[:, 1] >= self.n_moving].tolist())
            assert met == set(range(self.n_tiles)), (met, self.n_tiles)   # every environment tile holds an evaluated pair somewhere
            assert len(conf) == len(sel["pairs1"])
            if self.n_tiles > 1:                                          # in some pass-2 sweep a cell is dropped by Lt and one is not
                assert any(drop2[c].any() and not drop2[c].all() for c in range(self.n_conf)), drop2.sum(axis=(1, 2))
            elif n_cand >= env_model.SHARE_MIN_ALLOWED:                   # one tile: a sweep's cells are its row blocks; over the call's sweeps
                assert drop2.any() and not drop2.all(), drop2.sum(axis=(1, 2))  # (a scene of one pair has its seed in its only cell)
        return share, int(drop1.sum()), int(drop2.sum()), drop1.size


SIZES = [(1, 1), (2, 0), (5, 255), (17, 257), (65, 600)]
