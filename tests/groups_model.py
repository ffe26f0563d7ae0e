"""TEST INFRASTRUCTURE: the numpy model of object groups and a group matrix on the device-made pair lists (include/hppfcl_amd_groups.h),
and the group layouts tests/test_scene_groups_cpu.py and tests/test_scene_groups_gpu.py share.  The list with groups is
pairs_model.self_pairs(...) filtered by the rule of the header -- entry (i, j) stays iff bit group[j] of collides[group[i]] is set --
with conf_begin recounted.  The scenes are pairs_model.PairScene: configuration 1 has every pair touching, so its expected count is the
number of allowed pairs, in closed form."""
import numpy as np

import cull_model  # noqa: F401  (the rule of the unfiltered list: pairs_model builds on it)
import pairs_model

TILE = 256  # hfcl_pairs.hpp: PAIRS_TILE
ROWS = 16   # hfcl_pairs.hpp: PAIRS_ROWS


def words_of(matrix):
    """(G, G) bool -> uint64[G]: bit h of word g = matrix[g, h]."""
    m = np.asarray(matrix, dtype=bool)
    assert m.ndim == 2 and m.shape[0] == m.shape[1] <= 64
    bits = np.uint64(1) << np.arange(m.shape[0], dtype=np.uint64)
    return np.array([np.bitwise_or.reduce(bits[row]) if row.any() else np.uint64(0) for row in m], dtype=np.uint64)


def matrix_of(words):
    w = np.asarray(words, dtype=np.uint64)
    return ((w[:, None] >> np.arange(len(w), dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)


def allowed(group, words, i, j):
    """bit group[j] of collides[group[i]], for arrays of i and j."""
    g = np.asarray(group, dtype=np.int64)
    w = np.asarray(words, dtype=np.uint64)
    return ((w[g[np.asarray(i, dtype=np.int64)]] >> g[np.asarray(j, dtype=np.int64)].astype(np.uint64)) & np.uint64(1)).astype(bool)


def n_allowed(group, words):
    """Allowed pairs i < j of a scene."""
    i, j = np.triu_indices(len(group), 1)
    return int(allowed(group, words, i, j).sum())


def filter_list(pairs, conf_begin, group, words):
    """The list without groups -> the list with them: the entries that stay, conf_begin recounted."""
    keep = allowed(group, words, pairs[:, 0], pairs[:, 1]) if len(pairs) else np.zeros(0, dtype=bool)
    conf = pairs_model.conf_of(conf_begin)
    n_conf = len(conf_begin) - 1
    counts = np.bincount(conf[keep], minlength=n_conf).astype(np.uint64)
    cb = np.concatenate([[np.uint64(0)], np.cumsum(counts, dtype=np.uint64)]).astype(np.uint64)
    return np.ascontiguousarray(pairs[keep].reshape(-1, 2)), cb


def self_pairs(aabbs, inflate, group, words):
    pairs, cb = pairs_model.self_pairs(aabbs, inflate)
    return filter_list(pairs, cb, group, words)


# ---- what the sweep skips, counted from the tables ----------------------------------------------------------------------------------
def tile_words(group):
    """Per column tile of TILE objects: the OR of 1 << group[j] over its objects."""
    g = np.asarray(group, dtype=np.uint64)
    return np.array([np.bitwise_or.reduce(np.uint64(1) << g[t:t + TILE]) for t in range(0, len(g), TILE)], dtype=np.uint64)


def skipped(group, words):
    """(column tiles skipped, tiles looked at or skipped, row blocks that leave at once, row blocks) of one configuration's tiled sweep."""
    g = np.asarray(group, dtype=np.int64)
    w = np.asarray(words, dtype=np.uint64)
    tw = tile_words(group)
    n = len(g)
    tiles = skips = early = blocks = 0
    for i0 in range(0, n, ROWS):
        blocks += 1
        u = np.bitwise_or.reduce(w[g[i0:i0 + ROWS]])
        first = (i0 + 1) // TILE
        mine = tw[first:]
        tiles += len(mine)
        if u == 0:
            early += 1
            skips += len(mine)
        else:
            skips += int(((mine & u) == 0).sum())
    return skips, tiles, early, blocks


# ---- the layouts ------------------------------------------------------------------------------------------------------------------
def between(n_a, n):
    """Two managers: objects [0, n_a) against [n_a, n)."""
    group = np.zeros(n, dtype=np.uint8)
    group[n_a:] = 1
    return group, np.array([2, 1], dtype=np.uint64)


def chain(n):
    """One group per object (n <= 64), every pair allowed but an object and itself and the chain's neighbours (i, i + 1)."""
    m = np.ones((n, n), dtype=bool)
    k = np.arange(n)
    m[k, k] = False
    m[k[:-1], k[1:]] = m[k[1:], k[:-1]] = False
    return np.arange(n, dtype=np.uint8), words_of(m)


def random_matrix(n, n_groups, seed):
    """(c): a random symmetric matrix of density 0.5 and a random assignment.  With a handful of objects a draw can allow nearly all or
    nearly none of the pairs; such a draw is made again (as PairScene draws a placement again) until between 20 % and 80 % are allowed."""
    rng = np.random.default_rng([seed, n, n_groups])
    for _ in range(200):
        upper = rng.random((n_groups, n_groups)) < 0.5
        m = np.triu(upper) | np.triu(upper).T
        group, words = rng.integers(0, n_groups, n).astype(np.uint8), words_of(m)
        if 0.2 <= n_allowed(group, words) / (n * (n - 1) // 2) <= 0.8:
            return group, words
    raise AssertionError("no draw with a share of allowed pairs in range")


def sorted_600():
    """(f): objects 0..255 and 512..599 group 0, 256..511 group 1, only 0-0 allowed: the middle tile is skipped by every row block of
    group 0, every row block of group 1 leaves early."""
    group = np.zeros(600, dtype=np.uint8)
    group[256:512] = 1
    return group, np.array([1, 0], dtype=np.uint64)


def shuffled_600(seed=4):
    """(g): the matrix of (f), the assignment shuffled: every tile holds both groups, none can be skipped."""
    group, words = sorted_600()
    return np.random.default_rng(seed).permutation(group), words


def layouts(n, seed=0):
    """[(name, object_group uint8[n], collides uint64[G])] of the layouts a scene of n objects has."""
    rng = np.random.default_rng([seed, n])
    out = []
    for n_a in sorted({1, 16, 17, n - 1}):
        if 1 <= n_a < n:
            out.append(("a:%d" % n_a,) + between(n_a, n))
    if n <= 64:
        out.append(("b",) + chain(n))
    for n_groups in (8, 64):
        out.append(("c:%d" % n_groups,) + random_matrix(n, n_groups, seed))
    out.append(("d", rng.integers(0, 8, n).astype(np.uint8), np.full(8, 0xFF, dtype=np.uint64)))
    out.append(("e", rng.integers(0, 8, n).astype(np.uint8), np.zeros(8, dtype=np.uint64)))
    if n == 600:
        out.append(("f",) + sorted_600())
        out.append(("g",) + shuffled_600())
    return out


def check_layout(name, group, words):
    """What a layout promises, on the model alone: symmetric, inside its groups, and for (c) a share of allowed pairs that is neither
    nothing nor everything."""
    m = matrix_of(words)
    assert np.array_equal(m, m.T) and group.max() < len(words), name
    if name.startswith("c"):
        n = len(group)
        share = n_allowed(group, words) / (n * (n - 1) // 2)
        assert 0.2 <= share <= 0.8, (name, n, share)
