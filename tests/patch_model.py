"""Plain fp64 restatement of hpp::fcl::computeContactPatch (TEST INFRASTRUCTURE, the checker of the contact-patch kernels).

Restated from the reference's semantics, pair by pair:
  entry point        src/contact_patch.cpp:48-97; GEOM x BVH: ContactPatchResult::swapObjects (collision_data.h:968-980)
  frame              constructContactPatchFrameFromContact (collision_data.h:706-713), constructOrthonormalBasisFromVector
                     (math/transform.h:261-267) with Eigen's unitOrthogonal (OrthoMethods.h) and normalized()
  solver             contact_patch/contact_patch_solver.hxx:76-427, internal/shape_shape_contact_patch_func.h:85-250
  support sets       src/narrowphase/support_functions.cpp:529-945, hull 993-1113 with libstdc++'s std::stable_sort

Python floats are IEEE doubles and every expression below is evaluated in the order written, left to right, one rounding per
operation -- the order the device header (hpp-fcl_amd/csrc/hfcl_patch.hpp) uses, built without contraction.  Cone and cylinder
samples use math.cos / math.sin, which may differ from the device's by an ulp: compare points with a tolerance.
"""
import math

import numpy as np

BOX, SPHERE, CAPSULE, CONE, CYLINDER, CONVEX, PLANE, HALFSPACE, TRIANGLE, ELLIPSOID, BVH = 9, 10, 11, 12, 13, 14, 15, 16, 17, 19, 5
NONE, POINT, ONESIDED, CLIPPED = 0, 1, 2, 3
SWAPPED, OVERFLOW, SKIPPED = 1 << 2, 1 << 3, 1 << 31
DUMMY = 1e-12
EPS = 2.220446049250313e-16
TINY = 1e-12


def set_bound(kind, num_points, ns):
    if kind == BOX:
        return 4
    if kind == TRIANGLE:
        return 3
    if kind == CAPSULE:
        return 2
    if kind in (CONE, CYLINDER):
        return max(ns, 2)
    if kind == CONVEX:
        return int(num_points)
    return 1


def table_bound(shapes, ns):
    m = 1
    for s in shapes:
        m = max(m, set_bound(int(s["type"]), int(s["num_points"]), ns))
    return 2 * m


def request_values(ns, tol):
    return (3 if ns < 3 else ns), (1e-12 if tol < 0 else tol)


def classify(k1, k2, rec, max_num_patch):
    """(class, swapped) of a record (hfcl_patch.hpp: patch_class)."""
    if max_num_patch == 0 or int(rec["num_contacts"]) <= 0 or (int(rec["status"]) >> 31) & 1:
        return NONE, False
    if k1 == BVH or k2 == BVH:
        return POINT, k1 != BVH
    f1, f2 = k1 in (PLANE, HALFSPACE), k2 in (PLANE, HALFSPACE)
    if f1 and f2:
        return POINT, False
    if k1 in (SPHERE, ELLIPSOID) or k2 in (SPHERE, ELLIPSOID):
        return POINT, False
    if f1 or f2:
        return ONESIDED, False
    return CLIPPED, False


# ---- 3-vectors as tuples -------------------------------------------------------------------------------------------------
def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def scale(s, a):
    return (s * a[0], s * a[1], s * a[2])


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def normalized(a):
    z = dot(a, a)
    d = math.sqrt(z) if z > 0 else 1.0
    return (a[0] / d, a[1] / d, a[2] / d)


def unit_orthogonal(v):
    x, y, z = v
    if not (abs(x) <= abs(z) * DUMMY) or not (abs(y) <= abs(z) * DUMMY):
        inv = 1.0 / math.sqrt(x * x + y * y)
        return (-y * inv, x * inv, 0.0)
    inv = 1.0 / math.sqrt(y * y + z * z)
    return (0.0, -z * inv, y * inv)


class Frame:
    """Rotation as three columns c[0..2] and a translation t (R(r, c) = c[c][r])."""

    def __init__(self, cols, t):
        self.c = cols
        self.t = t

    def row(self, r):
        return (self.c[0][r], self.c[1][r], self.c[2][r])


def pose_frame(tf12):
    tf = [float(x) for x in tf12]
    return Frame([(tf[0], tf[1], tf[2]), (tf[3], tf[4], tf[5]), (tf[6], tf[7], tf[8])], (tf[9], tf[10], tf[11]))


def patch_frame(rec):
    n = tuple(float(x) for x in rec["normal"])
    c2 = normalized(n)
    u = unit_orthogonal(n)
    c1 = (-u[0], -u[1], -u[2])
    c0 = cross(c1, n)
    p1, p2 = rec["p1"], rec["p2"]
    t = tuple((float(p1[k]) + float(p2[k])) / 2.0 for k in range(3))
    return Frame([c0, c1, c2], t)


def inv_xy(f, p):
    d = sub(p, f.t)
    return (f.c[0][0] * d[0] + f.c[0][1] * d[1] + f.c[0][2] * d[2], f.c[1][0] * d[0] + f.c[1][1] * d[1] + f.c[1][2] * d[2])


def set_frame(fs, fc):
    """R = Rs^T Rc, t = Rs^T (tc - ts): column j of R is Rs^T c_j."""
    def tmulv(v):
        return (fs.c[0][0] * v[0] + fs.c[0][1] * v[1] + fs.c[0][2] * v[2],
                fs.c[1][0] * v[0] + fs.c[1][1] * v[1] + fs.c[1][2] * v[2],
                fs.c[2][0] * v[0] + fs.c[2][1] * v[1] + fs.c[2][2] * v[2])
    return Frame([tmulv(fc.c[0]), tmulv(fc.c[1]), tmulv(fc.c[2])], tmulv(sub(fc.t, fs.t)))


def frame_tf12(f, swapped=False):
    s = -1.0 if swapped else 1.0
    c0, c1, c2 = f.c
    return [c0[0] * s, c0[1] * s, c0[2] * s, c1[0], c1[1], c1[2], c2[0] * s, c2[1] * s, c2[2] * s, f.t[0], f.t[1], f.t[2]]


# ---- supports (getShapeSupport<NoSweptSphere>, hfcl_shapes.hpp: prim_support) -----------------------------------------
def prim_support(kind, p, d):
    if kind == BOX:
        inf = 1.0 + 1e-10
        return tuple(((p[i] if d[i] > TINY else 0.0) + ((-inf * p[i]) if d[i] < -TINY else 0.0)) for i in range(3))
    if kind == CAPSULE:
        z = p[1] if d[2] > TINY else (-p[1] if d[2] < -TINY else 0.0)
        return (0.0, 0.0, z)
    if kind == CONE:
        inflate = 1.0 + 1e-10
        h, r = p[1], p[0]
        if abs(d[0]) <= TINY and abs(d[1]) <= TINY:
            return (0.0, 0.0, h if d[2] > TINY else -inflate * h)
        zd = d[0] * d[0] + d[1] * d[1]
        ln = math.sqrt(zd + d[2] * d[2])
        zd = math.sqrt(zd)
        sin_a = r / math.sqrt(r * r + 4.0 * h * h)
        if d[2] > 0 and d[2] > ln * sin_a:
            return (0.0, 0.0, h)
        rad = r / zd
        return (rad * d[0], rad * d[1], -h)
    if kind == CYLINDER:
        inflate = 1.0 + 1e-10
        half_h, r = p[1], p[0]
        aligned = abs(d[0]) <= TINY and abs(d[1]) <= TINY
        if aligned:
            half_h *= inflate
        if d[2] > TINY:
            z = half_h
        elif d[2] < -TINY:
            z = -half_h
        else:
            z = 0.0
            r *= inflate
        if aligned:
            return (0.0, 0.0, z)
        n2 = d[0] * d[0] + d[1] * d[1]
        nx, ny = d[0], d[1]
        if n2 > 0:
            n = math.sqrt(n2)
            nx, ny = d[0] / n, d[1] / n
        return (nx * r, ny * r, z)
    return (0.0, 0.0, 0.0)


# ---- hull of a cloud with libstdc++'s stable_sort -------------------------------------------------------------------------
def hull_less(p1, p2, v):
    det = (p1[0] - v[0]) * (p2[1] - v[1]) - (p1[1] - v[1]) * (p2[0] - v[0])
    if abs(det) <= DUMMY:
        a = (p1[0] - v[0]) * (p1[0] - v[0]) + (p1[1] - v[1]) * (p1[1] - v[1])
        b = (p2[0] - v[0]) * (p2[0] - v[0]) + (p2[1] - v[1]) * (p2[1] - v[1])
        return a <= b
    return det > 0


def _insertion(a, lo, hi, v):
    for i in range(lo + 1, hi):
        val = a[i]
        if hull_less(val, a[lo], v):
            a[lo + 1:i + 1] = a[lo:i]
            a[lo] = val
        else:
            last = i
            while hull_less(val, a[last - 1], v):
                a[last] = a[last - 1]
                last -= 1
            a[last] = val


def _move_merge(s, f1, l1, f2, l2, out):
    while f1 != l1 and f2 != l2:
        if hull_less(s[f2], s[f1], _V[0]):
            out.append(s[f2])
            f2 += 1
        else:
            out.append(s[f1])
            f1 += 1
    out.extend(s[f1:l1])
    out.extend(s[f2:l2])


_V = [None]


def _merge_loop(src, step):
    n, two, f, out = len(src), 2 * step, 0, []
    while n - f >= two:
        _move_merge(src, f, f + step, f + step, f + two, out)
        f += two
    st = min(n - f, step)
    _move_merge(src, f, f + st, f + st, n, out)
    return out


def _merge_sort_with_buffer(a, v):
    n, step, f = len(a), 7, 0
    while n - f >= step:
        _insertion(a, f, f + step, v)
        f += step
    _insertion(a, f, n, v)
    while step < n:
        a = _merge_loop(a, step)
        step *= 2
        a = _merge_loop(a, step)
        step *= 2
    return a


def stable_sort(a, v):
    """libstdc++ std::stable_sort (buffered: __stable_sort_adaptive) with hull_less -- ties in its order."""
    _V[0] = v
    n = len(a)
    if n == 0:
        return a
    len1 = (n + 1) // 2
    x = _merge_sort_with_buffer(list(a[:len1]), v)
    y = _merge_sort_with_buffer(list(a[len1:]), v)
    if len1 <= len(y):  # forward merge, ties to the first half
        out, i, j = [], 0, 0
        while i < len(x) and j < len(y):
            if hull_less(y[j], x[i], v):
                out.append(y[j])
                j += 1
            else:
                out.append(x[i])
                i += 1
        return out + x[i:] + y[j:]
    if not y:
        return x
    res = [None] * n
    l1, l2, r = len(x) - 1, len(y) - 1, n
    while True:
        if hull_less(y[l2], x[l1], v):
            r -= 1
            res[r] = x[l1]
            if l1 == 0:
                for k in range(l2, -1, -1):
                    r -= 1
                    res[r] = y[k]
                return res
            l1 -= 1
        else:
            r -= 1
            res[r] = y[l2]
            if l2 == 0:
                res[:r] = x[:l1 + 1]
                return res
            l2 -= 1


def cloud_hull(cloud):
    cloud = list(cloud)
    n = len(cloud)
    if n <= 2:
        return cloud
    if n == 3:
        if cloud[0][1] > cloud[1][1]:
            cloud[0], cloud[1] = cloud[1], cloud[0]
        if cloud[0][1] > cloud[2][1]:
            cloud[0], cloud[2] = cloud[2], cloud[0]
        a, b, c = cloud
        det = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
        if det < 0:
            cloud[1], cloud[2] = cloud[2], cloud[1]
        return cloud
    si, sv = 0, cloud[0][1]
    for i in range(1, n):
        if cloud[i][1] < sv:
            sv, si = cloud[i][1], i
    cloud[0], cloud[si] = cloud[si], cloud[0]
    v = cloud[0]
    hull = [v]
    cloud = [v] + stable_sort(cloud[1:], v)
    i = 1
    while len(hull) < 3 and i < n:
        q = cloud[i]
        dx, dy = hull[-1][0] - q[0], hull[-1][1] - q[1]
        if dx * dx + dy * dy > EPS:
            hull.append(q)
        i += 1
    for i in range(i, n):
        q = cloud[i]
        while len(hull) > 1:
            a, b = hull[-2], hull[-1]
            det = (b[0] - a[0]) * (q[1] - a[1]) - (b[1] - a[1]) * (q[0] - a[0])
            if det > DUMMY:
                break
            hull.pop()
        hull.append(q)
    return hull


# ---- support sets ---------------------------------------------------------------------------------------------------------
def support_set(shape, verts, graph, tf, inverted, hint, ns, tol):
    kind = int(shape["type"])
    p = [float(x) for x in shape["params"]]
    ssr_r = float(shape["swept_sphere_radius"])
    c2 = tf.c[2]
    d = (-c2[0], -c2[1], -c2[2]) if inverted else c2
    ssr = scale(ssr_r, d)
    out = []
    if kind == TRIANGLE:
        o = int(shape["vertex_offset"])
        a, b, c = (tuple(float(x) for x in verts[o + k]) for k in range(3))
        da, db, dc = dot(d, a), dot(d, b), dot(d, c)
        sup = ((c if dc > da else a) if da > db else (c if dc > db else b))
        sv = dot(sup, d)
        for q in (a, b, c):
            if sv - dot(d, q) < tol:
                out.append(inv_xy(tf, add(q, ssr)))
        return out
    if kind == BOX:
        sup = prim_support(BOX, p, d)
        sv = dot(sup, d)
        x, y, z = p[0], p[1], p[2]
        corners = [(x, y, z), (-x, y, z), (-x, -y, z), (x, -y, z), (x, y, -z), (-x, y, -z), (-x, -y, -z), (x, -y, -z)]
        cloud = [inv_xy(tf, add(cr, ssr)) for cr in corners if sv - dot(cr, d) < tol]
        return cloud_hull(cloud)
    if kind == CAPSULE:
        sup = prim_support(CAPSULE, p, d)
        r, h = p[0], p[1]
        sv = dot(d, add(sup, scale(r, d)))
        q1, q2 = (r * d[0], r * d[1], h), (r * d[0], r * d[1], -h)
        if sv - dot(d, q1) <= tol and sv - dot(d, q2) <= tol:
            return [inv_xy(tf, add(q1, ssr)), inv_xy(tf, add(q2, ssr))]
        return [inv_xy(tf, add(sup, ssr))]
    if kind in (CONE, CYLINDER):
        sup = prim_support(kind, p, d)
        sv = dot(sup, d)
        r, h = p[0], p[1]
        z = -h if kind == CONE else (-h if d[2] <= 0 else h)
        q1, q2 = (r * d[0], r * d[1], z), (-r * d[0], -r * d[1], z)
        if sv - dot(d, q1) <= tol and sv - dot(d, q2) <= tol:
            inc = 2.0 * 3.141592653589793 / float(ns)
            for i in range(ns):
                th = float(i) * inc
                out.append(inv_xy(tf, add((r * math.cos(th), r * math.sin(th), z), ssr)))
        elif kind == CONE:
            tip = (0.0, 0.0, h)
            if sv - dot(d, tip) <= tol:
                out.append(inv_xy(tf, add(tip, ssr)))
            base = (r * d[0], r * d[1], z)
            if sv - dot(d, base) <= tol:
                out.append(inv_xy(tf, add(base, ssr)))
        else:
            for q in ((r * d[0], r * d[1], -h), (r * d[0], r * d[1], h)):
                if sv - dot(d, q) <= tol:
                    out.append(inv_xy(tf, add(q, ssr)))
        return out
    if kind == CONVEX:
        o, np_ = int(shape["vertex_offset"]), int(shape["num_points"])
        V = [tuple(float(x) for x in verts[o + k]) for k in range(np_)]
        cloud = []
        if np_ > 32 and graph is not None:
            off, ids = graph
            cur = 0 if (hint < 0 or hint >= np_) else hint
            visited = [False] * np_
            best = V[cur][0] * d[0] + V[cur][1] * d[1] + V[cur][2] * d[2]
            visited[cur] = True
            found, loose = True, True
            while found:
                found = False
                for k in range(int(off[cur]), int(off[cur + 1])):
                    ip = int(ids[k])
                    if visited[ip]:
                        continue
                    visited[ip] = True
                    dd = V[ip][0] * d[0] + V[ip][1] * d[1] + V[ip][2] * d[2]
                    better = False
                    if dd > best:
                        better, loose = True, False
                    elif loose and dd == best:
                        better = True
                    if better:
                        best, cur, found = dd, ip, True
            sup = V[cur]
            sv = dot(sup, d)
            visited = [False] * np_
            visited[cur] = True
            stack = []
            if sv - dot(sup, d) <= tol:
                cloud.append(inv_xy(tf, add(sup, ssr)))
                stack.append([cur, int(off[cur])])
            while stack:
                top = stack[-1]
                if top[1] >= int(off[top[0] + 1]):
                    stack.pop()
                    continue
                u = int(ids[top[1]])
                top[1] += 1
                if visited[u]:
                    continue
                visited[u] = True
                if sv - dot(V[u], d) <= tol:
                    cloud.append(inv_xy(tf, add(V[u], ssr)))
                    stack.append([u, int(off[u])])
        else:
            best, bd = 0, V[0][0] * d[0] + V[0][1] * d[1] + V[0][2] * d[2]
            for i in range(1, np_):
                dd = V[i][0] * d[0] + V[i][1] * d[1] + V[i][2] * d[2]
                if dd > bd:
                    bd, best = dd, i
            sv = dot(d, V[best])
            cloud = [inv_xy(tf, add(q, ssr)) for q in V if sv - dot(d, q) <= tol]
        return cloud_hull(cloud)
    return out


def line_segment_intersection(a, b, c, d):
    abx, aby = b[0] - a[0], b[1] - a[1]
    nx, ny = -aby, abx
    den = nx * (c[0] - d[0]) + ny * (c[1] - d[1])
    if abs(den) < EPS:
        return d
    al = (nx * (a[0] - d[0]) + ny * (a[1] - d[1])) / den
    al = min(1.0, max(0.0, al))
    return (al * c[0] + (1 - al) * d[0], al * c[1] + (1 - al) * d[1])


SEGMENT_DET_QUIRK = True     # the reference's boolean `det` in the segment x segment branch
LAST_BRANCH = [None]         # the branch the last compute() of a clipped record took (for tests that pin a branch)


def compute(s1, tf1, g1, s2, tf2, g2, verts, fr, guess, ns, tol):
    """Points of a PATCH_ONESIDED / PATCH_CLIPPED record (hfcl_patch.hpp: patch_compute)."""
    LAST_BRANCH[0] = None
    origin = inv_xy(fr, fr.t)
    k1, k2 = int(s1["type"]), int(s2["type"])
    f1 = k1 in (PLANE, HALFSPACE)
    if f1 or k2 in (PLANE, HALFSPACE):
        o, to, g, h = (s2, tf2, g2, guess[1]) if f1 else (s1, tf1, g1, guess[0])
        pts = support_set(o, verts, g, set_frame(to, fr), f1, h, ns, tol)
        return [origin] if len(pts) <= 1 else pts
    P1 = support_set(s1, verts, g1, set_frame(tf1, fr), False, guess[0], ns, tol)
    P2 = support_set(s2, verts, g2, set_frame(tf2, fr), True, guess[1], ns, tol)
    if len(P1) <= 1 or len(P2) <= 1:
        LAST_BRANCH[0] = "single_point_set"
        return [origin]
    eps = DUMMY
    if len(P1) == 2 and len(P2) == 2:
        a, b = P1
        c, dd = P2
        if SEGMENT_DET_QUIRK:  # the reference's `det` is the boolean of this comparison (contact_patch_solver.hxx:149-150)
            det = 1.0 if (b[0] - a[0]) * (dd[1] - c[1]) >= (b[1] - a[1]) * (dd[0] - c[0]) else 0.0
        else:  # (what a real determinant would give: only for showing that a test tells the two apart)
            det = (b[0] - a[0]) * (dd[1] - c[1]) - (b[1] - a[1]) * (dd[0] - c[0])
        cdx, cdy, bax, bay = c[0] - dd[0], c[1] - dd[1], b[0] - a[0], b[1] - a[1]
        if abs(det) > eps or (cdx * cdx + cdy * cdy) < eps or (bax * bax + bay * bay) < eps:
            LAST_BRANCH[0] = "segment_segment_point"
            return [origin]
        LAST_BRANCH[0] = "segment_segment_projection"
        ux, uy = dd[0] - c[0], dd[1] - c[1]
        ln = ux * ux + uy * uy
        out = []
        for q in (a, b):
            t = (q[0] - c[0]) * ux + (q[1] - c[1]) * uy
            t = 1.0 if t >= ln else (0.0 if t <= 0 else t / ln)
            out.append((c[0] + t * ux, c[1] + t * uy))
        ex, ey = out[0][0] - out[1][0], out[0][1] - out[1][1]
        return out if ex * ex + ey * ey >= eps else out[:1]
    LAST_BRANCH[0] = "clipping"
    cur, clipper = (P1, P2) if len(P1) < len(P2) else (P2, P1)
    nclip = len(clipper)
    for i in range(nclip):
        prev, cur = cur, []
        a, b = clipper[i], clipper[(i + 1) % nclip]
        abx, aby = b[0] - a[0], b[1] - a[1]
        if len(prev) == 2:
            p1, p2 = prev
            det1 = abx * (p1[1] - a[1]) - aby * (p1[0] - a[0])
            det2 = abx * (p2[1] - a[1]) - aby * (p2[0] - a[0])
            if det1 < 0 and det2 < 0:
                break
            if det1 >= 0 and det2 >= 0:
                cur = [p1, p2]
                continue
            if det1 >= 0:
                if det1 > eps:
                    cur = [p1, line_segment_intersection(a, b, p1, p2)]
                    continue
                cur = [p1]
                break
            if det2 > eps:
                cur = [p2, line_segment_intersection(a, b, p1, p2)]
                continue
            cur = [p2]
            break
        n = len(prev)
        added = [False] * n
        for j in range(n):
            p1, p2 = prev[j], prev[(j + 1) % n]
            det1 = abx * (p1[1] - a[1]) - aby * (p1[0] - a[0])
            det2 = abx * (p2[1] - a[1]) - aby * (p2[0] - a[0])
            if det1 < 0 and det2 < 0:
                continue
            if det1 >= 0 and det2 >= 0:
                if not added[j]:
                    cur.append(p1)
                    added[j] = True
                continue
            if det1 >= 0:
                if not added[j]:
                    cur.append(p1)
                    added[j] = True
                if det1 > eps:
                    cur.append(line_segment_intersection(a, b, p1, p2))
            else:
                if det2 > eps:
                    cur.append(line_segment_intersection(a, b, p1, p2))
                elif not added[(j + 1) % n]:
                    cur.append(p2)
                    added[(j + 1) % n] = True
        if len(cur) <= 1:
            break
    return [origin] if len(cur) <= 1 else cur


def patches(shapes, verts, s1, s2, tf1, tf2, records, guesses=None, max_num_patch=1, ns=12, tol=1e-3, graphs=None):
    """Model of hfcl_contact_patch_batch.  Returns a list of (class, swapped, tf12, depth, points[list of (x, y)])."""
    ns, tol = request_values(ns, tol)
    graphs = graphs or {}
    out = []
    for i in range(len(s1)):
        a, b = int(s1[i]), int(s2[i])
        sh1, sh2 = shapes[a], shapes[b]
        rec = records[i]
        cls, sw = classify(int(sh1["type"]), int(sh2["type"]), rec, max_num_patch)
        if cls == NONE:
            out.append((NONE, False, [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0], 0.0, []))
            continue
        fr = patch_frame(rec)
        depth = float(rec["distance"])
        if cls == POINT:
            o = inv_xy(fr, fr.t)
            out.append((POINT, sw, frame_tf12(fr, sw), depth, [(-o[0] if sw else o[0], o[1])]))
            continue
        guess = (0, 0) if guesses is None else (int(guesses[i]["support_guess"][0]), int(guesses[i]["support_guess"][1]))
        pts = compute(sh1, pose_frame(tf1[i]), graphs.get(a), sh2, pose_frame(tf2[i]), graphs.get(b), verts, fr, guess, ns, tol)
        out.append((cls, False, frame_tf12(fr), depth, pts))
    return out


def patch_point_world(tf12, xy):
    """ContactPatch::getPoint: the 2-D point in the patch frame, in the world."""
    R = np.asarray(tf12[:9], dtype=np.float64).reshape(3, 3).T
    return R @ np.array([xy[0], xy[1], 0.0]) + np.asarray(tf12[9:12], dtype=np.float64)


def _is_approx(a, b, tol):
    """Eigen's isApprox: |a - b| <= tol * min(|a|, |b|)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) <= tol * min(np.linalg.norm(a), np.linalg.norm(b))


def is_same(tf_a, depth_a, pts_a, tf_b, depth_b, pts_b, tol=1e-6):
    """ContactPatch::isSame (collision_data.h:660-704): same normal, depth and size; every point of `a` found in `b`."""
    if not _is_approx(np.asarray(tf_a[6:9]), np.asarray(tf_b[6:9]), tol):
        return False
    if abs(depth_a - depth_b) > tol or len(pts_a) != len(pts_b):
        return False
    wb = [patch_point_world(tf_b, q) for q in pts_b]
    return all(any(_is_approx(patch_point_world(tf_a, p), w, tol) for w in wb) for p in pts_a)


def expected_patch(rec, world_points):
    """The patch the reference's tests build by hand: the frame of the contact, the given world points added."""
    fr = patch_frame(rec)
    return frame_tf12(fr), float(rec["distance"]), [inv_xy(fr, tuple(map(float, w))) for w in world_points]


# The reference's own cases (test/contact_patch.cpp), restated: name -> (ShapeLibrary, index of o1, index of o2, tf1, tf2,
# expected world points of the patch as a function of the collide() record, or None: no collision).  Poses are 12-double
# Transform3f images.  As in the reference, a case passes when `expected.isSame(patch, 1e-6)` (expected points are projected
# onto the patch plane by addPoint, so a point given on either shape's surface is fine).
REFERENCE_CASE_NAMES = [
    "box_box_no_collision", "box_sphere", "box_box", "halfspace_box",
    "halfspace_capsule/1", "halfspace_capsule/2", "halfspace_capsule/3",
    "halfspace_cone/1", "halfspace_cone/2", "halfspace_cone/3",
    "halfspace_cylinder/1", "halfspace_cylinder/2", "halfspace_cylinder/3",
    "convex_convex",
    "edge_case_segment_segment/1", "edge_case_segment_segment/2", "edge_case_segment_segment/3",
    "edge_case_vertex_vertex/1", "edge_case_vertex_vertex/2", "edge_case_vertex_vertex/3",
    "edge_case_segment_face",
]


def reference_cases(geometry):
    I = geometry.make_pose()
    Ry180 = np.array([[-1.0, 0, 0], [0, 1.0, 0], [0, 0, -1.0]])  # columns (-1,0,0) (0,1,0) (0,0,-1)
    Ry90 = np.array([[0, 0, -1.0], [0, 1.0, 0], [1.0, 0, 0]])    # columns (0,0,1) (0,1,0) (-1,0,0)

    def pose(R=None, T=(0, 0, 0)):
        return geometry.make_pose(R=np.eye(3) if R is None else R, T=np.asarray(T, dtype=np.float64))

    def xf(tf, p):
        return np.asarray(tf[:9]).reshape(3, 3).T @ np.asarray(p, dtype=np.float64) + np.asarray(tf[9:12])

    def shifted(pts, rec, sign):
        n, d = np.asarray(rec["normal"], dtype=np.float64), float(rec["distance"])
        return [np.asarray(p, dtype=np.float64) + sign * (d * n) / 2 for p in pts]

    cases = {}
    h, off = 0.5, 0.001
    lib = geometry.ShapeLibrary()
    lib.add_box(2 * h, 2 * h, 2 * h)
    lib.add_box(2 * h, 2 * h, 2 * h)
    cases["box_box_no_collision"] = (lib, 0, 1, I, pose(T=(0, 0, 2 * h + off)), None)
    corners = [(h, h, h), (h, -h, h), (-h, -h, h), (-h, h, h)]
    cases["box_box"] = (lib, 0, 1, I, pose(T=(0, 0, 2 * h - off)), lambda r: shifted(corners, r, +1))
    lib = geometry.ShapeLibrary()
    lib.add_box(2 * h, 2 * h, 2 * h)
    lib.add_sphere(0.5)
    cases["box_sphere"] = (lib, 0, 1, I, pose(T=(0, 0, 2 * h - off)),
                           lambda r: [(np.asarray(r["p1"]) + np.asarray(r["p2"])) / 2])
    lib = geometry.ShapeLibrary()
    lib.add_halfspace((0, 0, 1.0), 0.0)
    lib.add_box(2 * h, 2 * h, 2 * h)
    T2 = np.array([0, 0, h - off])
    bottom = [np.array(c) + T2 for c in [(h, h, -h), (h, -h, -h), (-h, -h, -h), (-h, h, -h)]]
    cases["halfspace_box"] = (lib, 0, 1, I, pose(T=T2), lambda r: shifted(bottom, r, -1))

    # halfspace x capsule / cone / cylinder: radius 0.25, height 1 (halfLength 0.5)
    r_, hl = 0.25, 0.5
    for kind in ("capsule", "cone", "cylinder"):
        lib = geometry.ShapeLibrary()
        lib.add_halfspace((0, 0, 1.0), 0.0)
        getattr(lib, "add_" + kind)(r_, 2 * hl)
        t1 = pose(T=(0, 0, hl - off))
        t2 = pose(Ry180, (0, 0, hl - off))
        t3 = pose(Ry90, (0, 0, r_ - off))
        if kind == "capsule":
            e1 = [xf(t1, (0, 0, -hl))]
            e2 = [xf(t2, (0, 0, hl))]
            e3 = [xf(t3, (-r_, 0, hl)), xf(t3, (-r_, 0, -hl))]
        else:
            # the reference builds its 12 expected points with an increment of 2 pi / 6 (each base point twice): expected.isSame
            # then asks that each of them be one of the patch's 12 points
            inc = 2.0 * math.pi / 6.0
            base = [xf(t1, (math.cos(i * inc) * r_, math.sin(i * inc) * r_, -hl)) for i in range(12)]
            e1 = base
            if kind == "cone":
                e2 = [xf(t2, (0, 0, hl))]
                e3 = [xf(t3, (-r_, 0, -hl))]
            else:
                e2 = base
                e3 = [xf(t3, (r_, 0, hl)), xf(t3, (r_, 0, -hl))]
        for k, (t, e) in enumerate(((t1, e1), (t2, e2), (t3, e3))):
            cases["halfspace_%s/%d" % (kind, k + 1)] = (lib, 0, 1, I, t, (lambda e: lambda r: e)(e))

    # convex x convex: buildBox (test/utility.cpp:460-480), the box_box placement
    bx = [(h, h, h), (h, h, -h), (h, -h, h), (h, -h, -h), (-h, h, h), (-h, h, -h), (-h, -h, h), (-h, -h, -h)]
    lib = geometry.ShapeLibrary()
    lib.add_convex(bx)
    lib.add_convex(bx)
    cases["convex_convex"] = (lib, 0, 1, I, pose(T=(0, 0, 2 * h - off)), lambda r: shifted(corners, r, +1))

    # tetrahedra touching at identity poses
    def tetras(name, p1, p2, expect):
        lib = geometry.ShapeLibrary()
        lib.add_convex(p1)
        lib.add_convex(p2)
        cases[name] = (lib, 0, 1, I, I, lambda r: [np.asarray(e, dtype=np.float64) for e in expect])

    seg = [(0, 0.5, 0), (0, 1.0, 0)]
    tetras("edge_case_segment_segment/1", [(-1, 0, 0), (0, 0, 0), (0, 1, 0), (-1, -1, -1)],
           [(0, 0.5, 0), (0, 1.5, 0), (1, 0.5, 0), (1, 1, 1)], seg)
    tetras("edge_case_segment_segment/2", [(-1, 0, -0.2), (0, 0, 0), (0, 1, 0), (-1, -1, -1)],
           [(0, 0.5, 0), (0, 1.5, 0), (1, 0.5, 0), (1, 1, 1)], seg)
    tetras("edge_case_segment_segment/3", [(-1, 0, -0.2), (0, 0, 0), (0, 1, 0), (-1, -1, -1)],
           [(0, 0.5, 0), (0, 1.5, 0), (1, 0.5, 0.5), (1, 1, 1)], seg)
    vtx = [(0, 0, 0)]
    tetras("edge_case_vertex_vertex/1", [(-1, 0, 0), (0, 0, 0), (0, 1, 0), (-1, -1, -1)],
           [(1, 0, 0), (0, 0, 0), (0, -1, 0), (1, 1, 1)], vtx)
    tetras("edge_case_vertex_vertex/2", [(-1, 0, -0.5), (0, 0, 0), (0, 1, 0), (-1, -1, -1)],
           [(1, 0, 0), (0, 0, 0), (0, -1, 0), (1, 1, 1)], vtx)
    tetras("edge_case_vertex_vertex/3", [(-1, 0, -0.2), (0, 0, 0), (0, 1, 0), (-1, -1, -1)],
           [(1, 0, 0), (0, 0, 0), (0, -1, 0.5), (1, 1, 1)], vtx)
    tetras("edge_case_segment_face", [(-1, 0, 0), (0, 0, 0), (0, 1, 0), (-1, -1, -1)],
           [(-0.5, 0.5, 0), (0.5, -0.5, 0), (1, 0.5, 0.5), (1, 1, 1)], [(0, 0, 0), (-0.5, 0.5, 0)])
    assert sorted(cases) == sorted(REFERENCE_CASE_NAMES)
    return cases


def parallel_capsules(geometry):
    """Two capsules side by side, axes both along world x, the upper one shifted by 0.3 along x and resting 1e-3 deep.  The
    normal is exactly +z, so the patch frame's axes are the world's and both support sets are segments along the frame's x
    with exactly equal y: (b0-a0)(d1-c1) >= (b1-a1)(d0-c0) reads 0 >= 0.  The reference's boolean `det` is 1 there and the
    patch is the single point Contact::pos; a real determinant (0) would give the two ends of the overlap instead.
    Returns (library, tf1, tf2) for the pair (0, 1)."""
    L = geometry.ShapeLibrary()
    L.add_capsule(0.1, 1.0)
    L.add_capsule(0.1, 1.0)
    Rx = np.array([[0, 0, 1.0], [0, 1.0, 0], [-1.0, 0, 0]])  # capsule axis (local z) -> world x
    tf1 = geometry.make_pose(R=Rx, T=np.zeros(3)).reshape(1, 12)
    tf2 = geometry.make_pose(R=Rx, T=np.array([0.3, 0, 0.2 - 0.001])).reshape(1, 12)
    return L, tf1, tf2


def split_mismatches(out, pts, model, point_tol):
    """Engine patches against the model, record by record.  Returns (hard, ties):
    hard -- records that differ in class, swap bit, point count, frame bits or depth, or whose points differ beyond point_tol
            in a way that is not a reordering;
    ties -- records equal in all of that whose points are the model's points within point_tol, but in another order (the
            order of collinear points at equal distance in the hull's sort is the one place where that can happen)."""
    hard, ties = [], []
    for i, (cls, sw, tf, depth, mp) in enumerate(model):
        same = int(out["status"][i]) & 3 == cls and int(out["num_points"][i]) == len(mp)
        same = same and bool((int(out["status"][i]) & SWAPPED) != 0) == sw
        if same and cls != NONE:
            same = np.array_equal(out["tf"][i], np.asarray(tf, dtype=np.float64)) and out["penetration_depth"][i] == depth
        if not same:
            hard.append(i)
            continue
        if not mp:
            continue
        got, want = pts[i, :len(mp)], np.asarray(mp, dtype=np.float64)
        if np.abs(got - want).max() <= point_tol:
            continue
        used, matched = set(), True
        for q in got:
            j = next((j for j in range(len(want)) if j not in used and np.abs(q - want[j]).max() <= point_tol), None)
            if j is None:
                matched = False
                break
            used.add(j)
        (ties if matched else hard).append(i)
    return hard, ties
