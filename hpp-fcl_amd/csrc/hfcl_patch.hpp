// hfcl_patch.hpp -- contact patches of collide() records: hpp::fcl::computeContactPatch, fp64, one record per call.
//
// Behavioural contract (reference file:line):
//   entry point        src/contact_patch.cpp:48-97 (no collision / max_num_patch == 0: no patch; GEOM x BVH runs as
//                      (BVH, GEOM) and is then mirrored by ContactPatchResult::swapObjects, collision_data.h:968-980)
//   frame              constructContactPatchFrameFromContact (collision_data.h:706-713), constructOrthonormalBasisFromVector
//                      (math/transform.h:261-267) with Eigen's unitOrthogonal / normalized
//   solver             contact_patch/contact_patch_solver.hxx:76-427 (computePatch, getResult, reset,
//                      computeLineSegmentIntersection); Plane / Halfspace rows internal/shape_shape_contact_patch_func.h:85-250
//   support sets       src/narrowphase/support_functions.cpp:529-1113 (WithSweptSphere), hull of the cloud 993-1113
//
// Everything here is HFCL_HD: the kernels of hfcl_k_patch.hip and the host build of tests/patch_harness run the same code.
// Polygons live in caller storage (PatchWs): a workspace slot in device memory, plain arrays on the host -- never in
// runtime-indexed per-lane arrays.  Arithmetic is written out in one order (sums left to right); the units that include
// this header are built without contraction, so the host build and the device agree bit for bit.
#pragma once
#include "hfcl_shapes.hpp"
#include "../../include/hppfcl_amd.h"

namespace hfcl {

// Copies are written member by member: the implicit (memcpy) copy of points between workspace slots left 16-byte private
// temporaries that the backend then placed in LDS and scratch.
struct P2 {
  double x, y;
  P2() = default;
  HFCL_HD P2(double x_, double y_) : x(x_), y(y_) {}
  HFCL_HD P2(const P2& o) : x(o.x), y(o.y) {}
  HFCL_HD P2& operator=(const P2& o) {
    x = o.x;
    y = o.y;
    return *this;
  }
};

// record classes (k_patch_classify): each class runs in a kernel of its own
enum { PATCH_NONE = 0, PATCH_POINT = 1, PATCH_ONESIDED = 2, PATCH_CLIPPED = 3 };

// Eigen::NumTraits<double>::dummy_precision() / epsilon()
HFCL_HD double patch_dummy() { return 1e-12; }
HFCL_HD double patch_eps() { return 2.2204460492503131e-16; }

HFCL_HD bool kind_strictly_convex(int k) { return k == K_SPHERE || k == K_ELLIPSOID; }

// Upper bound on the support set of one shape (points of its polygon in the patch plane).
HFCL_HD uint32_t patch_set_bound(int kind, uint32_t num_points, uint32_t num_samples) {
  switch (kind) {
    case K_BOX: return 4u;
    case K_TRIANGLE: return 3u;
    case K_CAPSULE: return 2u;
    case K_CONE:
    case K_CYLINDER: return num_samples > 2u ? num_samples : 2u;
    case K_CONVEX: return num_points;
    default: return 1u;  // sphere, ellipsoid, plane, halfspace, BVH: a point
  }
}

// Class of a record whose shapes are (k1, k2); `swapped` receives whether the reference mirrors the patch (GEOM x BVH).
HFCL_HD int patch_class(int k1, int k2, const hfcl_result& r, uint32_t max_num_patch, bool& swapped) {
  swapped = false;
  if (max_num_patch == 0u || r.num_contacts <= 0 || ((r.status >> 31) & 1u)) return PATCH_NONE;
  if (k1 == K_BVH || k2 == K_BVH) {
    swapped = (k1 != K_BVH);
    return PATCH_POINT;
  }
  const bool f1 = kind_is_flat(k1), f2 = kind_is_flat(k2);
  if (f1 && f2) return PATCH_POINT;
  if (kind_strictly_convex(k1) || kind_strictly_convex(k2)) return PATCH_POINT;
  if (f1 || f2) return PATCH_ONESIDED;
  return PATCH_CLIPPED;
}

// ---------------------------------------------------------------------------------------
// Frame
// ---------------------------------------------------------------------------------------
// Eigen's unitOrthogonal for a 3-vector (OrthoMethods.h): the 2-D norm's reciprocal times the swapped components.
HFCL_HD V3<double> unit_orthogonal(const V3<double>& v) {
  const double p = patch_dummy();
  if (!(habs(v.x) <= habs(v.z) * p) || !(habs(v.y) <= habs(v.z) * p)) {
    const double invnm = 1.0 / hsqrt(v.x * v.x + v.y * v.y);
    return mk<double>(-v.y * invnm, v.x * invnm, 0.0);
  }
  const double invnm = 1.0 / hsqrt(v.y * v.y + v.z * v.z);
  return mk<double>(0.0, -v.z * invnm, v.y * invnm);
}

// Patch frame of a record: rotation rows (R.r0 = row 0) whose columns are (x, y, normal), translation contact.pos.
HFCL_HD Pose<double> patch_frame(const hfcl_result& r) {
  const V3<double> n = mk<double>(r.normal[0], r.normal[1], r.normal[2]);
  const V3<double> c2 = normalized(n);
  const V3<double> c1 = -unit_orthogonal(n);
  const V3<double> c0 = cross(c1, n);
  Pose<double> f;
  f.R.r0 = mk<double>(c0.x, c1.x, c2.x);
  f.R.r1 = mk<double>(c0.y, c1.y, c2.y);
  f.R.r2 = mk<double>(c0.z, c1.z, c2.z);
  f.t = mk<double>((r.p1[0] + r.p2[0]) / 2.0, (r.p1[1] + r.p2[1]) / 2.0, (r.p1[2] + r.p2[2]) / 2.0);
  return f;
}

// tf.inverseTransform(p).head<2>(): R^T (p - t), first two components
HFCL_HD P2 inv_xy(const Pose<double>& tf, const V3<double>& p) {
  const V3<double> d = p - tf.t;
  P2 q;
  q.x = tf.R.r0.x * d.x + tf.R.r1.x * d.y + tf.R.r2.x * d.z;
  q.y = tf.R.r0.y * d.x + tf.R.r1.y * d.y + tf.R.r2.y * d.z;
  return q;
}

// Frame of a shape's support set (ContactPatchSolver::reset, contact_patch_solver.hxx:375-409): patch frame in the shape's frame
HFCL_HD Pose<double> set_frame(const Pose<double>& tfs, const Pose<double>& tfc) {
  Pose<double> r;
  r.R = tmul(tfs.R, tfc.R);
  r.t = tmul(tfs.R, tfc.t - tfs.t);
  return r;
}

// ---------------------------------------------------------------------------------------
// Workspace of one record in flight
// ---------------------------------------------------------------------------------------
struct PatchWs {
  P2* poly0;          // support set of shape 1, of shape 2, Sutherland-Hodgman buffer: `cap` points each (three
  P2* poly1;          // named pointers, no array: a runtime-indexed member would put the whole struct in scratch)
  P2* poly2;
  P2* cloud;          // unsorted support points of a box / convex: `cloud_cap` points
  P2* sortbuf;        // stable_sort's buffer: cloud_cap / 2 + 1 points
  uint8_t* visited;   // neighbour-graph walk of a large convex: `vis_cap` flags
  uint32_t* stack;    // ... its depth-first stack: 2 * vis_cap words
  uint32_t cap, cloud_cap, vis_cap;
  bool overflow;      // a set outgrew its storage (never with the documented bound); the record gets no points
};

// Vertex adjacency of one convex shape (ConvexBase::neighbors): off[v] .. off[v + 1] index ids(k); off == nullptr: none.
struct PatchGraph {
  const uint32_t* off;
  const uint32_t* ids;     // host form: plain ids
  const uint32_t* ent;     // device form: the NbrEntry<double> image (8 words per entry, id at word 6)
  HFCL_HD uint32_t id(uint32_t k) const { return ids ? ids[k] : ent[8 * size_t(k) + 6]; }
};

HFCL_HD P2* ws_poly(const PatchWs& ws, int i) { return i == 0 ? ws.poly0 : (i == 1 ? ws.poly1 : ws.poly2); }

HFCL_HD void ws_push(PatchWs& ws, P2* poly, uint32_t& n, uint32_t lim, const P2& p) {
  if (n >= lim) {
    ws.overflow = true;
    return;
  }
  poly[n++] = p;
}

// ---------------------------------------------------------------------------------------
// Hull of a cloud (computeSupportSetConvexHull, support_functions.cpp:993-1113)
// ---------------------------------------------------------------------------------------
// The comparator of the Graham scan's sort: not a strict weak order (`<=` on collinear ties).
HFCL_HD bool hull_less(const P2& p1, const P2& p2, const P2& v) {
  const double det = (p1.x - v.x) * (p2.y - v.y) - (p1.y - v.y) * (p2.x - v.x);
  if (habs(det) <= patch_dummy()) {
    const double a = (p1.x - v.x) * (p1.x - v.x) + (p1.y - v.y) * (p1.y - v.y);
    const double b = (p2.x - v.x) * (p2.x - v.x) + (p2.y - v.y) * (p2.y - v.y);
    return a <= b;
  }
  return det > 0;
}

// libstdc++'s std::stable_sort with a buffer of (len + 1) / 2 elements (bits/stl_algo.h: __stable_sort ->
// __stable_sort_adaptive -> __merge_sort_with_buffer (insertion sort of 7-element chunks, merge passes) on each half, then
// __merge_adaptive).  Restated step for step: with a comparator that is not a strict weak order the order of ties is this
// algorithm's and no other's.
HFCL_HD void ss_insertion(P2* a, uint32_t n, const P2& v) {
  for (uint32_t i = 1; i < n; ++i) {
    const P2 val = a[i];
    if (hull_less(val, a[0], v)) {
      for (uint32_t k = i; k > 0; --k) a[k] = a[k - 1];
      a[0] = val;
    } else {
      uint32_t last = i;
      while (hull_less(val, a[last - 1], v)) {
        a[last] = a[last - 1];
        --last;
      }
      a[last] = val;
    }
  }
}
// __move_merge: [f1, l1) and [f2, l2) into out; ties take the first range
HFCL_HD uint32_t ss_move_merge(const P2* s, uint32_t f1, uint32_t l1, uint32_t f2, uint32_t l2, P2* out, uint32_t o, const P2& v) {
  while (f1 != l1 && f2 != l2) {
    if (hull_less(s[f2], s[f1], v))
      out[o++] = s[f2++];
    else
      out[o++] = s[f1++];
  }
  while (f1 != l1) out[o++] = s[f1++];
  while (f2 != l2) out[o++] = s[f2++];
  return o;
}
HFCL_HD void ss_merge_loop(const P2* src, uint32_t len, P2* dst, uint32_t step, const P2& v) {
  const uint32_t two = 2 * step;
  uint32_t f = 0, o = 0;
  while (len - f >= two) {
    o = ss_move_merge(src, f, f + step, f + step, f + two, dst, o, v);
    f += two;
  }
  const uint32_t s = (len - f) < step ? (len - f) : step;
  ss_move_merge(src, f, f + s, f + s, len, dst, o, v);
}
HFCL_HD void ss_merge_sort_with_buffer(P2* a, uint32_t len, P2* buf, const P2& v) {
  uint32_t step = 7;
  {
    uint32_t f = 0;
    while (len - f >= step) {
      ss_insertion(a + f, step, v);
      f += step;
    }
    ss_insertion(a + f, len - f, v);
  }
  while (step < len) {
    ss_merge_loop(a, len, buf, step, v);
    step *= 2;
    ss_merge_loop(buf, len, a, step, v);
    step *= 2;
  }
}
HFCL_HD void stable_sort_cloud(P2* a, uint32_t n, P2* buf, const P2& v) {
  if (n == 0) return;
  const uint32_t len1 = (n + 1) / 2, len2 = n - len1;
  ss_merge_sort_with_buffer(a, len1, buf, v);
  ss_merge_sort_with_buffer(a + len1, len2, buf, v);
  if (len1 <= len2) {  // __move_merge_adaptive: the first half through the buffer, forwards
    for (uint32_t k = 0; k < len1; ++k) buf[k] = a[k];
    uint32_t f1 = 0, f2 = len1, o = 0;
    while (f1 != len1 && f2 != n) {
      if (hull_less(a[f2], buf[f1], v))
        a[o++] = a[f2++];
      else
        a[o++] = buf[f1++];
    }
    while (f1 != len1) a[o++] = buf[f1++];
  } else {  // __move_merge_adaptive_backward: the second half through the buffer, backwards
    for (uint32_t k = 0; k < len2; ++k) buf[k] = a[len1 + k];
    if (len2 == 0) return;
    int l1 = int(len1) - 1, l2 = int(len2) - 1, res = int(n);
    for (;;) {
      if (hull_less(buf[l2], a[l1], v)) {
        a[--res] = a[l1];
        if (l1 == 0) {
          for (int k = l2; k >= 0; --k) a[--res] = buf[k];
          return;
        }
        --l1;
      } else {
        a[--res] = buf[l2];
        if (l2 == 0) return;
        --l2;
      }
    }
  }
}

// cloud[0, n) -> hull (counter-clockwise), returns its size.  `cloud` is permuted.
HFCL_HD uint32_t cloud_hull(PatchWs& ws, P2* cloud, uint32_t n, P2* hull, uint32_t lim) {
  uint32_t m = 0;
  if (n <= 2) {
    for (uint32_t i = 0; i < n; ++i) ws_push(ws, hull, m, lim, cloud[i]);
    return m;
  }
  if (n == 3) {
    P2 t;
    if (cloud[0].y > cloud[1].y) { t = cloud[0]; cloud[0] = cloud[1]; cloud[1] = t; }
    if (cloud[0].y > cloud[2].y) { t = cloud[0]; cloud[0] = cloud[2]; cloud[2] = t; }
    const P2 a = cloud[0], b = cloud[1], c = cloud[2];
    const double det = (b.x - a.x) * (c.y - a.y) - (b.y - a.y) * (c.x - a.x);
    if (det < 0) { t = cloud[1]; cloud[1] = cloud[2]; cloud[2] = t; }
    for (uint32_t i = 0; i < 3; ++i) ws_push(ws, hull, m, lim, cloud[i]);
    return m;
  }
  uint32_t si = 0;
  double sv = cloud[0].y;
  for (uint32_t i = 1; i < n; ++i)
    if (cloud[i].y < sv) {
      sv = cloud[i].y;
      si = i;
    }
  { const P2 t = cloud[0]; cloud[0] = cloud[si]; cloud[si] = t; }
  const P2 v = cloud[0];
  ws_push(ws, hull, m, lim, v);
  stable_sort_cloud(cloud + 1, n - 1, ws.sortbuf, v);
  uint32_t i = 1;
  // (the reference's loop reads past the cloud when fewer than three distinct points remain: stopped at its end here)
  while (m < 3 && i < n) {
    const P2 q = cloud[i];
    const double dx = hull[m - 1].x - q.x, dy = hull[m - 1].y - q.y;
    if (dx * dx + dy * dy > patch_eps()) ws_push(ws, hull, m, lim, q);
    if (ws.overflow) return 0;
    ++i;
  }
  for (; i < n; ++i) {
    const P2 q = cloud[i];
    while (m > 1) {
      const P2 a = hull[m - 2], b = hull[m - 1];
      const double det = (b.x - a.x) * (q.y - a.y) - (b.y - a.y) * (q.x - a.x);
      if (det > patch_dummy()) break;
      --m;
    }
    ws_push(ws, hull, m, lim, q);
  }
  return m;
}

// ---------------------------------------------------------------------------------------
// Support sets (getShapeSupportSet<WithSweptSphere>), in the patch plane.  `tf` is the set's frame (set_frame), `inverted`:
// the set looks along -normal (PatchDirection::INVERTED).  `hint`: cached support guess of this operand (convex log form).
// ---------------------------------------------------------------------------------------
HFCL_HD uint32_t support_set(PatchWs& ws, const DShape<double>& s, const double* verts, const PatchGraph& g, const Pose<double>& tf,
                             bool inverted, int hint, uint32_t num_samples, double tol, P2* out) {
  const uint32_t lim = ws.cap;
  uint32_t n = 0;
  const V3<double> c2 = mk<double>(tf.R.r0.z, tf.R.r1.z, tf.R.r2.z);
  const V3<double> d = inverted ? -c2 : c2;
  const V3<double> ssr = s.ssr * d;
  if (s.kind == K_TRIANGLE) {
    const double* v = verts + 3 * size_t(s.vertex_offset);
    const V3<double> a = mk<double>(v[0], v[1], v[2]), b = mk<double>(v[3], v[4], v[5]), c = mk<double>(v[6], v[7], v[8]);
    const double da = dot(d, a), db = dot(d, b), dc = dot(d, c);
    const V3<double> sup = (da > db) ? ((dc > da) ? c : a) : ((dc > db) ? c : b);
    const double sv = dot(sup, d);
    if (sv - dot(d, a) < tol) ws_push(ws, out, n, lim, inv_xy(tf, a + ssr));
    if (sv - dot(d, b) < tol) ws_push(ws, out, n, lim, inv_xy(tf, b + ssr));
    if (sv - dot(d, c) < tol) ws_push(ws, out, n, lim, inv_xy(tf, c + ssr));
    return n;
  }
  if (s.kind == K_BOX) {
    const V3<double> sup = prim_support(s, d);
    const double sv = dot(sup, d);
    const double x = s.p0, y = s.p1, z = s.p2;
    uint32_t m = 0;
    for (int k = 0; k < 8; ++k) {  // corners in the reference's order: (x,y,z) (-x,y,z) (-x,-y,z) (x,-y,z), then -z
      const double cx = (k == 0 || k == 3 || k == 4 || k == 7) ? x : -x;
      const double cy = (k == 0 || k == 1 || k == 4 || k == 5) ? y : -y;
      const double cz = k < 4 ? z : -z;
      const V3<double> cr = mk<double>(cx, cy, cz);
      if (sv - dot(cr, d) < tol) ws_push(ws, ws.cloud, m, ws.cloud_cap, inv_xy(tf, cr + ssr));
    }
    if (ws.overflow) return 0;
    return cloud_hull(ws, ws.cloud, m, out, lim);
  }
  if (s.kind == K_CAPSULE) {
    const V3<double> sup = prim_support(s, d);
    const double r = s.p0, h = s.p1;
    const double sv = dot(d, sup + r * d);
    const V3<double> q1 = mk<double>(r * d.x, r * d.y, h), q2 = mk<double>(r * d.x, r * d.y, -h);
    if ((sv - dot(d, q1) <= tol) && (sv - dot(d, q2) <= tol)) {
      ws_push(ws, out, n, lim, inv_xy(tf, q1 + ssr));
      ws_push(ws, out, n, lim, inv_xy(tf, q2 + ssr));
    } else {
      ws_push(ws, out, n, lim, inv_xy(tf, sup + ssr));
    }
    return n;
  }
  if (s.kind == K_CONE || s.kind == K_CYLINDER) {
    const V3<double> sup = prim_support(s, d);
    const double sv = dot(sup, d);
    const double r = s.p0, h = s.p1;
    const double z = (s.kind == K_CONE) ? -h : (d.z <= 0 ? -h : h);
    const V3<double> q1 = mk<double>(r * d.x, r * d.y, z), q2 = mk<double>(-r * d.x, -r * d.y, z);
    if ((sv - dot(d, q1) <= tol) && (sv - dot(d, q2) <= tol)) {
      const double inc = 2.0 * 3.141592653589793 / double(num_samples);
      for (uint32_t i = 0; i < num_samples; ++i) {
        const double th = double(i) * inc;
        const V3<double> q = mk<double>(r * cos(th), r * sin(th), z);
        ws_push(ws, out, n, lim, inv_xy(tf, q + ssr));
      }
    } else if (s.kind == K_CONE) {
      const V3<double> tip = mk<double>(0.0, 0.0, h);
      if (sv - dot(d, tip) <= tol) ws_push(ws, out, n, lim, inv_xy(tf, tip + ssr));
      const V3<double> base = mk<double>(r * d.x, r * d.y, z);
      if (sv - dot(d, base) <= tol) ws_push(ws, out, n, lim, inv_xy(tf, base + ssr));
    } else {
      const V3<double> lo = mk<double>(r * d.x, r * d.y, -h), hi = mk<double>(r * d.x, r * d.y, h);
      if (sv - dot(d, lo) <= tol) ws_push(ws, out, n, lim, inv_xy(tf, lo + ssr));
      if (sv - dot(d, hi) <= tol) ws_push(ws, out, n, lim, inv_xy(tf, hi + ssr));
    }
    return n;
  }
  if (s.kind == K_CONVEX) {
    const double* v = verts + 3 * size_t(s.vertex_offset);
    const uint32_t np = s.num_points;
    uint32_t m = 0;
    if (np > 32u && g.off != nullptr && np <= ws.vis_cap) {
      // getShapeSupportLog from the guess (no warm start: a fresh solver's last direction is zero), then
      // convexSupportSetRecurse: depth-first over the neighbours, vertices within `tol` of the support plane
      uint32_t cur = (hint < 0 || hint >= int(np)) ? 0u : uint32_t(hint);
      for (uint32_t k = 0; k < np; ++k) ws.visited[k] = 0;
      double best = v[3 * cur] * d.x + v[3 * cur + 1] * d.y + v[3 * cur + 2] * d.z;
      ws.visited[cur] = 1;
      bool found = true, loose = true;
      while (found) {
        found = false;
        const uint32_t b = g.off[cur], e = g.off[cur + 1];
        for (uint32_t k = b; k < e; ++k) {
          const uint32_t ip = g.id(k);
          if (ws.visited[ip]) continue;
          ws.visited[ip] = 1;
          const double dd = v[3 * ip] * d.x + v[3 * ip + 1] * d.y + v[3 * ip + 2] * d.z;
          bool better = false;
          if (dd > best) {
            better = true;
            loose = false;
          } else if (loose && dd == best) {
            better = true;
          }
          if (better) {
            best = dd;
            cur = ip;
            found = true;
          }
        }
      }
      const V3<double> sup = mk<double>(v[3 * cur], v[3 * cur + 1], v[3 * cur + 2]);
      const double sv = dot(sup, d);
      for (uint32_t k = 0; k < np; ++k) ws.visited[k] = 0;
      uint32_t sp = 0;
      ws.visited[cur] = 1;
      if (sv - dot(sup, d) <= tol) {
        ws_push(ws, ws.cloud, m, ws.cloud_cap, inv_xy(tf, sup + ssr));
        ws.stack[0] = cur;
        ws.stack[1] = g.off[cur];
        sp = 1;
      }
      while (sp > 0 && !ws.overflow) {
        const uint32_t vtx = ws.stack[2 * (sp - 1)], pos = ws.stack[2 * (sp - 1) + 1];
        if (pos >= g.off[vtx + 1]) {
          --sp;
          continue;
        }
        ws.stack[2 * (sp - 1) + 1] = pos + 1;
        const uint32_t u = g.id(pos);
        if (ws.visited[u]) continue;
        ws.visited[u] = 1;
        const V3<double> pu = mk<double>(v[3 * u], v[3 * u + 1], v[3 * u + 2]);
        if (sv - dot(pu, d) <= tol) {
          ws_push(ws, ws.cloud, m, ws.cloud_cap, inv_xy(tf, pu + ssr));
          if (sp >= ws.vis_cap) {
            ws.overflow = true;
            break;
          }
          ws.stack[2 * sp] = u;
          ws.stack[2 * sp + 1] = g.off[u];
          ++sp;
        }
      }
    } else {  // getShapeSupportSetLinear: the first maximum, then every vertex within `tol`, in vertex order
      uint32_t best = 0;
      double bd = v[0] * d.x + v[1] * d.y + v[2] * d.z;
      for (uint32_t i = 1; i < np; ++i) {
        const double dd = v[3 * i] * d.x + v[3 * i + 1] * d.y + v[3 * i + 2] * d.z;
        if (dd > bd) {
          bd = dd;
          best = i;
        }
      }
      const V3<double> sup = mk<double>(v[3 * best], v[3 * best + 1], v[3 * best + 2]);
      const double sv = dot(d, sup);
      for (uint32_t i = 0; i < np; ++i) {
        const V3<double> p = mk<double>(v[3 * i], v[3 * i + 1], v[3 * i + 2]);
        if (sv - dot(d, p) <= tol) ws_push(ws, ws.cloud, m, ws.cloud_cap, inv_xy(tf, p + ssr));
      }
    }
    if (ws.overflow) return 0;
    return cloud_hull(ws, ws.cloud, m, out, lim);
  }
  return 0;  // (strictly convex shapes never get here)
}

// computeLineSegmentIntersection (contact_patch_solver.hxx:410-427)
HFCL_HD P2 line_segment_intersection(const P2& a, const P2& b, const P2& c, const P2& d) {
  const double abx = b.x - a.x, aby = b.y - a.y;
  const double nx = -aby, ny = abx;
  const double den = nx * (c.x - d.x) + ny * (c.y - d.y);
  if (habs(den) < patch_eps()) return d;
  const double num = nx * (a.x - d.x) + ny * (a.y - d.y);
  double al = num / den;
  al = hmin(1.0, hmax(0.0, al));
  P2 r;
  r.x = al * c.x + (1 - al) * d.x;
  r.y = al * c.y + (1 - al) * d.y;
  return r;
}

// The point patch: contact.pos in the patch frame.
HFCL_HD P2 patch_origin(const Pose<double>& fr) { return inv_xy(fr, fr.t); }

// One record of class PATCH_ONESIDED or PATCH_CLIPPED.  Writes the result polygon to `pts` (room for `pcap` points), returns
// its size (>= 1; 0 only when ws.overflow).
HFCL_HD uint32_t patch_compute(PatchWs& ws, const DShape<double>& s1, const Pose<double>& tf1, const PatchGraph& g1,
                               const DShape<double>& s2, const Pose<double>& tf2, const PatchGraph& g2, const double* verts,
                               const Pose<double>& fr, int guess0, int guess1, uint32_t num_samples, double tol, P2* pts,
                               uint32_t pcap) {
  const double eps = patch_dummy();
  uint32_t np = 0;
  const bool f1 = kind_is_flat(s1.kind), f2 = kind_is_flat(s2.kind);
  if (f1 || f2) {  // computePatchPlaneOrHalfspace: the other shape's set, not clipped
    const bool inv = f1;  // the plane is the first operand: InvertShapes, the set looks along -normal
    const DShape<double>& o = f1 ? s2 : s1;
    const Pose<double>& to = f1 ? tf2 : tf1;
    const uint32_t n = support_set(ws, o, verts, f1 ? g2 : g1, set_frame(to, fr), inv, f1 ? guess1 : guess0, num_samples, tol,
                                   ws.poly0);
    if (ws.overflow) return 0;
    if (n <= 1) {
      ws_push(ws, pts, np, pcap, patch_origin(fr));
      return np;
    }
    if (n > pcap) {
      ws.overflow = true;
      return 0;
    }
    for (uint32_t i = 0; i < n; ++i) pts[i] = ws.poly0[i];
    return n;
  }
  const uint32_t n1 = support_set(ws, s1, verts, g1, set_frame(tf1, fr), false, guess0, num_samples, tol, ws.poly0);
  const uint32_t n2 = support_set(ws, s2, verts, g2, set_frame(tf2, fr), true, guess1, num_samples, tol, ws.poly1);
  if (ws.overflow) return 0;
  if (n1 <= 1 || n2 <= 1) {
    ws_push(ws, pts, np, pcap, patch_origin(fr));
    return np;
  }
  if (n1 == 2 && n2 == 2 && pcap >= 2) {  // segment x segment
    const P2 a = ws.poly0[0], b = ws.poly0[1], c = ws.poly1[0], dd = ws.poly1[1];
    // the reference's `det` is the boolean of this comparison converted to 0 / 1 (contact_patch_solver.hxx:149-150)
    const double det = ((b.x - a.x) * (dd.y - c.y) >= (b.y - a.y) * (dd.x - c.x)) ? 1.0 : 0.0;
    const double cdx = c.x - dd.x, cdy = c.y - dd.y, bax = b.x - a.x, bay = b.y - a.y;
    if ((habs(det) > eps) || ((cdx * cdx + cdy * cdy) < eps) || ((bax * bax + bay * bay) < eps)) {
      ws_push(ws, pts, np, pcap, patch_origin(fr));
      return np;
    }
    const double ux = dd.x - c.x, uy = dd.y - c.y;
    const double l = ux * ux + uy * uy;
    double t1 = (a.x - c.x) * ux + (a.y - c.y) * uy;
    t1 = (t1 >= l) ? 1.0 : ((t1 <= 0) ? 0.0 : (t1 / l));
    P2 q1;
    q1.x = c.x + t1 * ux;
    q1.y = c.y + t1 * uy;
    pts[np++] = q1;
    double t2 = (b.x - c.x) * ux + (b.y - c.y) * uy;
    t2 = (t2 >= l) ? 1.0 : ((t2 <= 0) ? 0.0 : (t2 / l));
    P2 q2;
    q2.x = c.x + t2 * ux;
    q2.y = c.y + t2 * uy;
    const double ex = q1.x - q2.x, ey = q1.y - q2.y;
    if (ex * ex + ey * ey >= eps) pts[np++] = q2;
    return np;
  }
  // Sutherland-Hodgman: the larger set clips the smaller
  int cur, clip;
  uint32_t ncur, nclip;
  if (n1 < n2) {
    cur = 0; clip = 1; ncur = n1; nclip = n2;
  } else {
    cur = 1; clip = 0; ncur = n2; nclip = n1;
  }
  int prev = 2;
  uint32_t nprev = 0;
  const P2* clipper = ws_poly(ws, clip);
  for (uint32_t i = 0; i < nclip; ++i) {
    { const int t = prev; prev = cur; cur = t; }
    nprev = ncur;
    ncur = 0;
    const P2* pv = ws_poly(ws, prev);
    P2* cu = ws_poly(ws, cur);
    const P2 a = clipper[i], b = clipper[(i + 1) % nclip];
    const double abx = b.x - a.x, aby = b.y - a.y;
    if (nprev == 2) {
      const P2 p1 = pv[0], p2 = pv[1];
      const double det1 = abx * (p1.y - a.y) - aby * (p1.x - a.x);
      const double det2 = abx * (p2.y - a.y) - aby * (p2.x - a.x);
      if (det1 < 0 && det2 < 0) break;
      if (det1 >= 0 && det2 >= 0) {
        cu[0] = p1;
        cu[1] = p2;
        ncur = 2;
        continue;
      }
      if (det1 >= 0) {
        if (det1 > eps) {
          const P2 p = line_segment_intersection(a, b, p1, p2);
          cu[0] = p1;
          cu[1] = p;
          ncur = 2;
          continue;
        }
        cu[0] = p1;
        ncur = 1;
        break;
      }
      if (det2 > eps) {
        const P2 p = line_segment_intersection(a, b, p1, p2);
        cu[0] = p2;
        cu[1] = p;
        ncur = 2;
        continue;
      }
      cu[0] = p2;
      ncur = 1;
      break;
    }
    // polygon x polygon.  added_to_patch[j] is set by step j (p1) or by step j - 1 (p2 of the edge before): a flag carried
    // from the step before, and the flag of vertex 0 for the last step
    bool added0 = false, carry = false;
    for (uint32_t j = 0; j < nprev; ++j) {
      const uint32_t jn = (j + 1) % nprev;
      const P2 p1 = pv[j], p2 = pv[jn];
      const double det1 = abx * (p1.y - a.y) - aby * (p1.x - a.x);
      const double det2 = abx * (p2.y - a.y) - aby * (p2.x - a.x);
      const bool added_j = (j == 0) ? added0 : carry;
      bool set_j = false, set_next = false;
      if (det1 < 0 && det2 < 0) {
      } else if (det1 >= 0 && det2 >= 0) {
        if (!added_j) {
          ws_push(ws, cu, ncur, ws.cap, p1);
          set_j = true;
        }
      } else if (det1 >= 0) {
        if (!added_j) {
          ws_push(ws, cu, ncur, ws.cap, p1);
          set_j = true;
        }
        if (det1 > eps) ws_push(ws, cu, ncur, ws.cap, line_segment_intersection(a, b, p1, p2));
      } else {
        if (det2 > eps) {
          ws_push(ws, cu, ncur, ws.cap, line_segment_intersection(a, b, p1, p2));
        } else {
          const bool added_n = (jn == 0) ? (added0 || (j == 0 && set_j)) : false;
          if (!added_n) {
            ws_push(ws, cu, ncur, ws.cap, p2);
            set_next = true;
          }
        }
      }
      if (j == 0 && set_j) added0 = true;
      if (set_next && jn == 0) added0 = true;
      carry = set_next;
    }
    if (ws.overflow) return 0;
    if (ncur <= 1) break;
  }
  if (ncur <= 1) {
    ws_push(ws, pts, np, pcap, patch_origin(fr));
    return np;
  }
  if (ncur > pcap) {
    ws.overflow = true;
    return 0;
  }
  for (uint32_t k = 0; k < ncur; ++k) pts[k] = ws_poly(ws, cur)[k];
  return ncur;
}

// Status word of an hfcl_contact_patch
HFCL_HD uint32_t patch_status(int cls, bool swapped, bool overflow, bool bad_id) {
  return uint32_t(cls) | (swapped ? HFCL_PATCH_SWAPPED : 0u) | (overflow ? HFCL_PATCH_OVERFLOW : 0u) | (bad_id ? HFCL_PATCH_SKIPPED : 0u);
}

// Write the frame of a record (and mirror it for GEOM x BVH: columns 0 and 2 negated).
HFCL_HD void patch_write_frame(hfcl_contact_patch& o, const Pose<double>& fr, double depth, bool swapped) {
  const double sx = swapped ? -1.0 : 1.0;
  o.tf[0] = fr.R.r0.x * sx; o.tf[1] = fr.R.r1.x * sx; o.tf[2] = fr.R.r2.x * sx;
  o.tf[3] = fr.R.r0.y;      o.tf[4] = fr.R.r1.y;      o.tf[5] = fr.R.r2.y;
  o.tf[6] = fr.R.r0.z * sx; o.tf[7] = fr.R.r1.z * sx; o.tf[8] = fr.R.r2.z * sx;
  o.tf[9] = fr.t.x; o.tf[10] = fr.t.y; o.tf[11] = fr.t.z;
  o.penetration_depth = depth;
}
HFCL_HD void patch_write_none(hfcl_contact_patch& o, uint32_t status) {
  for (int k = 0; k < 12; ++k) o.tf[k] = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
  o.penetration_depth = 0.0;
  o.num_points = 0;
  o.status = status;
}

}  // namespace hfcl
