// hfcl_hfield.hpp -- HeightField<AABB> x convex solid collide() (hppfcl_amd_hfield.h): the arithmetic shared by the kernels of
// hfcl_k_hfield.hip, the host builder (hfcl_host_hfield.hip) and the host build of the tests (tests/hfield_harness).
//   the tree         HeightField::init / recursiveBuildTree (include/hpp/fcl/hfield.h:308-479)
//   the box test     HeightFieldShapeCollisionTraversalNode::BVDisjoints (internal/traversal_node_hfield_shape.h:560-581) =
//                    overlap(R1, T1, node.bv, model2_bv, request, sqr) (src/BV/AABB.cpp:141-146, :51-73; rotate / translate BV/AABB.h:234-253)
//                    against computeBV<AABB, S> of the solid (src/shape/geometric_shapes_utility.cpp:292-382)
//   a leaf           leafCollides (:584-642): buildConvexTriangles (:121-232), shapeDistance (:402-509) with binCorrection (:321-400)
//   the walk, fold   collisionRecurse (src/traversal/traversal_recurse.cpp:44-85), updateDistanceLowerBoundFromBV / FromLeaf
//                    (collision_data.h:1177-1197)
// The prism x solid solve is the per-pair solver of hfcl_pair.hpp with the supports of hfcl_shapes.hpp (what a Convex x solid pair of a
// batch runs).  Every unit that includes this is built without contraction of a*b+c: device and host builds compute the same bits.
// Builds with hipcc and with g++.
#pragma once
#include "../../include/hppfcl_amd_hfield.h"
#include "hfcl_pair.hpp"
#include "hfcl_listed.hpp"

namespace hfcl {

constexpr int HF_STACK = 40;  // walk stack entries: a tree over at most 32768 x 32768 samples is 30 levels deep, the stack holds depth + 1

// ---- the tree (host) ----------------------------------------------------------------------------------------------------
// Eigen >= 3.3 LinSpaced, |high| == |low| (no flipped form): low + i * step, the last element exactly high
inline double hf_linspaced(size_t i, size_t n, double low, double high) {
  const double step = (high - low) / double(n - 1);
  return i == n - 1 ? high : low + double(i) * step;
}
struct HfBuilder {
  const double* h;  // clamped heights
  size_t nx;
  double min_height;
  const double* xg;
  const double* yg;
  hfcl_hfield_node* nodes;
  uint32_t num;
  size_t ncols, nrows;
  double rec(uint32_t id, int x_id, int x_size, int y_id, int y_size) {  // recursiveBuildTree; at most 30 levels
    hfcl_hfield_node& n = nodes[id];
    double mh;
    n.first_child = 0;
    n.contact_active_faces = 0;
    if (x_size == 1 && y_size == 1) {
      const double* c = h + size_t(y_id) * nx + size_t(x_id);
      mh = std::max(std::max(c[0], c[nx]), std::max(c[1], c[nx + 1]));
    } else {
      const uint32_t fc = num;
      n.first_child = fc;
      num += 2;
      double ml, mr;
      if (x_size >= y_size) {
        int half = x_size / 2;
        if (x_size == 1) half = 1;
        ml = rec(fc, x_id, half, y_id, y_size);
        mr = rec(fc + 1, x_id + half, x_size - half, y_id, y_size);
      } else {
        int half = y_size / 2;
        if (y_size == 1) half = 1;
        ml = rec(fc, x_id, x_size, y_id, half);
        mr = rec(fc + 1, x_id, x_size, y_id + half, y_size - half);
      }
      mh = std::max(ml, mr);
    }
    hfcl_hfield_node& m = nodes[id];
    m.max_height = mh;
    const double a[3] = {xg[x_id], yg[y_id], min_height}, b[3] = {xg[x_id + x_size], yg[y_id + y_size], mh};
    for (int k = 0; k < 3; ++k) {
      m.aabb_min[k] = std::min(a[k], b[k]);
      m.aabb_max[k] = std::max(a[k], b[k]);
    }
    m.x_id = x_id;
    m.x_size = x_size;
    m.y_id = y_id;
    m.y_size = y_size;
    if (x_size == 1 && y_size == 1) {
      int f = HFCL_HF_FACE_TOP | HFCL_HF_FACE_BOTTOM;
      if (x_id == 0) f |= HFCL_HF_FACE_WEST;
      if (y_id == 0) f |= HFCL_HF_FACE_NORTH;
      if (size_t(x_id) + 1 == ncols - 1) f |= HFCL_HF_FACE_EAST;
      if (size_t(y_id) + 1 == nrows - 1) f |= HFCL_HF_FACE_SOUTH;
      m.contact_active_faces = f;
    }
    return mh;
  }
};

// ---- the solid's world box: computeBV<AABB, S>(solid, tf) -- no swept-sphere radius, as the reference ---------------------------------
template <typename T>
HFCL_HD bool hf_solid_world_box(const DShape<T>& s, const T* verts, const Pose<T>& tf, V3<T>& lo, V3<T>& hi) {
  const M3<T>& R = tf.R;
  V3<T> d;
  if (s.kind == K_BOX) {  // R.cwiseAbs() * halfSide
    d = mk<T>(habs(R.r0.x) * s.p0 + habs(R.r0.y) * s.p1 + habs(R.r0.z) * s.p2, habs(R.r1.x) * s.p0 + habs(R.r1.y) * s.p1 + habs(R.r1.z) * s.p2,
              habs(R.r2.x) * s.p0 + habs(R.r2.y) * s.p1 + habs(R.r2.z) * s.p2);
  } else if (s.kind == K_SPHERE) {
    d = mk<T>(s.p0, s.p0, s.p0);
  } else if (s.kind == K_ELLIPSOID) {  // R * radii (no absolute values: the reference's)
    d = mul(R, mk<T>(s.p0, s.p1, s.p2));
  } else if (s.kind == K_CAPSULE) {  // R.col(2).cwiseAbs() * halfLength + radius
    d = mk<T>(habs(R.r0.z) * s.p1 + s.p0, habs(R.r1.z) * s.p1 + s.p0, habs(R.r2.z) * s.p1 + s.p0);
  } else if (s.kind == K_CONE || s.kind == K_CYLINDER) {
    d = mk<T>(habs(R.r0.x * s.p0) + habs(R.r0.y * s.p0) + habs(R.r0.z * s.p1), habs(R.r1.x * s.p0) + habs(R.r1.y * s.p0) + habs(R.r1.z * s.p1),
              habs(R.r2.x * s.p0) + habs(R.r2.y * s.p0) + habs(R.r2.z * s.p1));
  } else if (s.kind == K_CONVEX) {
    const T big = Lim<T>::max();
    lo = mk<T>(big, big, big);
    hi = mk<T>(-big, -big, -big);
    const T* v = verts + 3 * size_t(s.vertex_offset);
    for (uint32_t i = 0; i < s.num_points; ++i) {  // (bound: the hull's vertices)
      const V3<T> p = xform(tf, mk<T>(v[3 * size_t(i)], v[3 * size_t(i) + 1], v[3 * size_t(i) + 2]));
      lo = mk<T>(hmin(lo.x, p.x), hmin(lo.y, p.y), hmin(lo.z, p.z));
      hi = mk<T>(hmax(hi.x, p.x), hmax(hi.y, p.y), hmax(hi.z, p.z));
    }
    return true;
  } else {
    return false;
  }
  hi = tf.t + d;
  lo = tf.t - d;
  return true;
}
HFCL_HD bool hf_kind_supported(int k) {
  return k == K_BOX || k == K_SPHERE || k == K_CAPSULE || k == K_CONE || k == K_CYLINDER || k == K_ELLIPSOID || k == K_CONVEX;
}

// ---- the box test of one inner node --------------------------------------------------------------------------------------------
// true: disjoint, sq = the squared bound that said so
template <typename T>
HFCL_HD bool hf_node_disjoint(const Pose<T>& tfh, const hfcl_hfield_node& n, const V3<T>& blo, const V3<T>& bhi, T margin, T bd2, T& sq) {
  // rotate(): the box of the eight rotated corners, corner 0 = min_
  V3<T> lo = mul(tfh.R, mk<T>(T(n.aabb_min[0]), T(n.aabb_min[1]), T(n.aabb_min[2])));
  V3<T> hi = lo;
  for (int ic = 1; ic < 8; ++ic) {
    const V3<T> c = mul(tfh.R, mk<T>(T((ic & 1) ? n.aabb_max[0] : n.aabb_min[0]), T((ic & 2) ? n.aabb_max[1] : n.aabb_min[1]),
                                    T((ic & 4) ? n.aabb_max[2] : n.aabb_min[2])));
    lo = mk<T>(hmin(lo.x, c.x), hmin(lo.y, c.y), hmin(lo.z, c.z));
    hi = mk<T>(hmax(hi.x, c.x), hmax(hi.y, c.y), hmax(hi.z, c.z));
  }
  lo = lo + tfh.t;
  hi = hi + tfh.t;
  // AABB::overlap(other, request, sqrDistLowerBound)
  V3<T> g = mk<T>(hmax(lo.x - bhi.x - margin, T(0)), hmax(lo.y - bhi.y - margin, T(0)), hmax(lo.z - bhi.z - margin, T(0)));
  sq = sqnorm(g);
  if (sq > bd2) return true;
  g = mk<T>(hmax(blo.x - hi.x - margin, T(0)), hmax(blo.y - hi.y - margin, T(0)), hmax(blo.z - hi.z - margin, T(0)));
  sq = sqnorm(g);
  if (sq > bd2) return true;
  return false;
}

// ---- the walk --------------------------------------------------------------------------------------------------------------
// collisionRecurse flattened: children pushed right-then-left.  The box tests do not depend on the leaves, so the set and order of the
// visited leaves is fixed by the poses; on_leaf(node, m) gets the running minimum m of the box bounds met so far (sqrt of the squared
// bounds: a bound is > break_distance >= 0, so the `<= 0` latch of updateDistanceLowerBoundFromBV never changes what the minimum takes).
// Returns the minimum over all boxes (DBL_MAX: none was disjoint); overflow: the stack was too small (cannot happen within the limits).
// stack[i * stride]: HF_STACK entries.
template <typename T, class OnLeaf>
HFCL_HD T hf_walk(const hfcl_hfield_node* nodes, uint32_t n_nodes, const Pose<T>& tfh, const V3<T>& blo, const V3<T>& bhi, T margin, T bd2,
                  uint32_t* stack, int stride, OnLeaf on_leaf, bool& overflow) {
  T m = Lim<T>::max();
  int sp = 1;
  stack[0] = 0;
  overflow = false;
  for (uint32_t steps = 0; sp > 0 && steps < n_nodes; ++steps) {  // (a node is visited at most once)
    const uint32_t b1 = stack[(--sp) * stride];
    const hfcl_hfield_node& n = nodes[b1];
    if (n.x_size == 1 && n.y_size == 1) {
      on_leaf(b1, m);
      continue;
    }
    T sq;
    if (hf_node_disjoint(tfh, n, blo, bhi, margin, bd2, sq)) {
      const T nd = hsqrt(sq);
      if (nd < m) m = nd;
      continue;
    }
    if (sp + 2 > HF_STACK) {
      overflow = true;
      break;
    }
    stack[sp * stride] = n.first_child + 1u;
    stack[(sp + 1) * stride] = n.first_child;
    sp += 2;
  }
  return m;
}

// ---- the two prisms of a cell ---------------------------------------------------------------------------------------------
// triangle t of prism `part` (0 / 1), three octal digits a b c: the face tables of buildConvexTriangles
HFCL_HD void hf_prism_triangle(int part, int t, int& a, int& b, int& c) {
  const uint16_t t1[8] = {0021, 0345, 0013, 0314, 0125, 0154, 0052, 0503};
  const uint16_t t2[8] = {0210, 0345, 0013, 0314, 0052, 0035, 0125, 0412};
  const uint32_t w = part ? t2[t] : t1[t];
  a = int(w >> 6);
  b = int((w >> 3) & 7u);
  c = int(w & 7u);
}
template <typename T>
struct HfPrisms {
  V3<T> p[2][6];
  int active[2];
};
template <typename T>
HFCL_HD void hf_build_prisms(const hfcl_hfield_node& n, const double* heights, uint32_t nx, const double* xg, const double* yg, double min_height,
                             HfPrisms<T>& P) {
  const T x0 = T(xg[n.x_id]), x1 = T(xg[n.x_id + 1]), y0 = T(yg[n.y_id]), y1 = T(yg[n.y_id + 1]), mh = T(min_height);
  const double* c = heights + size_t(n.y_id) * nx + size_t(n.x_id);
  const T c00 = T(c[0]), c01 = T(c[1]), c10 = T(c[nx]), c11 = T(c[nx + 1]);  // cell(row, col)
  const int f = n.contact_active_faces;
  P.active[0] = (f & 1) | ((f & HFCL_HF_FACE_WEST) ? 2 : 0) | ((f & HFCL_HF_FACE_NORTH) ? 8 : 0);
  P.active[1] = (f & 1) | ((f & HFCL_HF_FACE_EAST) ? 8 : 0) | ((f & HFCL_HF_FACE_SOUTH) ? 2 : 0);
  P.p[0][0] = mk<T>(x0, y0, mh);
  P.p[0][1] = mk<T>(x0, y1, mh);
  P.p[0][2] = mk<T>(x1, y0, mh);
  P.p[0][3] = mk<T>(x0, y0, c00);
  P.p[0][4] = mk<T>(x0, y1, c10);
  P.p[0][5] = mk<T>(x1, y0, c01);
  P.p[1][0] = mk<T>(x0, y1, mh);
  P.p[1][1] = mk<T>(x1, y1, mh);
  P.p[1][2] = mk<T>(x1, y0, mh);
  P.p[1][3] = mk<T>(x0, y1, c10);
  P.p[1][4] = mk<T>(x1, y1, c11);
  P.p[1][5] = mk<T>(x1, y0, c01);
}

// ---- Project::projectLine / projectTriangle (src/intersect.cpp:432-508) and the point they parameterise ---------------------
// ok = false: a degenerate triangle (the reference's parameterisation is then uninitialised memory); the point returned is the origin
template <typename T>
HFCL_HD V3<T> hf_project_on_triangle(const V3<T>& a, const V3<T>& b, const V3<T>& c, const V3<T>& p, bool& ok) {
  const V3<T> dl0 = a - b, dl1 = b - c, dl2 = c - a;
  const V3<T> n = cross(dl0, dl1);
  const T l = sqnorm(n);
  T par[3] = {T(0), T(0), T(0)};
  ok = l > T(0);
  if (ok) {
    T mindist = T(-1);
    for (int i = 0; i < 3; ++i) {
      const V3<T>& vi = i == 0 ? a : (i == 1 ? b : c);
      const V3<T>& vj = i == 0 ? b : (i == 1 ? c : a);
      const V3<T>& dli = i == 0 ? dl0 : (i == 1 ? dl1 : dl2);
      if (dot(vi - p, cross(dli, n)) > T(0)) {
        const int j = i == 2 ? 0 : i + 1, k = j == 2 ? 0 : j + 1;
        // projectLine(vi, vj, p)
        const V3<T> d = vj - vi;
        const T ll = sqnorm(d);
        T p0 = T(0), p1 = T(0), sqr = T(-1);
        if (ll > T(0)) {
          const T t = dot(p - vi, d);
          p1 = (t >= ll) ? T(1) : ((t <= T(0)) ? T(0) : (t / ll));
          p0 = T(1) - p1;
          if (t >= ll) sqr = sqnorm(p - vj);
          else if (t <= T(0)) sqr = sqnorm(p - vi);
          else sqr = sqnorm(vi + d * p1 - p);
        }
        if (mindist < T(0) || sqr < mindist) {
          mindist = sqr;
          par[i] = p0;
          par[j] = p1;
          par[k] = T(0);
        }
      }
    }
    if (mindist < T(0)) {  // the projection falls inside
      const T d = dot(a - p, n);
      const T s = hsqrt(l);
      const V3<T> ptp = n * (d / l);
      par[0] = norm(cross(dl1, b - p - ptp)) / s;
      par[1] = norm(cross(dl2, c - p - ptp)) / s;
      par[2] = T(1) - par[0] - par[1];
    }
  }
  return par[0] * a + par[1] * b + par[2] * c;
}

// distanceContactPointToFace (:291-319): face 0 / 1 one triangle, a side face two; closest: the triangle
template <typename T>
HFCL_HD T hf_distance_to_face(const V3<T>* pts, int part, int face, const V3<T>& p, int& closest) {
  auto tri_distance = [&](int t) {
    int a, b, c;
    hf_prism_triangle(part, t, a, b, c);
    bool ok;
    const V3<T> q = hf_project_on_triangle(pts[a], pts[b], pts[c], p, ok);
    return ok ? norm(q - p) : Lim<T>::max();
  };
  closest = face;
  const T d1 = tri_distance(face);
  if (face <= 1) return d1;
  const T d2 = tri_distance(face + 1);
  if (d1 > d2) {
    closest = face + 1;
    return d2;
  }
  return d1;
}

// binCorrection (:321-400).  pts: the prism in the field's frame; contact_1 is compared with them as it is (world frame), as the
// reference does.  ssup(dir): getSupport<WithSweptSphere> of the solid in its own frame.  Returns hfield_witness_is_on_bin_side.
template <typename T, class SolidSw>
HFCL_HD bool hf_bin_correction(const V3<T>* pts, int part, int active, const SolidSw& ssup, const Pose<T>& tfs, T& distance, V3<T>& c1, V3<T>& c2,
                               V3<T>& normal, V3<T>& face_normal, bool is_collision) {
  const T prec = T(1e-12);
  bool on_bin_side = true;
  int face_tri = -1;
  T shortest = Lim<T>::max();
  face_normal = normal;
  const int faces[5] = {0, 1, (active & 2) ? 2 : -1, (active & 4) ? 4 : -1, (active & 8) ? 6 : -1};
  for (int k = 0; k < 5; ++k) {
    if (faces[k] < 0) continue;
    int closest;
    const T d = hf_distance_to_face(pts, part, faces[k], c1, closest);
    if (d <= prec) {
      on_bin_side = false;
      face_tri = closest;
      shortest = d;
      break;
    } else if (d < shortest) {
      face_tri = closest;
      shortest = d;
    }
  }
  if (is_collision) {
    if (face_tri < 0) {  // (the reference throws "face_triangle is not initialized": a NaN contact point)
      const T x = Lim<T>::nan();
      distance = x;
      c1 = c2 = normal = face_normal = mk<T>(x, x, x);
      return on_bin_side;
    }
    int a, b, c;
    hf_prism_triangle(part, face_tri, a, b, c);
    const V3<T> pa = pts[a];
    face_normal = normalized(cross(pts[b] - pa, pts[c] - pa));
    const V3<T> sl = ssup(-tmul(tfs.R, face_normal));
    const V3<T> support = xform(tfs, sl);
    const T offset = dot(face_normal, pa);
    // Plane(face_normal, offset): unitNormalTest (src/shape/geometric_shapes.cpp:133-143), then signedDistance (geometric_shapes.h:1003-1014)
    V3<T> pn = mk<T>(T(1), T(0), T(0));
    T pd = T(0);
    const T l = norm(face_normal);
    if (l > T(0)) {
      const T inv = T(1) / l;
      pn = face_normal * inv;
      pd = offset * inv;
    }
    const T dsp = dot(pn, support) - pd;
    const V3<T> projected = support - dsp * face_normal;
    bool ok;
    c1 = hf_project_on_triangle(pa, pts[b], pts[c], projected, ok);
    c2 = c1 + dsp * face_normal;
    normal = face_normal;
    distance = -habs(dsp);
  }
  return on_bin_side;
}

// ---- ShapeShapeDistance<Convex, S>(prism, tf_hfield, solid, tf_solid) with penetration ---------------------------------------------
// MinkowskiDiff of (prism: 6 vertices scanned, first maximum; solid): hfcl_pair.hpp's SerialSupport with the solid's support plugged in
template <typename T, class Solid>
struct PrismSolidSupport {
  const V3<T>* p;
  const Solid* solid;  // V3<T> (*solid)(dir): support of the solid in its own frame (NoSweptSphere)
  MDiff<T> md;
  HFCL_HD void operator()(const V3<T>& dir, V3<T>& w, V3<T>& w0) const {
    int best = 0;
    T bd = dot(p[0], dir);
    for (int i = 1; i < 6; ++i) {
      const T d = dot(p[i], dir);
      if (d > bd) {
        bd = d;
        best = i;
      }
    }
    w0 = p[best];
    const V3<T> d1 = md.identity ? -dir : -tmul(md.oR1, dir);
    V3<T> s1 = (*solid)(d1);
    s1 = md.identity ? s1 : (mul(md.oR1, s1) + md.ot1);
    w = w0 - s1;
  }
};
template <typename T, class Grp, class Solid>
HFCL_HD T hf_prism_distance(const V3<T>* pts, const Pose<T>& tfh, const MDiff<T>& md, const Solid& solid, bool solid_is_convex, T r1,
                            const QParams<T>& q, EpaScratch<T, EPA_MAX_ITER>* scratch, V3<T>& p1, V3<T>& p2, V3<T>& n) {
  PrismSolidSupport<T, Solid> sup;
  sup.p = pts;
  sup.solid = &solid;
  sup.md = md;
  const V3<T> guess0 = mk<T>(T(1), T(0), T(0));  // DefaultGuess
  Gjk<T, PW0<T>> g;
  gjk_run(g, q.gjk, guess0, r1, solid_is_convex, sup);  // normalize_support_direction: both ConvexBase (minkowski_difference.cpp:261-266)
  PairOut<T> o;
  EpaSeed<T> seed;
  if (gjk_finish(g, q, tfh, T(0), r1, guess0, o, seed)) {
    Grp::sync();
    epa_run<T, Grp, EPA_MAX_ITER>(scratch, seed, q, tfh, T(0), r1, sup, o);
    Grp::sync();
  }
  p1 = o.p1;
  p2 = o.p2;
  n = o.normal;
  return o.distance;
}

// ---- a leaf: shapeDistance (:402-509) and the gate of leafCollides (:621-632) -------------------------------------------------
template <typename T>
struct HfLeafOut {
  T distance;
  V3<T> c1, c2, normal;
  uint32_t addable;  // normal_face.isApprox(normal) && (collision || !hfield_witness_is_on_bin_side)
  uint32_t pad;
};
// Eigen isApprox, default precision: |a - b|^2 <= 1e-24 * min(|a|^2, |b|^2)
template <typename T>
HFCL_HD bool hf_is_approx(const V3<T>& a, const V3<T>& b) {
  return sqnorm(a - b) <= T(1e-12) * T(1e-12) * hmin(sqnorm(a), sqnorm(b));
}
// q: mode 1, compute_penetration 1, DefaultGuess, gjk.distance_upper_bound = DBL_MAX (hf_leaf_params)
template <typename T, class Grp, class Solid, class SolidSw>
HFCL_HD void hf_leaf(const hfcl_hfield_node& node, const double* heights, uint32_t nx, const double* xg, const double* yg, double min_height,
                     const Pose<T>& tfh, const Pose<T>& tfs, const Solid& solid, const SolidSw& ssup, bool solid_is_convex, T r1,
                     const QParams<T>& q, EpaScratch<T, EPA_MAX_ITER>* scratch, HfPrisms<T>& P, HfLeafOut<T>& out) {
  // P: the group's own storage (group-shared on the device: the support scans index the vertices at run time); every lane writes the same values
  hf_build_prisms(node, heights, nx, xg, yg, min_height, P);
  Grp::sync();
  const MDiff<T> md = make_mdiff(tfh, tfs);
  T dist[2];
  V3<T> c1[2], c2[2], nrm[2], ntop[2];
  bool coll[2], side[2];
  for (int k = 0; k < 2; ++k) {
    dist[k] = hf_prism_distance<T, Grp>(P.p[k], tfh, md, solid, solid_is_convex, r1, q, scratch, c1[k], c2[k], nrm[k]);
    coll[k] = dist[k] - q.security_margin <= q.collision_distance_threshold;
    side[k] = hf_bin_correction(P.p[k], k, P.active[k], ssup, tfs, dist[k], c1[k], c2[k], nrm[k], ntop[k], coll[k]);
  }
  int pick;
  if (coll[0] && coll[1]) pick = dist[0] > dist[1] ? 1 : 0;
  else if (coll[0]) pick = 0;
  else if (coll[1]) pick = 1;
  else pick = dist[0] > dist[1] ? 1 : 0;
  const bool collision = coll[0] || coll[1];
  out.distance = dist[pick];
  out.c1 = c1[pick];
  out.c2 = c2[pick];
  out.normal = nrm[pick];
  out.addable = (hf_is_approx(ntop[pick], nrm[pick]) && (collision || !side[pick])) ? 1u : 0u;
  out.pad = 0;
}
// the request of a leaf's solves: GJKSolver(request) (narrowphase.h:216-246) with compute_penetration = true (:419)
template <typename T>
HFCL_HD QParams<T> hf_leaf_params(QParams<T> q) {
  q.mode = 1;
  q.compute_penetration = 1;
  q.guess_mode = HFCL_GUESS_DEFAULT;
  return q;
}

// ---- the replay of one query ----------------------------------------------------------------------------------------------------
// A listed leaf of a query, in walk order: its node and the minimum of the box bounds met before it
template <typename T>
struct HfItem {
  uint32_t node, query;
  T box_min;
};
// The fold of a query's items in order: updateDistanceLowerBoundFromBV (the minimum logged with each leaf, the tail after the last one),
// the contact decision and updateDistanceLowerBoundFromLeaf of every leaf, the stop at num_max_contacts.  on_contact(k, node, leaf):
// contact k was added.  Writes the record (hppfcl_amd_hfield.h) and the bound; returns numContacts().
template <typename T, class OnContact>
HFCL_HD uint32_t hf_fold(const HfItem<T>* items, const HfLeafOut<T>* leaves, uint64_t n_items, T tail_box_min, T margin, T threshold,
                         uint32_t num_max_contacts, bool swapped, OnContact on_contact, hfcl_result* rec, double* dlb_out) {
  const T nanv = Lim<T>::nan();
  T dlb = Lim<T>::max();
  V3<T> np1 = mk<T>(nanv, nanv, nanv), np2 = np1, nn = np1;
  uint32_t nc = 0;
  int first_node = -1;
  HfLeafOut<T> first;
  first.distance = nanv;
  first.c1 = first.c2 = first.normal = np1;
  bool stopped = false;
  for (uint64_t i = 0; i < n_items; ++i) {
    const HfItem<T> it = items[i];
    const HfLeafOut<T> lf = leaves[i];
    if (!(dlb <= T(0)) && it.box_min < dlb) dlb = it.box_min;
    const T dtc = lf.distance - margin;
    if (dtc <= threshold) {
      if (nc < num_max_contacts && lf.addable) {
        if (nc == 0) {
          first = lf;
          first_node = int(it.node);
        }
        on_contact(nc, it.node, lf);
        ++nc;
      }
    }
    if (dtc < dlb) {
      dlb = dtc;
      np1 = lf.c1;
      np2 = lf.c2;
      nn = lf.normal;
    }
    if (nc >= num_max_contacts) {  // canStop()
      stopped = true;
      break;
    }
  }
  if (!stopped && !(dlb <= T(0)) && tail_box_min < dlb) dlb = tail_box_min;
  if (dlb_out) *dlb_out = double(dlb);
  if (rec) {
    const V3<T> p1 = nc ? first.c1 : np1, p2 = nc ? first.c2 : np2, n = nc ? first.normal : nn;
    const V3<T> a1 = swapped ? p2 : p1, a2 = swapped ? p1 : p2, an = swapped ? -n : n;
    rec->distance = double(nc ? first.distance : dlb);
    rec->normal[0] = an.x; rec->normal[1] = an.y; rec->normal[2] = an.z;
    rec->p1[0] = a1.x; rec->p1[1] = a1.y; rec->p1[2] = a1.z;
    rec->p2[0] = a2.x; rec->p2[1] = a2.y; rec->p2[2] = a2.z;
    rec->b1 = swapped ? -1 : first_node;
    rec->b2 = swapped ? first_node : -1;
    rec->status = (uint32_t(EPA_DID_NOT_RUN) << 3) | (nc ? 128u : 0u) | (swapped ? (1u << 23) : 0u);
    rec->num_contacts = int32_t(nc);
  }
  return nc;
}
template <typename T>
HFCL_HD void hf_fill_contact(hfcl_contact& c, uint32_t pair, uint32_t node, const HfLeafOut<T>& lf, bool swapped) {
  c.pair = pair;
  c.b1 = swapped ? -1 : int32_t(node);
  c.b2 = swapped ? int32_t(node) : -1;
  c._pad = 0;
  c.penetration_depth = double(lf.distance);
  const V3<T> a1 = swapped ? lf.c2 : lf.c1, a2 = swapped ? lf.c1 : lf.c2, an = swapped ? -lf.normal : lf.normal;
  c.normal[0] = an.x; c.normal[1] = an.y; c.normal[2] = an.z;
  c.p1[0] = a1.x; c.p1[1] = a1.y; c.p1[2] = a1.z;
  c.p2[0] = a2.x; c.p2[1] = a2.y; c.p2[2] = a2.z;
}
HFCL_HD void hf_skipped_record(hfcl_result* rec, double* dlb_out, bool swapped) {
  if (rec) {
    rec->distance = 0;
    for (int k = 0; k < 3; ++k) rec->normal[k] = rec->p1[k] = rec->p2[k] = 0;
    rec->b1 = rec->b2 = 0;
    rec->status = 0x80000000u | (swapped ? (1u << 23) : 0u);
    rec->num_contacts = 0;
  }
  if (dlb_out) *dlb_out = Lim<double>::max();
}

// getSupport<WithSweptSphere> of the solid in its own frame from its NoSweptSphere support (hfcl_shapes.hpp: support_with_swept_sphere)
template <typename T, class Solid>
struct HfSweptSupport {
  DShape<T> s;
  const Solid* solid;
  HFCL_HD V3<T> operator()(const V3<T>& dir) const {
    const V3<T> u = normalized(dir);
    if (s.kind == K_SPHERE) return u * (s.p0 + s.ssr);
    return (*solid)(dir) + u * (s.kind == K_CAPSULE ? s.p0 + s.ssr : s.ssr);
  }
};

// a height field registered on a library: where its tables start in the library's arrays
struct DHfield {
  uint64_t node_off, height_off, xg_off, yg_off;
  uint32_t n_nodes, nx, ny, pad;
  double min_height, max_height;
};

// ---- the kernels' parameter block (hfcl_k_hfield.hip) ---------------------------------------------------------------------------
// What a chunk of height-field queries adds to the pipeline's block (hfcl_listed.hpp; tf_c: the fields' poses)
struct HfArgs : ListedArgs {
  uint32_t n_fields;
  const DHfield* fields;
  const hfcl_hfield_node* nodes;
  const double* heights;
  const double* xgrid;
  const double* ygrid;
  const uint32_t* hfield;
  HfItem<double>* items;
  HfLeafOut<double>* leaves;
};

}  // namespace hfcl

#if defined(__HIPCC__)
// Launches of one chunk (hfcl_k_hfield.hip: launch_listed_count / launch_listed_solve of hfcl_listed.hpp for this kind)
void launch_hf_count(hipStream_t st, const hfcl::HfArgs& a);
void launch_hf_solve(hipStream_t st, const hfcl::HfArgs& a, int max_blocks, bool want_contacts, const char** names, hipEvent_t* e0, hipEvent_t* e1);
#endif
