// hfcl_cull.hpp -- culling a scene's pair list per configuration (hfcl_scene_cull*, hfcl_scene_*_listed*, hfcl_scene_*_culled): the
// arithmetic shared by the kernels of hfcl_k_cull.hip, the host broadphase (hfcl_broadphase.cpp) and the host build of the tests
// (tests/cull_harness).  World boxes as CollisionObject::computeAABB makes them (collision_object.h:259-276), the overlap test of
// AABB::overlap on boxes grown as AABB::expand grows them, and the ranges of the fold over a list of surviving queries.
// Every unit that includes this for its boxes is built without contraction of a*b+c: the boxes are the same bits everywhere.
// Builds with hipcc and with g++.
#pragma once
#include "hfcl_scene.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

namespace hfcl {

// ---- world boxes ----------------------------------------------------------------------------------------------------------
// Eigen::isIdentity with its default precision, on the column-major rotation of a pose row
HFCL_HD bool cull_rotation_is_identity(const double* R) {
  const double eps = 1e-12;
  for (int c = 0; c < 3; ++c)
    for (int r = 0; r < 3; ++r) {
      const double x = R[3 * c + r];
      const double ax = habs(x);
      if (r == c ? !(habs(x - 1.0) <= eps * (1.0 < ax ? 1.0 : ax)) : !(ax <= eps)) return false;
    }
  return true;
}
// local box L (min xyz, max xyz) under the pose (R column-major, T) -> world box o: the translation alone under an identity
// rotation, interval arithmetic row by row otherwise.  Unbounded boxes (+-DBL_MAX) go through the same arithmetic.
HFCL_HD void cull_world_box(const double* R, const double* T, const double* L, double* o) {
  if (cull_rotation_is_identity(R)) {
    for (int k = 0; k < 3; ++k) {
      o[k] = L[k] + T[k];
      o[3 + k] = L[3 + k] + T[k];
    }
    return;
  }
  for (int k = 0; k < 3; ++k) {  // interval arithmetic on row k of R
    double lo = 0, hi = 0;
    for (int j = 0; j < 3; ++j) {
      const double a = R[3 * j + k] * L[j], c = R[3 * j + k] * L[3 + j];
      const double mn = c < a ? c : a, mx = c > a ? c : a;
      lo = j ? lo + mn : mn;
      hi = j ? hi + mx : mx;
    }
    o[k] = T[k] + lo;
    o[3 + k] = T[k] + hi;
  }
}
// ... of a 7-float pose row (quaternion w, x, y, z + translation): widened to double, the rotation rebuilt as the compact-pose entry
// points rebuild it (pose_from_quat), then the same arithmetic
HFCL_HD void cull_world_box_quat(const float* p, const double* L, double* o) {
  const Pose<double> q = pose_from_quat<double, float>(p);
  const double R[9] = {q.R.r0.x, q.R.r1.x, q.R.r2.x, q.R.r0.y, q.R.r1.y, q.R.r2.y, q.R.r0.z, q.R.r1.z, q.R.r2.z};
  const double T[3] = {q.t.x, q.t.y, q.t.z};
  cull_world_box(R, T, L, o);
}

// ---- the predicate ----------------------------------------------------------------------------------------------------------
// Do the boxes a and b touch after each was grown by `inflate` on every side (AABB::expand: lo - inflate, hi + inflate)?
// AABB::overlap: closed intervals; a NaN makes every comparison false and keeps the pair.
HFCL_HD bool cull_boxes_touch(const double* a, const double* b) {
  return !(a[0] > b[3] || a[1] > b[4] || a[2] > b[5] || a[3] < b[0] || a[4] < b[1] || a[5] < b[2]);
}
HFCL_HD bool cull_keep(const double* a, const double* b, double inflate) {
  double ga[6], gb[6];
  for (int k = 0; k < 3; ++k) {
    ga[k] = a[k] - inflate;
    ga[3 + k] = a[3 + k] + inflate;
    gb[k] = b[k] - inflate;
    gb[3 + k] = b[3 + k] + inflate;
  }
  return cull_boxes_touch(ga, gb);
}

// ---- the compaction -----------------------------------------------------------------------------------------------------------
// A chunk [q0, q0 + m) of the flat query range is marked by workgroups of CULL_BLOCK lanes, a lane per query: a 64-bit ballot per
// wave, a count per workgroup; the counts are scanned (the running count of the chunks before it added); the survivors are written
// at their ranks.  The list is ascending in q and does not depend on the chunk.
constexpr uint32_t CULL_BLOCK = 256u;
constexpr uint32_t CULL_WAVES = CULL_BLOCK / 64u;
HFCL_HD uint32_t cull_popcount(uint64_t x) { return uint32_t(__builtin_popcountll(x)); }
// survivors of the wave below `lane`
HFCL_HD uint32_t cull_rank(uint64_t ballot, uint32_t lane) { return cull_popcount(ballot & ((uint64_t(1) << lane) - 1u)); }

// ---- the fold over a list ------------------------------------------------------------------------------------------------------
// Configuration c owns the records [begin, end) = conf_begin[c] .. conf_begin[c + 1] of the list, cut at multiples of SCENE_FOLD_SHARE
// from `begin` into at most scene_shares(n_pairs) pieces; piece s, cut to the chunk [k0, k1) of the list: [lo, hi) (hi <= lo: nothing)
// The configurations a chunk of the list spans: those of its first and last id (the list is ascending), the ones without an entry in
// between included -- a chunk of m entries has at most m configurations WITH entries, but may span any number.  Clamped to the call's
// n_conf configurations, so that a list that breaks its contract cannot send the fold past its tables.
HFCL_HD void scene_listed_span(uint64_t id_first, uint64_t id_last, uint32_t n_pairs, uint64_t n_conf, uint64_t& c_lo, uint64_t& count) {
  c_lo = id_first / n_pairs;
  uint64_t c_hi = id_last / n_pairs;
  if (c_hi >= n_conf) c_hi = n_conf - 1u;
  count = c_lo <= c_hi ? c_hi - c_lo + 1u : 0u;
}
HFCL_HD void scene_listed_piece(uint64_t begin, uint64_t end, uint32_t s, uint64_t k0, uint64_t k1, uint64_t& lo, uint64_t& hi) {
  lo = begin + uint64_t(s) * SCENE_FOLD_SHARE;
  hi = lo + SCENE_FOLD_SHARE < end ? lo + SCENE_FOLD_SHARE : end;
  if (lo < k0) lo = k0;
  if (hi > k1) hi = k1;
}

// ---- local boxes (host) ---------------------------------------------------------------------------------------------------------
struct Box3 {
  double lo[3], hi[3];
};
// computeLocalAABB of a shape of the library (src/shape/geometric_shapes.cpp:145-254), the swept-sphere radius included
inline Box3 shape_local_box(const hfcl_shape& s, const double* verts) {
  Box3 b;
  auto symmetric = [&b](double hx, double hy, double hz) {
    const double h[3] = {hx, hy, hz};
    for (int k = 0; k < 3; ++k) {
      b.lo[k] = -h[k];
      b.hi[k] = h[k];
    }
  };
  switch (s.type) {
    case HFCL_GEOM_HALFSPACE:
    case HFCL_GEOM_PLANE: {
      // computeBV<AABB, Halfspace|Plane> in the shape's own frame (geometric_shapes_utility.cpp:391-455): the volume
      // is unbounded (+-DBL_MAX) except along a coordinate axis the normal is aligned with
      const double big = std::numeric_limits<double>::max();
      for (int k = 0; k < 3; ++k) {
        b.lo[k] = -big;
        b.hi[k] = big;
      }
      const double* n = s.params;
      const int axis = (n[1] == 0.0 && n[2] == 0.0) ? 0 : (n[0] == 0.0 && n[2] == 0.0) ? 1 : (n[0] == 0.0 && n[1] == 0.0) ? 2 : -1;
      if (axis >= 0 && n[axis] != 0.0) {
        const double v = n[axis] < 0 ? -s.params[3] : s.params[3];
        if (s.type == HFCL_GEOM_PLANE) b.lo[axis] = b.hi[axis] = v;
        else if (n[axis] < 0) b.lo[axis] = v;
        else b.hi[axis] = v;
      }
      break;
    }
    case HFCL_GEOM_BOX:
    case HFCL_GEOM_ELLIPSOID: symmetric(s.params[0], s.params[1], s.params[2]); break;
    case HFCL_GEOM_SPHERE: symmetric(s.params[0], s.params[0], s.params[0]); break;
    case HFCL_GEOM_CAPSULE: symmetric(s.params[0], s.params[0], s.params[1] + s.params[0]); break;
    case HFCL_GEOM_CONE:
    case HFCL_GEOM_CYLINDER: symmetric(std::abs(s.params[0]), std::abs(s.params[0]), std::abs(s.params[1])); break;
    default: {  // point sets: Convex, Triangle
      const double big = std::numeric_limits<double>::max();
      for (int k = 0; k < 3; ++k) {
        b.lo[k] = big;
        b.hi[k] = -big;
      }
      const double* p = verts + 3 * size_t(s.vertex_offset);
      for (uint32_t i = 0; i < s.num_points; ++i, p += 3)
        for (int k = 0; k < 3; ++k) {
          b.lo[k] = std::min(b.lo[k], p[k]);
          b.hi[k] = std::max(b.hi[k], p[k]);
        }
    }
  }
  if (s.swept_sphere_radius > 0)
    for (int k = 0; k < 3; ++k) {
      b.lo[k] -= s.swept_sphere_radius;
      b.hi[k] += s.swept_sphere_radius;
    }
  return b;
}
// BVHModelBase::computeLocalAABB (src/BVH/BVH_model.cpp): the box of the model's vertices in the model frame
inline Box3 mesh_local_box(const double* verts, size_t n_vertices) {
  Box3 b;
  const double big = std::numeric_limits<double>::max();
  for (int k = 0; k < 3; ++k) {
    b.lo[k] = big;
    b.hi[k] = -big;
  }
  for (size_t i = 0; i < n_vertices; ++i)
    for (int k = 0; k < 3; ++k) {
      b.lo[k] = std::min(b.lo[k], verts[3 * i + k]);
      b.hi[k] = std::max(b.hi[k], verts[3 * i + k]);
    }
  return b;
}

}  // namespace hfcl
