// hppfcl_amd_compat.hpp -- header-only C++ shim exposing the C ABI (hppfcl_amd.h) under the
// reference's own names so hpp-fcl user code for the narrow-phase path recompiles against it.
//
// Mirrors (same names, argument meaning, defaults and error behaviour):
//   Transform3f                 include/hpp/fcl/math/transform.h:56-218
//   CollisionGeometry/ShapeBase include/hpp/fcl/collision_object.h:94-190, shape/geometric_shapes.h:59-102
//   Box, Sphere, Capsule, Ellipsoid, ConvexBase   shape/geometric_shapes.h:164-187,238-251,381-400,303-320,638-872
//   QueryRequest, CollisionRequest, DistanceRequest, Contact, CollisionResult, DistanceResult
//                               include/hpp/fcl/collision_data.h:59-166,171-273,312-383,391-494,987-1174
//   collide(), distance()       include/hpp/fcl/collision.h:58-70, distance.h:53-65 (src/collision.cpp:69-130,
//                               src/distance.cpp:60-109); std::invalid_argument for num_max_contacts == 0 and for
//                               unsupported node-type pairs, exactly where the reference throws.
//   CollisionCallBackCollect-style batching: amd::BatchQueries (default_broadphase_callbacks.h:224-252)
//
// No Eigen: Vec3f / Matrix3f are minimal PODs with the same memory image as the Eigen types the
// reference uses (Matrix3f column-major), so `Transform3f` is bit-compatible with the ABI pose.
// There is no CPU fallback: every query runs on the GPU through libhppfcl_amd.so.
#pragma once
#include <array>
#include <cmath>
#include <cstddef>
#include <limits>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <typeinfo>
#include <type_traits>
#include <vector>

#include <algorithm>
#include <cstring>

#include "hppfcl_amd.h"

namespace hpp {
namespace fcl {

typedef double FCL_REAL;

struct Vec3f {
  FCL_REAL v[3];
  Vec3f() : v{0, 0, 0} {}
  Vec3f(FCL_REAL x, FCL_REAL y, FCL_REAL z) : v{x, y, z} {}
  FCL_REAL& operator[](int i) { return v[i]; }
  const FCL_REAL& operator[](int i) const { return v[i]; }
  const FCL_REAL* data() const { return v; }
  static Vec3f Constant(FCL_REAL c) { return Vec3f(c, c, c); }
  static Vec3f Zero() { return Vec3f(0, 0, 0); }
  Vec3f operator+(const Vec3f& o) const { return Vec3f(v[0] + o.v[0], v[1] + o.v[1], v[2] + o.v[2]); }
  Vec3f operator-(const Vec3f& o) const { return Vec3f(v[0] - o.v[0], v[1] - o.v[1], v[2] - o.v[2]); }
  Vec3f operator*(FCL_REAL s) const { return Vec3f(v[0] * s, v[1] * s, v[2] * s); }
  Vec3f operator/(FCL_REAL s) const { return Vec3f(v[0] / s, v[1] / s, v[2] / s); }
  Vec3f operator-() const { return Vec3f(-v[0], -v[1], -v[2]); }
  FCL_REAL dot(const Vec3f& o) const { return v[0] * o.v[0] + v[1] * o.v[1] + v[2] * o.v[2]; }
  FCL_REAL norm() const { return std::sqrt(dot(*this)); }
};

struct Matrix3f {  // column-major, like Eigen::Matrix<double,3,3>
  FCL_REAL m[9];
  Matrix3f() { setIdentity(); }
  void setIdentity() {
    for (int i = 0; i < 9; ++i) m[i] = (i % 4 == 0) ? 1.0 : 0.0;
  }
  static Matrix3f Identity() { return Matrix3f(); }
  FCL_REAL& operator()(int r, int c) { return m[c * 3 + r]; }
  const FCL_REAL& operator()(int r, int c) const { return m[c * 3 + r]; }
  Vec3f operator*(const Vec3f& x) const {
    return Vec3f((*this)(0, 0) * x[0] + (*this)(0, 1) * x[1] + (*this)(0, 2) * x[2],
                 (*this)(1, 0) * x[0] + (*this)(1, 1) * x[1] + (*this)(1, 2) * x[2],
                 (*this)(2, 0) * x[0] + (*this)(2, 1) * x[1] + (*this)(2, 2) * x[2]);
  }
  Matrix3f operator*(const Matrix3f& o) const {
    Matrix3f r;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) r(i, j) = (*this)(i, 0) * o(0, j) + (*this)(i, 1) * o(1, j) + (*this)(i, 2) * o(2, j);
    return r;
  }
};

struct Quatf {  // makeQuat(w, x, y, z)
  FCL_REAL w, x, y, z;
  Matrix3f toRotationMatrix() const {  // Eigen::Quaternion::toRotationMatrix
    Matrix3f R;
    const FCL_REAL tx = 2 * x, ty = 2 * y, tz = 2 * z, twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x,
                   txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R(0, 0) = 1 - (tyy + tzz); R(0, 1) = txy - twz; R(0, 2) = txz + twy;
    R(1, 0) = txy + twz; R(1, 1) = 1 - (txx + tzz); R(1, 2) = tyz - twx;
    R(2, 0) = txz - twy; R(2, 1) = tyz + twx; R(2, 2) = 1 - (txx + tyy);
    return R;
  }
};
inline Quatf makeQuat(FCL_REAL w, FCL_REAL x, FCL_REAL y, FCL_REAL z) { return Quatf{w, x, y, z}; }

class Transform3f {
  Matrix3f R;
  Vec3f T;

 public:
  Transform3f() {}
  Transform3f(const Matrix3f& R_, const Vec3f& T_) : R(R_), T(T_) {}
  Transform3f(const Quatf& q, const Vec3f& T_) : R(q.toRotationMatrix()), T(T_) {}
  explicit Transform3f(const Matrix3f& R_) : R(R_) {}
  explicit Transform3f(const Quatf& q) : R(q.toRotationMatrix()) {}
  explicit Transform3f(const Vec3f& T_) : T(T_) {}
  static Transform3f Identity() { return Transform3f(); }
  const Vec3f& getTranslation() const { return T; }
  const Matrix3f& getRotation() const { return R; }
  void setTranslation(const Vec3f& t) { T = t; }
  void setRotation(const Matrix3f& r) { R = r; }
  void setQuatRotation(const Quatf& q) { R = q.toRotationMatrix(); }
  Vec3f transform(const Vec3f& x) const { return R * x + T; }
  Transform3f operator*(const Transform3f& o) const { return Transform3f(R * o.R, R * o.T + T); }
};
static_assert(sizeof(Transform3f) == HFCL_POSE_DOUBLES * sizeof(double), "Transform3f must be the ABI pose image");

enum NODE_TYPE {  // include/hpp/fcl/collision_object.h:65-89 (subset in scope)
  BV_OBBRSS = HFCL_BV_OBBRSS, GEOM_BOX = HFCL_GEOM_BOX, GEOM_SPHERE = HFCL_GEOM_SPHERE, GEOM_CAPSULE = HFCL_GEOM_CAPSULE,
  GEOM_CONE = HFCL_GEOM_CONE, GEOM_CYLINDER = HFCL_GEOM_CYLINDER, GEOM_PLANE = HFCL_GEOM_PLANE,
  GEOM_HALFSPACE = HFCL_GEOM_HALFSPACE,
  GEOM_CONVEX = HFCL_GEOM_CONVEX, GEOM_TRIANGLE = HFCL_GEOM_TRIANGLE, GEOM_ELLIPSOID = HFCL_GEOM_ELLIPSOID,
  HF_AABB = 20, HF_OBBRSS = 21,  // height fields: HF_AABB has collide() against the convex solids (hppfcl_amd_hfield.h)
  GEOM_OCTREE = 18               // an occupancy octree: collide() against the convex solids (hppfcl_amd_octree.h)
};
enum GJKInitialGuess { DefaultGuess, CachedGuess, BoundingVolumeGuess };
enum GJKVariant { DefaultGJK, PolyakAcceleration, NesterovAcceleration };
enum GJKConvergenceCriterion { Default, DualityGap, Hybrid };
enum GJKConvergenceCriterionType { Relative, Absolute };
typedef std::array<int, 2> support_func_guess_t;

class CollisionGeometry {
 public:
  virtual ~CollisionGeometry() {}
  virtual NODE_TYPE getNodeType() const = 0;
};
class ShapeBase : public CollisionGeometry {
 public:
  void setSweptSphereRadius(FCL_REAL r) {
    if (r < 0) throw std::invalid_argument("Swept-sphere radius must be positive.");
    m_swept_sphere_radius = r;
  }
  FCL_REAL getSweptSphereRadius() const { return m_swept_sphere_radius; }

 protected:
  FCL_REAL m_swept_sphere_radius = 0;
};
class Box : public ShapeBase {
 public:
  Box(FCL_REAL x, FCL_REAL y, FCL_REAL z) : halfSide(x / 2, y / 2, z / 2) {}
  explicit Box(const Vec3f& side) : halfSide(side * 0.5) {}
  Vec3f halfSide;
  NODE_TYPE getNodeType() const override { return GEOM_BOX; }
};
class Sphere : public ShapeBase {
 public:
  explicit Sphere(FCL_REAL r) : radius(r) {}
  FCL_REAL radius;
  NODE_TYPE getNodeType() const override { return GEOM_SPHERE; }
};
class Capsule : public ShapeBase {
 public:
  Capsule(FCL_REAL r, FCL_REAL lz) : radius(r), halfLength(lz / 2) {}
  FCL_REAL radius, halfLength;
  NODE_TYPE getNodeType() const override { return GEOM_CAPSULE; }
};
class Cone : public ShapeBase {
 public:
  Cone(FCL_REAL r, FCL_REAL lz) : radius(r), halfLength(lz / 2) {}
  FCL_REAL radius, halfLength;
  NODE_TYPE getNodeType() const override { return GEOM_CONE; }
};
class Cylinder : public ShapeBase {
 public:
  Cylinder(FCL_REAL r, FCL_REAL lz) : radius(r), halfLength(lz / 2) {}
  FCL_REAL radius, halfLength;
  NODE_TYPE getNodeType() const override { return GEOM_CYLINDER; }
};
class Halfspace : public ShapeBase {  // {x : n.x <= d}, geometric_shapes.h:873-962
 public:
  Halfspace(const Vec3f& n_, FCL_REAL d_) : n(n_), d(d_) { unitNormalTest(); }
  Halfspace(FCL_REAL a, FCL_REAL b, FCL_REAL c, FCL_REAL d_) : n(a, b, c), d(d_) { unitNormalTest(); }
  Halfspace() : n(1, 0, 0), d(0) {}
  Vec3f n;
  FCL_REAL d;
  FCL_REAL signedDistance(const Vec3f& p) const { return n.dot(p) - (d + getSweptSphereRadius()); }
  NODE_TYPE getNodeType() const override { return GEOM_HALFSPACE; }

 private:
  void unitNormalTest() {  // geometric_shapes.cpp:121-131
    const FCL_REAL l = n.norm();
    if (l > 0) { n = n * (1.0 / l); d *= 1.0 / l; } else { n = Vec3f(1, 0, 0); d = 0; }
  }
};
class Plane : public ShapeBase {  // {x : n.x = d}, geometric_shapes.h:968-1049
 public:
  Plane(const Vec3f& n_, FCL_REAL d_) : n(n_), d(d_) { unitNormalTest(); }
  Plane(FCL_REAL a, FCL_REAL b, FCL_REAL c, FCL_REAL d_) : n(a, b, c), d(d_) { unitNormalTest(); }
  Plane() : n(1, 0, 0), d(0) {}
  Vec3f n;
  FCL_REAL d;
  NODE_TYPE getNodeType() const override { return GEOM_PLANE; }

 private:
  void unitNormalTest() {  // geometric_shapes.cpp:133-143
    const FCL_REAL l = n.norm();
    if (l > 0) { n = n * (1.0 / l); d *= 1.0 / l; } else { n = Vec3f(1, 0, 0); d = 0; }
  }
};
class Ellipsoid : public ShapeBase {
 public:
  Ellipsoid(FCL_REAL rx, FCL_REAL ry, FCL_REAL rz) : radii(rx, ry, rz) {}
  Vec3f radii;
  NODE_TYPE getNodeType() const override { return GEOM_ELLIPSOID; }
};
class ConvexBase : public ShapeBase {
 public:
  explicit ConvexBase(std::shared_ptr<std::vector<Vec3f>> pts) : points(std::move(pts)) {
    num_points = static_cast<unsigned int>(points->size());
  }
  std::shared_ptr<std::vector<Vec3f>> points;
  unsigned int num_points;
  /// ConvexBase::neighbors (geometric_shapes.h: per vertex the vertices it shares a facet edge with), kept as CSR:
  /// neighbor_offsets[num_points + 1] into neighbor_ids.  Empty: none known (Convex<PolygonT> fills them).  The engine
  /// climbs them for hulls of HFCL_CLIMB_MIN vertices and more (hfcl_lib_set_convex_neighbors).
  std::vector<uint32_t> neighbor_offsets, neighbor_ids;
  NODE_TYPE getNodeType() const override { return GEOM_CONVEX; }
};

class TriangleP : public ShapeBase {  // geometric_shapes.h:98-134
 public:
  TriangleP(const Vec3f& a_, const Vec3f& b_, const Vec3f& c_) : a(a_), b(b_), c(c_) {}
  Vec3f a, b, c;
  NODE_TYPE getNodeType() const override { return GEOM_TRIANGLE; }
};

struct Triangle {  // include/hpp/fcl/data_types.h:101-144
  typedef std::size_t index_type;
  Triangle() : vids{0, 0, 0} {}
  Triangle(index_type a, index_type b, index_type c) : vids{a, b, c} {}
  index_type operator[](index_type i) const { return vids[i]; }
  index_type& operator[](index_type i) { return vids[i]; }
  index_type vids[3];
};
/// Convex<PolygonT> (include/hpp/fcl/shape/convex.h:49-105): a convex polytope given by its vertices and facets; the
/// constructor derives the vertex adjacency from the facets (fillNeighbors, shape/details/convex.hxx:231-280: the
/// ascending set of the two facet-cycle neighbours of every vertex over all facets).
template <typename PolygonT>
class Convex : public ConvexBase {
 public:
  Convex(std::shared_ptr<std::vector<Vec3f>> points_, unsigned int num_points_, std::shared_ptr<std::vector<PolygonT>> polygons_,
         unsigned int num_polygons_)
      : ConvexBase(std::move(points_)), polygons(std::move(polygons_)), num_polygons(num_polygons_) {
    if (num_points_ < num_points) num_points = num_points_;
    fillNeighbors();
  }
  std::shared_ptr<std::vector<PolygonT>> polygons;
  unsigned int num_polygons;

 protected:
  void fillNeighbors() {
    std::vector<std::vector<uint32_t>> nb(num_points);
    if (!polygons) return;
    for (unsigned int l = 0; l < num_polygons && l < polygons->size(); ++l) {
      const PolygonT& poly = (*polygons)[l];
      const std::size_t n = poly_size(poly);
      for (std::size_t j = 0; j < n; ++j) {
        const std::size_t pi = poly[static_cast<typename PolygonT::index_type>(j == 0 ? n - 1 : j - 1)], pj = poly[static_cast<typename PolygonT::index_type>(j)],
                          pk = poly[static_cast<typename PolygonT::index_type>(j == n - 1 ? 0 : j + 1)];
        if (pj >= num_points || pi >= num_points || pk >= num_points) throw std::invalid_argument("Convex: polygon vertex index out of range");
        nb[pj].push_back(static_cast<uint32_t>(pi));
        nb[pj].push_back(static_cast<uint32_t>(pk));
      }
    }
    neighbor_offsets.assign(num_points + 1, 0);
    neighbor_ids.clear();
    for (unsigned int i = 0; i < num_points; ++i) {
      std::sort(nb[i].begin(), nb[i].end());
      nb[i].erase(std::unique(nb[i].begin(), nb[i].end()), nb[i].end());
      neighbor_ids.insert(neighbor_ids.end(), nb[i].begin(), nb[i].end());
      neighbor_offsets[i + 1] = static_cast<uint32_t>(neighbor_ids.size());
    }
  }
  static std::size_t poly_size(const Triangle&) { return 3; }
  template <typename P>
  static std::size_t poly_size(const P& p) { return p.size(); }
};

struct OBBRSS {};  // tag: the one BV type in scope (include/hpp/fcl/BV/OBBRSS.h)
enum BVHReturnCode { BVH_OK = 0, BVH_ERR_BUILD_OUT_OF_SEQUENCE = -2, BVH_ERR_BUILD_EMPTY_MODEL = -3 };

/// BVHModel<OBBRSS> (include/hpp/fcl/BVH/BVH_model.h:61-368): triangle soup assembled with
/// beginModel / addVertex / addTriangle / addSubModel / endModel; endModel() builds the tree on the
/// host (hfcl_bvh_build, the reference's SPLIT_METHOD_MEAN construction).
template <typename BV>
class BVHModel : public CollisionGeometry {
 public:
  std::vector<Vec3f> vertices;
  std::vector<Triangle> tri_indices;
  unsigned int num_tris = 0, num_vertices = 0;

  NODE_TYPE getNodeType() const override { return BV_OBBRSS; }
  int beginModel(unsigned int = 0, unsigned int = 0) {  // BVH_model.cpp:264-306
    vertices.clear();
    tri_indices.clear();
    nodes_.clear();
    building_ = true;
    return BVH_OK;
  }
  int addVertex(const Vec3f& p) {
    if (!building_) return BVH_ERR_BUILD_OUT_OF_SEQUENCE;
    vertices.push_back(p);
    return BVH_OK;
  }
  int addTriangle(const Vec3f& p1, const Vec3f& p2, const Vec3f& p3) {  // BVH_model.cpp:385-438
    if (!building_) return BVH_ERR_BUILD_OUT_OF_SEQUENCE;
    const std::size_t o = vertices.size();
    vertices.push_back(p1);
    vertices.push_back(p2);
    vertices.push_back(p3);
    tri_indices.emplace_back(o, o + 1, o + 2);
    return BVH_OK;
  }
  int addSubModel(const std::vector<Vec3f>& ps, const std::vector<Triangle>& ts) {  // BVH_model.cpp:440-506
    if (!building_) return BVH_ERR_BUILD_OUT_OF_SEQUENCE;
    const std::size_t o = vertices.size();
    vertices.insert(vertices.end(), ps.begin(), ps.end());
    for (const Triangle& t : ts) tri_indices.emplace_back(t[0] + o, t[1] + o, t[2] + o);
    return BVH_OK;
  }
  int endModel() {  // BVH_model.cpp:508-576
    if (!building_) return BVH_ERR_BUILD_OUT_OF_SEQUENCE;
    if (tri_indices.empty() || vertices.empty()) return BVH_ERR_BUILD_EMPTY_MODEL;
    num_tris = static_cast<unsigned int>(tri_indices.size());
    num_vertices = static_cast<unsigned int>(vertices.size());
    flat_tris_.resize(3 * tri_indices.size());
    for (std::size_t i = 0; i < tri_indices.size(); ++i)
      for (int k = 0; k < 3; ++k) flat_tris_[3 * i + k] = static_cast<uint32_t>(tri_indices[i][k]);
    nodes_.resize(2 * tri_indices.size() - 1);
    primitive_indices_.resize(tri_indices.size());
    const int rc = hfcl_bvh_build(reinterpret_cast<const double*>(vertices.data()), vertices.size(), flat_tris_.data(),
                                  tri_indices.size(), nodes_.data(), primitive_indices_.data(), 0);
    if (rc) throw std::invalid_argument(hfcl_last_error());
    building_ = false;
    return BVH_OK;
  }
  unsigned int getNumBVs() const { return static_cast<unsigned int>(nodes_.size()); }
  const hfcl_bvh_node& getBV(unsigned int i) const { return nodes_[i]; }
  const std::vector<hfcl_bvh_node>& nodes() const { return nodes_; }
  const std::vector<uint32_t>& flatTriangles() const { return flat_tris_; }

 private:
  bool building_ = false;
  std::vector<hfcl_bvh_node> nodes_;
  std::vector<uint32_t> flat_tris_, primitive_indices_;
};

struct AABB {
  Vec3f min_, max_;
  bool overlap(const AABB& o) const {  // BV/AABB.h:112-122
    for (int k = 0; k < 3; ++k)
      if (min_[k] > o.max_[k] || max_[k] < o.min_[k]) return false;
    return true;
  }
};

/// The two Eigen types HeightField's interface names, as far as it uses them: a dense matrix of heights (rows = y, north edge first)
/// and a vector.
struct MatrixXf {
  MatrixXf() {}
  MatrixXf(std::size_t rows, std::size_t cols) : rows_(rows), cols_(cols), v_(rows * cols, 0.0) {}
  static MatrixXf Constant(std::size_t rows, std::size_t cols, FCL_REAL c) {
    MatrixXf m(rows, cols);
    m.fill(c);
    return m;
  }
  static MatrixXf Ones(std::size_t rows, std::size_t cols) { return Constant(rows, cols, 1.0); }
  void fill(FCL_REAL c) { std::fill(v_.begin(), v_.end(), c); }
  std::size_t rows() const { return rows_; }
  std::size_t cols() const { return cols_; }
  FCL_REAL& operator()(std::size_t r, std::size_t c) { return v_[r * cols_ + c]; }
  const FCL_REAL& operator()(std::size_t r, std::size_t c) const { return v_[r * cols_ + c]; }
  FCL_REAL maxCoeff() const { return *std::max_element(v_.begin(), v_.end()); }
  const FCL_REAL* data() const { return v_.data(); }  // row-major

 private:
  std::size_t rows_ = 0, cols_ = 0;
  std::vector<FCL_REAL> v_;
};
typedef std::vector<FCL_REAL> VecXf;

/// HeightField<AABB> (include/hpp/fcl/hfield.h:202-520): x_dim by y_dim, centred at the origin, heights(row, col) over
/// x_grid = LinSpaced(cols, -x_dim/2, x_dim/2) and y_grid = LinSpaced(rows, y_dim/2, -y_dim/2), solid down to min_height.  The tree is
/// built on the host (hfcl_hfield_build, the reference's numbering); collide() against a convex solid, in either operand order, goes to
/// hfcl_hfield_collide_batch.  Only BV = AABB has collide() here.
template <typename BV>
class HeightField : public CollisionGeometry {
  static_assert(std::is_same<BV, AABB>::value, "only HeightField<AABB> is built (HeightField<OBBRSS>: not done)");

 public:
  typedef hfcl_hfield_node Node;
  typedef std::vector<Node> BVS;
  HeightField(FCL_REAL x_dim, FCL_REAL y_dim, const MatrixXf& heights, FCL_REAL min_height = 0) : x_dim_(x_dim), y_dim_(y_dim), min_height_(min_height) {
    init(heights);
  }
  NODE_TYPE getNodeType() const override { return HF_AABB; }
  const VecXf& getXGrid() const { return x_grid_; }
  const VecXf& getYGrid() const { return y_grid_; }
  const MatrixXf& getHeights() const { return heights_; }
  FCL_REAL getXDim() const { return x_dim_; }
  FCL_REAL getYDim() const { return y_dim_; }
  FCL_REAL getMinHeight() const { return min_height_; }
  FCL_REAL getMaxHeight() const { return max_height_; }
  const BVS& getNodes() const { return bvs_; }
  const Node& getBV(unsigned int i) const {
    if (i >= bvs_.size()) throw std::invalid_argument("Index out of bounds");
    return bvs_[i];
  }
  void computeLocalAABB() {  // hfield.h:278-287
    const Vec3f A(x_grid_.front(), y_grid_.front(), min_height_), B(x_grid_.back(), y_grid_.back(), max_height_);
    for (int k = 0; k < 3; ++k) {
      aabb_local.min_[k] = std::min(A[k], B[k]);
      aabb_local.max_[k] = std::max(A[k], B[k]);
    }
    aabb_radius = (A - B).norm() / 2.;
    aabb_center = (aabb_local.min_ + aabb_local.max_) * 0.5;
  }
  void updateHeights(const MatrixXf& new_heights) {  // hfield.h:290-305: the tree is rebuilt, the next collide() uploads it again
    if (new_heights.rows() != heights_.rows() || new_heights.cols() != heights_.cols())
      throw std::invalid_argument("The matrix containing the new heights values does not have the same matrix size as the original one.");
    init(new_heights);
  }
  unsigned int version() const { return version_; }  // counts init / updateHeights: what a context has registered is this version
  AABB aabb_local;
  FCL_REAL aabb_radius = 0;
  Vec3f aabb_center;

 private:
  void init(const MatrixXf& heights) {
    std::size_t n = 0;
    int rc = hfcl_hfield_build(x_dim_, y_dim_, heights.data(), heights.rows(), heights.cols(), min_height_, nullptr, &n, nullptr, nullptr);
    if (rc) throw std::invalid_argument(hfcl_last_error());
    bvs_.resize(n);
    x_grid_.resize(heights.cols());
    y_grid_.resize(heights.rows());
    rc = hfcl_hfield_build(x_dim_, y_dim_, heights.data(), heights.rows(), heights.cols(), min_height_, bvs_.data(), &n, x_grid_.data(), y_grid_.data());
    if (rc) throw std::invalid_argument(hfcl_last_error());
    heights_ = heights;
    for (std::size_t r = 0; r < heights_.rows(); ++r)
      for (std::size_t c = 0; c < heights_.cols(); ++c) heights_(r, c) = std::max(heights_(r, c), min_height_);  // cwiseMax(min_height)
    max_height_ = bvs_[0].max_height;
    ++version_;
  }
  FCL_REAL x_dim_, y_dim_, min_height_, max_height_ = 0;
  MatrixXf heights_;
  VecXf x_grid_, y_grid_;
  BVS bvs_;
  unsigned int version_ = 0;
};

/// OcTree (include/hpp/fcl/octree.h:53-296) over a node array instead of an octomap tree: node 0 is the root, child[i] the index of
/// child i (0: none).  Every box is halved down from getRootBV, as the reference computes them.  collide() against a convex solid, in
/// either operand order, goes to hfcl_octree_collide_batch and returns the octree-first result (the reference does not swap it back).
class OcTree : public CollisionGeometry {
 public:
  typedef hfcl_octree_node OcTreeNode;
  typedef std::array<FCL_REAL, 6> Vec6f;
  OcTree(const std::vector<OcTreeNode>& nodes, FCL_REAL resolution, unsigned int depth = HFCL_OCTREE_MAX_DEPTH)
      : nodes_(nodes), resolution_(resolution), depth_(depth) {
    if (hfcl_octree_validate(nodes_.data(), nodes_.size(), depth_)) throw std::invalid_argument(hfcl_last_error());
    if (!(resolution_ > 0)) throw std::invalid_argument("OcTree: the resolution must be positive");
  }
  NODE_TYPE getNodeType() const override { return GEOM_OCTREE; }
  unsigned int getTreeDepth() const { return depth_; }
  FCL_REAL getResolution() const { return resolution_; }
  unsigned long size() const { return nodes_.size(); }
  const std::vector<OcTreeNode>& getNodes() const { return nodes_; }
  AABB getRootBV() const {  // octree.h:139-144
    const FCL_REAL delta = (1 << depth_) * resolution_ / 2;
    AABB bv;
    bv.min_ = Vec3f(-delta, -delta, -delta);
    bv.max_ = Vec3f(delta, delta, delta);
    return bv;
  }
  FCL_REAL getOccupancyThres() const { return occupancy_threshold_; }
  FCL_REAL getFreeThres() const { return free_threshold_; }
  void setOccupancyThres(FCL_REAL d) { occupancy_threshold_ = d; }
  void setFreeThres(FCL_REAL d) { free_threshold_ = d; }
  bool isNodeOccupied(const OcTreeNode* n) const { return n->occupancy >= occupancy_threshold_; }
  bool isNodeFree(const OcTreeNode* n) const { return n->occupancy <= free_threshold_; }
  bool isNodeUncertain(const OcTreeNode* n) const { return !isNodeOccupied(n) && !isNodeFree(n); }
  /// toBoxes (octree.h:178-200): (x, y, z, size, occupancy, threshold) of the occupied leaves, depth-first with the children in index
  /// order, centre and size from the halved boxes
  std::vector<Vec6f> toBoxes() const {
    std::vector<Vec6f> boxes;
    if (!nodes_.empty()) to_boxes(0, getRootBV(), boxes);
    return boxes;
  }

 private:
  void to_boxes(uint32_t i, const AABB& bv, std::vector<Vec6f>& out) const {  // (at most depth + 1 levels: the validator's)
    const OcTreeNode& n = nodes_[i];
    bool leaf = true;
    for (unsigned int k = 0; k < 8; ++k) {
      if (!n.child[k]) continue;
      leaf = false;
      AABB c = bv;
      for (int a = 0; a < 3; ++a) {  // computeChildBV, octree.h:299-324
        if (k & (1u << a)) c.min_[a] = (bv.min_[a] + bv.max_[a]) * 0.5;
        else c.max_[a] = (bv.min_[a] + bv.max_[a]) * 0.5;
      }
      to_boxes(n.child[k], c, out);
    }
    if (leaf && isNodeOccupied(&n))
      out.push_back({{(bv.min_[0] + bv.max_[0]) * 0.5, (bv.min_[1] + bv.max_[1]) * 0.5, (bv.min_[2] + bv.max_[2]) * 0.5, bv.max_[0] - bv.min_[0],
                      n.occupancy, occupancy_threshold_}});
  }
  std::vector<OcTreeNode> nodes_;
  FCL_REAL resolution_;
  unsigned int depth_;
  FCL_REAL occupancy_threshold_ = 0.5, free_threshold_ = 0;
};
/// makeOctree (src/octree.cpp:188-202) without octomap: points as x y z triples; hfcl_octree_from_points at octomap's depth of 16
inline std::shared_ptr<OcTree> makeOctree(const std::vector<Vec3f>& point_cloud, FCL_REAL resolution) {
  static_assert(sizeof(Vec3f) == 3 * sizeof(double), "Vec3f must be three doubles");
  std::size_t n = 0;
  const double* xyz = point_cloud.empty() ? nullptr : reinterpret_cast<const double*>(point_cloud.data());
  if (hfcl_octree_from_points(xyz, point_cloud.size(), resolution, HFCL_OCTREE_MAX_DEPTH, nullptr, 0, &n)) throw std::invalid_argument(hfcl_last_error());
  std::vector<hfcl_octree_node> nodes(n);
  if (n && hfcl_octree_from_points(xyz, point_cloud.size(), resolution, HFCL_OCTREE_MAX_DEPTH, nodes.data(), n, &n))
    throw std::invalid_argument(hfcl_last_error());
  return std::make_shared<OcTree>(nodes, resolution, HFCL_OCTREE_MAX_DEPTH);
}

struct QueryRequest {
  GJKInitialGuess gjk_initial_guess = DefaultGuess;
  mutable Vec3f cached_gjk_guess = Vec3f(1, 0, 0);
  mutable support_func_guess_t cached_support_func_guess = {{0, 0}};
  size_t gjk_max_iterations = 128;
  FCL_REAL gjk_tolerance = 1e-6;
  GJKVariant gjk_variant = DefaultGJK;
  GJKConvergenceCriterion gjk_convergence_criterion = Default;
  GJKConvergenceCriterionType gjk_convergence_criterion_type = Relative;
  size_t epa_max_iterations = 64;
  FCL_REAL epa_tolerance = 1e-6;
  bool enable_timings = false;
  FCL_REAL collision_distance_threshold = 1e-12;
};
struct CollisionRequest : QueryRequest {
  size_t num_max_contacts = 1;
  bool enable_contact = true;
  FCL_REAL security_margin = 0;
  FCL_REAL break_distance = 1e-3;
  FCL_REAL distance_upper_bound = (std::numeric_limits<FCL_REAL>::max)();
};
struct DistanceRequest : QueryRequest {
  bool enable_nearest_points = true;
  bool enable_signed_distance = true;
  FCL_REAL rel_err = 0, abs_err = 0;
  DistanceRequest(bool enable_nearest_points_ = true, bool enable_signed_distance_ = true, FCL_REAL rel_err_ = 0,
                  FCL_REAL abs_err_ = 0)
      : enable_nearest_points(enable_nearest_points_), enable_signed_distance(enable_signed_distance_),
        rel_err(rel_err_), abs_err(abs_err_) {}
};

struct Contact {
  const CollisionGeometry* o1 = nullptr;
  const CollisionGeometry* o2 = nullptr;
  int b1 = -1, b2 = -1;
  Vec3f normal;
  std::array<Vec3f, 2> nearest_points;
  Vec3f pos;
  FCL_REAL penetration_depth = (std::numeric_limits<FCL_REAL>::max)();
  static const int NONE = -1;
};

struct QueryResult {
  Vec3f cached_gjk_guess;
  support_func_guess_t cached_support_func_guess = {{-1, -1}};
};
struct CollisionResult : QueryResult {
  FCL_REAL distance_lower_bound = (std::numeric_limits<FCL_REAL>::max)();
  Vec3f normal = Vec3f::Constant(std::numeric_limits<FCL_REAL>::quiet_NaN());
  std::array<Vec3f, 2> nearest_points = {{normal, normal}};
  bool isCollision() const { return !contacts.empty(); }
  size_t numContacts() const { return contacts.size(); }
  const Contact& getContact(size_t i) const {
    if (contacts.empty()) throw std::invalid_argument("The number of contacts is zero. No Contact can be returned.");
    return contacts[i < contacts.size() ? i : contacts.size() - 1];
  }
  void addContact(const Contact& c) { contacts.push_back(c); }
  void clear() { *this = CollisionResult(); }

 private:
  std::vector<Contact> contacts;
};
struct DistanceResult : QueryResult {
  FCL_REAL min_distance = (std::numeric_limits<FCL_REAL>::max)();
  Vec3f normal = Vec3f::Constant(std::numeric_limits<FCL_REAL>::quiet_NaN());
  std::array<Vec3f, 2> nearest_points = {{normal, normal}};
  const CollisionGeometry* o1 = nullptr;
  const CollisionGeometry* o2 = nullptr;
  int b1 = -1, b2 = -1;
  static const int NONE = -1;
  void clear() { *this = DistanceResult(); }
};

namespace amd {

inline void fill_query(hfcl_query_request& q, const QueryRequest& r) {
  q.gjk_initial_guess = r.gjk_initial_guess;
  q.gjk_variant = r.gjk_variant;
  q.gjk_convergence_criterion = r.gjk_convergence_criterion;
  q.gjk_convergence_criterion_type = r.gjk_convergence_criterion_type;
  q.gjk_max_iterations = static_cast<uint32_t>(r.gjk_max_iterations);
  q.epa_max_iterations = static_cast<uint32_t>(r.epa_max_iterations);
  q.gjk_tolerance = r.gjk_tolerance;
  q.epa_tolerance = r.epa_tolerance;
  q.collision_distance_threshold = r.collision_distance_threshold;
  for (int k = 0; k < 3; ++k) q.cached_gjk_guess[k] = r.cached_gjk_guess[k];
  q.cached_support_func_guess[0] = r.cached_support_func_guess[0];
  q.cached_support_func_guess[1] = r.cached_support_func_guess[1];
}
inline hfcl_collision_request to_abi(const CollisionRequest& r) {
  hfcl_collision_request a;
  hfcl_collision_request_init(&a);
  fill_query(a.q, r);
  a.num_max_contacts = static_cast<uint32_t>(r.num_max_contacts);
  a.enable_contact = r.enable_contact;
  a.security_margin = r.security_margin;
  a.break_distance = r.break_distance;
  a.distance_upper_bound = r.distance_upper_bound;
  return a;
}
inline hfcl_distance_request to_abi(const DistanceRequest& r) {
  hfcl_distance_request a;
  hfcl_distance_request_init(&a);
  fill_query(a.q, r);
  a.enable_nearest_points = r.enable_nearest_points;
  a.enable_signed_distance = r.enable_signed_distance;
  a.rel_err = r.rel_err;
  a.abs_err = r.abs_err;
  return a;
}
[[noreturn]] inline void throw_for(int rc) {
  const std::string msg = hfcl_last_error();
  if (rc == HFCL_ERR_INVALID_ARGUMENT || rc == HFCL_ERR_UNSUPPORTED_PAIR) throw std::invalid_argument(msg);
  throw std::runtime_error(msg);
}

// A set of geometries registered once (the device shape library) + batched queries on it:
// the CollisionCallBackCollect hand-off (collect pairs on the host, evaluate them in one call).
class BatchQueries {
 public:
  explicit BatchQueries(int device = 0) : devices_(1, device) {}
  /// Several devices of this process: the library is replicated on each and every batch is cut into contiguous shards, one per
  /// device (hfcl_multi_*, include/hppfcl_amd.h); the results are the single-device ones.  A device may be listed more than once.
  explicit BatchQueries(const std::vector<int>& devices) : devices_(devices.empty() ? std::vector<int>(1, 0) : devices) {}
  ~BatchQueries() { hfcl_multi_destroy(lib_); }
  size_t numDevices() const { return devices_.size(); }
  BatchQueries(const BatchQueries&) = delete;
  BatchQueries& operator=(const BatchQueries&) = delete;

  /// Forget every registered geometry (and free the device library): a long-lived context that has seen many temporary
  /// geometries -- the thread's default one behind collide() / distance() -- is pruned this way.
  void reset() {
    hfcl_multi_destroy(lib_);
    lib_ = nullptr;
    ++generation_;
    shapes_.clear();
    verts_.clear();
    geoms_.clear();
    ids_.clear();
    meshes_.clear();
    rec_.clear();
    guess_.clear();
    contacts_.clear();
    shapes_dirty_ = false;
    meshes_uploaded_ = 0;
    adjacency_.clear();
    adjacency_pending_ = false;
  }
  size_t numGeometries() const { return shapes_.size(); }
  const CollisionGeometry* geometry(uint32_t id) const { return geoms_.at(id); }
  /// Counts the device libraries this context has had (a new one after the first query and after every reset()): what was registered on
  /// an earlier library directly -- height fields -- is gone when this number has changed, whatever address the new library has.
  uint64_t libraryGeneration() const { return generation_; }

  uint32_t add(const CollisionGeometry* g) {
    hfcl_shape s{};
    std::vector<double> v;
    s.type = g->getNodeType();
    const ShapeBase* sb = dynamic_cast<const ShapeBase*>(g);
    s.swept_sphere_radius = sb ? sb->getSweptSphereRadius() : 0.0;
    switch (g->getNodeType()) {
      case GEOM_BOX: { auto* b = static_cast<const Box*>(g); for (int i = 0; i < 3; ++i) s.params[i] = b->halfSide[i]; break; }
      case GEOM_SPHERE: s.params[0] = static_cast<const Sphere*>(g)->radius; break;
      case GEOM_CAPSULE: { auto* c = static_cast<const Capsule*>(g); s.params[0] = c->radius; s.params[1] = c->halfLength; break; }
      case GEOM_CONE: { auto* c = static_cast<const Cone*>(g); s.params[0] = c->radius; s.params[1] = c->halfLength; break; }
      case GEOM_CYLINDER: { auto* c = static_cast<const Cylinder*>(g); s.params[0] = c->radius; s.params[1] = c->halfLength; break; }
      case GEOM_ELLIPSOID: { auto* e = static_cast<const Ellipsoid*>(g); for (int i = 0; i < 3; ++i) s.params[i] = e->radii[i]; break; }
      case GEOM_HALFSPACE: { auto* h = static_cast<const Halfspace*>(g); for (int i = 0; i < 3; ++i) s.params[i] = h->n[i]; s.params[3] = h->d; break; }
      case GEOM_PLANE: { auto* h = static_cast<const Plane*>(g); for (int i = 0; i < 3; ++i) s.params[i] = h->n[i]; s.params[3] = h->d; break; }
      case GEOM_CONVEX: {
        auto* c = static_cast<const ConvexBase*>(g);
        s.num_points = c->num_points;
        for (unsigned int k = 0; k < c->num_points; ++k) v.insert(v.end(), (*c->points)[k].data(), (*c->points)[k].data() + 3);
        break;
      }
      case GEOM_TRIANGLE: {
        auto* t = static_cast<const TriangleP*>(g);
        s.num_points = 3;
        for (const Vec3f* p : {&t->a, &t->b, &t->c}) v.insert(v.end(), p->data(), p->data() + 3);
        break;
      }
      case BV_OBBRSS: {
        auto* m = dynamic_cast<const BVHModel<OBBRSS>*>(g);
        if (!m || m->getNumBVs() == 0) throw std::invalid_argument("BVHModel: endModel() has not been called");
        auto it = ids_.find(g);
        // same object, same content?  (the address may have belonged to another geometry before)
        if (it != ids_.end() && shapes_[it->second].type == BV_OBBRSS &&
            static_cast<size_t>(shapes_[it->second].bvh_index) < meshes_.size()) {
          const MeshRef& r = meshes_[static_cast<size_t>(shapes_[it->second].bvh_index)];
          if (r.model == m && r.n_nodes == m->getNumBVs() && r.n_vertices == m->num_vertices &&
              r.checksum == checksum(*m))
            return it->second;
        }
        s.bvh_index = static_cast<int32_t>(meshes_.size());
        s.num_points = m->num_vertices;
        // the context keeps its own copy: the model may be destroyed before the library is (re)built
        meshes_.push_back(MeshRef{m, m->getNumBVs(), m->num_vertices, checksum(*m), m->nodes(),
                                  std::vector<double>(reinterpret_cast<const double*>(m->vertices.data()),
                                                      reinterpret_cast<const double*>(m->vertices.data()) + 3 * m->vertices.size()),
                                  m->flatTriangles()});
        break;
      }
      default: throw std::invalid_argument("unsupported node type");
    }
    // The cache is keyed by address; a hit is only trusted if the geometry's *content* is still
    // what was registered (addresses get reused once a geometry is destroyed).
    auto it = ids_.find(g);
    if (it != ids_.end() && s.type != BV_OBBRSS) {
      const hfcl_shape& o = shapes_[it->second];
      bool same = o.type == s.type && o.num_points == s.num_points && o.swept_sphere_radius == s.swept_sphere_radius &&
                  o.params[0] == s.params[0] && o.params[1] == s.params[1] && o.params[2] == s.params[2] &&
                  o.params[3] == s.params[3];
      if (same && (s.type == GEOM_CONVEX || s.type == GEOM_TRIANGLE))  // both carry their vertices in verts_
        for (size_t k = 0; k < v.size() && same; ++k) same = verts_[3 * size_t(o.vertex_offset) + k] == v[k];
      if (same) return it->second;
    }
    s.vertex_offset = static_cast<uint32_t>(verts_.size() / 3);
    verts_.insert(verts_.end(), v.begin(), v.end());
    shapes_.push_back(s);
    geoms_.push_back(g);
    shapes_dirty_ = true;  // the device tables follow at the next query (hfcl_lib_set_shapes: meshes and workspaces stay)
    const uint32_t id = static_cast<uint32_t>(shapes_.size() - 1);
    ids_[g] = id;
    if (s.type == GEOM_CONVEX) {  // a copy, like the vertices: the geometry may be gone by the next query
      auto* c = static_cast<const ConvexBase*>(g);
      if (c->neighbor_offsets.size() == size_t(c->num_points) + 1) {
        adjacency_[id] = std::make_pair(c->neighbor_offsets, c->neighbor_ids);
        adjacency_pending_ = true;
      }
    }
    return id;
  }

  void collide(const std::vector<std::pair<uint32_t, uint32_t>>& pairs, const std::vector<Transform3f>& tf1,
               const std::vector<Transform3f>& tf2, const CollisionRequest& request, std::vector<CollisionResult>& results) {
    run(pairs, tf1, tf2, &request, nullptr);
    results.assign(pairs.size(), CollisionResult());
    for (size_t i = 0; i < pairs.size(); ++i) fill(results[i], pairs[i], request, rec_[i], guess_[i]);
  }
  void distance(const std::vector<std::pair<uint32_t, uint32_t>>& pairs, const std::vector<Transform3f>& tf1,
                const std::vector<Transform3f>& tf2, const DistanceRequest& request, std::vector<DistanceResult>& results) {
    run(pairs, tf1, tf2, nullptr, &request);
    results.assign(pairs.size(), DistanceResult());
    for (size_t i = 0; i < pairs.size(); ++i) fill(results[i], pairs[i], rec_[i], guess_[i]);
  }

  void fill(CollisionResult& res, const std::pair<uint32_t, uint32_t>& p, const CollisionRequest& request,
            const hfcl_result& r, const hfcl_guess& g) const {
    if (!HFCL_STATUS_SKIPPED(r.status)) {
      const Vec3f n(r.normal[0], r.normal[1], r.normal[2]), p1(r.p1[0], r.p1[1], r.p1[2]), p2(r.p2[0], r.p2[1], r.p2[2]);
      const FCL_REAL dtc = r.distance - request.security_margin;  // updateDistanceLowerBoundFromLeaf
      if (dtc < res.distance_lower_bound) {
        res.distance_lower_bound = dtc;
        res.nearest_points = {{p1, p2}};
        res.normal = n;
      }
      if (r.num_contacts > 1 && !contacts_.empty()) {
        // contacts_ is ordered by query (run() sorts it once): this query's contacts are one contiguous range
        const uint32_t qi = static_cast<uint32_t>(&r - rec_.data());
        auto lo = std::lower_bound(contacts_.begin(), contacts_.end(), qi,
                                   [](const hfcl_contact& c, uint32_t q) { return c.pair < q; });
        for (; lo != contacts_.end() && lo->pair == qi; ++lo) {
          const hfcl_contact& k = *lo;
          if (res.numContacts() >= request.num_max_contacts) break;
          Contact c;
          c.o1 = geoms_[p.first];
          c.o2 = geoms_[p.second];
          c.b1 = k.b1;
          c.b2 = k.b2;
          c.normal = Vec3f(k.normal[0], k.normal[1], k.normal[2]);
          c.nearest_points = {{Vec3f(k.p1[0], k.p1[1], k.p1[2]), Vec3f(k.p2[0], k.p2[1], k.p2[2])}};
          c.pos = (c.nearest_points[0] + c.nearest_points[1]) / 2;
          c.penetration_depth = k.penetration_depth;
          res.addContact(c);
        }
      } else if (r.num_contacts > 0 && res.numContacts() < request.num_max_contacts) {
        Contact c;
        c.o1 = geoms_[p.first];
        c.o2 = geoms_[p.second];
        c.b1 = r.b1;
        c.b2 = r.b2;
        c.normal = n;
        c.nearest_points = {{p1, p2}};
        c.pos = (p1 + p2) / 2;
        c.penetration_depth = r.distance;
        res.addContact(c);
      }
    }
    res.cached_gjk_guess = Vec3f(g.gjk_guess[0], g.gjk_guess[1], g.gjk_guess[2]);
    res.cached_support_func_guess = {{g.support_guess[0], g.support_guess[1]}};
  }
  void fill(DistanceResult& res, const std::pair<uint32_t, uint32_t>& p, const hfcl_result& r, const hfcl_guess& g) const {
    if (res.min_distance > r.distance) {  // DistanceResult::update
      res.min_distance = r.distance;
      res.o1 = geoms_[p.first];
      res.o2 = geoms_[p.second];
      res.b1 = r.b1;
      res.b2 = r.b2;
      res.nearest_points = {{Vec3f(r.p1[0], r.p1[1], r.p1[2]), Vec3f(r.p2[0], r.p2[1], r.p2[2])}};
      res.normal = Vec3f(r.normal[0], r.normal[1], r.normal[2]);
    }
    res.cached_gjk_guess = Vec3f(g.gjk_guess[0], g.gjk_guess[1], g.gjk_guess[2]);
    res.cached_support_func_guess = {{g.support_guess[0], g.support_guess[1]}};
  }
  const std::vector<hfcl_result>& records() const { return rec_; }
  const std::vector<hfcl_contact>& contacts() const { return contacts_; }  // filled when num_max_contacts > 1 on meshes
  const std::vector<hfcl_guess>& guesses() const { return guess_; }

  /// The device library brought up to date with every geometry registered so far (created on first use).
  void prepare() {
    if (!lib_) {
      lib_ = hfcl_multi_create(devices_.data(), static_cast<int>(devices_.size()), shapes_.data(), shapes_.size(), verts_.data(), verts_.size() / 3);
      if (!lib_) throw std::runtime_error(hfcl_last_error());
      ++generation_;
      meshes_uploaded_ = 0;
    } else if (shapes_dirty_) {  // geometries were added since the last query: new shape tables, everything else stays
      const int rc = hfcl_multi_set_shapes(lib_, shapes_.data(), shapes_.size(), verts_.data(), verts_.size() / 3);
      if (rc) throw_for(rc);
    }
    if (shapes_dirty_ || adjacency_pending_) {  // (hfcl_lib_set_shapes dropped the adjacencies of the old table)
      for (const auto& kv : adjacency_) {
        const int rc = hfcl_multi_set_convex_neighbors(lib_, kv.first, kv.second.first.data(), kv.second.second.data());
        if (rc) throw_for(rc);
      }
      adjacency_pending_ = false;
    }
    shapes_dirty_ = false;
    for (; meshes_uploaded_ < meshes_.size(); ++meshes_uploaded_) {  // bvh_index = registration order
      const MeshRef& r = meshes_[meshes_uploaded_];
      if (hfcl_multi_add_bvh(lib_, r.nodes.data(), r.nodes.size(), r.verts.data(), r.verts.size() / 3, r.tris.data(),
                             r.tris.size() / 3) < 0)
        throw std::runtime_error(hfcl_last_error());
    }
  }
  /// The library of the first device (up to date): what the contact-patch calls run on.
  hfcl_lib* library() {
    prepare();
    return hfcl_multi_replica(lib_, 0);
  }
  void run(const std::vector<std::pair<uint32_t, uint32_t>>& pairs, const std::vector<Transform3f>& tf1,
           const std::vector<Transform3f>& tf2, const CollisionRequest* creq, const DistanceRequest* dreq) {
    if (tf1.size() != pairs.size() || tf2.size() != pairs.size()) throw std::invalid_argument("pairs/poses size mismatch");
    prepare();
    std::vector<uint32_t> s1(pairs.size()), s2(pairs.size());
    for (size_t i = 0; i < pairs.size(); ++i) {
      s1[i] = pairs[i].first;
      s2[i] = pairs[i].second;
    }
    rec_.resize(pairs.size());
    guess_.resize(pairs.size());
    int rc;
    contacts_.clear();
    if (creq && creq->num_max_contacts > 1 && !meshes_.empty()) {
      // mesh-mesh queries can produce several contacts each: use the contact-list entry point
      const hfcl_collision_request a = to_abi(*creq);
      size_t cap = std::max<size_t>(1024, 64 * pairs.size()), produced = 0;
      for (int attempt = 0; attempt < 2; ++attempt) {
        contacts_.resize(cap);
        // (contact lists are appended through one device counter: the first replica takes the whole batch)
        rc = hfcl_collide_batch_contacts(hfcl_multi_replica(lib_, 0), s1.data(), s2.data(), reinterpret_cast<const double*>(tf1.data()),
                                         reinterpret_cast<const double*>(tf2.data()), pairs.size(), &a, rec_.data(),
                                         contacts_.data(), cap, &produced);
        if (rc || produced <= cap) break;
        cap = produced;
      }
      contacts_.resize(rc ? 0 : std::min(produced, cap));
      // the device appends contacts in completion order: group them by query once (the order of one query's
      // contacts -- its traversal order -- is kept), so that fill() finds a query's range by binary search
      std::stable_sort(contacts_.begin(), contacts_.end(),
                       [](const hfcl_contact& x, const hfcl_contact& y) { return x.pair < y.pair; });
      for (auto& g : guess_) g = hfcl_guess{{1, 0, 0}, {0, 0}};
    } else if (creq) {
      const hfcl_collision_request a = to_abi(*creq);
      rc = hfcl_collide_batch_multi(lib_, s1.data(), s2.data(), reinterpret_cast<const double*>(tf1.data()),
                                    reinterpret_cast<const double*>(tf2.data()), pairs.size(), &a, rec_.data(), nullptr, guess_.data());
    } else {
      const hfcl_distance_request a = to_abi(*dreq);
      rc = hfcl_distance_batch_multi(lib_, s1.data(), s2.data(), reinterpret_cast<const double*>(tf1.data()),
                                     reinterpret_cast<const double*>(tf2.data()), pairs.size(), &a, rec_.data(), nullptr, guess_.data());
    }
    if (rc) throw_for(rc);
  }

 private:
  std::vector<int> devices_;
  uint64_t generation_ = 0;
  hfcl_multi* lib_ = nullptr;  // one replica of the library per device (one device: a single library behind the same calls)
  std::vector<hfcl_shape> shapes_;
  std::vector<double> verts_;
  std::vector<const CollisionGeometry*> geoms_;
  std::map<const CollisionGeometry*, uint32_t> ids_;
  std::vector<hfcl_result> rec_;
  std::vector<hfcl_guess> guess_;
  std::vector<hfcl_contact> contacts_;
  bool shapes_dirty_ = false;
  std::map<uint32_t, std::pair<std::vector<uint32_t>, std::vector<uint32_t>>> adjacency_;  // shape id -> ConvexBase::neighbors (CSR)
  bool adjacency_pending_ = false;
  size_t meshes_uploaded_ = 0;
  struct MeshRef {
    const BVHModel<OBBRSS>* model;
    unsigned int n_nodes, n_vertices;
    double checksum;
    std::vector<hfcl_bvh_node> nodes;
    std::vector<double> verts;
    std::vector<uint32_t> tris;
  };
  std::vector<MeshRef> meshes_;
  static double checksum(const BVHModel<OBBRSS>& m) {  // cheap content fingerprint for the address-keyed cache
    double c = 0;
    for (size_t i = 0; i < m.vertices.size(); i += 1 + m.vertices.size() / 64) c += m.vertices[i][0] + 2 * m.vertices[i][1] + 3 * m.vertices[i][2];
    return c + m.getBV(0).rss_radius;
  }
};

inline BatchQueries& default_context() {
  static thread_local BatchQueries ctx(0);
  return ctx;
}

/// Batched collide() of HeightField<AABB> against convex solids (hfcl_hfield_collide_batch) on the library of a BatchQueries context:
/// the solids are that context's geometries, the fields are registered here (a field whose heights were updated, and every field after
/// the context was reset, is registered again).  One HeightFieldBatch per context.  The batch keeps a copy of every field it was given
/// and the library a set of tables for each: reset() drops both (the indices addField returned are void then).
class HeightFieldBatch {
 public:
  explicit HeightFieldBatch(BatchQueries& ctx) : ctx_(ctx) {}
  uint32_t addSolid(const CollisionGeometry* g) { return ctx_.add(g); }
  size_t numFields() const { return fields_.size(); }
  /// Forget every field (and clear the library's height-field tables, if the library this batch registered on is still the context's).
  void reset() {
    if (lib_ && generation_ == ctx_.libraryGeneration()) hfcl_lib_clear_hfields(lib_);
    fields_.clear();
    ++epoch_;
  }
  /// counts the reset() calls: an index addField or libraryIndex returned before the last one is void
  uint64_t epoch() const { return epoch_; }
  /// The index of field k (addField) on the context's library as it is now; the field is registered there if it is not yet.
  uint32_t libraryIndex(uint32_t k) {
    hfcl_lib* lib = ctx_.library();
    if (lib != lib_ || generation_ != ctx_.libraryGeneration()) {  // a new library (the first query, or the context was reset -- the new one
      lib_ = lib;                                                 // may sit at the old address): nothing of ours is on it
      generation_ = ctx_.libraryGeneration();
      for (Entry& e : fields_) e.index = -1;
    }
    Entry& e = fields_.at(k);
    if (e.index < 0) {
      e.index = hfcl_lib_add_hfield(lib, e.x_dim, e.y_dim, e.heights.data(), e.rows, e.cols, e.min_height);
      if (e.index < 0) throw std::invalid_argument(hfcl_last_error());
    }
    return static_cast<uint32_t>(e.index);
  }
  uint32_t addField(const HeightField<AABB>* f) {
    // The cache is keyed by address; a hit is only trusted if the field's CONTENT is still what was copied (addresses get reused once a
    // field is destroyed: a stack object in a loop, a freed and reallocated one -- and every new field starts at version 1).
    for (size_t k = 0; k < fields_.size(); ++k) {
      const Entry& o = fields_[k];
      if (o.field != f || o.version != f->version()) continue;
      const MatrixXf& h = f->getHeights();
      if (o.x_dim == f->getXDim() && o.y_dim == f->getYDim() && o.min_height == f->getMinHeight() && o.rows == h.rows() && o.cols == h.cols() &&
          std::equal(o.heights.begin(), o.heights.end(), h.data()))
        return static_cast<uint32_t>(k);
    }
    Entry e;
    e.field = f;
    e.version = f->version();
    e.x_dim = f->getXDim();
    e.y_dim = f->getYDim();
    e.min_height = f->getMinHeight();
    e.rows = f->getHeights().rows();
    e.cols = f->getHeights().cols();
    e.heights.assign(f->getHeights().data(), f->getHeights().data() + e.rows * e.cols);  // a copy: the field may be gone by the next query
    fields_.push_back(e);
    return static_cast<uint32_t>(fields_.size() - 1);
  }
  /// Query i: collide(field, solid), or collide(solid, field) where swapped[i] (swapped: empty, or one flag per query).  tf_field /
  /// tf_solid are the field's and the solid's pose either way.  Results are fresh objects.
  void collide(const std::vector<std::pair<uint32_t, uint32_t>>& field_solid, const std::vector<Transform3f>& tf_field,
               const std::vector<Transform3f>& tf_solid, const std::vector<uint8_t>& swapped, const CollisionRequest& request,
               std::vector<CollisionResult>& results) {
    const size_t n = field_solid.size();
    if (tf_field.size() != n || tf_solid.size() != n || (!swapped.empty() && swapped.size() != n))
      throw std::invalid_argument("pairs/poses size mismatch");
    hfcl_lib* lib = ctx_.library();
    std::vector<uint32_t> hf(n), sh(n);
    for (size_t i = 0; i < n; ++i) {
      hf[i] = libraryIndex(field_solid[i].first);
      sh[i] = field_solid[i].second;
    }
    const hfcl_collision_request a = to_abi(request);
    rec_.resize(n);
    bound_.resize(n);
    size_t cap = std::max<size_t>(64, 4 * n), produced = 0;
    int rc = HFCL_OK;
    for (int attempt = 0; attempt < 2; ++attempt) {  // (a list that outgrew the guess: once more with the count)
      contacts_.resize(cap);
      rc = hfcl_hfield_collide_batch(lib, hf.data(), sh.data(), reinterpret_cast<const double*>(tf_field.data()),
                                     reinterpret_cast<const double*>(tf_solid.data()), n, swapped.empty() ? nullptr : swapped.data(), &a,
                                     rec_.data(), bound_.data(), contacts_.data(), cap, &produced);
      if (rc || produced <= cap) break;
      cap = produced;
    }
    if (rc == HFCL_ERR_LIMIT) throw std::invalid_argument(hfcl_last_error());
    if (rc) throw_for(rc);
    contacts_.resize(std::min(produced, cap));
    results.assign(n, CollisionResult());
    size_t k = 0;
    for (size_t i = 0; i < n; ++i) {
      const bool sw = !swapped.empty() && swapped[i];
      const CollisionGeometry* field = fields_[field_solid[i].first].field;
      const CollisionGeometry* solid = ctx_.geometry(sh[i]);
      fill(results[i], rec_[i], bound_[i], sw ? solid : field, sw ? field : solid, static_cast<uint32_t>(i), k, request);
    }
  }
  /// One record into a result that may hold earlier ones: every contact, the call's bound; nearest_points / normal are the record's
  /// (the first contact's when there is one).
  void fill(CollisionResult& res, const hfcl_result& r, double bound, const CollisionGeometry* o1, const CollisionGeometry* o2, uint32_t query,
            size_t& k, const CollisionRequest& request) const {
    fill(contacts_, res, r, bound, o1, o2, query, k, request);
  }
  /// ... with the contacts of a call made elsewhere (Scene::collideTerrain)
  static void fill(const std::vector<hfcl_contact>& contacts_, CollisionResult& res, const hfcl_result& r, double bound, const CollisionGeometry* o1,
                   const CollisionGeometry* o2, uint32_t query, size_t& k, const CollisionRequest& request) {
    while (k < contacts_.size() && contacts_[k].pair < query) ++k;
    if (HFCL_STATUS_SKIPPED(r.status)) return;
    if (bound < res.distance_lower_bound) {
      res.distance_lower_bound = bound;
      res.normal = Vec3f(r.normal[0], r.normal[1], r.normal[2]);
      res.nearest_points = {{Vec3f(r.p1[0], r.p1[1], r.p1[2]), Vec3f(r.p2[0], r.p2[1], r.p2[2])}};
    }
    for (; k < contacts_.size() && contacts_[k].pair == query; ++k) {
      if (res.numContacts() >= request.num_max_contacts) continue;
      const hfcl_contact& h = contacts_[k];
      Contact c;
      c.o1 = o1;
      c.o2 = o2;
      c.b1 = h.b1;
      c.b2 = h.b2;
      c.normal = Vec3f(h.normal[0], h.normal[1], h.normal[2]);
      c.nearest_points = {{Vec3f(h.p1[0], h.p1[1], h.p1[2]), Vec3f(h.p2[0], h.p2[1], h.p2[2])}};
      c.pos = (c.nearest_points[0] + c.nearest_points[1]) / 2;
      c.penetration_depth = h.penetration_depth;
      res.addContact(c);
    }
  }
  const std::vector<hfcl_result>& records() const { return rec_; }
  const std::vector<double>& bounds() const { return bound_; }
  const std::vector<hfcl_contact>& contacts() const { return contacts_; }

 private:
  struct Entry {
    const HeightField<AABB>* field;
    unsigned int version;
    FCL_REAL x_dim, y_dim, min_height;
    size_t rows, cols;
    std::vector<double> heights;
    int index = -1;  // on lib_
  };
  BatchQueries& ctx_;
  hfcl_lib* lib_ = nullptr;
  uint64_t generation_ = 0;  // ctx_.libraryGeneration() when lib_ was taken
  uint64_t epoch_ = 0;
  std::vector<Entry> fields_;
  std::vector<hfcl_result> rec_;
  std::vector<double> bound_;
  std::vector<hfcl_contact> contacts_;
};
constexpr size_t DEFAULT_HFIELD_BATCH_MAX = 16;  // fields (and versions of fields) the thread's default batch keeps before it starts over
inline HeightFieldBatch& default_hfield_batch() {
  static thread_local HeightFieldBatch b(default_context());
  return b;
}
/// does collide() have a function for this pair with a height field in it?
inline bool hfield_pair_supported(const CollisionGeometry* o1, const CollisionGeometry* o2) {
  const bool h1 = o1->getNodeType() == HF_AABB, h2 = o2->getNodeType() == HF_AABB;
  return h1 != h2 && hfcl_hfield_pair_supported((h1 ? o2 : o1)->getNodeType()) != 0;
}
inline bool is_hfield(const CollisionGeometry* g) { return g->getNodeType() == HF_AABB || g->getNodeType() == HF_OBBRSS; }

/// Batched collide() of OcTree objects against convex solids (hfcl_octree_collide_batch) on the library of a BatchQueries context: the
/// solids are that context's geometries, the trees are registered here (and again after the context was reset, or when a tree's
/// thresholds were set since).  One OcTreeBatch per context; reset() forgets the trees, here and on the library.
class OcTreeBatch {
 public:
  explicit OcTreeBatch(BatchQueries& ctx) : ctx_(ctx) {}
  uint32_t addSolid(const CollisionGeometry* g) { return ctx_.add(g); }
  size_t numTrees() const { return trees_.size(); }
  void reset() {
    if (lib_ && generation_ == ctx_.libraryGeneration()) hfcl_lib_clear_octrees(lib_);
    trees_.clear();
  }
  uint32_t addTree(const OcTree* t) {
    // keyed by address; a hit is trusted only while the tree's content is what was copied (addresses get reused)
    for (size_t k = 0; k < trees_.size(); ++k) {
      const Entry& o = trees_[k];
      if (o.tree != t || o.resolution != t->getResolution() || o.depth != t->getTreeDepth() || o.nodes.size() != t->getNodes().size()) continue;
      if (o.nodes.empty() || std::memcmp(o.nodes.data(), t->getNodes().data(), o.nodes.size() * sizeof(hfcl_octree_node)) == 0) return static_cast<uint32_t>(k);
    }
    Entry e;
    e.tree = t;
    e.resolution = t->getResolution();
    e.depth = t->getTreeDepth();
    e.nodes = t->getNodes();  // a copy: the tree may be gone by the next query
    trees_.push_back(e);
    return static_cast<uint32_t>(trees_.size() - 1);
  }
  /// The index of tree k (addTree) on the context's library as it is now, registered or its thresholds set there as needed.
  uint32_t libraryIndex(uint32_t k) {
    hfcl_lib* lib = ctx_.library();
    if (lib != lib_ || generation_ != ctx_.libraryGeneration()) {
      lib_ = lib;
      generation_ = ctx_.libraryGeneration();
      for (Entry& e : trees_) e.index = -1;
    }
    Entry& e = trees_.at(k);
    const FCL_REAL occ = e.tree->getOccupancyThres(), fr = e.tree->getFreeThres();
    if (e.index < 0) {
      e.index = hfcl_lib_add_octree(lib, e.nodes.data(), e.nodes.size(), e.resolution, e.depth, occ, fr);
      if (e.index < 0) throw std::invalid_argument(hfcl_last_error());
    } else if (e.occ != occ || e.free != fr) {
      if (hfcl_lib_octree_set_thresholds(lib, e.index, occ, fr)) throw std::invalid_argument(hfcl_last_error());
    }
    e.occ = occ;
    e.free = fr;
    return static_cast<uint32_t>(e.index);
  }
  /// Query i: collide(tree, solid), or collide(solid, tree) where swapped[i] -- the same result either way but for the order of the
  /// operands the caller named (the reference does not swap an octree query back).  Results are fresh objects: the tree is o1 of every
  /// contact and its node b1.
  void collide(const std::vector<std::pair<uint32_t, uint32_t>>& tree_solid, const std::vector<Transform3f>& tf_tree,
               const std::vector<Transform3f>& tf_solid, const std::vector<uint8_t>& swapped, const CollisionRequest& request,
               std::vector<CollisionResult>& results) {
    collideWith(hfcl_octree_collide_batch, tree_solid, tf_tree, tf_solid, swapped, request, results);
  }
  /// The same for BVHModel<OBBRSS> meshes of the context in the place of the solids (hfcl_octree_mesh_collide_batch,
  /// hppfcl_amd_octree_mesh.h): query i is collide(tree, mesh), or collide(mesh, tree) where swapped[i].  The tree is o1 of every contact,
  /// its node b1, the mesh's triangle b2, and the nearest points are the solver's own.
  void collideMesh(const std::vector<std::pair<uint32_t, uint32_t>>& tree_mesh, const std::vector<Transform3f>& tf_tree,
                   const std::vector<Transform3f>& tf_mesh, const std::vector<uint8_t>& swapped, const CollisionRequest& request,
                   std::vector<CollisionResult>& results) {
    collideWith(hfcl_octree_mesh_collide_batch, tree_mesh, tf_tree, tf_mesh, swapped, request, results);
  }

 private:
  typedef int (*CollideCall)(hfcl_lib*, const uint32_t*, const uint32_t*, const double*, const double*, size_t, const uint8_t*,
                             const hfcl_collision_request*, hfcl_result*, double*, hfcl_contact*, size_t, size_t*);
  void collideWith(CollideCall call, const std::vector<std::pair<uint32_t, uint32_t>>& tree_solid, const std::vector<Transform3f>& tf_tree,
                   const std::vector<Transform3f>& tf_solid, const std::vector<uint8_t>& swapped, const CollisionRequest& request,
                   std::vector<CollisionResult>& results) {
    const size_t n = tree_solid.size();
    if (tf_tree.size() != n || tf_solid.size() != n || (!swapped.empty() && swapped.size() != n))
      throw std::invalid_argument("pairs/poses size mismatch");
    hfcl_lib* lib = ctx_.library();
    std::vector<uint32_t> ot(n), sh(n);
    for (size_t i = 0; i < n; ++i) {
      ot[i] = libraryIndex(tree_solid[i].first);
      sh[i] = tree_solid[i].second;
    }
    const hfcl_collision_request a = to_abi(request);
    rec_.resize(n);
    bound_.resize(n);
    size_t cap = std::max<size_t>(64, 4 * n), produced = 0;
    int rc = HFCL_OK;
    for (int attempt = 0; attempt < 2; ++attempt) {  // (a list that outgrew the guess: once more with the count)
      contacts_.resize(cap);
      rc = call(lib, ot.data(), sh.data(), reinterpret_cast<const double*>(tf_tree.data()), reinterpret_cast<const double*>(tf_solid.data()), n,
                swapped.empty() ? nullptr : swapped.data(), &a, rec_.data(), bound_.data(), contacts_.data(), cap, &produced);
      if (rc || produced <= cap) break;
      cap = produced;
    }
    if (rc == HFCL_ERR_LIMIT) throw std::invalid_argument(hfcl_last_error());
    if (rc) throw_for(rc);
    contacts_.resize(std::min(produced, cap));
    results.assign(n, CollisionResult());
    size_t k = 0;
    for (size_t i = 0; i < n; ++i)
      fill(results[i], rec_[i], bound_[i], trees_[tree_solid[i].first].tree, ctx_.geometry(sh[i]), static_cast<uint32_t>(i), k, request);
  }

 public:
  /// One record into a result that may hold earlier ones: every contact and the call's bound; the result's nearest_points / normal
  /// are set from a record without a contact (one with a contact carries the contact's rebuilt points instead).
  void fill(CollisionResult& res, const hfcl_result& r, double bound, const CollisionGeometry* tree, const CollisionGeometry* solid, uint32_t query,
            size_t& k, const CollisionRequest& request) const {
    while (k < contacts_.size() && contacts_[k].pair < query) ++k;
    if (HFCL_STATUS_SKIPPED(r.status)) return;
    if (bound < res.distance_lower_bound) {
      res.distance_lower_bound = bound;
      if (r.num_contacts == 0) {
        res.normal = Vec3f(r.normal[0], r.normal[1], r.normal[2]);
        res.nearest_points = {{Vec3f(r.p1[0], r.p1[1], r.p1[2]), Vec3f(r.p2[0], r.p2[1], r.p2[2])}};
      }
    }
    for (; k < contacts_.size() && contacts_[k].pair == query; ++k) {
      if (res.numContacts() >= request.num_max_contacts) continue;
      const hfcl_contact& h = contacts_[k];
      Contact c;
      c.o1 = tree;
      c.o2 = solid;
      c.b1 = h.b1;
      c.b2 = h.b2;
      c.normal = Vec3f(h.normal[0], h.normal[1], h.normal[2]);
      c.nearest_points = {{Vec3f(h.p1[0], h.p1[1], h.p1[2]), Vec3f(h.p2[0], h.p2[1], h.p2[2])}};
      c.pos = (c.nearest_points[0] + c.nearest_points[1]) / 2;
      c.penetration_depth = h.penetration_depth;
      res.addContact(c);
    }
  }
  /// Query i: distance(tree, solid), or distance(solid, tree) where swapped[i]: the result of the reference's ordered walk
  /// (hfcl_octree_distance_batch, hppfcl_amd_octree_distance.h) -- the same either way but for the order the caller named.  Results are
  /// fresh objects: the tree is o1 and its node b1.  visited (optional): the leaves each walk solved.
  void distance(const std::vector<std::pair<uint32_t, uint32_t>>& tree_solid, const std::vector<Transform3f>& tf_tree,
                const std::vector<Transform3f>& tf_solid, const std::vector<uint8_t>& swapped, const DistanceRequest& request,
                std::vector<DistanceResult>& results, std::vector<uint32_t>* visited = nullptr) {
    distanceWith(hfcl_octree_distance_batch, tree_solid, tf_tree, tf_solid, swapped, request, results, visited);
  }
  /// The same for BVHModel<OBBRSS> meshes of the context in the place of the solids (hfcl_octree_mesh_distance_batch,
  /// hppfcl_amd_octree_mesh_distance.h): query i is distance(tree, mesh), or distance(mesh, tree) where swapped[i].  The tree is o1, its
  /// node b1, the mesh's triangle b2.  visited (optional): the (leaf, triangle) pairs each walk solved.
  void distanceMesh(const std::vector<std::pair<uint32_t, uint32_t>>& tree_mesh, const std::vector<Transform3f>& tf_tree,
                    const std::vector<Transform3f>& tf_mesh, const std::vector<uint8_t>& swapped, const DistanceRequest& request,
                    std::vector<DistanceResult>& results, std::vector<uint32_t>* visited = nullptr) {
    distanceWith(hfcl_octree_mesh_distance_batch, tree_mesh, tf_tree, tf_mesh, swapped, request, results, visited);
  }

 private:
  typedef int (*DistanceCall)(hfcl_lib*, const uint32_t*, const uint32_t*, const double*, const double*, size_t, const uint8_t*,
                              const hfcl_distance_request*, hfcl_result*, uint32_t*);
  void distanceWith(DistanceCall call, const std::vector<std::pair<uint32_t, uint32_t>>& tree_solid, const std::vector<Transform3f>& tf_tree,
                    const std::vector<Transform3f>& tf_solid, const std::vector<uint8_t>& swapped, const DistanceRequest& request,
                    std::vector<DistanceResult>& results, std::vector<uint32_t>* visited) {
    const size_t n = tree_solid.size();
    if (tf_tree.size() != n || tf_solid.size() != n || (!swapped.empty() && swapped.size() != n))
      throw std::invalid_argument("pairs/poses size mismatch");
    hfcl_lib* lib = ctx_.library();
    std::vector<uint32_t> ot(n), sh(n);
    for (size_t i = 0; i < n; ++i) {
      ot[i] = libraryIndex(tree_solid[i].first);
      sh[i] = tree_solid[i].second;
    }
    const hfcl_distance_request a = to_abi(request);
    rec_.resize(n);
    if (visited) visited->assign(n, 0u);
    const int rc = call(lib, ot.data(), sh.data(), reinterpret_cast<const double*>(tf_tree.data()), reinterpret_cast<const double*>(tf_solid.data()), n,
                        swapped.empty() ? nullptr : swapped.data(), &a, rec_.data(), visited ? visited->data() : nullptr);
    if (rc == HFCL_ERR_LIMIT) throw std::invalid_argument(hfcl_last_error());
    if (rc) throw_for(rc);
    results.assign(n, DistanceResult());
    for (size_t i = 0; i < n; ++i) fill(results[i], rec_[i], trees_[tree_solid[i].first].tree, ctx_.geometry(sh[i]));
  }

 public:
  /// DistanceResult::update with one record
  void fill(DistanceResult& res, const hfcl_result& r, const CollisionGeometry* tree, const CollisionGeometry* solid) const {
    if (HFCL_STATUS_SKIPPED(r.status)) return;
    if (res.min_distance > r.distance) {
      res.min_distance = r.distance;
      res.o1 = tree;
      res.o2 = solid;
      res.b1 = r.b1;
      res.b2 = r.b2;
      res.nearest_points = {{Vec3f(r.p1[0], r.p1[1], r.p1[2]), Vec3f(r.p2[0], r.p2[1], r.p2[2])}};
      res.normal = Vec3f(r.normal[0], r.normal[1], r.normal[2]);
    }
  }
  const std::vector<hfcl_result>& records() const { return rec_; }
  const std::vector<double>& bounds() const { return bound_; }
  const std::vector<hfcl_contact>& contacts() const { return contacts_; }

 private:
  struct Entry {
    const OcTree* tree;
    FCL_REAL resolution;
    unsigned int depth;
    std::vector<hfcl_octree_node> nodes;
    FCL_REAL occ = 0, free = 0;  // as set on lib_
    int index = -1;              // on lib_
  };
  BatchQueries& ctx_;
  hfcl_lib* lib_ = nullptr;
  uint64_t generation_ = 0;  // ctx_.libraryGeneration() when lib_ was taken
  std::vector<Entry> trees_;
  std::vector<hfcl_result> rec_;
  std::vector<double> bound_;
  std::vector<hfcl_contact> contacts_;
};
constexpr size_t DEFAULT_OCTREE_BATCH_MAX = 16;  // trees the thread's default batch keeps before it starts over
inline OcTreeBatch& default_octree_batch() {
  static thread_local OcTreeBatch b(default_context());
  return b;
}
inline bool is_octree(const CollisionGeometry* g) { return g->getNodeType() == GEOM_OCTREE; }
/// does collide() have a function for this pair with an octree in it?
inline bool octree_pair_supported(const CollisionGeometry* o1, const CollisionGeometry* o2) {
  const bool t1 = is_octree(o1), t2 = is_octree(o2);
  const int other = (t1 ? o2 : o1)->getNodeType();
  return t1 != t2 && (hfcl_octree_pair_supported(other) != 0 || hfcl_octree_mesh_pair_supported(other) != 0);
}
/// ... and distance()?
inline bool octree_distance_pair_supported(const CollisionGeometry* o1, const CollisionGeometry* o2) {
  const bool t1 = is_octree(o1), t2 = is_octree(o2);
  return t1 != t2 && hfcl_octree_distance_pair_supported((t1 ? o2 : o1)->getNodeType()) != 0;
}

/// distance() between an OcTree and a BVHModel<OBBRSS>, either operand order, as a batch of one through
/// OcTreeBatch::distanceMesh (hppfcl_amd_octree_mesh_distance.h).  A call of its own BESIDE the dispatch: hpp::fcl::distance() and
/// ComputeDistance keep refusing the pair (taking it there is the follow-up; two tests hold the refusal).  Either order gets the
/// octree-first result: the tree is result.o1 and its node b1, the mesh result.o2 and its triangle b2.
inline FCL_REAL distanceOcTreeMesh(const CollisionGeometry* o1, const Transform3f& tf1, const CollisionGeometry* o2, const Transform3f& tf2,
                                   const DistanceRequest& request, DistanceResult& result) {
  const bool t1 = is_octree(o1), t2 = is_octree(o2);
  if (t1 == t2 || hfcl_octree_mesh_distance_pair_supported((t1 ? o2 : o1)->getNodeType()) == 0)
    throw std::invalid_argument("Distance function between the two node types is not yet supported.");
  if (result.min_distance <= 0) return result.min_distance;  // DistanceRequest::isSatisfied
  const bool swapped = !t1;
  OcTreeBatch& ob = default_octree_batch();
  if (ob.numTrees() >= DEFAULT_OCTREE_BATCH_MAX) ob.reset();
  const std::pair<uint32_t, uint32_t> ts(ob.addTree(static_cast<const OcTree*>(swapped ? o2 : o1)), ob.addSolid(swapped ? o1 : o2));
  std::vector<DistanceResult> one;
  ob.distanceMesh({ts}, {swapped ? tf2 : tf1}, {swapped ? tf1 : tf2}, {static_cast<uint8_t>(swapped ? 1 : 0)}, request, one);
  ob.fill(result, ob.records()[0], swapped ? o2 : o1, swapped ? o1 : o2);
  return ob.records()[0].distance;
}

}  // namespace amd

/// hpp::fcl::collide (src/collision.cpp:69-130) as a batch of one.  Results accumulate in
/// `result` like in the reference (the caller clears between queries).
inline std::size_t collide(const CollisionGeometry* o1, const Transform3f& tf1, const CollisionGeometry* o2,
                           const Transform3f& tf2, const CollisionRequest& request, CollisionResult& result) {
  if (request.security_margin == -std::numeric_limits<FCL_REAL>::infinity()) {
    result.clear();
    return 0;
  }
  if (request.num_max_contacts == 0)
    throw std::invalid_argument("Invalid number of max contacts (current value is 0).");
  if (result.isCollision() && request.num_max_contacts <= result.numContacts()) return result.numContacts();
  if (amd::is_hfield(o1) || amd::is_hfield(o2)) {  // a height field against a solid, either order (hppfcl_amd_hfield.h)
    if (!amd::hfield_pair_supported(o1, o2)) throw std::invalid_argument("Collision function between the two node types is not yet supported.");
    const bool swapped = !amd::is_hfield(o1);
    amd::HeightFieldBatch& hb = amd::default_hfield_batch();
    if (hb.numFields() >= amd::DEFAULT_HFIELD_BATCH_MAX) hb.reset();  // (fields that came and went, versions of updated ones: not kept for ever)
    const std::pair<uint32_t, uint32_t> fs(hb.addField(static_cast<const HeightField<AABB>*>(swapped ? o2 : o1)), hb.addSolid(swapped ? o1 : o2));
    std::vector<CollisionResult> one;
    hb.collide({fs}, {swapped ? tf2 : tf1}, {swapped ? tf1 : tf2}, {static_cast<uint8_t>(swapped ? 1 : 0)}, request, one);
    size_t k = 0;
    hb.fill(result, hb.records()[0], hb.bounds()[0], o1, o2, 0, k, request);
    return result.numContacts();
  }
  if (amd::is_octree(o1) || amd::is_octree(o2)) {  // an octree against a solid or a mesh, either order (hppfcl_amd_octree.h, hppfcl_amd_octree_mesh.h)
    if (!amd::octree_pair_supported(o1, o2)) throw std::invalid_argument("Collision function between the two node types is not yet supported.");
    const bool swapped = !amd::is_octree(o1);
    amd::OcTreeBatch& ob = amd::default_octree_batch();
    if (ob.numTrees() >= amd::DEFAULT_OCTREE_BATCH_MAX) ob.reset();
    const std::pair<uint32_t, uint32_t> ts(ob.addTree(static_cast<const OcTree*>(swapped ? o2 : o1)), ob.addSolid(swapped ? o1 : o2));
    std::vector<CollisionResult> one;
    if (hfcl_octree_mesh_pair_supported((swapped ? o1 : o2)->getNodeType()))  // a BVHModel<OBBRSS> (hppfcl_amd_octree_mesh.h)
      ob.collideMesh({ts}, {swapped ? tf2 : tf1}, {swapped ? tf1 : tf2}, {static_cast<uint8_t>(swapped ? 1 : 0)}, request, one);
    else
      ob.collide({ts}, {swapped ? tf2 : tf1}, {swapped ? tf1 : tf2}, {static_cast<uint8_t>(swapped ? 1 : 0)}, request, one);
    size_t k = 0;
    ob.fill(result, ob.records()[0], ob.bounds()[0], swapped ? o2 : o1, swapped ? o1 : o2, 0, k, request);
    return result.numContacts();
  }
  amd::BatchQueries& ctx = amd::default_context();
  const std::pair<uint32_t, uint32_t> p(ctx.add(o1), ctx.add(o2));
  ctx.run({p}, {tf1}, {tf2}, &request, nullptr);
  ctx.fill(result, p, request, ctx.records()[0], ctx.guesses()[0]);
  if (request.gjk_initial_guess == CachedGuess) {  // QueryRequest::updateGuess
    request.cached_gjk_guess = result.cached_gjk_guess;
    request.cached_support_func_guess = result.cached_support_func_guess;
  }
  return result.numContacts();
}

/// hpp::fcl::distance (src/distance.cpp:60-109) as a batch of one.
inline FCL_REAL distance(const CollisionGeometry* o1, const Transform3f& tf1, const CollisionGeometry* o2,
                         const Transform3f& tf2, const DistanceRequest& request, DistanceResult& result) {
  if (result.min_distance <= 0) return result.min_distance;  // DistanceRequest::isSatisfied
  if (amd::is_octree(o1) || amd::is_octree(o2)) {  // an octree against a solid, either order (hppfcl_amd_octree_distance.h)
    if (!amd::octree_distance_pair_supported(o1, o2)) throw std::invalid_argument("Distance function between the two node types is not yet supported.");
    const bool swapped = !amd::is_octree(o1);
    amd::OcTreeBatch& ob = amd::default_octree_batch();
    if (ob.numTrees() >= amd::DEFAULT_OCTREE_BATCH_MAX) ob.reset();
    const std::pair<uint32_t, uint32_t> ts(ob.addTree(static_cast<const OcTree*>(swapped ? o2 : o1)), ob.addSolid(swapped ? o1 : o2));
    std::vector<DistanceResult> one;
    ob.distance({ts}, {swapped ? tf2 : tf1}, {swapped ? tf1 : tf2}, {static_cast<uint8_t>(swapped ? 1 : 0)}, request, one);
    ob.fill(result, ob.records()[0], swapped ? o2 : o1, swapped ? o1 : o2);  // the octree-first result: the tree is o1, its node b1
    return ob.records()[0].distance;
  }
  amd::BatchQueries& ctx = amd::default_context();
  const std::pair<uint32_t, uint32_t> p(ctx.add(o1), ctx.add(o2));
  ctx.run({p}, {tf1}, {tf2}, nullptr, &request);
  ctx.fill(result, p, ctx.records()[0], ctx.guesses()[0]);
  if (request.gjk_initial_guess == CachedGuess) {
    request.cached_gjk_guess = result.cached_gjk_guess;
    request.cached_support_func_guess = result.cached_support_func_guess;
  }
  return ctx.records()[0].distance;
}

/// ComputeCollision / ComputeDistance (include/hpp/fcl/collision.h:79-117, distance.h:74-112): the geometry pair is
/// looked up once at construction (std::invalid_argument for a pair without an evaluator, src/collision.cpp:132-158,
/// src/distance.cpp:111-137); every call is the batch-of-one path of collide() / distance().
class ComputeCollision {
 public:
  ComputeCollision(const CollisionGeometry* o1_, const CollisionGeometry* o2_) : o1(o1_), o2(o2_) {
    if (amd::is_octree(o1) || amd::is_octree(o2) ? !amd::octree_pair_supported(o1, o2)
        : amd::is_hfield(o1) || amd::is_hfield(o2) ? !amd::hfield_pair_supported(o1, o2)
                                                   : !hfcl_pair_supported(o1->getNodeType(), o2->getNodeType(), 0))
      throw std::invalid_argument("Collision function between the two node types is not yet supported.");
  }
  virtual ~ComputeCollision() {}
  std::size_t operator()(const Transform3f& tf1, const Transform3f& tf2, const CollisionRequest& request,
                         CollisionResult& result) const {
    return collide(o1, tf1, o2, tf2, request, result);
  }
  bool operator==(const ComputeCollision& other) const { return o1 == other.o1 && o2 == other.o2; }
  bool operator!=(const ComputeCollision& other) const { return !(*this == other); }

 protected:
  const CollisionGeometry* o1;
  const CollisionGeometry* o2;
};
class ComputeDistance {
 public:
  ComputeDistance(const CollisionGeometry* o1_, const CollisionGeometry* o2_) : o1(o1_), o2(o2_) {
    if (amd::is_octree(o1) || amd::is_octree(o2) ? !amd::octree_distance_pair_supported(o1, o2)
                                                 : !hfcl_pair_supported(o1->getNodeType(), o2->getNodeType(), 1))
      throw std::invalid_argument("Distance function between the two node types is not yet supported.");
  }
  virtual ~ComputeDistance() {}
  FCL_REAL operator()(const Transform3f& tf1, const Transform3f& tf2, const DistanceRequest& request,
                      DistanceResult& result) const {
    return distance(o1, tf1, o2, tf2, request, result);
  }
  bool operator==(const ComputeDistance& other) const { return o1 == other.o1 && o2 == other.o2; }
  bool operator!=(const ComputeDistance& other) const { return !(*this == other); }

 protected:
  const CollisionGeometry* o1;
  const CollisionGeometry* o2;
};

// ---------------------------------------------------------------------------------------------
// Contact patches (hpp-fcl 3.0: include/hpp/fcl/contact_patch.h, collision_data.h:519-981), forwarded to
// hfcl_contact_patch_batch on the thread's default context: one patch per contact of the collision result.
// ---------------------------------------------------------------------------------------------
struct ContactPatchRequest {  // collision_data.h:726-823
  size_t max_num_patch;
  explicit ContactPatchRequest(size_t max_num_patch_ = 1, size_t num_samples_curved_shapes = 12, FCL_REAL patch_tolerance = 1e-3)
      : max_num_patch(max_num_patch_) {
    setNumSamplesCurvedShapes(num_samples_curved_shapes);
    setPatchTolerance(patch_tolerance);
  }
  void setNumSamplesCurvedShapes(size_t n) { ns_ = n < 3 ? 3 : n; }
  size_t getNumSamplesCurvedShapes() const { return ns_; }
  void setPatchTolerance(FCL_REAL t) { tol_ = t < 0 ? 1e-12 : t; }
  FCL_REAL getPatchTolerance() const { return tol_; }

 private:
  size_t ns_ = 12;
  FCL_REAL tol_ = 1e-3;
};

struct ContactPatch {  // collision_data.h:519-717: frame (z = normal), depth, 2-D points in the frame
  enum PatchDirection { DEFAULT = 0, INVERTED = 1 };
  Transform3f tf;
  PatchDirection direction = DEFAULT;
  FCL_REAL penetration_depth = 0;
  std::vector<std::array<FCL_REAL, 2>> m_points;
  size_t size() const { return m_points.size(); }
  Vec3f getNormal() const {
    const Matrix3f& R = tf.getRotation();
    const Vec3f n(R(0, 2), R(1, 2), R(2, 2));
    return direction == INVERTED ? -n : n;
  }
  void addPoint(const Vec3f& p) {  // tf.inverseTransform(p).head<2>()
    const Matrix3f& R = tf.getRotation();
    const Vec3f d = p - tf.getTranslation();
    m_points.push_back({{R(0, 0) * d[0] + R(1, 0) * d[1] + R(2, 0) * d[2], R(0, 1) * d[0] + R(1, 1) * d[1] + R(2, 1) * d[2]}});
  }
  Vec3f getPoint(size_t i) const {
    if (m_points.empty()) throw std::logic_error("Patch is empty.");
    const auto& q = m_points[i < m_points.size() ? i : m_points.size() - 1];
    return tf.transform(Vec3f(q[0], q[1], 0));
  }
  Vec3f getPointShape1(size_t i) const { return getPoint(i) - getNormal() * (penetration_depth / 2); }
  Vec3f getPointShape2(size_t i) const { return getPoint(i) + getNormal() * (penetration_depth / 2); }
  bool isSame(const ContactPatch& other, FCL_REAL tol = 1e-12) const {  // collision_data.h:660-704
    auto approx = [tol](const Vec3f& a, const Vec3f& b) { return (a - b).norm() <= tol * std::min(a.norm(), b.norm()); };
    if (!approx(getNormal(), other.getNormal())) return false;
    if (std::abs(penetration_depth - other.penetration_depth) > tol || direction != other.direction || size() != other.size()) return false;
    for (size_t i = 0; i < size(); ++i) {
      bool found = false;
      for (size_t j = 0; j < other.size(); ++j) found = found || approx(getPoint(i), other.getPoint(j));
      if (!found) return false;
    }
    return true;
  }
};

struct ContactPatchResult {  // collision_data.h:826-981
  ContactPatchResult() {}
  explicit ContactPatchResult(const ContactPatchRequest&) {}
  size_t numContactPatches() const { return patches.size(); }
  const ContactPatch& getContactPatch(size_t i) const {
    if (patches.empty()) throw std::invalid_argument("The number of contact patches is zero. No ContactPatch can be returned.");
    return patches[i < patches.size() ? i : patches.size() - 1];
  }
  void clear() { patches.clear(); }
  void set(const ContactPatchRequest&) { clear(); }
  std::vector<ContactPatch> patches;
};

/// hpp::fcl::computeContactPatch (src/contact_patch.cpp:48-97) on the records of the contacts in `collision_result`.
inline void computeContactPatch(const CollisionGeometry* o1, const Transform3f& tf1, const CollisionGeometry* o2,
                                const Transform3f& tf2, const CollisionResult& collision_result, const ContactPatchRequest& request,
                                ContactPatchResult& result) {
  if (!collision_result.isCollision() || request.max_num_patch == 0) return;
  result.set(request);
  if (!hfcl_patch_supported(o1->getNodeType(), o2->getNodeType()))
    throw std::invalid_argument("Contact patch computation between these node types is not yet supported.");
  amd::BatchQueries& ctx = amd::default_context();
  const uint32_t i1 = ctx.add(o1), i2 = ctx.add(o2);
  hfcl_lib* lib = ctx.library();
  const size_t n = std::min(request.max_num_patch, collision_result.numContacts());
  std::vector<uint32_t> s1(n, i1), s2(n, i2);
  std::vector<Transform3f> t1(n, tf1), t2(n, tf2);
  std::vector<hfcl_result> rec(n);
  std::vector<hfcl_guess> guess(n);
  for (size_t k = 0; k < n; ++k) {
    const Contact& c = collision_result.getContact(k);
    hfcl_result& r = rec[k];
    std::memset(&r, 0, sizeof(r));
    r.distance = c.penetration_depth;
    for (int d = 0; d < 3; ++d) {
      r.normal[d] = c.normal[d];
      r.p1[d] = c.nearest_points[0][d];
      r.p2[d] = c.nearest_points[1][d];
    }
    r.b1 = c.b1;
    r.b2 = c.b2;
    r.num_contacts = 1;
    std::memset(&guess[k], 0, sizeof(hfcl_guess));
    guess[k].support_guess[0] = collision_result.cached_support_func_guess[0];
    guess[k].support_guess[1] = collision_result.cached_support_func_guess[1];
  }
  hfcl_patch_request preq;
  preq.max_num_patch = static_cast<uint32_t>(request.max_num_patch);
  preq.num_samples_curved_shapes = static_cast<uint32_t>(request.getNumSamplesCurvedShapes());
  preq.patch_tolerance = request.getPatchTolerance();
  uint32_t cap = 0;
  int rc = hfcl_contact_patch_max_points(lib, &preq, &cap);
  if (rc) amd::throw_for(rc);
  std::vector<hfcl_contact_patch> out(n);
  std::vector<double> pts(n * size_t(cap) * 2);
  rc = hfcl_contact_patch_batch(lib, s1.data(), s2.data(), reinterpret_cast<const double*>(t1.data()),
                                reinterpret_cast<const double*>(t2.data()), rec.data(), guess.data(), n, &preq, cap, out.data(),
                                pts.data());
  if (rc) amd::throw_for(rc);
  for (size_t k = 0; k < n; ++k) {
    ContactPatch p;
    Matrix3f R;
    for (int i = 0; i < 9; ++i) R.m[i] = out[k].tf[i];
    p.tf = Transform3f(R, Vec3f(out[k].tf[9], out[k].tf[10], out[k].tf[11]));
    p.penetration_depth = out[k].penetration_depth;
    for (uint32_t j = 0; j < out[k].num_points; ++j) p.m_points.push_back({{pts[(k * cap + j) * 2], pts[(k * cap + j) * 2 + 1]}});
    result.patches.push_back(p);
  }
}

/// ComputeContactPatch (include/hpp/fcl/contact_patch.h): the pair is checked once at construction.
class ComputeContactPatch {
 public:
  ComputeContactPatch(const CollisionGeometry* o1, const CollisionGeometry* o2) : o1_(o1), o2_(o2) {
    if (!hfcl_patch_supported(o1->getNodeType(), o2->getNodeType()))
      throw std::invalid_argument("Contact patch computation between these node types is not yet supported.");
  }
  void operator()(const Transform3f& tf1, const Transform3f& tf2, const CollisionResult& collision_result,
                  const ContactPatchRequest& request, ContactPatchResult& result) const {
    computeContactPatch(o1_, tf1, o2_, tf2, collision_result, request, result);
  }

 private:
  const CollisionGeometry* o1_;
  const CollisionGeometry* o2_;
};

// ---------------------------------------------------------------------------------------------
// Broadphase hand-off (include/hpp/fcl/collision_object.h:215-357, broadphase/broadphase_callbacks.h,
// broadphase/default_broadphase_callbacks.h:200-230, broadphase/broadphase_dynamic_AABB_tree.h).
// ---------------------------------------------------------------------------------------------
class CollisionObject {
 public:
  CollisionObject(const std::shared_ptr<CollisionGeometry>& g, const Transform3f& tf = Transform3f()) : cgeom(g), t(tf) {}
  const std::shared_ptr<CollisionGeometry>& collisionGeometry() const { return cgeom; }
  const CollisionGeometry* collisionGeometryPtr() const { return cgeom.get(); }
  const Transform3f& getTransform() const { return t; }
  void setTransform(const Transform3f& tf) { t = tf; }
  const AABB& getAABB() const { return aabb; }
  AABB& getAABB() { return aabb; }

 private:
  std::shared_ptr<CollisionGeometry> cgeom;
  Transform3f t;
  AABB aabb;
};

// collide() / distance() on CollisionObjects (src/collision.cpp:60-67, src/distance.cpp:51-58)
inline std::size_t collide(const CollisionObject* o1, const CollisionObject* o2, const CollisionRequest& request,
                           CollisionResult& result) {
  return collide(o1->collisionGeometryPtr(), o1->getTransform(), o2->collisionGeometryPtr(), o2->getTransform(), request, result);
}
inline FCL_REAL distance(const CollisionObject* o1, const CollisionObject* o2, const DistanceRequest& request,
                         DistanceResult& result) {
  return distance(o1->collisionGeometryPtr(), o1->getTransform(), o2->collisionGeometryPtr(), o2->getTransform(), request, result);
}

struct CollisionCallBackBase {  // broadphase/broadphase_callbacks.h:52-75
  virtual ~CollisionCallBackBase() {}
  virtual void init() {}
  virtual bool collide(CollisionObject* o1, CollisionObject* o2) = 0;
  bool operator()(CollisionObject* o1, CollisionObject* o2) { return collide(o1, o2); }
};

struct CollisionCallBackCollect : CollisionCallBackBase {  // default_broadphase_callbacks.h:200-230
  typedef std::pair<CollisionObject*, CollisionObject*> CollisionPair;
  explicit CollisionCallBackCollect(size_t max_size_) : max_size(max_size_) { collision_pairs.reserve(max_size_); }
  bool collide(CollisionObject* o1, CollisionObject* o2) override {
    collision_pairs.push_back(std::make_pair(o1, o2));
    return false;
  }
  void init() override { collision_pairs.clear(); }
  size_t numCollisionPairs() const { return collision_pairs.size(); }
  const std::vector<CollisionPair>& getCollisionPairs() const { return collision_pairs; }
  bool exist(const CollisionPair& p) const {
    for (const auto& q : collision_pairs)
      if ((q.first == p.first && q.second == p.second) || (q.first == p.second && q.second == p.first)) return true;
    return false;
  }

 protected:
  std::vector<CollisionPair> collision_pairs;
  size_t max_size;
};

struct DistanceCallBackBase {  // broadphase/broadphase_callbacks.h:77-103
  virtual ~DistanceCallBackBase() {}
  virtual void init() {}
  virtual bool distance(CollisionObject* o1, CollisionObject* o2, FCL_REAL& dist) = 0;
  bool operator()(CollisionObject* o1, CollisionObject* o2, FCL_REAL& dist) { return distance(o1, o2, dist); }
};

/// CollisionData / DistanceData and the default callbacks (broadphase/default_broadphase_callbacks.h:55-98,118,192;
/// src/broadphase/default_broadphase_callbacks.cpp:43-91).  Called directly, a default callback evaluates its pair with
/// collide() / distance(): one query = one batch of one, tens of microseconds of launch latency where the reference
/// spends two.  Handed to DynamicAABBTreeCollisionManager::collide / distance, the manager recognises the default
/// callbacks and evaluates the culled pairs in device batches (geometrically growing: 256, 1024, ... pairs), then folds
/// the records into the callback's CollisionData / DistanceData in the order, and with the stop rule, of the sequential
/// calls: same result object, a fraction of a microsecond per pair (tests/cpp/test_compat.cpp measures both).
struct CollisionData {
  CollisionData() : done(false) {}
  CollisionRequest request;
  CollisionResult result;
  bool done;  // the broadphase evaluation stops when set
  void clear() {
    result.clear();
    done = false;
  }
};
struct DistanceData {
  DistanceData() : done(false) {}
  DistanceRequest request;
  DistanceResult result;
  bool done;
  void clear() {
    result.clear();
    done = false;
  }
};
inline bool defaultCollisionFunction(CollisionObject* o1, CollisionObject* o2, void* data) {
  CollisionData* cd = static_cast<CollisionData*>(data);
  if (cd->done) return true;
  collide(o1, o2, cd->request, cd->result);
  if (cd->result.isCollision() && cd->result.numContacts() >= cd->request.num_max_contacts) cd->done = true;
  return cd->done;
}
inline bool defaultDistanceFunction(CollisionObject* o1, CollisionObject* o2, void* data, FCL_REAL& dist) {
  DistanceData* cd = static_cast<DistanceData*>(data);
  if (cd->done) {
    dist = cd->result.min_distance;
    return true;
  }
  distance(o1, o2, cd->request, cd->result);
  dist = cd->result.min_distance;
  if (dist <= 0) return true;  // in collision or in touch
  return cd->done;
}
struct CollisionCallBackDefault : CollisionCallBackBase {
  void init() override { data.clear(); }
  bool collide(CollisionObject* o1, CollisionObject* o2) override { return defaultCollisionFunction(o1, o2, &data); }
  CollisionData data;
};
struct DistanceCallBackDefault : DistanceCallBackBase {
  void init() override { data.clear(); }
  bool distance(CollisionObject* o1, CollisionObject* o2, FCL_REAL& dist) override { return defaultDistanceFunction(o1, o2, &data, dist); }
  DistanceData data;
};

/// Same calls as the reference manager (registerObject(s) / setup / update / collide(callback));
/// the candidate set is identical (all AABB-overlapping pairs), produced by the host pair-list
/// builder behind hfcl_broadphase_self_pairs instead of an incremental tree.
class DynamicAABBTreeCollisionManager {
 public:
  void registerObject(CollisionObject* obj) { objs_.push_back(obj); dirty_ = true; }
  void registerObjects(const std::vector<CollisionObject*>& v) { objs_.insert(objs_.end(), v.begin(), v.end()); dirty_ = true; }
  void unregisterObject(CollisionObject* obj) {
    objs_.erase(std::remove(objs_.begin(), objs_.end(), obj), objs_.end());
    dirty_ = true;
  }
  void clear() { objs_.clear(); dirty_ = true; }
  size_t size() const { return objs_.size(); }
  bool empty() const { return objs_.empty(); }
  void getObjects(std::vector<CollisionObject*>& out) const { out = objs_; }
  void setup() { refresh(); }
  void update() { dirty_ = true; refresh(); }

  /// self collision: callback on every pair with overlapping AABBs, until it returns true
  void collide(CollisionCallBackBase* callback) {
    callback->init();
    refresh();
    if (objs_.size() < 2) return;
    hfcl_pairlist* pl = hfcl_broadphase_self_pairs(aabbs_.data(), objs_.size(), 0);
    const uint32_t* p = hfcl_pairlist_data(pl);
    const size_t n = hfcl_pairlist_size(pl);
    struct Free { hfcl_pairlist* l; ~Free() { hfcl_pairlist_free(l); } } guard{pl};
    auto at = [&](size_t k) { return std::make_pair(objs_[p[2 * k]], objs_[p[2 * k + 1]]); };
    if (collide_default_batched(callback, n, at)) return;
    for (size_t k = 0; k < n; ++k)
      if ((*callback)(objs_[p[2 * k]], objs_[p[2 * k + 1]])) break;
  }
  /// self distance (broadphase_dynamic_AABB_tree.cpp:745-751): the callback sees the pairs whose AABBs are closer than the
  /// smallest distance reported so far (the pruning rule of distanceRecurse, :350-420), nearest boxes first, until it
  /// returns true.  The reference visits them in tree order; the minimum a callback accumulates is the same.
  void distance(DistanceCallBackBase* callback) {
    callback->init();
    refresh();
    const size_t n = objs_.size();
    std::vector<std::pair<FCL_REAL, std::pair<uint32_t, uint32_t>>> cand;
    cand.reserve(n * (n - 1) / 2);
    for (size_t i = 0; i < n; ++i)
      for (size_t j = i + 1; j < n; ++j) cand.push_back({aabb_distance(i, j), {uint32_t(i), uint32_t(j)}});
    std::sort(cand.begin(), cand.end());
    FCL_REAL min_dist = std::numeric_limits<FCL_REAL>::max();
    if (auto* def = dynamic_cast<DistanceCallBackDefault*>(callback)) {
      if (typeid(*callback) == typeid(DistanceCallBackDefault) && def->data.request.gjk_initial_guess != CachedGuess) {
        // the default callback: the candidates in device batches, folded in the sequential order with the sequential rules
        DistanceData& d = def->data;
        amd::BatchQueries& ctx = amd::default_context();
        size_t k = 0, batch = 256;
        while (k < cand.size() && !d.done && cand[k].first < min_dist) {
          size_t m = 0;  // candidates of this batch: those the sequential walk could still look at
          std::vector<std::pair<uint32_t, uint32_t>> ids;
          std::vector<Transform3f> tf1, tf2;
          while (k + m < cand.size() && m < batch && cand[k + m].first < min_dist) {
            CollisionObject *a = objs_[cand[k + m].second.first], *b = objs_[cand[k + m].second.second];
            ids.push_back({ctx.add(a->collisionGeometryPtr()), ctx.add(b->collisionGeometryPtr())});
            tf1.push_back(a->getTransform());
            tf2.push_back(b->getTransform());
            ++m;
          }
          ctx.run(ids, tf1, tf2, nullptr, &d.request);
          bool stop = false;
          for (size_t j = 0; j < m && !stop; ++j) {
            if (cand[k + j].first >= min_dist) { stop = true; break; }  // no closer pair can be left
            if (!(d.result.min_distance <= 0)) ctx.fill(d.result, ids[j], ctx.records()[j], ctx.guesses()[j]);  // distance(): isSatisfied
            min_dist = d.result.min_distance;
            if (min_dist <= 0) stop = true;  // in collision or in touch
          }
          if (stop) return;
          k += m;
          batch = std::min<size_t>(batch * 4, size_t(1) << 20);
        }
        return;
      }
    }
    for (const auto& c : cand) {
      if (c.first >= min_dist) break;  // no closer pair can be left
      if ((*callback)(objs_[c.second.first], objs_[c.second.second], min_dist)) break;
    }
  }
  /// against another manager (broadphase_dynamic_AABB_tree.cpp:734-743)
  void collide(DynamicAABBTreeCollisionManager* other, CollisionCallBackBase* callback) {
    callback->init();
    refresh();
    other->refresh();
    if (objs_.empty() || other->objs_.empty()) return;
    hfcl_pairlist* pl = hfcl_broadphase_pairs_between(aabbs_.data(), objs_.size(), other->aabbs_.data(), other->objs_.size(), 0);
    const uint32_t* p = hfcl_pairlist_data(pl);
    const size_t n = hfcl_pairlist_size(pl);
    struct Free { hfcl_pairlist* l; ~Free() { hfcl_pairlist_free(l); } } guard{pl};
    auto at = [&](size_t k) { return std::make_pair(objs_[p[2 * k]], other->objs_[p[2 * k + 1]]); };
    if (collide_default_batched(callback, n, at)) return;
    for (size_t k = 0; k < n; ++k)
      if ((*callback)(objs_[p[2 * k]], other->objs_[p[2 * k + 1]])) break;
  }

 private:
  /// The default collision callback over a list of culled pairs, evaluated in device batches.  Returns false (nothing
  /// done) for any other callback -- a user callback sees its pairs one by one -- and for requests that chain the GJK guess
  /// from pair to pair (CachedGuess: QueryRequest::updateGuess makes pair k depend on pair k - 1).
  /// Sequential semantics kept: records are folded in pair order by the same routine collide() uses, and nothing is
  /// folded once data.done is set (default_broadphase_callbacks.cpp:43-57); pairs of a batch beyond that point were
  /// evaluated for nothing, which is why the batches start small and grow.
  template <class At>
  bool collide_default_batched(CollisionCallBackBase* callback, size_t n, At at) {
    auto* def = dynamic_cast<CollisionCallBackDefault*>(callback);
    if (!def || typeid(*callback) != typeid(CollisionCallBackDefault)) return false;
    CollisionData& d = def->data;
    if (d.request.gjk_initial_guess == CachedGuess) return false;
    if (d.request.security_margin == -std::numeric_limits<FCL_REAL>::infinity() || d.request.num_max_contacts == 0) return false;
    amd::BatchQueries& ctx = amd::default_context();
    size_t k = 0, batch = 256;
    while (k < n && !d.done) {
      const size_t m = std::min(batch, n - k);
      std::vector<std::pair<uint32_t, uint32_t>> ids(m);
      std::vector<Transform3f> tf1(m), tf2(m);
      for (size_t j = 0; j < m; ++j) {
        const auto pr = at(k + j);
        ids[j] = {ctx.add(pr.first->collisionGeometryPtr()), ctx.add(pr.second->collisionGeometryPtr())};
        tf1[j] = pr.first->getTransform();
        tf2[j] = pr.second->getTransform();
      }
      ctx.run(ids, tf1, tf2, &d.request, nullptr);
      for (size_t j = 0; j < m && !d.done; ++j) {
        if (!(d.result.isCollision() && d.request.num_max_contacts <= d.result.numContacts()))  // collide()'s early return
          ctx.fill(d.result, ids[j], d.request, ctx.records()[j], ctx.guesses()[j]);
        if (d.result.isCollision() && d.result.numContacts() >= d.request.num_max_contacts) d.done = true;
      }
      k += m;
      batch = std::min<size_t>(batch * 4, size_t(1) << 20);
    }
    return true;
  }
  FCL_REAL aabb_distance(size_t i, size_t j) const {  // AABB::distance (BV/AABB.cpp:53-110): 0 when the boxes overlap
    FCL_REAL s = 0;
    for (int k = 0; k < 3; ++k) {
      const FCL_REAL lo = aabbs_[6 * i + k] - aabbs_[6 * j + 3 + k], hi = aabbs_[6 * j + k] - aabbs_[6 * i + 3 + k];
      const FCL_REAL d = std::max(FCL_REAL(0), std::max(lo, hi));
      s += d * d;
    }
    return std::sqrt(s);
  }
  void refresh() {  // CollisionObject::computeAABB for every object (collision_object.h:259-276)
    if (!dirty_ && aabbs_.size() == 6 * objs_.size()) return;
    std::vector<hfcl_shape> shapes(objs_.size());
    std::vector<double> verts;
    std::vector<uint32_t> ids(objs_.size());
    std::vector<double> tf(12 * objs_.size());
    for (size_t i = 0; i < objs_.size(); ++i) {
      const CollisionGeometry* g = objs_[i]->collisionGeometryPtr();
      hfcl_shape s{};
      s.type = g->getNodeType();
      const ShapeBase* sb = dynamic_cast<const ShapeBase*>(g);
      s.swept_sphere_radius = sb ? sb->getSweptSphereRadius() : 0.0;
      switch (g->getNodeType()) {
        case GEOM_BOX: { auto* b = static_cast<const Box*>(g); for (int k = 0; k < 3; ++k) s.params[k] = b->halfSide[k]; break; }
        case GEOM_SPHERE: s.params[0] = static_cast<const Sphere*>(g)->radius; break;
        case GEOM_CAPSULE: { auto* c = static_cast<const Capsule*>(g); s.params[0] = c->radius; s.params[1] = c->halfLength; break; }
        case GEOM_CONE: { auto* c = static_cast<const Cone*>(g); s.params[0] = c->radius; s.params[1] = c->halfLength; break; }
        case GEOM_CYLINDER: { auto* c = static_cast<const Cylinder*>(g); s.params[0] = c->radius; s.params[1] = c->halfLength; break; }
        case GEOM_ELLIPSOID: { auto* e = static_cast<const Ellipsoid*>(g); for (int k = 0; k < 3; ++k) s.params[k] = e->radii[k]; break; }
        case GEOM_CONVEX: {
          auto* c = static_cast<const ConvexBase*>(g);
          s.num_points = c->num_points;
          s.vertex_offset = static_cast<uint32_t>(verts.size() / 3);
          for (const Vec3f& q : *c->points) verts.insert(verts.end(), q.data(), q.data() + 3);
          break;
        }
        case BV_OBBRSS: {  // a mesh enters the broadphase as the point set of its vertices (BVHModelBase::computeLocalAABB, BVH_model.cpp:782-800)
          auto* m = static_cast<const BVHModel<OBBRSS>*>(g);
          s.type = GEOM_CONVEX;
          s.num_points = m->num_vertices;
          s.vertex_offset = static_cast<uint32_t>(verts.size() / 3);
          for (const Vec3f& q : m->vertices) verts.insert(verts.end(), q.data(), q.data() + 3);
          break;
        }
        default: throw std::invalid_argument("unsupported node type");
      }
      shapes[i] = s;
      ids[i] = static_cast<uint32_t>(i);
      std::memcpy(&tf[12 * i], &objs_[i]->getTransform(), 12 * sizeof(double));
    }
    aabbs_.assign(6 * objs_.size(), 0.0);
    const int rc = hfcl_world_aabbs(shapes.data(), shapes.size(), verts.data(), ids.data(), tf.data(), objs_.size(), aabbs_.data(), 0);
    if (rc) amd::throw_for(rc);
    for (size_t i = 0; i < objs_.size(); ++i) {
      AABB& a = objs_[i]->getAABB();
      a.min_ = Vec3f(aabbs_[6 * i], aabbs_[6 * i + 1], aabbs_[6 * i + 2]);
      a.max_ = Vec3f(aabbs_[6 * i + 3], aabbs_[6 * i + 4], aabbs_[6 * i + 5]);
    }
    dirty_ = false;
  }
  std::vector<CollisionObject*> objs_;
  std::vector<double> aabbs_;
  bool dirty_ = true;
};

namespace amd {
/// Evaluate the pairs a CollisionCallBackCollect holds in ONE device batch: results[i] belongs to
/// pairs[i] (each with its own CollisionResult, see SURVEY.md 8e on accumulation).
inline void collide(const std::vector<CollisionCallBackCollect::CollisionPair>& pairs, const CollisionRequest& request,
                    std::vector<CollisionResult>& results, BatchQueries& ctx = default_context()) {
  std::vector<std::pair<uint32_t, uint32_t>> ids(pairs.size());
  std::vector<Transform3f> tf1(pairs.size()), tf2(pairs.size());
  for (size_t i = 0; i < pairs.size(); ++i) {
    ids[i] = {ctx.add(pairs[i].first->collisionGeometryPtr()), ctx.add(pairs[i].second->collisionGeometryPtr())};
    tf1[i] = pairs[i].first->getTransform();
    tf2[i] = pairs[i].second->getTransform();
  }
  ctx.collide(ids, tf1, tf2, request, results);
}

/// A scene (hfcl_scene_*, include/hppfcl_amd.h): CollisionObjects and a list of object pairs -- what a broadphase pass collected, or what a
/// robot model fixes -- kept on the device; a query evaluates the list for one or many tables of object transforms.  Every transform
/// crosses the host link once per configuration instead of once per pair, and a caller that only wants the default callbacks' answer
/// asks for the summaries alone (hfcl_scene_summary: n_contacts > 0 is CollisionCallBackDefault's isCollision(), min_distance of a
/// distance query DistanceCallBackDefault's answer).
///   manager.collide(&collect);                                        // host broadphase
///   amd::Scene scene(objects, collect.getCollisionPairs());           // once per pair list
///   scene.collide(tables, n_conf, request, nullptr, &summaries);      // per batch of configurations
/// Runs on the first device of the context.  One contact per pair (contact lists of mesh pairs go through amd::collide).  The scene must
/// be destroyed before its context, and the context must not be reset() while the scene lives; geometries added to the context later are
/// followed (the scene is re-created on the next query).
class Scene {
 public:
  Scene(const std::vector<CollisionObject*>& objects, const std::vector<std::pair<size_t, size_t>>& pairs, BatchQueries& ctx = default_context())
      : ctx_(ctx), objects_(objects) {
    pairs_.reserve(2 * pairs.size());
    for (const auto& p : pairs) {
      if (p.first >= objects.size() || p.second >= objects.size()) throw std::invalid_argument("Scene: pair index outside the objects");
      pairs_.push_back(static_cast<uint32_t>(p.first));
      pairs_.push_back(static_cast<uint32_t>(p.second));
    }
    init();
  }
  /// ... from the pairs a CollisionCallBackCollect holds (every object of a pair must be one of `objects`)
  Scene(const std::vector<CollisionObject*>& objects, const std::vector<CollisionCallBackCollect::CollisionPair>& pairs,
        BatchQueries& ctx = default_context())
      : ctx_(ctx), objects_(objects) {
    std::map<const CollisionObject*, uint32_t> index;
    for (size_t i = 0; i < objects.size(); ++i) index.emplace(objects[i], static_cast<uint32_t>(i));
    pairs_.reserve(2 * pairs.size());
    for (const auto& p : pairs) {
      auto a = index.find(p.first), b = index.find(p.second);
      if (a == index.end() || b == index.end()) throw std::invalid_argument("Scene: a collected pair holds an object that is not in the scene");
      pairs_.push_back(a->second);
      pairs_.push_back(b->second);
    }
    init();
  }
  ~Scene() { hfcl_scene_destroy(scene_); }
  Scene(const Scene&) = delete;
  Scene& operator=(const Scene&) = delete;
  size_t numObjects() const { return objects_.size(); }
  size_t numPairs() const { return pairs_.size() / 2; }

  /// The objects' current transforms: one configuration.  results: nullptr or numPairs() results, results[p] what
  /// hpp::fcl::collide gives for pair p; summaries: nullptr or one record.  Not both nullptr.
  void collide(const CollisionRequest& request, std::vector<CollisionResult>* results, std::vector<hfcl_scene_summary>* summaries) {
    const std::vector<Transform3f> table = current();
    collide(table.data(), 1, request, results, summaries);
  }
  /// n_conf tables of numObjects() transforms each: results[c * numPairs() + p], summaries[c].
  void collide(const Transform3f* tables, size_t n_conf, const CollisionRequest& request, std::vector<CollisionResult>* results,
               std::vector<hfcl_scene_summary>* summaries) {
    ensure();
    const hfcl_collision_request a = to_abi(request);
    const size_t n = n_conf * numPairs();
    if (results) {
      rec_.resize(n);
      guess_.resize(n);
    }
    if (summaries) summaries->resize(n_conf);
    const int rc = hfcl_scene_collide(scene_, reinterpret_cast<const double*>(tables), n_conf, &a, results ? rec_.data() : nullptr,
                                      summaries ? summaries->data() : nullptr, nullptr, results ? guess_.data() : nullptr);
    if (rc) throw_for(rc);
    if (!results) return;
    results->assign(n, CollisionResult());
    for (size_t q = 0; q < n; ++q) {
      hfcl_result r = rec_[q];
      if (r.num_contacts > 1) r.num_contacts = 1;  // (a mesh pair under num_max_contacts > 1: the record holds its first contact)
      ctx_.fill((*results)[q], shape_pair(q % numPairs()), request, r, guess_[q]);
    }
  }
  void distance(const DistanceRequest& request, std::vector<DistanceResult>* results, std::vector<hfcl_scene_summary>* summaries) {
    const std::vector<Transform3f> table = current();
    distance(table.data(), 1, request, results, summaries);
  }
  void distance(const Transform3f* tables, size_t n_conf, const DistanceRequest& request, std::vector<DistanceResult>* results,
                std::vector<hfcl_scene_summary>* summaries) {
    ensure();
    const hfcl_distance_request a = to_abi(request);
    const size_t n = n_conf * numPairs();
    if (results) {
      rec_.resize(n);
      guess_.resize(n);
    }
    if (summaries) summaries->resize(n_conf);
    const int rc = hfcl_scene_distance(scene_, reinterpret_cast<const double*>(tables), n_conf, &a, results ? rec_.data() : nullptr,
                                       summaries ? summaries->data() : nullptr, nullptr, results ? guess_.data() : nullptr);
    if (rc) throw_for(rc);
    if (!results) return;
    results->assign(n, DistanceResult());
    for (size_t q = 0; q < n; ++q) ctx_.fill((*results)[q], shape_pair(q % numPairs()), rec_[q], guess_[q]);
  }
  const std::vector<hfcl_result>& records() const { return rec_; }

  /// The pair list culled per configuration on the device (hfcl_scene_cull, include/hppfcl_amd_cull.h): the queries
  /// q = c * numPairs() + p whose two world AABBs, each grown by `inflate` >= 0 on every side, overlap -- with inflate = 0 the pairs
  /// DynamicAABBTreeCollisionManager::collide passes to its callback under configuration c.  query_ids: ascending;
  /// conf_begin (n_conf + 1 entries): configuration c owns query_ids[conf_begin[c] .. conf_begin[c + 1]).
  /// The outputs of the culled calls are sized by a guess (an eighth of the queries): one call, the tables cross the link once; a
  /// longer list is refused with its length before any narrow-phase work, and the call is made once more with that.
  void cull(const Transform3f* tables, size_t n_conf, double inflate, std::vector<uint64_t>& query_ids, std::vector<uint64_t>& conf_begin) {
    ensure();
    conf_begin.assign(n_conf + 1, 0);
    size_t n = 0, capacity = list_guess(n_conf);
    for (int attempt = 0;; ++attempt) {
      query_ids.assign(capacity, 0);
      const int rc = hfcl_scene_cull(scene_, reinterpret_cast<const double*>(tables), n_conf, inflate, query_ids.data(), capacity, conf_begin.data(), &n);
      if (rc == HFCL_ERR_LIMIT && attempt == 0 && n > capacity) {
        capacity = n;
        continue;
      }
      if (rc) throw_for(rc);
      break;
    }
    query_ids.resize(n);
  }
  /// collide() on the culled list: results[k] (nullptr: summaries only) is what hpp::fcl::collide gives for query query_ids[k];
  /// summaries[c] folds configuration c's surviving pairs (n_contacts and first_contact as without the cull when inflate = 0).
  void collideCulled(const Transform3f* tables, size_t n_conf, double inflate, const CollisionRequest& request,
                     std::vector<CollisionResult>* results, std::vector<uint64_t>& query_ids, std::vector<uint64_t>& conf_begin,
                     std::vector<hfcl_scene_summary>* summaries) {
    ensure();
    const hfcl_collision_request a = to_abi(request);
    const size_t n = culled(tables, n_conf, results != nullptr, query_ids, conf_begin, summaries, [&](size_t capacity, size_t* listed) {
      return hfcl_scene_collide_culled(scene_, reinterpret_cast<const double*>(tables), n_conf, inflate, &a, results ? rec_.data() : nullptr,
                                       capacity, query_ids.data(), conf_begin.data(), summaries ? summaries->data() : nullptr, nullptr,
                                       results ? guess_.data() : nullptr, listed);
    });
    if (!results) return;
    results->assign(n, CollisionResult());
    for (size_t k = 0; k < n; ++k) {
      hfcl_result r = rec_[k];
      if (r.num_contacts > 1) r.num_contacts = 1;
      ctx_.fill((*results)[k], shape_pair(query_ids[k] % numPairs()), request, r, guess_[k]);
    }
  }
  /// distance() on the culled list.  inflate = D / 2 keeps every pair whose boxes are within D along each axis: a box-shaped filter,
  /// not the manager's distance traversal with its shrinking bound.
  void distanceCulled(const Transform3f* tables, size_t n_conf, double inflate, const DistanceRequest& request,
                      std::vector<DistanceResult>* results, std::vector<uint64_t>& query_ids, std::vector<uint64_t>& conf_begin,
                      std::vector<hfcl_scene_summary>* summaries) {
    ensure();
    const hfcl_distance_request a = to_abi(request);
    const size_t n = culled(tables, n_conf, results != nullptr, query_ids, conf_begin, summaries, [&](size_t capacity, size_t* listed) {
      return hfcl_scene_distance_culled(scene_, reinterpret_cast<const double*>(tables), n_conf, inflate, &a, results ? rec_.data() : nullptr,
                                        capacity, query_ids.data(), conf_begin.data(), summaries ? summaries->data() : nullptr, nullptr,
                                        results ? guess_.data() : nullptr, listed);
    });
    if (!results) return;
    results->assign(n, DistanceResult());
    for (size_t k = 0; k < n; ++k) ctx_.fill((*results)[k], shape_pair(query_ids[k] % numPairs()), rec_[k], guess_[k]);
  }

  /// The self-collision pairs per configuration, made on the device without a list (hfcl_scene_self_pairs, include/hppfcl_amd_pairs.h):
  /// for configuration c, then i, then j ascending, every (i < j) whose two world AABBs, each grown by `inflate` >= 0, overlap -- with
  /// inflate = 0 the pairs DynamicAABBTreeCollisionManager::collide passes to its callback.  pairs: two object indices per entry;
  /// conf_begin (n_conf + 1 entries): configuration c owns the entries conf_begin[c] .. conf_begin[c + 1].  The scene's own pair list
  /// plays no part (a Scene made with an empty list serves).
  void selfPairs(const Transform3f* tables, size_t n_conf, double inflate, std::vector<uint32_t>& pairs, std::vector<uint64_t>& conf_begin) {
    ensure();
    listed(n_conf, false, pairs, conf_begin, nullptr, [&](size_t capacity, size_t* n) {
      return hfcl_scene_self_pairs(scene_, reinterpret_cast<const double*>(tables), n_conf, inflate, pairs.data(), capacity, conf_begin.data(), n);
    });
  }
  /// collide() on that list: results[k] (nullptr: summaries only) is what hpp::fcl::collide gives for entry k; summaries[c] folds
  /// configuration c's entries, min_pair and first_contact being RANKS inside the configuration: entry conf_begin[c] + rank.
  void collideSelf(const Transform3f* tables, size_t n_conf, double inflate, const CollisionRequest& request, std::vector<CollisionResult>* results,
                   std::vector<uint32_t>& pairs, std::vector<uint64_t>& conf_begin, std::vector<hfcl_scene_summary>* summaries) {
    ensure();
    const hfcl_collision_request a = to_abi(request);
    const size_t n = listed(n_conf, results != nullptr, pairs, conf_begin, summaries, [&](size_t capacity, size_t* count) {
      return hfcl_scene_collide_self(scene_, reinterpret_cast<const double*>(tables), n_conf, inflate, &a, results ? rec_.data() : nullptr, capacity,
                                     pairs.data(), conf_begin.data(), summaries ? summaries->data() : nullptr, nullptr,
                                     results ? guess_.data() : nullptr, count);
    });
    if (!results) return;
    results->assign(n, CollisionResult());
    for (size_t k = 0; k < n; ++k) {
      hfcl_result r = rec_[k];
      if (r.num_contacts > 1) r.num_contacts = 1;
      ctx_.fill((*results)[k], {shape_[pairs[2 * k]], shape_[pairs[2 * k + 1]]}, request, r, guess_[k]);
    }
  }
  void distanceSelf(const Transform3f* tables, size_t n_conf, double inflate, const DistanceRequest& request, std::vector<DistanceResult>* results,
                    std::vector<uint32_t>& pairs, std::vector<uint64_t>& conf_begin, std::vector<hfcl_scene_summary>* summaries) {
    ensure();
    const hfcl_distance_request a = to_abi(request);
    const size_t n = listed(n_conf, results != nullptr, pairs, conf_begin, summaries, [&](size_t capacity, size_t* count) {
      return hfcl_scene_distance_self(scene_, reinterpret_cast<const double*>(tables), n_conf, inflate, &a, results ? rec_.data() : nullptr, capacity,
                                      pairs.data(), conf_begin.data(), summaries ? summaries->data() : nullptr, nullptr,
                                      results ? guess_.data() : nullptr, count);
    });
    if (!results) return;
    results->assign(n, DistanceResult());
    for (size_t k = 0; k < n; ++k) ctx_.fill((*results)[k], {shape_[pairs[2 * k]], shape_[pairs[2 * k + 1]]}, rec_[k], guess_[k]);
  }

  /// Object groups and a group matrix for the lists of selfPairs / collideSelf / distanceSelf (hfcl_scene_set_groups,
  /// include/hppfcl_amd_groups.h): object_group[i] < collides.size() <= 64 for every object; bit h of collides[g] set = an object of
  /// group g and one of group h may be listed; the matrix must be symmetric.  Groups {0 .. 0, 1 .. 1} with collides {2, 1} give what
  /// DynamicAABBTreeCollisionManager::collide(otherManager, callback) collects; one group per link with the neighbours' bits cleared a
  /// robot's allowed-collision matrix.  The groups stay until clearGroups(), also when the scene is re-created.
  void setGroups(const std::vector<uint8_t>& object_group, const std::vector<uint64_t>& collides) {
    ensure();
    if (object_group.size() != objects_.size()) throw std::invalid_argument("Scene::setGroups: one group per object");
    const int rc = hfcl_scene_set_groups(scene_, object_group.data(), collides.size(), collides.data());
    if (rc) throw_for(rc);
    group_ = object_group;
    collides_ = collides;
  }
  void clearGroups() {
    ensure();
    const int rc = hfcl_scene_clear_groups(scene_);
    if (rc) throw_for(rc);
    group_.clear();
    collides_.clear();
  }
  size_t numGroups() const { return hfcl_scene_num_groups(scene_); }
  /// How the last list of selfPairs / collideSelf / distanceSelf was made (hfcl_scene_last_pairs_form, include/hppfcl_amd_pairs_sorted.h):
  /// 0 the tiled all-pairs test, 1 its wave-per-configuration form, 2 sort and sweep (library option scene_pairs_sorted); -1: none yet
  int lastPairsForm() const { return hfcl_scene_last_pairs_form(scene_); }

  /// A static environment kept on the device (hfcl_scene_set_environment, include/hppfcl_amd_env.h): objects [n_moving, numObjects())
  /// stand still at env_transforms (one per environment object); the calls below take tables of n_moving transforms a configuration.
  /// Put the moving objects first and the environment in a spatial order: a box per 256 consecutive environment objects decides what a
  /// sweep may skip.  The environment stays until clearEnvironment(), also when the scene is re-created.
  void setEnvironment(size_t n_moving, const std::vector<Transform3f>& env_transforms) {
    ensure();
    if (n_moving > objects_.size() || env_transforms.size() != objects_.size() - n_moving)
      throw std::invalid_argument("Scene::setEnvironment: one transform per object from n_moving on");
    const int rc = hfcl_scene_set_environment(scene_, n_moving, reinterpret_cast<const double*>(env_transforms.data()));
    if (rc) throw_for(rc);
    env_ = env_transforms;
    n_moving_ = n_moving;
    has_env_ = true;
  }
  void clearEnvironment() {
    ensure();
    const int rc = hfcl_scene_clear_environment(scene_);
    if (rc) throw_for(rc);
    env_.clear();
    has_env_ = false;
  }
  size_t numMoving() const { return hfcl_scene_n_moving(scene_); }
  /// selfPairs / collideSelf / distanceSelf for a scene with an environment: the list of the full tables -- moving_tables[c] followed
  /// by the environment -- less every entry whose first object is not a moving one (no environment x environment pair), from tables of
  /// numMoving() transforms a configuration.  j of an entry (i, j) is an index into the whole scene.
  void envPairs(const Transform3f* moving_tables, size_t n_conf, double inflate, std::vector<uint32_t>& pairs, std::vector<uint64_t>& conf_begin) {
    ensure();
    listed(n_conf, false, pairs, conf_begin, nullptr, [&](size_t capacity, size_t* n) {
      return hfcl_scene_env_pairs(scene_, reinterpret_cast<const double*>(moving_tables), n_conf, inflate, pairs.data(), capacity, conf_begin.data(), n);
    });
  }
  void collideEnv(const Transform3f* moving_tables, size_t n_conf, double inflate, const CollisionRequest& request,
                  std::vector<CollisionResult>* results, std::vector<uint32_t>& pairs, std::vector<uint64_t>& conf_begin,
                  std::vector<hfcl_scene_summary>* summaries) {
    ensure();
    const hfcl_collision_request a = to_abi(request);
    const size_t n = listed(n_conf, results != nullptr, pairs, conf_begin, summaries, [&](size_t capacity, size_t* count) {
      return hfcl_scene_collide_env(scene_, reinterpret_cast<const double*>(moving_tables), n_conf, inflate, &a, results ? rec_.data() : nullptr,
                                    capacity, pairs.data(), conf_begin.data(), summaries ? summaries->data() : nullptr, nullptr,
                                    results ? guess_.data() : nullptr, count);
    });
    if (!results) return;
    results->assign(n, CollisionResult());
    for (size_t k = 0; k < n; ++k) {
      hfcl_result r = rec_[k];
      if (r.num_contacts > 1) r.num_contacts = 1;
      ctx_.fill((*results)[k], {shape_[pairs[2 * k]], shape_[pairs[2 * k + 1]]}, request, r, guess_[k]);
    }
  }
  void distanceEnv(const Transform3f* moving_tables, size_t n_conf, double inflate, const DistanceRequest& request,
                   std::vector<DistanceResult>* results, std::vector<uint32_t>& pairs, std::vector<uint64_t>& conf_begin,
                   std::vector<hfcl_scene_summary>* summaries) {
    ensure();
    const hfcl_distance_request a = to_abi(request);
    const size_t n = listed(n_conf, results != nullptr, pairs, conf_begin, summaries, [&](size_t capacity, size_t* count) {
      return hfcl_scene_distance_env(scene_, reinterpret_cast<const double*>(moving_tables), n_conf, inflate, &a, results ? rec_.data() : nullptr,
                                     capacity, pairs.data(), conf_begin.data(), summaries ? summaries->data() : nullptr, nullptr,
                                     results ? guess_.data() : nullptr, count);
    });
    if (!results) return;
    results->assign(n, DistanceResult());
    for (size_t k = 0; k < n; ++k) ctx_.fill((*results)[k], {shape_[pairs[2 * k]], shape_[pairs[2 * k + 1]]}, rec_[k], guess_[k]);
  }

  /// The clearance per configuration (hfcl_scene_nearest, include/hppfcl_amd_nearest.h): what DistanceCallBackDefault leaves behind
  /// after DynamicAABBTreeCollisionManager::distance -- the smallest distance over the listed pairs and the pair that has it --, with
  /// the pairs pruned by a bound from their world boxes instead of evaluated one by one.  summaries[c].min_distance / min_pair equal
  /// those of distance() wherever that minimum is <= upper_bound (+inf: always); elsewhere min_distance is some value above
  /// upper_bound, or +inf.  results: nullptr or one DistanceResult per configuration, filled from the closest pair's record (o1, o2,
  /// nearest points, normal, b1, b2); a configuration without an evaluated pair keeps a default DistanceResult.
  void nearest(const Transform3f* tables, size_t n_conf, const DistanceRequest& request, double upper_bound,
               std::vector<hfcl_scene_summary>& summaries, std::vector<DistanceResult>* results, size_t* n_evaluated = nullptr) {
    ensure();
    const hfcl_distance_request a = to_abi(request);
    summaries.resize(n_conf);
    if (results) rec_.resize(n_conf);
    const int rc = hfcl_scene_nearest(scene_, reinterpret_cast<const double*>(tables), n_conf, &a, upper_bound, summaries.data(),
                                      results ? rec_.data() : nullptr, n_evaluated);
    if (rc) throw_for(rc);
    if (!results) return;
    results->assign(n_conf, DistanceResult());
    hfcl_guess g;
    std::memset(&g, 0, sizeof(g));
    g.gjk_guess[0] = 1.0;  // (DistanceResult's own default: no guess comes back from this call)
    for (size_t c = 0; c < n_conf; ++c)
      if (summaries[c].min_pair != 0xFFFFFFFFu) ctx_.fill((*results)[c], shape_pair(summaries[c].min_pair), rec_[c], g);
  }

  /// The clearance per configuration from the poses and the groups alone (hfcl_scene_nearest_self, include/hppfcl_amd_nearest_self.h):
  /// DynamicAABBTreeCollisionManager::distance(otherManager, DistanceCallBackDefault) -- the smallest distance over every pair of objects
  /// the groups allow (setGroups; none: all pairs) and the pair that has it, the pairs made and pruned on the device: no pair list, no
  /// inflate.  clearances[c].min_distance / min_i / min_j equal what distance() on the explicit list of all allowed pairs gives wherever
  /// that minimum is <= upper_bound (+inf: always); elsewhere min_distance is some value above upper_bound, or +inf.  results: nullptr or
  /// one DistanceResult per configuration, filled from the closest pair's record; a configuration without one keeps a default
  /// DistanceResult.
  void nearestSelf(const Transform3f* tables, size_t n_conf, const DistanceRequest& request, double upper_bound,
                   std::vector<hfcl_scene_clearance>& clearances, std::vector<DistanceResult>* results = nullptr, size_t* n_evaluated = nullptr) {
    ensure();
    const hfcl_distance_request a = to_abi(request);
    clearances.resize(n_conf);
    if (results) rec_.resize(n_conf);
    const int rc = hfcl_scene_nearest_self(scene_, reinterpret_cast<const double*>(tables), n_conf, &a, upper_bound, clearances.data(),
                                           results ? rec_.data() : nullptr, n_evaluated);
    if (rc) throw_for(rc);
    if (!results) return;
    results->assign(n_conf, DistanceResult());
    hfcl_guess g;
    std::memset(&g, 0, sizeof(g));
    g.gjk_guess[0] = 1.0;  // (DistanceResult's own default: no guess comes back from this call)
    for (size_t c = 0; c < n_conf; ++c)
      if (clearances[c].min_i != 0xFFFFFFFFu) ctx_.fill((*results)[c], {shape_[clearances[c].min_i], shape_[clearances[c].min_j]}, rec_[c], g);
  }

  /// nearestSelf for a scene with an environment set (hfcl_scene_nearest_env, include/hppfcl_amd_nearest_env.h): `moving` holds n_conf
  /// tables of the moving objects alone (hfcl_scene_n_moving rows each); the candidates are the allowed pairs with a moving object in
  /// them, never environment x environment; min_i / min_j index the full scene.  Outputs as nearestSelf.
  void nearestEnv(const Transform3f* moving, size_t n_conf, const DistanceRequest& request, double upper_bound,
                  std::vector<hfcl_scene_clearance>& clearances, std::vector<DistanceResult>* results = nullptr, size_t* n_evaluated = nullptr) {
    ensure();
    const hfcl_distance_request a = to_abi(request);
    clearances.resize(n_conf);
    if (results) rec_.resize(n_conf);
    const int rc = hfcl_scene_nearest_env(scene_, reinterpret_cast<const double*>(moving), n_conf, &a, upper_bound, clearances.data(),
                                          results ? rec_.data() : nullptr, n_evaluated);
    if (rc) throw_for(rc);
    if (!results) return;
    results->assign(n_conf, DistanceResult());
    hfcl_guess g;
    std::memset(&g, 0, sizeof(g));
    g.gjk_guess[0] = 1.0;  // (DistanceResult's own default: no guess comes back from this call)
    for (size_t c = 0; c < n_conf; ++c)
      if (clearances[c].min_i != 0xFFFFFFFFu) ctx_.fill((*results)[c], {shape_[clearances[c].min_i], shape_[clearances[c].min_j]}, rec_[c], g);
  }

  /// A height-field terrain under the moving objects (hfcl_scene_set_terrain, include/hppfcl_amd_terrain.h): `field` at `tf` is the ground
  /// under the objects listed in `objects` (strictly ascending indices), or under every moving object.  The field's heights are copied
  /// now and again after updateHeights(); the field must stay alive while it is the terrain.  A scene of the default context registers the
  /// field through the thread's default HeightFieldBatch, a scene of another context through a batch of its own.
  void setTerrain(const HeightField<AABB>* field, const Transform3f& tf, const std::vector<uint32_t>& objects) { set_terrain(field, tf, objects, false); }
  void setTerrain(const HeightField<AABB>* field, const Transform3f& tf) { set_terrain(field, tf, std::vector<uint32_t>(), true); }
  void clearTerrain() {
    ensure();
    const int rc = hfcl_scene_clear_terrain(scene_);
    if (rc) throw_for(rc);
    has_terrain_ = false;
    terrain_field_ = nullptr;
  }
  size_t numTerrainObjects() const { return hfcl_scene_n_terrain_objects(scene_); }
  /// The terrain against its listed objects for n_conf tables of numMoving() transforms each: query c * numTerrainObjects() + k is
  /// hpp::fcl::collide(field, tf, object o_k, moving_tables[c][o_k]).  results: nullptr or one fresh CollisionResult per query (every
  /// contact up to num_max_contacts, distance_lower_bound); summaries: nullptr or one record per configuration -- min_distance the
  /// smallest distance_lower_bound, min_pair / first_contact OBJECT indices, n_contacts > 0: isCollision() of the default callback.
  void collideTerrain(const Transform3f* moving_tables, size_t n_conf, const CollisionRequest& request, std::vector<CollisionResult>* results,
                      std::vector<hfcl_scene_summary>* summaries) {
    ensure();
    if (!has_terrain_) throw std::invalid_argument("Scene::collideTerrain: no terrain set");
    if (terrain_epoch_ != terrain_batch().epoch() || terrain_version_ != terrain_field_->version()) apply_terrain();
    const hfcl_collision_request a = to_abi(request);
    const size_t n_t = numTerrainObjects(), n = n_conf * n_t;
    if (summaries) summaries->resize(n_conf);
    if (!results) {
      const int rc = hfcl_scene_collide_terrain(scene_, reinterpret_cast<const double*>(moving_tables), n_conf, &a, nullptr, nullptr,
                                                summaries ? summaries->data() : nullptr, nullptr, 0, nullptr);
      if (rc == HFCL_ERR_LIMIT) throw std::invalid_argument(hfcl_last_error());
      if (rc) throw_for(rc);
      return;
    }
    rec_.resize(n);
    terrain_bound_.resize(n);
    size_t cap = std::max<size_t>(64, 4 * n), produced = 0;
    int rc = HFCL_OK;
    for (int attempt = 0; attempt < 2; ++attempt) {  // (a list that outgrew the guess: once more with the count)
      terrain_contacts_.resize(cap);
      rc = hfcl_scene_collide_terrain(scene_, reinterpret_cast<const double*>(moving_tables), n_conf, &a, rec_.data(), terrain_bound_.data(),
                                      summaries ? summaries->data() : nullptr, terrain_contacts_.data(), cap, &produced);
      if (rc || produced <= cap) break;
      cap = produced;
    }
    if (rc == HFCL_ERR_LIMIT) throw std::invalid_argument(hfcl_last_error());
    if (rc) throw_for(rc);
    terrain_contacts_.resize(std::min(produced, cap));
    results->assign(n, CollisionResult());
    std::vector<uint32_t> listed(terrain_objects_);
    if (terrain_all_) {
      listed.resize(n_t);
      for (size_t k = 0; k < n_t; ++k) listed[k] = static_cast<uint32_t>(k);
    }
    size_t k = 0;
    for (size_t q = 0; q < n; ++q)
      HeightFieldBatch::fill(terrain_contacts_, (*results)[q], rec_[q], terrain_bound_[q], terrain_field_,
                             objects_[listed[q % n_t]]->collisionGeometryPtr(), static_cast<uint32_t>(q), k, request);
  }
  const std::vector<double>& terrainBounds() const { return terrain_bound_; }
  const std::vector<hfcl_contact>& terrainContacts() const { return terrain_contacts_; }

 private:
  HeightFieldBatch& terrain_batch() {
    if (&ctx_ == &default_context()) return default_hfield_batch();
    if (!own_hfields_) own_hfields_.reset(new HeightFieldBatch(ctx_));
    return *own_hfields_;
  }
  void set_terrain(const HeightField<AABB>* field, const Transform3f& tf, const std::vector<uint32_t>& objects, bool all) {
    ensure();
    const HeightField<AABB>* old_field = terrain_field_;
    const Transform3f old_tf = terrain_tf_;
    std::vector<uint32_t> old_objects = objects;
    old_objects.swap(terrain_objects_);
    const bool old_all = terrain_all_, old_has = has_terrain_;
    terrain_field_ = field;
    terrain_tf_ = tf;
    terrain_all_ = all;
    try {
      apply_terrain();
    } catch (...) {  // (a refused terrain sets nothing: the one before stays)
      terrain_field_ = old_field;
      terrain_tf_ = old_tf;
      terrain_objects_.swap(old_objects);
      terrain_all_ = old_all;
      has_terrain_ = old_has;
      throw;
    }
    has_terrain_ = true;
  }
  void apply_terrain() {  // the device scene is there (ensure)
    HeightFieldBatch& hb = terrain_batch();
    const uint32_t index = hb.libraryIndex(hb.addField(terrain_field_));
    static const uint32_t none = 0;  // (an empty list is a non-null pointer and a count of 0)
    const int rc = hfcl_scene_set_terrain(scene_, index, reinterpret_cast<const double*>(&terrain_tf_),
                                          terrain_all_ ? nullptr : (terrain_objects_.empty() ? &none : terrain_objects_.data()), terrain_objects_.size());
    if (rc == HFCL_ERR_UNSUPPORTED_PAIR) throw std::invalid_argument(hfcl_last_error());
    if (rc) throw_for(rc);
    terrain_epoch_ = hb.epoch();
    terrain_version_ = terrain_field_->version();
  }
  size_t list_guess(size_t n_conf) const {
    const size_t total = n_conf * numPairs();
    return std::min(total, std::max<size_t>(total / 8, 1024));
  }
  // a culled call with outputs sized by the guess, repeated once with the list's length if that was too small; returns the length
  template <class Call>
  size_t culled(const Transform3f*, size_t n_conf, bool records, std::vector<uint64_t>& query_ids, std::vector<uint64_t>& conf_begin,
                std::vector<hfcl_scene_summary>* summaries, Call call) {
    conf_begin.assign(n_conf + 1, 0);
    if (summaries) summaries->resize(n_conf);
    size_t n = 0, capacity = list_guess(n_conf);
    for (int attempt = 0;; ++attempt) {
      query_ids.assign(capacity, 0);
      if (records) {
        rec_.resize(capacity);
        guess_.resize(capacity);
      }
      const int rc = call(capacity, &n);
      if (rc == HFCL_ERR_LIMIT && attempt == 0 && n > capacity) {
        capacity = n;
        continue;
      }
      if (rc) throw_for(rc);
      break;
    }
    query_ids.resize(n);
    return n;
  }
  // a self-pairs call with outputs sized by a guess (16 entries per configuration and object), repeated once with the list's length
  template <class Call>
  size_t listed(size_t n_conf, bool records, std::vector<uint32_t>& pairs, std::vector<uint64_t>& conf_begin,
                std::vector<hfcl_scene_summary>* summaries, Call call) {
    conf_begin.assign(n_conf + 1, 0);
    if (summaries) summaries->resize(n_conf);
    size_t n = 0, capacity = std::max<size_t>(16 * n_conf * numObjects(), 1024);
    for (int attempt = 0;; ++attempt) {
      pairs.assign(2 * capacity, 0);
      if (records) {
        rec_.resize(capacity);
        guess_.resize(capacity);
      }
      const int rc = call(capacity, &n);
      if (rc == HFCL_ERR_LIMIT && attempt == 0 && n > capacity) {
        capacity = n;
        continue;
      }
      if (rc) throw_for(rc);
      break;
    }
    pairs.resize(2 * n);
    return n;
  }
  void init() {
    shape_.resize(objects_.size());
    for (size_t i = 0; i < objects_.size(); ++i) shape_[i] = ctx_.add(objects_[i]->collisionGeometryPtr());
    ensure();
  }
  void ensure() {  // the device scene, made for the context's library as it is now
    hfcl_lib* lib = ctx_.library();
    if (scene_ && lib == lib_ && geometries_ == ctx_.numGeometries()) return;
    hfcl_scene_destroy(scene_);
    scene_ = hfcl_scene_create(lib, shape_.data(), shape_.size(), pairs_.data(), pairs_.size() / 2);
    if (!scene_) throw_for(HFCL_ERR_INVALID_ARGUMENT);
    lib_ = lib;
    geometries_ = ctx_.numGeometries();
    if (!collides_.empty()) {  // (the groups of the scene before)
      const int rc = hfcl_scene_set_groups(scene_, group_.data(), collides_.size(), collides_.data());
      if (rc) throw_for(rc);
    }
    if (has_env_) {  // (the environment of the scene before)
      const int rc = hfcl_scene_set_environment(scene_, n_moving_, reinterpret_cast<const double*>(env_.data()));
      if (rc) throw_for(rc);
    }
    if (has_terrain_) apply_terrain();  // (the terrain of the scene before)
  }
  std::vector<Transform3f> current() const {
    std::vector<Transform3f> t(objects_.size());
    for (size_t i = 0; i < objects_.size(); ++i) t[i] = objects_[i]->getTransform();
    return t;
  }
  std::pair<uint32_t, uint32_t> shape_pair(size_t p) const { return {shape_[pairs_[2 * p]], shape_[pairs_[2 * p + 1]]}; }
  BatchQueries& ctx_;
  std::vector<CollisionObject*> objects_;
  std::vector<uint32_t> shape_, pairs_;
  std::vector<uint8_t> group_;      // setGroups: kept for a scene made again
  std::vector<uint64_t> collides_;
  std::vector<Transform3f> env_;    // setEnvironment: kept for a scene made again
  size_t n_moving_ = 0;
  bool has_env_ = false;
  hfcl_scene* scene_ = nullptr;
  hfcl_lib* lib_ = nullptr;
  size_t geometries_ = 0;
  std::vector<hfcl_result> rec_;
  std::vector<hfcl_guess> guess_;
  const HeightField<AABB>* terrain_field_ = nullptr;  // setTerrain: kept for a scene made again, and for updated heights
  Transform3f terrain_tf_;
  std::vector<uint32_t> terrain_objects_;
  bool terrain_all_ = false, has_terrain_ = false;
  uint64_t terrain_epoch_ = 0;
  unsigned int terrain_version_ = 0;
  std::unique_ptr<HeightFieldBatch> own_hfields_;
  std::vector<double> terrain_bound_;
  std::vector<hfcl_contact> terrain_contacts_;
};
}  // namespace amd

}  // namespace fcl
}  // namespace hpp
