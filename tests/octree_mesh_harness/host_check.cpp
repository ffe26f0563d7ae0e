// TEST INFRASTRUCTURE: the walk of hpp-fcl_amd/csrc/hfcl_octree_mesh.hpp and its depth computation in a stand-alone program: built
// and run by tests/test_octree_mesh_cpu.py with plain g++; the same line with -fsanitize=address,undefined is how the walk's two
// stacks are run under a sanitizer (nothing here touches a device or is loaded into another process).  A map built from points at
// depth 16 against chain BVHs of 1 .. 64 levels under random poses, in stacks of exactly the sizes the walk may use; then a chain two
// levels deeper and a cyclic one, which the walk must leave through its overflow guard.
// Prints "host_check ok" and returns 0, or says what failed.
#include <cstdio>
#include <cstdlib>

#include "../../hpp-fcl_amd/csrc/hfcl_octree_mesh.hpp"

using namespace hfcl;

static int fails = 0;
#define CHECK(c)                                            \
  do {                                                      \
    if (!(c)) {                                             \
      std::printf("FAILED line %d: %s\n", __LINE__, #c);    \
      ++fails;                                              \
    }                                                       \
  } while (0)

static uint64_t lcg(uint64_t& s) {
  s = s * 6364136223846793005ull + 1442695040888963407ull;
  return s >> 33;
}
static double unit(uint64_t& s) { return double(lcg(s) % 1000000) / 1000000.0; }

// a chain of `levels` levels over `levels` boxes along x: node 2k inner (children 2k + 1: leaf k, 2k + 2), the last node leaf levels - 1
static std::vector<DNode<double>> chain(int levels, double reach) {
  std::vector<DNode<double>> n(size_t(2 * levels - 1));
  auto box = [&](DNode<double>& d, double x0, double x1) {
    d.pad_ = 0;
    d.axes.r0 = mk<double>(1, 0, 0);
    d.axes.r1 = mk<double>(0, 1, 0);
    d.axes.r2 = mk<double>(0, 0, 1);
    d.To = mk<double>(0.5 * (x0 + x1), 0.0, 0.0);
    d.extent = mk<double>(0.5 * (x1 - x0), 0.05, 0.05);
  };
  const double step = reach / levels;
  for (int k = 0; k < levels; ++k) {
    const int leaf = k < levels - 1 ? 2 * k + 1 : 2 * k;
    n[size_t(leaf)].first_child = -(k + 1);
    box(n[size_t(leaf)], k * step, (k + 1) * step);
    if (k < levels - 1) {
      n[size_t(2 * k)].first_child = 2 * k + 1;
      box(n[size_t(2 * k)], k * step, reach);
    }
  }
  return n;
}

struct Walk {
  uint64_t leaves = 0;
  bool overflow = false;
  double total = 0;
};
static Walk walk(const std::vector<hfcl_octree_node>& nodes, const DOctree& tr, const std::vector<DNode<double>>& mn, const Pose<double>& tft,
                 const Pose<double>& tfm) {
  // heap arrays of exactly the stacks' sizes: one entry past either is an error a sanitizer names
  std::vector<uint32_t> st_node(OCT_STACK), st_next(OCT_STACK), st_m(OCTM_MESH_STACK);
  std::vector<uint8_t> st_mo(OCTM_MESH_STACK);
  std::vector<double> st_box(6 * OCT_STACK);
  Walk w;
  w.total = octm_walk(nodes.data(), tr, tft, mn.data(), uint32_t(mn.size()), tfm, 0.01, 1e-6, st_node.data(), st_next.data(), st_box.data(), st_m.data(),
                      st_mo.data(), 1,
                      [&](uint32_t node, const V3<double>& lo, const V3<double>& hi, uint32_t prim, double) {
                        CHECK(node < nodes.size() && prim < (mn.size() + 1) / 2 && lo.x < hi.x);
                        ++w.leaves;
                      },
                      w.overflow);
  return w;
}

int main() {
  uint64_t seed = 11;
  std::string why;
  // a map of depth 16: points on a wavy sheet and a few columns, so that the walks go deep in places
  std::vector<double> xyz;
  for (int i = 0; i < 3000; ++i) {
    const double x = 2.0 * unit(seed) - 1.0, y = 2.0 * unit(seed) - 1.0;
    xyz.push_back(x);
    xyz.push_back(y);
    xyz.push_back(0.2 * std::sin(3.0 * x) * std::cos(2.0 * y) + (i % 50 == 0 ? unit(seed) : 0.0));
  }
  std::vector<hfcl_octree_node> nodes;
  CHECK(oct_from_points(xyz.data(), xyz.size() / 3, 0.01, 16, nodes, &why) == HFCL_OK);
  CHECK(oct_validate(nodes.data(), nodes.size(), 16, &why) == HFCL_OK);
  DOctree tr;
  tr.node_off = 0;
  tr.n_nodes = uint32_t(nodes.size());
  tr.depth = 16;
  tr.resolution = 0.01;
  tr.root_half = oct_root_half(16, 0.01);
  tr.occupancy_threshold = 0.5;
  tr.free_threshold = 0.0;
  uint64_t reached = 0;
  for (int levels : {1, 2, 3, 17, 63, OCTM_MESH_DEPTH}) {
    const std::vector<DNode<double>> mn = chain(levels, 1.5);
    CHECK(octm_bvh_depth(mn.size(), [&](uint32_t i) { return mn[i].first_child; }) == uint32_t(levels));
    for (int q = 0; q < 40; ++q) {
      Pose<double> tft = pose_from_quat<double, double>(std::vector<double>{1, 0, 0, 0, 0, 0, 0}.data()), tfm;
      double qu[7] = {unit(seed) - 0.5, unit(seed) - 0.5, unit(seed) - 0.5, unit(seed) - 0.5, 1.6 * unit(seed) - 1.2, 1.6 * unit(seed) - 0.8, 0.3 * unit(seed) - 0.1};
      const double nq = std::sqrt(qu[0] * qu[0] + qu[1] * qu[1] + qu[2] * qu[2] + qu[3] * qu[3]);
      for (int k = 0; k < 4; ++k) qu[k] /= nq;
      tfm = pose_from_quat<double, double>(qu);
      if (q % 3 == 0) std::swap(tft, tfm);  // the tree under the rotated pose
      const Walk w = walk(nodes, tr, mn, tft, tfm);
      CHECK(!w.overflow);
      CHECK(w.total > 0.0);
      reached += w.leaves;
    }
  }
  CHECK(reached > 1000);
  // every box grown over the whole map and a tree of one voxel: the mesh side descends to every leaf.  A path of a BVH of D levels
  // holds D - 1 inner nodes, so at the limit the mesh stack has one frame to spare; two levels deeper the depth says so and the walk,
  // given the mesh all the same, ends through its guard
  std::vector<hfcl_octree_node> one(1);
  for (int k = 0; k < 8; ++k) one[0].child[k] = 0;
  one[0].occupancy = 0.9;
  DOctree small = tr;
  small.n_nodes = 1;
  const Pose<double> id = pose_from_quat<double, double>(std::vector<double>{1, 0, 0, 0, 0, 0, 0}.data());
  std::vector<DNode<double>> full = chain(OCTM_MESH_DEPTH, 1.5), deep = chain(OCTM_MESH_DEPTH + 2, 1.5);
  for (DNode<double>& d : full) d.extent = mk<double>(50.0, 50.0, 50.0);
  for (DNode<double>& d : deep) d.extent = mk<double>(50.0, 50.0, 50.0);
  Walk w = walk(one, small, full, id, id);
  CHECK(!w.overflow && w.leaves == uint64_t(OCTM_MESH_DEPTH));
  CHECK(octm_bvh_depth(deep.size(), [&](uint32_t i) { return deep[i].first_child; }) == uint32_t(OCTM_MESH_DEPTH + 2));
  w = walk(one, small, deep, id, id);
  CHECK(w.overflow);
  // a cycle: the deepest inner node names the root's children again; the depth is unbounded and the walk must stop at its guard
  std::vector<DNode<double>> cyc = chain(8, 1.5);
  cyc[12].first_child = 1;
  CHECK(octm_bvh_depth(cyc.size(), [&](uint32_t i) { return cyc[i].first_child; }) == 0xFFFFFFFFu);
  for (DNode<double>& d : cyc) d.extent = mk<double>(50.0, 50.0, 50.0);  // every box test overlaps: the mesh side descends for ever
  w = walk(one, small, cyc, id, id);
  CHECK(w.overflow);
  if (!fails) std::printf("host_check ok\n");
  return fails ? 1 : 0;
}
