// TEST INFRASTRUCTURE: the octree distance walk (hpp-fcl_amd/csrc/hfcl_octree_distance.hpp) in a stand-alone program, the form in which
// it is run under a sanitizer (tests/test_octree_distance_cpu.py::test_host_check_program builds it with -fsanitize=address,undefined).
// Trees: one chain down to a voxel at level 16 (the stack at its depth), a full 8 x 8 x 8 block (every inner node has 8 children), the
// root alone, the empty tree.  For Sphere, Box and Capsule the ordered walk must equal the brute-force minimum over every leaf.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../hpp-fcl_amd/csrc/hfcl_octree_distance.hpp"

using namespace hfcl;

struct HostSolid {
  DShape<double> s;
  V3<double> operator()(const V3<double>& d) const { return prim_support(s, d); }
};

static hfcl_octree_node node(double occ) {
  hfcl_octree_node n;
  std::memset(&n, 0, sizeof(n));
  n.occupancy = occ;
  return n;
}
static uint32_t full(std::vector<hfcl_octree_node>& out, int levels) {
  const uint32_t id = uint32_t(out.size());
  out.push_back(node(0.8));
  if (levels)
    for (int k = 0; k < 8; ++k) {
      const uint32_t c = full(out, levels - 1);
      out[id].child[k] = c;
    }
  return id;
}

struct Leaf {
  uint32_t node;
  V3<double> lo, hi;
};
static void leaves_of(const std::vector<hfcl_octree_node>& t, uint32_t i, const V3<double>& lo, const V3<double>& hi, std::vector<Leaf>& out) {
  bool any = false;
  for (int k = 0; k < 8; ++k)
    if (t[i].child[k]) {
      any = true;
      V3<double> clo, chi;
      oct_child_box(lo, hi, uint32_t(k), clo, chi);
      leaves_of(t, t[i].child[k], clo, chi, out);
    }
  if (!any) out.push_back(Leaf{i, lo, hi});
}

static int fails = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("FAILED line %d: %s\n", __LINE__, #c);           \
      ++fails;                                                     \
    }                                                              \
  } while (0)

int main() {
  QParams<double> q;
  std::memset(&q, 0, sizeof(q));
  q.gjk.tolerance = 1e-6;
  q.gjk.max_iterations = 128;
  q.gjk.distance_upper_bound = Lim<double>::max();
  q.epa_tolerance = 1e-6;
  q.epa_max_iterations = 64;
  q.compute_penetration = 1;
  q.guess[0] = 1;
  static EpaScratch<double, EPA_MAX_ITER> scratch;
  static OctDistStack<double> stack;

  std::vector<std::vector<hfcl_octree_node>> trees(4);
  std::vector<uint32_t> depth = {16, 4, 2, 3};
  std::vector<double> res = {0.001, 0.1, 0.1, 0.1};
  {  // the chain: child 7, 0, 7, 0 ... with a sibling leaf at a few levels
    auto& t = trees[0];
    t.push_back(node(0.8));
    uint32_t at = 0;
    for (int level = 0; level < 16; ++level) {
      if (level == 1 || level == 6 || level == 15) {
        t[at].child[3] = uint32_t(t.size());
        t.push_back(node(0.8));
      }
      t[at].child[level % 2 == 0 ? 7 : 0] = uint32_t(t.size());
      at = uint32_t(t.size());
      t.push_back(node(0.8));
    }
  }
  {  // the block under child 0 of the root
    auto& t = trees[1];
    t.push_back(node(0.8));
    const uint32_t c = full(t, 3);
    t[0].child[0] = c;
  }
  trees[2].push_back(node(0.8));  // the root alone; trees[3]: empty
  for (size_t k = 0; k < 3; ++k) CHECK(oct_validate(trees[k].data(), trees[k].size(), depth[k], nullptr) == HFCL_OK);

  uint64_t state = 12345;
  auto uni = [&]() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return double(state >> 11) / double(1ull << 53);
  };
  size_t solved = 0, queries = 0;
  for (size_t k = 0; k < trees.size(); ++k) {
    DOctree tr;
    tr.node_off = 0;
    tr.n_nodes = uint32_t(trees[k].size());
    tr.depth = depth[k];
    tr.resolution = res[k];
    tr.root_half = oct_root_half(depth[k], res[k]);
    tr.occupancy_threshold = 0.5;
    tr.free_threshold = 0.0;
    std::vector<Leaf> lv;
    const double d = tr.root_half;
    if (!trees[k].empty()) leaves_of(trees[k], 0, mk<double>(-d, -d, -d), mk<double>(d, d, d), lv);
    for (int it = 0; it < 60; ++it) {
      HostSolid solid;
      std::memset(&solid.s, 0, sizeof(solid.s));
      solid.s.kind = (it % 3 == 0) ? K_SPHERE : (it % 3 == 1 ? K_BOX : K_CAPSULE);
      const double size = k == 0 ? 0.002 : 0.05;
      solid.s.p0 = size;
      solid.s.p1 = size * 1.5;
      solid.s.p2 = size * 0.5;
      Pose<double> tft, tfs;
      const double c = it % 2 ? 0.8 : 1.0, s = it % 2 ? 0.6 : 0.0;  // a rotation about z by a 3-4-5 angle, or the identity
      tft.R.r0 = mk<double>(c, -s, 0.0);
      tft.R.r1 = mk<double>(s, c, 0.0);
      tft.R.r2 = mk<double>(0.0, 0.0, 1.0);
      tft.t = mk<double>(uni() - 0.5, uni() - 0.5, uni() - 0.5);
      tfs.R = tft.R;
      const V3<double> local = lv.empty() ? mk<double>(0.1, 0.2, 0.3)
                                          : (lv[size_t(uni() * double(lv.size())) % lv.size()].hi +
                                             mk<double>(uni(), uni(), uni()) * (k == 0 ? 0.01 : 0.4));
      tfs.t = mul(tft.R, local) + tft.t;
      OctDistResult<double> r;
      bool overflow = true;
      oct_distance_query<double, SerialGroup<1>>(trees[k].data(), tr, tft, solid.s, nullptr, tfs, solid, q, &stack, &scratch, r, overflow);
      CHECK(!overflow);
      CHECK(r.visited <= lv.size());
      ++queries;
      solved += r.visited;
      if (lv.empty()) {
        CHECK(r.min_distance == Lim<double>::max() && r.b1 == -1 && r.visited == 0 && r.p1.x != r.p1.x);
        continue;
      }
      CHECK(r.visited >= 1 && r.b1 >= 0);
      double best = Lim<double>::max();
      uint32_t best_node = 0;
      for (const Leaf& l : lv) {
        OctLeafOut<double> lf;
        oct_leaf<double, SerialGroup<1>>(l.lo, l.hi, tft, solid.s, nullptr, tfs, solid, q, &scratch, lf);
        if (lf.distance < best) {
          best = lf.distance;
          best_node = l.node;
        }
      }
      if (best > 0) CHECK(r.min_distance == best && uint32_t(r.b1) == best_node);
      else CHECK(r.min_distance <= 0);
    }
  }
  std::printf("%zu queries, %zu leaves solved\n", queries, solved);
  if (fails) return 1;
  std::printf("host_check ok\n");
  return 0;
}
