// TEST INFRASTRUCTURE: the octree x mesh distance walk (hpp-fcl_amd/csrc/hfcl_octree_mesh_distance.hpp) in a stand-alone program, the form
// in which it is run under a sanitizer (tests/test_octree_mesh_distance_cpu.py::test_host_check_program builds it with
// -fsanitize=address,undefined).  The deepest path stack: one chain of the octree down to a voxel at level 16 against a mesh whose BVH is
// a chain of OCTM_MESH_DEPTH levels (16 octree frames and 63 mesh frames at once); a full 8 x 8 x 8 block against the 12 triangles of a
// box; the root alone; the empty tree.  For every separated query the ordered walk must equal the brute-force minimum over every leaf x
// triangle.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../hpp-fcl_amd/csrc/hfcl_octree_mesh_distance.hpp"

using namespace hfcl;

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

struct HostMesh {
  std::vector<double> verts;
  std::vector<uint32_t> tris;
  std::vector<DNode<double>> nodes;
  // the axis-aligned box of some triangles as node `at`'s OBB
  void box(uint32_t at, const std::vector<uint32_t>& ts) {
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (uint32_t t : ts)
      for (int c = 0; c < 3; ++c)
        for (int a = 0; a < 3; ++a) {
          const double x = verts[3 * size_t(tris[3 * size_t(t) + c]) + a];
          lo[a] = std::min(lo[a], x);
          hi[a] = std::max(hi[a], x);
        }
    DNode<double>& n = nodes[at];
    n.pad_ = 0;
    n.axes.r0 = mk<double>(1.0, 0.0, 0.0);
    n.axes.r1 = mk<double>(0.0, 1.0, 0.0);
    n.axes.r2 = mk<double>(0.0, 0.0, 1.0);
    n.To = mk<double>(0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2]));
    n.extent = mk<double>(0.5 * (hi[0] - lo[0]), 0.5 * (hi[1] - lo[1]), 0.5 * (hi[2] - lo[2]));
  }
  // halves by the triangles' order, children side by side
  void build(uint32_t at, const std::vector<uint32_t>& ts) {
    box(at, ts);
    if (ts.size() == 1) {
      nodes[at].first_child = -(int32_t(ts[0]) + 1);
      return;
    }
    const uint32_t c = uint32_t(nodes.size());
    nodes.resize(nodes.size() + 2);
    nodes[at].first_child = int32_t(c);
    const size_t h = ts.size() / 2;
    build(c, std::vector<uint32_t>(ts.begin(), ts.begin() + h));
    build(c + 1, std::vector<uint32_t>(ts.begin() + h, ts.end()));
  }
  // node 2k: the inner node of triangles k .., its left child the leaf of triangle k, its right child node 2k + 2
  void build_chain() {
    const uint32_t levels = uint32_t(tris.size() / 3);
    nodes.resize(2 * levels - 1);
    for (uint32_t k = 0; k < levels; ++k) {
      const uint32_t leaf = k + 1 < levels ? 2 * k + 1 : 2 * k;
      box(leaf, {k});
      nodes[leaf].first_child = -(int32_t(k) + 1);
      if (k + 1 < levels) {
        std::vector<uint32_t> rest;
        for (uint32_t j = k; j < levels; ++j) rest.push_back(j);
        box(2 * k, rest);
        nodes[2 * k].first_child = int32_t(2 * k + 1);
      }
    }
  }
};

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
  static OctMeshDistStack<double> stack;

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

  HostMesh chain, box12;
  for (int k = 0; k < OCTM_MESH_DEPTH; ++k) {  // small triangles along a diagonal, the first ones nearest the chain tree's voxel
    const double x = 0.0005 * k, s = 0.0004;
    const double v[9] = {x, 0.5 * x, -x, x + s, 0.5 * x, -x, x, 0.5 * x + s, -x + 0.3 * s};
    chain.verts.insert(chain.verts.end(), v, v + 9);
    for (uint32_t c = 0; c < 3; ++c) chain.tris.push_back(uint32_t(3 * k) + c);
  }
  chain.build_chain();
  CHECK(octm_bvh_depth(chain.nodes.size(), [&](uint32_t i) { return chain.nodes[i].first_child; }) == uint32_t(OCTM_MESH_DEPTH));
  {
    const double h[3] = {0.12, 0.08, 0.15};
    for (int sx = -1; sx <= 1; sx += 2)
      for (int sy = -1; sy <= 1; sy += 2)
        for (int sz = -1; sz <= 1; sz += 2) {
          box12.verts.push_back(sx * h[0]);
          box12.verts.push_back(sy * h[1]);
          box12.verts.push_back(sz * h[2]);
        }
    const uint32_t t[36] = {0, 1, 3, 0, 3, 2, 4, 6, 7, 4, 7, 5, 0, 4, 5, 0, 5, 1, 2, 3, 7, 2, 7, 6, 0, 2, 6, 0, 6, 4, 1, 5, 7, 1, 7, 3};
    box12.tris.assign(t, t + 36);
    box12.nodes.resize(1);
    std::vector<uint32_t> all;
    for (uint32_t k = 0; k < 12; ++k) all.push_back(k);
    box12.build(0, all);
    CHECK(box12.nodes.size() == 23);
  }

  uint64_t state = 12345;
  auto uni = [&]() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return double(state >> 11) / double(1ull << 53);
  };
  size_t solved = 0, queries = 0, separated = 0;
  int deepest_o = 0, deepest_m = 0;
  for (size_t k = 0; k < trees.size(); ++k) {
    DOctree tr;
    tr.node_off = 0;
    tr.n_nodes = uint32_t(trees[k].size());
    tr.depth = depth[k];
    tr.resolution = res[k];
    tr.root_half = oct_root_half(depth[k], res[k]);
    tr.occupancy_threshold = 0.5;
    tr.free_threshold = 0.0;
    const HostMesh& me = k == 0 ? chain : box12;
    std::vector<Leaf> lv;
    const double d = tr.root_half;
    if (!trees[k].empty()) leaves_of(trees[k], 0, mk<double>(-d, -d, -d), mk<double>(d, d, d), lv);
    for (int it = 0; it < (k == 1 ? 12 : 30); ++it) {
      Pose<double> tft, tfm;
      const double c = it % 2 ? 0.8 : 1.0, s = it % 2 ? 0.6 : 0.0;  // a rotation about z by a 3-4-5 angle, or the identity
      tft.R.r0 = mk<double>(c, -s, 0.0);
      tft.R.r1 = mk<double>(s, c, 0.0);
      tft.R.r2 = mk<double>(0.0, 0.0, 1.0);
      tft.t = mk<double>(uni() - 0.5, uni() - 0.5, uni() - 0.5);
      tfm.R.r0 = mk<double>(1.0, 0.0, 0.0);
      tfm.R.r1 = mk<double>(0.0, c, -s);
      tfm.R.r2 = mk<double>(0.0, s, c);
      const V3<double> local = lv.empty() ? mk<double>(0.1, 0.2, 0.3)
                                          : (lv[size_t(uni() * double(lv.size())) % lv.size()].hi +
                                             mk<double>(uni(), uni(), uni()) * (k == 0 ? 0.002 : 0.5));
      tfm.t = mul(tft.R, local) + tft.t;
      if (k == 0) {  // the chain's LAST triangle next to the tree's deepest voxel: every level of both chains lies on the way to the nearest pair
        const Leaf* deep = &lv[0];
        for (const Leaf& l : lv)
          if (l.node > deep->node) deep = &l;
        const double* v = &me.verts[9 * size_t(OCTM_MESH_DEPTH - 1)];
        tfm.t = mul(tft.R, deep->hi + mk<double>(uni(), uni(), uni()) * 0.002) + tft.t - mul(tfm.R, mk<double>(v[0], v[1], v[2]));
      }
      OctMeshDistResult<double> r;
      bool overflow = true;
      // the same walk by hand first, for the depth the two stacks reach
      {
        OctMeshDistWalk w;
        octmd_walk_init(w, tr, uint32_t(me.nodes.size()));
        OctMeshDistResult<double> rr;
        octmd_clear(rr);
        for (uint64_t pass = 0; pass < w.max_steps; ++pass) {
          uint32_t leaf = 0, prim = 0;
          V3<double> llo, lhi;
          if (!octmd_next<double, SerialGroup<1>>(trees[k].data(), tr, tft, me.nodes.data(), uint32_t(me.nodes.size()), tfm, rr.min_distance, &stack, w, leaf,
                                                  llo, lhi, prim))
            break;
          deepest_o = std::max(deepest_o, w.osp);
          deepest_m = std::max(deepest_m, w.msp);
          OctMeshLeafOut<double> lf;
          octm_leaf<double, SerialGroup<1>>(llo, lhi, tft, me.verts.data(), me.tris.data() + 3 * size_t(prim), tfm, q, &scratch, lf);
          octmd_update(rr, leaf, prim, lf);
          if (rr.min_distance <= 0) break;
        }
        CHECK(!w.overflow && w.steps < w.max_steps);
      }
      octm_distance_query<double, SerialGroup<1>>(trees[k].data(), tr, tft, me.nodes.data(), uint32_t(me.nodes.size()), me.verts.data(), me.tris.data(), tfm, q,
                                                  &stack, &scratch, r, overflow, OctMeshDistNoList());
      CHECK(!overflow);
      CHECK(r.visited <= lv.size() * (me.tris.size() / 3));
      ++queries;
      solved += r.visited;
      if (lv.empty()) {
        CHECK(r.min_distance == Lim<double>::max() && r.b1 == -1 && r.b2 == -1 && r.visited == 0 && r.p1.x != r.p1.x);
        continue;
      }
      CHECK(r.visited >= 1 && r.b1 >= 0 && r.b2 >= 0);
      double best = Lim<double>::max();
      for (const Leaf& l : lv)
        for (uint32_t t = 0; t < me.tris.size() / 3; ++t) {
          OctMeshLeafOut<double> lf;
          octm_leaf<double, SerialGroup<1>>(l.lo, l.hi, tft, me.verts.data(), me.tris.data() + 3 * size_t(t), tfm, q, &scratch, lf);
          if (lf.distance < best) best = lf.distance;
        }
      if (best > 0) {
        CHECK(r.min_distance == best);
        ++separated;
      } else {
        CHECK(r.min_distance <= 0);
      }
    }
  }
  std::printf("%zu queries, %zu separated, %zu pairs solved, deepest stacks %d octree + %d mesh frames\n", queries, separated, solved, deepest_o, deepest_m);
  CHECK(deepest_o == OCT_STACK && deepest_m == OCTM_MESH_DEPTH - 1);
  CHECK(separated > 20);
  if (fails) return 1;
  std::printf("host_check ok\n");
  return 0;
}
