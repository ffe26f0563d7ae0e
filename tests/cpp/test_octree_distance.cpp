// tests/cpp/test_octree_distance.cpp -- the hpp::fcl-named shim (include/hppfcl_amd_compat.hpp) on distance() with an OcTree: built and
// run by tests/test_octree_distance_gpu.py, which compares what this prints with the engine call on the same cases, number for number
// (hex floats).
//
// argv[1]: a text file.  Line 1: resolution depth n_nodes n_queries; then a line per node: 8 child indices and the occupancy; then a
// line per query: kind (0 box, 1 sphere, 2 capsule, 3 cylinder, 4 cone, 5 ellipsoid) a b c, 12 numbers of the tree's pose, 12 of the
// solid's (the ABI's pose image), swapped (1: distance(solid, tree)), enable_signed_distance.
// Prints a line per query: the returned distance, min_distance, b1 b2, normal, the nearest points; "tree first: ok" where the tree is o1
// of every result; then the same queries through amd::OcTreeBatch::distance in one call ("batch: ok" where they agree).  Exit code 3
// with "no CPU fallback" in the output when there is no device.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "hppfcl_amd_compat.hpp"

using namespace hpp::fcl;

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  double resolution;
  unsigned depth, n_nodes, n_queries;
  if (std::fscanf(f, "%lf %u %u %u", &resolution, &depth, &n_nodes, &n_queries) != 4) return 2;
  std::vector<hfcl_octree_node> nodes(n_nodes);
  for (auto& n : nodes) {
    for (int k = 0; k < 8; ++k)
      if (std::fscanf(f, "%u", &n.child[k]) != 1) return 2;
    if (std::fscanf(f, "%lf", &n.occupancy) != 1) return 2;
  }
  try {
    OcTree tree(nodes, resolution, depth);
    bool tree_first = true;
    std::vector<std::unique_ptr<ShapeBase>> solids;
    std::vector<Transform3f> tf_tree, tf_solid;
    std::vector<uint8_t> order;
    std::vector<DistanceResult> single;
    std::vector<int> signed_flags;
    for (unsigned q = 0; q < n_queries; ++q) {
      int kind, swapped, signed_distance;
      double a, b, c, tf[24];
      if (std::fscanf(f, "%d %lf %lf %lf", &kind, &a, &b, &c) != 4) return 2;
      for (double& x : tf)
        if (std::fscanf(f, "%lf", &x) != 1) return 2;
      if (std::fscanf(f, "%d %d", &swapped, &signed_distance) != 2) return 2;
      std::unique_ptr<ShapeBase> solid;
      if (kind == 0) solid.reset(new Box(a, b, c));
      else if (kind == 1) solid.reset(new Sphere(a));
      else if (kind == 2) solid.reset(new Capsule(a, b));
      else if (kind == 3) solid.reset(new Cylinder(a, b));
      else if (kind == 4) solid.reset(new Cone(a, b));
      else solid.reset(new Ellipsoid(a, b, c));
      Transform3f tft, tfs;
      std::memcpy(static_cast<void*>(&tft), tf, 12 * sizeof(double));
      std::memcpy(static_cast<void*>(&tfs), tf + 12, 12 * sizeof(double));
      DistanceRequest req;
      req.enable_signed_distance = signed_distance != 0;
      DistanceResult res;
      const FCL_REAL d = swapped ? distance(solid.get(), tfs, &tree, tft, req, res) : ComputeDistance(&tree, solid.get())(tft, tfs, req, res);
      tree_first = tree_first && res.o1 == &tree && res.o2 == solid.get();
      std::printf("%a %a %d %d %a %a %a %a %a %a %a %a %a\n", d, res.min_distance, res.b1, res.b2, res.normal[0], res.normal[1], res.normal[2],
                  res.nearest_points[0][0], res.nearest_points[0][1], res.nearest_points[0][2], res.nearest_points[1][0], res.nearest_points[1][1],
                  res.nearest_points[1][2]);
      solids.push_back(std::move(solid));
      tf_tree.push_back(tft);
      tf_solid.push_back(tfs);
      order.push_back(static_cast<uint8_t>(swapped));
      single.push_back(res);
      signed_flags.push_back(signed_distance);
    }
    std::printf(tree_first ? "tree first: ok\n" : "tree first: FAILED\n");
    // the signed queries once more as one batch
    amd::OcTreeBatch& batch = amd::default_octree_batch();
    std::vector<std::pair<uint32_t, uint32_t>> pairs;
    std::vector<Transform3f> bt, bs;
    std::vector<uint8_t> bo;
    std::vector<size_t> which;
    const uint32_t t = batch.addTree(&tree);
    for (size_t q = 0; q < solids.size(); ++q)
      if (signed_flags[q]) {
        pairs.emplace_back(t, batch.addSolid(solids[q].get()));
        bt.push_back(tf_tree[q]);
        bs.push_back(tf_solid[q]);
        bo.push_back(order[q]);
        which.push_back(q);
      }
    std::vector<DistanceResult> many;
    std::vector<uint32_t> visited;
    batch.distance(pairs, bt, bs, bo, DistanceRequest(), many, &visited);
    bool same = many.size() == which.size() && !many.empty();
    for (size_t k = 0; same && k < many.size(); ++k) {
      const DistanceResult& a = many[k];
      const DistanceResult& b = single[which[k]];
      same = a.min_distance == b.min_distance && a.b1 == b.b1 && a.o1 == &tree && visited[k] >= 1 && ((batch.records()[k].status >> 23) & 1u) == bo[k];
    }
    std::printf(same ? "batch: ok\n" : "batch: FAILED\n");
    // what has no function
    Halfspace hs(Vec3f(0, 0, 1), 0.0);
    bool refused = false;
    try {
      DistanceRequest req;
      DistanceResult res;
      distance(&tree, Transform3f(), &hs, Transform3f(), req, res);
    } catch (const std::invalid_argument&) {
      refused = true;
    }
    bool two_trees = false;
    try {
      ComputeDistance cd(&tree, &tree);
    } catch (const std::invalid_argument&) {
      two_trees = true;
    }
    std::printf(refused && two_trees ? "halfspace and octree x octree refused\n" : "refusals FAILED\n");
  } catch (const std::exception& e) {
    std::printf("exception: %s\n", e.what());
    return std::strstr(e.what(), "no CPU fallback") ? 3 : 1;
  }
  std::fclose(f);
  return 0;
}
