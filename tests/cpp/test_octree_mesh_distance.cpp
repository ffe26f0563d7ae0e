// tests/cpp/test_octree_mesh_distance.cpp -- the hpp::fcl-named shim (include/hppfcl_amd_compat.hpp) on distance() between an OcTree and
// BVHModel<OBBRSS> meshes: built and run by tests/test_octree_mesh_distance_gpu.py, which compares what this prints with
// compat.distance_octree_mesh on the same cases, number for number (hex floats).
//
// argv[1]: a text file.  Line 1: resolution depth n_nodes n_meshes n_queries; then a line per node: 8 child indices and the occupancy;
// then per mesh a line "n_vertices n_triangles", its vertices (x y z a line) and its triangles (three vertex ids a line); then a line
// per query: the mesh, 12 numbers of the tree's pose, 12 of the mesh's (the ABI's pose image), swapped (1: distance(mesh, tree)),
// enable_signed_distance.
// Prints a line per query: b1 b2 min_distance normal p1 p2; "tree first: ok" where the tree is o1 and the mesh o2 of every result;
// "batch: ok" where OcTreeBatch::distanceMesh on the queries of the first query's request gives the same records; "dispatch refuses the
// pair" where hpp::fcl::distance and ComputeDistance still throw for it.  Exit code 3 with "no CPU fallback" in the output when there is
// no device.
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
  unsigned depth, n_nodes, n_meshes, n_queries;
  if (std::fscanf(f, "%lf %u %u %u %u", &resolution, &depth, &n_nodes, &n_meshes, &n_queries) != 5) return 2;
  std::vector<hfcl_octree_node> nodes(n_nodes);
  for (auto& n : nodes) {
    for (int k = 0; k < 8; ++k)
      if (std::fscanf(f, "%u", &n.child[k]) != 1) return 2;
    if (std::fscanf(f, "%lf", &n.occupancy) != 1) return 2;
  }
  try {
    std::vector<std::unique_ptr<BVHModel<OBBRSS>>> meshes;
    for (unsigned m = 0; m < n_meshes; ++m) {
      unsigned nv, nt;
      if (std::fscanf(f, "%u %u", &nv, &nt) != 2) return 2;
      std::vector<Vec3f> ps(nv);
      std::vector<Triangle> ts;
      for (auto& p : ps)
        if (std::fscanf(f, "%lf %lf %lf", &p[0], &p[1], &p[2]) != 3) return 2;
      for (unsigned t = 0; t < nt; ++t) {
        unsigned a, b, c;
        if (std::fscanf(f, "%u %u %u", &a, &b, &c) != 3) return 2;
        ts.emplace_back(a, b, c);
      }
      meshes.emplace_back(new BVHModel<OBBRSS>());
      meshes.back()->beginModel();
      meshes.back()->addSubModel(ps, ts);
      meshes.back()->endModel();
    }
    OcTree tree(nodes, resolution, depth);
    bool tree_first = true;
    std::vector<std::pair<uint32_t, uint32_t>> ids;
    std::vector<Transform3f> tf_t, tf_m;
    std::vector<uint8_t> sw;
    std::vector<DistanceResult> want;
    DistanceRequest batch_req;
    amd::OcTreeBatch& ob = amd::default_octree_batch();
    for (unsigned q = 0; q < n_queries; ++q) {
      int swapped, is_signed;
      unsigned mesh;
      double tf[24];
      if (std::fscanf(f, "%u", &mesh) != 1 || mesh >= n_meshes) return 2;
      for (double& x : tf)
        if (std::fscanf(f, "%lf", &x) != 1) return 2;
      if (std::fscanf(f, "%d %d", &swapped, &is_signed) != 2) return 2;
      Transform3f tft, tfm;
      std::memcpy(static_cast<void*>(&tft), tf, 12 * sizeof(double));
      std::memcpy(static_cast<void*>(&tfm), tf + 12, 12 * sizeof(double));
      DistanceRequest req;
      req.enable_signed_distance = is_signed != 0;
      DistanceResult res;
      const BVHModel<OBBRSS>* me = meshes[mesh].get();
      const FCL_REAL d = swapped ? amd::distanceOcTreeMesh(me, tfm, &tree, tft, req, res) : amd::distanceOcTreeMesh(&tree, tft, me, tfm, req, res);
      tree_first = tree_first && res.o1 == &tree && res.o2 == me && d == res.min_distance;
      std::printf("%d %d %a %a %a %a %a %a %a %a %a %a\n", res.b1, res.b2, res.min_distance, res.normal[0], res.normal[1], res.normal[2],
                  res.nearest_points[0][0], res.nearest_points[0][1], res.nearest_points[0][2], res.nearest_points[1][0], res.nearest_points[1][1],
                  res.nearest_points[1][2]);
      if (q == 0) batch_req = req;
      if (req.enable_signed_distance == batch_req.enable_signed_distance) {
        ids.emplace_back(ob.addTree(&tree), ob.addSolid(me));
        tf_t.push_back(tft);
        tf_m.push_back(tfm);
        sw.push_back(static_cast<uint8_t>(swapped ? 1 : 0));
        want.push_back(res);
      }
    }
    std::printf(tree_first ? "tree first: ok\n" : "tree first: FAILED\n");
    std::vector<DistanceResult> all;
    std::vector<uint32_t> visited;
    ob.distanceMesh(ids, tf_t, tf_m, sw, batch_req, all, &visited);
    bool same = all.size() == want.size() && !want.empty() && visited.size() == all.size();
    for (size_t i = 0; same && i < all.size(); ++i)
      same = all[i].min_distance == want[i].min_distance && all[i].b1 == want[i].b1 && all[i].b2 == want[i].b2 && all[i].o1 == &tree &&
             (visited[i] > 0) == (all[i].b1 >= 0);
    std::printf(same ? "batch: ok (%zu queries)\n" : "batch: FAILED (%zu queries)\n", all.size());
    // the dispatch keeps refusing the pair (the follow-up); the call of its own refuses what is no octree x mesh pair
    int refused = 0;
    try {
      DistanceRequest req;
      DistanceResult res;
      distance(&tree, Transform3f(), meshes[0].get(), Transform3f(), req, res);
    } catch (const std::invalid_argument&) {
      ++refused;
    }
    try {
      ComputeDistance cd(meshes[0].get(), &tree);
    } catch (const std::invalid_argument&) {
      ++refused;
    }
    try {
      DistanceRequest req;
      DistanceResult res;
      amd::distanceOcTreeMesh(&tree, Transform3f(), &tree, Transform3f(), req, res);
    } catch (const std::invalid_argument&) {
      ++refused;
    }
    try {
      Sphere ball(0.1);
      DistanceRequest req;
      DistanceResult res;
      amd::distanceOcTreeMesh(&ball, Transform3f(), &tree, Transform3f(), req, res);
    } catch (const std::invalid_argument&) {
      ++refused;
    }
    std::printf(refused == 4 ? "dispatch refuses the pair\n" : "refusals FAILED\n");
  } catch (const std::exception& e) {
    std::printf("exception: %s\n", e.what());
    return std::strstr(e.what(), "no CPU fallback") ? 3 : 1;
  }
  std::fclose(f);
  return 0;
}
