// tests/cpp/test_octree_mesh.cpp -- the hpp::fcl-named shim (include/hppfcl_amd_compat.hpp) on an OcTree against BVHModel<OBBRSS>
// meshes: built and run by tests/test_octree_mesh_gpu.py, which compares what this prints with compat.collide on the same cases, number
// for number (hex floats).
//
// argv[1]: a text file.  Line 1: resolution depth n_nodes n_meshes n_queries; then a line per node: 8 child indices and the occupancy;
// then per mesh a line "n_vertices n_triangles", its vertices (x y z a line) and its triangles (three vertex ids a line); then a line
// per query: the mesh, 12 numbers of the tree's pose, 12 of the mesh's (the ABI's pose image), swapped (1: collide(mesh, tree)),
// security_margin, num_max_contacts.
// Prints a line per query: numContacts distance_lower_bound, then per contact: b1 b2 depth normal p1 p2; "tree first: ok" where the
// tree is o1 of every contact; "batch: ok" where OcTreeBatch::collideMesh on all queries at once gives the same contacts.  Exit code 3
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
    // one request for the batch: the queries that share the first query's margin and num_max_contacts
    std::vector<std::pair<uint32_t, uint32_t>> ids;
    std::vector<Transform3f> tf_t, tf_m;
    std::vector<uint8_t> sw;
    std::vector<size_t> want;
    CollisionRequest batch_req;
    amd::OcTreeBatch& ob = amd::default_octree_batch();
    for (unsigned q = 0; q < n_queries; ++q) {
      int swapped;
      unsigned mesh, nmax;
      double tf[24], margin;
      if (std::fscanf(f, "%u", &mesh) != 1 || mesh >= n_meshes) return 2;
      for (double& x : tf)
        if (std::fscanf(f, "%lf", &x) != 1) return 2;
      if (std::fscanf(f, "%d %lf %u", &swapped, &margin, &nmax) != 3) return 2;
      Transform3f tft, tfm;
      std::memcpy(static_cast<void*>(&tft), tf, 12 * sizeof(double));
      std::memcpy(static_cast<void*>(&tfm), tf + 12, 12 * sizeof(double));
      CollisionRequest req;
      req.security_margin = margin;
      req.num_max_contacts = nmax;
      CollisionResult res;
      const BVHModel<OBBRSS>* me = meshes[mesh].get();
      if (swapped) collide(me, tfm, &tree, tft, req, res);
      else ComputeCollision(&tree, me)(tft, tfm, req, res);
      std::printf("%zu %a", res.numContacts(), res.distance_lower_bound);
      for (size_t k = 0; k < res.numContacts(); ++k) {
        const Contact& ct = res.getContact(k);
        tree_first = tree_first && ct.o1 == &tree && ct.o2 == me;
        std::printf(" %d %d %a %a %a %a %a %a %a %a %a %a", ct.b1, ct.b2, ct.penetration_depth, ct.normal[0], ct.normal[1], ct.normal[2],
                    ct.nearest_points[0][0], ct.nearest_points[0][1], ct.nearest_points[0][2], ct.nearest_points[1][0], ct.nearest_points[1][1],
                    ct.nearest_points[1][2]);
      }
      std::printf("\n");
      if (q == 0) batch_req = req;
      if (margin == batch_req.security_margin && nmax == batch_req.num_max_contacts) {
        ids.emplace_back(ob.addTree(&tree), ob.addSolid(me));
        tf_t.push_back(tft);
        tf_m.push_back(tfm);
        sw.push_back(static_cast<uint8_t>(swapped ? 1 : 0));
        want.push_back(res.numContacts());
      }
    }
    std::printf(tree_first ? "tree first: ok\n" : "tree first: FAILED\n");
    std::vector<CollisionResult> all;
    ob.collideMesh(ids, tf_t, tf_m, sw, batch_req, all);
    bool same = all.size() == want.size() && !want.empty();
    for (size_t i = 0; same && i < all.size(); ++i) same = all[i].numContacts() == want[i];
    std::printf(same ? "batch: ok (%zu queries)\n" : "batch: FAILED (%zu queries)\n", all.size());
    // what the reference refuses: a negative margin; and what this library does not have: distance() for the pair
    bool negative = false, no_distance = false;
    try {
      CollisionRequest req;
      req.security_margin = -0.01;
      CollisionResult res;
      collide(&tree, Transform3f(), meshes[0].get(), Transform3f(), req, res);
    } catch (const std::invalid_argument&) {
      negative = true;
    }
    try {
      DistanceRequest req;
      DistanceResult res;
      distance(&tree, Transform3f(), meshes[0].get(), Transform3f(), req, res);
    } catch (const std::invalid_argument&) {
      no_distance = true;
    }
    std::printf(negative && no_distance ? "negative margin and distance refused\n" : "refusals FAILED\n");
  } catch (const std::exception& e) {
    std::printf("exception: %s\n", e.what());
    return std::strstr(e.what(), "no CPU fallback") ? 3 : 1;
  }
  std::fclose(f);
  return 0;
}
