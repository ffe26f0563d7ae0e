// tests/cpp/test_octree.cpp -- the hpp::fcl-named shim (include/hppfcl_amd_compat.hpp) on an OcTree: built and run by
// tests/test_octree_gpu.py, which compares what this prints with compat.collide on the same cases, number for number (hex floats).
//
// argv[1]: a text file.  Line 1: resolution depth n_nodes n_queries; then a line per node: 8 child indices and the occupancy; then a
// line per query: kind (0 box, 1 sphere, 2 capsule, 3 cylinder, 4 cone, 5 ellipsoid) a b c, 12 numbers of the tree's pose, 12 of the
// solid's (the ABI's pose image), swapped (1: collide(solid, tree)), security_margin, num_max_contacts.
// Prints a line per query: numContacts distance_lower_bound, then per contact: b1 b2 depth normal p1 p2; and "tree first: ok" where
// the tree is o1 of every contact.  Exit code 3 with "no CPU fallback" in the output when there is no device.
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
    const AABB root = tree.getRootBV();
    std::printf("root %a %a boxes %zu\n", root.min_[0], root.max_[2], tree.toBoxes().size());
    bool tree_first = true;
    for (unsigned q = 0; q < n_queries; ++q) {
      int kind, swapped;
      double a, b, c, tf[24], margin;
      unsigned nmax;
      if (std::fscanf(f, "%d %lf %lf %lf", &kind, &a, &b, &c) != 4) return 2;
      for (double& x : tf)
        if (std::fscanf(f, "%lf", &x) != 1) return 2;
      if (std::fscanf(f, "%d %lf %u", &swapped, &margin, &nmax) != 3) return 2;
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
      CollisionRequest req;
      req.security_margin = margin;
      req.num_max_contacts = nmax;
      CollisionResult res;
      if (swapped) collide(solid.get(), tfs, &tree, tft, req, res);
      else ComputeCollision(&tree, solid.get())(tft, tfs, req, res);
      std::printf("%zu %a", res.numContacts(), res.distance_lower_bound);
      for (size_t k = 0; k < res.numContacts(); ++k) {
        const Contact& ct = res.getContact(k);
        tree_first = tree_first && ct.o1 == &tree && ct.o2 == solid.get();
        std::printf(" %d %d %a %a %a %a %a %a %a %a %a %a", ct.b1, ct.b2, ct.penetration_depth, ct.normal[0], ct.normal[1], ct.normal[2],
                    ct.nearest_points[0][0], ct.nearest_points[0][1], ct.nearest_points[0][2], ct.nearest_points[1][0], ct.nearest_points[1][1],
                    ct.nearest_points[1][2]);
      }
      std::printf("\n");
    }
    std::printf(tree_first ? "tree first: ok\n" : "tree first: FAILED\n");
    // what the reference refuses
    Halfspace hs(Vec3f(0, 0, 1), 0.0);
    bool refused = false;
    try {
      CollisionRequest req;
      CollisionResult res;
      collide(&tree, Transform3f(), &hs, Transform3f(), req, res);
    } catch (const std::invalid_argument&) {
      refused = true;
    }
    bool negative = false;
    try {
      Sphere s(0.1);
      CollisionRequest req;
      req.security_margin = -0.01;
      CollisionResult res;
      collide(&tree, Transform3f(), &s, Transform3f(), req, res);
    } catch (const std::invalid_argument&) {
      negative = true;
    }
    std::printf(refused && negative ? "halfspace and negative margin refused\n" : "refusals FAILED\n");
    std::vector<Vec3f> cloud = {Vec3f(0.1, 0.1, 0.1), Vec3f(0.1, 0.1, 0.1), Vec3f(-0.6, 0.3, 0.2)};
    std::shared_ptr<OcTree> made = makeOctree(cloud, 0.25);
    std::printf("makeOctree %lu nodes %zu boxes depth %u\n", made->size(), made->toBoxes().size(), made->getTreeDepth());
  } catch (const std::exception& e) {
    std::printf("exception: %s\n", e.what());
    return std::strstr(e.what(), "no CPU fallback") ? 3 : 1;
  }
  std::fclose(f);
  return 0;
}
