// A height-field terrain under a scene's objects through the C++ shim (hpp::fcl::amd::Scene::setTerrain / collideTerrain /
// clearTerrain), built and run by tests/test_scene_terrain_gpu.py: every query against hpp::fcl::collide(field, tf, link, tf_link) --
// contact count, first contact and bound field-equal --, the summaries against a fold of those results, a list of objects, the heights
// updated under a terrain that is set, and a halfspace refused.
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "hppfcl_amd_compat.hpp"

using namespace hpp::fcl;

static bool same_vec(const Vec3f& a, const Vec3f& b) { return a[0] == b[0] && a[1] == b[1] && a[2] == b[2]; }

// collideTerrain on `tables` against the loop of collide(); `listed`: the objects of the terrain's list
static bool check(amd::Scene& scene, const HeightField<AABB>& field, const Transform3f& ftf, const std::vector<CollisionObject*>& objects,
                  const std::vector<uint32_t>& listed, const std::vector<Transform3f>& tables, size_t n_conf, const CollisionRequest& req,
                  int& hits, const char* what) {
  std::vector<CollisionResult> results;
  std::vector<hfcl_scene_summary> summaries, only;
  scene.collideTerrain(tables.data(), n_conf, req, &results, &summaries);
  scene.collideTerrain(tables.data(), n_conf, req, nullptr, &only);
  bool ok = results.size() == n_conf * listed.size() && summaries.size() == n_conf && only.size() == n_conf &&
            scene.numTerrainObjects() == listed.size();
  for (size_t c = 0; ok && c < n_conf; ++c) {
    uint32_t first = 0xFFFFFFFFu, count = 0, min_pair = 0xFFFFFFFFu;
    double min_distance = INFINITY;
    for (size_t k = 0; k < listed.size(); ++k) {
      const uint32_t o = listed[k];
      CollisionResult ref;
      collide(&field, ftf, objects[o]->collisionGeometryPtr(), tables[c * objects.size() + o], req, ref);
      const CollisionResult& got = results[c * listed.size() + k];
      ok = ok && got.numContacts() == ref.numContacts() && got.distance_lower_bound == ref.distance_lower_bound;
      if (ok && ref.isCollision()) {
        const Contact &a = got.getContact(0), &b = ref.getContact(0);
        ok = a.b1 == b.b1 && a.b2 == b.b2 && a.penetration_depth == b.penetration_depth && same_vec(a.normal, b.normal) && same_vec(a.pos, b.pos) &&
             a.o1 == &field && a.o2 == objects[o]->collisionGeometryPtr();
        ++count;
        if (o < first) first = o;
      }
      if (ref.distance_lower_bound < min_distance) {
        min_distance = ref.distance_lower_bound;
        min_pair = o;
      }
    }
    const hfcl_scene_summary& s = summaries[c];
    ok = ok && s.n_contacts == count && s.first_contact == first && s.min_distance == min_distance && s.min_pair == min_pair && s.n_skipped == 0;
    ok = ok && only[c].n_contacts == s.n_contacts && only[c].first_contact == s.first_contact && only[c].min_distance == s.min_distance &&
         only[c].min_pair == s.min_pair;
    hits += int(count);
  }
  if (!ok) std::printf("FAILED %s\n", what);
  return ok;
}

int main() {
  MatrixXf h(size_t(6), size_t(5));
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 5; ++c) h(r, c) = 0.4 + 0.1 * ((3 * r + 5 * c) % 7);
  HeightField<AABB> field(2.0, 3.0, h, -0.2);
  const Transform3f ftf(Vec3f(0.1, -0.2, 0.05));
  std::vector<std::shared_ptr<CollisionGeometry>> geoms = {std::make_shared<Sphere>(0.3), std::make_shared<Box>(0.4, 0.3, 0.5),
                                                          std::make_shared<Capsule>(0.15, 0.4), std::make_shared<Cylinder>(0.2, 0.3),
                                                          std::make_shared<Ellipsoid>(0.3, 0.2, 0.15)};
  std::vector<std::unique_ptr<CollisionObject>> owned;
  std::vector<CollisionObject*> objects;
  for (auto& g : geoms) {
    owned.emplace_back(new CollisionObject(g));
    objects.push_back(owned.back().get());
  }
  const size_t n_conf = 6, n = objects.size();
  std::vector<Transform3f> tables(n_conf * n);
  for (size_t c = 0; c < n_conf; ++c)
    for (size_t o = 0; o < n; ++o)  // a lattice over the field, lower with every configuration
      tables[c * n + o] = Transform3f(Vec3f(-0.7 + 0.35 * double(o), -1.0 + 0.4 * double((c + 2 * o) % 6), 1.7 - 0.2 * double(c) + 0.05 * double(o)));
  CollisionRequest req;
  req.num_max_contacts = 3;
  req.security_margin = 0.01;
  amd::Scene scene(objects, std::vector<std::pair<size_t, size_t>>());
  int hits = 0;
  bool ok = scene.numTerrainObjects() == 0;
  scene.setTerrain(&field, ftf);
  ok = check(scene, field, ftf, objects, {0, 1, 2, 3, 4}, tables, n_conf, req, hits, "every object") && ok;
  const int hits_all = hits;
  scene.setTerrain(&field, ftf, {1, 3, 4});
  ok = check(scene, field, ftf, objects, {1, 3, 4}, tables, n_conf, req, hits, "a list of objects") && ok;
  ok = ok && hits_all > 0 && hits_all < int(n_conf * n);
  // the heights updated under the terrain: the next call answers for the new ones
  MatrixXf low = h;
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 5; ++c) low(r, c) = 0.1;
  field.updateHeights(low);
  int hits_low = 0;
  ok = check(scene, field, ftf, objects, {1, 3, 4}, tables, n_conf, req, hits_low, "updated heights") && ok;
  ok = ok && hits_low < hits - hits_all;
  // a halfspace has no evaluator against a height field
  std::vector<CollisionObject*> with_flat = objects;
  CollisionObject flat(std::make_shared<Halfspace>(Vec3f(0, 0, 1), -5.0));
  with_flat.push_back(&flat);
  amd::Scene scene2(with_flat, std::vector<std::pair<size_t, size_t>>());
  bool refused = false;
  try {
    scene2.setTerrain(&field, ftf);
  } catch (const std::invalid_argument&) {
    refused = true;
  }
  scene2.setTerrain(&field, ftf, {0, 4});
  ok = ok && refused && scene2.numTerrainObjects() == 2;
  scene.clearTerrain();
  ok = ok && scene.numTerrainObjects() == 0;
  std::printf("hits %d of %zu, then %d; halfspace %s\n", hits_all, n_conf * n, hits_low, refused ? "refused" : "FAILED");
  std::printf(ok ? "terrain shim ok\n" : "terrain shim FAILED\n");
  return ok ? 0 : 1;
}
