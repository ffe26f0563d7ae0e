// C++ shim check of the culled scene calls (include/hppfcl_amd_compat.hpp: hpp::fcl::amd::Scene::cull / collideCulled / distanceCulled):
// all pairs of a few objects as the scene's list; per configuration the cull must keep exactly the pairs the host manager collects, the
// culled results must be the unculled Scene's results of those queries bit for bit, and the summaries' contacts the unculled ones.
// Built with g++ by tests/test_scene_cull_gpu.py; exits 0 on success.
#include <cstdio>
#include <cstring>
#include <memory>
#include <set>

#include "hppfcl_amd_compat.hpp"

using namespace hpp::fcl;

static int bad = 0;
#define CHECK(x)                                                    \
  do {                                                              \
    if (!(x)) {                                                     \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);    \
      ++bad;                                                        \
    }                                                               \
  } while (0)

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }
static bool same_result(const CollisionResult& a, const CollisionResult& b) {
  if (a.numContacts() != b.numContacts() || !same_bits(a.distance_lower_bound, b.distance_lower_bound)) return false;
  for (size_t k = 0; k < a.numContacts(); ++k) {
    const Contact &x = a.getContact(k), &y = b.getContact(k);
    if (x.o1 != y.o1 || x.o2 != y.o2 || !same_bits(x.penetration_depth, y.penetration_depth)) return false;
    for (int i = 0; i < 3; ++i)
      if (!same_bits(x.normal[i], y.normal[i]) || !same_bits(x.pos[i], y.pos[i])) return false;
  }
  return true;
}

int main() {
  unsigned state = 4321u;
  auto rnd = [&]() {
    state = state * 1664525u + 1013904223u;
    return double(state >> 8) / double(1u << 24);
  };
  std::vector<std::shared_ptr<CollisionGeometry>> geoms;
  for (int i = 0; i < 3; ++i) {
    geoms.push_back(std::make_shared<Box>(0.4 + rnd(), 0.4 + rnd(), 0.4 + rnd()));
    geoms.push_back(std::make_shared<Sphere>(0.3 + 0.5 * rnd()));
    geoms.push_back(std::make_shared<Capsule>(0.2 + 0.3 * rnd(), 0.5 + rnd()));
  }
  const size_t G = 30;
  std::vector<std::unique_ptr<CollisionObject>> owned;
  std::vector<CollisionObject*> objects;
  for (size_t i = 0; i < G; ++i) {
    owned.emplace_back(new CollisionObject(geoms[i % geoms.size()], Transform3f(Vec3f(4 * rnd(), 4 * rnd(), 4 * rnd()))));
    objects.push_back(owned.back().get());
  }
  std::vector<std::pair<size_t, size_t>> all;
  for (size_t i = 0; i < G; ++i)
    for (size_t j = i + 1; j < G; ++j) all.emplace_back(i, j);
  const size_t P = all.size();
  amd::Scene scene(objects, all);

  // two configurations: the objects' transforms, and the same moved along x by a per-object amount
  std::vector<Transform3f> tables(2 * G);
  for (size_t i = 0; i < G; ++i) {
    tables[i] = objects[i]->getTransform();
    tables[G + i] = Transform3f(objects[i]->getTransform().getTranslation() + Vec3f(rnd(), 0, 0));
  }
  std::vector<uint64_t> ids, conf_begin;
  scene.cull(tables.data(), 2, 0.0, ids, conf_begin);
  CHECK(conf_begin.size() == 3 && conf_begin[0] == 0 && conf_begin[2] == ids.size());
  // the host manager's pairs under each configuration
  size_t agree = 0;
  for (size_t c = 0; c < 2; ++c) {
    for (size_t i = 0; i < G; ++i) {
      objects[i]->setTransform(tables[c * G + i]);
    }
    DynamicAABBTreeCollisionManager manager;
    for (CollisionObject* o : objects) manager.registerObject(o);
    manager.setup();
    CollisionCallBackCollect collect(100000);
    manager.collide(&collect);
    std::set<uint64_t> expected;
    for (const auto& pr : collect.getCollisionPairs()) {
      size_t a = 0, b = 0;
      for (size_t i = 0; i < G; ++i) {
        if (objects[i] == pr.first) a = i;
        if (objects[i] == pr.second) b = i;
      }
      if (a > b) std::swap(a, b);
      for (size_t p = 0; p < P; ++p)
        if (all[p].first == a && all[p].second == b) expected.insert(c * P + p);
    }
    const std::set<uint64_t> got(ids.begin() + conf_begin[c], ids.begin() + conf_begin[c + 1]);
    CHECK(!expected.empty() && expected.size() < P);
    agree += got == expected;
  }
  CHECK(agree == 2);
  std::printf("cull: %zu of %zu queries survive, the manager's pairs %s\n", ids.size(), 2 * P, agree == 2 ? "same" : "DIFFERENT");

  CollisionRequest request;
  std::vector<CollisionResult> full, culled;
  std::vector<hfcl_scene_summary> full_summ, summ, summ_only;
  scene.collide(tables.data(), 2, request, &full, &full_summ);
  std::vector<uint64_t> ids2, cb2;
  scene.collideCulled(tables.data(), 2, 0.0, request, &culled, ids2, cb2, &summ);
  CHECK(ids2 == ids && cb2 == conf_begin && culled.size() == ids.size() && summ.size() == 2);
  size_t same = 0;
  for (size_t k = 0; k < culled.size(); ++k) same += same_result(culled[k], full[ids[k]]);
  CHECK(same == culled.size());
  bool contacts = true;
  for (size_t c = 0; c < 2; ++c)
    contacts = contacts && summ[c].n_contacts == full_summ[c].n_contacts && summ[c].first_contact == full_summ[c].first_contact;
  CHECK(contacts && full_summ[0].n_contacts > 0);
  scene.collideCulled(tables.data(), 2, 0.0, request, nullptr, ids2, cb2, &summ_only);
  CHECK(std::memcmp(summ_only.data(), summ.data(), 2 * sizeof(hfcl_scene_summary)) == 0);
  std::printf("collideCulled: results %s\n", same == culled.size() && contacts && bad == 0 ? "same" : "DIFFERENT");

  DistanceRequest drequest;
  std::vector<DistanceResult> dfull, dculled;
  scene.distance(tables.data(), 2, drequest, &dfull, nullptr);
  scene.distanceCulled(tables.data(), 2, 0.5, drequest, &dculled, ids2, cb2, &summ);
  CHECK(ids2.size() > ids.size() && dculled.size() == ids2.size());
  size_t dsame = 0;
  for (size_t k = 0; k < dculled.size(); ++k) dsame += same_bits(dculled[k].min_distance, dfull[ids2[k]].min_distance);
  CHECK(dsame == dculled.size());
  std::printf("distanceCulled: distances %s\n", dsame == dculled.size() && bad == 0 ? "same" : "DIFFERENT");

  bool threw = false;
  try {
    scene.cull(tables.data(), 2, -1.0, ids, conf_begin);
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  CHECK(threw);
  return bad == 0 ? 0 : 1;
}
