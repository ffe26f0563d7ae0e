// C++ shim check of scene queries (include/hppfcl_amd_compat.hpp: hpp::fcl::amd::Scene): the pairs a CollisionCallBackCollect holds after
// manager.collide, evaluated through a Scene, against amd::collide on the same pairs (result by result, bit for bit) and against the
// summaries' definition; several configurations through tables of transforms; summaries alone.  Built with g++ by
// tests/test_scene_gpu.py; exits 0 on success.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>

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
// the summary's definition, from per-pair results of one configuration
static hfcl_scene_summary fold(const CollisionResult* r, size_t n) {
  hfcl_scene_summary s{std::numeric_limits<double>::infinity(), 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u};
  for (size_t p = 0; p < n; ++p) {
    if (r[p].distance_lower_bound < s.min_distance) {
      s.min_distance = r[p].distance_lower_bound;
      s.min_pair = uint32_t(p);
    }
    if (r[p].isCollision()) {
      ++s.n_contacts;
      if (s.first_contact == 0xFFFFFFFFu) s.first_contact = uint32_t(p);
    }
  }
  return s;
}
static bool same_summary(const hfcl_scene_summary& a, const hfcl_scene_summary& b) {
  return same_bits(a.min_distance, b.min_distance) && a.min_pair == b.min_pair && a.first_contact == b.first_contact &&
         a.n_contacts == b.n_contacts && a.n_skipped == b.n_skipped;
}

int main() {
  unsigned state = 12345u;
  auto rnd = [&]() {
    state = state * 1664525u + 1013904223u;
    return double(state >> 8) / double(1u << 24);
  };
  std::vector<std::shared_ptr<CollisionGeometry>> geoms;
  for (int i = 0; i < 6; ++i) {
    geoms.push_back(std::make_shared<Box>(0.4 + rnd(), 0.4 + rnd(), 0.4 + rnd()));
    geoms.push_back(std::make_shared<Sphere>(0.3 + 0.5 * rnd()));
    geoms.push_back(std::make_shared<Capsule>(0.2 + 0.3 * rnd(), 0.5 + rnd()));
  }
  std::vector<std::unique_ptr<CollisionObject>> owned;
  std::vector<CollisionObject*> objects;
  for (int i = 0; i < 120; ++i) {
    owned.emplace_back(new CollisionObject(geoms[size_t(i) % geoms.size()], Transform3f(Vec3f(5 * rnd(), 5 * rnd(), 5 * rnd()))));
    objects.push_back(owned.back().get());
  }
  DynamicAABBTreeCollisionManager manager;
  for (CollisionObject* o : objects) manager.registerObject(o);
  manager.setup();
  CollisionCallBackCollect collect(100000);
  manager.collide(&collect);
  const auto& pairs = collect.getCollisionPairs();
  CHECK(pairs.size() > 50);

  CollisionRequest request;
  request.security_margin = 0.05;
  std::vector<CollisionResult> expected;
  amd::collide(pairs, request, expected);

  amd::Scene scene(objects, pairs);
  CHECK(scene.numPairs() == pairs.size() && scene.numObjects() == objects.size());
  std::vector<CollisionResult> got;
  std::vector<hfcl_scene_summary> summ, summ_only;
  scene.collide(request, &got, &summ);
  CHECK(got.size() == expected.size() && summ.size() == 1);
  size_t same = 0, colliding = 0;
  for (size_t p = 0; p < got.size() && p < expected.size(); ++p) {
    same += same_result(got[p], expected[p]);
    colliding += got[p].isCollision();
  }
  CHECK(same == expected.size());
  CHECK(colliding > 0 && colliding < got.size());
  CHECK(same_summary(summ[0], fold(got.data(), got.size())));
  scene.collide(request, nullptr, &summ_only);
  CHECK(summ_only.size() == 1 && same_summary(summ_only[0], summ[0]));
  std::printf("collected pairs: %zu, colliding %zu, results %s, summary %s\n", pairs.size(), colliding,
              same == expected.size() ? "same" : "DIFFERENT", same_summary(summ_only[0], summ[0]) ? "same" : "DIFFERENT");

  // three configurations: the current transforms, everything shifted apart (no contact), the current ones again
  const size_t G = objects.size(), P = scene.numPairs();
  std::vector<Transform3f> tables(3 * G);
  for (size_t i = 0; i < G; ++i) {
    tables[i] = tables[2 * G + i] = objects[i]->getTransform();
    tables[G + i] = Transform3f(Vec3f(10.0 * double(i), 0, 0));
  }
  scene.collide(tables.data(), 3, request, &got, &summ);
  CHECK(got.size() == 3 * P && summ.size() == 3);
  size_t same3 = 0;
  for (size_t p = 0; p < P; ++p) same3 += same_result(got[p], expected[p]) && same_result(got[2 * P + p], expected[p]);
  CHECK(same3 == P);
  CHECK(summ[1].n_contacts == 0 && summ[1].first_contact == 0xFFFFFFFFu && summ[1].min_distance > 0);
  for (size_t c = 0; c < 3; ++c) CHECK(same_summary(summ[c], fold(got.data() + c * P, P)));
  std::printf("three configurations: %s\n", same3 == P && bad == 0 ? "same" : "DIFFERENT");

  // a pair outside the objects is refused on the host
  bool threw = false;
  try {
    amd::Scene broken(objects, std::vector<std::pair<size_t, size_t>>{{0, G}});
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  CHECK(threw);
  return bad == 0 ? 0 : 1;
}
