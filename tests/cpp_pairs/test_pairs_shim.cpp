// C++ shim check of the self-pairs scene calls (include/hppfcl_amd_compat.hpp: hpp::fcl::amd::Scene::selfPairs / collideSelf / distanceSelf):
// a scene made WITHOUT a pair list must list, per configuration, exactly the pairs the cull keeps of a scene whose list is all pairs, in the
// same order; its results must be that scene's culled results bit for bit, and a summary's min_pair a rank inside the configuration.
// Built with g++ by tests/test_scene_pairs_gpu.py; exits 0 on success.
#include <cstdio>
#include <cstring>
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

int main() {
  unsigned state = 97531u;
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
  const size_t G = 70;  // (more than 64 objects: the tiled form; the guess of 16 entries per object holds the list)
  std::vector<std::unique_ptr<CollisionObject>> owned;
  std::vector<CollisionObject*> objects;
  for (size_t i = 0; i < G; ++i) {
    owned.emplace_back(new CollisionObject(geoms[i % geoms.size()], Transform3f(Vec3f(6 * rnd(), 6 * rnd(), 6 * rnd()))));
    objects.push_back(owned.back().get());
  }
  std::vector<std::pair<size_t, size_t>> all, none;
  for (size_t i = 0; i < G; ++i)
    for (size_t j = i + 1; j < G; ++j) all.emplace_back(i, j);
  const size_t P = all.size();
  amd::Scene listed(objects, all), scene(objects, none);
  std::vector<Transform3f> tables(2 * G);
  for (size_t i = 0; i < G; ++i) {
    tables[i] = objects[i]->getTransform();
    tables[G + i] = Transform3f(objects[i]->getTransform().getTranslation() + Vec3f(rnd(), 0, 0));
  }
  std::vector<uint64_t> ids, cb_ids, cb;
  std::vector<uint32_t> pairs;
  listed.cull(tables.data(), 2, 0.0, ids, cb_ids);
  scene.selfPairs(tables.data(), 2, 0.0, pairs, cb);
  CHECK(!ids.empty() && pairs.size() == 2 * ids.size() && cb == cb_ids);
  size_t same = 0;
  for (size_t k = 0; k < ids.size() && 2 * k + 1 < pairs.size(); ++k)
    same += pairs[2 * k] == all[ids[k] % P].first && pairs[2 * k + 1] == all[ids[k] % P].second;
  CHECK(same == ids.size());
  std::printf("selfPairs: %zu pairs, the cull of the all-pairs list %s\n", ids.size(), same == ids.size() && bad == 0 ? "same" : "DIFFERENT");

  CollisionRequest request;
  std::vector<CollisionResult> culled, self;
  std::vector<hfcl_scene_summary> summ_culled, summ, summ_only;
  std::vector<uint64_t> ids2, cb2;
  std::vector<uint32_t> pairs2;
  listed.collideCulled(tables.data(), 2, 0.0, request, &culled, ids2, cb2, &summ_culled);
  scene.collideSelf(tables.data(), 2, 0.0, request, &self, pairs2, cb2, &summ);
  CHECK(pairs2 == pairs && cb2 == cb && self.size() == culled.size() && summ.size() == 2);
  same = 0;
  for (size_t k = 0; k < self.size() && k < culled.size(); ++k) same += same_result(self[k], culled[k]);
  CHECK(same == self.size());
  bool ranks = true;
  for (size_t c = 0; c < 2; ++c) {  // a summary names a pair by its rank in the configuration: the culled summary names the same pair by p
    ranks = ranks && summ[c].n_contacts == summ_culled[c].n_contacts && same_bits(summ[c].min_distance, summ_culled[c].min_distance);
    ranks = ranks && summ[c].min_pair != 0xFFFFFFFFu && ids[cb[c] + summ[c].min_pair] % P == summ_culled[c].min_pair;
  }
  CHECK(ranks && summ[0].n_contacts > 0);
  scene.collideSelf(tables.data(), 2, 0.0, request, nullptr, pairs2, cb2, &summ_only);
  CHECK(std::memcmp(summ_only.data(), summ.data(), 2 * sizeof(hfcl_scene_summary)) == 0);
  std::printf("collideSelf: results %s\n", same == self.size() && ranks && bad == 0 ? "same" : "DIFFERENT");

  DistanceRequest drequest;
  std::vector<DistanceResult> dculled, dself;
  listed.distanceCulled(tables.data(), 2, 0.5, drequest, &dculled, ids2, cb2, &summ_culled);
  scene.distanceSelf(tables.data(), 2, 0.5, drequest, &dself, pairs2, cb, &summ);
  CHECK(dself.size() == dculled.size() && dself.size() > self.size() && cb == cb2);
  size_t dsame = 0;
  for (size_t k = 0; k < dself.size() && k < dculled.size(); ++k) dsame += same_bits(dself[k].min_distance, dculled[k].min_distance);
  CHECK(dsame == dself.size());
  std::printf("distanceSelf: distances %s\n", dsame == dself.size() && bad == 0 ? "same" : "DIFFERENT");

  // a list longer than the guess (1024 entries for a few objects): every pair of 60 objects at one place, the call repeated with the length
  std::vector<Transform3f> heap(60);
  std::vector<CollisionObject*> few(objects.begin(), objects.begin() + 60);
  amd::Scene crowd(few, none);
  crowd.selfPairs(heap.data(), 1, 0.0, pairs, cb);
  CHECK(pairs.size() == 2 * 1770 && cb[1] == 1770 && pairs[2 * 1769] == 58 && pairs[2 * 1769 + 1] == 59);
  bool threw = false;
  try {
    scene.selfPairs(tables.data(), 2, -1.0, pairs, cb);
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  CHECK(threw);
  return bad == 0 ? 0 : 1;
}
