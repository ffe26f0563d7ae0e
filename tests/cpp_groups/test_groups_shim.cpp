// C++ shim check of object groups (include/hppfcl_amd_compat.hpp: hpp::fcl::amd::Scene::setGroups / clearGroups / numGroups): with groups
// set, selfPairs must list exactly the entries of the list without groups whose groups may pair -- filtered here on the host --, in the
// same order; collideSelf's results must be the results of those entries bit for bit; clearGroups brings the whole list back; a matrix
// that is not symmetric is a std::invalid_argument and leaves the groups in force.
// Built with g++ by tests/test_scene_groups_gpu.py; exits 0 on success.
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
  unsigned state = 24680u;
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
  const size_t G = 70, n_a = 17;  // (more than 64 objects: the tiled form; a split off a 16-row block edge)
  std::vector<std::unique_ptr<CollisionObject>> owned;
  std::vector<CollisionObject*> objects;
  for (size_t i = 0; i < G; ++i) {
    owned.emplace_back(new CollisionObject(geoms[i % geoms.size()], Transform3f(Vec3f(5 * rnd(), 5 * rnd(), 5 * rnd()))));
    objects.push_back(owned.back().get());
  }
  const std::vector<std::pair<size_t, size_t>> none;
  amd::Scene scene(objects, none);
  std::vector<Transform3f> tables(2 * G);
  for (size_t i = 0; i < G; ++i) {
    tables[i] = objects[i]->getTransform();
    tables[G + i] = Transform3f(objects[i]->getTransform().getTranslation() + Vec3f(rnd(), 0, 0));
  }
  // the list without groups and its results
  CollisionRequest request;
  std::vector<uint32_t> all, pairs;
  std::vector<uint64_t> cb_all, cb;
  std::vector<CollisionResult> res_all, res;
  std::vector<hfcl_scene_summary> summ_all, summ;
  CHECK(scene.numGroups() == 0);
  scene.collideSelf(tables.data(), 2, 0.0, request, &res_all, all, cb_all, &summ_all);
  CHECK(all.size() >= 40 && cb_all.size() == 3);

  // two managers: objects [0, n_a) against [n_a, G)
  std::vector<uint8_t> group(G, 1);
  for (size_t i = 0; i < n_a; ++i) group[i] = 0;
  const std::vector<uint64_t> collides = {2, 1};
  auto filtered = [&](std::vector<uint32_t>& want, std::vector<uint64_t>& want_cb, std::vector<size_t>& from) {
    want.clear();
    from.clear();
    want_cb.assign(3, 0);
    for (size_t c = 0; c < 2; ++c) {
      for (uint64_t k = cb_all[c]; k < cb_all[c + 1]; ++k)
        if ((collides[group[all[2 * k]]] >> group[all[2 * k + 1]]) & 1u) {
          want.push_back(all[2 * k]);
          want.push_back(all[2 * k + 1]);
          from.push_back(size_t(k));
        }
      want_cb[c + 1] = want.size() / 2;
    }
  };
  std::vector<uint32_t> want;
  std::vector<uint64_t> want_cb;
  std::vector<size_t> from;
  filtered(want, want_cb, from);
  CHECK(!want.empty() && want.size() < all.size());
  scene.setGroups(group, collides);
  CHECK(scene.numGroups() == 2);
  scene.selfPairs(tables.data(), 2, 0.0, pairs, cb);
  CHECK(pairs == want && cb == want_cb);
  std::printf("setGroups + selfPairs: %zu of %zu pairs, the list filtered on the host %s\n", pairs.size() / 2, all.size() / 2,
              pairs == want && cb == want_cb ? "same" : "DIFFERENT");

  scene.collideSelf(tables.data(), 2, 0.0, request, &res, pairs, cb, &summ);
  CHECK(pairs == want && cb == want_cb && res.size() == from.size() && summ.size() == 2);
  size_t same = 0, contacts[2] = {0, 0};
  for (size_t k = 0; k < res.size() && k < from.size(); ++k) {
    same += same_result(res[k], res_all[from[k]]);
    contacts[k >= want_cb[1]] += res[k].isCollision();
  }
  CHECK(same == res.size());
  CHECK(summ[0].n_contacts == contacts[0] && summ[1].n_contacts == contacts[1]);
  std::printf("collideSelf with groups: results %s\n", same == res.size() && bad == 0 ? "same" : "DIFFERENT");

  // a refused matrix leaves the groups in force; clearGroups brings the whole list back
  bool threw = false;
  try {
    scene.setGroups(group, {2, 0});
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  CHECK(threw && scene.numGroups() == 2);
  scene.selfPairs(tables.data(), 2, 0.0, pairs, cb);
  CHECK(pairs == want && cb == want_cb);
  scene.clearGroups();
  CHECK(scene.numGroups() == 0);
  scene.selfPairs(tables.data(), 2, 0.0, pairs, cb);
  CHECK(pairs == all && cb == cb_all);
  std::printf("refusal and clearGroups: lists %s\n", threw && pairs == all && bad == 0 ? "same" : "DIFFERENT");
  return bad == 0 ? 0 : 1;
}
