// C++ shim check of the clearance among a kept environment (include/hppfcl_amd_compat.hpp: hpp::fcl::amd::Scene::nearestEnv): with and
// without groups its clearances, from tables of the moving objects alone, must be what Scene::distance gives on a second scene that
// holds P_env -- every allowed pair with a moving object in it -- as an explicit lexicographic list on the full tables: min_distance bit
// for bit, the pair, the closest pair's DistanceResult; and what Scene::nearest counts there.
// Built with g++ by tests/test_scene_nearest_env_gpu.py; exits 0 on success.
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
static bool same_result(const DistanceResult& a, const DistanceResult& b) {
  if (!same_bits(a.min_distance, b.min_distance) || a.o1 != b.o1 || a.o2 != b.o2 || a.b1 != b.b1 || a.b2 != b.b2) return false;
  for (int i = 0; i < 3; ++i)
    if (!same_bits(a.normal[i], b.normal[i]) || !same_bits(a.nearest_points[0][i], b.nearest_points[0][i]) ||
        !same_bits(a.nearest_points[1][i], b.nearest_points[1][i]))
      return false;
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
  const size_t K = 17, E = 300, G = K + E, n_conf = 3;  // (a row block of one row; two environment tiles)
  std::vector<std::unique_ptr<CollisionObject>> owned;
  std::vector<CollisionObject*> objects;
  for (size_t i = 0; i < G; ++i) {
    // the environment in two slabs along x, a tile each; the moving objects beside the first
    const double x = i < K ? 9 * rnd() : (i - K < 256 ? 9 * rnd() : 30 + 9 * rnd());
    owned.emplace_back(new CollisionObject(geoms[i % geoms.size()], Transform3f(Vec3f(x, 9 * rnd(), i < K ? 11 + 4 * rnd() : 9 * rnd()))));
    objects.push_back(owned.back().get());
  }
  std::vector<Transform3f> moving(n_conf * K), full(n_conf * G), env(E);
  for (size_t e = 0; e < E; ++e) env[e] = objects[K + e]->getTransform();
  for (size_t c = 0; c < n_conf; ++c)
    for (size_t i = 0; i < G; ++i) {
      full[c * G + i] = i < K ? Transform3f(objects[i]->getTransform().getTranslation() + Vec3f(c * rnd(), 0, -1.5 * double(c))) : env[i - K];
      if (i < K) moving[c * K + i] = full[c * G + i];
    }
  const std::vector<std::pair<size_t, size_t>> none;
  amd::Scene scene(objects, none);
  scene.setEnvironment(K, env);
  CHECK(scene.numMoving() == K);
  const double inf = std::numeric_limits<double>::infinity();
  DistanceRequest request;

  std::vector<uint8_t> group(G, 2);
  for (size_t i = 0; i < K; ++i) group[i] = uint8_t(i % 2);
  const std::vector<uint64_t> collides = {6, 5, 3};  // the moving objects in two halves that do not pair inside themselves
  for (int with_groups = 0; with_groups < 2; ++with_groups) {
    std::vector<std::pair<size_t, size_t>> P;
    for (size_t i = 0; i < K; ++i)
      for (size_t j = i + 1; j < G; ++j)
        if (!with_groups || ((collides[group[i]] >> group[j]) & 1u)) P.push_back({i, j});
    amd::Scene listed(objects, P);
    std::vector<DistanceResult> all;
    std::vector<hfcl_scene_summary> full_summ, near_summ;
    listed.distance(full.data(), n_conf, request, &all, &full_summ);
    size_t near_n[2] = {0, 0};
    listed.nearest(full.data(), n_conf, request, inf, near_summ, nullptr, near_n);

    if (with_groups) scene.setGroups(group, collides);
    std::vector<hfcl_scene_clearance> clear;
    std::vector<DistanceResult> res;
    size_t n[2] = {99, 99};
    scene.nearestEnv(moving.data(), n_conf, request, inf, clear, &res, n);
    CHECK(clear.size() == n_conf && res.size() == n_conf);
    size_t same = 0, evaluated = 0;
    for (size_t c = 0; c < n_conf && c < clear.size(); ++c) {
      const uint32_t mp = full_summ[c].min_pair;
      CHECK(mp < P.size());
      const bool ok = same_bits(clear[c].min_distance, full_summ[c].min_distance) && clear[c].min_i == P[mp].first && clear[c].min_j == P[mp].second &&
                      same_result(res[c], all[c * P.size() + mp]) && clear[c].n_skipped == near_summ[c].n_skipped;
      same += ok;
      evaluated += clear[c].n_evaluated;
    }
    CHECK(same == n_conf);
    CHECK(n[0] == near_n[0] && n[1] == near_n[1] && evaluated == n[0] + n[1] && evaluated < n_conf * P.size() / 4);
    std::printf("nearestEnv %s groups: %zu + %zu of %zu candidates evaluated, clearances %s\n", with_groups ? "with" : "without", n[0], n[1],
                n_conf * P.size(), same == n_conf && bad == 0 ? "same" : "DIFFERENT");

    // clearances alone, with a bound
    std::vector<hfcl_scene_clearance> bounded;
    scene.nearestEnv(moving.data(), n_conf, request, 0.25, bounded);
    size_t held = 0;
    for (size_t c = 0; c < n_conf; ++c)
      held += full_summ[c].min_distance <= 0.25 ? same_bits(bounded[c].min_distance, full_summ[c].min_distance) : bounded[c].min_distance > 0.25;
    CHECK(held == n_conf);
    std::printf("nearestEnv %s groups, upper bound 0.25: %s\n", with_groups ? "with" : "without", held == n_conf ? "same" : "DIFFERENT");
  }
  return bad == 0 ? 0 : 1;
}
