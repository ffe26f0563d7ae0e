// C++ shim check of the pruned minimum distance (include/hppfcl_amd_compat.hpp: hpp::fcl::amd::Scene::nearest): all pairs of a few
// objects as the scene's list, two configurations; the summaries' min_distance / min_pair must be those of the unculled Scene::distance
// bit for bit, and the per-configuration DistanceResult must be the closest pair's.
// Built with g++ by tests/test_scene_nearest_gpu.py; exits 0 on success.
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
  const size_t G = 20;
  std::vector<std::unique_ptr<CollisionObject>> owned;
  std::vector<CollisionObject*> objects;
  for (size_t i = 0; i < G; ++i) {
    owned.emplace_back(new CollisionObject(geoms[i % geoms.size()], Transform3f(Vec3f(9 * rnd(), 9 * rnd(), 9 * rnd()))));
    objects.push_back(owned.back().get());
  }
  std::vector<std::pair<size_t, size_t>> all;
  for (size_t i = 0; i < G; ++i)
    for (size_t j = i + 1; j < G; ++j) all.emplace_back(i, j);
  const size_t P = all.size();
  amd::Scene scene(objects, all);
  std::vector<Transform3f> tables(2 * G);
  for (size_t i = 0; i < G; ++i) {
    tables[i] = objects[i]->getTransform();
    tables[G + i] = Transform3f(objects[i]->getTransform().getTranslation() + Vec3f(3 * rnd(), 0, 0));
  }

  DistanceRequest request;
  std::vector<DistanceResult> full, near;
  std::vector<hfcl_scene_summary> full_summ, summ, summ_only;
  scene.distance(tables.data(), 2, request, &full, &full_summ);
  size_t evaluated[2] = {0, 0};
  scene.nearest(tables.data(), 2, request, std::numeric_limits<double>::infinity(), summ, &near, evaluated);
  CHECK(summ.size() == 2 && near.size() == 2);
  size_t same = 0;
  for (size_t c = 0; c < 2 && summ.size() == 2; ++c)
    same += same_bits(summ[c].min_distance, full_summ[c].min_distance) && summ[c].min_pair == full_summ[c].min_pair;
  CHECK(same == 2);
  CHECK(evaluated[0] >= 2 && evaluated[0] + evaluated[1] < 2 * P);
  std::printf("nearest: %zu + %zu of %zu queries evaluated, summaries %s\n", evaluated[0], evaluated[1], 2 * P, same == 2 ? "same" : "DIFFERENT");
  size_t rsame = 0;
  for (size_t c = 0; c < 2 && near.size() == 2; ++c) {
    const DistanceResult& e = full[c * P + full_summ[c].min_pair];
    const DistanceResult& g = near[c];
    bool ok = same_bits(g.min_distance, e.min_distance) && g.o1 == e.o1 && g.o2 == e.o2 && g.b1 == e.b1 && g.b2 == e.b2;
    for (int i = 0; i < 3; ++i)
      ok = ok && same_bits(g.nearest_points[0][i], e.nearest_points[0][i]) && same_bits(g.nearest_points[1][i], e.nearest_points[1][i]) &&
           same_bits(g.normal[i], e.normal[i]);
    rsame += ok;
  }
  CHECK(rsame == 2);
  scene.nearest(tables.data(), 2, request, std::numeric_limits<double>::infinity(), summ_only, nullptr);
  CHECK(summ_only.size() == 2 && std::memcmp(summ_only.data(), summ.data(), 2 * sizeof(hfcl_scene_summary)) == 0);
  std::printf("nearest: results %s\n", rsame == 2 && bad == 0 ? "same" : "DIFFERENT");

  bool threw = false;
  try {
    scene.nearest(tables.data(), 2, request, std::numeric_limits<double>::quiet_NaN(), summ, nullptr);
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  CHECK(threw);
  return bad == 0 ? 0 : 1;
}
