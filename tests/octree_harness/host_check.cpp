// TEST INFRASTRUCTURE: the host-only parts of hpp-fcl_amd/csrc/hfcl_octree.hpp -- the validator and the builder from points -- in a
// stand-alone program: built and run by tests/test_octree_cpu.py with plain g++; the same line with -fsanitize=address,undefined is
// how these two are run under a sanitizer (nothing here touches a device or is loaded into another process).
// Prints "host_check ok" and returns 0, or says what failed.
#include <cstdio>
#include <cstdlib>
#include <map>

#include "../../hpp-fcl_amd/csrc/hfcl_octree.hpp"

using namespace hfcl;

static int fails = 0;
#define CHECK(c)                                            \
  do {                                                      \
    if (!(c)) {                                             \
      std::printf("FAILED line %d: %s\n", __LINE__, #c);    \
      ++fails;                                              \
    }                                                       \
  } while (0)

static uint64_t lcg(uint64_t& s) {
  s = s * 6364136223846793005ull + 1442695040888963407ull;
  return s >> 33;
}

int main() {
  std::string why;
  uint64_t seed = 7;
  for (uint32_t depth : {1u, 2u, 5u, 16u}) {
    for (int n : {0, 1, 17, 400}) {
      std::vector<double> xyz(3 * size_t(n));
      const double side = double(1u << depth) * 0.1;
      for (double& x : xyz) x = (double(lcg(seed) % 100000) / 100000.0 - 0.5) * 1.3 * side;  // some outside
      if (n >= 17) {
        for (int k = 0; k < 3; ++k) xyz[3 + k] = xyz[k];  // a voxel hit twice
        xyz[6] = __builtin_nan("");
        xyz[11] = __builtin_inf();
      }
      std::vector<hfcl_octree_node> nodes;
      CHECK(oct_from_points(xyz.data(), size_t(n), 0.1, depth, nodes, &why) == HFCL_OK);
      CHECK(oct_validate(nodes.data(), nodes.size(), depth, &why) == HFCL_OK);
      // the leaves are the distinct keys inside the map
      std::map<std::vector<long>, int> keys;
      for (int i = 0; i < n; ++i) {
        std::vector<long> key;
        for (int k = 0; k < 3; ++k) {
          const double kd = std::floor(xyz[3 * i + k] / 0.1) + double(1u << (depth - 1u));
          if (kd >= 0.0 && kd < double(1u << depth)) key.push_back(long(kd));
        }
        if (key.size() == 3) ++keys[key];
      }
      size_t leaves = 0;
      for (const hfcl_octree_node& nd : nodes) {
        bool any = false;
        for (int k = 0; k < 8; ++k) any = any || nd.child[k];
        leaves += any ? 0 : 1;
        CHECK(nd.occupancy >= 0.7 && nd.occupancy <= 0.97);
      }
      CHECK(leaves == keys.size());
      CHECK(nodes.empty() == keys.empty());
      // every refusal of the validator on a copy of this tree
      if (nodes.size() >= 3) {
        std::vector<hfcl_octree_node> t = nodes;
        t[1].child[7] = uint32_t(t.size());
        CHECK(oct_validate(t.data(), t.size(), depth, &why) == HFCL_ERR_INVALID_ARGUMENT);
        t = nodes;
        t.back().occupancy = __builtin_nan("");
        CHECK(oct_validate(t.data(), t.size(), depth, &why) == HFCL_ERR_INVALID_ARGUMENT);
        t = nodes;
        for (int k = 0; k < 8; ++k)
          if (t[0].child[k]) {
            t[0].child[k] = 0;  // an orphan
            break;
          }
        CHECK(oct_validate(t.data(), t.size(), depth, &why) == HFCL_ERR_INVALID_ARGUMENT);
        t = nodes;
        t.back().child[0] = 1;  // a second parent for node 1 (and a cycle)
        CHECK(oct_validate(t.data(), t.size(), depth, &why) == HFCL_ERR_INVALID_ARGUMENT);
        if (depth > 1) CHECK(oct_validate(nodes.data(), nodes.size(), depth - 1, &why) == HFCL_ERR_INVALID_ARGUMENT);
      }
    }
  }
  std::vector<hfcl_octree_node> none;
  double p[3] = {0, 0, 0};
  CHECK(oct_from_points(p, 1, 0.0, 4, none, &why) == HFCL_ERR_INVALID_ARGUMENT);
  CHECK(oct_from_points(p, 1, 0.1, 0, none, &why) == HFCL_ERR_INVALID_ARGUMENT);
  CHECK(oct_from_points(p, 1, 0.1, 17, none, &why) == HFCL_ERR_INVALID_ARGUMENT);
  CHECK(oct_from_points(nullptr, 1, 0.1, 4, none, &why) == HFCL_ERR_INVALID_ARGUMENT);
  CHECK(oct_validate(nullptr, 0, 4, &why) == HFCL_OK);
  CHECK(oct_validate(nullptr, 3, 4, &why) == HFCL_ERR_INVALID_ARGUMENT);
  CHECK(oct_validate(nullptr, 0, 0, &why) == HFCL_ERR_INVALID_ARGUMENT);
  // two nodes that name each other beside a root that names neither: one parent each, and a cycle
  hfcl_octree_node cyc[3] = {};
  cyc[0].occupancy = cyc[1].occupancy = cyc[2].occupancy = 0.8;
  cyc[1].child[0] = 2;
  cyc[2].child[0] = 1;
  CHECK(oct_validate(cyc, 3, 4, &why) == HFCL_ERR_INVALID_ARGUMENT);
  if (!fails) std::printf("host_check ok\n");
  return fails ? 1 : 0;
}
