// TEST INFRASTRUCTURE: host build of the contact-patch device header (hpp-fcl_amd/csrc/hfcl_patch.hpp) with g++, built by
// tests/test_contact_patch_cpu.py into a temporary directory.  ph_patches runs the records one after the other exactly as
// k_patch_classify / k_patch_sets do on the device; ph_sort_check holds the header's restatement of libstdc++'s
// std::stable_sort against std::stable_sort itself with the hull's comparator (which is not a strict weak order).
#include <algorithm>
#include <vector>

#include "../../hpp-fcl_amd/csrc/hfcl_patch.hpp"

using namespace hfcl;

static DShape<double> dshape(const hfcl_shape& s) {
  DShape<double> d;
  d.kind = s.type;
  d.num_points = s.num_points;
  d.vertex_offset = s.vertex_offset;
  d.bvh_index = s.bvh_index;
  d.p0 = s.params[0]; d.p1 = s.params[1]; d.p2 = s.params[2]; d.p3 = s.params[3];
  d.ssr = s.swept_sphere_radius;
  return d;
}

extern "C" int ph_patches(const hfcl_shape* shapes, uint32_t n_shapes, const double* verts, const uint32_t* graph_base,
                          const uint32_t* graph_off, const uint32_t* graph_ids, const uint32_t* s1, const uint32_t* s2,
                          const double* tf1, const double* tf2, const hfcl_result* rec, const hfcl_guess* guess, size_t n,
                          uint32_t max_num_patch, uint32_t ns, double tol, uint32_t pcap, hfcl_contact_patch* out, double* out_pts) {
  if (ns < 3) ns = 3;
  if (tol < 0) tol = 1e-12;
  uint32_t m = 1, cloud_cap = 8, vis_cap = 0;
  for (uint32_t k = 0; k < n_shapes; ++k) {
    m = std::max(m, patch_set_bound(shapes[k].type, shapes[k].num_points, ns));
    if (shapes[k].type == HFCL_GEOM_CONVEX) {
      cloud_cap = std::max(cloud_cap, shapes[k].num_points);
      vis_cap = std::max(vis_cap, shapes[k].num_points);
    }
  }
  const uint32_t cap = 2 * m;
  std::vector<P2> poly(3 * size_t(cap)), cloud(cloud_cap), sortbuf(cloud_cap / 2 + 1);
  std::vector<uint8_t> visited(vis_cap + 1);
  std::vector<uint32_t> stack(2 * size_t(vis_cap) + 2);
  PatchWs ws;
  ws.poly0 = poly.data();
  ws.poly1 = poly.data() + cap;
  ws.poly2 = poly.data() + 2 * size_t(cap);
  ws.cloud = cloud.data();
  ws.sortbuf = sortbuf.data();
  ws.visited = visited.data();
  ws.stack = stack.data();
  ws.cap = cap;
  ws.cloud_cap = cloud_cap;
  ws.vis_cap = vis_cap;
  for (size_t i = 0; i < n; ++i) {
    hfcl_contact_patch o;
    const uint32_t i1 = s1[i], i2 = s2[i];
    if (i1 >= n_shapes || i2 >= n_shapes) {
      patch_write_none(o, patch_status(PATCH_NONE, false, false, true));
      out[i] = o;
      continue;
    }
    bool swapped = false;
    const int cls = patch_class(shapes[i1].type, shapes[i2].type, rec[i], max_num_patch, swapped);
    if (cls == PATCH_NONE) {
      patch_write_none(o, patch_status(PATCH_NONE, false, false, false));
      out[i] = o;
      continue;
    }
    const Pose<double> fr = patch_frame(rec[i]);
    patch_write_frame(o, fr, rec[i].distance, swapped);
    if (cls == PATCH_POINT) {
      const P2 p = patch_origin(fr);
      o.num_points = 1;
      o.status = patch_status(cls, swapped, false, false);
      out[i] = o;
      out_pts[2 * i * pcap] = swapped ? -p.x : p.x;
      out_pts[2 * i * pcap + 1] = p.y;
      continue;
    }
    const DShape<double> d1 = dshape(shapes[i1]), d2 = dshape(shapes[i2]);
    auto graph = [&](uint32_t id, const DShape<double>& s) {
      PatchGraph g{nullptr, nullptr, nullptr};
      if (s.kind == K_CONVEX && s.num_points > 32u && graph_base && graph_base[id] != 0xFFFFFFFFu) {
        g.off = graph_off + graph_base[id];
        g.ids = graph_ids;
      }
      return g;
    };
    int g0 = 0, g1 = 0;
    if (guess) {
      g0 = guess[i].support_guess[0];
      g1 = guess[i].support_guess[1];
    }
    ws.overflow = false;
    const uint32_t np = patch_compute(ws, d1, pose_from_abi<double>(tf1 + 12 * i), graph(i1, d1), d2, pose_from_abi<double>(tf2 + 12 * i),
                                      graph(i2, d2), verts, fr, g0, g1, ns, tol, reinterpret_cast<P2*>(out_pts + 2 * i * pcap), pcap);
    o.num_points = ws.overflow ? 0u : np;
    o.status = patch_status(cls, false, ws.overflow, false);
    out[i] = o;
  }
  return 0;
}

// pts: m clouds of k points (x, y); v: m pivots.  Returns the number of clouds the two sorts order differently.
extern "C" int ph_sort_check(const double* pts, const double* v, size_t m, uint32_t k) {
  int bad = 0;
  std::vector<P2> a(k), b(k), buf(k / 2 + 1);
  for (size_t c = 0; c < m; ++c) {
    const P2 piv{v[2 * c], v[2 * c + 1]};
    for (uint32_t j = 0; j < k; ++j) a[j] = b[j] = P2{pts[2 * (c * k + j)], pts[2 * (c * k + j) + 1]};
    stable_sort_cloud(a.data(), k, buf.data(), piv);
    std::stable_sort(b.begin(), b.end(), [&](const P2& p, const P2& q) { return hull_less(p, q, piv); });
    for (uint32_t j = 0; j < k; ++j)
      if (a[j].x != b[j].x || a[j].y != b[j].y) {
        ++bad;
        break;
      }
  }
  return bad;
}
