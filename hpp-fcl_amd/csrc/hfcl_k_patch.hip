// hfcl_k_patch.hip -- contact patches of collide() records (hfcl_contact_patch_batch*), fp64, built without contraction.
//   k_patch_classify        one record per lane: the class of its pair (hfcl_patch.hpp: patch_class); records without a
//                           patch and point patches are finished here (frame + Contact::pos), the others are appended to the
//                           list of their class
//   k_patch_sets<CLS>       one record of the class's list per lane, a workspace slot per lane for its polygons: the
//                           one-sided rows (Plane / Halfspace x a shape: that shape's support set) and the clipped pairs
//                           (two support sets, Sutherland-Hodgman) in launches of their own, so that a wave of short
//                           one-sided records does not wait on a wave's longest clipping
#include "hfcl_dev.hpp"
#include "hfcl_launch.hpp"
#include "hfcl_patch.hpp"

static __device__ __forceinline__ PatchGraph patch_graph(const PatchArgs& a, uint32_t shape_id, const DShape<double>& s) {
  PatchGraph g{nullptr, nullptr, nullptr};
  if (s.kind != K_CONVEX || s.num_points <= 32u || a.graph_base == nullptr) return g;
  const uint32_t base = a.graph_base[shape_id];
  if (base == HFCL_NO_GRAPH) return g;
  g.off = a.graph_off + base;
  g.ent = a.graph_ent;
  return g;
}

__global__ void __launch_bounds__(256) k_patch_classify(PatchArgs a) {
  // (the loop bound is uniform over the wave: every lane reaches the list appends below together)
  // (64-bit index: n may come within one grid stride of 2^32)
  for (uint64_t i0 = uint64_t(blockIdx.x) * 256u; i0 < a.n; i0 += uint64_t(gridDim.x) * 256u) {
    const uint32_t i = uint32_t(i0) + threadIdx.x;
    const bool live = i0 + threadIdx.x < a.n;
    int cls = PATCH_NONE;
    if (live) {
      hfcl_contact_patch o;
      const uint32_t i1 = a.s1[i], i2 = a.s2[i];
      if (i1 >= a.n_shapes || i2 >= a.n_shapes) {
        patch_write_none(o, patch_status(PATCH_NONE, false, false, true));
      } else {
        const hfcl_result r = a.rec[i];
        bool swapped = false;
        cls = patch_class(a.shapes[i1].kind, a.shapes[i2].kind, r, a.max_num_patch, swapped);
        if (cls == PATCH_NONE) {
          patch_write_none(o, patch_status(PATCH_NONE, false, false, false));
        } else {
          const Pose<double> fr = patch_frame(r);
          patch_write_frame(o, fr, r.distance, swapped);
          o.status = patch_status(cls, swapped, false, false);
          o.num_points = 0;
          if (cls == PATCH_POINT) {
            const P2 p = patch_origin(fr);
            o.num_points = 1;
            // (swapObjects negates x of point(i), not point(j): with one point at the origin that is -0 or 0 alike)
            a.out_pts[2 * size_t(i) * a.pcap] = swapped ? -p.x : p.x;
            a.out_pts[2 * size_t(i) * a.pcap + 1] = p.y;
          }
        }
      }
      a.out[i] = o;
    }
    // append the one-sided / clipped records to their lists: one atomic per wave and class
    for (int c = PATCH_ONESIDED; c <= PATCH_CLIPPED; ++c) {
      const uint64_t mask = __ballot(cls == c);
      if (mask == 0) continue;
      const int leader = __ffsll((unsigned long long)mask) - 1;
      uint32_t base = 0;
      if (int(__lane_id()) == leader) base = atomicAdd(&a.counts[c - PATCH_ONESIDED], uint32_t(__popcll(mask)));
      base = __shfl(base, leader);
      if (cls == c) a.lists[size_t(c - PATCH_ONESIDED) * a.n + base + __popcll(mask & __lanemask_lt())] = i;
    }
  }
}

template <int CLS>
__global__ void __launch_bounds__(256) k_patch_sets(PatchArgs a) {
  const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
  if (slot >= a.nslots) return;
  char* base = a.ws + size_t(slot) * a.slot_bytes;
  PatchWs ws;
  ws.cap = a.cap;
  ws.cloud_cap = a.cloud_cap;
  ws.vis_cap = a.vis_cap;
  ws.poly0 = reinterpret_cast<P2*>(base);
  ws.poly1 = ws.poly0 + a.cap;
  ws.poly2 = ws.poly1 + a.cap;
  ws.cloud = ws.poly2 + a.cap;
  ws.sortbuf = ws.cloud + a.cloud_cap;
  ws.stack = reinterpret_cast<uint32_t*>(ws.sortbuf + (a.cloud_cap / 2 + 1));
  ws.visited = reinterpret_cast<uint8_t*>(ws.stack + 2 * size_t(a.vis_cap));
  const uint32_t cnt = a.counts[CLS - PATCH_ONESIDED];
  const uint32_t* list = a.lists + size_t(CLS - PATCH_ONESIDED) * a.n;
  for (uint64_t k = slot; k < cnt; k += a.nslots) {
    const uint32_t i = list[k];
    const uint32_t i1 = a.s1[i], i2 = a.s2[i];
    const DShape<double> s1 = a.shapes[i1], s2 = a.shapes[i2];
    const Pose<double> tf1 = load_pose(a.tf1, i), tf2 = load_pose(a.tf2, i);
    const hfcl_result r = a.rec[i];
    int g0 = 0, g1 = 0;
    if (a.guess) {
      g0 = a.guess[i].support_guess[0];
      g1 = a.guess[i].support_guess[1];
    }
    const Pose<double> fr = patch_frame(r);
    ws.overflow = false;
    P2* pts = reinterpret_cast<P2*>(a.out_pts + 2 * size_t(i) * a.pcap);
    const uint32_t np = patch_compute(ws, s1, tf1, patch_graph(a, i1, s1), s2, tf2, patch_graph(a, i2, s2), a.verts, fr, g0, g1,
                                      a.num_samples, a.tol, pts, a.plim);
    a.out[i].num_points = ws.overflow ? 0u : np;
    a.out[i].status = patch_status(CLS, false, ws.overflow, false);
  }
}

void launch_patch(hipStream_t st, const PatchArgs& a, int max_blocks, const char** names, hipEvent_t* e0, hipEvent_t* e1) {
  const uint32_t gc = std::max<uint32_t>(1u, std::min<uint32_t>((a.n + 255u) / 256u, uint32_t(max_blocks)));
  const uint32_t gs = std::max<uint32_t>(1u, (a.nslots + 255u) / 256u);
  names[0] = "k_patch_classify";
  names[1] = "k_patch_sets<onesided>";
  names[2] = "k_patch_sets<clipped>";
  if (e0) hipEventRecord(e0[0], st);
  hipLaunchKernelGGL(k_patch_classify, dim3(gc), dim3(256), 0, st, a);
  if (e1) hipEventRecord(e1[0], st);
  if (e0) hipEventRecord(e0[1], st);
  hipLaunchKernelGGL(k_patch_sets<PATCH_ONESIDED>, dim3(gs), dim3(256), 0, st, a);
  if (e1) hipEventRecord(e1[1], st);
  if (e0) hipEventRecord(e0[2], st);
  hipLaunchKernelGGL(k_patch_sets<PATCH_CLIPPED>, dim3(gs), dim3(256), 0, st, a);
  if (e1) hipEventRecord(e1[2], st);
}
