// hfcl_k_redo.hip -- the last stage of an fp32 batch: the pairs whose fp32 run was inconsistent, solved again in fp64.
//
// The fp32 kernels check their own runs (hfcl_gjk.hpp: REDO_*; gjk_end<true>, gjk_finish<true>, Epa::loop_suspect, epa_depth_suspect,
// closed_form_suspect) and whoever writes the record of a marked pair appends it to IO<float>::redo_list (write_out, hfcl_dev.hpp).  This
// kernel walks that list -- its length is a device-side counter, the grid strides over it -- with one pair per BS_W-lane group, as
// k_triangle and the leaves of the mesh x solid walks do: the fp64 shape and vertex tables of the library, the fp32 poses promoted, the
// fp64 per-pair solver (GJK, EPA of the reference's capacity in LDS, the closed forms, the TriangleP rows), and the record rounded to the
// 44-byte form.  Built without contraction (FLAGS_k_redo), so a redone record is the fp64 entry points' record of the same pair, rounded.
// Every loop is bounded by what its callee names: a hull's vertices, gjk_max_iterations / epa_max_iterations.
#include "hfcl_dev.hpp"
#include "hfcl_launch.hpp"

using namespace hfcl;

namespace {

// support of one solid in its own frame, evaluated by the lane group (NoSweptSphere)
struct RedoSolid {
  DShape<double> s;
  HullRegs<double, BS_W> h;
  const double* v;
  int lig;
  __device__ __forceinline__ void set(const DShape<double>& shape, const double* verts, int lane_in_group) {
    s = shape;
    v = verts + 3 * size_t(s.vertex_offset);
    lig = lane_in_group;
    if (s.kind == K_CONVEX && s.num_points <= uint32_t(HULL_MAX)) h.load(v, s.num_points, lig);
  }
  __device__ __forceinline__ V3<double> operator()(const V3<double>& d) const {
    if (s.kind != K_CONVEX) return prim_support(s, d);
    if (s.num_points > uint32_t(HULL_MAX)) return scan_support<double, BS_W>(v, s.num_points, d, lig);
    return h.support(d, lig);
  }
};
// MinkowskiDiff::support (hfcl_pair.hpp: SerialSupport) over two of them
struct RedoPairSupport {
  RedoSolid a, b;
  MDiff<double> md;
  __device__ __forceinline__ void operator()(const V3<double>& dir, V3<double>& w, V3<double>& w0) const {
    w0 = a(dir);
    const V3<double> d1 = md.identity ? -dir : -tmul(md.oR1, dir);
    V3<double> s1 = b(d1);
    s1 = md.identity ? s1 : (mul(md.oR1, s1) + md.ot1);
    w = w0 - s1;
  }
};

struct RedoArgs {
  const uint32_t* list;
  const uint32_t* count;
  uint32_t n;  // pairs of the batch: an index beyond it is never followed
  const uint32_t* shape1;
  const uint32_t* shape2;
  const DShape<double>* shapes;
  const double* verts;
  const float* tf1;
  const float* tf2;
  hfcl_result_f32* out;
  QParams<double> q;
};

__global__ void __launch_bounds__(64) k_redo(RedoArgs a) {
  constexpr int G = 64 / BS_W;
  __shared__ EpaScratch<double, EPA_MAX_ITER> scratch[G];
  const uint32_t cnt = min(*a.count, a.n);
  const int lane = threadIdx.x & 63, grp = lane / BS_W, lig = lane & (BS_W - 1);
  for (uint32_t it = blockIdx.x * G + grp; it < cnt; it += gridDim.x * G) {
    const uint32_t pair = a.list[it];
    if (pair >= a.n) continue;  // (group-uniform)
    const DShape<double> s1 = a.shapes[a.shape1[pair]], s2 = a.shapes[a.shape2[pair]];
    const Pose<double> tf1 = pose_from_quat<double>(a.tf1 + 7 * size_t(pair)), tf2 = pose_from_quat<double>(a.tf2 + 7 * size_t(pair));
    // the solver's guess as the fp32 kernels take it (initial_guess, hfcl_dev.hpp: no per-pair guesses in the fp32 forms)
    const V3<double> guess0 = (a.q.guess_mode == HFCL_GUESS_CACHED || a.q.guess_mode == HFCL_GUESS_BOUNDING_VOLUME)
                                  ? mk<double>(a.q.guess[0], a.q.guess[1], a.q.guess[2])
                                  : mk<double>(1.0, 0.0, 0.0);
    PairOut<double> o;
    const bool t1 = s1.kind == K_TRIANGLE, t2 = s2.kind == K_TRIANGLE;
    if (pair_class(s1.kind, s2.kind) == CLS_CLOSED) {
      o.distance = closed_form_distance(s1, tf1, s2, tf2, a.verts, o.p1, o.p2, o.normal);
      o.gjk_status = GJK_DID_NOT_RUN;
      o.epa_status = EPA_DID_NOT_RUN;
      o.gjk_iters = o.epa_iters = 0;
    } else if (t1 || t2) {
      RedoSolid solid;  // the non-triangle shape (unused for TriangleP x TriangleP)
      solid.set(t1 ? s2 : s1, a.verts, lig);
      triangle_pair<double, LaneGroup<BS_W>>(s1, s2, a.verts, tf1, tf2, solid, a.q, guess0, &scratch[grp], o);
    } else {
      RedoPairSupport sup;
      sup.a.set(s1, a.verts, lig);
      sup.b.set(s2, a.verts, lig);
      sup.md = make_mdiff(tf1, tf2);
      const double r0 = swept_radius(s1), r1 = swept_radius(s2);
      Gjk<double, PW0<double>> g;
      gjk_run(g, a.q.gjk, start_guess(a.q, s1, s2, sup.md, guess0), r0 + r1, s1.kind == K_CONVEX && s2.kind == K_CONVEX, sup);
      EpaSeed<double> seed;
      if (gjk_finish(g, a.q, tf1, r0, r1, guess0, o, seed)) {
        LaneGroup<BS_W>::sync();
        epa_run<double, LaneGroup<BS_W>, EPA_MAX_ITER>(&scratch[grp], seed, a.q, tf1, r0, r1, sup, o);
        LaneGroup<BS_W>::sync();
      }
    }
    int nc;
    const bool contact = apply_query_semantics(a.q, o, nc);
    if (lig == 0) a.out[pair] = redo_record<hfcl_result_f32>(o, contact);
    LaneGroup<BS_W>::sync();
  }
}

}  // namespace

void launch_redo(int grid, hipStream_t st, const Work& wk, const DShape<double>* shapes64, const double* verts64, const IO<float>& io, const QParams<double>& q) {
  if (!io.redo_list || grid < 1) return;
  RedoArgs a;
  a.list = io.redo_list;
  a.count = io.redo_count;
  a.n = wk.n;
  a.shape1 = wk.shape1;
  a.shape2 = wk.shape2;
  a.shapes = shapes64;
  a.verts = verts64;
  a.tf1 = io.tf1;
  a.tf2 = io.tf2;
  a.out = io.out;
  a.q = q;
  hipLaunchKernelGGL(k_redo, dim3(grid), dim3(64), 0, st, a);
}
