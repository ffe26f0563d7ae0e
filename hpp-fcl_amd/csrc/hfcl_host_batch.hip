// hfcl_host_batch.hip -- host side, one device-resident batch: its workspace and table sets, the stream sets made on first use, and the
// dispatcher -- which kernels run, in which order, on which stream (run_batch -> run_batch_one: a short sequence of stages over one
// context, Batch<T>; every stage is a function that is GIVEN the stream it launches on).  The library object and what the host units share:
// hfcl_host.hpp; the entry points that call run_batch: hfcl_host.hip, hfcl_host_scene.hip; the kernels: hfcl_launch.hpp.
#include "hfcl_host.hpp"

// Device workspace of a batch of n pairs.  The bucket lists (4 B per pair and bucket the library's shape kinds can reach)
// are always needed; the EPA queues (two seeds of ~230 B per pair) and the hand-over area (one slot of ~4 KB per 8 pairs)
// only when the batch has a GJK bucket and asks for penetration data -- a closed-form or mesh-only library never pays
// for them.  ~0.05 KB per pair without EPA, ~1 KB with (it was 1.8 KB for every library).
static int ensure_workspace(hfcl_lib* lib, size_t n, bool need_epa) {
  if (n > lib->ws_capacity) {
    lib->ws_capacity = 0;
    const size_t cap = n + n / 8 + 1024;
    HIP_TRY(lib->d_lists.grow(size_t(B_COUNT) * cap));
    lib->ws_capacity = cap;
  }
  if (need_epa && lib->ws_capacity > lib->epa_capacity) {
    reset_all(lib->d_epa_queue, lib->d_epa_queue2, lib->d_epa_resume, lib->d_epa_cc_over);
    lib->resume_cap = 0;
    lib->epa_capacity = 0;
    const size_t cap = lib->ws_capacity;
    HIP_TRY(lib->d_epa_queue.grow(cap * sizeof(EpaItem<double>)));
    HIP_TRY(lib->d_epa_queue2.grow(cap * sizeof(EpaItem<double>)));
    // saved polytopes for the tier hand-over: room for an eighth of the batch (cfg5: 4 % of the pairs outgrow the fast
    // tier; beyond the area the full tier simply redoes the pair from its seed)
    size_t rcap = std::min(cap, std::max<size_t>(65536, cap / 8));
    if (lib->opt.epa_resume_slots) rcap = std::max<size_t>(1, std::min<size_t>(cap, lib->opt.epa_resume_slots));  // test knob (option epa_resume_slots)
    HIP_TRY(lib->d_epa_resume.grow(rcap * std::max(epa_resume_stride<double>, epa_resume_stride<float>)));
    HIP_TRY(lib->d_epa_cc_over.grow(rcap));
    lib->resume_cap = rcap;
    lib->epa_capacity = cap;
  }
  return HFCL_OK;
}

// Tables of a split traversal (mesh x mesh, mesh x solid) for a batch of n queries: room for `per_query` tasks per query (16: a long query
// suspends with a stack of ~20 entries, one query in five is long; mesh x solid walks are cut finer) -- ~2.4 KB of device memory per query
// in fp64.  cuts: the set has the tables of cut walks.
static int ensure_split(SplitTables& t, size_t n, size_t per_query, bool cuts) {
  if (n <= t.n) return HFCL_OK;
  reset_all(t.tasks, t.sums, t.susp, t.cut_words, t.cut_vals);
  t.n = 0;
  const size_t nq = n + n / 8 + 1024, cap = per_query * nq + 65536;
  HIP_TRY(t.tasks.grow(cap));
  HIP_TRY(t.sums.grow((nq + cap) * sizeof(BvhSum<double>)));
  if (cuts) {
    HIP_TRY(t.cut_words.grow(cap));
    HIP_TRY(t.cut_vals.grow(cap));
  }
  HIP_TRY(t.susp.grow(nq));
  HIP_TRY(t.ctr.grow(BVH_CTR_WORDS));
  t.n = nq;
  t.cap = cap;
  return HFCL_OK;
}
// the main set: tasks per query by option bvh_task_slots (test / tuning knob); the set beside keeps 16 whatever the option says
static int ensure_split_main(hfcl_lib* lib, size_t n) {
  return ensure_split(lib->split_main, n, lib->opt.bvh_task_slots ? std::max<size_t>(1, lib->opt.bvh_task_slots) : 16, true);
}

// Tables of a collide() walk in rounds: `lists` query lists, `order_per_query` entries of WalkTables::order per query, `ctr_words` counters
static int ensure_walk(WalkTables& t, size_t n, size_t lists, size_t order_per_query, size_t ctr_words) {
  if (n <= t.n) return HFCL_OK;
  reset_all(t.recs, t.items, t.res, t.lists, t.order);
  t.n = 0;
  const size_t nq = n + n / 8 + 1024;
  HIP_TRY(t.recs.grow(nq * sizeof(WalkRec<double>)));
  HIP_TRY(t.items.grow(nq * WALK_K));
  HIP_TRY(t.res.grow(nq * WALK_K * 10 * sizeof(double)));  // TriLeafOut<double>: distance, p1, p2, n
  HIP_TRY(t.lists.grow(lists * nq));
  HIP_TRY(t.order.grow(order_per_query * nq));
  HIP_TRY(t.ctr.grow(ctr_words));
  t.n = nq;
  return HFCL_OK;
}

// How the mesh x mesh traversals of this library keep their stacks.  A stack never holds more than depth1 + depth2 + 2
// entries (every step pops one entry and pushes at most two, one level deeper in one of the trees).
static int make_bvh_spill(hfcl_lib* lib, BvhSpill& sp, bool distance) {
  memset(&sp, 0, sizeof(sp));
  const size_t need = 2 * size_t(lib->bvh_max_depth) + 4;
  // collide(): a full LDS stack first suspends into tasks (HFCL_BVH_LEVELS levels of BVH_STACK entries); distance() has
  // no task form: anything deeper than its LDS stack takes the wide form with slabs
  const size_t narrow_holds = distance ? size_t(BVHD_STACK) : size_t(std::min(BVH_STACK, BVH_STACK_FILT)) * HFCL_BVH_LEVELS;
  sp.wide = (lib->bvh_max_nodes > 65535 || need > narrow_holds) ? 1u : 0u;
  if (lib->opt.bvh_force_wide) sp.wide = 1u;  // test knob (option bvh_force_wide): the wide form (and its slabs) on small models
  if (!sp.wide || need <= size_t(std::min(BVH_STACK, BVH_STACK_FILT)) / 2) return HFCL_OK;  // the LDS stack of the wide form suffices
  const size_t cap = ((need + 63) / 64) * 64;                     // entries per lane
  const size_t per_block = size_t(BVH_BLOCK) * cap * 2 * sizeof(uint64_t);  // (entry, bound) records: k_bvh_distance
  size_t blocks = std::min<size_t>(size_t(lib->n_cus) * 16, std::max<size_t>(1, (size_t(2) << 30) / per_block));
  const size_t bytes = blocks * per_block;
  HIP_TRY(lib->d_bvh_slab.grow(bytes));
  sp.slab = lib->d_bvh_slab;
  sp.cap = uint32_t(cap);
  sp.max_blocks = uint32_t(blocks);
  return HFCL_OK;
}

// the helper stream of a library (tail kernels beside the main ones) and its fork / join events, made on first use
static int ensure_aux(hfcl_lib* lib) {
  if (lib->aux) return HFCL_OK;
  // created into locals and committed together: a failure half way leaves the library without a helper stream, not with null events
  Stream s;
  Event ev[4];
  HIP_TRY(s.create());
  for (Event& e : ev) HIP_TRY(e.create());
  lib->ev_aux0 = std::move(ev[0]);
  lib->ev_aux1 = std::move(ev[1]);
  lib->ev_aux2 = std::move(ev[2]);
  lib->ev_aux3 = std::move(ev[3]);
  lib->aux = std::move(s);
  return HFCL_OK;
}
static int ensure_mesh_stream(hfcl_lib* lib) {
  if (lib->mesh_st) return HFCL_OK;  // (committed last)
  Stream st[3];
  Event ev[4];
  // option mesh_prio: [0] the mesh x solid walks and [2] their helper at the device's highest priority -- hardware queues of their own (the runtime
  // maps the streams of one priority onto four queues; two chains that share one run one after the other): cfgmix 2.90 -> 2.72 ms, but a process
  // that has created them runs cfg4s's in-line batches 1 ms slower (3.7 against 2.65 ms; profiles/r06_g).  Off.
  int prio_lo = 0, prio_hi = 0;
  if (lib->opt.mesh_prio) (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
  for (int k = 0; k < 3; ++k) HIP_TRY(st[k].create_with_priority(k == 1 ? 0 : prio_hi));
  for (Event& e : ev) HIP_TRY(e.create());
  lib->ev_mesh_fork = std::move(ev[0]);
  lib->ev_mesh_join = std::move(ev[1]);
  lib->ev_mesh_fork2 = std::move(ev[2]);
  lib->ev_mesh_join2 = std::move(ev[3]);
  lib->mesh_st2 = std::move(st[1]);
  lib->mesh_aux = std::move(st[2]);
  lib->mesh_st = std::move(st[0]);
  return HFCL_OK;
}
static int ensure_walk_streams(hfcl_lib* lib) {
  if (lib->walk_st[WALK_ROUNDS - 2]) return HFCL_OK;  // (committed last)
  Stream s[WALK_ROUNDS - 1];
  Event ev[2 * (WALK_ROUNDS - 1)];
  for (Stream& x : s) HIP_TRY(x.create());
  for (Event& e : ev) HIP_TRY(e.create());
  for (int k = 0; k < WALK_ROUNDS - 1; ++k) {
    lib->walk_fork[k] = std::move(ev[2 * k]);
    lib->walk_join[k] = std::move(ev[2 * k + 1]);
  }
  for (int k = 0; k < WALK_ROUNDS - 1; ++k) lib->walk_st[k] = std::move(s[k]);
  return HFCL_OK;
}
static int ensure_gjk_streams(hfcl_lib* lib) {
  if (lib->gjk_fork) return HFCL_OK;  // (committed last)
  Stream s[3];
  Event ev[4];
  for (Stream& x : s) HIP_TRY(x.create());
  for (Event& e : ev) HIP_TRY(e.create());
  for (int k = 0; k < 3; ++k) {
    lib->gjk_st[k] = std::move(s[k]);
    lib->gjk_join[k] = std::move(ev[k]);
  }
  lib->gjk_fork = std::move(ev[3]);
  return HFCL_OK;
}
// Lane-group width of the convex GJK kernels.  A/B on cfg3 / cfg5 (profiles/r01_k_gjk_lane_group_w2.txt): 2-lane
// groups (16 vertices of each hull per lane, 32 pairs per wave: half the redundancy of the serial simplex code)
// beat 4-lane groups wherever their 96 / 192 vertex registers fit -- everywhere but fp64 convex x convex.
template <typename T, int M>
static int auto_cvx_w() {
  return (sizeof(T) == 8 && M == 0) ? 4 : 2;
}
template <typename T, int M>
static void launch_cvx_m(hfcl_lib* lib, const Work& wk, const LibView<T>& lv, const IO<T>& io, const QParams<T>& q,
                         hipStream_t st, size_t n) {
  const int w = lib->opt.cvx_w ? lib->opt.cvx_w : auto_cvx_w<T, M>();
  note_form(lib, M == 0 ? "cvx_w_cc" : (M == 1 ? "cvx_w_pc" : "cvx_w_cp"), unsigned(w));
  const size_t nt = size_t(gjk_cvx_threads<T>(w, M));
  size_t b = (n + nt / w - 1) / (nt / w);
  if (b < 1) b = 1;
  // single-wave workgroups: one per round of pairs, handed out by the dispatcher as waves end (the kernel's grid-stride loop serves what is beyond 2^20 rounds)
  const size_t cap = nt == 64 ? size_t(1) << 20 : size_t(lib->n_cus) * 16;
  if (b > cap) b = cap;
  launch_gjk_cvx<T>(M, w, q.guess_mode == HFCL_GUESS_BOUNDING_VOLUME, int(b), st, wk, lv, io, q);
}

// ---------------------------------------------------------------------------------------
// One batch: the context of its stages.
// ---------------------------------------------------------------------------------------
template <typename T>
struct Batch {
  hfcl_lib* lib;
  // ONE object that the stages mutate in order, each launch taking the block as it stands then: the mesh section sets shape_defer* /
  // shape_oq BEFORE its split plan reads shape_defer_cap; the EPA section sets epa_ready* last
  Work wk;
  LibView<T> lv;
  IO<T> io;
  QParams<T> q;
  size_t n;
  size_t ti = 0;  // the next slot of lib->timers (Timed)
  int blocks_for(size_t items, size_t per_block) const {
    const size_t b = std::max<size_t>(1, (items + per_block - 1) / per_block);
    return int(std::min<size_t>(b, size_t(lib->n_cus) * 16));
  }
  // buckets no pair of this library's shape kinds can fall into are not launched at all
  bool may(int b) const { return (lib->possible_buckets >> b) & 1u; }
  bool any_gjk() const { return may(B_PRIM) || may(B_CC) || may(B_PC) || may(B_CP) || may(B_LARGE); }
  bool bvg() const { return q.guess_mode == HFCL_GUESS_BOUNDING_VOLUME; }
  T break_distance2() const { return T(lib->break_distance * lib->break_distance); }
};

// HIP events around what is launched in a scope (hfcl_last_kernel_breakdown), on the stream given: e0 where it is made, e1 where the scope
// ends -- on every way out of it.  Nothing when kernel_timing is off.  (The slot by index: a later slot may move the vector.)
struct Timed {
  hfcl_lib* lib = nullptr;
  size_t slot = 0;
  hipStream_t st;
  template <typename T>
  Timed(Batch<T>& b, const char* name, hipStream_t s) : st(s) {
    if (!b.lib->kernel_timing) return;
    lib = b.lib;
    slot = b.ti++;
    hipEventRecord(timer_slot(lib, slot, name)->e0, st);
  }
  ~Timed() {
    if (lib) hipEventRecord(lib->timers[slot].e1, st);
  }
  Timed(const Timed&) = delete;
};

// ---- stage: the parameter blocks of the batch (Work, LibView)
template <typename T>
static void make_views(Batch<T>& b, const uint32_t* d_s1, const uint32_t* d_s2) {
  hfcl_lib* lib = b.lib;
  constexpr bool F64 = std::is_same<T, double>::value;
  Work& wk = b.wk;  // (zeroed: shape_defer*, shape_oq, epa_ready* are the mesh and EPA sections' to set)
  wk.shape1 = d_s1;
  wk.shape2 = d_s2;
  wk.n = uint32_t(b.n);
  wk.lists = lib->d_lists;
  wk.counts = lib->d_counts;
  wk.epa_queue = lib->d_epa_queue;
  wk.epa_queue2 = lib->d_epa_queue2;
  wk.epa_resume = lib->d_epa_resume;
  wk.epa_v0 = lib->d_epa_v0;
  wk.resume_cap = uint32_t(std::min<size_t>(lib->resume_cap, 0xFFFFFFFFu));
  wk.epa_cc_over = lib->d_epa_cc_over;
  // fp32 slots are shorter than the area's stride (the fp64 slot): the slots past resume_cap are the convex x convex tier's own
  wk.cc_resume_base = wk.resume_cap;
  const size_t fslots = lib->resume_cap * std::max(epa_resume_stride<double>, epa_resume_stride<float>) / epa_resume_stride<float>;
  wk.cc_resume_cap = !F64 && fslots > lib->resume_cap ? uint32_t(std::min<size_t>(fslots - lib->resume_cap, lib->resume_cap)) : 0u;
  LibView<T>& lv = b.lv;
  lv.shapes = F64 ? (const DShape<T>*)lib->d_shapes64 : (const DShape<T>*)lib->d_shapes32;
  lv.verts = F64 ? (const T*)lib->d_verts64 : (const T*)lib->d_verts32;
  lv.kinds = lib->d_kinds;
  lv.n_shapes = uint32_t(lib->n_shapes);
  lv.graph_base = lib->d_graph_base;
  lv.graph_off = lib->d_graph_off;
  lv.graph_ent = F64 ? (const NbrEntry<T>*)lib->d_graph_ent64 : (const NbrEntry<T>*)lib->d_graph_ent32;
  lv.climb_min = lib->opt.climb_min;
  if (b.may(B_LARGE)) note_form(lib, "climb_min", lv.climb_min);
}
template <typename T>
static BvhView<T> make_bvh_view(const hfcl_lib* lib) {
  constexpr bool F64 = std::is_same<T, double>::value;
  BvhView<T> bv;
  bv.nodes = F64 ? (const DNode<T>*)lib->d_nodes64.get() : (const DNode<T>*)lib->d_nodes32.get();
  bv.fnodes = (F64 && lib->opt.bvh_filter) ? lib->d_fnodes.get() : nullptr;
  bv.rss = F64 ? (const DRss<T>*)lib->d_rss64.get() : (const DRss<T>*)lib->d_rss32.get();
  bv.dnodes = F64 ? (const DNodeD<T>*)lib->d_dnodes64.get() : (const DNodeD<T>*)lib->d_dnodes32.get();
  bv.verts = F64 ? (const T*)lib->d_bverts64.get() : (const T*)lib->d_bverts32.get();
  bv.tris = lib->d_btris;
  bv.meshes = lib->d_meshes;
  bv.n_meshes = uint32_t(lib->h_meshes.size());
  return bv;
}

// one of the solids' kernels, timed, on the stream next_stream() gives it (called in front of every kernel: a small batch's fan out)
template <typename T, class Next, class Launch>
static void on_next(Batch<T>& b, const char* name, Next& next_stream, Launch&& launch) {
  hipStream_t const s = next_stream();
  Timed t(b, name, s);
  launch(s);
}

// ---- stage: the solids' kernels of the batch (closed forms, GJK; their EPA is a stage of its own, behind the mesh walks: a mesh x solid leaf
// can queue for it).  All in `caller`'s order when the stage returns.
template <typename T>
static int launch_solids(Batch<T>& b, hipStream_t caller) {
  hfcl_lib* lib = b.lib;
  const size_t n = b.n;
  // A small batch (option gjk_beside_max) of a library without meshes: its buckets' kernels -- independent of each other, each a chain of
  // GJK trips on a chip it does not fill -- fan out over the caller's stream and three helpers, joined in front of the EPA section
  // (cfg5 at 20 000 pairs: four GJK kernels of 40-116 us in a row).
  // From three iterative kernels on: a fork and a join cost ~0.08 ms themselves (cfg2, closed forms + one GJK kernel: 0.10 -> 0.20 ms with them).
  int kernels = 0;
  for (int k : {int(B_PRIM), int(B_CC), int(B_PC), int(B_CP), int(B_LARGE), int(B_TRI)}) kernels += b.may(k) ? 1 : 0;
  bool fan = lib->opt.gjk_beside_max && n <= lib->opt.gjk_beside_max && lib->h_meshes.empty() && kernels >= 3;
  if (fan && ensure_gjk_streams(lib) != HFCL_OK) fan = false;
  note_form(lib, "gjk_fan", fan);
  if (b.may(B_CLOSED)) note_form(lib, "closed_staged", lib->opt.closed_staged);
  int fan_i = 0;
  uint32_t used = 0;
  if (fan) HIP_TRY(hipEventRecord(lib->gjk_fork, caller));
  auto next_stream = [&]() -> hipStream_t {
    if (!fan) return caller;
    const int k = fan_i;
    fan_i = (fan_i + 1) % 4;
    if (k && !(used & (1u << (k - 1)))) {
      used |= 1u << (k - 1);
      (void)hipStreamWaitEvent(lib->gjk_st[k - 1], lib->gjk_fork, 0);
    }
    return k ? lib->gjk_st[k - 1].get() : caller;
  };
  if (b.may(B_CLOSED)) on_next(b, "k_closed", next_stream, [&](hipStream_t s) { launch_closed<T>(b.blocks_for(n, 256), s, b.wk, b.lv, b.io, b.q, lib->opt.closed_staged); });
  if (b.may(B_PRIM)) on_next(b, "k_gjk_prim", next_stream, [&](hipStream_t s) { launch_gjk_prim<T>(b.blocks_for(n, 256), s, b.wk, b.lv, b.io, b.q, b.bvg()); });
  if (b.may(B_CC)) on_next(b, "k_gjk_cvx<cc>", next_stream, [&](hipStream_t s) { launch_cvx_m<T, 0>(lib, b.wk, b.lv, b.io, b.q, s, n); });
  if (b.may(B_PC)) on_next(b, "k_gjk_cvx<pc>", next_stream, [&](hipStream_t s) { launch_cvx_m<T, 1>(lib, b.wk, b.lv, b.io, b.q, s, n); });
  if (b.may(B_CP)) on_next(b, "k_gjk_cvx<cp>", next_stream, [&](hipStream_t s) { launch_cvx_m<T, 2>(lib, b.wk, b.lv, b.io, b.q, s, n); });
  if (b.may(B_LARGE)) on_next(b, "k_gjk_large", next_stream, [&](hipStream_t s) { launch_gjk_large<T>(b.blocks_for(n, 256 / LARGE_W), s, b.wk, b.lv, b.io, b.q, b.bvg()); });
  if (b.may(B_TRI)) on_next(b, "k_triangle", next_stream, [&](hipStream_t s) { launch_triangle<T>(b.blocks_for(n / 8 + 1, 64 / BS_W), s, b.wk, b.lv, b.io, b.q); });
  for (int k = 0; k < 3; ++k)
    if (used & (1u << k)) {
      HIP_TRY(hipEventRecord(lib->gjk_join[k], lib->gjk_st[k]));
      HIP_TRY(hipStreamWaitEvent(caller, lib->gjk_join[k], 0));
    }
  return HFCL_OK;
}

static void fill_walk(WalkArgs& a, const WalkTables& w) {
  a.recs = w.recs;
  a.items = w.items;
  a.res = w.res;
  a.ctr = w.ctr;
  a.list_in = a.list_out = w.lists;
  a.item_cap = uint32_t(std::min<size_t>(w.n * WALK_K, 0xFFFFFFFFu));
  a.list_stride = uint32_t(w.n);
}
// ---- stage: the split plan of a collide() walk on the table set `tabs`, its counters zeroed on `st`.  Long traversals are cut into tasks
// when the batch is large enough for the tail to matter (`want`) and the request keeps no query-wide contact count (mesh x mesh and the
// one-query-per-lane form of mesh x solid alike).  Reads wk.shape_defer_cap: the mesh section has sized the EPA queue by then.
template <typename T>
static int plan_split(Batch<T>& b, hipStream_t st, BvhSplit& split, bool want, bool solid, SplitTables& tabs) {
  hfcl_lib* lib = b.lib;
  const hfcl_options& o = lib->opt;
  const size_t n = b.n;
  memset(&split, 0, sizeof(split));
  split.leaf_cost = o.shape_leaf_cost;
  if (!(want && (solid ? o.shape_levels : o.bvh_levels) > 1 && lib->bvh_params.num_max_contacts == 1 && !lib->bvh_params.contacts)) {
    note_form(lib, solid ? "ms_split" : "mm_split", 0);
    return HFCL_OK;
  }
  const bool main_set = &tabs == &lib->split_main;
  int r = main_set ? ensure_split_main(lib, n) : ensure_split(tabs, n, 16, false);
  if (r) return r;
  HIP_TRY(hipMemsetAsync(tabs.ctr, 0, BVH_CTR_WORDS * sizeof(uint32_t), st));
  split.tasks = tabs.tasks;
  split.sums = tabs.sums;
  split.suspended = tabs.susp;
  split.ctr = tabs.ctr;
  split.cap = uint32_t(std::min<size_t>(tabs.cap, 0x7FFFFFFFu));
  split.n_queries = uint32_t(tabs.n);
  split.budget = o.bvh_budget;
  split.budget0 = o.bvh_budget0;
  split.n_levels = o.bvh_levels;
  if (o.bvh_auto && 2 * n <= 3 * size_t(lib->n_cus) * 512) {  // (8 waves of 64 lanes per CU are resident)
    split.budget0 = 512;
    split.budget = 16;
    split.n_levels = BVH_MAX_LEVELS;
  }
  split.coop_grid = uint32_t(lib->n_cus) * 8u;
  split.cut_ticks = solid ? o.shape_cut_ticks : (main_set ? o.bvh_cut_ticks : 0u);  // (the set beside has no chunk tables)
  split.cut_cap = split.cap;
  // (mesh x solid: the EPA queue has room for one item per query and per chunk -- shape_defer_cap entries, sized before the walk)
  split.cut_task_cap = solid ? (b.wk.shape_defer_cap > n ? uint32_t(std::min<size_t>(b.wk.shape_defer_cap - n, split.cap)) : 0u) : split.cap;
  split.cut_words = lib->split_main.cut_words;  // (the main set's whichever set walks: never cut, the set beside never reads them)
  split.cut_vals = lib->split_main.cut_vals;
  if (!solid && o.bvh_coop) {
    split.coop = 1u;
    const bool one_round = o.walk_auto && n <= 220000;
    const uint32_t rounds = o.walk_auto ? (one_round ? 1u : 2u) : o.walk_rounds;
    split.budget0 = o.bvh_budget0_coop ? o.bvh_budget0_coop
                                       : (n > 500000 ? 640u : (one_round ? (n > 120000 ? 320u : 256u) : (rounds ? (n > 150000 ? std::max(320u, o.walk_budget[0]) : o.walk_budget[0]) : 256u)));
    // the queries' own phase as walk / leaves / resolve rounds (narrow node ids; rec indices travel in 28 bits)
    if (rounds && n < (size_t(1) << 28)) {
      WalkTables& w = lib->walk_mm;  // (ONE set: also of the walks that run beside on `split_beside`, never together with the main set's)
      r = ensure_walk(w, n, 2, 1, 8 * WALK_ROUNDS);
      if (r) return r;
      HIP_TRY(hipMemsetAsync(w.ctr, 0, 8 * WALK_ROUNDS * sizeof(uint32_t), st));
      fill_walk(split.walk, w);
      split.order = o.walk_order ? w.order.get() : nullptr;
      split.walk_rounds = std::min<uint32_t>(rounds, WALK_ROUNDS);
      for (int k = 0; k < WALK_ROUNDS; ++k) {
        split.walk_k[k] = (one_round && k == 0) ? uint32_t(WALK_K) : o.walk_k[k];
        split.walk_budget[k] = k == 0 ? split.budget0 : o.walk_budget[k];
      }
    }
  }
  if (solid) {
    split.coop = o.shape_coop ? 1u : 0u;
    split.budget0 = o.shape_coop ? o.shape_budget0_coop : o.shape_budget0;
    split.budget = o.shape_budget;
    split.n_levels = o.shape_levels;
    // the queries' own phase as walk / leaves / resolve (one round; what is left of a walk is k_bvh_shape_coop's)
    if (split.coop && o.shape_walk && n >= o.shape_walk_min && n < (size_t(1) << 28)) {
      WalkTables& w = lib->walk_ms;
      r = ensure_walk(w, n, 3, WALK_K + 1, 8 * WALK_ROUNDS + 64);
      if (r) return r;
      HIP_TRY(hipMemsetAsync(w.ctr, 0, (8 * WALK_ROUNDS + 64) * sizeof(uint32_t), st));
      split.walk.hist = w.ctr + 8 * WALK_ROUNDS;
      split.walk.perm = o.shape_walk_sort ? w.order.get() : nullptr;
      fill_walk(split.walk, w);
      split.walk.redo = w.lists + 2 * w.n;
      split.walk_rounds = 1u;
      split.walk_k[0] = uint32_t(WALK_K);
      split.walk_budget[0] = o.shape_walk_budget;
    }
  }
  // (the plan as the kernels get it)
  const char* const names[2][12] = {{"mm_coop", "mm_budget0", "mm_budget", "mm_levels", "mm_cap", "mm_cut_ticks", "mm_rounds", "mm_order", "mm_walk_k", "mm_walk_budget", "mm_leaf_cost", "mm_perm"},
                                    {"ms_coop", "ms_budget0", "ms_budget", "ms_levels", "ms_cap", "ms_cut_ticks", "ms_rounds", "ms_order", "ms_walk_k", "ms_walk_budget", "ms_leaf_cost", "ms_perm"}};
  const char* const* nm = names[solid ? 1 : 0];
  note_form(lib, nm[0], split.coop);
  note_form(lib, nm[1], split.budget0);
  note_form(lib, nm[2], split.budget);
  note_form(lib, nm[3], split.n_levels);
  note_form(lib, nm[4], split.cap);
  note_form(lib, nm[5], split.cut_ticks);
  note_form(lib, nm[6], split.walk.recs ? split.walk_rounds : 0u);
  note_form(lib, nm[7], split.order != nullptr);
  for (int k = 0; k < WALK_ROUNDS && split.walk.recs; ++k) {
    note_form(lib, nm[8], split.walk_k[k]);
    note_form(lib, nm[9], split.walk_budget[k]);
  }
  note_form(lib, nm[10], split.leaf_cost);
  note_form(lib, nm[11], split.walk.perm != nullptr);
  return HFCL_OK;
}

// ---- stage: mesh x mesh collide() on `st`, its split tables `tabs`
template <typename T>
static int mesh_mesh_collide(Batch<T>& b, hipStream_t st, const BvhView<T>& bv, const BvhSpill& spill, SplitTables& tabs) {
  hfcl_lib* lib = b.lib;
  const size_t n = b.n;
  Timed t(b, "k_bvh_collide", st);
  BvhSplit split;
  int rc = plan_split(b, st, split, b.may(B_BVH) && !spill.wide && (n >= 256 || 2 * size_t(lib->bvh_max_depth) + 4 > size_t(std::min(BVH_STACK, BVH_STACK_FILT))), false, tabs);
  if (rc) return rc;
  AsideStream beside[WALK_ROUNDS - 1] = {};
  const bool early = split.walk.recs && split.walk_rounds > 1 && lib->opt.walk_early_coop;
  note_form(lib, "mm_early_coop", early);
  if (early) {
    rc = ensure_walk_streams(lib);
    if (rc) return rc;
    for (int k = 0; k < WALK_ROUNDS - 1; ++k) beside[k] = AsideStream{lib->walk_st[k], lib->walk_fork[k], lib->walk_join[k]};
  }
  launch_bvh_collide<T>(b.blocks_for(n, BVH_BLOCK), st, b.wk, b.lv, bv, b.io, b.q, lib->bvh_params, b.break_distance2(), split, spill, early ? beside : nullptr);
  return HFCL_OK;
}

// ---- stage: mesh x solid collide() on `st`.  lane: one query per lane (k_bvh_collide's SOLID form); otherwise the 16-lane group kernel.
// own_stream: the mesh section runs beside the solids' kernels, whose EPA section has `aux`
template <typename T>
static int mesh_solid_collide(Batch<T>& b, hipStream_t st, const BvhView<T>& bv, const BvhSpill& spill, bool lane, bool own_stream) {
  hfcl_lib* lib = b.lib;
  const size_t n = b.n;
  Timed t(b, "k_bvh_shape", st);
  note_form(lib, "ms_lane", lane);
  if (!lane) {
    launch_bvh_shape<T>(b.blocks_for(n / 8 + 1, 64 / BS_W), st, b.wk, b.lv, bv, b.io, b.q, lib->bvh_params, b.break_distance2());
    return HFCL_OK;
  }
  // tasks re-start the leaf solver from the request's guess: a walk whose leaves hand the cached guess on, or whose
  // final guess is read, stays in one piece
  BvhSplit split;
  int rc = plan_split(b, st, split, n >= 256 && b.q.guess_mode != HFCL_GUESS_CACHED && !b.io.gout, true, lib->split_main);
  if (rc) return rc;
  AsideStream aside = {nullptr, nullptr, nullptr};
  if (lib->opt.shape_finish_aside && b.wk.shape_finish_over && split.tasks && split.coop && split.cut_ticks) {
    rc = ensure_aux(lib);
    if (rc) return rc;
    aside = AsideStream{own_stream ? lib->mesh_aux : lib->aux, lib->ev_aux2, lib->ev_aux3};  // (`aux` is the solids' EPA section's, beside)
  }
  note_form(lib, "ms_finish_aside", aside.stream != nullptr);
  note_form(lib, "ms_finish_tiers", b.wk.shape_finish_over != nullptr);
  launch_bvh_shape_fast<T>(b.blocks_for(n, BVH_BLOCK), b.blocks_for(n / 8 + 1, 64 / BS_W), int(std::min<size_t>(n / 4 + 1, size_t(lib->n_cus) * 8)), st, b.wk, b.lv, bv, b.io, b.q,
                           lib->bvh_params, b.break_distance2(), split, spill, aside.stream ? &aside : nullptr);
  return HFCL_OK;
}

// what the two distance() walks hand to their continuation kernels: the suspended records, their counters in the batch's counter block, the pool's knobs
static void fill_continuation(BvhSpill& sp, hfcl_lib* lib, void* susp, int ctr_susp, int ctr_rerun, int ctr_ticket, uint32_t budget, uint32_t pool,
                              uint32_t leaf_min, uint32_t starve) {
  sp.susp = susp;
  sp.rerun_count = lib->opt.pool_rerun ? lib->d_counts + ctr_rerun : nullptr;
  sp.rerun_all = lib->opt.pool_rerun >= 2 ? 1u : 0u;
  sp.susp_count = lib->d_counts + ctr_susp;
  sp.budget = budget;
  sp.max_blocks = uint32_t(lib->n_cus) * 8u;
  sp.pool = pool;
  sp.pool_ticket = lib->d_counts + ctr_ticket;
  sp.pool_leaf_min = leaf_min;
  sp.pool_starve = starve;
  const bool solid = ctr_susp == CTR_SHAPE_DIST_SUSP;
  note_form(lib, solid ? "msd_budget" : "mmd_budget", budget);
  note_form(lib, solid ? "msd_pool" : "mmd_pool", pool);
  note_form(lib, solid ? "msd_leaf_min" : "mmd_leaf_min", leaf_min);
  note_form(lib, solid ? "msd_starve" : "mmd_starve", starve);
  note_form(lib, solid ? "msd_rerun" : "mmd_rerun", lib->opt.pool_rerun);
}
// ---- stage: the two distance() walks on `st`: mesh x solid (lane: one query per lane), then mesh x mesh
template <typename T>
static int mesh_distance(Batch<T>& b, hipStream_t st, const BvhView<T>& bv, BvhSpill spill, bool lane) {
  hfcl_lib* lib = b.lib;
  const hfcl_options& o = lib->opt;
  const size_t n = b.n;
  {
    Timed t(b, "k_bvh_shape_distance", st);
    note_form(lib, "msd_lane", lane);
    if (lane) {
      // long walks are handed to waves -- unless their leaves hand a cached guess on, or the final guess is read
      BvhSpill ss;
      memset(&ss, 0, sizeof(ss));
      if (o.shape_dist_budget && b.q.guess_mode != HFCL_GUESS_CACHED && !b.io.gout) {
        HIP_TRY(lib->d_shape_dist_susp.grow(lib->ws_capacity * sizeof(ShapeDistSusp<double>)));
        fill_continuation(ss, lib, lib->d_shape_dist_susp, CTR_SHAPE_DIST_SUSP, CTR_SHAPE_DIST_RERUN, CTR_SHAPE_DIST_TICKET, o.shape_dist_budget,
                          lib->has_flats ? 0u : o.shape_dist_pool, o.shape_dist_leaf_min, o.shape_dist_starve);
      }
      launch_bvh_shape_distance_fast<T>(b.blocks_for(n, BVHD_BLOCK), b.blocks_for(n / 8 + 1, 64 / BS_W), st, b.wk, b.lv, bv, b.io, b.q, ss);
    } else {
      launch_bvh_shape_distance<T>(b.blocks_for(n / 8 + 1, 64 / BS_W), st, b.wk, b.lv, bv, b.io, b.q);
    }
  }
  Timed t(b, "k_bvh_distance", st);
  if (b.may(B_BVH) && !spill.wide && o.bvhd_budget) {
    HIP_TRY(lib->d_dist_susp.grow(lib->ws_capacity * sizeof(DistSusp<double>)));
    // (15-bit node ids in the pool's entry word: POOL_MAX_NODES)
    fill_continuation(spill, lib, lib->d_dist_susp, CTR_DIST_SUSP, CTR_DIST_RERUN, CTR_DIST_TICKET, o.bvhd_budget, lib->bvh_max_nodes > 32767 ? 0u : o.bvhd_pool,
                      o.bvhd_pool_leaf_min, o.bvhd_pool_starve);
    spill.pool_part_min = o.bvhd_pool_part_min;
    note_form(lib, "mmd_part_min", spill.pool_part_min);
  }
  launch_bvh_distance<T>(b.blocks_for(n, BVHD_BLOCK), st, b.wk, b.lv, bv, b.io, b.q, spill);
  return HFCL_OK;
}

// The EPA queue of the one-query-per-lane mesh x solid forms and the solids' boxes, into b.wk (before any split plan of the batch).
// One EPA item per unit at most (a contact ends the unit): a query, or -- when suspended walks are cut into task levels instead of being
// continued by a wave (HFCL_SHAPE_COOP=0) -- every task of the split's table as well
template <typename T>
static int size_shape_defer(Batch<T>& b, bool collide_lane) {
  hfcl_lib* lib = b.lib;
  const size_t n = b.n;
  size_t need = lib->ws_capacity;
  // (the chunks of a cut walk are units too, and every unit can queue one item: room for four chunks per query -- 336 B each --; a walk
  // whose chunks would not fit is not cut, BvhSplit::cut_task_cap.  cfg4s makes ~0.6 chunks per query; n / 2 was too tight: cuts refused,
  // 3.5 -> 4.4 ms)
  if (collide_lane && lib->opt.shape_coop && lib->opt.shape_cut_ticks) need = std::max(need, n + 4 * n + 4096);
  if (collide_lane && !lib->opt.shape_coop && n >= 256) {
    const int rc = ensure_split_main(lib, n);
    if (rc) return rc;
    need = std::max(need, n + lib->split_main.cap);
  }
  constexpr size_t DEFER_ITEM = sizeof(ShapeDeferItem<double>) + 2 * sizeof(uint32_t);  // (+ the two lists of k_bvh_shape_finish's second tier)
  HIP_TRY(lib->d_shape_defer.grow(need * DEFER_ITEM));
  const size_t defer_cap = lib->d_shape_defer.capacity() / DEFER_ITEM;
  // (the solids' boxes are indexed by pair: one per pair of the workspace, not one per EPA item -- 1M pairs: 0.14 GB instead of 0.7)
  HIP_TRY(lib->d_shape_oq.grow(lib->ws_capacity * std::max(sizeof(ObbQuery<double>), sizeof(RssQuery<double>))));
  b.wk.shape_defer = lib->d_shape_defer;
  b.wk.shape_defer_cap = uint32_t(std::min<size_t>(defer_cap, 0xFFFFFFFFu));
  b.wk.shape_finish_over = lib->opt.shape_finish_tiers ? reinterpret_cast<uint32_t*>(static_cast<char*>(lib->d_shape_defer.get()) + defer_cap * sizeof(ShapeDeferItem<double>)) : nullptr;
  b.wk.shape_oq = lib->d_shape_oq;
  return HFCL_OK;
}

// ---- stage: the mesh walks of the batch, on `st` (own_stream: a stream of their own, beside the solids' kernels)
template <typename T>
static int launch_meshes(Batch<T>& b, hipStream_t st, bool own_stream) {
  hfcl_lib* lib = b.lib;
  const hfcl_options& o = lib->opt;
  if (lib->h_meshes.empty() || !(b.may(B_BVH) || b.may(B_BVHSHAPE))) return HFCL_OK;
  // every BVH shape must name a registered model: checked on the host, the kernels index the mesh table with it (helpers never run mesh batches)
  for (const hfcl_shape& sh : lib->h_shapes)
    if (sh.type == HFCL_BV_OBBRSS && (sh.bvh_index < 0 || size_t(sh.bvh_index) >= lib->h_meshes.size())) {
      set_error("BVH shape with bvh_index " + std::to_string(sh.bvh_index) + " but only " + std::to_string(lib->h_meshes.size()) +
                " BVHModel(s) registered (hfcl_lib_add_bvh)");
      return HFCL_ERR_INVALID_ARGUMENT;
    }
  int rc = upload_bvh(lib);
  if (rc) return rc;
  const BvhView<T> bv = make_bvh_view<T>(lib);
  const bool collide = b.q.mode == 1;
  BvhSpill spill;
  rc = make_bvh_spill(lib, spill, !collide);
  if (rc) return rc;
  // mesh x solid: one query per lane (k_bvh_collide's SOLID form) where the request lets a leaf that needs EPA end the
  // walk (hfcl_bvh_shape.hpp: mesh_shape_lane_request) and the lanes' stacks hold the models; the 16-lane group kernel
  // otherwise.  distance(): a leaf that needs EPA always ends the walk; models deeper than the lanes' stacks take the group kernel
  const bool lane = b.may(B_BVHSHAPE) && o.bvh_shape_lane &&
                    (collide ? size_t(lib->bvh_max_depth) + 1 <= size_t(BVH_STACK) && mesh_shape_lane_request(b.q, lib->bvh_params.num_max_contacts)
                             : size_t(lib->bvh_max_depth) + 1 <= size_t(BVHD_STACK));
  note_form(lib, "bvh_wide", spill.wide);
  note_form(lib, "bvh_filter", bv.fnodes != nullptr);
  if (lane) {
    rc = size_shape_defer(b, collide);
    if (rc) return rc;
  }
  if (!collide) return mesh_distance(b, st, bv, spill, lane);
  // Both kinds of mesh pairs in the batch's library, and the mesh walks on streams of their own: the mesh x mesh walks (tables of
  // their own) on a second one, beside the mesh x solid walks -- the two share nothing else, and each is a chain that leaves the chip
  // half empty (cfgmix: 1.45 ms of mesh x mesh behind 2.3 ms of mesh x solid)
  const bool mm_beside = own_stream && o.mesh_beside >= 2 && b.may(B_BVH) && b.may(B_BVHSHAPE) && !spill.wide && !o.bvh_cut_ticks && o.bvh_coop && (o.walk_auto || o.walk_rounds != 0);
  note_form(lib, "mm_beside", mm_beside);
  if (mm_beside) {
    HIP_TRY(hipEventRecord(lib->ev_mesh_fork2, st));
    HIP_TRY(hipStreamWaitEvent(lib->mesh_st2, lib->ev_mesh_fork2, 0));
    rc = mesh_mesh_collide(b, lib->mesh_st2, bv, spill, lib->split_beside);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(lib->ev_mesh_join2, lib->mesh_st2));
  }
  rc = mesh_solid_collide(b, st, bv, spill, lane, own_stream);
  if (rc) return rc;
  if (mm_beside) HIP_TRY(hipStreamWaitEvent(st, lib->ev_mesh_join2, 0));
  else rc = mesh_mesh_collide(b, st, bv, spill, lib->split_main);
  return rc;
}

// A library with meshes AND solids: the mesh walks on a stream of their own BESIDE the solids' kernels -- the walks are chains of dependent
// steps that leave the chip half empty (section 3 item 6f), and every kernel of a bucket the library COULD fill is launched whether or not
// this batch fills it (a mesh-only batch of a mixed library used to wait for ~0.08 ms of empty GJK launches in front of its walks).
template <typename T>
static bool meshes_run_beside(const Batch<T>& b) {
  hfcl_lib* lib = b.lib;
  const bool any_mesh = !lib->h_meshes.empty() && (b.may(B_BVH) || b.may(B_BVHSHAPE));
  const bool any_solid = b.may(B_CLOSED) || b.any_gjk() || b.may(B_TRI);
  bool beside = any_mesh && any_solid && lib->opt.mesh_beside;
  // ... when the batch holds both: a batch of mesh pairs alone pays for the solids' empty launches when they stand BESIDE its walks (grids sized
  // for the batch, every block waiting for a wave slot of a full chip: cfg4s 2.67 -> 2.80 ms) and nothing when they stand in front of them
  // (4 us each on an empty chip).  The witness is the library's batch before this one (its bucket counts, read without waiting for them:
  // they only choose between two orders of the same launches); the first batch runs beside.
  if (beside && lib->opt.mesh_beside < 4 && lib->ran_batch && lib->h_counts) {
    uint32_t solids_before = 0, meshes_before = one_count(lib->h_counts, int(B_BVH)) + one_count(lib->h_counts, int(B_BVHSHAPE));
    for (int k : {int(B_CLOSED), int(B_PRIM), int(B_CC), int(B_PC), int(B_CP), int(B_LARGE), int(B_TRI)}) solids_before += one_count(lib->h_counts, k);
    if (!solids_before || !meshes_before) beside = false;
  }
  if (beside && ensure_mesh_stream(lib) != HFCL_OK) beside = false;  // (no helper stream: one after the other, as before)
  return beside;
}

// ---- stage: EPA on `st`.  Fast tiers in three stages (hfcl_k_epa.hip) for batches large enough to pay for the extra launches: one lane per
// polytope prepares it (encloseOrigin, first tetrahedron) and writes its record; the loop kernels between them do nothing but expand.
//   fp32 convex x convex (the top queue): k_epa_prepare / k_epa_loop / k_epa_records, k_epa_resume_cc for the polytopes that outgrow the block
//   every other queue, both precisions:    k_epa_prepare_general / k_epa_loop_general / k_epa_records_general, the full-capacity tier behind them
// Otherwise the one-kernel forms (launch_epa_fast: fp32 streams, fp64 lockstep kernels).
template <typename T>
static int launch_epa(Batch<T>& b, hipStream_t st) {
  hfcl_lib* lib = b.lib;
  const hfcl_options& o = lib->opt;
  const size_t n = b.n;
  Work& wk = b.wk;
  constexpr bool F32 = std::is_same<T, float>::value;
  const bool general_q = b.may(B_PRIM) || b.may(B_PC) || b.may(B_CP) || (!F32 && b.may(B_CC));
  // A very small batch: the full-capacity tier alone, over every seed (k_epa_requeue) -- the batch is as long as its longest polytope either way, and
  // the fast tier in front of the full one is a second such chain (cfg5's mix at 2 000 pairs: 0.18 + 0.22 ms)
  // (fp64 only: its tiers are compiled without contraction and agree bit for bit; the fp32 tiers are different instantiations of contracted code)
  const bool direct = sizeof(T) == 8 && o.epa_direct_max && n <= o.epa_direct_max;
  const bool cc_staged = F32 && !direct && b.may(B_CC) && o.epa_cc_staged && n >= o.epa_cc_staged_min;
  const bool gen_staged = !direct && general_q && o.epa_general_staged && n >= o.epa_general_staged_min;
  note_form(lib, "epa_direct", direct);
  note_form(lib, "epa_cc_staged", cc_staged);
  note_form(lib, "epa_gen_staged", gen_staged);
  note_form(lib, "epa_resume_cap", wk.resume_cap);
  if (cc_staged) {
    note_form(lib, "epa_pool_share", o.epa_pool_share);
    note_form(lib, "epa_pool_min_refills", o.epa_pool_min_refills);
    note_form(lib, "epa_records_aside", o.records_aside);
    HIP_TRY(lib->d_epa_ready.grow(lib->ws_capacity * sizeof(EpaReady<float>)));
    wk.epa_ready = lib->d_epa_ready;
  }
  if (gen_staged) {
    HIP_TRY(lib->d_epa_ready_g.grow(lib->ws_capacity * sizeof(EpaReadyG<T>)));
    wk.epa_ready_g = lib->d_epa_ready_g;
  }
  if constexpr (F32) {
    if (cc_staged) {
      Timed t(b, "k_epa_prepare", st);
      launch_epa_prepare(b.blocks_for(n / 4 + 1, 256), st, wk, b.lv, b.io, b.q);
    }
  }
  if (gen_staged) {
    Timed t(b, "k_epa_prepare_general", st);
    launch_epa_prepare_general<T>(b.blocks_for(n / 4 + 1, 256), st, wk, b.lv, b.io, b.q, F32);
  }
  if (direct) {
    Timed t(b, "k_epa<full>", st);
    launch_epa_requeue<T>(st, wk);
    // (the grid: a lane group per seed, up to what k_epa's shape-0 support point area holds -- n_cus * 16 blocks)
    launch_epa_full<T>(int(std::min<size_t>(b.blocks_for(n / 2 + 1, 64 / epa_we2<T>), size_t(lib->n_cus) * 16)), st, wk, b.lv, b.io, b.q);
    return HFCL_OK;
  }
  const int epa_batches = int(std::min<size_t>((n + 64 / EPA_WE - 1) / (64 / EPA_WE), size_t(1) << 22));
  {
    Timed t(b, "k_epa<fast>", st);
    // fp64 with both classes of pairs: their fast-tier kernels on two streams (each one's tail under the other's body)
    hipStream_t st2 = nullptr;
    if constexpr (!F32) {
      if (o.epa64_two_streams && lib->has_curved && general_q) {
        if (int rc = ensure_aux(lib)) return rc;
        st2 = lib->aux;
        note_form(lib, "epa64_two_streams", 1);
        HIP_TRY(hipEventRecord(lib->ev_aux0, st));
        HIP_TRY(hipStreamWaitEvent(st2, lib->ev_aux0, 0));
      }
    }
    // (the launchers size the grids of the persistent forms themselves: here only the number of wave-sized batches)
    if constexpr (F32)
      if (cc_staged) launch_epa_loop(epa_batches, st, wk, b.lv, b.q, lib->n_cus, o.epa_pool_share, o.epa_pool_min_refills);
    if (gen_staged) launch_epa_loop_general<T>(epa_batches, st, st2, wk, b.lv, b.q, lib->n_cus, lib->has_curved);
    if ((F32 && b.may(B_CC) && !cc_staged) || (general_q && !gen_staged))
      launch_epa_fast<T>(epa_batches, st, wk, b.lv, b.io, b.q, b.may(B_CC) && !cc_staged, general_q && !gen_staged, lib->n_cus, lib->has_curved, st2);
    if (st2) {
      HIP_TRY(hipEventRecord(lib->ev_aux1, st2));
      HIP_TRY(hipStreamWaitEvent(st, lib->ev_aux1, 0));
    }
  }
  if (!(cc_staged || gen_staged)) {
    Timed t(b, "k_epa<full>", st);
    launch_epa_full<T>(b.blocks_for(n / 16 + 1, 64 / epa_we2<T>), st, wk, b.lv, b.io, b.q);
    return HFCL_OK;
  }
  // What ends the batch: the records of the finished polytopes (bound by memory), the continuation of the handed-over ones
  // (k_epa_resume_cc; as long as its longest chain of iterations) and the full-capacity tier (likewise).  The records run on a stream of
  // their own beside the latter two (with a convex x convex tier the full-capacity tier joins them there, beside the continuation).
  const bool aside = o.records_aside;
  if (aside) {
    if (int rc = ensure_aux(lib)) return rc;
    HIP_TRY(hipEventRecord(lib->ev_aux0, st));
    HIP_TRY(hipStreamWaitEvent(lib->aux, lib->ev_aux0, 0));
  }
  hipStream_t const rs = aside ? lib->aux.get() : st;
  {
    Timed t(b, "k_epa_records", rs);
    if constexpr (F32)
      if (cc_staged) launch_epa_records(b.blocks_for(n / 4 + 1, 256), rs, wk, b.lv, b.io, b.q);
    if (gen_staged) launch_epa_records_general<T>(b.blocks_for(n / 4 + 1, 256), rs, wk, b.lv, b.io, b.q, F32);
  }
  // (without a continuation kernel of its own the batch's stream takes the full-capacity tier)
  hipStream_t const fs = cc_staged ? rs : st;
  {
    Timed t(b, "k_epa<full>", fs);
    launch_epa_full<T>(b.blocks_for(n / 16 + 1, 64 / epa_we2<T>), fs, wk, b.lv, b.io, b.q);
  }
  if (aside) HIP_TRY(hipEventRecord(lib->ev_aux1, rs));
  if constexpr (F32) {
    if (cc_staged) {
      Timed t(b, "k_epa_resume_cc", st);
      launch_epa_resume_cc(b.blocks_for(n / 16 + 1, 64 / HFCL_EPA_CC_RESUME_WE), st, wk, b.lv, b.io, b.q);
    }
  }
  if (aside) HIP_TRY(hipStreamWaitEvent(st, lib->ev_aux1, 0));
  return HFCL_OK;
}

// ---- stage: the tail on `st` -- the buckets nothing evaluates, and the copy of the counts.  Last: a launch of a few waves that, between
// the GJK and the EPA kernels, only waited for a free CU while the other half of a split batch had the chip (0.2 ms of this stream's
// timeline on cfg5)
template <typename T>
static int finish_batch(Batch<T>& b, hipStream_t st) {
  hfcl_lib* lib = b.lib;
  {
    Timed t(b, "k_unsupported", st);
    // fp32: the pairs the batch's kernels marked as inconsistent, solved again in fp64 (hfcl_k_redo.hip) -- every record writer of the
    // batch is in `st`'s order by now.  Part of the tail's entry in last_kernel_breakdown.  A few percent of the batch at most, and a block
    // holds four full-capacity polytopes in LDS (three blocks fit a CU): a grid of resident blocks that stride over the list.
    if constexpr (std::is_same<T, float>::value) {
      if (b.io.redo_list)
        launch_redo(int(std::min<size_t>(b.blocks_for(b.n / 64 + 1, 64 / BS_W), size_t(lib->n_cus) * 3)), st, b.wk, lib->d_shapes64, lib->d_verts64, b.io, redo_params(b.q));
    }
    if (b.may(B_UNSUPPORTED)) launch_unsupported<T>(b.blocks_for(b.n, 256 * 64), st, b.wk, b.io, int(B_UNSUPPORTED));
    if (lib->h_meshes.empty()) {  // BVH shapes without any registered mesh: flagged, never left unwritten
      if (b.may(B_BVHSHAPE)) launch_unsupported<T>(b.blocks_for(b.n, 256 * 64), st, b.wk, b.io, int(B_BVHSHAPE));
      if (b.may(B_BVH)) launch_unsupported<T>(b.blocks_for(b.n, 256 * 64), st, b.wk, b.io, int(B_BVH));
    }
  }
  HIP_TRY(hipMemcpyAsync(lib->counts_dst ? lib->counts_dst : lib->h_counts.get(), lib->d_counts, N_COUNTERS * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  lib->ran_batch = lib->counts_dst == nullptr;
  HIP_TRY(hipGetLastError());
  return HFCL_OK;
}

// The whole pipeline for one batch, asynchronous on `st`.
template <typename T>
static int run_batch_one(hfcl_lib* lib, const uint32_t* d_s1, const uint32_t* d_s2, IO<T> io, size_t n, QParams<T> q, hipStream_t st) {
  if (n == 0) return HFCL_OK;
  if (n > 0xFFFFFFF0ull) {
    set_error("batch too large (max 2^32-16 pairs per call)");
    return HFCL_ERR_LIMIT;
  }
  HIP_TRY(hipSetDevice(lib->device));
  Batch<T> b{lib, Work(), LibView<T>(), io, q, n};
  lib->form_notes.clear();
  int rc = ensure_workspace(lib, n, b.any_gjk() && q.compute_penetration);
  if (rc) return rc;
  make_views(b, d_s1, d_s2);
  if constexpr (std::is_same<T, float>::value) {
    // The kernels that can mark a pair as inconsistent (hfcl_gjk.hpp: REDO_*) list it for k_redo, the batch's last stage: every GJK kernel
    // but the one of hull x hull pairs, their EPA tiers, k_triangle, and the Capsule x Capsule closed form.  A library that reaches
    // none of them (hulls only: the headline) has no list, no launch, and the records it always had.
    if (b.may(B_PRIM) || b.may(B_PC) || b.may(B_CP) || b.may(B_LARGE) || b.may(B_TRI) || (b.may(B_CLOSED) && lib->has_capsules)) {
      HIP_TRY(lib->d_redo.grow(lib->ws_capacity));
      b.io.redo_list = lib->d_redo;
      b.io.redo_count = lib->d_counts + CTR_REDO;
      b.io.redo_cap = uint32_t(n);
    }
  }
  for (auto& t : lib->timers) t.used = false;
  HIP_TRY(hipMemsetAsync(lib->d_counts, 0, N_COUNTER_WORDS * sizeof(uint32_t), st));
  {
    Timed t(b, "k_classify", st);
    launch_classify(b.blocks_for(n, CLS_BLOCK * 8), st, b.wk, lib->d_kinds, uint32_t(lib->n_shapes), q.mode != 1);
  }
  bool mesh_join_pending = false;
  const bool meshes_beside = meshes_run_beside(b);
  if (!lib->h_meshes.empty()) note_form(lib, "mesh_beside", meshes_beside);
  if (meshes_beside) {
    HIP_TRY(hipEventRecord(lib->ev_mesh_fork, st));
    HIP_TRY(hipStreamWaitEvent(lib->mesh_st, lib->ev_mesh_fork, 0));
    rc = launch_meshes(b, lib->mesh_st.get(), true);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(lib->ev_mesh_join, lib->mesh_st));
    rc = launch_solids(b, st);
    if (rc) return rc;
    if (lib->opt.mesh_beside < 2) HIP_TRY(hipStreamWaitEvent(st, lib->ev_mesh_join, 0));
    else mesh_join_pending = true;  // (the solids' EPA section first: no mesh kernel feeds its queues; joined in front of the batch's last launches)
  } else {
    rc = launch_solids(b, st);
    if (rc) return rc;
    rc = launch_meshes(b, st, false);
    if (rc) return rc;
  }
  if (q.compute_penetration && b.any_gjk()) {
    rc = launch_epa(b, st);
    if (rc) return rc;
  }
  if (mesh_join_pending) HIP_TRY(hipStreamWaitEvent(st, lib->ev_mesh_join, 0));
  return finish_batch(b, st);
}

// shallow clone for the second half of a split batch: a view of its owner's device shape tables (`own` of a helper stays empty), its
// owner's options (run_batch), everything else its own.  The view of `h` onto the tables `lib` owns (h == lib: the library's own):
void share_tables(hfcl_lib* h, const hfcl_lib* lib) {
  const hfcl_lib::Tables& t = lib->own;
  h->n_shapes = lib->n_shapes;
  h->d_shapes64 = t.shapes64;
  h->d_shapes32 = t.shapes32;
  h->d_verts64 = t.verts64;
  h->d_verts32 = t.verts32;
  h->d_kinds = t.kinds;
  h->possible_buckets = lib->possible_buckets;
  h->has_curved = lib->has_curved;
  h->has_flats = lib->has_flats;
  h->has_capsules = lib->has_capsules;
  h->d_graph_base = t.graph.base;
  h->d_graph_off = t.graph.off;
  h->d_graph_ent32 = t.graph.ent32;
  h->d_graph_ent64 = t.graph.ent64;
}
static hfcl_lib* make_helper(hfcl_lib* lib) {
  hfcl_lib* h = new hfcl_lib;
  h->device = lib->device;
  share_tables(h, lib);
  h->n_cus = lib->n_cus;
  bool ok = h->d_counts.grow(N_COUNTER_WORDS) == hipSuccess;
  ok = ok && h->h_counts.alloc(N_COUNTERS) == hipSuccess;
  ok = ok && h->d_epa_v0.grow(size_t(h->n_cus) * 16 * (64 / EPA_WE2) * EPA_MAX_VERTS * sizeof(Quad<double>)) == hipSuccess;
  if (!ok) {
    hfcl_lib_destroy(h);
    return nullptr;
  }
  memset(h->h_counts, 0, N_COUNTERS * sizeof(uint32_t));
  return h;
}

template <typename T>
static IO<T> io_at(const IO<T>& io, size_t lo) {  // (fp32: 7-float poses, no guesses)
  const size_t w = std::is_same<T, double>::value ? 12 : 7;
  return IO<T>{io.tf1 + w * lo, io.tf2 + w * lo, io.out + lo, io.gin ? io.gin + lo : nullptr, io.gout ? io.gout + lo : nullptr};
}

// Does a batch of n pairs of this library run as two halves on two streams?  Automatic choice: a library whose pairs
// spread over three or more of the iterative buckets (mixed scenes: cfg5 4.05 -> 3.80 ms) -- the halves then run different
// kernels side by side; with one or two kernels in the batch the halves only share the machine phase by phase and the
// doubled fixed costs lose 3 % (cfg2, cfg3).  A/B in profiles/r01_k_two_stream_overlap.txt.
bool batch_splits(const hfcl_lib* lib, size_t n) {
  constexpr size_t MIN_SPLIT = 1u << 17;
  int parts = lib->opt.split;
  if (parts == 0) {
    int kinds = 0;
    for (int b : {int(B_PRIM), int(B_CC), int(B_PC), int(B_CP), int(B_LARGE)}) kinds += (lib->possible_buckets >> b) & 1u;
    parts = kinds >= 3 ? 2 : 1;
  }
  // meshes keep query-wide side state (contact lists, pair ids in them): they run unsplit
  return parts >= 2 && n >= MIN_SPLIT && lib->h_meshes.empty();
}
int ensure_helper(hfcl_lib* lib) {
  if (lib->helper) return HFCL_OK;
  HIP_TRY(hipSetDevice(lib->device));
  hfcl_lib* h = make_helper(lib);
  Stream side;
  Event fork, join;
  if (!h || side.create() != hipSuccess || fork.create() != hipSuccess || join.create() != hipSuccess) {
    if (h) hfcl_lib_destroy(h);  // nothing half-made stays behind: the next call retries cleanly
    set_error("split batches: HIP allocation failed");
    return HFCL_ERR_HIP;
  }
  lib->side = std::move(side);
  lib->ev_fork = std::move(fork);
  lib->ev_join = std::move(join);
  lib->helper = h;
  return HFCL_OK;
}

template <typename T>
int run_batch(hfcl_lib* lib, const uint32_t* d_s1, const uint32_t* d_s2, IO<T> io, size_t n, QParams<T> q, hipStream_t st) {
  lib->last_split = false;
  if (!lib->in_host_batch) {
    lib->last_host = false;
    lib->host_notes.clear();
  }
  if (lib->graph_dirty) {
    const int rcg = upload_graph(lib);
    if (rcg) return rcg;
  }
  if (!batch_splits(lib, n)) return run_batch_one<T>(lib, d_s1, d_s2, io, n, q, st);
  int rc0 = ensure_helper(lib);
  if (rc0) return rc0;
  hfcl_lib* h2 = lib->helper;
  h2->opt = lib->opt;  // (the whole block, every batch: an option set since the helper was made holds for both halves)
  h2->kernel_timing = lib->kernel_timing;
  h2->break_distance = lib->break_distance;
  h2->bvh_params = lib->bvh_params;
  const size_t h = n / 2;  // unequal parts (0.35 / 0.6 / 0.7 of the batch first) measured slower on cfg3 and cfg5
  HIP_TRY(hipEventRecord(lib->ev_fork, st));  // the inputs are ready where the caller's stream stands now
  HIP_TRY(hipStreamWaitEvent(lib->side, lib->ev_fork, 0));
  int rc = run_batch_one<T>(lib, d_s1, d_s2, io, h, q, st);
  if (rc) return rc;
  rc = run_batch_one<T>(h2, d_s1 + h, d_s2 + h, io_at<T>(io, h), n - h, q, lib->side);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(lib->ev_join, lib->side));
  HIP_TRY(hipStreamWaitEvent(st, lib->ev_join, 0));  // results are complete in the caller's stream order
  lib->last_split = true;
  return HFCL_OK;
}

template int run_batch<double>(hfcl_lib*, const uint32_t*, const uint32_t*, IO<double>, size_t, QParams<double>, hipStream_t);
template int run_batch<float>(hfcl_lib*, const uint32_t*, const uint32_t*, IO<float>, size_t, QParams<float>, hipStream_t);
