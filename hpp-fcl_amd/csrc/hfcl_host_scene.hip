// hfcl_host_scene.hip -- host side of the scene queries (hfcl_scene_*) and of the cull of their pair lists (the kernels: hfcl_k_scene.hip,
// hfcl_k_cull.hip, ...; the terrain calls: hfcl_k_terrain.hip around hfcl_host_hfield.hip's hf_run).  The library object and what this
// unit calls of the other host units: hfcl_host.hpp.
#include "hfcl_host.hpp"
#include "hfcl_plan.hpp"
#include "hfcl_nearest.hpp"
#include "hfcl_nearest_self.hpp"
#include "hfcl_env.hpp"
#include "hfcl_nearest_env.hpp"
#include "hfcl_terrain.hpp"
#include "../../include/hppfcl_amd_nearest.h"
#include "../../include/hppfcl_amd_groups.h"
#include "../../include/hppfcl_amd_nearest_self.h"
#include "../../include/hppfcl_amd_nearest_env.h"
#include "../../include/hppfcl_amd_pairs.h"
#include "../../include/hppfcl_amd_env.h"

// =======================================================================================
// Scene queries (include/hppfcl_amd.h: hfcl_scene_*): an object -> shape table and a pair list resident on the library's device; a call
// evaluates the pair list for n_conf pose tables.  The flat query range q = c * n_pairs + p is cut into chunks; a chunk is expanded into the
// per-pair arrays of the batch entry points (k_scene_expand*), goes through hfcl_*_batch_device* exactly as a caller's batch of that size
// would, and its records are folded into the summaries of the configurations it touches (k_scene_fold).  No record changes on the way.
// =======================================================================================
struct hfcl_scene {
  hfcl_lib* lib = nullptr;
  size_t n_objects = 0, n_pairs = 0;
  DevBuf<uint32_t> d_object_shape, d_pairs;
  uint64_t epoch = 0;  // hfcl_lib::shapes_epoch when the scene was made
  int last_pairs_form = -1;  // hfcl_scene_last_pairs_form: how the last list of self pairs was made (-1: none yet)
  // object groups (hfcl_scene_set_groups; 0: none): an object's group, the groups' row masks, the groups present per column tile
  size_t n_groups = 0;
  DevBuf<uint8_t> d_group;
  DevBuf<uint64_t> d_collides, d_tile_groups;
  std::vector<uint8_t> h_group;  // (the groups again, for the tiling of a scene with an environment)
  // a static environment (hfcl_scene_set_environment*; has_env false: none): objects [n_moving, n_objects) with their poses in the
  // precision of the setter, their world boxes, a box per tile of PAIRS_TILE of them, and -- with groups -- the groups present per column
  // tile of hfcl_env.hpp's tiling (moving tiles, then environment tiles)
  bool has_env = false, env_f32 = false;
  size_t n_moving = 0;
  DevBuf<void> d_env_table;
  DevBuf<double> d_env_boxes, d_env_tile_boxes;
  DevBuf<uint64_t> d_env_tile_groups;
  // ... and the terms of the clearance bound (hfcl_nearest_env.hpp): two doubles per environment box, two per tile
  DevBuf<double> d_env_terms, d_env_tile_terms;
  size_t n_env() const { return n_objects - n_moving; }
  size_t rows() const { return has_env ? n_moving : n_objects; }  // hfcl_scene_n_moving: pose rows a configuration of an _env / terrain table
  // a height-field terrain (hfcl_scene_set_terrain; has_terrain false: none): a field of the library at one pose and the ascending list
  // of the objects tested against it; the objects' shapes on the host, for the setter's checks; the workspace of a chunk of terrain
  // queries -- the four arrays of the height-field call, and its records when the caller takes none --, what a call keeps per query for
  // the fold (bounds when the caller gives no buffer for them, status words), and the host form's summaries
  std::vector<uint32_t> h_object_shape;
  bool has_terrain = false;
  uint32_t terrain_hfield = 0;
  std::vector<uint32_t> h_terrain_objects;
  DevBuf<uint32_t> d_terrain_objects;
  DevBuf<double> d_terrain_tf;
  struct TerrainWs {
    DevBuf<uint32_t> d_hfield, d_shape, d_status;
    DevBuf<double> d_tfh, d_tfs, d_bounds;
    DevBuf<hfcl_result> d_rec;
    DevBuf<hfcl_scene_summary> d_summary;
  } tw;
};

static int scene_check_pairs(const char* who, const uint32_t* pairs, size_t n_pairs, size_t n_objects) {
  if (n_pairs > 0xFFFFFFF0ull) {
    set_error(std::string(who) + ": pair list too long (max 2^32-16 pairs)");
    return HFCL_ERR_LIMIT;
  }
  if (n_pairs && !pairs) {
    set_error(std::string(who) + ": null pair list");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  for (size_t k = 0; k < 2 * n_pairs; ++k)
    if (pairs[k] >= n_objects) {
      set_error(std::string(who) + ": object index " + std::to_string(pairs[k]) + " of pair " + std::to_string(k / 2) + " is outside the " +
                std::to_string(n_objects) + " objects");
      return HFCL_ERR_INVALID_ARGUMENT;
    }
  return HFCL_OK;
}
static int scene_upload(DevBuf<uint32_t>& dst, const uint32_t* src, size_t words) {  // (dst: empty)
  if (!words) return HFCL_OK;
  HIP_TRY(dst.grow(words));
  if (hipMemcpy(dst, src, words * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) {
    dst.reset();
    set_error("scene: copy to the device failed");
    return HFCL_ERR_HIP;
  }
  return HFCL_OK;
}

template <typename T> struct SceneTypes;
template <> struct SceneTypes<double> {
  using R = hfcl_result;
  static constexpr size_t WIDTH = 12;
};
template <> struct SceneTypes<float> {
  using R = hfcl_result_f32;
  static constexpr size_t WIDTH = 7;
};

// a chunk through the batch entry point of its precision
static int scene_batch(hfcl_lib* lib, const uint32_t* s1, const uint32_t* s2, const void* tf1, const void* tf2, size_t m,
                       const hfcl_collision_request* creq, const hfcl_distance_request* dreq, hfcl_result* rec, const hfcl_guess* gin,
                       hfcl_guess* gout, hipStream_t st) {
  return creq ? hfcl_collide_batch_device(lib, s1, s2, static_cast<const double*>(tf1), static_cast<const double*>(tf2), m, creq, rec, gin, gout, st)
              : hfcl_distance_batch_device(lib, s1, s2, static_cast<const double*>(tf1), static_cast<const double*>(tf2), m, dreq, rec, gin, gout, st);
}
static int scene_batch(hfcl_lib* lib, const uint32_t* s1, const uint32_t* s2, const void* tf1, const void* tf2, size_t m,
                       const hfcl_collision_request* creq, const hfcl_distance_request* dreq, hfcl_result_f32* rec, const hfcl_guess*, hfcl_guess*,
                       hipStream_t st) {
  return creq ? hfcl_collide_batch_device_f32(lib, s1, s2, static_cast<const float*>(tf1), static_cast<const float*>(tf2), m, creq, rec, st)
              : hfcl_distance_batch_device_f32(lib, s1, s2, static_cast<const float*>(tf1), static_cast<const float*>(tf2), m, dreq, rec, st);
}

// What every scene and cull call refuses before any work, in this order: a null scene, a stale one, a null table, an overflow; total:
// n_conf * n_pairs.  nothing_if_zero: the member (n_pairs: the scene calls, n_objects: the cull calls) that, like n_conf, leaves a call with
// nothing to do when it is 0 -- HFCL_OK before the table is looked at.  (The overflow test skips n_pairs == 0, which only the cull calls'
// rule lets through.)
template <typename T>
static int scene_validate_core(const char* who, const hfcl_scene* s, const void* table, size_t n_conf, size_t hfcl_scene::*nothing_if_zero,
                               size_t& total, bool own_list = true) {
  total = 0;
  if (!s) {
    set_error(std::string(who) + ": null scene");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (s->epoch != s->lib->shapes_epoch) {
    set_error(std::string(who) + ": the library's shapes were replaced (hfcl_lib_set_shapes) after this scene was created; create a new scene");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (n_conf == 0 || s->*nothing_if_zero == 0) return HFCL_OK;
  if (!table) {
    set_error(std::string(who) + ": null pose table");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (n_conf > ~size_t(0) / (s->n_objects * SceneTypes<T>::WIDTH * sizeof(T))) {
    set_error(std::string(who) + ": the pose table's size overflows");
    return HFCL_ERR_LIMIT;
  }
  if (!own_list) return HFCL_OK;  // (the calls that make or take a list of pairs: the scene's own plays no part, total stays 0)
  if (s->n_pairs && n_conf > ~size_t(0) / s->n_pairs) {
    set_error(std::string(who) + ": n_conf * n_pairs overflows");
    return HFCL_ERR_LIMIT;
  }
  total = n_conf * s->n_pairs;
  return HFCL_OK;
}
// Of a scene that is there, a narrow-phase call looks at the request (a null one: "null request", setup_collide / setup_distance) and at
// the outputs before the scene's state; a null scene is refused after this
template <typename T>
static int scene_request_and_outputs(const char* who, const hfcl_scene* s, const hfcl_collision_request* creq, const hfcl_distance_request* dreq,
                                     const void* out, const void* summary) {
  if (!s) return HFCL_OK;
  QParams<T> q;
  bool skip;
  const int rc = creq ? setup_collide<T>(creq, q, skip) : setup_distance<T>(dreq, q);
  if (rc) return rc;
  if (!out && !summary) {
    set_error(std::string(who) + ": records and summaries both NULL");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  return HFCL_OK;
}
// everything a scene call refuses before any work; total: n_conf * n_pairs (0: nothing to do)
template <typename T>
static int scene_validate(const char* who, const hfcl_scene* s, const void* table, size_t n_conf, const hfcl_collision_request* creq,
                          const hfcl_distance_request* dreq, const void* out, const void* summary, size_t& total,
                          size_t hfcl_scene::*nothing_if_zero = &hfcl_scene::n_pairs) {
  total = 0;
  const int rc = scene_request_and_outputs<T>(who, s, creq, dreq, out, summary);
  return rc ? rc : scene_validate_core<T>(who, s, table, n_conf, nothing_if_zero, total, nothing_if_zero == &hfcl_scene::n_pairs);
}
// what the cull calls refuse before any work; total: n_conf * n_pairs (0: no query)
template <typename T>
static int cull_validate(const char* who, const hfcl_scene* s, const void* table, size_t n_conf, size_t& total) {
  return scene_validate_core<T>(who, s, table, n_conf, &hfcl_scene::n_objects, total);
}
// ... the calls that make the list of pairs themselves (hfcl_scene_self_pairs*): the scene's own list is not looked at
template <typename T>
static int self_validate(const char* who, const hfcl_scene* s, const void* table, size_t n_conf) {
  size_t total;
  return scene_validate_core<T>(who, s, table, n_conf, &hfcl_scene::n_objects, total, false);
}

// workspace of chunks of up to m queries; recs: how many of the two record buffers; pieces: fold partials (0: none)
static int scene_workspace(hfcl_lib* lib, size_t m, int recs, bool gin, int gouts, size_t pieces) {
  hfcl_lib::SceneWs& w = lib->scene;
  if (m > w.cap) {
    reset_all(w.d_s1, w.d_s2, w.d_tf1, w.d_tf2);
    w.cap = 0;
    HIP_TRY(w.d_s1.grow(m));
    HIP_TRY(w.d_s2.grow(m));
    HIP_TRY(w.d_tf1.grow(m * 12 * sizeof(double)));  // (rows of either precision)
    HIP_TRY(w.d_tf2.grow(m * 12 * sizeof(double)));
    w.cap = m;
  }
  // (a buffer that grows is freed first, which waits for the device: nothing in flight reads the old one)
  for (int k = 0; k < recs; ++k) HIP_TRY(w.d_rec[k].grow(m * sizeof(hfcl_result)));
  if (gin) HIP_TRY(w.d_gin.grow(m));
  for (int k = 0; k < gouts; ++k) HIP_TRY(w.d_gout[k].grow(m));
  HIP_TRY(w.d_partials.grow(pieces));
  return HFCL_OK;
}
// How the list a call works on comes about -- named once, here, wherever a flavour is meant (SceneList, SceneCull, the functions on a
// list of pairs): culled from the scene's own pair list (hfcl_scene_cull*), made by the all-pairs sweep (hfcl_scene_self_pairs*), made by
// the sweep of the moving objects against a kept environment (hfcl_scene_env_pairs*)
enum class ListKind { Culled, Self, Env };
// A list of flat queries on the device, as hfcl_scene_cull_device leaves it (Culled): ascending ids, conf_begin theirs.  Where a function
// takes a pointer to one, nullptr is the flat range itself.
// The other flavour (Self: hfcl_scene_self_pairs_device leaves it): d_ids == nullptr, the entries are the pairs (i, j) themselves (d_pairs,
// two words an entry), the scene's own pair list plays no part, an entry's pair index in the summaries is its rank in its configuration,
// and a configuration has at most `shares` fold pieces (hfcl_pairs.hpp: pairs_shares).
// ... of a scene with an environment (Env: hfcl_scene_env_pairs_device leaves it): the call's table holds n_moving rows a configuration,
// the rows of j >= n_moving come from d_env_table.
// Made by query_list / pair_list below, nowhere else.
struct SceneList {
  ListKind kind;
  const uint64_t* d_ids;
  const uint64_t* d_conf_begin;
  size_t n_conf;
  const uint32_t* d_pairs;
  uint32_t shares;
  const void* d_env_table;
  size_t n_moving;
  bool ranked() const { return kind != ListKind::Culled; }
};
static SceneList query_list(const uint64_t* d_ids, const uint64_t* d_conf_begin, size_t n_conf) {
  return SceneList{ListKind::Culled, d_ids, d_conf_begin, n_conf, nullptr, 0u, nullptr, 0};
}
// kind: Self or Env; n_listed > 0 entries at d_pairs
static SceneList pair_list(const hfcl_scene* s, ListKind kind, const uint32_t* d_pairs, const uint64_t* d_conf_begin, size_t n_conf, size_t n_listed) {
  if (kind == ListKind::Env)
    return SceneList{kind, nullptr, d_conf_begin, n_conf, d_pairs, uint32_t(env_shares(n_listed, s->n_moving, s->n_env())), s->d_env_table.get(), s->n_moving};
  return SceneList{kind, nullptr, d_conf_begin, n_conf, d_pairs, uint32_t(pairs_shares(n_listed, s->n_objects)), nullptr, 0};
}
// fold pieces of a configuration of a call
static uint32_t scene_list_shares(const hfcl_scene* s, const SceneList* list) {
  return list && list->ranked() ? list->shares : scene_shares(uint32_t(s->n_pairs));
}
// fold partials of a call in chunks of `chunk`
static size_t scene_pieces(const hfcl_scene* s, const SceneList* list, size_t chunk) {
  if (list && list->ranked()) return list->shares <= 1u ? 0 : list->n_conf * size_t(list->shares);
  return list ? scene_listed_pieces_bound(s->n_pairs, list->n_conf) : scene_pieces_bound(s->n_pairs, chunk);
}

// expansion of the chunk [k0, k0 + m) of the flat range or of the list, the batch, the fold: all on st
template <typename T>
static int scene_chunk_run(hfcl_scene* s, const void* d_table, const SceneList* list, size_t k0, size_t m, const hfcl_collision_request* creq,
                           const hfcl_distance_request* dreq, typename SceneTypes<T>::R* d_rec, hfcl_scene_summary* d_summary,
                           const hfcl_guess* d_gin, hfcl_guess* d_gout, hipStream_t st) {
  hfcl_lib* lib = s->lib;
  hfcl_lib::SceneWs& w = lib->scene;
  constexpr bool f32 = std::is_same<T, float>::value;
  const int max_blocks = lib->n_cus * 16;
  SceneExpandArgs ea;
  ea.pairs = s->d_pairs;
  ea.object_shape = s->d_object_shape;
  ea.object_tf = d_table;
  ea.n_objects = s->n_objects;
  ea.n_pairs = uint32_t(s->n_pairs);
  ea.q0 = list ? 0 : k0;  // (a list's rows name their queries)
  ea.c0 = 0;
  ea.p0 = 0;
  if (!list || !list->ranked()) scene_query(ea.q0, ea.n_pairs, ea.c0, ea.p0);
  ea.m = uint32_t(m);
  ea.s1 = w.d_s1;
  ea.s2 = w.d_s2;
  ea.tf1 = w.d_tf1;
  ea.tf2 = w.d_tf2;
  if (list && list->kind == ListKind::Env) {
    ea.n_objects = list->n_moving;
    launch_scene_expand_env(st, ea, list->d_pairs, list->d_conf_begin, list->n_conf, k0, list->d_env_table, f32, max_blocks);
  } else if (list && list->ranked())
    launch_scene_expand_pairs(st, ea, list->d_pairs, list->d_conf_begin, list->n_conf, k0, f32, max_blocks);
  else if (list)
    launch_scene_expand_listed(st, ea, list->d_ids + k0, f32, max_blocks);
  else
    launch_scene_expand(st, ea, f32, max_blocks);
  const int rc = scene_batch(lib, w.d_s1, w.d_s2, w.d_tf1, w.d_tf2, m, creq, dreq, d_rec, d_gin, d_gout, st);
  if (rc || !d_summary) return rc;
  const double margin = creq ? creq->security_margin : 0.0;
  hfcl_scene_summary* partials = scene_list_shares(s, list) > 1u ? w.d_partials.get() : nullptr;
  if (list) {
    SceneFoldListedArgs fa;
    fa.rec = d_rec;
    fa.ids = list->d_ids;
    fa.conf_begin = list->d_conf_begin;
    fa.k0 = k0;
    fa.k1 = k0 + m;
    fa.n_pairs = ea.n_pairs;
    fa.margin = margin;
    fa.collide = creq ? 1 : 0;
    fa.summary = d_summary;
    fa.partials = partials;
    fa.n_conf = list->n_conf;
    fa.shares = scene_list_shares(s, list);
    if (list->ranked())
      launch_scene_fold_ranked(st, fa, list->shares, f32, max_blocks);
    else
      launch_scene_fold_listed(st, fa, f32, max_blocks);
  } else {
    SceneFoldArgs fa;
    fa.rec = d_rec;
    fa.q0 = k0;
    fa.q1 = k0 + m;
    fa.n_pairs = ea.n_pairs;
    fa.g0 = scene_piece_of(k0, fa.n_pairs);
    fa.n_pieces = scene_piece_of(k0 + m - 1, fa.n_pairs) - fa.g0 + 1;
    fa.margin = margin;
    fa.collide = creq ? 1 : 0;
    fa.summary = d_summary;
    fa.partials = partials;
    launch_scene_fold(st, fa, f32, max_blocks);
  }
  return HFCL_OK;
}
// An error after work was enqueued: the second half of a split batch may be running on the library's side stream -- the caller's stream
// waits for it, so that "everything this call started is ordered before what the caller enqueues next" holds on the error path too
static void scene_join_side(hfcl_lib* lib, hipStream_t st) {
  if (lib->side && lib->ev_join && hipEventRecord(lib->ev_join, lib->side) == hipSuccess) (void)hipStreamWaitEvent(st, lib->ev_join, 0);
}

// The bucket populations of a host form (one at a time: HostBatchScope): COUNT_SLOTS pinned slots, a chunk's populations in the first half
// of its slot, its second half's -- when it ran split -- in the other.  Chunk k uses slot k % COUNT_SLOTS once chunk k - COUNT_SLOTS has
// been added up.
struct SceneCountSlots {
  static constexpr int CS = hfcl_lib::SceneWs::COUNT_SLOTS;
  static constexpr size_t SLOT_WORDS = 2 * size_t(N_COUNTERS);
  // the pinned block and the events, once per library: before the first SceneCountSlots
  static int ready(hfcl_lib::SceneWs& w) {
    if (!w.h_counts) HIP_TRY(w.h_counts.alloc(CS * SLOT_WORDS));
    for (Event& e : w.ev_counts)
      if (!e) HIP_TRY(e.create());
    return HFCL_OK;
  }
  hfcl_lib* lib;
  HostBatchScope scope;
  bool slot_split[CS] = {};
  size_t k = 0;  // chunks so far
  explicit SceneCountSlots(hfcl_lib* l) : lib(l), scope(l) {
    memset(lib->scene.h_counts, 0, CS * SLOT_WORDS * sizeof(uint32_t));  // (a skipped batch -- -inf margin -- copies no counters)
  }
  void harvest(int slot) {  // a finished chunk's bucket populations into the call's sums; the slot is free again
    uint32_t* c = lib->scene.h_counts + size_t(slot) * SLOT_WORDS;
    for (int i = 0; i < N_COUNTERS; ++i) lib->acc_counts[i] += c[i] + (slot_split[slot] ? c[N_COUNTERS + i] : 0u);
    memset(c, 0, SLOT_WORDS * sizeof(uint32_t));
  }
  int before_chunk(size_t m) {
    hfcl_lib::SceneWs& w = lib->scene;
    const int slot = int(k % CS);
    if (k >= size_t(CS)) {  // the chunk that used this slot has run: its counters are on the host
      HIP_TRY(hipEventSynchronize(w.ev_counts[slot]));
      harvest(slot);
    }
    lib->counts_dst = w.h_counts + size_t(slot) * SLOT_WORDS;
    if (batch_splits(lib, m)) {
      const int rc = ensure_helper(lib);
      if (rc) return rc;
      lib->helper->counts_dst = lib->counts_dst + N_COUNTERS;
    }
    return HFCL_OK;
  }
  int after_chunk(hipStream_t st) {
    const int slot = int(k % CS);
    slot_split[slot] = lib->last_split;
    HIP_TRY(hipEventRecord(lib->scene.ev_counts[slot], st));
    ++k;
    return HFCL_OK;
  }
  // the call's streams have been waited for and nothing failed: the populations are complete
  void harvest_rest() {
    for (int slot = 0; slot < CS && size_t(slot) < k; ++slot) harvest(slot);
  }
};

// `work` queries of the flat range (list: entries of the list) in chunks, one after the other on st: the workspace, then per chunk its
// records to d_out (nullptr: the workspace's buffer), a host form's count slots (counts; nullptr: none) around it.
template <typename T>
static int scene_chunks_device(hfcl_scene* s, const void* d_table, const SceneList* list, size_t work, const hfcl_collision_request* creq,
                               const hfcl_distance_request* dreq, typename SceneTypes<T>::R* d_out, hfcl_scene_summary* d_summary,
                               const hfcl_guess* d_gin, hfcl_guess* d_gout, hipStream_t st, SceneCountSlots* counts = nullptr) {
  hfcl_lib* lib = s->lib;
  const size_t chunk = scene_chunk_size(work, lib->opt.scene_chunk);
  int rc = scene_workspace(lib, chunk, d_out ? 0 : 1, false, 0, d_summary ? scene_pieces(s, list, chunk) : 0);
  if (rc) return rc;
  for (size_t k0 = 0; k0 < work; k0 += chunk) {
    const size_t m = std::min(chunk, work - k0);
    auto* rec = d_out ? d_out + k0 : static_cast<typename SceneTypes<T>::R*>(lib->scene.d_rec[0].get());
    rc = counts ? counts->before_chunk(m) : HFCL_OK;
    if (!rc) rc = scene_chunk_run<T>(s, d_table, list, k0, m, creq, dreq, rec, d_summary, d_gin ? d_gin + k0 : nullptr, d_gout ? d_gout + k0 : nullptr, st);
    if (!rc && counts) rc = counts->after_chunk(st);
    if (rc) {
      scene_join_side(lib, st);
      return rc;
    }
  }
  HIP_TRY(hipGetLastError());
  return HFCL_OK;
}

template <typename T>
static int scene_device(const char* who, hfcl_scene* s, const void* d_table, size_t n_conf, const hfcl_collision_request* creq,
                        const hfcl_distance_request* dreq, typename SceneTypes<T>::R* d_out, hfcl_scene_summary* d_summary,
                        const hfcl_guess* d_gin, hfcl_guess* d_gout, hipStream_t st) {
  size_t total;
  const int rc = scene_validate<T>(who, s, d_table, n_conf, creq, dreq, d_out, d_summary, total);
  if (rc || !total) return rc;
  HIP_TRY(hipSetDevice(s->lib->device));
  return scene_chunks_device<T>(s, d_table, nullptr, total, creq, dreq, d_out, d_summary, d_gin, d_gout, st);
}


// ---------------------------------------------------------------------------------------
// Culling the pair list per configuration (hfcl_scene_cull*), and the scene calls on the list that is left (hfcl_scene_*_listed*,
// hfcl_scene_*_culled).  hfcl_k_cull.hip has the kernels, hfcl_cull.hpp the arithmetic.
// ---------------------------------------------------------------------------------------
// the library's local boxes on the device, rebuilt when shapes or meshes were registered since
int ensure_local_boxes(hfcl_lib* lib) {  // (declared in hfcl_host.hpp: the octree unit builds the solids' OBBs from them)
  if (!lib->local_boxes_dirty && lib->d_local_boxes) return HFCL_OK;
  const double nan = __builtin_nan("");
  std::vector<double> boxes(6 * lib->n_shapes);
  for (size_t i = 0; i < lib->n_shapes; ++i) {
    const hfcl_shape& s = lib->h_shapes[i];
    Box3 b;
    if (s.type == HFCL_BV_OBBRSS) {
      if (s.bvh_index < lib->h_meshes.size())
        b = mesh_local_box(lib->h_bvh_verts.data() + 3 * size_t(lib->h_meshes[s.bvh_index].vert_off), lib->h_mesh_nverts[s.bvh_index]);
      else  // (no such model: the narrow phase refuses the pair; a NaN box keeps it in the list)
        for (int k = 0; k < 3; ++k) b.lo[k] = b.hi[k] = nan;
    } else {
      b = shape_local_box(s, lib->h_verts.data());
    }
    for (int k = 0; k < 3; ++k) {
      boxes[6 * i + k] = b.lo[k];
      boxes[6 * i + 3 + k] = b.hi[k];
    }
  }
  lib->d_local_boxes.reset();  // (waits for the device: nothing in flight reads the old table)
  HIP_TRY(lib->d_local_boxes.grow(std::max<size_t>(boxes.size(), 6)));
  HIP_TRY(hipMemcpy(lib->d_local_boxes, boxes.data(), boxes.size() * sizeof(double), hipMemcpyHostToDevice));
  lib->local_boxes_dirty = false;
  return HFCL_OK;
}

static int cull_check_inflate(const char* who, double inflate) {
  if (!(inflate >= 0.0)) {
    set_error(std::string(who) + ": inflate must be >= 0 (and not NaN)");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  return HFCL_OK;
}

// world boxes of the whole table -> d_out (n_conf * n_objects * 6 doubles), on st
template <typename T>
static int scene_boxes_device(const char* who, hfcl_scene* s, const void* d_table, size_t n_conf, double* d_out, hipStream_t st) {
  size_t total;
  int rc = cull_validate<T>(who, s, d_table, n_conf, total);
  if (rc || n_conf == 0 || s->n_objects == 0) return rc;
  if (!d_out) {
    set_error(std::string(who) + ": null output");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  hfcl_lib* lib = s->lib;
  HIP_TRY(hipSetDevice(lib->device));
  rc = ensure_local_boxes(lib);
  if (rc) return rc;
  launch_cull_aabbs(st, d_table, std::is_same<T, float>::value, s->d_object_shape, lib->d_local_boxes, s->n_objects, n_conf * s->n_objects, d_out);
  HIP_TRY(hipGetLastError());
  return HFCL_OK;
}

// ballots, workgroup counts and offsets of a chunk of `chunk` queries, the running count
static int cull_chunk_buffers(hfcl_lib* lib, size_t chunk) {
  hfcl_lib::SceneWs& w = lib->scene;
  const size_t n_blocks = (chunk + CULL_BLOCK - 1) / CULL_BLOCK;
  HIP_TRY(w.d_words.grow(n_blocks * CULL_WAVES));
  if (n_blocks > w.blocks_cap) {
    reset_all(w.d_block_counts, w.d_block_offsets);
    w.blocks_cap = 0;
    HIP_TRY(w.d_block_counts.grow(n_blocks));
    HIP_TRY(w.d_block_offsets.grow(n_blocks));
    w.blocks_cap = n_blocks;
  }
  HIP_TRY(w.d_running.grow(2));
  return HFCL_OK;
}

// what every cull of a scene's flat range gives its kernels, whatever marks the queries
static void cull_args(CullArgs& a, const hfcl_scene* s, size_t total, size_t n_conf, double inflate, uint64_t* d_n_listed) {
  hfcl_lib::SceneWs& w = s->lib->scene;
  a.pairs = s->d_pairs;
  a.boxes = w.d_boxes;
  a.n_objects = s->n_objects;
  a.n_pairs = uint32_t(s->n_pairs);
  a.total = total;
  a.n_conf = n_conf;
  a.inflate = inflate;
  a.words = w.d_words;
  a.block_counts = w.d_block_counts;
  a.block_offsets = w.d_block_offsets;
  a.running = w.d_running;
  a.n_listed = d_n_listed;
}
// the chunks of the flat range [0, a.total) in turn: a's q0, c0, p0, m and first are the chunk's when per_chunk() is called
template <typename F>
static void cull_chunks(CullArgs& a, size_t chunk, F&& per_chunk) {
  for (size_t q0 = 0; q0 < a.total; q0 += chunk) {
    a.q0 = q0;
    scene_query(q0, a.n_pairs, a.c0, a.p0);
    a.m = uint32_t(std::min<size_t>(chunk, a.total - q0));
    a.first = q0 == 0 ? 1 : 0;
    per_chunk();
  }
}
// A list whose length is known only afterwards: make() enqueues its making into `ids` (as large as it is then) on st, the count at d_count
// is read back -- 8 bytes, st waited for --, and a list that outgrew the buffer is made once more in one of its size.  want_ids = false:
// the count alone.
// (words: the buffer's elements per list entry -- 1 for a list of queries, 2 for a list of pairs)
template <typename W, typename Make>
static int list_and_count(DevBuf<W>& ids, bool want_ids, const uint64_t* d_count, hipStream_t st, uint64_t& n, Make&& make, size_t words = 1) {
  for (int attempt = 0; attempt < 2; ++attempt) {
    const int rc = make();
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(&n, d_count, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (!want_ids || n <= ids.capacity() / words) break;
    HIP_TRY(ids.grow(size_t(n) * words));
  }
  return HFCL_OK;
}

// The cull of the whole flat range on st: the list (ids below `capacity`), conf_begin, the count.  Nothing is read back.
template <typename T>
static int cull_device(const char* who, hfcl_scene* s, const void* d_table, size_t n_conf, double inflate, uint64_t* d_ids, size_t capacity,
                       uint64_t* d_conf_begin, uint64_t* d_n_listed, hipStream_t st) {
  size_t total;
  int rc = cull_validate<T>(who, s, d_table, n_conf, total);
  if (rc) return rc;
  rc = cull_check_inflate(who, inflate);
  if (rc) return rc;
  if (!d_n_listed) {
    set_error(std::string(who) + ": null count");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  hfcl_lib* lib = s->lib;
  HIP_TRY(hipSetDevice(lib->device));
  if (!total) {  // no query: an empty list
    HIP_TRY(hipMemsetAsync(d_n_listed, 0, sizeof(uint64_t), st));
    if (d_conf_begin) HIP_TRY(hipMemsetAsync(d_conf_begin, 0, (n_conf + 1) * sizeof(uint64_t), st));
    return HFCL_OK;
  }
  rc = ensure_local_boxes(lib);
  if (rc) return rc;
  hfcl_lib::SceneWs& w = lib->scene;
  const size_t chunk = cull_chunk_size(total, lib->opt.scene_cull_chunk);
  const size_t conf_per_chunk = std::min<size_t>(n_conf, chunk / s->n_pairs + 2);
  HIP_TRY(w.d_boxes.grow(conf_per_chunk * s->n_objects * 6));
  rc = cull_chunk_buffers(lib, chunk);
  if (rc) return rc;
  constexpr bool f32 = std::is_same<T, float>::value;
  CullArgs a;
  cull_args(a, s, total, n_conf, inflate, d_n_listed);
  a.ids = d_ids;
  a.capacity = d_ids ? capacity : 0;
  a.conf_begin = d_conf_begin;
  cull_chunks(a, chunk, [&]() {  // the boxes of the configurations the chunk touches, then the chunk
    a.c_box0 = a.c0;
    const uint64_t c_last = (a.q0 + a.m - 1) / s->n_pairs;
    const char* rows = static_cast<const char*>(d_table) + a.c0 * s->n_objects * SceneTypes<T>::WIDTH * sizeof(T);
    launch_cull_aabbs(st, rows, f32, s->d_object_shape, lib->d_local_boxes, s->n_objects, (c_last - a.c0 + 1) * s->n_objects, w.d_boxes);
    launch_cull_chunk(st, a);
  });
  HIP_TRY(hipGetLastError());
  return HFCL_OK;
}

// the host forms' stream
static int scene_host_stream(hfcl_lib::SceneWs& w) {
  if (!w.s_cmp) HIP_TRY(w.s_cmp.create());
  return HFCL_OK;
}
// the table of a host form onto the device (w.d_table), on w.s_cmp
static int scene_table_in(hfcl_lib::SceneWs& w, const void* table, size_t bytes) {
  HIP_TRY(w.d_table.grow(bytes));
  HIP_TRY(hipMemcpyAsync(w.d_table, table, bytes, hipMemcpyHostToDevice, w.s_cmp));
  return HFCL_OK;
}
// The cull of a table that is on the device into the library's own list (w.d_ids, w.d_conf_begin), and the one read-back: the count.
// A list that outgrows the buffer is culled again into a larger one.
template <typename T>
static int cull_into_workspace(const char* who, hfcl_scene* s, const void* d_table, size_t n_conf, size_t total, double inflate, bool want_ids,
                               uint64_t& n_listed) {
  hfcl_lib* lib = s->lib;
  hfcl_lib::SceneWs& w = lib->scene;
  HIP_TRY(w.d_conf_begin.grow(n_conf + 1));
  HIP_TRY(w.d_running.grow(2));
  if (want_ids) HIP_TRY(w.d_ids.grow(list_capacity_guess(total)));
  return list_and_count(w.d_ids, want_ids, w.d_running + 1, w.s_cmp, n_listed, [&]() {
    return cull_device<T>(who, s, d_table, n_conf, inflate, want_ids ? w.d_ids.get() : nullptr, w.d_ids.capacity(), w.d_conf_begin, w.d_running + 1, w.s_cmp);
  });
}

template <typename T>
static int scene_cull_host(const char* who, hfcl_scene* s, const void* table, size_t n_conf, double inflate, uint64_t* query_ids, size_t capacity,
                           uint64_t* conf_begin, size_t* n_listed) {
  size_t total;
  int rc = cull_validate<T>(who, s, table, n_conf, total);
  if (!rc) rc = cull_check_inflate(who, inflate);
  if (!rc && !n_listed) {
    set_error(std::string(who) + ": null count");
    rc = HFCL_ERR_INVALID_ARGUMENT;
  }
  if (rc) return rc;
  *n_listed = 0;
  if (!total) {
    if (conf_begin) memset(conf_begin, 0, (n_conf + 1) * sizeof(uint64_t));
    return HFCL_OK;
  }
  hfcl_lib* lib = s->lib;
  hfcl_lib::SceneWs& w = lib->scene;
  HIP_TRY(hipSetDevice(lib->device));
  rc = scene_host_stream(w);
  if (!rc) rc = scene_table_in(w, table, n_conf * s->n_objects * SceneTypes<T>::WIDTH * sizeof(T));
  uint64_t n = 0;
  if (!rc) rc = cull_into_workspace<T>(who, s, w.d_table, n_conf, total, inflate, query_ids != nullptr, n);
  if (rc) {
    hipStreamSynchronize(w.s_cmp);
    return rc;
  }
  *n_listed = size_t(n);
  if (query_ids && capacity < n) {
    set_error(std::string(who) + ": " + std::to_string(n) + " queries survive, the list holds " + std::to_string(capacity));
    return HFCL_ERR_LIMIT;
  }
  if (query_ids && n) HIP_TRY(hipMemcpyAsync(query_ids, w.d_ids, n * sizeof(uint64_t), hipMemcpyDeviceToHost, w.s_cmp));
  if (conf_begin) HIP_TRY(hipMemcpyAsync(conf_begin, w.d_conf_begin, (n_conf + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, w.s_cmp));
  HIP_TRY(hipStreamSynchronize(w.s_cmp));
  return HFCL_OK;
}

template <typename T>
static int scene_boxes_host(const char* who, hfcl_scene* s, const void* table, size_t n_conf, double* aabbs_out) {
  size_t total;
  int rc = cull_validate<T>(who, s, table, n_conf, total);
  if (rc || n_conf == 0 || s->n_objects == 0) return rc;
  if (!aabbs_out) {
    set_error(std::string(who) + ": null output");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  hfcl_lib* lib = s->lib;
  hfcl_lib::SceneWs& w = lib->scene;
  HIP_TRY(hipSetDevice(lib->device));
  const size_t rows = n_conf * s->n_objects;
  rc = scene_host_stream(w);
  if (!rc) rc = [&]() -> int { HIP_TRY(w.d_boxes.grow(rows * 6)); return HFCL_OK; }();
  if (!rc) rc = scene_table_in(w, table, rows * SceneTypes<T>::WIDTH * sizeof(T));
  if (!rc) rc = scene_boxes_device<T>(who, s, w.d_table, n_conf, w.d_boxes, w.s_cmp);
  if (rc) {
    hipStreamSynchronize(w.s_cmp);
    return rc;
  }
  HIP_TRY(hipMemcpyAsync(aabbs_out, w.d_boxes, rows * 6 * sizeof(double), hipMemcpyDeviceToHost, w.s_cmp));
  HIP_TRY(hipStreamSynchronize(w.s_cmp));
  return HFCL_OK;
}

// The device form on a list.  The ids are not checked: ascending, below n_conf * n_pairs, conf_begin theirs -- as hfcl_scene_cull_device leaves them.
// merge (hfcl_scene_nearest*): the summaries are not re-initialised, the list's records are merged into what is stored; counts: as
// scene_chunks_device takes them.
template <typename T>
static int scene_listed_device(const char* who, hfcl_scene* s, const void* d_table, size_t n_conf, const uint64_t* d_ids, size_t n_listed,
                               const uint64_t* d_conf_begin, const hfcl_collision_request* creq, const hfcl_distance_request* dreq,
                               typename SceneTypes<T>::R* d_out, hfcl_scene_summary* d_summary, const hfcl_guess* d_gin, hfcl_guess* d_gout,
                               hipStream_t st, bool merge = false, SceneCountSlots* counts = nullptr) {
  size_t total;
  const int rc = scene_validate<T>(who, s, d_table, n_conf, creq, dreq, d_out, d_summary, total);
  if (rc) return rc;
  if (d_summary && !d_conf_begin) {
    set_error(std::string(who) + ": summaries need conf_begin");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (n_listed > total) {
    set_error(std::string(who) + ": more list entries than queries");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (n_listed && !d_ids) {
    set_error(std::string(who) + ": null list");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  hfcl_lib* lib = s->lib;
  HIP_TRY(hipSetDevice(lib->device));
  if (d_summary && !merge) launch_scene_summary_init(st, d_summary, n_conf, lib->n_cus * 16);
  if (!n_listed) {
    HIP_TRY(hipGetLastError());
    return HFCL_OK;
  }
  const SceneList list = query_list(d_ids, d_conf_begin, n_conf);
  return scene_chunks_device<T>(s, d_table, &list, n_listed, creq, dreq, d_out, d_summary, d_gin, d_gout, st, counts);
}

// ---------------------------------------------------------------------------------------
// The self-collision pairs per configuration (include/hppfcl_amd_pairs.h: hfcl_scene_self_pairs*): what is the all-pairs sweep's own.  The
// list maker and the scene calls on such a list (hfcl_scene_*_pairs_device*, hfcl_scene_*_self) are one with the environment's: further
// down, "A list of pairs made on the device, of either kind".  hfcl_k_pairs.hip has the kernels, hfcl_pairs.hpp the arithmetic.
// ---------------------------------------------------------------------------------------
// every entry point of hppfcl_amd_pairs.h, before anything else
static int pairs_need_device() {
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) {
    set_error("no HIP device available (hipGetDeviceCount): the engine has no CPU fallback");
    return HFCL_ERR_NO_DEVICE;
  }
  return HFCL_OK;
}
// the entry points of hppfcl_amd_groups.h: a null scene, then a stale one; a table to the device
static int groups_scene(const char* who, const hfcl_scene* s) {
  if (!s) {
    set_error(std::string(who) + ": null scene");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (s->epoch != s->lib->shapes_epoch) {
    set_error(std::string(who) + ": the library's shapes were replaced (hfcl_lib_set_shapes) after this scene was created; create a new scene");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  return HFCL_OK;
}
template <typename W>
static int groups_upload(DevBuf<W>& dst, const W* src, size_t n) {  // (dst: empty)
  HIP_TRY(dst.grow(n));
  HIP_TRY(hipMemcpy(dst, src, n * sizeof(W), hipMemcpyHostToDevice));
  return HFCL_OK;
}
// a scan workgroup adds the counts of PAIRS_SCAN_BLOCK rows in 32 bits: a row has fewer than n_objects entries
constexpr size_t PAIRS_MAX_OBJECTS = (size_t(1) << 32) / PAIRS_SCAN_BLOCK;
static int self_pairs_limits(const char* who, const hfcl_scene* s) {
  if (s->n_objects > PAIRS_MAX_OBJECTS) {
    set_error(std::string(who) + ": the all-pairs test takes scenes of at most " + std::to_string(PAIRS_MAX_OBJECTS) + " objects");
    return HFCL_ERR_LIMIT;
  }
  return HFCL_OK;
}
// summaries name a pair by its rank in its configuration, in 32 bits
static int pairs_rank_limit(const char* who, uint64_t n_listed, size_t n_objects) {
  if (pairs_shares(n_listed, n_objects) > 0xFFFFFFFFull / SCENE_FOLD_SHARE) {
    set_error(std::string(who) + ": a configuration could hold 2^32 entries or more; summaries rank an entry in 32 bits");
    return HFCL_ERR_LIMIT;
  }
  return HFCL_OK;
}
// counts, offsets and scan sums of a chunk of `rows` rows, the running count
static int pairs_chunk_buffers(hfcl_lib* lib, size_t rows) {
  hfcl_lib::SceneWs& w = lib->scene;
  if (rows > w.rows_cap) {
    reset_all(w.d_row_counts, w.d_row_offsets, w.d_row_sums, w.d_row_sum_offsets);
    w.rows_cap = 0;
    const size_t n_sums = (rows + PAIRS_SCAN_BLOCK - 1) / PAIRS_SCAN_BLOCK;
    HIP_TRY(w.d_row_counts.grow(rows));
    HIP_TRY(w.d_row_offsets.grow(rows));
    HIP_TRY(w.d_row_sums.grow(n_sums));
    HIP_TRY(w.d_row_sum_offsets.grow(n_sums));
    w.rows_cap = rows;
  }
  HIP_TRY(w.d_running.grow(2));
  return HFCL_OK;
}

// what every sweep over a scene's row blocks gives its kernels, whatever it lists: the geometry, the chunk's row arrays, the groups
static void pairs_args(PairsArgs& a, const hfcl_scene* s, const PairsGeometry& geo, bool small, size_t n_conf) {
  hfcl_lib::SceneWs& w = s->lib->scene;
  a.boxes = w.d_boxes;
  a.n_objects = geo.n_objects;
  a.rows_per_block = geo.rows_per_block;
  a.blocks_per_conf = geo.blocks_per_conf;
  a.small = small ? 1 : 0;
  a.total_rows = uint64_t(n_conf) * geo.n_objects;
  a.n_conf = n_conf;
  a.inflate = 0.0;
  a.row_counts = w.d_row_counts;
  a.row_offsets = w.d_row_offsets;
  a.sums = w.d_row_sums;
  a.sum_offsets = w.d_row_sum_offsets;
  a.running = w.d_running;
  a.pairs = nullptr;
  a.capacity = 0;
  a.conf_begin = nullptr;
  a.n_listed = nullptr;
  a.group = s->n_groups ? s->d_group.get() : nullptr;
  a.collides = s->n_groups ? s->d_collides.get() : nullptr;
  a.tile_groups = s->n_groups ? s->d_tile_groups.get() : nullptr;
}
// the chunks of n_blocks row blocks, `per` a chunk, in turn: the boxes of the configurations a chunk touches (w.d_boxes), then
// per_chunk() with a's chunk members set
template <typename T, typename F>
static void pairs_chunks(PairsArgs& a, const hfcl_scene* s, const void* d_table, const PairsGeometry& geo, uint64_t n_blocks, uint64_t per,
                         hipStream_t st, F&& per_chunk) {
  hfcl_lib* lib = s->lib;
  const uint32_t n = geo.n_objects;
  for (uint64_t g0 = 0; g0 < n_blocks; g0 += per) {
    a.g0 = g0;
    a.n_blocks = uint32_t(std::min<uint64_t>(per, n_blocks - g0));
    a.row0 = pairs_block_row(geo, g0);
    a.n_rows = uint32_t(pairs_block_row(geo, g0 + a.n_blocks) - a.row0);
    a.first = g0 == 0 ? 1 : 0;
    a.c_box0 = g0 / geo.blocks_per_conf;
    const uint64_t c_last = (g0 + a.n_blocks - 1) / geo.blocks_per_conf;
    const char* rows = static_cast<const char*>(d_table) + a.c_box0 * n * SceneTypes<T>::WIDTH * sizeof(T);
    launch_cull_aabbs(st, rows, std::is_same<T, float>::value, s->d_object_shape, lib->d_local_boxes, n, (c_last - a.c_box0 + 1) * n, lib->scene.d_boxes);
    per_chunk();
  }
}

// The all-pairs sweep of a call over n_conf configurations, planned once (hfcl_plan.hpp: self_sweep_plan): the list maker and the
// clearance walk the same chunks with the same buffers
struct SelfSweep {
  hfcl_scene* s = nullptr;
  SelfSweepPlan p;
  // the plan; the boxes of the configurations a chunk touches, a chunk's row arrays
  int ready(hfcl_scene* scene, size_t n_conf) {
    s = scene;
    hfcl_lib* lib = s->lib;
    const uint32_t n = uint32_t(s->n_objects);
    p = self_sweep_plan(n, n_conf, lib->opt.scene_pairs_small_max, lib->opt.scene_cull_chunk);
    HIP_TRY(lib->scene.d_boxes.grow(p.conf_per_chunk * n * 6));
    return pairs_chunk_buffers(lib, size_t(p.chunk_rows));
  }
  // what does not depend on the caller: inflate 0, no list
  void args(PairsArgs& a, size_t n_conf) const { pairs_args(a, s, p.geo, p.small, n_conf); }
  // the chunks in turn on st: a chunk's boxes, then launch() with a's chunk members set
  template <typename T, typename F>
  void walk(PairsArgs& a, const void* d_table, hipStream_t st, F&& launch) const {
    pairs_chunks<T>(a, s, d_table, p.geo, p.n_blocks, p.per, st, launch);
  }
};

// The same list by sort and sweep along one axis (option scene_pairs_sorted; hfcl_plan.hpp: sorted_sweep_plan, hfcl_k_pairs_sorted.hip):
// chunks of whole configurations on st.  Per chunk its boxes, the count half -- keys, sort, windows, count, scan --, the ONE wait: the
// entries so far (8 bytes) size the chunk's emitted words and their sort; then the emit half, unless the list is not asked for or the
// chunk lies behind its capacity.  the_list: the caller's part of the arguments, as the all-pairs sweep takes it.
template <typename T, typename F>
static int pairs_sorted_chunks(hfcl_scene* s, const void* d_table, size_t n_conf, hipStream_t st, F&& the_list) {
  hfcl_lib* lib = s->lib;
  hfcl_lib::SceneWs& w = lib->scene;
  const uint32_t n = uint32_t(s->n_objects);
  const SortedSweepPlan plan = sorted_sweep_plan(n, n_conf, lib->opt.scene_cull_chunk);
  const size_t rows = size_t(plan.chunk_rows);
  HIP_TRY(w.d_boxes.grow(rows * 6));
  int rc = pairs_chunk_buffers(lib, rows);
  if (rc) return rc;
  PairsSortedArgs a;
  pairs_args(a.p, s, pairs_geometry(n, false), false, n_conf);
  the_list(a.p);
  a.p.tile_groups = nullptr;
  a.p.g0 = 0;
  a.axis = lib->opt.scene_pairs_sorted_axis;
  a.blocks_per_conf = plan.blocks_per_conf;
  a.conf_bits = plan.conf_bits;
  a.obj_bits = plan.obj_bits;
  a.spread_blocks = (n + PSORT_SPREAD_BLOCK - 1u) / PSORT_SPREAD_BLOCK;
  for (int k = 0; k < 2; ++k) {
    HIP_TRY(w.d_ps_keys[k].grow(rows));
    HIP_TRY(w.d_ps_vals[k].grow(rows));
    a.keys[k] = w.d_ps_keys[k];
    a.vals[k] = w.d_ps_vals[k];
  }
  HIP_TRY(w.d_ps_boxes.grow(rows * 6));
  HIP_TRY(w.d_ps_ends.grow(rows));
  if (a.p.group) HIP_TRY(w.d_ps_group.grow(rows));
  if (a.axis >= PSORT_AXIS_AUTO) {
    HIP_TRY(w.d_ps_axis.grow(plan.conf_per_chunk));
    HIP_TRY(w.d_ps_spread.grow(plan.conf_per_chunk * a.spread_blocks * 6));
  }
  a.sorted_boxes = w.d_ps_boxes;
  a.ends = w.d_ps_ends;
  a.sorted_group = a.p.group ? w.d_ps_group.get() : nullptr;
  a.conf_axis = w.d_ps_axis;
  a.spread = w.d_ps_spread;
  a.emit[0] = a.emit[1] = nullptr;
  a.n_emit = a.emit_base = 0;
  uint64_t before = 0;
  for (size_t c0 = 0; c0 < n_conf; c0 += plan.conf_per_chunk) {
    const size_t confs = std::min(plan.conf_per_chunk, n_conf - c0);
    a.n_conf_chunk = uint32_t(confs);
    a.p.c_box0 = c0;
    a.p.n_blocks = uint32_t(confs * plan.blocks_per_conf);
    a.p.row0 = uint64_t(c0) * n;
    a.p.n_rows = uint32_t(confs * n);
    a.p.first = c0 == 0 ? 1 : 0;
    a.n_emit = 0;
    size_t bytes;
    HIP_TRY(pairs_sorted_temp_bytes(a, false, bytes));
    HIP_TRY(w.d_ps_temp.grow(std::max<size_t>(bytes, 16)));  // (never a null pointer: that would be the size query again)
    a.temp = w.d_ps_temp;
    a.temp_bytes = w.d_ps_temp.capacity();
    const char* table_rows = static_cast<const char*>(d_table) + c0 * n * SceneTypes<T>::WIDTH * sizeof(T);
    launch_cull_aabbs(st, table_rows, std::is_same<T, float>::value, s->d_object_shape, lib->d_local_boxes, n, confs * n, w.d_boxes);
    HIP_TRY(launch_pairs_sorted_count(st, a));
    uint64_t upto = 0;
    HIP_TRY(hipMemcpyAsync(&upto, w.d_running, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    a.n_emit = upto - before;
    a.emit_base = before;
    before = upto;
    if (!a.p.pairs || !a.n_emit || a.emit_base >= a.p.capacity) continue;
    for (int k = 0; k < 2; ++k) {
      HIP_TRY(w.d_ps_emit[k].grow(size_t(a.n_emit)));
      a.emit[k] = w.d_ps_emit[k];
    }
    HIP_TRY(pairs_sorted_temp_bytes(a, true, bytes));
    HIP_TRY(w.d_ps_temp.grow(std::max<size_t>(bytes, 16)));  // (never a null pointer: that would be the size query again)
    a.temp = w.d_ps_temp;
    a.temp_bytes = w.d_ps_temp.capacity();
    HIP_TRY(launch_pairs_sorted_emit(st, a));
  }
  return HFCL_OK;
}

// ---------------------------------------------------------------------------------------
// A static environment kept on the device (include/hppfcl_amd_env.h): what is its own of the pairs of the moving objects among themselves
// and against the environment per configuration (hfcl_scene_env_pairs*) -- the validator, the limits, the setter, the sweep.
// hfcl_k_env.hip has the kernels, hfcl_env.hpp the arithmetic.
// ---------------------------------------------------------------------------------------
// What every _env call refuses before any work, in this order: a null scene, a stale one, no environment, one of the other precision, a
// null table (with something to do), an overflow.  nothing: n_conf == 0 or no moving object -- HFCL_OK before the table is looked at.
template <typename T>
static int env_validate(const char* who, const hfcl_scene* s, const void* table, size_t n_conf, bool& nothing) {
  nothing = true;
  if (const int rc = groups_scene(who, s)) return rc;
  if (!s->has_env) {
    set_error(std::string(who) + ": the scene has no environment (hfcl_scene_set_environment)");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (s->env_f32 != std::is_same<T, float>::value) {
    set_error(std::string(who) + ": the environment was set in " + (s->env_f32 ? "fp32 (hfcl_scene_set_environment_f32)" : "fp64 (hfcl_scene_set_environment)") +
              ", this call is of the other precision; the two pose formats are not converted into each other");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (n_conf == 0 || s->n_moving == 0) return HFCL_OK;
  if (!table) {
    set_error(std::string(who) + ": null pose table");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (n_conf > ~size_t(0) / (s->n_moving * SceneTypes<T>::WIDTH * sizeof(T))) {
    set_error(std::string(who) + ": the pose table's size overflows");
    return HFCL_ERR_LIMIT;
  }
  nothing = false;
  return HFCL_OK;
}
// ... of a narrow-phase call: of a scene that is there, the request and the outputs first (scene_validate)
template <typename T>
static int env_scene_validate(const char* who, const hfcl_scene* s, const void* table, size_t n_conf, const hfcl_collision_request* creq,
                              const hfcl_distance_request* dreq, const void* out, const void* summary, bool& nothing) {
  nothing = true;
  const int rc = scene_request_and_outputs<T>(who, s, creq, dreq, out, summary);
  return rc ? rc : env_validate<T>(who, s, table, n_conf, nothing);
}
static int env_limits(const char* who, const hfcl_scene* s) {
  if (s->n_moving > ENV_MAX_OBJECTS || s->n_env() > ENV_MAX_OBJECTS) {
    set_error(std::string(who) + ": at most " + std::to_string(ENV_MAX_OBJECTS) + " moving objects and as many in the environment");
    return HFCL_ERR_LIMIT;
  }
  return HFCL_OK;
}
static int env_rank_limit(const char* who, uint64_t n_listed, const hfcl_scene* s) {
  if (env_shares(n_listed, s->n_moving, s->n_env()) > 0xFFFFFFFFull / SCENE_FOLD_SHARE) {
    set_error(std::string(who) + ": a configuration could hold 2^32 entries or more; summaries rank an entry in 32 bits");
    return HFCL_ERR_LIMIT;
  }
  return HFCL_OK;
}
// the groups present per column tile of a scene that has both groups and an environment (either may have been set last)
static int env_tile_groups(hfcl_scene* s) {
  s->d_env_tile_groups.reset();
  if (!s->has_env || !s->n_groups || s->n_moving > ENV_MAX_OBJECTS || s->n_env() > ENV_MAX_OBJECTS) return HFCL_OK;
  const EnvGeometry geo = env_geometry(uint32_t(s->n_moving), uint32_t(s->n_env()), 0u);
  std::vector<uint64_t> words(std::max<uint32_t>(geo.tiles, 1u), 0u);
  for (uint32_t u = 0; u < geo.tiles; ++u) words[u] = env_tile_word(geo, s->h_group.data(), u);
  return groups_upload(s->d_env_tile_groups, words.data(), words.size());
}

template <typename T>
static int env_set(const char* who, hfcl_scene* s, size_t n_moving, const T* env_rows) {
  int rc = groups_scene(who, s);
  if (rc) return rc;
  if (n_moving > s->n_objects) {
    set_error(std::string(who) + ": " + std::to_string(n_moving) + " moving objects in a scene of " + std::to_string(s->n_objects));
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  const size_t n_env = s->n_objects - n_moving;
  if (n_env && !env_rows) {
    set_error(std::string(who) + ": null environment poses");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (n_env > 0xFFFFFFFFull - PAIRS_TILE) {
    set_error(std::string(who) + ": too many environment objects");
    return HFCL_ERR_LIMIT;
  }
  hfcl_lib* lib = s->lib;
  HIP_TRY(hipSetDevice(lib->device));
  rc = ensure_local_boxes(lib);
  if (rc) return rc;
  DevBuf<void> d_table;
  DevBuf<double> d_boxes, d_tile_boxes, d_terms, d_tile_terms;
  if (n_env) {
    const size_t bytes = n_env * SceneTypes<T>::WIDTH * sizeof(T);
    HIP_TRY(d_table.grow(bytes));
    HIP_TRY(d_boxes.grow(n_env * 6));
    HIP_TRY(d_tile_boxes.grow(size_t(env_tiles(uint32_t(n_env))) * 6));
    HIP_TRY(d_terms.grow(n_env * 2));
    HIP_TRY(d_tile_terms.grow(size_t(env_tiles(uint32_t(n_env))) * 2));
    HIP_TRY(hipMemcpy(d_table, env_rows, bytes, hipMemcpyHostToDevice));
    // the boxes with the kernel of hfcl_scene_world_aabbs*: row r of this table is object n_moving + r
    launch_cull_aabbs(nullptr, d_table, std::is_same<T, float>::value, s->d_object_shape.get() + n_moving, lib->d_local_boxes, n_env, n_env, d_boxes);
    launch_env_tile_boxes(nullptr, d_boxes, uint32_t(n_env), d_tile_boxes);
    launch_nenv_terms(nullptr, d_boxes, uint32_t(n_env), d_terms, d_tile_terms);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(nullptr));
  }
  // (freeing the old tables waits for the device: a query in flight on some stream may still be reading them)
  s->d_env_table = std::move(d_table);
  s->d_env_boxes = std::move(d_boxes);
  s->d_env_tile_boxes = std::move(d_tile_boxes);
  s->d_env_terms = std::move(d_terms);
  s->d_env_tile_terms = std::move(d_tile_terms);
  s->has_env = true;
  s->env_f32 = std::is_same<T, float>::value;
  s->n_moving = n_moving;
  return env_tile_groups(s);
}

// The sweep of the moving rows of n_conf configurations against their own and the environment's columns, planned once (hfcl_plan.hpp:
// env_sweep_plan): the list maker and the clearance walk the same cells with the same buffers
struct EnvSweep {
  hfcl_scene* s = nullptr;
  EnvSweepPlan p;
  // the plan; the boxes of the moving rows of the configurations a chunk touches, a chunk's (row, span) arrays
  int ready(hfcl_scene* scene, size_t n_conf) {
    s = scene;
    hfcl_lib* lib = s->lib;
    const uint32_t nm = uint32_t(s->n_moving);
    p = env_sweep_plan(nm, uint32_t(s->n_env()), n_conf, lib->opt.scene_env_span, lib->n_cus, lib->opt.scene_cull_chunk);
    HIP_TRY(lib->scene.d_boxes.grow(p.conf_per_chunk * nm * 6));
    return pairs_chunk_buffers(lib, size_t(p.scan_rows));
  }
  // what does not depend on the caller: inflate 0, no list
  void args(EnvArgs& a, size_t n_conf) const {
    const uint32_t nm = p.geo.n_moving;
    pairs_args(a.p, s, p.rows, false, n_conf);
    a.p.tile_groups = nullptr;
    a.p.n_objects = nm * p.geo.n_spans;  // (the scan's rows: (row, span) counts, row-major)
    a.p.total_rows = uint64_t(n_conf) * nm * p.geo.n_spans;
    a.n_moving = nm;
    a.n_env = p.geo.n_env;
    a.tiles_moving = p.geo.tiles_moving;
    a.tiles = p.geo.tiles;
    a.span_len = p.geo.span_len;
    a.n_spans = p.geo.n_spans;
    a.blocks_per_conf = p.rows.blocks_per_conf;
    a.env_boxes = s->d_env_boxes;
    a.env_tile_boxes = s->d_env_tile_boxes;
    a.col_tile_groups = s->n_groups ? s->d_env_tile_groups.get() : nullptr;
  }
  // the chunks in turn on st: the boxes of a chunk's moving rows (the first n_moving objects' shapes), then launch() with a's chunk
  // members set -- the scan's rows are the chunk's rows times the spans
  template <typename T, typename F>
  void walk(EnvArgs& a, const void* d_table, hipStream_t st, F&& launch) const {
    pairs_chunks<T>(a.p, s, d_table, p.rows, p.n_blocks, p.per, st, [&]() {
      a.row0 = a.p.row0;
      a.p.row0 = a.row0 * p.geo.n_spans;
      a.p.n_rows = uint32_t(uint64_t(a.p.n_rows) * p.geo.n_spans);
      launch();
    });
  }
};

// ---------------------------------------------------------------------------------------
// A list of pairs made on the device, of either kind (ListKind::Self / ListKind::Env): what differs between the two, then the forms that
// are one for both -- the list into the library's workspace, the host form, the narrow phase on such a list.
// ---------------------------------------------------------------------------------------
// pose rows a configuration of the call's table has
static size_t pair_rows(const hfcl_scene* s, ListKind kind) { return kind == ListKind::Env ? s->n_moving : s->n_objects; }
static int pair_limits(const char* who, const hfcl_scene* s, ListKind kind) {
  return kind == ListKind::Env ? env_limits(who, s) : self_pairs_limits(who, s);
}
static int pair_rank_limit(const char* who, uint64_t n_listed, const hfcl_scene* s, ListKind kind) {
  return kind == ListKind::Env ? env_rank_limit(who, n_listed, s) : pairs_rank_limit(who, n_listed, s->n_objects);
}
// What a maker of such a list refuses of the scene and the table; nothing: the list is empty whatever the table holds -- n_conf == 0, or
// fewer than two objects (Self; a scene of ONE object still has its table refused when it is null) / no moving object (Env)
template <typename T>
static int pair_validate(ListKind kind, const char* who, const hfcl_scene* s, const void* table, size_t n_conf, bool& nothing) {
  if (kind == ListKind::Env) return env_validate<T>(who, s, table, n_conf, nothing);
  const int rc = self_validate<T>(who, s, table, n_conf);
  nothing = rc || n_conf == 0 || s->n_objects < 2;
  return rc;
}
// ... and a narrow-phase call on one: of a scene that is there, the request and the outputs first
template <typename T>
static int pair_scene_validate(ListKind kind, const char* who, const hfcl_scene* s, const void* table, size_t n_conf, const hfcl_collision_request* creq,
                               const hfcl_distance_request* dreq, const void* out, const void* summary, bool& nothing) {
  if (kind == ListKind::Env) return env_scene_validate<T>(who, s, table, n_conf, creq, dreq, out, summary, nothing);
  size_t total;
  const int rc = scene_validate<T>(who, s, table, n_conf, creq, dreq, out, summary, total, &hfcl_scene::n_objects);
  nothing = rc || n_conf == 0 || s->n_objects < 2;
  return rc;
}
// The list of the whole table on st (hfcl_scene_self_pairs_device*, hfcl_scene_env_pairs_device*): the pairs (below `capacity`),
// conf_begin, the count.  Nothing is read back.
template <typename T>
static int pairs_device(ListKind kind, const char* who, hfcl_scene* s, const void* d_table, size_t n_conf, double inflate, uint32_t* d_pairs,
                        size_t capacity, uint64_t* d_conf_begin, uint64_t* d_n_listed, hipStream_t st) {
  bool nothing;
  int rc = pair_validate<T>(kind, who, s, d_table, n_conf, nothing);
  if (rc) return rc;
  rc = cull_check_inflate(who, inflate);
  if (rc) return rc;
  if (!d_n_listed) {
    set_error(std::string(who) + ": null count");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  rc = pair_limits(who, s, kind);
  if (rc) return rc;
  hfcl_lib* lib = s->lib;
  HIP_TRY(hipSetDevice(lib->device));
  if (nothing) {  // no pair: an empty list
    HIP_TRY(hipMemsetAsync(d_n_listed, 0, sizeof(uint64_t), st));
    if (d_conf_begin) HIP_TRY(hipMemsetAsync(d_conf_begin, 0, (n_conf + 1) * sizeof(uint64_t), st));
    return HFCL_OK;
  }
  rc = ensure_local_boxes(lib);
  if (rc) return rc;
  auto the_list = [&](PairsArgs& p) {  // the caller's part of a sweep's arguments
    p.inflate = inflate;
    p.pairs = d_pairs;
    p.capacity = d_pairs ? capacity : 0;
    p.conf_begin = d_conf_begin;
    p.n_listed = d_n_listed;
  };
  if (kind == ListKind::Env) {
    EnvSweep sweep;
    rc = sweep.ready(s, n_conf);
    if (rc) return rc;
    EnvArgs a;
    sweep.args(a, n_conf);
    the_list(a.p);
    sweep.walk<T>(a, d_table, st, [&]() { launch_env_chunk(st, a); });
  } else if (lib->opt.scene_pairs_sorted) {  // the same list by sort and sweep: waits on st once per chunk
    rc = pairs_sorted_chunks<T>(s, d_table, n_conf, st, the_list);
    if (rc) return rc;
    s->last_pairs_form = 2;
  } else {
    SelfSweep sweep;
    rc = sweep.ready(s, n_conf);
    if (rc) return rc;
    PairsArgs a;
    sweep.args(a, n_conf);
    the_list(a);
    sweep.walk<T>(a, d_table, st, [&]() { launch_pairs_chunk(st, a); });
    s->last_pairs_form = sweep.p.small ? 1 : 0;
  }
  HIP_TRY(hipGetLastError());
  return HFCL_OK;
}

// entries a list of pairs of `rows` rows is first given room for (a longer one is made again in a buffer of its size)
static size_t pairs_capacity_guess(size_t rows) { return std::max<size_t>(16 * rows, 4096); }
// The list of a table that is on the device into the library's own (w.d_pair_list, w.d_conf_begin), and the one read-back: the count.
template <typename T>
static int pairs_into_workspace(ListKind kind, const char* who, hfcl_scene* s, const void* d_table, size_t n_conf, double inflate, bool want_pairs,
                                uint64_t& n_listed) {
  hfcl_lib* lib = s->lib;
  hfcl_lib::SceneWs& w = lib->scene;
  HIP_TRY(w.d_conf_begin.grow(n_conf + 1));
  HIP_TRY(w.d_running.grow(2));
  if (want_pairs) HIP_TRY(w.d_pair_list.grow(2 * pairs_capacity_guess(n_conf * pair_rows(s, kind))));
  return list_and_count(w.d_pair_list, want_pairs, w.d_running + 1, w.s_cmp, n_listed, [&]() {
    return pairs_device<T>(kind, who, s, d_table, n_conf, inflate, want_pairs ? w.d_pair_list.get() : nullptr, w.d_pair_list.capacity() / 2,
                           w.d_conf_begin, w.d_running + 1, w.s_cmp);
  }, 2);
}

template <typename T>
static int pairs_host(ListKind kind, const char* who, hfcl_scene* s, const void* table, size_t n_conf, double inflate, uint32_t* pairs,
                      size_t capacity, uint64_t* conf_begin, size_t* n_listed) {
  bool nothing;
  int rc = pair_validate<T>(kind, who, s, table, n_conf, nothing);
  if (!rc) rc = cull_check_inflate(who, inflate);
  if (!rc && !n_listed) {
    set_error(std::string(who) + ": null count");
    rc = HFCL_ERR_INVALID_ARGUMENT;
  }
  if (!rc) rc = pair_limits(who, s, kind);
  if (rc) return rc;
  *n_listed = 0;
  if (nothing) {
    if (conf_begin) memset(conf_begin, 0, (n_conf + 1) * sizeof(uint64_t));
    return HFCL_OK;
  }
  hfcl_lib* lib = s->lib;
  hfcl_lib::SceneWs& w = lib->scene;
  HIP_TRY(hipSetDevice(lib->device));
  rc = scene_host_stream(w);
  if (!rc) rc = scene_table_in(w, table, n_conf * pair_rows(s, kind) * SceneTypes<T>::WIDTH * sizeof(T));
  uint64_t n = 0;
  if (!rc) rc = pairs_into_workspace<T>(kind, who, s, w.d_table, n_conf, inflate, pairs != nullptr, n);
  if (rc) {
    hipStreamSynchronize(w.s_cmp);
    return rc;
  }
  *n_listed = size_t(n);
  if (pairs && capacity < n) {
    set_error(std::string(who) + ": " + std::to_string(n) + " pairs are listed, the list holds " + std::to_string(capacity));
    return HFCL_ERR_LIMIT;
  }
  if (pairs && n) HIP_TRY(hipMemcpyAsync(pairs, w.d_pair_list, n * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, w.s_cmp));
  if (conf_begin) HIP_TRY(hipMemcpyAsync(conf_begin, w.d_conf_begin, (n_conf + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, w.s_cmp));
  HIP_TRY(hipStreamSynchronize(w.s_cmp));
  return HFCL_OK;
}

// The device form on a list of pairs.  The list is not checked: i < j < n_objects (Env: i < n_moving), conf_begin its spans -- as
// hfcl_scene_self_pairs_device / hfcl_scene_env_pairs_device leave them.  counts: as scene_chunks_device takes them.
// Kept as the two were: with configurations but no pose row, a Self call returns here, an Env call goes on to the summary init.
template <typename T>
static int scene_pairs_device(ListKind kind, const char* who, hfcl_scene* s, const void* d_table, size_t n_conf, const uint32_t* d_pairs,
                              size_t n_listed, const uint64_t* d_conf_begin, const hfcl_collision_request* creq, const hfcl_distance_request* dreq,
                              typename SceneTypes<T>::R* d_out, hfcl_scene_summary* d_summary, const hfcl_guess* d_gin, hfcl_guess* d_gout,
                              hipStream_t st, SceneCountSlots* counts = nullptr) {
  bool nothing;
  int rc = pair_scene_validate<T>(kind, who, s, d_table, n_conf, creq, dreq, d_out, d_summary, nothing);
  if (rc) return rc;
  if (n_conf == 0 || pair_rows(s, kind) == 0) {
    if (n_listed) {
      set_error(std::string(who) + ": list entries without a configuration or " + (kind == ListKind::Env ? "a moving object" : "an object"));
      return HFCL_ERR_INVALID_ARGUMENT;
    }
    if (n_conf == 0 || kind == ListKind::Self) return HFCL_OK;
  }
  if (n_listed && (!d_pairs || !d_conf_begin)) {
    set_error(std::string(who) + ": null list / conf_begin");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (d_summary && (rc = pair_rank_limit(who, n_listed, s, kind))) return rc;
  hfcl_lib* lib = s->lib;
  HIP_TRY(hipSetDevice(lib->device));
  if (d_summary) launch_scene_summary_init(st, d_summary, n_conf, lib->n_cus * 16);
  if (!n_listed) {
    HIP_TRY(hipGetLastError());
    return HFCL_OK;
  }
  const SceneList list = pair_list(s, kind, d_pairs, d_conf_begin, n_conf, n_listed);
  return scene_chunks_device<T>(s, d_table, &list, n_listed, creq, dreq, d_out, d_summary, d_gin, d_gout, st, counts);
}

// What the culled host forms add to scene_host.  kind: Culled (hfcl_scene_*_culled): the list is culled from the scene's own, its ids to
// query_ids_out; Self / Env (hfcl_scene_*_self / _env): the list is made by pairs_into_workspace, its pairs to pairs_out -- Env from a
// table of the moving objects alone
struct SceneCull {
  ListKind kind;
  double inflate;
  size_t out_capacity;
  uint64_t* query_ids_out;   // Culled: nullptr or out_capacity
  uint32_t* pairs_out;       // Self, Env: nullptr or 2 x out_capacity
  uint64_t* conf_begin_out;  // nullptr or n_conf + 1
  size_t* n_listed;
};

// Host form.  The object table goes in once; chunk k computes on one stream while chunk k - 1's records leave on another from the other of
// two record buffers (the copy is issued AFTER chunk k's launches: a copy into pageable memory holds its caller until the data has moved);
// the summaries come back once at the end.  No feeder threads: nothing per pair goes in.
template <typename T>
static int scene_host(const char* who, hfcl_scene* s, const void* table, size_t n_conf, const hfcl_collision_request* creq,
                      const hfcl_distance_request* dreq, typename SceneTypes<T>::R* out, hfcl_scene_summary* summary, const hfcl_guess* gin,
                      hfcl_guess* gout, const SceneCull* cull = nullptr) {
  using R = typename SceneTypes<T>::R;
  size_t total = 0;
  const bool made = cull && cull->kind != ListKind::Culled;  // the list is made from the table's rows, not culled from the scene's own
  int rc;
  if (made) {
    bool nothing;
    rc = pair_scene_validate<T>(cull->kind, who, s, table, n_conf, creq, dreq, out, summary, nothing);
    if (!rc) rc = pair_limits(who, s, cull->kind);
    if (!rc) total = nothing ? 0 : n_conf * pair_rows(s, cull->kind);  // (rows: what the list is made from)
  } else {
    rc = scene_validate<T>(who, s, table, n_conf, creq, dreq, out, summary, total);
  }
  if (!rc && cull) {
    rc = cull_check_inflate(who, cull->inflate);
    if (!rc && !cull->n_listed) {
      set_error(std::string(who) + ": null count");
      rc = HFCL_ERR_INVALID_ARGUMENT;
    }
    if (!rc) *cull->n_listed = 0;
  }
  auto nothing_listed = [&]() {  // no surviving query: an empty list, the summaries of configurations without records
    if (cull->conf_begin_out) memset(cull->conf_begin_out, 0, (n_conf + 1) * sizeof(uint64_t));
    for (size_t c = 0; summary && c < n_conf; ++c) scene_summary_init(summary[c]);
    return HFCL_OK;
  };
  if (!rc && !total && cull) return nothing_listed();
  if (rc || !total) return rc;
  hfcl_lib* lib = s->lib;
  hfcl_lib::SceneWs& w = lib->scene;
  HIP_TRY(hipSetDevice(lib->device));
  if (!w.s_cmp) HIP_TRY(w.s_cmp.create());
  if (!w.s_copy) HIP_TRY(w.s_copy.create());
  for (int k = 0; k < 2; ++k) {
    if (!w.ev_done[k]) HIP_TRY(w.ev_done[k].create());
    if (!w.ev_copied[k]) HIP_TRY(w.ev_copied[k].create());
  }
  const size_t table_bytes = n_conf * (made ? pair_rows(s, cull->kind) : s->n_objects) * SceneTypes<T>::WIDTH * sizeof(T);
  size_t work = total;  // records of the call: every query, or (culled form) the surviving ones
  if (cull) {  // the table goes in, the cull runs, the count comes back: 8 bytes, the one read-back before the narrow phase
    rc = scene_table_in(w, table, table_bytes);
    uint64_t n = 0;
    if (!rc)
      rc = made ? pairs_into_workspace<T>(cull->kind, who, s, w.d_table, n_conf, cull->inflate, true, n)
                : cull_into_workspace<T>(who, s, w.d_table, n_conf, total, cull->inflate, true, n);
    if (rc) {
      hipStreamSynchronize(w.s_cmp);
      return rc;
    }
    *cull->n_listed = size_t(n);
    if ((out || gout || cull->query_ids_out || cull->pairs_out) && cull->out_capacity < n) {
      set_error(std::string(who) + ": " + std::to_string(n) + " queries survive, the outputs hold " + std::to_string(cull->out_capacity));
      return HFCL_ERR_LIMIT;
    }
    if (!n) return nothing_listed();
    if (made && summary && (rc = pair_rank_limit(who, n, s, cull->kind))) return rc;
    if (cull->query_ids_out) HIP_TRY(hipMemcpyAsync(cull->query_ids_out, w.d_ids, n * sizeof(uint64_t), hipMemcpyDeviceToHost, w.s_cmp));
    if (cull->pairs_out) HIP_TRY(hipMemcpyAsync(cull->pairs_out, w.d_pair_list, n * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, w.s_cmp));
    if (cull->conf_begin_out)
      HIP_TRY(hipMemcpyAsync(cull->conf_begin_out, w.d_conf_begin, (n_conf + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, w.s_cmp));
    work = size_t(n);
  }
  const SceneList listed = made ? pair_list(s, cull->kind, w.d_pair_list, w.d_conf_begin, n_conf, work) : query_list(w.d_ids, w.d_conf_begin, n_conf);
  const SceneList* list = cull ? &listed : nullptr;
  const size_t chunk = scene_chunk_size(work, lib->opt.scene_chunk);
  const size_t n_chunks = (work + chunk - 1) / chunk;
  const bool back = out != nullptr || gout != nullptr;  // something per pair goes back: two buffers, the copy stream
  rc = scene_workspace(lib, chunk, out ? 2 : 1, gin != nullptr, gout ? 2 : 0, summary ? scene_pieces(s, list, chunk) : 0);
  if (rc) return rc;
  if (!cull) HIP_TRY(w.d_table.grow(table_bytes));
  if (summary) HIP_TRY(w.d_summary.grow(n_conf));
  rc = SceneCountSlots::ready(w);
  if (rc) return rc;
  SceneCountSlots counts(lib);  // (ends after finish, or the tail, has waited for the streams)

  auto finish = [&](int code) {  // nothing of this call stays in flight, whatever happened
    hipStreamSynchronize(w.s_cmp);
    hipStreamSynchronize(w.s_copy);
    if (lib->side) hipStreamSynchronize(lib->side);
    return code;
  };
#define SCENE_TRY(expr)                                                      \
  do {                                                                       \
    hipError_t _e = (expr);                                                  \
    if (_e != hipSuccess) {                                                  \
      set_error(std::string(#expr) + ": " + hipGetErrorString(_e));          \
      return finish(HFCL_ERR_HIP);                                           \
    }                                                                        \
  } while (0)
  // which of the two record / guess buffers chunk k computes into while chunk k - 1's leave from the other (one buffer: nothing goes back)
  auto buffer_of = [&](size_t k) { return back ? int(k & 1) : 0; };
  auto copy_back = [&](size_t k) -> hipError_t {  // chunk k's records (and guesses) to the caller's arrays, behind its kernels
    const int b = buffer_of(k);
    const size_t q0 = k * chunk, m = std::min(chunk, work - q0);
    hipError_t e = hipStreamWaitEvent(w.s_copy, w.ev_done[b], 0);
    if (e == hipSuccess && out) e = hipMemcpyAsync(out + q0, w.d_rec[b], m * sizeof(R), hipMemcpyDeviceToHost, w.s_copy);
    if (e == hipSuccess && gout) e = hipMemcpyAsync(gout + q0, w.d_gout[b], m * sizeof(hfcl_guess), hipMemcpyDeviceToHost, w.s_copy);
    if (e == hipSuccess) e = hipEventRecord(w.ev_copied[b], w.s_copy);
    return e;
  };

  if (!cull) SCENE_TRY(hipMemcpyAsync(w.d_table, table, table_bytes, hipMemcpyHostToDevice, w.s_cmp));
  if (cull && summary) launch_scene_summary_init(w.s_cmp, w.d_summary, n_conf, lib->n_cus * 16);
  for (size_t k = 0; k < n_chunks; ++k) {
    const int b = buffer_of(k);
    const size_t q0 = k * chunk, m = std::min(chunk, work - q0);
    if (back && k >= 2) SCENE_TRY(hipStreamWaitEvent(w.s_cmp, w.ev_copied[b], 0));  // chunk k - 2 has left the buffers
    if (gin) SCENE_TRY(hipMemcpyAsync(w.d_gin, gin + q0, m * sizeof(hfcl_guess), hipMemcpyHostToDevice, w.s_cmp));
    rc = counts.before_chunk(m);
    if (!rc)
      rc = scene_chunk_run<T>(s, w.d_table, list, q0, m, creq, dreq, static_cast<R*>(w.d_rec[out ? b : 0].get()), summary ? w.d_summary : nullptr,
                              gin ? w.d_gin : nullptr, gout ? w.d_gout[b] : nullptr, w.s_cmp);
    if (!rc) rc = counts.after_chunk(w.s_cmp);
    if (rc) return finish(rc);
    if (back) {
      SCENE_TRY(hipEventRecord(w.ev_done[b], w.s_cmp));
      if (k >= 1) SCENE_TRY(copy_back(k - 1));
    }
  }
  if (back) SCENE_TRY(copy_back(n_chunks - 1));
  if (summary) SCENE_TRY(hipMemcpyAsync(summary, w.d_summary, n_conf * sizeof(hfcl_scene_summary), hipMemcpyDeviceToHost, w.s_cmp));
  SCENE_TRY(hipStreamSynchronize(w.s_cmp));
  SCENE_TRY(hipStreamSynchronize(w.s_copy));
  SCENE_TRY(hipGetLastError());
#undef SCENE_TRY
  counts.harvest_rest();
  lib->last_host = true;
  return host_batch_checks(lib, creq, dreq);
}

// ---------------------------------------------------------------------------------------
// The per-configuration minimum distance with box-bound pruning (include/hppfcl_amd_nearest.h: hfcl_scene_nearest*).  hfcl_k_nearest.hip has
// the kernels, hfcl_nearest.hpp the arithmetic.  The boxes of the whole table once; the seeds; the list of pass 1 (mark / scan / emit), its
// count read back, its narrow phase through scene_listed_device; the thresholds; the same for pass 2, merged into the same summaries; the
// min records gathered.  Two read-backs of 8 bytes.
// ---------------------------------------------------------------------------------------
// What the three families of pruned-clearance calls (nearest, nearest_self, nearest_env) refuse first, in this order: a NaN bound; of a
// scene that is there a null request, a null output -- in the family's words, no_out -- and the request's own checks.  A null scene is
// the family's validator's to refuse, after this.
template <typename T>
static int nearest_head(const char* who, const hfcl_scene* s, const hfcl_distance_request* req, double upper, const void* out, const char* no_out) {
  if (upper != upper) {
    set_error(std::string(who) + ": upper_bound is NaN");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (!s) return HFCL_OK;
  if (!req) {
    set_error("null request");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (!out) {
    set_error(std::string(who) + ": " + no_out);
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  QParams<T> q;
  return setup_distance<T>(req, q);
}
template <typename T>
static int nearest_validate(const char* who, const hfcl_scene* s, const void* table, size_t n_conf, const hfcl_distance_request* req, double upper,
                            const void* summary, size_t& total) {
  total = 0;
  const int rc = nearest_head<T>(who, s, req, upper, summary, "null summaries");
  return rc ? rc : scene_validate<T>(who, s, table, n_conf, nullptr, req, nullptr, summary, total);  // (the request's checks once more: they passed)
}

// The host shell of the three families once there is something to do: the stream, the output (d_out: the library's buffer of the family's
// per-configuration output) and min-record buffers, the count slots, the table of n_conf x rows pose rows in, run(d_table, d_out, d_min,
// counts, st) -- the family's *_run --, the outputs back, nothing left in flight, the tail of a host form.
// (scene_host has a shell of its own: two streams, and a finish that waits for both and does not harvest.)
template <typename T, typename Out, typename Run>
static int nearest_host_shell(const char* who, hfcl_scene* s, const void* table, size_t rows, size_t n_conf, const hfcl_distance_request* req,
                              DevBuf<Out>& d_out, Out* out, typename SceneTypes<T>::R* min_records, Run&& run) {
  using R = typename SceneTypes<T>::R;
  hfcl_lib* lib = s->lib;
  hfcl_lib::SceneWs& w = lib->scene;
  HIP_TRY(hipSetDevice(lib->device));
  int rc = scene_host_stream(w);
  if (rc) return rc;
  HIP_TRY(d_out.grow(n_conf));
  if (min_records) HIP_TRY(w.d_minrec.grow(n_conf * sizeof(R)));
  rc = SceneCountSlots::ready(w);
  if (rc) return rc;
  SceneCountSlots counts(lib);  // (ends after finish has waited for the streams)
  auto finish = [&](int code) {  // nothing of this call stays in flight, whatever happened
    const bool synced = hipStreamSynchronize(w.s_cmp) == hipSuccess;
    if (lib->side) hipStreamSynchronize(lib->side);
    if (code == HFCL_OK && synced) counts.harvest_rest();
    if (code == HFCL_OK && !synced) {
      set_error(std::string(who) + ": the device reported an error");
      return int(HFCL_ERR_HIP);
    }
    return code;
  };
  rc = scene_table_in(w, table, n_conf * rows * SceneTypes<T>::WIDTH * sizeof(T));
  if (!rc) rc = run(w.d_table.get(), d_out.get(), min_records ? static_cast<R*>(w.d_minrec.get()) : nullptr, &counts, w.s_cmp.get());
  if (!rc && hipMemcpyAsync(out, d_out, n_conf * sizeof(Out), hipMemcpyDeviceToHost, w.s_cmp) != hipSuccess) rc = HFCL_ERR_HIP;
  if (!rc && min_records && hipMemcpyAsync(min_records, w.d_minrec, n_conf * sizeof(R), hipMemcpyDeviceToHost, w.s_cmp) != hipSuccess)
    rc = HFCL_ERR_HIP;
  rc = finish(rc);
  if (rc) return rc;
  lib->last_host = true;
  return host_batch_checks(lib, nullptr, req);
}

// table on the device, total > 0, everything on st (which is waited for twice)
template <typename T>
static int nearest_run(const char* who, hfcl_scene* s, const void* d_table, size_t n_conf, size_t total, const hfcl_distance_request* req,
                       double upper, hfcl_scene_summary* d_summary, typename SceneTypes<T>::R* d_min, size_t* n_evaluated, SceneCountSlots* counts,
                       hipStream_t st) {
  using R = typename SceneTypes<T>::R;
  constexpr bool f32 = std::is_same<T, float>::value;
  hfcl_lib* lib = s->lib;
  hfcl_lib::SceneWs& w = lib->scene;
  const int max_blocks = lib->n_cus * 16;
  int rc = ensure_local_boxes(lib);
  if (rc) return rc;
  const size_t chunk = cull_chunk_size(total, lib->opt.scene_cull_chunk);
  const uint32_t shares = scene_shares(uint32_t(s->n_pairs));
  rc = cull_chunk_buffers(lib, chunk);
  if (rc) return rc;
  HIP_TRY(w.d_boxes.grow(n_conf * s->n_objects * 6));
  HIP_TRY(w.d_conf_begin.grow(n_conf + 1));
  HIP_TRY(w.d_conf_begin2.grow(n_conf + 1));
  HIP_TRY(w.d_seed.grow(n_conf));
  HIP_TRY(w.d_thr.grow(n_conf));
  if (shares > 1u) HIP_TRY(w.d_seed_partials.grow(n_conf * shares * sizeof(NearestSeed)));
  HIP_TRY(w.d_ids.grow(list_capacity_guess(total)));
  HIP_TRY(w.d_ids2.grow(list_capacity_guess(total)));

  launch_cull_aabbs(st, d_table, f32, s->d_object_shape, lib->d_local_boxes, s->n_objects, n_conf * s->n_objects, w.d_boxes);
  NearestArgs a{};
  cull_args(a.c, s, total, n_conf, 0.0, w.d_running + 1);
  a.c.c_box0 = 0;
  a.r = f32 ? NEAREST_R32 : NEAREST_R64;
  a.upper = upper;
  a.seed = w.d_seed;
  a.seed_partials = shares > 1u ? w.d_seed_partials.get() : nullptr;
  a.thr = w.d_thr;
  launch_nearest_seed(st, a, max_blocks);

  // the list of a pass into ids / conf_begin, and the one read-back: its count
  auto compact = [&](int pass, DevBuf<uint64_t>& ids, uint64_t* conf_begin, uint64_t& n) -> int {
    return list_and_count(ids, true, w.d_running + 1, st, n, [&]() {
      a.c.ids = ids;
      a.c.capacity = ids.capacity();
      a.c.conf_begin = conf_begin;
      cull_chunks(a.c, chunk, [&]() { launch_nearest_chunk(st, a, pass); });
      return int(HFCL_OK);
    });
  };
  uint64_t n_list[2] = {0, 0};
  DevBuf<uint64_t>* ids[2] = {&w.d_ids, &w.d_ids2};
  uint64_t* conf_begin[2] = {w.d_conf_begin, w.d_conf_begin2};
  for (int pass = 1; pass <= 2; ++pass) {
    const int l = pass - 1;
    if (pass == 2) launch_nearest_threshold(st, a, d_summary);
    rc = compact(pass, *ids[l], conf_begin[l], n_list[l]);
    if (rc) return rc;
    if (d_min) HIP_TRY(w.d_nrec[l].grow(size_t(n_list[l]) * sizeof(R)));
    rc = scene_listed_device<T>(who, s, d_table, n_conf, ids[l]->get(), size_t(n_list[l]), conf_begin[l], nullptr, req,
                                d_min ? static_cast<R*>(w.d_nrec[l].get()) : nullptr, d_summary, nullptr, nullptr, st, pass == 2, counts);
    if (rc) return rc;
  }
  if (d_min) {
    NearestGatherArgs g;
    g.summary = d_summary;
    g.n_conf = n_conf;
    g.n_pairs = uint32_t(s->n_pairs);
    for (int l = 0; l < 2; ++l) {
      g.ids[l] = ids[l]->get();
      g.conf_begin[l] = conf_begin[l];
      g.rec[l] = w.d_nrec[l].get();
    }
    g.out = d_min;
    launch_nearest_gather(st, g, f32);
  }
  if (n_evaluated) {
    n_evaluated[0] = size_t(n_list[0]);
    n_evaluated[1] = size_t(n_list[1]);
  }
  HIP_TRY(hipGetLastError());
  return HFCL_OK;
}

template <typename T>
static int nearest_device(const char* who, hfcl_scene* s, const void* d_table, size_t n_conf, const hfcl_distance_request* req, double upper,
                          hfcl_scene_summary* d_summary, typename SceneTypes<T>::R* d_min, size_t* n_evaluated, hipStream_t st) {
  size_t total;
  const int rc = nearest_validate<T>(who, s, d_table, n_conf, req, upper, d_summary, total);
  if (rc) return rc;
  if (n_evaluated) n_evaluated[0] = n_evaluated[1] = 0;
  if (!n_conf) return HFCL_OK;
  hfcl_lib* lib = s->lib;
  HIP_TRY(hipSetDevice(lib->device));
  if (!total) {  // no query: every configuration is one without records
    launch_scene_summary_init(st, d_summary, n_conf, lib->n_cus * 16);
    if (d_min) {
      NearestGatherArgs g = {};
      g.summary = d_summary;
      g.n_conf = n_conf;
      g.out = d_min;
      launch_nearest_gather(st, g, std::is_same<T, float>::value);
    }
    HIP_TRY(hipGetLastError());
    return HFCL_OK;
  }
  return nearest_run<T>(who, s, d_table, n_conf, total, req, upper, d_summary, d_min, n_evaluated, nullptr, st);
}

template <typename T>
static int nearest_host(const char* who, hfcl_scene* s, const void* table, size_t n_conf, const hfcl_distance_request* req, double upper,
                        hfcl_scene_summary* summary, typename SceneTypes<T>::R* min_records, size_t* n_evaluated) {
  using R = typename SceneTypes<T>::R;
  size_t total;
  int rc = nearest_validate<T>(who, s, table, n_conf, req, upper, summary, total);
  if (rc) return rc;
  if (n_evaluated) n_evaluated[0] = n_evaluated[1] = 0;
  if (!total) {
    for (size_t c = 0; c < n_conf; ++c) {
      scene_summary_init(summary[c]);
      if (min_records) {
        memset(&min_records[c], 0, sizeof(R));
        nearest_no_record(min_records[c]);
      }
    }
    return HFCL_OK;
  }
  return nearest_host_shell<T>(who, s, table, s->n_objects, n_conf, req, s->lib->scene.d_summary, summary, min_records,
                               [&](const void* d_table, hfcl_scene_summary* d_summary, R* d_min, SceneCountSlots* counts, hipStream_t st) {
                                 return nearest_run<T>(who, s, d_table, n_conf, total, req, upper, d_summary, d_min, n_evaluated, counts, st);
                               });
}

// ---------------------------------------------------------------------------------------
// The clearance per configuration on device-made pairs (include/hppfcl_amd_nearest_self.h: hfcl_scene_nearest_self*).
// hfcl_k_nearest_self.hip has the kernels, hfcl_nearest_self.hpp the arithmetic.  Five walks of the all-pairs sweep (SelfSweep: the chunks
// of the list maker, the boxes made per chunk): the seeds; count and emit of pass 1, its count read back, its narrow phase through
// scene_pairs_device into summaries of its own; the thresholds; the same for pass 2; the two combined (clearance_passes).  Two read-backs
// of 8 bytes.  The clearance among a kept environment (hfcl_scene_nearest_env*) is the same over EnvSweep; the validator, the device form
// and the host form are one for both (clearance_validate / _device / _host).
// ---------------------------------------------------------------------------------------
// What the two passes keep per configuration, whatever sweeps: seeds and thresholds, and per pass conf_begin, summaries and a list with
// first room for the entries of `rows` rows
static int clearance_buffers(hfcl_lib::SceneWs& w, size_t n_conf, size_t rows) {
  HIP_TRY(w.d_ns_seed.grow(n_conf));
  HIP_TRY(w.d_ns_thr.grow(n_conf));
  for (int l = 0; l < 2; ++l) {
    HIP_TRY(w.d_ns_conf_begin[l].grow(n_conf + 1));
    HIP_TRY(w.d_ns_summary[l].grow(n_conf));
    HIP_TRY(w.d_ns_list[l].grow(2 * pairs_capacity_guess(rows)));
  }
  return HFCL_OK;
}
// the clearance and the min record of n_conf configurations from the two passes' lists (nullptr: every configuration is one without records)
static void clearance_combine(hfcl_lib::SceneWs* w, size_t n_conf, hfcl_scene_clearance* d_out, void* d_min, bool f32, hipStream_t st) {
  NselfCombineArgs g{};
  g.n_conf = n_conf;
  for (int l = 0; w && l < 2; ++l) {
    g.summary[l] = w->d_ns_summary[l];
    g.pairs[l] = w->d_ns_list[l];
    g.conf_begin[l] = w->d_ns_conf_begin[l];
    g.rec[l] = d_min ? w->d_ns_rec[l].get() : nullptr;
  }
  g.out = d_out;
  g.min_out = d_min;
  launch_nself_combine(st, g, f32);
}
// The two passes of a clearance call on st, the seeds made: per pass the thresholds (pass 2: thr[c] = min(D, min_distance of pass 1)), the
// pass's list -- list_chunks() walks the family's sweep with `pass`, and `p`'s list members, set --, its count read back, the rank limit,
// its narrow phase through scene_pairs_device into summaries of its own; then the two combined.  Two read-backs of 8 bytes.
// (hfcl_scene_nearest's nearest_run is the same skeleton on ids: its lists go through scene_listed_device, pass 2 merged into the
// summaries of pass 1, and a gather ends it.)
template <typename T, typename Walk>
static int clearance_passes(ListKind kind, const char* who, hfcl_scene* s, const void* d_table, size_t n_conf, const hfcl_distance_request* req,
                            double upper, PairsArgs& p, int& pass_of_args, Walk&& list_chunks, hfcl_scene_clearance* d_out,
                            typename SceneTypes<T>::R* d_min, size_t* n_evaluated, SceneCountSlots* counts, hipStream_t st) {
  using R = typename SceneTypes<T>::R;
  hfcl_lib::SceneWs& w = s->lib->scene;
  uint64_t n_list[2] = {0, 0};
  for (int pass = 1; pass <= 2; ++pass) {
    const int l = pass - 1;
    if (pass == 2) {
      NearestArgs t{};
      t.c.n_conf = n_conf;
      t.upper = upper;
      t.thr = w.d_ns_thr;
      launch_nearest_threshold(st, t, w.d_ns_summary[0]);
    }
    pass_of_args = pass;
    p.conf_begin = w.d_ns_conf_begin[l];
    p.n_listed = w.d_running + 1;
    int rc = list_and_count(w.d_ns_list[l], true, w.d_running + 1, st, n_list[l], [&]() {
      p.pairs = w.d_ns_list[l];
      p.capacity = w.d_ns_list[l].capacity() / 2;
      list_chunks();
      return int(HFCL_OK);
    }, 2);
    if (!rc) rc = pair_rank_limit(who, n_list[l], s, kind);
    if (rc) return rc;
    if (d_min) HIP_TRY(w.d_ns_rec[l].grow(size_t(n_list[l]) * sizeof(R)));
    rc = scene_pairs_device<T>(kind, who, s, d_table, n_conf, w.d_ns_list[l], size_t(n_list[l]), w.d_ns_conf_begin[l], nullptr, req,
                               d_min ? static_cast<R*>(w.d_ns_rec[l].get()) : nullptr, w.d_ns_summary[l], nullptr, nullptr, st, counts);
    if (rc) return rc;
  }
  clearance_combine(&w, n_conf, d_out, d_min, std::is_same<T, float>::value, st);
  if (n_evaluated) {
    n_evaluated[0] = size_t(n_list[0]);
    n_evaluated[1] = size_t(n_list[1]);
  }
  HIP_TRY(hipGetLastError());
  return HFCL_OK;
}

// table on the device, n_conf > 0, at least two objects, everything on st (which is waited for twice)
template <typename T>
static int nearest_self_run(const char* who, hfcl_scene* s, const void* d_table, size_t n_conf, const hfcl_distance_request* req, double upper,
                            hfcl_scene_clearance* d_out, typename SceneTypes<T>::R* d_min, size_t* n_evaluated, SceneCountSlots* counts,
                            hipStream_t st) {
  hfcl_lib* lib = s->lib;
  hfcl_lib::SceneWs& w = lib->scene;
  int rc = ensure_local_boxes(lib);
  if (rc) return rc;
  SelfSweep sweep;
  rc = sweep.ready(s, n_conf);
  if (rc) return rc;
  const bool small = sweep.p.small;
  const size_t rows = n_conf * s->n_objects;
  if (!small) HIP_TRY(w.d_ns_row_seeds.grow(rows * sizeof(NselfRowSeed)));
  rc = clearance_buffers(w, n_conf, rows);
  if (rc) return rc;
  NselfArgs a{};
  sweep.args(a.p, n_conf);
  a.r = std::is_same<T, float>::value ? NEAREST_R32 : NEAREST_R64;
  a.upper = upper;
  a.row_seeds = small ? nullptr : w.d_ns_row_seeds.get();
  a.seed = w.d_ns_seed;
  a.thr = w.d_ns_thr;
  sweep.walk<T>(a.p, d_table, st, [&]() { launch_nself_seed(st, a); });
  if (!small) launch_nself_seed_combine(st, a, lib->n_cus * 16);
  return clearance_passes<T>(ListKind::Self, who, s, d_table, n_conf, req, upper, a.p, a.pass,
                             [&]() { sweep.walk<T>(a.p, d_table, st, [&]() { launch_nself_chunk(st, a); }); }, d_out, d_min, n_evaluated, counts, st);
}

// ... of the moving objects among an environment kept on the device (include/hppfcl_amd_nearest_env.h: hfcl_scene_nearest_env*;
// hfcl_k_nearest_env.hip has the kernels, hfcl_nearest_env.hpp the arithmetic): nearest_self_run over the cells, chunks and spans of
// the env list maker (EnvSweep); the seeds are a partial per (row, span), then a wave per configuration.
// moving table on the device, n_conf > 0, at least one moving object, everything on st (which is waited for twice)
template <typename T>
static int nearest_env_run(const char* who, hfcl_scene* s, const void* d_table, size_t n_conf, const hfcl_distance_request* req, double upper,
                           hfcl_scene_clearance* d_out, typename SceneTypes<T>::R* d_min, size_t* n_evaluated, SceneCountSlots* counts,
                           hipStream_t st) {
  hfcl_lib* lib = s->lib;
  hfcl_lib::SceneWs& w = lib->scene;
  int rc = ensure_local_boxes(lib);
  if (rc) return rc;
  EnvSweep sweep;
  rc = sweep.ready(s, n_conf);
  if (rc) return rc;
  const size_t moving_rows = n_conf * s->n_moving;
  HIP_TRY(w.d_ns_row_seeds.grow(moving_rows * sweep.p.geo.n_spans * sizeof(NselfRowSeed)));
  rc = clearance_buffers(w, n_conf, moving_rows);
  if (rc) return rc;
  NenvArgs a{};
  sweep.args(a.e, n_conf);
  a.r = std::is_same<T, float>::value ? NEAREST_R32 : NEAREST_R64;
  a.upper = upper;
  a.prune = lib->opt.scene_nearest_env_prune ? 1 : 0;
  a.row_seeds = w.d_ns_row_seeds.get();
  a.seed = w.d_ns_seed;
  a.thr = w.d_ns_thr;
  a.env_terms = s->d_env_terms;
  a.env_tile_terms = s->d_env_tile_terms;
  sweep.walk<T>(a.e, d_table, st, [&]() { launch_nenv_seed(st, a); });
  launch_nenv_seed_combine(st, a, lib->n_cus * 16);
  return clearance_passes<T>(ListKind::Env, who, s, d_table, n_conf, req, upper, a.e.p, a.pass,
                             [&]() { sweep.walk<T>(a.e, d_table, st, [&]() { launch_nenv_chunk(st, a); }); }, d_out, d_min, n_evaluated, counts, st);
}

// ---- the three forms of either family (kind: Self / Env) ----
// head, then what the family's list maker refuses, then its limits.  nothing: n_conf == 0, or no pair whatever the table holds
template <typename T>
static int clearance_validate(ListKind kind, const char* who, const hfcl_scene* s, const void* table, size_t n_conf, const hfcl_distance_request* req,
                              double upper, const void* out, bool& nothing) {
  nothing = true;
  int rc = nearest_head<T>(who, s, req, upper, out, "null output");
  if (!rc) rc = pair_validate<T>(kind, who, s, table, n_conf, nothing);
  return rc ? rc : pair_limits(who, s, kind);
}
template <typename T>
static int clearance_run(ListKind kind, const char* who, hfcl_scene* s, const void* d_table, size_t n_conf, const hfcl_distance_request* req,
                         double upper, hfcl_scene_clearance* d_out, typename SceneTypes<T>::R* d_min, size_t* n_evaluated, SceneCountSlots* counts,
                         hipStream_t st) {
  return kind == ListKind::Env ? nearest_env_run<T>(who, s, d_table, n_conf, req, upper, d_out, d_min, n_evaluated, counts, st)
                               : nearest_self_run<T>(who, s, d_table, n_conf, req, upper, d_out, d_min, n_evaluated, counts, st);
}
template <typename T>
static int clearance_device(ListKind kind, const char* who, hfcl_scene* s, const void* d_table, size_t n_conf, const hfcl_distance_request* req,
                            double upper, hfcl_scene_clearance* d_out, typename SceneTypes<T>::R* d_min, size_t* n_evaluated, hipStream_t st) {
  bool nothing;
  const int rc = clearance_validate<T>(kind, who, s, d_table, n_conf, req, upper, d_out, nothing);
  if (rc) return rc;
  if (n_evaluated) n_evaluated[0] = n_evaluated[1] = 0;
  if (!n_conf) return HFCL_OK;
  HIP_TRY(hipSetDevice(s->lib->device));
  if (nothing) {  // no pair: every configuration is one without records
    clearance_combine(nullptr, n_conf, d_out, d_min, std::is_same<T, float>::value, st);
    HIP_TRY(hipGetLastError());
    return HFCL_OK;
  }
  return clearance_run<T>(kind, who, s, d_table, n_conf, req, upper, d_out, d_min, n_evaluated, nullptr, st);
}
template <typename T>
static int clearance_host(ListKind kind, const char* who, hfcl_scene* s, const void* table, size_t n_conf, const hfcl_distance_request* req,
                          double upper, hfcl_scene_clearance* out, typename SceneTypes<T>::R* min_records, size_t* n_evaluated) {
  using R = typename SceneTypes<T>::R;
  bool nothing;
  const int rc = clearance_validate<T>(kind, who, s, table, n_conf, req, upper, out, nothing);
  if (rc) return rc;
  if (n_evaluated) n_evaluated[0] = n_evaluated[1] = 0;
  if (!n_conf) return HFCL_OK;
  if (nothing) {  // no pair: the combine of no list, on the host
    const hfcl_scene_summary* no_summary[2] = {nullptr, nullptr};
    const uint32_t* no_pairs[2] = {nullptr, nullptr};
    const uint64_t* no_begin[2] = {nullptr, nullptr};
    const R* no_rec[2] = {nullptr, nullptr};
    for (size_t c = 0; c < n_conf; ++c) nself_combine<R>(c, no_summary, no_pairs, no_begin, no_rec, out[c], min_records ? &min_records[c] : nullptr);
    return HFCL_OK;
  }
  return nearest_host_shell<T>(who, s, table, pair_rows(s, kind), n_conf, req, s->lib->scene.d_ns_out, out, min_records,
                               [&](const void* d_table, hfcl_scene_clearance* d_out, R* d_min, SceneCountSlots* counts, hipStream_t st) {
                                 return clearance_run<T>(kind, who, s, d_table, n_conf, req, upper, d_out, d_min, n_evaluated, counts, st);
                               });
}

// ---------------------------------------------------------------------------------------
// A height-field terrain under the moving objects (include/hppfcl_amd_terrain.h): query q = c * n_t + k is the terrain against listed
// object k under configuration c.  The flat range goes in chunks of hfield_chunk queries: k_terrain_expand writes the chunk's four
// per-query arrays into the scene's workspace, hf_run (hfcl_host_hfield.hip) runs them exactly as a caller's batch of that size -- with
// the chunk's place in the call for hfcl_contact::pair and the running contact count --, k_terrain_status keeps the status words; after
// the last chunk k_terrain_fold folds the kept bounds and status words.  hfcl_k_terrain.hip has the kernels, hfcl_terrain.hpp the arithmetic.
// ---------------------------------------------------------------------------------------
// What a terrain call refuses before any work, in this order: a null scene, a null request, the request checks of the height-field
// calls, a stale scene, no terrain, a field that left the library, a listed object that is no pose row of the table any more, then
// (n_conf > 0) an overflow, nothing asked for, a null table.  nothing: n_conf == 0.  total: n_conf * n_t
static int terrain_validate(const char* who, const hfcl_scene* s, const void* table, size_t n_conf, const hfcl_collision_request* req,
                            bool any_output, size_t* n_contacts_out, QParams<double>& q, bool& skip_all, bool& nothing, size_t& total) {
  nothing = true;
  total = 0;
  if (!s) {
    set_error(std::string(who) + ": null scene");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (!req) {
    set_error(std::string(who) + ": null request");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (const int rc = hf_request(who, req, q, skip_all)) return rc;
  if (const int rc = groups_scene(who, s)) return rc;
  if (n_contacts_out) *n_contacts_out = 0;
  if (!s->has_terrain) {
    set_error(std::string(who) + ": the scene has no terrain (hfcl_scene_set_terrain)");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (s->terrain_hfield >= s->lib->hf.h_fields.size()) {
    set_error(std::string(who) + ": height field " + std::to_string(s->terrain_hfield) + " is no longer on the library (hfcl_lib_clear_hfields); set the terrain again");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  const size_t n_t = s->h_terrain_objects.size();
  if (n_t && s->h_terrain_objects.back() >= s->rows()) {
    set_error(std::string(who) + ": listed object " + std::to_string(s->h_terrain_objects.back()) + " is none of the " + std::to_string(s->rows()) +
              " moving objects (an environment was set after the terrain)");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (n_conf == 0) return HFCL_OK;
  if (n_t && n_conf > 0xFFFFFFF0ull / n_t) {
    set_error(std::string(who) + ": batch too large (max 2^32-16 queries per call)");
    return HFCL_ERR_LIMIT;
  }
  if (!any_output) {
    set_error(std::string(who) + ": records, bounds, summaries, contacts and the contact count all NULL");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (n_t && !table) {
    set_error(std::string(who) + ": null pose table");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  nothing = false;
  total = n_conf * n_t;
  return HFCL_OK;
}

// The call on a table that is on the device, on st.  d_out / d_bounds / d_summary / d_contacts: device destinations (nullptr each: not
// asked for); h_out / h_bounds: the host form's, filled chunk by chunk (the stream is waited for after every chunk then: the record
// buffer is the next chunk's)
static int terrain_run(hfcl_scene* s, const double* d_table, size_t n_conf, const hfcl_collision_request* req, const QParams<double>& q, bool skip_all,
                       hfcl_result* d_out, double* d_bounds, hfcl_scene_summary* d_summary, hfcl_contact* d_contacts, size_t contacts_cap,
                       bool want_contacts, hfcl_result* h_out, double* h_bounds, hipStream_t st) {
  hfcl_lib* lib = s->lib;
  hfcl_scene::TerrainWs& w = s->tw;
  const size_t n_t = s->h_terrain_objects.size(), total = n_conf * n_t;
  const size_t chunk = std::min(hf_chunk(lib), total);
  const bool fold = d_summary != nullptr;
  if (total) {  // (a buffer that grows is freed first, which waits for the device: nothing in flight reads the old one)
    HIP_TRY(w.d_hfield.grow(chunk));
    HIP_TRY(w.d_shape.grow(chunk));
    HIP_TRY(w.d_tfh.grow(12 * chunk));
    HIP_TRY(w.d_tfs.grow(12 * chunk));
    if (!d_out) HIP_TRY(w.d_rec.grow(chunk));
    if (!d_bounds && (fold || h_bounds)) {
      HIP_TRY(w.d_bounds.grow(total));
      d_bounds = w.d_bounds;
    }
    if (fold) HIP_TRY(w.d_status.grow(total));
  }
  const int max_blocks = lib->n_cus * 16;
  TerrainExpandArgs e;
  e.table = d_table;
  e.tf_terrain = s->d_terrain_tf;
  e.objects = s->d_terrain_objects;
  e.object_shape = s->d_object_shape;
  e.n_rows = s->rows();
  e.n_t = uint32_t(n_t);
  e.hfield = s->terrain_hfield;
  e.out_hfield = w.d_hfield;
  e.out_shape = w.d_shape;
  e.out_tfh = w.d_tfh;
  e.out_tfs = w.d_tfs;
  for (size_t q0 = 0; q0 < total; q0 += chunk) {
    const size_t m = std::min(chunk, total - q0);
    e.q0 = q0;
    e.m = uint32_t(m);
    launch_terrain_expand(st, e, max_blocks);
    hfcl_result* rec = d_out ? d_out + q0 : w.d_rec.get();
    const int rc = hf_run(lib, w.d_hfield, w.d_shape, w.d_tfh, w.d_tfs, m, nullptr, req, q, skip_all, rec, d_bounds ? d_bounds + q0 : nullptr, d_contacts,
                          contacts_cap, want_contacts, uint32_t(q0), q0 == 0, st);
    if (rc) return rc;
    if (fold) launch_terrain_status(st, rec, w.d_status.get() + q0, uint32_t(m), max_blocks);
    if (h_out || h_bounds) {
      if (h_out) HIP_TRY(hipMemcpyAsync(h_out + q0, rec, m * sizeof(hfcl_result), hipMemcpyDeviceToHost, st));
      if (h_bounds) HIP_TRY(hipMemcpyAsync(h_bounds + q0, d_bounds + q0, m * sizeof(double), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
    }
  }
  if (fold) {
    TerrainFoldArgs f;
    f.bounds = d_bounds;
    f.status = w.d_status;
    f.objects = s->d_terrain_objects;
    f.n_conf = n_conf;
    f.n_t = uint32_t(n_t);
    f.summary = d_summary;
    launch_terrain_fold(st, f, max_blocks);
  }
  HIP_TRY(hipGetLastError());
  return HFCL_OK;
}

extern "C" {

hfcl_scene* hfcl_scene_create(hfcl_lib* lib, const uint32_t* object_shape, size_t n_objects, const uint32_t* pairs, size_t n_pairs) {
  if (!lib) {
    set_error("hfcl_scene_create: null library");
    return nullptr;
  }
  if (n_objects && !object_shape) {
    set_error("hfcl_scene_create: null object table");
    return nullptr;
  }
  for (size_t o = 0; o < n_objects; ++o)
    if (object_shape[o] >= lib->n_shapes) {
      set_error("hfcl_scene_create: shape id " + std::to_string(object_shape[o]) + " of object " + std::to_string(o) + " is outside the library");
      return nullptr;
    }
  // (no return code here: the two causes that are not HFCL_ERR_INVALID_ARGUMENT name theirs at the head of the message)
  if (const int rc = scene_check_pairs("hfcl_scene_create", pairs, n_pairs, n_objects)) {
    if (rc == HFCL_ERR_LIMIT) set_error("HFCL_ERR_LIMIT: " + std::string(hfcl_last_error()));
    return nullptr;
  }
  if (hipSetDevice(lib->device) != hipSuccess) {
    set_error("HFCL_ERR_HIP: hfcl_scene_create: hipSetDevice failed");
    return nullptr;
  }
  hfcl_scene* s = new hfcl_scene();
  s->lib = lib;
  s->n_objects = n_objects;
  s->n_pairs = n_pairs;
  s->epoch = lib->shapes_epoch;
  s->h_object_shape.assign(object_shape, object_shape + n_objects);
  if (scene_upload(s->d_object_shape, object_shape, n_objects) != HFCL_OK || scene_upload(s->d_pairs, pairs, 2 * n_pairs) != HFCL_OK) {
    set_error("HFCL_ERR_HIP: hfcl_scene_create: " + std::string(hfcl_last_error()));
    hfcl_scene_destroy(s);
    return nullptr;
  }
  return s;
}

int hfcl_scene_set_pairs(hfcl_scene* s, const uint32_t* pairs, size_t n_pairs) {
  if (!s) {
    set_error("hfcl_scene_set_pairs: null scene");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  int rc = scene_check_pairs("hfcl_scene_set_pairs", pairs, n_pairs, s->n_objects);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(s->lib->device));
  DevBuf<uint32_t> d;
  rc = scene_upload(d, pairs, 2 * n_pairs);
  if (rc) return rc;
  s->d_pairs = std::move(d);  // (freeing the old list waits for the device: a query in flight on some stream may still be reading it)
  s->n_pairs = n_pairs;
  return HFCL_OK;
}

void hfcl_scene_destroy(hfcl_scene* s) {
  if (!s) return;
  hipSetDevice(s->lib->device);
  delete s;
}
size_t hfcl_scene_num_objects(const hfcl_scene* s) { return s ? s->n_objects : 0; }
int hfcl_scene_last_pairs_form(const hfcl_scene* s) { return s ? s->last_pairs_form : -1; }
size_t hfcl_scene_num_pairs(const hfcl_scene* s) { return s ? s->n_pairs : 0; }

int hfcl_scene_collide(hfcl_scene* s, const double* object_tf, size_t n_conf, const hfcl_collision_request* req, hfcl_result* out,
                       hfcl_scene_summary* summary, const hfcl_guess* guess_in, hfcl_guess* guess_out) {
  return scene_host<double>("hfcl_scene_collide", s, object_tf, n_conf, req, nullptr, out, summary, guess_in, guess_out);
}
int hfcl_scene_distance(hfcl_scene* s, const double* object_tf, size_t n_conf, const hfcl_distance_request* req, hfcl_result* out,
                        hfcl_scene_summary* summary, const hfcl_guess* guess_in, hfcl_guess* guess_out) {
  return scene_host<double>("hfcl_scene_distance", s, object_tf, n_conf, nullptr, req, out, summary, guess_in, guess_out);
}
int hfcl_scene_collide_device(hfcl_scene* s, const double* d_object_tf, size_t n_conf, const hfcl_collision_request* req, hfcl_result* d_out,
                              hfcl_scene_summary* d_summary, const hfcl_guess* d_guess_in, hfcl_guess* d_guess_out, void* stream) {
  return scene_device<double>("hfcl_scene_collide_device", s, d_object_tf, n_conf, req, nullptr, d_out, d_summary, d_guess_in, d_guess_out,
                              (hipStream_t)stream);
}
int hfcl_scene_distance_device(hfcl_scene* s, const double* d_object_tf, size_t n_conf, const hfcl_distance_request* req, hfcl_result* d_out,
                               hfcl_scene_summary* d_summary, const hfcl_guess* d_guess_in, hfcl_guess* d_guess_out, void* stream) {
  return scene_device<double>("hfcl_scene_distance_device", s, d_object_tf, n_conf, nullptr, req, d_out, d_summary, d_guess_in, d_guess_out,
                              (hipStream_t)stream);
}
int hfcl_scene_collide_f32(hfcl_scene* s, const float* object_pose, size_t n_conf, const hfcl_collision_request* req, hfcl_result_f32* out,
                           hfcl_scene_summary* summary) {
  return scene_host<float>("hfcl_scene_collide_f32", s, object_pose, n_conf, req, nullptr, out, summary, nullptr, nullptr);
}
int hfcl_scene_distance_f32(hfcl_scene* s, const float* object_pose, size_t n_conf, const hfcl_distance_request* req, hfcl_result_f32* out,
                            hfcl_scene_summary* summary) {
  return scene_host<float>("hfcl_scene_distance_f32", s, object_pose, n_conf, nullptr, req, out, summary, nullptr, nullptr);
}
int hfcl_scene_collide_device_f32(hfcl_scene* s, const float* d_object_pose, size_t n_conf, const hfcl_collision_request* req,
                                  hfcl_result_f32* d_out, hfcl_scene_summary* d_summary, void* stream) {
  return scene_device<float>("hfcl_scene_collide_device_f32", s, d_object_pose, n_conf, req, nullptr, d_out, d_summary, nullptr, nullptr,
                             (hipStream_t)stream);
}
int hfcl_scene_distance_device_f32(hfcl_scene* s, const float* d_object_pose, size_t n_conf, const hfcl_distance_request* req,
                                   hfcl_result_f32* d_out, hfcl_scene_summary* d_summary, void* stream) {
  return scene_device<float>("hfcl_scene_distance_device_f32", s, d_object_pose, n_conf, nullptr, req, d_out, d_summary, nullptr, nullptr,
                             (hipStream_t)stream);
}

// ---- culling the pair list per configuration ---------------------------------------------------------------------------------------
int hfcl_scene_world_aabbs(hfcl_scene* s, const double* object_tf, size_t n_conf, double* aabbs_out) {
  return scene_boxes_host<double>("hfcl_scene_world_aabbs", s, object_tf, n_conf, aabbs_out);
}
int hfcl_scene_world_aabbs_f32(hfcl_scene* s, const float* object_pose, size_t n_conf, double* aabbs_out) {
  return scene_boxes_host<float>("hfcl_scene_world_aabbs_f32", s, object_pose, n_conf, aabbs_out);
}
int hfcl_scene_world_aabbs_device(hfcl_scene* s, const double* d_object_tf, size_t n_conf, double* d_aabbs_out, void* stream) {
  return scene_boxes_device<double>("hfcl_scene_world_aabbs_device", s, d_object_tf, n_conf, d_aabbs_out, (hipStream_t)stream);
}
int hfcl_scene_world_aabbs_device_f32(hfcl_scene* s, const float* d_object_pose, size_t n_conf, double* d_aabbs_out, void* stream) {
  return scene_boxes_device<float>("hfcl_scene_world_aabbs_device_f32", s, d_object_pose, n_conf, d_aabbs_out, (hipStream_t)stream);
}
int hfcl_scene_cull(hfcl_scene* s, const double* object_tf, size_t n_conf, double inflate, uint64_t* query_ids, size_t capacity,
                    uint64_t* conf_begin, size_t* n_listed) {
  return scene_cull_host<double>("hfcl_scene_cull", s, object_tf, n_conf, inflate, query_ids, capacity, conf_begin, n_listed);
}
int hfcl_scene_cull_f32(hfcl_scene* s, const float* object_pose, size_t n_conf, double inflate, uint64_t* query_ids, size_t capacity,
                        uint64_t* conf_begin, size_t* n_listed) {
  return scene_cull_host<float>("hfcl_scene_cull_f32", s, object_pose, n_conf, inflate, query_ids, capacity, conf_begin, n_listed);
}
int hfcl_scene_cull_device(hfcl_scene* s, const double* d_object_tf, size_t n_conf, double inflate, uint64_t* d_query_ids, size_t capacity,
                           uint64_t* d_conf_begin, uint64_t* d_n_listed, void* stream) {
  return cull_device<double>("hfcl_scene_cull_device", s, d_object_tf, n_conf, inflate, d_query_ids, capacity, d_conf_begin, d_n_listed,
                             (hipStream_t)stream);
}
int hfcl_scene_cull_device_f32(hfcl_scene* s, const float* d_object_pose, size_t n_conf, double inflate, uint64_t* d_query_ids, size_t capacity,
                               uint64_t* d_conf_begin, uint64_t* d_n_listed, void* stream) {
  return cull_device<float>("hfcl_scene_cull_device_f32", s, d_object_pose, n_conf, inflate, d_query_ids, capacity, d_conf_begin, d_n_listed,
                            (hipStream_t)stream);
}
int hfcl_scene_collide_listed_device(hfcl_scene* s, const double* d_object_tf, size_t n_conf, const uint64_t* d_query_ids, size_t n_listed,
                                     const uint64_t* d_conf_begin, const hfcl_collision_request* req, hfcl_result* d_out,
                                     hfcl_scene_summary* d_summary, const hfcl_guess* d_guess_in, hfcl_guess* d_guess_out, void* stream) {
  return scene_listed_device<double>("hfcl_scene_collide_listed_device", s, d_object_tf, n_conf, d_query_ids, n_listed, d_conf_begin, req, nullptr,
                                     d_out, d_summary, d_guess_in, d_guess_out, (hipStream_t)stream);
}
int hfcl_scene_distance_listed_device(hfcl_scene* s, const double* d_object_tf, size_t n_conf, const uint64_t* d_query_ids, size_t n_listed,
                                      const uint64_t* d_conf_begin, const hfcl_distance_request* req, hfcl_result* d_out,
                                      hfcl_scene_summary* d_summary, const hfcl_guess* d_guess_in, hfcl_guess* d_guess_out, void* stream) {
  return scene_listed_device<double>("hfcl_scene_distance_listed_device", s, d_object_tf, n_conf, d_query_ids, n_listed, d_conf_begin, nullptr, req,
                                     d_out, d_summary, d_guess_in, d_guess_out, (hipStream_t)stream);
}
int hfcl_scene_collide_listed_device_f32(hfcl_scene* s, const float* d_object_pose, size_t n_conf, const uint64_t* d_query_ids, size_t n_listed,
                                         const uint64_t* d_conf_begin, const hfcl_collision_request* req, hfcl_result_f32* d_out,
                                         hfcl_scene_summary* d_summary, void* stream) {
  return scene_listed_device<float>("hfcl_scene_collide_listed_device_f32", s, d_object_pose, n_conf, d_query_ids, n_listed, d_conf_begin, req,
                                    nullptr, d_out, d_summary, nullptr, nullptr, (hipStream_t)stream);
}
int hfcl_scene_distance_listed_device_f32(hfcl_scene* s, const float* d_object_pose, size_t n_conf, const uint64_t* d_query_ids, size_t n_listed,
                                          const uint64_t* d_conf_begin, const hfcl_distance_request* req, hfcl_result_f32* d_out,
                                          hfcl_scene_summary* d_summary, void* stream) {
  return scene_listed_device<float>("hfcl_scene_distance_listed_device_f32", s, d_object_pose, n_conf, d_query_ids, n_listed, d_conf_begin, nullptr,
                                    req, d_out, d_summary, nullptr, nullptr, (hipStream_t)stream);
}
int hfcl_scene_collide_culled(hfcl_scene* s, const double* object_tf, size_t n_conf, double inflate, const hfcl_collision_request* req,
                              hfcl_result* out, size_t out_capacity, uint64_t* query_ids_out, uint64_t* conf_begin_out,
                              hfcl_scene_summary* summary, const hfcl_guess* guess_in, hfcl_guess* guess_out, size_t* n_listed) {
  const SceneCull cull{ListKind::Culled, inflate, out_capacity, query_ids_out, nullptr, conf_begin_out, n_listed};
  return scene_host<double>("hfcl_scene_collide_culled", s, object_tf, n_conf, req, nullptr, out, summary, guess_in, guess_out, &cull);
}
int hfcl_scene_distance_culled(hfcl_scene* s, const double* object_tf, size_t n_conf, double inflate, const hfcl_distance_request* req,
                               hfcl_result* out, size_t out_capacity, uint64_t* query_ids_out, uint64_t* conf_begin_out,
                               hfcl_scene_summary* summary, const hfcl_guess* guess_in, hfcl_guess* guess_out, size_t* n_listed) {
  const SceneCull cull{ListKind::Culled, inflate, out_capacity, query_ids_out, nullptr, conf_begin_out, n_listed};
  return scene_host<double>("hfcl_scene_distance_culled", s, object_tf, n_conf, nullptr, req, out, summary, guess_in, guess_out, &cull);
}
int hfcl_scene_collide_culled_f32(hfcl_scene* s, const float* object_pose, size_t n_conf, double inflate, const hfcl_collision_request* req,
                                  hfcl_result_f32* out, size_t out_capacity, uint64_t* query_ids_out, uint64_t* conf_begin_out,
                                  hfcl_scene_summary* summary, size_t* n_listed) {
  const SceneCull cull{ListKind::Culled, inflate, out_capacity, query_ids_out, nullptr, conf_begin_out, n_listed};
  return scene_host<float>("hfcl_scene_collide_culled_f32", s, object_pose, n_conf, req, nullptr, out, summary, nullptr, nullptr, &cull);
}
int hfcl_scene_distance_culled_f32(hfcl_scene* s, const float* object_pose, size_t n_conf, double inflate, const hfcl_distance_request* req,
                                   hfcl_result_f32* out, size_t out_capacity, uint64_t* query_ids_out, uint64_t* conf_begin_out,
                                   hfcl_scene_summary* summary, size_t* n_listed) {
  const SceneCull cull{ListKind::Culled, inflate, out_capacity, query_ids_out, nullptr, conf_begin_out, n_listed};
  return scene_host<float>("hfcl_scene_distance_culled_f32", s, object_pose, n_conf, nullptr, req, out, summary, nullptr, nullptr, &cull);
}

// ---- the self-collision pairs per configuration (include/hppfcl_amd_pairs.h) ---------------------------------------------------------
#define PAIRS_ENTRY                                     \
  if (const int no_device = pairs_need_device()) return no_device
int hfcl_scene_self_pairs(hfcl_scene* s, const double* object_tf, size_t n_conf, double inflate, uint32_t* pairs, size_t capacity,
                          uint64_t* conf_begin, size_t* n_listed) {
  PAIRS_ENTRY;
  return pairs_host<double>(ListKind::Self, "hfcl_scene_self_pairs", s, object_tf, n_conf, inflate, pairs, capacity, conf_begin, n_listed);
}
int hfcl_scene_self_pairs_f32(hfcl_scene* s, const float* object_pose, size_t n_conf, double inflate, uint32_t* pairs, size_t capacity,
                              uint64_t* conf_begin, size_t* n_listed) {
  PAIRS_ENTRY;
  return pairs_host<float>(ListKind::Self, "hfcl_scene_self_pairs_f32", s, object_pose, n_conf, inflate, pairs, capacity, conf_begin, n_listed);
}
int hfcl_scene_self_pairs_device(hfcl_scene* s, const double* d_object_tf, size_t n_conf, double inflate, uint32_t* d_pairs, size_t capacity,
                                 uint64_t* d_conf_begin, uint64_t* d_n_listed, void* stream) {
  PAIRS_ENTRY;
  return pairs_device<double>(ListKind::Self, "hfcl_scene_self_pairs_device", s, d_object_tf, n_conf, inflate, d_pairs, capacity, d_conf_begin, d_n_listed,
                                   (hipStream_t)stream);
}
int hfcl_scene_self_pairs_device_f32(hfcl_scene* s, const float* d_object_pose, size_t n_conf, double inflate, uint32_t* d_pairs, size_t capacity,
                                     uint64_t* d_conf_begin, uint64_t* d_n_listed, void* stream) {
  PAIRS_ENTRY;
  return pairs_device<float>(ListKind::Self, "hfcl_scene_self_pairs_device_f32", s, d_object_pose, n_conf, inflate, d_pairs, capacity, d_conf_begin,
                                  d_n_listed, (hipStream_t)stream);
}
int hfcl_scene_collide_pairs_device(hfcl_scene* s, const double* d_object_tf, size_t n_conf, const uint32_t* d_pairs, size_t n_listed,
                                    const uint64_t* d_conf_begin, const hfcl_collision_request* req, hfcl_result* d_out,
                                    hfcl_scene_summary* d_summary, const hfcl_guess* d_guess_in, hfcl_guess* d_guess_out, void* stream) {
  PAIRS_ENTRY;
  return scene_pairs_device<double>(ListKind::Self, "hfcl_scene_collide_pairs_device", s, d_object_tf, n_conf, d_pairs, n_listed, d_conf_begin, req, nullptr, d_out,
                                    d_summary, d_guess_in, d_guess_out, (hipStream_t)stream);
}
int hfcl_scene_distance_pairs_device(hfcl_scene* s, const double* d_object_tf, size_t n_conf, const uint32_t* d_pairs, size_t n_listed,
                                     const uint64_t* d_conf_begin, const hfcl_distance_request* req, hfcl_result* d_out,
                                     hfcl_scene_summary* d_summary, const hfcl_guess* d_guess_in, hfcl_guess* d_guess_out, void* stream) {
  PAIRS_ENTRY;
  return scene_pairs_device<double>(ListKind::Self, "hfcl_scene_distance_pairs_device", s, d_object_tf, n_conf, d_pairs, n_listed, d_conf_begin, nullptr, req, d_out,
                                    d_summary, d_guess_in, d_guess_out, (hipStream_t)stream);
}
int hfcl_scene_collide_pairs_device_f32(hfcl_scene* s, const float* d_object_pose, size_t n_conf, const uint32_t* d_pairs, size_t n_listed,
                                        const uint64_t* d_conf_begin, const hfcl_collision_request* req, hfcl_result_f32* d_out,
                                        hfcl_scene_summary* d_summary, void* stream) {
  PAIRS_ENTRY;
  return scene_pairs_device<float>(ListKind::Self, "hfcl_scene_collide_pairs_device_f32", s, d_object_pose, n_conf, d_pairs, n_listed, d_conf_begin, req, nullptr,
                                   d_out, d_summary, nullptr, nullptr, (hipStream_t)stream);
}
int hfcl_scene_distance_pairs_device_f32(hfcl_scene* s, const float* d_object_pose, size_t n_conf, const uint32_t* d_pairs, size_t n_listed,
                                         const uint64_t* d_conf_begin, const hfcl_distance_request* req, hfcl_result_f32* d_out,
                                         hfcl_scene_summary* d_summary, void* stream) {
  PAIRS_ENTRY;
  return scene_pairs_device<float>(ListKind::Self, "hfcl_scene_distance_pairs_device_f32", s, d_object_pose, n_conf, d_pairs, n_listed, d_conf_begin, nullptr, req,
                                   d_out, d_summary, nullptr, nullptr, (hipStream_t)stream);
}
int hfcl_scene_collide_self(hfcl_scene* s, const double* object_tf, size_t n_conf, double inflate, const hfcl_collision_request* req,
                            hfcl_result* out, size_t out_capacity, uint32_t* pairs_out, uint64_t* conf_begin_out, hfcl_scene_summary* summary,
                            const hfcl_guess* guess_in, hfcl_guess* guess_out, size_t* n_listed) {
  PAIRS_ENTRY;
  const SceneCull cull{ListKind::Self, inflate, out_capacity, nullptr, pairs_out, conf_begin_out, n_listed};
  return scene_host<double>("hfcl_scene_collide_self", s, object_tf, n_conf, req, nullptr, out, summary, guess_in, guess_out, &cull);
}
int hfcl_scene_distance_self(hfcl_scene* s, const double* object_tf, size_t n_conf, double inflate, const hfcl_distance_request* req,
                             hfcl_result* out, size_t out_capacity, uint32_t* pairs_out, uint64_t* conf_begin_out, hfcl_scene_summary* summary,
                             const hfcl_guess* guess_in, hfcl_guess* guess_out, size_t* n_listed) {
  PAIRS_ENTRY;
  const SceneCull cull{ListKind::Self, inflate, out_capacity, nullptr, pairs_out, conf_begin_out, n_listed};
  return scene_host<double>("hfcl_scene_distance_self", s, object_tf, n_conf, nullptr, req, out, summary, guess_in, guess_out, &cull);
}
int hfcl_scene_collide_self_f32(hfcl_scene* s, const float* object_pose, size_t n_conf, double inflate, const hfcl_collision_request* req,
                                hfcl_result_f32* out, size_t out_capacity, uint32_t* pairs_out, uint64_t* conf_begin_out,
                                hfcl_scene_summary* summary, size_t* n_listed) {
  PAIRS_ENTRY;
  const SceneCull cull{ListKind::Self, inflate, out_capacity, nullptr, pairs_out, conf_begin_out, n_listed};
  return scene_host<float>("hfcl_scene_collide_self_f32", s, object_pose, n_conf, req, nullptr, out, summary, nullptr, nullptr, &cull);
}
int hfcl_scene_distance_self_f32(hfcl_scene* s, const float* object_pose, size_t n_conf, double inflate, const hfcl_distance_request* req,
                                 hfcl_result_f32* out, size_t out_capacity, uint32_t* pairs_out, uint64_t* conf_begin_out,
                                 hfcl_scene_summary* summary, size_t* n_listed) {
  PAIRS_ENTRY;
  const SceneCull cull{ListKind::Self, inflate, out_capacity, nullptr, pairs_out, conf_begin_out, n_listed};
  return scene_host<float>("hfcl_scene_distance_self_f32", s, object_pose, n_conf, nullptr, req, out, summary, nullptr, nullptr, &cull);
}

// ---- object groups of the lists made above (include/hppfcl_amd_groups.h) ---------------------------------------------------------------
int hfcl_scene_set_groups(hfcl_scene* s, const uint8_t* object_group, size_t n_groups, const uint64_t* collides) {
  PAIRS_ENTRY;
  const char* who = "hfcl_scene_set_groups";
  int rc = groups_scene(who, s);
  if (rc) return rc;
  auto refuse = [&](const std::string& why) {
    set_error(std::string(who) + ": " + why);
    return HFCL_ERR_INVALID_ARGUMENT;
  };
  if (n_groups < 1 || n_groups > PAIRS_MAX_GROUPS) return refuse(std::to_string(n_groups) + " groups (1 to " + std::to_string(PAIRS_MAX_GROUPS) + ")");
  if (!collides) return refuse("null group matrix");
  if (s->n_objects && !object_group) return refuse("null group table");
  for (size_t o = 0; o < s->n_objects; ++o)
    if (object_group[o] >= n_groups)
      return refuse("group " + std::to_string(object_group[o]) + " of object " + std::to_string(o) + " is outside the " + std::to_string(n_groups) + " groups");
  for (size_t g = 0; g < n_groups; ++g) {
    if (n_groups < 64 && (collides[g] >> n_groups) != 0u)
      return refuse("word " + std::to_string(g) + " of the group matrix has a bit set at or above the " + std::to_string(n_groups) + " groups");
    for (size_t h = 0; h < g; ++h)
      if (((collides[g] >> h) & 1u) != ((collides[h] >> g) & 1u))
        return refuse("the group matrix is not symmetric: groups " + std::to_string(h) + " and " + std::to_string(g));
  }
  // the tables: the masks padded to PAIRS_MAX_GROUPS words, the groups present per column tile (hfcl_pairs.hpp: the sweep skips by them)
  uint64_t masks[PAIRS_MAX_GROUPS] = {};
  std::copy(collides, collides + n_groups, masks);
  const uint32_t n = uint32_t(std::min<size_t>(s->n_objects, 0xFFFFFFFFu));  // (scenes beyond the self forms' limit are refused there)
  std::vector<uint64_t> tiles(std::max<uint32_t>(pairs_tiles(n), 1u), 0u);
  for (uint32_t t = 0; t < pairs_tiles(n); ++t) tiles[t] = pairs_tile_word(object_group, n, t);
  const uint8_t none = 0;
  HIP_TRY(hipSetDevice(s->lib->device));
  DevBuf<uint8_t> d_group;
  DevBuf<uint64_t> d_collides, d_tile_groups;
  rc = groups_upload(d_group, s->n_objects ? object_group : &none, std::max<size_t>(s->n_objects, 1));
  if (!rc) rc = groups_upload(d_collides, masks, size_t(PAIRS_MAX_GROUPS));
  if (!rc) rc = groups_upload(d_tile_groups, tiles.data(), tiles.size());
  if (rc) return rc;  // (the scene as it was)
  // (freeing the old tables waits for the device: a query in flight on some stream may still be reading them)
  s->d_group = std::move(d_group);
  s->d_collides = std::move(d_collides);
  s->d_tile_groups = std::move(d_tile_groups);
  s->n_groups = n_groups;
  s->h_group.assign(object_group, object_group + s->n_objects);
  return env_tile_groups(s);  // (a scene with an environment: the groups per tile of its tiling)
}
int hfcl_scene_clear_groups(hfcl_scene* s) {
  PAIRS_ENTRY;
  if (const int rc = groups_scene("hfcl_scene_clear_groups", s)) return rc;
  HIP_TRY(hipSetDevice(s->lib->device));
  reset_all(s->d_group, s->d_collides, s->d_tile_groups, s->d_env_tile_groups);  // (waits for the device, as above)
  s->n_groups = 0;
  return HFCL_OK;
}
size_t hfcl_scene_num_groups(const hfcl_scene* s) { return s ? s->n_groups : 0; }

// ---- the clearance per configuration on device-made pairs (include/hppfcl_amd_nearest_self.h) -------------------------------------------
int hfcl_scene_nearest_self(hfcl_scene* s, const double* object_tf, size_t n_conf, const hfcl_distance_request* req, double upper_bound,
                            hfcl_scene_clearance* out, hfcl_result* min_records, size_t* n_evaluated) {
  PAIRS_ENTRY;
  return clearance_host<double>(ListKind::Self, "hfcl_scene_nearest_self", s, object_tf, n_conf, req, upper_bound, out, min_records, n_evaluated);
}
int hfcl_scene_nearest_self_f32(hfcl_scene* s, const float* object_pose, size_t n_conf, const hfcl_distance_request* req, double upper_bound,
                                hfcl_scene_clearance* out, hfcl_result_f32* min_records, size_t* n_evaluated) {
  PAIRS_ENTRY;
  return clearance_host<float>(ListKind::Self, "hfcl_scene_nearest_self_f32", s, object_pose, n_conf, req, upper_bound, out, min_records, n_evaluated);
}
int hfcl_scene_nearest_self_device(hfcl_scene* s, const double* d_object_tf, size_t n_conf, const hfcl_distance_request* req, double upper_bound,
                                   hfcl_scene_clearance* d_out, hfcl_result* d_min_records, size_t* n_evaluated, void* stream) {
  PAIRS_ENTRY;
  return clearance_device<double>(ListKind::Self, "hfcl_scene_nearest_self_device", s, d_object_tf, n_conf, req, upper_bound, d_out, d_min_records, n_evaluated,
                                     (hipStream_t)stream);
}
int hfcl_scene_nearest_self_device_f32(hfcl_scene* s, const float* d_object_pose, size_t n_conf, const hfcl_distance_request* req,
                                       double upper_bound, hfcl_scene_clearance* d_out, hfcl_result_f32* d_min_records, size_t* n_evaluated,
                                       void* stream) {
  PAIRS_ENTRY;
  return clearance_device<float>(ListKind::Self, "hfcl_scene_nearest_self_device_f32", s, d_object_pose, n_conf, req, upper_bound, d_out, d_min_records,
                                    n_evaluated, (hipStream_t)stream);
}

// ---- a static environment kept on the device (include/hppfcl_amd_env.h) ----------------------------------------------------------------
int hfcl_scene_set_environment(hfcl_scene* s, size_t n_moving, const double* env_tf) {
  PAIRS_ENTRY;
  return env_set<double>("hfcl_scene_set_environment", s, n_moving, env_tf);
}
int hfcl_scene_set_environment_f32(hfcl_scene* s, size_t n_moving, const float* env_pose) {
  PAIRS_ENTRY;
  return env_set<float>("hfcl_scene_set_environment_f32", s, n_moving, env_pose);
}
int hfcl_scene_clear_environment(hfcl_scene* s) {
  PAIRS_ENTRY;
  if (const int rc = groups_scene("hfcl_scene_clear_environment", s)) return rc;
  HIP_TRY(hipSetDevice(s->lib->device));
  s->d_env_table.reset();  // (waits for the device: a query in flight on some stream may still be reading the tables)
  reset_all(s->d_env_boxes, s->d_env_tile_boxes, s->d_env_terms, s->d_env_tile_terms);
  s->d_env_tile_groups.reset();
  s->has_env = false;
  s->n_moving = 0;
  return HFCL_OK;
}
size_t hfcl_scene_n_moving(const hfcl_scene* s) { return s ? (s->has_env ? s->n_moving : s->n_objects) : 0; }
int hfcl_scene_environment_aabbs(hfcl_scene* s, double* aabbs_out, double* tile_aabbs_out) {
  PAIRS_ENTRY;
  const char* who = "hfcl_scene_environment_aabbs";
  if (const int rc = groups_scene(who, s)) return rc;
  if (!s->has_env) {
    set_error(std::string(who) + ": the scene has no environment (hfcl_scene_set_environment)");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  const size_t n_env = s->n_env();
  if (!n_env) return HFCL_OK;
  HIP_TRY(hipSetDevice(s->lib->device));
  if (aabbs_out) HIP_TRY(hipMemcpy(aabbs_out, s->d_env_boxes, n_env * 6 * sizeof(double), hipMemcpyDeviceToHost));
  if (tile_aabbs_out)
    HIP_TRY(hipMemcpy(tile_aabbs_out, s->d_env_tile_boxes, size_t(env_tiles(uint32_t(n_env))) * 6 * sizeof(double), hipMemcpyDeviceToHost));
  return HFCL_OK;
}
int hfcl_scene_env_pairs(hfcl_scene* s, const double* moving_tf, size_t n_conf, double inflate, uint32_t* pairs, size_t capacity,
                         uint64_t* conf_begin, size_t* n_listed) {
  PAIRS_ENTRY;
  return pairs_host<double>(ListKind::Env, "hfcl_scene_env_pairs", s, moving_tf, n_conf, inflate, pairs, capacity, conf_begin, n_listed);
}
int hfcl_scene_env_pairs_f32(hfcl_scene* s, const float* moving_pose, size_t n_conf, double inflate, uint32_t* pairs, size_t capacity,
                             uint64_t* conf_begin, size_t* n_listed) {
  PAIRS_ENTRY;
  return pairs_host<float>(ListKind::Env, "hfcl_scene_env_pairs_f32", s, moving_pose, n_conf, inflate, pairs, capacity, conf_begin, n_listed);
}
int hfcl_scene_env_pairs_device(hfcl_scene* s, const double* d_moving_tf, size_t n_conf, double inflate, uint32_t* d_pairs, size_t capacity,
                                uint64_t* d_conf_begin, uint64_t* d_n_listed, void* stream) {
  PAIRS_ENTRY;
  return pairs_device<double>(ListKind::Env, "hfcl_scene_env_pairs_device", s, d_moving_tf, n_conf, inflate, d_pairs, capacity, d_conf_begin, d_n_listed,
                                  (hipStream_t)stream);
}
int hfcl_scene_env_pairs_device_f32(hfcl_scene* s, const float* d_moving_pose, size_t n_conf, double inflate, uint32_t* d_pairs,
                                    size_t capacity, uint64_t* d_conf_begin, uint64_t* d_n_listed, void* stream) {
  PAIRS_ENTRY;
  return pairs_device<float>(ListKind::Env, "hfcl_scene_env_pairs_device_f32", s, d_moving_pose, n_conf, inflate, d_pairs, capacity, d_conf_begin,
                                 d_n_listed, (hipStream_t)stream);
}
int hfcl_scene_collide_env_pairs_device(hfcl_scene* s, const double* d_moving_tf, size_t n_conf, const uint32_t* d_pairs, size_t n_listed,
                                        const uint64_t* d_conf_begin, const hfcl_collision_request* req, hfcl_result* d_out,
                                        hfcl_scene_summary* d_summary, const hfcl_guess* d_guess_in, hfcl_guess* d_guess_out, void* stream) {
  PAIRS_ENTRY;
  return scene_pairs_device<double>(ListKind::Env, "hfcl_scene_collide_env_pairs_device", s, d_moving_tf, n_conf, d_pairs, n_listed, d_conf_begin, req, nullptr,
                                        d_out, d_summary, d_guess_in, d_guess_out, (hipStream_t)stream);
}
int hfcl_scene_distance_env_pairs_device(hfcl_scene* s, const double* d_moving_tf, size_t n_conf, const uint32_t* d_pairs, size_t n_listed,
                                         const uint64_t* d_conf_begin, const hfcl_distance_request* req, hfcl_result* d_out,
                                         hfcl_scene_summary* d_summary, const hfcl_guess* d_guess_in, hfcl_guess* d_guess_out, void* stream) {
  PAIRS_ENTRY;
  return scene_pairs_device<double>(ListKind::Env, "hfcl_scene_distance_env_pairs_device", s, d_moving_tf, n_conf, d_pairs, n_listed, d_conf_begin, nullptr, req,
                                        d_out, d_summary, d_guess_in, d_guess_out, (hipStream_t)stream);
}
int hfcl_scene_collide_env_pairs_device_f32(hfcl_scene* s, const float* d_moving_pose, size_t n_conf, const uint32_t* d_pairs,
                                            size_t n_listed, const uint64_t* d_conf_begin, const hfcl_collision_request* req,
                                            hfcl_result_f32* d_out, hfcl_scene_summary* d_summary, void* stream) {
  PAIRS_ENTRY;
  return scene_pairs_device<float>(ListKind::Env, "hfcl_scene_collide_env_pairs_device_f32", s, d_moving_pose, n_conf, d_pairs, n_listed, d_conf_begin, req,
                                       nullptr, d_out, d_summary, nullptr, nullptr, (hipStream_t)stream);
}
int hfcl_scene_distance_env_pairs_device_f32(hfcl_scene* s, const float* d_moving_pose, size_t n_conf, const uint32_t* d_pairs,
                                             size_t n_listed, const uint64_t* d_conf_begin, const hfcl_distance_request* req,
                                             hfcl_result_f32* d_out, hfcl_scene_summary* d_summary, void* stream) {
  PAIRS_ENTRY;
  return scene_pairs_device<float>(ListKind::Env, "hfcl_scene_distance_env_pairs_device_f32", s, d_moving_pose, n_conf, d_pairs, n_listed, d_conf_begin,
                                       nullptr, req, d_out, d_summary, nullptr, nullptr, (hipStream_t)stream);
}
int hfcl_scene_collide_env(hfcl_scene* s, const double* moving_tf, size_t n_conf, double inflate, const hfcl_collision_request* req,
                           hfcl_result* out, size_t out_capacity, uint32_t* pairs_out, uint64_t* conf_begin_out, hfcl_scene_summary* summary,
                           const hfcl_guess* guess_in, hfcl_guess* guess_out, size_t* n_listed) {
  PAIRS_ENTRY;
  const SceneCull cull{ListKind::Env, inflate, out_capacity, nullptr, pairs_out, conf_begin_out, n_listed};
  return scene_host<double>("hfcl_scene_collide_env", s, moving_tf, n_conf, req, nullptr, out, summary, guess_in, guess_out, &cull);
}
int hfcl_scene_distance_env(hfcl_scene* s, const double* moving_tf, size_t n_conf, double inflate, const hfcl_distance_request* req,
                            hfcl_result* out, size_t out_capacity, uint32_t* pairs_out, uint64_t* conf_begin_out, hfcl_scene_summary* summary,
                            const hfcl_guess* guess_in, hfcl_guess* guess_out, size_t* n_listed) {
  PAIRS_ENTRY;
  const SceneCull cull{ListKind::Env, inflate, out_capacity, nullptr, pairs_out, conf_begin_out, n_listed};
  return scene_host<double>("hfcl_scene_distance_env", s, moving_tf, n_conf, nullptr, req, out, summary, guess_in, guess_out, &cull);
}
int hfcl_scene_collide_env_f32(hfcl_scene* s, const float* moving_pose, size_t n_conf, double inflate, const hfcl_collision_request* req,
                               hfcl_result_f32* out, size_t out_capacity, uint32_t* pairs_out, uint64_t* conf_begin_out,
                               hfcl_scene_summary* summary, size_t* n_listed) {
  PAIRS_ENTRY;
  const SceneCull cull{ListKind::Env, inflate, out_capacity, nullptr, pairs_out, conf_begin_out, n_listed};
  return scene_host<float>("hfcl_scene_collide_env_f32", s, moving_pose, n_conf, req, nullptr, out, summary, nullptr, nullptr, &cull);
}
int hfcl_scene_distance_env_f32(hfcl_scene* s, const float* moving_pose, size_t n_conf, double inflate, const hfcl_distance_request* req,
                                hfcl_result_f32* out, size_t out_capacity, uint32_t* pairs_out, uint64_t* conf_begin_out,
                                hfcl_scene_summary* summary, size_t* n_listed) {
  PAIRS_ENTRY;
  const SceneCull cull{ListKind::Env, inflate, out_capacity, nullptr, pairs_out, conf_begin_out, n_listed};
  return scene_host<float>("hfcl_scene_distance_env_f32", s, moving_pose, n_conf, nullptr, req, out, summary, nullptr, nullptr, &cull);
}

// ---- the clearance of the moving objects among the environment (include/hppfcl_amd_nearest_env.h) ---------------------------------------
int hfcl_scene_nearest_env(hfcl_scene* s, const double* moving_tf, size_t n_conf, const hfcl_distance_request* req, double upper_bound,
                           hfcl_scene_clearance* out, hfcl_result* min_records, size_t* n_evaluated) {
  PAIRS_ENTRY;
  return clearance_host<double>(ListKind::Env, "hfcl_scene_nearest_env", s, moving_tf, n_conf, req, upper_bound, out, min_records, n_evaluated);
}
int hfcl_scene_nearest_env_f32(hfcl_scene* s, const float* moving_pose, size_t n_conf, const hfcl_distance_request* req, double upper_bound,
                               hfcl_scene_clearance* out, hfcl_result_f32* min_records, size_t* n_evaluated) {
  PAIRS_ENTRY;
  return clearance_host<float>(ListKind::Env, "hfcl_scene_nearest_env_f32", s, moving_pose, n_conf, req, upper_bound, out, min_records, n_evaluated);
}
int hfcl_scene_nearest_env_device(hfcl_scene* s, const double* d_moving_tf, size_t n_conf, const hfcl_distance_request* req, double upper_bound,
                                  hfcl_scene_clearance* d_out, hfcl_result* d_min_records, size_t* n_evaluated, void* stream) {
  PAIRS_ENTRY;
  return clearance_device<double>(ListKind::Env, "hfcl_scene_nearest_env_device", s, d_moving_tf, n_conf, req, upper_bound, d_out, d_min_records, n_evaluated,
                                    (hipStream_t)stream);
}
int hfcl_scene_nearest_env_device_f32(hfcl_scene* s, const float* d_moving_pose, size_t n_conf, const hfcl_distance_request* req,
                                      double upper_bound, hfcl_scene_clearance* d_out, hfcl_result_f32* d_min_records, size_t* n_evaluated,
                                      void* stream) {
  PAIRS_ENTRY;
  return clearance_device<float>(ListKind::Env, "hfcl_scene_nearest_env_device_f32", s, d_moving_pose, n_conf, req, upper_bound, d_out, d_min_records,
                                   n_evaluated, (hipStream_t)stream);
}
#undef PAIRS_ENTRY

// ---- the per-configuration minimum distance with box-bound pruning -----------------------------------------------------------------
int hfcl_scene_nearest(hfcl_scene* s, const double* object_tf, size_t n_conf, const hfcl_distance_request* req, double upper_bound,
                       hfcl_scene_summary* summary, hfcl_result* min_records, size_t* n_evaluated) {
  return nearest_host<double>("hfcl_scene_nearest", s, object_tf, n_conf, req, upper_bound, summary, min_records, n_evaluated);
}
int hfcl_scene_nearest_f32(hfcl_scene* s, const float* object_pose, size_t n_conf, const hfcl_distance_request* req, double upper_bound,
                           hfcl_scene_summary* summary, hfcl_result_f32* min_records, size_t* n_evaluated) {
  return nearest_host<float>("hfcl_scene_nearest_f32", s, object_pose, n_conf, req, upper_bound, summary, min_records, n_evaluated);
}
int hfcl_scene_nearest_device(hfcl_scene* s, const double* d_object_tf, size_t n_conf, const hfcl_distance_request* req, double upper_bound,
                              hfcl_scene_summary* d_summary, hfcl_result* d_min_records, size_t* n_evaluated, void* stream) {
  return nearest_device<double>("hfcl_scene_nearest_device", s, d_object_tf, n_conf, req, upper_bound, d_summary, d_min_records, n_evaluated,
                                (hipStream_t)stream);
}
int hfcl_scene_nearest_device_f32(hfcl_scene* s, const float* d_object_pose, size_t n_conf, const hfcl_distance_request* req, double upper_bound,
                                  hfcl_scene_summary* d_summary, hfcl_result_f32* d_min_records, size_t* n_evaluated, void* stream) {
  return nearest_device<float>("hfcl_scene_nearest_device_f32", s, d_object_pose, n_conf, req, upper_bound, d_summary, d_min_records, n_evaluated,
                               (hipStream_t)stream);
}

// ---- a height-field terrain under the moving objects (include/hppfcl_amd_terrain.h) ----------------------------------------------------
int hfcl_scene_set_terrain(hfcl_scene* s, uint32_t hfield, const double* tf_terrain, const uint32_t* objects, size_t n_terrain_objects) {
  if (const int rc = no_device()) return rc;
  const char* who = "hfcl_scene_set_terrain";
  if (const int rc = groups_scene(who, s)) return rc;
  hfcl_lib* lib = s->lib;
  if (hfield >= lib->hf.h_fields.size()) {
    set_error(std::string(who) + ": not a height field of the scene's library (hfcl_lib_add_hfield)");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  if (!tf_terrain) {
    set_error(std::string(who) + ": null terrain pose");
    return HFCL_ERR_INVALID_ARGUMENT;
  }
  std::vector<uint32_t> list;
  if (!objects) {
    list.resize(s->rows());
    for (size_t o = 0; o < list.size(); ++o) list[o] = uint32_t(o);
  } else {
    for (size_t k = 0; k < n_terrain_objects; ++k) {
      if (objects[k] >= s->n_objects) {
        set_error(std::string(who) + ": object index " + std::to_string(objects[k]) + " is outside the " + std::to_string(s->n_objects) + " objects");
        return HFCL_ERR_INVALID_ARGUMENT;
      }
      if (k && objects[k] <= objects[k - 1]) {
        set_error(std::string(who) + ": the object list must ascend strictly (entry " + std::to_string(k) + ")");
        return HFCL_ERR_INVALID_ARGUMENT;
      }
    }
    list.assign(objects, objects + n_terrain_objects);
  }
  for (const uint32_t o : list) {
    const int32_t type = lib->h_shapes[s->h_object_shape[o]].type;
    if (!hfcl_hfield_pair_supported(type)) {
      set_error("Collision function between a height field and node type " + std::to_string(type) + " (object " + std::to_string(o) +
                ") is not yet supported.");
      return HFCL_ERR_UNSUPPORTED_PAIR;
    }
  }
  HIP_TRY(hipSetDevice(lib->device));
  DevBuf<uint32_t> d_list;
  DevBuf<double> d_tf;
  if (!list.empty())
    if (const int rc = groups_upload(d_list, list.data(), list.size())) return rc;
  if (const int rc = groups_upload(d_tf, tf_terrain, size_t(12))) return rc;
  // (freeing the old list waits for the device: a query in flight on some stream may still be reading it)
  s->d_terrain_objects = std::move(d_list);
  s->d_terrain_tf = std::move(d_tf);
  s->h_terrain_objects.swap(list);
  s->terrain_hfield = hfield;
  s->has_terrain = true;
  return HFCL_OK;
}
int hfcl_scene_clear_terrain(hfcl_scene* s) {
  if (const int rc = no_device()) return rc;
  if (const int rc = groups_scene("hfcl_scene_clear_terrain", s)) return rc;
  HIP_TRY(hipSetDevice(s->lib->device));
  s->d_terrain_objects.reset();  // (waits for the device)
  s->d_terrain_tf.reset();
  s->h_terrain_objects.clear();
  s->has_terrain = false;
  return HFCL_OK;
}
size_t hfcl_scene_n_terrain_objects(const hfcl_scene* s) { return s && s->has_terrain ? s->h_terrain_objects.size() : 0; }

int hfcl_scene_collide_terrain_device(hfcl_scene* s, const double* d_moving_tf, size_t n_conf, const hfcl_collision_request* req, hfcl_result* d_out,
                                      double* d_bounds, hfcl_scene_summary* d_summary, hfcl_contact* d_contacts, size_t max_contacts_total,
                                      size_t* n_contacts_out, void* stream) {
  if (const int rc = no_device()) return rc;
  QParams<double> q;
  bool skip_all = false, nothing = true;
  size_t total = 0;
  if (const int rc = terrain_validate("hfcl_scene_collide_terrain_device", s, d_moving_tf, n_conf, req,
                                      d_out || d_bounds || d_summary || d_contacts || n_contacts_out, n_contacts_out, q, skip_all, nothing, total))
    return rc;
  if (nothing) return HFCL_OK;
  hfcl_lib* lib = s->lib;
  HIP_TRY(hipSetDevice(lib->device));
  hipStream_t st = (hipStream_t)stream;
  const bool want_contacts = d_contacts || n_contacts_out;
  if (const int rc = terrain_run(s, d_moving_tf, n_conf, req, q, skip_all, d_out, d_bounds, d_summary, d_contacts, max_contacts_total, want_contacts,
                                 nullptr, nullptr, st))
    return rc;
  if (n_contacts_out && total) HIP_TRY(listed_contacts_back(lib->hf.ws, st, n_contacts_out));
  return HFCL_OK;
}

int hfcl_scene_collide_terrain(hfcl_scene* s, const double* moving_tf, size_t n_conf, const hfcl_collision_request* req, hfcl_result* out,
                               double* bounds, hfcl_scene_summary* summary, hfcl_contact* contacts, size_t max_contacts_total,
                               size_t* n_contacts_out) {
  if (const int rc = no_device()) return rc;
  const char* who = "hfcl_scene_collide_terrain";
  QParams<double> q;
  bool skip_all = false, nothing = true;
  size_t total = 0;
  if (const int rc = terrain_validate(who, s, moving_tf, n_conf, req, out || bounds || summary || contacts || n_contacts_out, n_contacts_out, q,
                                      skip_all, nothing, total))
    return rc;
  if (nothing) return HFCL_OK;
  hfcl_lib* lib = s->lib;
  auto& ws = lib->hf.ws;
  HIP_TRY(hipSetDevice(lib->device));
  if (!ws.st) HIP_TRY(ws.st.create());
  hipStream_t st = ws.st;
  if (total) {  // the table crosses the link once
    const size_t bytes = n_conf * s->rows() * 12 * sizeof(double);
    HIP_TRY(lib->scene.d_table.grow(bytes));
    HIP_TRY(hipMemcpyAsync(lib->scene.d_table, moving_tf, bytes, hipMemcpyHostToDevice, st));
  }
  const bool want_contacts = contacts || n_contacts_out;
  // the contact list of the whole call stays on the device until the last chunk has run (as hfcl_hfield_collide_batch)
  const size_t ccap = listed_contact_cap(contacts, max_contacts_total, total, req);
  if (ccap) HIP_TRY(ws.s_contacts.grow(ccap));
  if (summary) HIP_TRY(s->tw.d_summary.grow(n_conf));
  int rc = terrain_run(s, static_cast<const double*>(lib->scene.d_table.get()), n_conf, req, q, skip_all, nullptr, nullptr,
                       summary ? s->tw.d_summary.get() : nullptr, ccap ? ws.s_contacts.get() : nullptr, ccap, want_contacts, out, bounds, st);
  if (!rc) {
    bool ok = !summary || hipMemcpyAsync(summary, s->tw.d_summary, n_conf * sizeof(hfcl_scene_summary), hipMemcpyDeviceToHost, st) == hipSuccess;
    if (ok && want_contacts && total) ok = listed_contacts_back(ws, st, n_contacts_out, contacts, ccap) == hipSuccess;
    ok = ok && hipStreamSynchronize(st) == hipSuccess;
    if (!ok) {
      set_error(std::string(who) + ": HIP copy failed");
      rc = HFCL_ERR_HIP;
    }
  }
  hipStreamSynchronize(st);
  return rc;
}

}  // extern "C"
