// hfcl_host.hpp -- internal header of the host units (hfcl_host.hip: the library object, options, uploads, request set-up, the entry points
// and the host pipeline; hfcl_host_batch.hip: one device-resident batch -- workspace, stream sets, the dispatcher run_batch;
// hfcl_host_patch.hip: contact patches; hfcl_host_scene.hip: scene queries and the cull; hfcl_host_hfield.hip / hfcl_host_octree.hip:
// height fields and octrees, both over hfcl_host_listed.hpp): the library object and what the units call of each other.  Not included
// by the kernel units.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <map>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

#include "hfcl_dev.hpp"
#include "hfcl_launch.hpp"
#include "hfcl_patch.hpp"
#include "hfcl_scene.hpp"
#include "hfcl_cull.hpp"
#include "hfcl_pairs.hpp"
#include "hfcl_hfield.hpp"
#include "hfcl_octree.hpp"
#include "hfcl_octree_mesh.hpp"
#include "hfcl_own.hpp"

__attribute__((visibility("hidden"))) void set_error(const std::string& s);  // the calling thread's hfcl_last_error()

#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess) {                                                                   \
      set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                           \
      return HFCL_ERR_HIP;                                                                    \
    }                                                                                         \
  } while (0)

struct KernelTime {
  const char* name;
  Event e0, e1;
  bool used;
};

// Tables of a split traversal (BvhSplit): task table, unit summaries, suspended-query list, counters; the main set also the stack entries of
// cut walks (BvhSplit::cut_words / cut_vals, `cap` entries each).  n / cap: queries / tasks they are sized for (0: not allocated)
struct SplitTables {
  DevBuf<BvhTask> tasks;
  DevBuf<void> sums;
  DevBuf<uint32_t> susp, ctr, cut_words;
  DevBuf<double> cut_vals;
  size_t n = 0, cap = 0;
};
// Tables of a collide() walk in walk / leaves / resolve rounds (hfcl_dev.hpp: WalkRec): records, item list, leaf results, the query lists,
// counters (8 words per round; mesh x solid: then the 64 words of WalkArgs::hist), and `order`: BvhSplit::order of mesh x mesh (one entry
// per suspended slot), WalkArgs::perm of mesh x solid
struct WalkTables {
  DevBuf<void> recs;
  DevBuf<uint32_t> items;
  DevBuf<void> res;
  DevBuf<uint32_t> lists, ctr, order;
  size_t n = 0;
};

// Workspace of a call of the listed-leaf pipeline (hfcl_listed.hpp; the driver: hfcl_host_listed.hpp), one per kind on a library -- a
// height-field call and an octree call on two streams share nothing: the counts, offsets and box minima of a chunk of queries, its items
// and their leaf results, the call's running contact count, and of the host form its stream, its staging and the call's contact list
template <class Item, class Leaf>
struct ListedWs {
  DevBuf<uint32_t> d_counts, d_ccounts;
  DevBuf<uint64_t> d_offsets, d_coffsets, d_running;
  DevBuf<double> d_box_total;
  DevBuf<Item> d_items;
  DevBuf<Leaf> d_leaves;
  PinnedBuf<uint64_t> h_words;  // pinned: [0] a chunk's item count, [1] the call's contact count
  Stream st;
  DevBuf<uint32_t> s_id, s_shape;  // (s_id: the container ids)
  DevBuf<double> s_tf_a, s_tf_s, s_dlb;  // (s_tf_a: the containers' poses)
  DevBuf<uint8_t> s_swapped;
  DevBuf<hfcl_result> s_out;
  DevBuf<hfcl_contact> s_contacts;
};

// Everything hfcl_lib_set_option sets (hfcl_host.hip: apply_option): plain values, read when a batch is set up.  A split batch's helper takes
// its owner's block as it is (run_batch).
struct hfcl_options {
  uint32_t climb_min = HFCL_CLIMB_MIN;  // HFCL_CLIMB_MIN: hulls of at least this many vertices with a graph hill-climb
  // 0 in line; 1 the mesh walks beside the solids' GJK kernels; 2 also mesh x mesh beside mesh x solid, the solids' EPA section beside both
  // (1, 2: when the library's last batch held meshes and solids); 4: as 2 whatever the last batch held
  uint32_t mesh_beside = 2;
  bool mesh_prio = false;  // option mesh_prio = 1: the streams of the mesh x solid walks at the device's highest priority (read when they are created)
  uint32_t epa_direct_max = 4096;    // largest batch whose EPA seeds all go to the full-capacity tier, the fast tiers not launched (0: never)
  uint32_t gjk_beside_max = 120000;  // largest batch whose GJK kernels fan out (0: never; below the size from which batches run as two halves)
  bool epa_general_staged = false;       // HFCL_EPA_GENERAL_STAGED=1: prepare / loop / records for the general queues too.  Byte-identical
                                         // records; measured slower in wall-clock on cfg2 (0.416 -> 0.479 ms) and cfg5 unsplit (4.77 -> 5.30 ms
                                         // per 1M mixed pairs), faster only on cfg5 split (5.34 -> 5.13): profiles/r05_e_general_staged.md
  size_t epa_general_staged_min = 32768; // HFCL_EPA_GENERAL_STAGED_MIN
  bool records_aside = true;     // HFCL_EPA_RECORDS_ASIDE=0: k_epa_records on the batch's stream
  bool epa64_two_streams = true; // HFCL_EPA64_TWO_STREAMS=0: the two fp64 fast-tier kernels one after the other
  bool epa_cc_staged = true;     // HFCL_EPA_CC_STAGED=0: the one-kernel form (k_epa_stream<.., CC>)
  size_t epa_cc_staged_min = 32768;  // ... which batches below this many pairs keep (two launches less); HFCL_EPA_CC_STAGED_MIN
  // k_epa_loop's end-game pool (hfcl_epa_pool.hpp): percent of a batch's polytopes drawn by ticket instead of strided (0 - 50; 0: the static
  // schedule), in batches that give every wave at least epa_pool_min_refills full refills (tests: 0, so that a small batch draws too)
  uint32_t epa_pool_share = 20, epa_pool_min_refills = 2;
  bool shape_finish_tiers = true;  // HFCL_SHAPE_FINISH_TIERS=0: k_bvh_shape_finish in one launch at full capacity
  bool shape_finish_aside = true;  // HFCL_SHAPE_FINISH_ASIDE=0: all of k_bvh_shape_finish behind the last launch of k_bvh_shape_coop
  bool bvh_shape_lane = true;     // HFCL_BVH_SHAPE_LANE=0: the group kernels for every request (A/B switch)
  // step budgets of the one-query-per-lane mesh x solid walk (a unit suspends into tasks when it has taken that many BV-test
  // equivalents; a GJK leaf counts shape_leaf_cost): the queries themselves / their tasks.  The steps per query have a heavy
  // tail whatever the batch size (median 1, mean ~60, maximum > 3000 steps with > 1000 leaves), so the walk is always split.
  uint32_t shape_budget0 = 128, shape_budget = 96, shape_leaf_cost = 32, shape_levels = BVH_MAX_LEVELS;
  // Suspended queries are continued by k_bvh_shape_coop (a wave per query, 64 stack entries per trip) instead of task levels
  // (HFCL_SHAPE_COOP=0: the levels); the queries' own budget is then 16 steps (100k queries per kind, budgets 8 / 16 / 32 / 128:
  // sphere 2.0 / 2.0 / 2.4 / 2.6 ms, ellipsoid 7.5 / 8.1 / 8.4 / 8.3, box 1.4 / 1.3 / 1.2 / 1.1; profiles/r03_i)
  bool shape_coop = true;
  // ... and a walk such a kernel has worked on for this many clock ticks is cut into chunk tasks for its next launch (BvhSplit::cut_ticks;
  // HFCL_BVH_CUT_TICKS / HFCL_SHAPE_CUT_TICKS; 0: never).  The records equal the uncut walks' in every field wherever the cuts fall
  // (tools/cut_check.py).  mesh x solid, 600 000 ticks (~2.3x the mean walk): 100k mixed queries 4.4 -> 3.7 ms on one box, the single
  // kinds within +-5 %; shorter budgets lose (200 000: 3.5 against 3.3 at 400 000, 100 000: 6.8 ms -- every cut walks the chunks
  // behind a contact for nothing and pays three launches).  mesh x mesh: off -- its waves are busy 79 % of the kernel's time already
  // and cfg4 went 2.97 -> 3.18 ms (profiles/r04_j)
  uint32_t bvh_cut_ticks = 0, shape_cut_ticks = 350000;  // (600 000 until the queries' own phase became three kernels: profiles/r06_g section 5)
  uint32_t shape_budget0_coop = 16;
  // Mesh x mesh queries past their step budget are continued by k_bvh_coop (a wave per query, 64 stack entries per trip)
  // instead of task levels (HFCL_BVH_COOP=0: the levels).  cfg4, budgets 160 / 192 / 256 / 320 / 384: 100k queries 3.82 / 3.53 /
  // 3.28 / 3.39 / 3.57 ms (levels: 5.03); 1M queries, 256 / 512 / 640 / 1024: 15.1 / 10.95 / 10.86 / 11.9 ms (unsplit stream:
  // 14.7); 250k: 5.03 ms (8.78); 10k: 2.63 (3.74) -- profiles/r03_k.  HFCL_BVH_BUDGET0_COOP overrides both.
  bool bvh_coop = true;
  uint32_t bvh_budget0_coop = 0;  // 0: 256 steps up to 500k queries, 640 beyond
  // distance(): a mesh x mesh walk that has taken this many steps is continued by a wave (k_bvh_distance_coop); 0: never
  uint32_t bvhd_budget = 64;      // HFCL_BVHD_BUDGET: steps a lane walks before its walk goes to k_bvh_distance_pool (cfg4d 100k queries, budgets 16 / 64 / 256: 34.4 / 33.2 / 34.1 ms, profiles/r04_c; with the wave-per-walk form of round 3, HFCL_BVHD_POOL=0, 1024 was best: 55.7 ms)
  uint32_t bvhd_pool = 1;         // HFCL_BVHD_POOL: the walks past the budget are continued by k_bvh_distance_pool (0: k_bvh_distance_coop)
  uint32_t bvhd_pool_leaf_min = 24, bvhd_pool_starve = 32, bvhd_pool_part_min = 48;  // HFCL_BVHD_LEAF_MIN / HFCL_BVHD_STARVE / HFCL_BVHD_PART_MIN
  uint32_t pool_rerun = 1;          // HFCL_POOL_RERUN: pooled distance() walks whose result could hang on a rounding error are walked again in order (0: never -- the round-5 behaviour; 2: every walk, a test of the ordered mode)
  uint32_t shape_dist_pool = 1;     // HFCL_SHAPE_DIST_POOL: mesh x solid distance() walks past the budget continue in k_bvh_shape_distance_pool (0: k_bvh_shape_distance_coop)
  uint32_t shape_dist_leaf_min = 48, shape_dist_starve = 16;  // HFCL_SHAPE_DIST_LEAF_MIN / HFCL_SHAPE_DIST_STARVE (a GJK pass is worth waiting for: profiles/r04_i)
  uint32_t shape_dist_budget = 64;  // HFCL_SHAPE_DIST_BUDGET: the same for mesh x solid (a GJK leaf counts 16 steps; k_bvh_shape_distance_coop)
  size_t pipe_chunk = 0;                  // pairs per chunk (0 = automatic); HFCL_PIPE_CHUNK / hfcl_lib_set_host_chunk
  int split = 0;  // 0 = automatic (auto_split), 1 = never, 2 = always (large batches without meshes)
  // Queries per chunk of the cull (option scene_cull_chunk; 0: automatic -- at most 2^22 queries, 16384 workgroup counts for the one-workgroup scan)
  size_t scene_cull_chunk = 0;
  // hfcl_scene_self_pairs*: scenes of at most this many objects (option scene_pairs_small_max, at most PAIRS_SMALL_MAX) take the
  // wave-per-configuration form of the all-pairs test, larger ones the tiled form; both write the same bytes.  Measured: 16 objects x 2048
  // configurations 0.029 against 0.033 ms, 32 x 2048 0.040 against 0.047 - 0.050 ms, 64 x 256 0.051 against 0.027 ms -- a wave walks a
  // configuration's rows one after the other (profiles/r14_a_scene_pairs.md).  scene_cull_chunk is, for these calls, the rows
  // (configuration, object) per chunk, in whole row blocks
  uint32_t scene_pairs_small_max = 32;
  // hfcl_scene_self_pairs* and the _self host forms: option scene_pairs_sorted = 1 makes the same list by sort and sweep along one axis
  // (hfcl_pairs_sorted.hpp) for every scene of two objects or more, 0 (the default) never; option scene_pairs_sorted_axis: the sweep axis
  // 0 / 1 / 2, or 3 -- per configuration the axis on which the boxes' centres spread widest.  The list's bytes depend on neither.  With the
  // option set the device forms wait on their stream once per chunk (the count of the chunk's entries sizes the second sort)
  bool scene_pairs_sorted = false;
  uint32_t scene_pairs_sorted_axis = 3;
  // hfcl_scene_env_pairs*: column tiles per workgroup of the sweep (option scene_env_span; 0: automatic, hfcl_env.hpp: env_auto_span)
  uint32_t scene_env_span = 0;
  // hfcl_scene_nearest_env*: drop whole (row block, environment tile) cells of a pass by a bound of their distance (option
  // scene_nearest_env_prune; hfcl_nearest_env.hpp: nenv_tile_bound).  0: no cell is dropped by distance; the same bytes either way
  bool scene_nearest_env_prune = true;
  // Queries per chunk of a scene call (option scene_chunk; 0: automatic -- at most 2^21 queries, the call cut into equal chunks).  The chunks of a
  // call run one after the other, and the solvers' kernels are chains of dependent steps that fill the chip only with a large batch: cfg5's
  // 1.07 M queries in chunks of 262144 (the host pipeline's steady chunk) took 5.9 ms against 2.4 ms for the per-pair call on resident arrays,
  // 9.0 ms of kernel time against 5.5 (profiles/r08_a_scene.md).  2^21 queries are 0.8 GB of workspace, allocated only by calls that large.
  size_t scene_chunk = 0;
  // Queries per chunk of hfcl_hfield_collide_batch* (option hfield_chunk; 0: automatic -- 65536): bounds the per-query workspace; a chunk that
  // lists more than 2^20 (query, leaf) items is cut down further.  The records do not depend on it
  size_t hfield_chunk = 0;
  size_t hfield_items = 0;  // option hfield_items: the items a chunk may list before it is cut down (0: automatic -- 2^20); a chunk of one query is never cut
  // Queries per chunk of hfcl_octree_collide_batch* (option octree_chunk; 0: automatic -- 65536) and the items a chunk may list before it is
  // cut down (option octree_items; 0: automatic -- 2^20; a chunk of one query is never cut).  The records depend on neither
  size_t octree_chunk = 0;
  size_t octree_items = 0;
  int cvx_w = 0;  // 0 = per kernel (auto_cvx_w); HFCL_CVX_W forces one width for all
  bool closed_staged = true;  // HFCL_CLOSED_STAGED=0: A/B switch back to the direct-access k_closed<double>
  bool bvh_filter = false;     // HFCL_BVH_FILTER=1: the fp32 filter form of k_bvh_collide (exact, measured slower: profiles/r03_b)
  bool walk_order = true;            // option bvh_walk_order: the continuation launches draw the queries with the most stack entries first
  bool shape_walk_sort = true;       // option shape_walk_sort = 0: the listed leaves evaluated in the order the walks listed them
  bool shape_walk = true;            // option shape_walk = 0: the queries' own phase of mesh x solid collide() by k_bvh_collide's SOLID form (walk and leaves in one kernel)
  uint32_t shape_walk_budget = 256;  // box tests a query's walk may take before k_bvh_shape_coop continues it
  uint32_t shape_walk_min = 65536;   // batch size from which that phase is used (its eight launches are 0.2 ms of latency: 20k queries 1.63 against 1.42 ms,
                                     // 50k 1.96 / 1.82, 100k 2.43 / 2.70, 200k 3.55 / 4.16)
  size_t epa_resume_slots = 0, bvh_task_slots = 0;  // options epa_resume_slots / bvh_task_slots (0: sized by the batch)
  bool bvh_force_wide = false, pipe_trace = false;   // options bvh_force_wide / pipe_trace
  bool walk_early_coop = true;                               // HFCL_BVH_WALK_EARLY_COOP: the queries round 0 hands over are continued beside the later rounds
  // Rounds of walk / leaves / resolve (option bvh_walk_rounds; 0: k_bvh_collide walks the queries, leaves inline).  Not set: chosen per
  // batch -- ONE round of up to 16 listed leaves and 256 box tests (320 above 120 000 queries), then the continuation, up to 220 000 queries
  // (100k: 1.86 against 1.94 ms with two rounds, 20k: 1.20 against 1.78, 50k: 1.46 against 1.74: a round is as long as its longest lane,
  // and with the node records kept the lanes carry the walks far enough in one); TWO rounds (6 then 16 leaves; 320 -- above 500 000 queries
  // 640 -- then 256 box tests) with the first round's hand-overs continued beside the second above that (250k: 3.32 against 3.36-3.58 ms,
  // 400k: 4.78 against 4.92, 1M: 9.2 against 10.0 with one round).  profiles/r06_a section 6.  tests/test_bvh_plan_sizes_gpu.py
  bool walk_auto = true;
  uint32_t walk_rounds = 2;
  uint32_t walk_k[WALK_ROUNDS] = {6, 16, 16, 16};           // option bvh_walk_k: leaves a walk lists per round (setting it switches the automatic choice off)
  uint32_t walk_budget[WALK_ROUNDS] = {224, 256, 512, 512};  // option bvh_walk_budget: box tests per round from round 1 on before the walk goes to k_bvh_coop
  uint32_t bvh_budget0 = HFCL_BVH_BUDGET0;  // HFCL_BVH_BUDGET0: step budget of the queries (level 0); bvh_budget: of the tasks
  // No budget given by the environment: chosen per batch.  A batch that does not fill the chip's lanes more than ~1.5
  // times is a walk with one query per lane whose waves run on with most lanes finished; there the queries are cut at
  // 512 steps and their remainders spread over levels of small tasks (profiles/r02_w: 100k queries 6.4 -> 5.1 ms,
  // 10k 4.7 -> 3.4 ms).  A larger batch keeps its lanes busy by refilling and loses with the split (1M: 68 -> 51 M q/s).
  bool bvh_auto = true;
  uint32_t bvh_budget = HFCL_BVH_BUDGET, bvh_levels = HFCL_BVH_LEVELS;  // HFCL_BVH_BUDGET / HFCL_BVH_LEVELS (1: unsplit)
};

struct hfcl_lib {
  hfcl_options opt;
  // split traversals: the main set, and the set of the mesh x mesh walks of a batch that run beside its mesh x solid walks (no cut tables)
  SplitTables split_main, split_beside;
  // collide() walks in rounds: mesh x mesh; mesh x solid (their own: the two kinds of walks of a mixed batch run beside each other; lists: [2 n] + the redo list [n])
  WalkTables walk_mm, walk_ms;
  int device = 0;
  size_t n_shapes = 0;
  std::vector<hfcl_shape> h_shapes;
  std::vector<uint8_t> h_kinds;  // host copy of d_kinds: small host batches are classified on the host (host_batch)
  // The device shape tables and the adjacency image as the kernels' parameter blocks read them: a VIEW (share_tables) of what `own` of
  // the library holds -- a split batch's helper reads its owner's tables through the same fields and owns none
  const DShape<double>* d_shapes64 = nullptr;
  const DShape<float>* d_shapes32 = nullptr;
  const double* d_verts64 = nullptr;
  const float* d_verts32 = nullptr;
  const uint8_t* d_kinds = nullptr;
  struct GraphImage {
    DevBuf<uint32_t> base, off;
    DevBuf<NbrEntry<float>> ent32;
    DevBuf<NbrEntry<double>> ent64;
  };
  struct Tables {
    DevBuf<DShape<double>> shapes64;
    DevBuf<DShape<float>> shapes32;
    DevBuf<double> verts64;
    DevBuf<float> verts32;
    DevBuf<uint8_t> kinds;
    GraphImage graph;
  } own;
  // vertex adjacency of convex shapes (hfcl_lib_set_convex_neighbors): host copies per shape, device image built lazily
  std::vector<double> h_verts;
  struct HostGraph { std::vector<uint32_t> off, ids; };
  std::map<uint32_t, HostGraph> h_graphs;
  bool graph_dirty = false;
  const uint32_t* d_graph_base = nullptr;
  std::vector<GraphImage> graph_retired;  // adjacency images replaced by a later registration: batches in flight on other streams may still read
                                      // them, so they are freed where the library waits for the device anyway (set_shapes, destroy)
  Stream upload_stream;  // non-blocking stream of the adjacency upload (the host waits for it alone)
  const uint32_t* d_graph_off = nullptr;
  const NbrEntry<float>* d_graph_ent32 = nullptr;
  const NbrEntry<double>* d_graph_ent64 = nullptr;
  // workspace (grown on demand)
  size_t ws_capacity = 0;  // pairs
  size_t epa_capacity = 0;  // pairs the EPA queues / hand-over area are sized for (0: not allocated yet)
  DevBuf<uint32_t> d_lists;
  DevBuf<uint32_t> d_counts;
  DevBuf<void> d_epa_queue;
  DevBuf<void> d_epa_queue2;
  DevBuf<uint32_t> d_epa_cc_over;  // Work::epa_cc_over (resume_cap entries)
  DevBuf<uint32_t> d_redo;         // IO<float>::redo_list (ws_capacity entries; fp32 batches of libraries whose kernels mark)
  Stream aux;     // k_epa_records runs here, beside the tiers that continue the handed-over polytopes
  Stream mesh_st;  // the mesh walks of a mixed library's batch run here, beside the solids' kernels (option mesh_beside)
  Event ev_mesh_fork, ev_mesh_join;
  // ... the mesh x mesh walks of such a batch beside its mesh x solid walks (tables of their own: d_bvh2_*), and the helper stream the
  // mesh x solid walks use instead of `aux` (which the solids' EPA section, now beside them, uses)
  Stream mesh_st2, mesh_aux;
  bool ran_batch = false;  // h_counts holds the bucket counts of this library's last batch (once its copy has landed)
  Event ev_mesh_fork2, ev_mesh_join2;
  // the solids' GJK kernels of a small batch run beside each other on these (option gjk_beside_max): one bucket's kernel does not fill the chip
  Stream gjk_st[3];
  Event gjk_fork, gjk_join[3];
  Stream walk_st[WALK_ROUNDS - 1];  // mesh x mesh collide(): the continuation of what round r of the walk hands over runs on walk_st[r]
  Event walk_fork[WALK_ROUNDS - 1], walk_join[WALK_ROUNDS - 1];
  Event ev_aux0, ev_aux1, ev_aux2, ev_aux3;  // fork / join of the EPA tail; of k_bvh_shape_finish's first half
  DevBuf<void> d_epa_ready;   // EpaReady<float>[ws_capacity]: the staged convex x convex fast tier (k_epa_prepare / k_epa_loop / k_epa_records)
  DevBuf<void> d_epa_ready_g; // EpaReadyG<T>[ws_capacity]: the staged fast tier of the general queues (both precisions)
  DevBuf<void> d_epa_resume;
  DevBuf<void> d_epa_v0;
  size_t resume_cap = 0;
  DevBuf<void> d_shape_defer;  // ShapeDeferItem<double>[], two words more each: EPA queue of the one-query-per-lane mesh x solid form
  DevBuf<void> d_shape_oq;     // ObbQuery<double>[ws_capacity]: the solids' OBBs against the mesh poses, by pair
  DevBuf<void> d_dist_susp;    // DistSusp<double>[ws_capacity]
  DevBuf<void> d_shape_dist_susp;
  // host-call staging: PIPE_SLOTS device buffer sets of `st_capacity` pairs each (a chunk of a host batch), three streams
  // (H2D | kernels | D2H) and per-slot events / pinned counter blocks (host_batch)
  static constexpr int PIPE_SLOTS = 6;  // (three left the feeder waiting for records to leave: profiles/r03_c)
  struct Staging {
    DevBuf<uint32_t> d_s1, d_s2;
    DevBuf<double> d_tf1, d_tf2;
    DevBuf<double> d_qt1, d_qt2;  // compact host poses (7 doubles), expanded into d_tf1/2 on the device
    DevBuf<hfcl_result> d_out;
    DevBuf<hfcl_guess> d_gin, d_gout;
    Event ev_in, ev_in2, ev_done;  // inputs of object 1 / object 2 arrived, kernels done
    PinnedBuf<uint32_t> h_counts;  // pinned: bucket populations of the chunk that last ran in this slot
    PinnedBuf<uint32_t> h_counts2; // ... of its second half when the chunk ran split
    bool split = false;
  };
  Staging stage[PIPE_SLOTS];
  size_t st_capacity = 0;
  // small host batches (<= SMALL_MAX pairs): every input array packed into one pinned block and one device block (one
  // copy in, one copy out, one stream) instead of five copies and the pipeline's threads
  static constexpr size_t SMALL_MAX = 4096;
  PinnedBuf<char> h_pack;  // pinned
  DevBuf<char> d_pack;
  PinnedBuf<uint32_t> h_pack_counts;  // pinned: bucket populations of a small batch (and of its second half: never split)
  Stream s_h2d, s_h2d2, s_cmp, s_d2h;
  uint32_t acc_counts[N_COUNTERS] = {0};  // host batches: bucket populations summed over the chunks
  bool last_host = false;                 // the last call was a host batch: acc_counts are its populations
  bool in_host_batch = false;
  uint32_t* counts_dst = nullptr;         // where run_batch_one sends the bucket populations (default: h_counts)
  // instrumentation
  std::vector<KernelTime> timers;
  // A batch can run as two halves on two streams (hfcl_lib_set_split): the second half goes to `helper`, a shallow
  // clone (same device shape tables, own workspace / counters / timers) on the internal stream `side`, whose kernels
  // fill the drain phases of the first half's GJK / EPA launches (profiles/r01_k_two_stream_overlap.txt).
  hfcl_lib* helper = nullptr;
  bool last_split = false;  // the last batch ran split: counters / timers of the helper belong to it
  Stream side;
  Event ev_fork, ev_join;
  bool kernel_timing = true;         // HIP events around every kernel (hfcl_lib_set_kernel_timing)
  // contact patches (hfcl_contact_patch_batch*): workspace slots, class lists, their counters; staging of the host form
  DevBuf<void> d_patch_ws;
  DevBuf<uint32_t> d_patch_lists;
  DevBuf<uint32_t> d_patch_counts;
  Stream patch_st;
  // scene queries (hfcl_scene_*): the workspace of a chunk of queries -- expanded ids and poses, two record / guess buffers (summary-only
  // calls and the host form), the fold's partials --, the host form's object table and summaries, its two streams and per-chunk counters
  struct SceneWs {
    DevBuf<uint32_t> d_s1, d_s2;
    DevBuf<void> d_tf1, d_tf2;
    size_t cap = 0;                 // queries the four arrays above hold
    DevBuf<void> d_rec[2];          // (records of 96 B in either precision)
    DevBuf<hfcl_guess> d_gin, d_gout[2];
    DevBuf<hfcl_scene_summary> d_partials;
    DevBuf<void> d_table;        // host form: the object pose table
    DevBuf<hfcl_scene_summary> d_summary;
    Stream s_cmp, s_copy;
    Event ev_done[2], ev_copied[2];
    static constexpr int COUNT_SLOTS = 8;
    PinnedBuf<uint32_t> h_counts;   // pinned: COUNT_SLOTS x 2 * N_COUNTERS words of the host form (a chunk, its second half when it ran split);
                                    // chunk k uses slot k % COUNT_SLOTS once chunk k - COUNT_SLOTS has been added up (ev_counts: its kernels are done)
    Event ev_counts[COUNT_SLOTS];
    // culling the pair list (hfcl_scene_cull*): world boxes of the configurations a chunk touches (host forms of hfcl_scene_world_aabbs: of
    // the whole table), ballots / workgroup counts / offsets of a chunk, the running count, and the list of the host forms
    DevBuf<double> d_boxes;         // (6 doubles a box)
    DevBuf<uint64_t> d_words;
    DevBuf<uint32_t> d_block_counts;
    DevBuf<uint64_t> d_block_offsets;
    size_t blocks_cap = 0;
    DevBuf<uint64_t> d_running;  // [0]: the running count of a cull, [1]: n_listed of the host forms
    DevBuf<uint64_t> d_ids;      // host forms: the surviving queries
    DevBuf<uint64_t> d_conf_begin;
    // the pruned minimum distance (hfcl_scene_nearest*): the second pass's list, the seeds and thresholds by configuration, both passes'
    // records when min records are asked for, and the host forms' min records
    DevBuf<uint64_t> d_ids2, d_conf_begin2;
    DevBuf<uint32_t> d_seed;
    DevBuf<void> d_seed_partials;
    DevBuf<double> d_thr;
    DevBuf<void> d_nrec[2];
    DevBuf<void> d_minrec;
    // the self-collision pairs (hfcl_scene_self_pairs*): counts and offsets of a chunk's rows, the sums of its scan workgroups and the
    // entries before them, and the list of the host forms
    DevBuf<uint32_t> d_row_counts, d_row_sums;
    DevBuf<uint64_t> d_row_offsets, d_row_sum_offsets;
    size_t rows_cap = 0;
    DevBuf<uint32_t> d_pair_list;  // (two words an entry)
    // ... by sort and sweep (option scene_pairs_sorted): of a chunk of whole configurations the words as made and sorted with their
    // objects, the grown boxes, groups and window ends in sorted order, the axis of a configuration and the centre ranges behind it, the
    // entries' words as emitted and sorted, and the sorts' temporary storage
    DevBuf<uint64_t> d_ps_keys[2], d_ps_emit[2];
    DevBuf<uint32_t> d_ps_vals[2], d_ps_ends, d_ps_axis;
    DevBuf<double> d_ps_boxes, d_ps_spread;
    DevBuf<uint8_t> d_ps_group;
    DevBuf<void> d_ps_temp;
    // the clearance on device-made pairs (hfcl_scene_nearest_self*): a row seed per row of the table, seed and threshold by
    // configuration, per pass the list of pairs with its conf_begin, its summaries and -- when min records are asked for -- its records,
    // and the host forms' clearances
    DevBuf<void> d_ns_row_seeds;
    DevBuf<uint64_t> d_ns_seed;
    DevBuf<double> d_ns_thr;
    DevBuf<uint32_t> d_ns_list[2];  // (two words an entry)
    DevBuf<uint64_t> d_ns_conf_begin[2];
    DevBuf<hfcl_scene_summary> d_ns_summary[2];
    DevBuf<void> d_ns_rec[2];
    DevBuf<hfcl_scene_clearance> d_ns_out;
  } scene;
  // height fields (hfcl_lib_add_hfield; hfcl_host_hfield.hip): the host tables of every registered field one after the other, their device
  // images (uploaded by the next call when a field was added since), and the workspace of their calls (the terrain calls of a scene use it too)
  struct Hfields {
    std::vector<DHfield> h_fields;
    std::vector<hfcl_hfield_node> h_nodes;
    std::vector<double> h_heights, h_xgrid, h_ygrid;
    bool dirty = false;
    DevBuf<DHfield> d_fields;
    DevBuf<hfcl_hfield_node> d_nodes;
    DevBuf<double> d_heights, d_xgrid, d_ygrid;
    ListedWs<HfItem<double>, HfLeafOut<double>> ws;
  } hf;
  // octrees (hfcl_lib_add_octree; hfcl_host_octree.hip): the host tables of every registered tree one after the other, their device
  // images (uploaded by the next call when a tree was added or its thresholds set since), and the workspace of their calls
  struct Octrees {
    std::vector<DOctree> h_trees;
    std::vector<hfcl_octree_node> h_nodes;
    bool dirty = false;
    DevBuf<DOctree> d_trees;
    DevBuf<hfcl_octree_node> d_nodes;
    ListedWs<OctItem<double>, OctLeafOut<double>> ws;
    // ... against meshes (hfcl_octree_mesh_collide_batch*): a workspace of its own kind of items, and the levels of every registered
    // mesh's BVH (hfcl_octree_mesh.hpp: octm_bvh_depth), computed by the first call that needs them
    ListedWs<OctMeshItem<double>, OctMeshLeafOut<double>> ws_mesh;
    std::vector<uint32_t> mesh_depth;
  } oct;
  // local AABB of every library shape (hfcl_cull.hpp: shape_local_box; BVH models: the box of their vertices), 6 doubles each, rebuilt when
  // shapes or meshes were registered since (hfcl_lib_set_shapes, hfcl_lib_add_bvh)
  DevBuf<double> d_local_boxes;
  bool local_boxes_dirty = true;
  std::vector<uint32_t> h_mesh_nverts;  // vertices of each registered BVH model
  uint64_t shapes_epoch = 0;        // hfcl_lib_set_shapes counts: a scene made before the last one is stale
  uint32_t possible_buckets = ~0u;   // bit b: some pair of this library's shape kinds classifies into bucket b
  bool has_flats = true;             // some shape is a Plane / Halfspace: their "very rough" volumes are no lower bounds, so what a mesh walk
                                     // against them reports depends on the ORDER of its visits -- the ordered continuation, not the pool
  bool has_capsules = true;          // some shape is a Capsule: the closed form that marks nearly parallel pairs can occur (closed_form_suspect)
  bool has_curved = true;            // some shape is an Ellipsoid / Cone / Cylinder: the curved class of the fp64 EPA tiers can occur
  int n_cus = 256;
  std::string dominant;
  // (diagnostic, off unless hfcl_debug_note_forms switched it on) what the host entry point chose for the last host call (its chunks) and
  // what the dispatcher chose for the last batch, one "name=value;" per decision (note_form; hfcl_debug_last_forms)
  bool note_forms = false;
  std::string form_notes, host_notes, notes_out;
  // bucket populations of the last call; PINNED host memory so that the device-to-host copy at the end of a batch is
  // asynchronous (a pageable destination makes hipMemcpyAsync block the host until the whole batch has run)
  PinnedBuf<uint32_t> h_counts;
  // BVH models (host staging + device images in both precisions; uploaded lazily)
  std::vector<hfcl_bvh_node> h_bvh_nodes;
  std::vector<double> h_bvh_verts;
  std::vector<uint32_t> h_bvh_tris;
  std::vector<DMesh> h_meshes;
  bool bvh_dirty = false;
  DevBuf<DNode<double>> d_nodes64;
  DevBuf<DNode<float>> d_nodes32;
  DevBuf<DNodeF> d_fnodes;  // 64-byte records of the fp32 separating-axis filter (fp64 collide)
  DevBuf<DRss<double>> d_rss64;
  DevBuf<DRss<float>> d_rss32;
  DevBuf<DNodeD<double>> d_dnodes64;  // the distance() walk's packed node records
  DevBuf<DNodeD<float>> d_dnodes32;
  DevBuf<double> d_bverts64;
  DevBuf<float> d_bverts32;
  DevBuf<uint32_t> d_btris;
  DevBuf<DMesh> d_meshes;
  // models too large (> 65535 nodes) or too deep for the LDS stacks: 32-bit node ids + per-lane global slabs (BvhSpill)
  uint32_t bvh_max_depth = 0;
  size_t bvh_max_nodes = 0;
  DevBuf<void> d_bvh_slab;
  // contact list of the last hfcl_collide_batch_contacts call
  DevBuf<hfcl_contact> d_contacts;
  DevBuf<uint32_t> d_contacts_count;
  BvhParams bvh_params = {1u, nullptr, 0u, nullptr};
  double break_distance = 1e-3;
};

// (diagnostic) one decision of the dispatcher about the batch being set up: the form it takes, a budget or a table size as the kernels get it
inline void note_form(hfcl_lib* lib, const char* name, unsigned long long value) {
  if (!lib->note_forms) return;
  lib->form_notes += name;
  lib->form_notes += '=';
  lib->form_notes += std::to_string(value);
  lib->form_notes += ';';
}

// bucket population i of a batch's counter block: a bucket = its bottom + its curved part; the EPA queue = the general + the second queue
inline uint32_t one_count(const uint32_t* c, int i) {
  return c[i] + (i < B_COUNT ? c[B_CURVED0 + i] : 0u) + (i == B_COUNT ? c[B_COUNT + 3] : 0u);
}

// A host call whose chunks go through the device batch entry points, for its duration: the populations of the chunks are summed into
// acc_counts, run_batch_one sends a chunk's where counts_dst points.  Declared before the call enqueues anything, so that it ends after
// the call's streams have been waited for and its threads joined.
struct HostBatchScope {
  hfcl_lib* lib;
  explicit HostBatchScope(hfcl_lib* l) : lib(l) {
    memset(lib->acc_counts, 0, sizeof(lib->acc_counts));
    lib->in_host_batch = true;
  }
  ~HostBatchScope() {
    lib->in_host_batch = false;
    lib->counts_dst = nullptr;
    if (lib->helper) lib->helper->counts_dst = nullptr;
  }
  HostBatchScope(const HostBatchScope&) = delete;
  HostBatchScope& operator=(const HostBatchScope&) = delete;
};

// what the units call of each other (internal to the shared library: hidden)
#pragma GCC visibility push(hidden)
// hfcl_host_batch.hip
template <typename T> int run_batch(hfcl_lib* lib, const uint32_t* d_s1, const uint32_t* d_s2, IO<T> io, size_t n, QParams<T> q, hipStream_t st);
void share_tables(hfcl_lib* h, const hfcl_lib* lib);  // the view of `h` onto the device tables `lib` owns (h == lib: the library's own)
bool batch_splits(const hfcl_lib* lib, size_t n);
int ensure_helper(hfcl_lib* lib);
// hfcl_host.hip
extern "C" int host_batch_checks(hfcl_lib* lib, const hfcl_collision_request* creq, const hfcl_distance_request* dreq);  // (defined among hfcl_host.hip's extern "C" entry points)
template <typename T> int setup_collide(const hfcl_collision_request* req, QParams<T>& q, bool& skip_all);
template <typename T> int setup_distance(const hfcl_distance_request* req, QParams<T>& q);
KernelTime* timer_slot(hfcl_lib* lib, size_t i, const char* name);
int upload_graph(hfcl_lib* lib);
int upload_bvh(hfcl_lib* lib);
int no_device();  // HFCL_ERR_NO_DEVICE (with its error text) or 0
// hfcl_host_hfield.hip: the height-field call's own pieces, which the terrain calls of the scene unit run their chunks through.
// hf_request: what every form checks of a request before any work (q: hf_leaf_params of it); hf_chunk: queries per chunk (option
// hfield_chunk); hf_run: queries [0, n) on device pointers in chunks (hfcl_host_listed.hpp: listed_run) -- pair0: the index of query 0 in
// the caller's batch, first: this is the first part of that batch (the running contact count, lib->hf.ws.d_running, starts at 0)
int hf_request(const char* who, const hfcl_collision_request* req, QParams<double>& q, bool& skip_all);
size_t hf_chunk(const hfcl_lib* lib);
int hf_run(hfcl_lib* lib, const uint32_t* d_hfield, const uint32_t* d_shape, const double* d_tfh, const double* d_tfs, size_t n,
           const uint8_t* d_swapped, const hfcl_collision_request* req, const QParams<double>& q, bool skip_all, hfcl_result* d_out, double* d_dlb,
           hfcl_contact* d_contacts, size_t contacts_cap, bool want_contacts, uint32_t pair0, bool first, hipStream_t st);
// hfcl_host_scene.hip: the library's local boxes on the device (lib->d_local_boxes), rebuilt when shapes or meshes were registered since
int ensure_local_boxes(hfcl_lib* lib);
#pragma GCC visibility pop

// ---- the calls of the listed-leaf pipeline: what the height-field, octree and terrain entry points share of their contact lists ----
constexpr uint64_t LISTED_ITEM_HARD_CAP = 1u << 26;  // leaves one query may list (7 GB of item workspace); no query yields more contacts
// The contact list of a whole host call stays on the device until the last chunk has run: room for at most what its n queries can
// produce (a query adds at most num_max_contacts contacts, and no more than the 2^26 leaves it may list).  No list asked for: 0
inline size_t listed_contact_cap(const hfcl_contact* contacts, size_t max_contacts_total, size_t n, const hfcl_collision_request* req) {
  return contacts ? std::min(max_contacts_total, n * size_t(std::min<uint64_t>(req->num_max_contacts, LISTED_ITEM_HARD_CAP))) : 0;
}
// After the last chunk of a call: its contact count (w.d_running) read through w.h_words[1] -- st is waited for -- into *n_contacts_out
// where given; contacts: then the stored ones, at most ccap, from w.s_contacts to the host.  The first HIP error, or hipSuccess
template <class Ws>
hipError_t listed_contacts_back(Ws& w, hipStream_t st, size_t* n_contacts_out, hfcl_contact* contacts = nullptr, size_t ccap = 0) {
  hipError_t e = hipMemcpyAsync(w.h_words.get() + 1, w.d_running, sizeof(uint64_t), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return e;
  const size_t total = size_t(w.h_words[1]);
  if (n_contacts_out) *n_contacts_out = total;
  const size_t stored = contacts ? std::min(total, ccap) : 0;
  return stored ? hipMemcpy(contacts, w.s_contacts, stored * sizeof(hfcl_contact), hipMemcpyDeviceToHost) : hipSuccess;
}
