// hfcl_launch.hpp -- host-callable launchers of the HIP kernels.  One translation unit per kernel family, so that a
// change to one kernel recompiles in parallel with nothing else and A/B builds of a single family are cheap:
//
//   hfcl_k_gjk.hip   k_classify       pair -> bucket lists (block-aggregated atomics), one pass over the shape ids
//                    k_closed<T>      closed forms (sphere / capsule / cylinder / box-sphere pairs, every Plane /
//                                     Halfspace row), one pair per lane (fp64: poses / records staged through LDS)
//                    k_gjk_prim<T>    GJK for Box/Capsule/Cone/Cylinder/Ellipsoid/Sphere pairs, one pair per lane
//                    k_gjk_cvx<W,M>   GJK with hulls of <= 32 vertices: one pair per W-lane group, hull vertices in the
//                                     group's registers, support = per-lane dots + DPP-butterfly arg-max
//                    k_gjk_large<T>   GJK when a hull has more than 32 vertices (scan / hill-climb from memory)
//                    k_unsupported<T>, k_fill_skipped
//   hfcl_k_epa.hip   k_epa<T,WE,CAP,TIER>, k_epa_stream<T,WE,CAP>   EPA on the pairs GJK left in `Collision`
//                    k_epa_prepare / k_epa_loop / k_epa_records   the fp32 convex x convex fast tier in three stages
//   hfcl_k_bvh.hip   k_bvh_collide<T>   BVHModel<OBBRSS> x BVHModel<OBBRSS> collide(), one query per lane for a step budget
//                                     (hfcl_mesh_collide.hpp: what this source shares with hfcl_k_bvhc.hip, this kernel among it);
//                                     k_bvh_coop<T>: the queries past it, a wave each, 64 stack entries per trip
//                                     (BvhSplit::cut_ticks: a walk a wave has had for that long is cut into chunk tasks for the kernel's next
//                                     launch, k_bvh_combine folds them back; on for mesh x solid, k_bvh_shape_coop)
//                                     (k_bvh_combine<T>: the task-level alternative)
//   hfcl_k_bvhd.hip  k_bvh_distance<T>  ... distance(), one query per lane for a step budget (this unit is built without
//                                     contraction: triangle ids equal to the reference's); k_bvh_distance_pool<T, PQ>: the walks past
//                                     it, PQ per wave, their box and triangle tests pooled, DFS order kept by a marker
//                                     (k_bvh_distance_coop<T>: the ordered wave-per-walk form)
//   hfcl_k_bvhc.hip  k_shape_obb<T>, k_bvh_collide<T, ., ., SOLID>, k_bvh_shape_coop<T>, k_bvh_shape_finish<T>
//                                     BVHModel<OBBRSS> x convex solid, first-contact collide(): the solids' OBBs, the walk
//                                     (lane, then wave), the leaves that need EPA
//   hfcl_k_bvhs.hip  k_shape_obbrss<T>, k_bvh_shape_distance_lane<T>, k_bvh_shape_distance_pool<T>   ... distance() (a source of its own;
//                                     hfcl_mesh.hpp: what it shares with the two collide() sources, k_bvh_shape_finish among it)
//                                     (k_bvh_shape_distance_coop<T>: the ordered form, libraries with a Plane / Halfspace)
//                    k_bvh_shape<T> (hfcl_k_bvhc.hip) / k_bvh_shape_distance<T>   the same rows, one 16-lane group per query: requests
//                                     that keep walking after a contact, models deeper than the lanes' stacks
//   hfcl_k_bvh.hip   k_triangle<T>    top-level TriangleP pairs
//
// Every launcher is asynchronous on `st` and does no error checking of its own (hfcl_host_batch.hip: run_batch_one checks hipGetLastError once, in its last stage).
#pragma once
#include "hfcl_dev.hpp"

void launch_classify(int grid, hipStream_t st, const Work& wk, const uint8_t* kinds, uint32_t n_shapes, bool distance_mode);
template <typename T> void launch_unsupported(int grid, hipStream_t st, const Work& wk, const IO<T>& io, int bucket);
template <typename T> void launch_closed(int grid, hipStream_t st, const Work& wk, const LibView<T>& lv, const IO<T>& io, const QParams<T>& q, bool staged);
template <typename T> void launch_gjk_prim(int grid, hipStream_t st, const Work& wk, const LibView<T>& lv, const IO<T>& io, const QParams<T>& q, bool bvg);
// m: 0 = convex-convex, 1 = prim-convex, 2 = convex-prim; w: lanes per pair (2 / 4 / 8 / 16 / 32 / 64)
// grid: workgroups of gjk_cvx_threads<T>(w, m) threads
template <typename T> constexpr int gjk_cvx_threads(int w, int m) { return (sizeof(T) == 4 && w == 2 && m == 0) ? 64 : 256; }
template <typename T> void launch_gjk_cvx(int m, int w, bool bvg, int grid, hipStream_t st, const Work& wk, const LibView<T>& lv, const IO<T>& io, const QParams<T>& q);
template <typename T> void launch_gjk_large(int grid, hipStream_t st, const Work& wk, const LibView<T>& lv, const IO<T>& io, const QParams<T>& q, bool bvg);
// 7-double (quaternion w,x,y,z + translation) poses -> 12-double Transform3f images
void launch_expand_poses(hipStream_t st, const double* qt, double* tf, uint32_t n);
void launch_fill_skipped(hipStream_t st, hfcl_result* out, uint32_t n);
void launch_fill_skipped(hipStream_t st, hfcl_result_f32* out, uint32_t n);
// hfcl_k_util.hip: full records -> compact records (hfcl_result_compact{,_f32})
void launch_compact_records(hipStream_t st, const hfcl_result* in, hfcl_result_compact* out, uint32_t n);
void launch_compact_records(hipStream_t st, const hfcl_result_f32* in, hfcl_result_compact_f32* out, uint32_t n);

// tier 1 (fp32: streaming form) and tier 2 of EPA; the grids are in blocks of one wavefront
// cc_queue / general_queue (fp32): which of the two streaming forms have anything to do (convex x convex pairs have a
// queue and a kernel of their own); curved_class (fp64): the library has a shape whose support is not a vertex, i.e. the
// curved class of pairs -- a queue and a fast-tier kernel of its own -- can occur
// st2 (fp64, both classes present): the polytope-class kernel goes there, beside the curved-class kernel on st (the caller forks and joins)
template <typename T> void launch_epa_fast(int grid, hipStream_t st, const Work& wk, const LibView<T>& lv, const IO<T>& io, const QParams<T>& q, bool cc_queue, bool general_queue, int n_cus, bool curved_class = true, hipStream_t st2 = nullptr);
// the fp32 convex x convex fast tier in three stages (Work::epa_ready set): one lane per polytope before and after the loop kernel
void launch_epa_prepare(int grid, hipStream_t st, const Work& wk, const LibView<float>& lv, const IO<float>& io, const QParams<float>& q);
void launch_epa_loop(int grid, hipStream_t st, const Work& wk, const LibView<float>& lv, const QParams<float>& q, int n_cus, uint32_t pool_share, uint32_t pool_min_refills);
void launch_epa_resume_cc(int grid, hipStream_t st, const Work& wk, const LibView<float>& lv, const IO<float>& io, const QParams<float>& q);
void launch_epa_records(int grid, hipStream_t st, const Work& wk, const LibView<float>& lv, const IO<float>& io, const QParams<float>& q);
// ... and for pairs of any convex kinds, both precisions (Work::epa_ready_g set)
template <typename T> void launch_epa_prepare_general(int grid, hipStream_t st, const Work& wk, const LibView<T>& lv, const IO<T>& io, const QParams<T>& q, bool skip_top);
template <typename T> void launch_epa_loop_general(int grid, hipStream_t st, hipStream_t st2, const Work& wk, const LibView<T>& lv, const QParams<T>& q, int n_cus, bool curved_class);
template <typename T> void launch_epa_records_general(int grid, hipStream_t st, const Work& wk, const LibView<T>& lv, const IO<T>& io, const QParams<T>& q, bool skip_top);
template <typename T> void launch_epa_requeue(hipStream_t st, const Work& wk);
template <typename T> void launch_epa_full(int grid, hipStream_t st, const Work& wk, const LibView<T>& lv, const IO<T>& io, const QParams<T>& q);

// A helper stream with its fork / join events: k_bvh_shape_finish for the items of whole walks runs there, beside the launches that walk the
// chunks of the cut ones; k_bvh_coop for the queries round 0 of a mesh x mesh walk handed over, beside the later rounds
struct AsideStream {
  hipStream_t stream;
  hipEvent_t fork, join;
};
// split: the task tables of a split traversal (tasks == nullptr: single pass)
// aside: nullptr, or WALK_ROUNDS - 1 helper streams (the continuation of what round r of the walk hands over runs on aside[r])
template <typename T> void launch_bvh_collide(int grid, hipStream_t st, const Work& wk, const LibView<T>& lv, const BvhView<T>& bv, const IO<T>& io, const QParams<T>& q, const BvhParams& bp, T break_distance2, BvhSplit split, BvhSpill spill, const AsideStream* aside = nullptr);
template <typename T> void launch_bvh_distance(int grid, hipStream_t st, const Work& wk, const LibView<T>& lv, const BvhView<T>& bv, const IO<T>& io, const QParams<T>& q, BvhSpill spill);
template <typename T> void launch_bvh_shape(int grid, hipStream_t st, const Work& wk, const LibView<T>& lv, const BvhView<T>& bv, const IO<T>& io, const QParams<T>& q, const BvhParams& bp, T break_distance2);
template <typename T> void launch_bvh_shape_distance_fast(int grid, int grid_finish, hipStream_t st, const Work& wk, const LibView<T>& lv, const BvhView<T>& bv, const IO<T>& io, const QParams<T>& q, BvhSpill spill);
template <typename T> void launch_bvh_shape_fast(int grid, int grid_finish, int coop_grid, hipStream_t st, const Work& wk, const LibView<T>& lv, const BvhView<T>& bv, const IO<T>& io, const QParams<T>& q, const BvhParams& bp, T break_distance2, BvhSplit split, BvhSpill spill, const AsideStream* aside = nullptr);
template <typename T> void launch_bvh_shape_distance(int grid, hipStream_t st, const Work& wk, const LibView<T>& lv, const BvhView<T>& bv, const IO<T>& io, const QParams<T>& q);
// hfcl_k_redo.hip: the pairs an fp32 batch marked as inconsistent (IO<float>::redo_list), solved again in fp64 from the fp64 tables and the
// promoted fp32 poses; the record rounded to the 44-byte form.  The grid strides over the device-side count.
void launch_redo(int grid, hipStream_t st, const Work& wk, const DShape<double>* shapes64, const double* verts64, const IO<float>& io, const QParams<double>& q);
template <typename T> void launch_triangle(int grid, hipStream_t st, const Work& wk, const LibView<T>& lv, const IO<T>& io, const QParams<T>& q);

// hfcl_k_patch.hip: contact patches of collide() records (hfcl_contact_patch_batch*).  lists: 2 x n record ids (one-sided,
// clipped), counts: their 2 lengths, zeroed by the caller; ws: nslots workspace slots of slot_bytes (hfcl_patch.hpp: PatchWs)
struct PatchArgs {
  const uint32_t* s1;
  const uint32_t* s2;
  const double* tf1;
  const double* tf2;
  const hfcl_result* rec;
  const hfcl_guess* guess;
  uint32_t n, n_shapes;
  const DShape<double>* shapes;
  const double* verts;
  const uint32_t* graph_base;
  const uint32_t* graph_off;
  const uint32_t* graph_ent;  // NbrEntry<double> image as 32-bit words
  uint32_t max_num_patch, num_samples;
  double tol;
  uint32_t pcap, plim;  // points per record in out_pts (row stride), points a record may have
  hfcl_contact_patch* out;
  double* out_pts;
  uint32_t* lists;
  uint32_t* counts;
  char* ws;
  size_t slot_bytes;
  uint32_t nslots, cap, cloud_cap, vis_cap;
};
// three launches (classify, one-sided, clipped); names / e0 / e1: three entries (e0 == nullptr: no timing)
void launch_patch(hipStream_t st, const PatchArgs& a, int max_blocks, const char** names, hipEvent_t* e0, hipEvent_t* e1);

// hfcl_k_scene.hip: scene queries (hfcl_scene_*).  A chunk [q0, q0 + m) of the flat query range q = c * n_pairs + p ...
struct SceneExpandArgs {
  const uint32_t* pairs;         // 2 x n_pairs object indices
  const uint32_t* object_shape;  // n_objects shape ids
  const void* object_tf;         // n_conf x n_objects pose rows (12 doubles / 7 floats)
  uint64_t n_objects;
  uint32_t n_pairs;
  uint64_t q0;
  uint64_t c0;                   // (c0, p0) = scene_query(q0)
  uint32_t p0;
  uint32_t m;
  uint32_t* s1;
  uint32_t* s2;
  void* tf1;                     // m rows each, 16-byte aligned
  void* tf2;
};
// ... -> the per-pair arrays of run_batch
void launch_scene_expand(hipStream_t st, const SceneExpandArgs& a, bool f32, int max_blocks);
struct SceneFoldArgs {
  const void* rec;               // the chunk's records (hfcl_result / hfcl_result_f32): rec[0] is query q0's
  uint64_t q0, q1;
  uint32_t n_pairs;
  uint64_t g0;                   // first piece of the chunk (hfcl_scene.hpp: scene_piece_of(q0)) and how many it touches
  uint64_t n_pieces;
  double margin;                 // collide: the request's security margin
  int collide;
  hfcl_scene_summary* summary;   // by configuration
  hfcl_scene_summary* partials;  // nullptr (pair lists of one piece) or n_pieces slots
};
// ... -> the summaries of the configurations it touches (one launch, or two when a pair list has several pieces)
void launch_scene_fold(hipStream_t st, const SceneFoldArgs& a, bool f32, int max_blocks);

// hfcl_k_cull.hip: culling a scene's pair list per configuration (hfcl_scene_cull*) and the scene calls on the list that is left
// (hfcl_scene_*_listed*).  World boxes of n_rows = configurations x objects pose rows (row r: object r % n_objects), 48 B each
void launch_cull_aabbs(hipStream_t st, const void* object_tf, bool f32, const uint32_t* object_shape, const double* local_boxes,
                       uint64_t n_objects, uint64_t n_rows, double* boxes);
// A chunk [q0, q0 + m) of the flat query range: mark (a lane per query: a ballot per wave, a count per workgroup), scan (the counts, on
// top of the survivors of the chunks before: *running), emit (the surviving q at their ranks, conf_begin of the configurations that start in
// the chunk).  Three ordered launches; no kernel waits for another workgroup.
struct CullArgs {
  const uint32_t* pairs;     // 2 x n_pairs object indices
  const double* boxes;       // world boxes of the configurations [c_box0, ...) the chunk touches
  uint64_t c_box0;
  uint64_t n_objects;
  uint32_t n_pairs;
  uint64_t q0;
  uint64_t c0;               // (c0, p0) = scene_query(q0)
  uint32_t p0;
  uint32_t m;
  uint64_t total;            // n_conf * n_pairs: the chunk that holds the last query writes conf_begin[n_conf] and *n_listed
  uint64_t n_conf;
  double inflate;
  uint64_t* words;           // ceil(m / 64) ballots
  uint32_t* block_counts;    // ceil(m / CULL_BLOCK)
  uint64_t* block_offsets;   // ... survivors before the workgroup, over all chunks
  uint64_t* running;         // survivors of the chunks before this one (first: taken as 0), then of this one too
  int first;
  uint64_t* ids;             // nullptr / capacity 0: count only
  uint64_t capacity;
  uint64_t* conf_begin;      // nullptr or n_conf + 1
  uint64_t* n_listed;        // nullptr or one word
};
void launch_cull_chunk(hipStream_t st, const CullArgs& a);
// the expansion of a chunk of the list: a.m queries, query of row r = ids[r]; a.q0 / c0 / p0 unused
void launch_scene_expand_listed(hipStream_t st, const SceneExpandArgs& a, const uint64_t* ids, bool f32, int max_blocks);
void launch_scene_summary_init(hipStream_t st, hfcl_scene_summary* summary, uint64_t n_conf, int max_blocks);
struct SceneFoldListedArgs {
  const void* rec;               // the chunk's records: rec[0] is list entry k0's
  const uint64_t* ids;           // the whole list
  const uint64_t* conf_begin;
  uint64_t k0, k1;
  uint32_t n_pairs;
  double margin;
  int collide;
  hfcl_scene_summary* summary;   // by configuration, initialised (launch_scene_summary_init) before the first chunk
  hfcl_scene_summary* partials;  // nullptr (pair lists of one piece) or n_conf * scene_shares(n_pairs) slots
  uint64_t n_conf;               // configurations of the call: the bound on those a chunk spans (it may span empty ones: not bounded by k1 - k0)
  uint32_t shares;               // launch_scene_fold_ranked: pieces per configuration (launch_scene_fold_listed: scene_shares(n_pairs), not read)
};
void launch_scene_fold_listed(hipStream_t st, const SceneFoldListedArgs& a, bool f32, int max_blocks);
// (hfcl_k_cull.hip) the expansion of a chunk of a list of explicit pairs: a.m entries from entry k0 on; pairs: the whole list, 2 x uint32 an
// entry; the configuration of an entry: the span of conf_begin that holds it; a.pairs / n_pairs / q0 / c0 / p0 unused
void launch_scene_expand_pairs(hipStream_t st, const SceneExpandArgs& a, const uint32_t* pairs, const uint64_t* conf_begin, uint64_t n_conf,
                               uint64_t k0, bool f32, int max_blocks);
// (hfcl_k_cull.hip) the fold of a chunk of a list of explicit pairs (hfcl_scene_*_pairs_device*): a.ids unused, a.n_pairs unused; an entry's
// pair index is its rank k - conf_begin[c], the configurations of the chunk are found in conf_begin, a configuration has at most `shares` pieces
void launch_scene_fold_ranked(hipStream_t st, const SceneFoldListedArgs& a, uint32_t shares, bool f32, int max_blocks);
// (hfcl_k_cull.hip) the scan and the emit of launch_cull_chunk alone, behind a mark kernel of another unit that left a.words / a.block_counts
void launch_cull_scan_emit(hipStream_t st, const CullArgs& a);

// hfcl_k_nearest.hip: the per-configuration minimum distance with box-bound pruning (hfcl_scene_nearest*; hfcl_nearest.hpp has the arithmetic).
// c.boxes: the world boxes of the WHOLE table (c.c_box0 = 0); c.inflate unused
struct NearestArgs {
  CullArgs c;
  double r;                  // the bound's rounding term: NEAREST_R64 / NEAREST_R32
  double upper;              // the caller's upper bound D
  uint32_t* seed;            // n_conf: written by launch_nearest_seed, read by the marks
  void* seed_partials;       // nullptr (pair lists of one piece) or n_conf * scene_shares(n_pairs) NearestSeed
  double* thr;               // n_conf: written by launch_nearest_threshold, read by the mark of pass 2
};
// seed[c] of every configuration: a wave per (configuration, piece of SCENE_FOLD_SHARE pairs), then a wave per configuration
void launch_nearest_seed(hipStream_t st, const NearestArgs& a, int max_blocks);
// a chunk [q0, q0 + m) of the flat range: the mark of pass 1 / pass 2, then launch_cull_scan_emit
void launch_nearest_chunk(hipStream_t st, const NearestArgs& a, int pass);
// thr[c] = min(D, summary[c].min_distance)
void launch_nearest_threshold(hipStream_t st, const NearestArgs& a, const hfcl_scene_summary* summary);
// min record of every configuration: the record of c * n_pairs + min_pair out of the two lists' records (rec[k] is for ids[k]); a
// configuration without a min_pair gets distance = +inf, status bit 31
struct NearestGatherArgs {
  const hfcl_scene_summary* summary;
  uint64_t n_conf;
  uint32_t n_pairs;
  const uint64_t* ids[2];
  const uint64_t* conf_begin[2];
  const void* rec[2];
  void* out;
};
void launch_nearest_gather(hipStream_t st, const NearestGatherArgs& a, bool f32);

// hfcl_k_pairs.hip: the self-collision pairs of a scene per configuration (hfcl_scene_self_pairs*; hfcl_pairs.hpp has the arithmetic).
// A chunk of consecutive row blocks [g0, g0 + n_blocks): count (a uint32 per row), scan (row offsets on top of the
// entries of the chunks before: *running; conf_begin of the configurations that start in the chunk; the total with the last row), emit (the
// pairs at their positions, below the capacity).  Launches in stream order; no atomics, no kernel waits for another workgroup.
struct PairsArgs {
  const double* boxes;       // world boxes of the configurations [c_box0, ...) the chunk touches, n_objects each
  uint64_t c_box0;
  uint32_t n_objects;
  uint32_t rows_per_block;   // hfcl_pairs.hpp: PairsGeometry
  uint32_t blocks_per_conf;
  int small;                 // the wave-per-configuration form (n_objects <= PAIRS_SMALL_MAX)
  uint64_t g0;               // first row block of the chunk
  uint32_t n_blocks;         // row blocks of the chunk
  uint64_t row0;             // first row of the chunk in the table
  uint32_t n_rows;           // rows of the chunk
  uint64_t total_rows;       // n_conf * n_objects
  uint64_t n_conf;
  double inflate;
  uint32_t* row_counts;      // n_rows
  uint64_t* row_offsets;     // n_rows
  uint32_t* sums;            // ceil(n_rows / PAIRS_SCAN_BLOCK): entries of a scan workgroup's rows
  uint64_t* sum_offsets;     // ... entries before them, over all chunks
  uint64_t* running;         // entries of the chunks before this one (first: taken as 0), then of this one too
  int first;
  uint32_t* pairs;           // nullptr / capacity 0: count only
  uint64_t capacity;
  uint64_t* conf_begin;      // nullptr or n_conf + 1
  uint64_t* n_listed;        // nullptr or one word
  // object groups (hppfcl_amd_groups.h; hfcl_pairs.hpp has the rule): all three nullptr without groups, which picks the kernels
  const uint8_t* group;          // n_objects: an object's group
  const uint64_t* collides;      // PAIRS_MAX_GROUPS words: the row mask of a group
  const uint64_t* tile_groups;   // a word per column tile of PAIRS_TILE objects: the groups present
};
void launch_pairs_chunk(hipStream_t st, const PairsArgs& a);
// (hfcl_k_pairs.hip) the three scan launches of launch_pairs_chunk alone, behind a count kernel of another unit that left a.row_counts
void launch_pairs_scan(hipStream_t st, const PairsArgs& a);

// hfcl_k_pairs_sorted.hip: the same list by sort and sweep along one axis (option scene_pairs_sorted; hfcl_pairs_sorted.hpp has the
// arithmetic).  A chunk of n_conf_chunk WHOLE configurations.  p: the chunk's boxes (c_box0 = the chunk's first configuration), n_objects,
// row0 / n_rows / total_rows / n_conf, inflate, the row arrays and the scan's (a row is a SORTED position of the chunk), running / first,
// the list, the groups (tile_groups unused).  Two halves around the one read-back of a chunk: ..._count leaves the rows' counts, their
// offsets, conf_begin and the count (p.running[0]: the entries up to and with this chunk); the host sizes emit[] and temp by the chunk's
// entries; ..._emit writes the entries [emit_base, emit_base + n_emit) of the list below p.capacity.
struct PairsSortedArgs {
  PairsArgs p;
  uint32_t axis;             // 0, 1, 2, or PSORT_AXIS_AUTO: per configuration, conf_axis
  uint32_t n_conf_chunk, blocks_per_conf, conf_bits, obj_bits;
  uint32_t* conf_axis;       // n_conf_chunk (automatic axis)
  double* spread;            // n_conf_chunk x spread_blocks x 6: centre min / max per workgroup of the spread kernel (automatic axis)
  uint32_t spread_blocks;    // ceil(n_objects / PSORT_SPREAD_BLOCK)
  uint64_t* keys[2];         // n_rows each: the words as made, sorted
  uint32_t* vals[2];         // n_rows each: the object of a word
  double* sorted_boxes;      // n_rows x 6: the grown boxes in sorted order
  uint8_t* sorted_group;     // n_rows (with groups)
  uint32_t* ends;            // n_rows: a position's window end, a position of its configuration
  uint64_t* emit[2];         // n_emit each: the entries' words as emitted, sorted
  uint64_t n_emit, emit_base;
  void* temp;                // the sorts' temporary storage
  size_t temp_bytes;
};
// temporary storage of the sort of a chunk's p.n_rows keys (emit false) / of its n_emit entries (emit true), over the bits in use
hipError_t pairs_sorted_temp_bytes(const PairsSortedArgs& a, bool emit, size_t& bytes);
hipError_t launch_pairs_sorted_count(hipStream_t st, const PairsSortedArgs& a);
hipError_t launch_pairs_sorted_emit(hipStream_t st, const PairsSortedArgs& a);

// hfcl_k_env.hip: a static environment kept on the device (hfcl_scene_set_environment*, hfcl_scene_env_pairs*; hfcl_env.hpp has the
// arithmetic).  The boxes of one tile of PAIRS_TILE environment boxes each (set time)
void launch_env_tile_boxes(hipStream_t st, const double* env_boxes, uint32_t n_env, double* tile_boxes);
// A chunk of consecutive row blocks of the moving rows, times the spans of column tiles: count (a uint32 per (row, span)), launch_pairs_scan
// with rows x spans as its rows, emit.  p: the chunk's blocks (g0, n_blocks, c_box0, boxes: of the MOVING rows, n_moving a configuration),
// inflate, the list, the groups (tile_groups unused), and -- for the scan -- n_objects = n_moving * n_spans, row0, n_rows, total_rows in
// (row, span) counts.
struct EnvArgs {
  PairsArgs p;
  uint32_t n_moving, n_env;
  uint32_t tiles_moving, tiles;      // hfcl_env.hpp: EnvGeometry
  uint32_t span_len, n_spans;
  uint32_t blocks_per_conf;
  uint64_t row0;                     // first moving row of the chunk, c * n_moving + i
  const double* env_boxes;           // n_env world boxes
  const double* env_tile_boxes;      // ceil(n_env / PAIRS_TILE)
  const uint64_t* col_tile_groups;   // a word per column tile (moving tiles, then environment tiles): the groups present; nullptr without groups
};
void launch_env_chunk(hipStream_t st, const EnvArgs& a);
// the expansion of a chunk of an env list: launch_scene_expand_pairs with two tables -- a.object_tf: n_conf x n_moving rows, a.n_objects =
// n_moving; rows of j >= n_moving from env_tf[j - n_moving]
void launch_scene_expand_env(hipStream_t st, const SceneExpandArgs& a, const uint32_t* pairs, const uint64_t* conf_begin, uint64_t n_conf,
                             uint64_t k0, const void* env_tf, bool f32, int max_blocks);

// hfcl_k_nearest_self.hip: the clearance per configuration on device-made pairs (hfcl_scene_nearest_self*; hfcl_nearest_self.hpp has the
// arithmetic).  The row blocks, chunks and row arrays are those of PairsArgs (p.inflate unused: nothing is inflated).
struct NselfArgs {
  PairsArgs p;
  double r;                  // the bound's rounding term: NEAREST_R64 / NEAREST_R32
  double upper;              // the caller's upper bound D
  int pass;                  // launch_nself_chunk: 1 / 2
  void* row_seeds;           // tiled form: a NselfRowSeed per row of the WHOLE table (a configuration may straddle chunks)
  uint64_t* seed;            // n_conf pairs as words (nself_key; NSELF_NO_PAIR: no candidate)
  const double* thr;         // n_conf: read by pass 2
};
// a chunk's part of the seeds: the tiled form writes its rows' row_seeds, the small form seed[c] of its configurations
void launch_nself_seed(hipStream_t st, const NselfArgs& a);
// tiled form, after the last chunk: seed[c] from the rows' partials, a wave per configuration
void launch_nself_seed_combine(hipStream_t st, const NselfArgs& a, int max_blocks);
// a chunk of pass a.pass: count, launch_pairs_scan, emit (p.pairs == nullptr / capacity 0: count only)
void launch_nself_chunk(hipStream_t st, const NselfArgs& a);
// the two passes' summaries, lists and records into the clearance and the min record of every configuration (null conf_begin: no list)
struct NselfCombineArgs {
  uint64_t n_conf;
  const hfcl_scene_summary* summary[2];
  const uint32_t* pairs[2];
  const uint64_t* conf_begin[2];
  const void* rec[2];        // nullptr: no min records
  hfcl_scene_clearance* out;
  void* min_out;             // nullptr or n_conf records
};
void launch_nself_combine(hipStream_t st, const NselfCombineArgs& a, bool f32);

// hfcl_k_nearest_env.hip: the clearance of the moving objects among an environment kept on the device (hfcl_scene_nearest_env*;
// hfcl_nearest_env.hpp has the arithmetic).  Set time: two doubles per environment box (nenv_box_terms) and per tile (nenv_tile_terms)
void launch_nenv_terms(hipStream_t st, const double* env_boxes, uint32_t n_env, double* env_terms, double* tile_terms);
// The cells, chunks and (row, span) arrays are those of EnvArgs (e.p.inflate unused: nothing is inflated).
struct NenvArgs {
  EnvArgs e;
  double r;                      // the bound's rounding term: NEAREST_R64 / NEAREST_R32
  double upper;                  // the caller's upper bound D
  int pass;                      // launch_nenv_chunk: 1 / 2
  int prune;                     // 0: no environment tile is dropped by its distance (option scene_nearest_env_prune)
  void* row_seeds;               // a NselfRowSeed per (row, span) of the WHOLE table, row-major (a configuration may straddle chunks)
  uint64_t* seed;                // n_conf pairs as words (nself_key; NSELF_NO_PAIR: no candidate)
  const double* thr;             // n_conf: read by pass 2
  const double* env_terms;       // 2 x n_env
  const double* env_tile_terms;  // 2 x ceil(n_env / PAIRS_TILE)
};
// a chunk's part of the seeds: its cells' partials
void launch_nenv_seed(hipStream_t st, const NenvArgs& a);
// after the last chunk: seed[c] from the partials, a wave per configuration
void launch_nenv_seed_combine(hipStream_t st, const NenvArgs& a, int max_blocks);
// a chunk of pass a.pass: count, launch_pairs_scan, emit (e.p.pairs == nullptr / capacity 0: count only)
void launch_nenv_chunk(hipStream_t st, const NenvArgs& a);
