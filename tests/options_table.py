"""Every tuning option of the library (engine.option_keys(), hfcl_lib_set_option) and how its forms are held against each other.

One entry per key in TABLE; an entry is a list of rows (an option that acts on two families has two).  A row is either

  Row(key, family, values, witness, ...)   run by tests/test_options_gpu.py: the family's small batch with the option at each value against
                                           the same batch with the row's `base` options alone, byte for byte; or
  Covered(key, by)                         the node id of an existing test that already compares the option's forms by bytes at small size
                                           (tests/test_options_table_cpu.py checks that the function exists and that its source -- or the
                                           source of a helper of the same module that it calls -- names the key).

Fields of a Row
  family     the batch and the calls (FAMILIES below; built once per module by test_options_gpu.py, the default records held to the oracle)
  calls      which of the family's calls the row runs (default: all)
  base       options both runs have (the row's form only exists under them: a continuation needs a small budget to have work, ...)
  values     every value that selects a distinct form, the default excepted (the default is the run compared against)
  threshold  a size option: Threshold(t, kind, off).  The option is set to t and the batch cut to n = t - 1, t, t + 1; kind "max": the form
             applies to n <= t, "min": to n >= t.  `off` is a value that switches the form off at all three sizes.  The three sizes must show
             the switch where the documentation puts it, and at every size the records equal the runs at `off` and at the default
  witness    observables (test_options_gpu.observe) that must DIFFER between the run at a value and the default run: the other form ran.
             "forms.x" is entry x of the dispatcher's plan of the last batch (hfcl_debug_last_forms: what the kernels were launched with),
             "walk_mm" / "walk_ms" the device counters of the walk rounds and split tables (hfcl_debug_walk_counters), "reruns"
             last_ordered_reruns(), "kernels" the names of last_kernel_breakdown() in order, "stderr" what the call wrote to stderr.
             EVERY component named must differ (in at least one of the row's calls); components in an inner tuple make one observable.
             None only for options that move work between streams and nothing else; `why` then says so
  expect     {value: ((path, op), ...)}: counts the DEVICE wrote, read after the row's first call, in the direction the value must move
             them.  op: ">0", "==0", ">default", "<default", "!=default" (against the run at `base`), or "==path" (another count of the same
             run).  reruns.*_continued: distance() walks handed to a continuation; reruns.*_rerun: walks walked again in order;
             mm_suspended / ms_suspended: collide() queries that suspended (the same in every run); mm_tasks / ms_tasks: tasks made (vary
             a little from run to run with the order the waves take them in: compared where the forms are far apart);
             buckets.epa_overflow: polytopes that outgrew the fast EPA tier.  A small budget must raise the count, a large one bring it to
             zero where the budget is the only reason to suspend
  work       counts of the value's run that must be above zero: the path the option tunes had work on this batch
  decisions_at  every value is held by BYTES: records (and guesses, and the contact list in a canonical order, where the call produces them)
             byte for byte -- the claim of include/hppfcl_amd.h.  The values named here are the one exception, in the call mm_collide alone
             (fp64 mesh x mesh collide(), built with the compiler's default contraction: csrc/Makefile, FLAGS_k_bvh): the value selects a kernel
             that holds another inlined copy of the triangle-pair leaf, fused differently, so status, num_contacts, b1, b2 and the NaN pattern
             are byte-equal and distance / p1, p2, normal agree to 2e-6 / 2e-5 (each form is held to the oracle at 1e-6 / 1e-5 by
             test_gpu_parity._check_bvh_records, so two forms are within twice that).  Measured: at most 8.95e-16 in the distance field
  needs_ab   the form exists only in builds with HFCL_KEEP_AB_FORMS (engine.has_ab_forms()); the product build must refuse `refused`
"""
from collections import namedtuple

Threshold = namedtuple("Threshold", "t kind off")


class Row:
    def __init__(self, key, family, values=(), witness=None, why=None, base=None, calls=None, threshold=None, decisions_at=(), needs_ab=False,
                 refused=None, expect=None, work=()):
        self.key, self.family, self.values, self.witness, self.why = key, family, tuple(values), witness, why
        self.base, self.calls, self.threshold, self.needs_ab, self.refused = dict(base or {}), calls, threshold, needs_ab, refused
        self.decisions_at = tuple(decisions_at)
        self.expect, self.work = dict(expect or {}), ((work,) if isinstance(work, str) else tuple(work))
        self.equal = "decisions" if self.decisions_at else "bytes"
        if isinstance(self.witness, str):
            self.witness = (self.witness,)


class Covered:
    def __init__(self, key, by):
        self.key, self.by = key, by


# family -> the calls it has (test_options_gpu.py builds the batches)
FAMILIES = {
    "solids64": ("prim_collide", "prim_distance", "mix_collide", "mix_distance"),
    "solids32": ("prim_collide_f32", "prim_distance_f32", "mix_collide_f32", "mix_distance_f32"),
    "hulls32": ("hulls_distance_f32",),
    "large": ("large_distance", "large_collide"),
    "mm": ("mm_collide", "mm_distance", "ties_mm_distance"),
    "ms": ("ms_collide", "ms_contacts", "ms_distance", "ties_ms_distance"),
    "mixed": ("mixed_collide", "mixed_distance", "mixed_after_meshes"),
    "host": ("host_collide", "host_distance"),
}

STREAMS = "moves kernels between streams; the launches, their arguments and their order on the batch's stream are the same"
MM = {"bvh_budget0_coop": 24}  # mesh x mesh collide(): 200-triangle meshes end most walks inside the default 256 box tests
MMD = {"bvhd_budget": 16}      # ... distance(): the same for the default 64 steps
LEVELS = {"bvh_coop": 0}       # the task-level form of mesh x mesh collide()
WALK = {"shape_walk_min": 0}   # mesh x solid collide(): the walk / leaves / resolve phase starts at 65 536 queries by default
DIRECT_OFF = {"epa_direct_max": 0}  # the EPA tiers of a batch of up to 4096 pairs: all seeds go to the full tier by default
CC = {"epa_cc_staged_min": 0}       # the staged fp32 hull x hull EPA starts at 32 768 pairs by default

ROWS = [
    # ---- solids, fp64
    Row("closed_staged", "solids64", (0,), "forms.closed_staged"),
    Row("epa64_two_streams", "solids64", (0,), "forms.epa64_two_streams", base=DIRECT_OFF, why=STREAMS),
    Row("epa_direct_max", "solids64", threshold=Threshold(1024, "max", 0), witness=("forms.epa_direct", "kernels")),
    Row("gjk_beside_max", "solids64", threshold=Threshold(1024, "max", 0), witness="forms.gjk_fan", why=STREAMS),
    Row("gjk_beside_max", "solids32", threshold=Threshold(1024, "max", 0), witness="forms.gjk_fan", why=STREAMS),
    Row("epa_general_staged", "solids64", (1,), "kernels", base=dict(DIRECT_OFF, epa_general_staged_min=0), needs_ab=True,
        refused=("epa_general_staged", 1)),
    Row("epa_general_staged_min", "solids64", threshold=Threshold(1024, "min", 100000), witness="forms.epa_gen_staged",
        base=dict(DIRECT_OFF, epa_general_staged=1), needs_ab=True, refused=("epa_general_staged", 1)),
    # the save area of the tier hand-over: the default (an eighth of the batch, 65 536 at the least), a generous one, a tight one that still
    # holds this batch's hand-overs, and one slot -- beyond the area the full tier redoes the pair from its seed, the same bytes
    # (hfcl_host_batch.hip: ensure_workspace; tests/test_gpu_parity.py::test_epa_hand_over_equals_restart runs 64 slots at 60 000 pairs)
    # (a generous value is no other form at this size: the default already is the whole workspace, 3329 slots)
    # (forms.epa_resume_cap is the capacity the kernels were given.  prim_collide hands 46 polytopes over, mix_collide 62: 256 slots hold
    # them all, one slot sends all but one back to their seeds)
    Row("epa_resume_slots", "solids64", (256, 1), "forms.epa_resume_cap", base=DIRECT_OFF,
        expect={256: (("buckets.epa_overflow", ">0"), ("buckets.epa_overflow", "<=256")), 1: (("buckets.epa_overflow", ">1"),)}),
    Row("cvx_w", "solids64", (2, 4, 8, 16, 32, 64), (("forms.cvx_w_cc", "forms.cvx_w_pc", "forms.cvx_w_cp"),), work=("buckets.cc", "buckets.pc", "buckets.cp"), calls=("mix_collide", "mix_distance", "prim_collide", "prim_distance")),
    # ---- hulls, fp32 (the automatic width of every fp32 kernel is 2)
    Row("cvx_w", "hulls32", (4, 8, 16, 32, 64), "forms.cvx_w_cc", work="buckets.cc"),
    Row("epa_cc_staged", "hulls32", (0,), "kernels", base=CC),
    Row("epa_cc_staged_min", "hulls32", threshold=Threshold(2048, "min", 100000), witness=("forms.epa_cc_staged", "kernels")),
    Row("epa_records_aside", "hulls32", (0,), "forms.epa_records_aside", base=CC, why=STREAMS),
    Row("epa_pool_share", "hulls32", (0, 50), "forms.epa_pool_share", base=dict(CC, epa_pool_min_refills=0)),
    Row("epa_pool_min_refills", "hulls32", (0, 1000), "forms.epa_pool_min_refills", base=CC),
    # ---- large hulls: 33, 48, 64, 100 and 256 vertices; the default (512) scans them all
    Row("climb_min", "large", (33, 49, 65, 101, 257), "forms.climb_min", work="buckets.large"),
    # ---- mesh x mesh
    # (decisions_at: the default is k_bvh_walk / k_tri_leaves / k_bvh_resolve with k_bvh_coop behind them; the task levels, k_bvh_collide with
    # its leaves inline and the wide form's whole walks each hold their own copy of the leaf)
    Row("bvh_coop", "mm", (0,), "forms.mm_coop", base=MM, calls=("mm_collide",), decisions_at=(0,), expect={0: (("mm_suspended", "!=default"), ("mm_tasks", ">0"))}),
    # (100000: the queries that still suspend do so on a full list of leaves, not on the budget)
    Row("bvh_budget0_coop", "mm", (24, 100000), "forms.mm_budget0", calls=("mm_collide",),
        expect={24: (("mm_suspended", ">default"),), 100000: (("mm_suspended", "<default"),)}),
    Row("bvh_walk_rounds", "mm", (0, 1, 2, 3, 4), (("forms.mm_rounds", "forms.mm_walk_k"),), base=MM, calls=("mm_collide",), decisions_at=(0,), work="mm_suspended"),
    Row("bvh_walk_k", "mm", ("2,3,4,16", "1,1,1,1", "16,16,16,16"), ("forms.mm_walk_k", "mm_round_counters"), base={"bvh_walk_rounds": 4},
        calls=("mm_collide",)),
    Row("bvh_walk_budget", "mm", ("24,24,48", "100000,100000,100000"), ("forms.mm_walk_budget", "mm_round_counters"), base={"bvh_walk_rounds": 4, "bvh_walk_k": "1,1,2,16"},
        calls=("mm_collide",)),
    Row("bvh_walk_early_coop", "mm", (0,), "forms.mm_early_coop", base=dict(MM, bvh_walk_rounds=4), calls=("mm_collide",), why=STREAMS),
    Row("bvh_walk_order", "mm", (0,), "forms.mm_order", base=MM, calls=("mm_collide",), work="mm_suspended"),
    Row("bvh_cut_ticks", "mm", (15000,), "forms.mm_cut_ticks", base=MM, calls=("mm_collide",), expect={15000: (("mm_tasks", ">default"),)}),
    Row("bvh_budget", "mm", (24, 100000), "forms.mm_budget", base=LEVELS, calls=("mm_collide",),
        expect={24: (("mm_tasks", ">default"), ("mm_suspended", ">default")), 100000: (("mm_tasks", "==0"), ("mm_suspended", "==0"))}),
    Row("bvh_budget0", "mm", (24, 100000), "forms.mm_budget0", base=LEVELS, calls=("mm_collide",),
        expect={24: (("mm_suspended", ">default"),), 100000: (("mm_suspended", "==0"),)}),
    Row("bvh_levels", "mm", (1, 2), (("forms.mm_levels", "forms.mm_split"),), base=LEVELS, calls=("mm_collide",), expect={1: (("mm_tasks", "==0"),), 2: (("mm_tasks", "!=default"),)}),
    # the task table: slots x (n + n / 8 + 1024) + 65 536 entries (hfcl_host_batch.hip: ensure_split), so at this size no value is too small;
    # 0 is 16 slots, 64 generous, 1 tight
    Row("bvh_task_slots", "mm", (64, 1), "forms.mm_cap", base=LEVELS, calls=("mm_collide",), work="mm_tasks"),
    Row("bvh_force_wide", "mm", (1,), "forms.bvh_wide", decisions_at=(1,)),
    Row("bvh_filter", "mm", (1,), "forms.bvh_filter", calls=("mm_collide",), needs_ab=True, refused=("bvh_filter", 1)),
    Row("bvhd_budget", "mm", (16, 0, 100000), "forms.mmd_budget", calls=("mm_distance", "ties_mm_distance"),
        expect={16: (("reruns.mesh_continued", ">default"),), 0: (("reruns.mesh_continued", "==0"),), 100000: (("reruns.mesh_continued", "==0"),)}),
    # (the ordered continuation has nothing to walk again: the pooled default walks 10 of these 1025 again)
    Row("bvhd_pool", "mm", (0,), "forms.mmd_pool", base=MMD, calls=("mm_distance", "ties_mm_distance"), work="reruns.mesh_continued",
        expect={0: (("reruns.mesh_rerun", "==0"), ("reruns.mesh_rerun", "<default"))}),
    Row("bvhd_leaf_min", "mm", (1, 1000), "forms.mmd_leaf_min", base=MMD, calls=("mm_distance", "ties_mm_distance"), work="reruns.mesh_continued"),
    Row("bvhd_starve", "mm", (1, 1000), "forms.mmd_starve", base=MMD, calls=("mm_distance", "ties_mm_distance"), work="reruns.mesh_continued"),
    Row("bvhd_part_min", "mm", (0, 64), "forms.mmd_part_min", base=MMD, calls=("mm_distance", "ties_mm_distance"), work="reruns.mesh_continued"),
    Row("pool_rerun", "mm", (0, 2), "forms.mmd_rerun", base=MMD, calls=("mm_distance", "ties_mm_distance"), work="reruns.mesh_continued",
        expect={0: (("reruns.mesh_rerun", "==0"), ("reruns.mesh_rerun", "<default")), 2: (("reruns.mesh_rerun", "==reruns.mesh_continued"),)}),
    # ---- mesh x solid
    Row("pool_rerun", "ms", (0, 2), "forms.msd_rerun", base={"shape_dist_budget": 16}, calls=("ms_distance", "ties_ms_distance"), work="reruns.solid_continued",
        expect={0: (("reruns.solid_rerun", "==0"), ("reruns.solid_rerun", "<default")), 2: (("reruns.solid_rerun", "==reruns.solid_continued"),)}),
    Row("bvh_shape_lane", "ms", (0,), ("forms.ms_lane", "forms.msd_lane"), calls=("ms_distance", "ms_collide", "ms_contacts", "ties_ms_distance"),
        expect={0: (("reruns.solid_continued", "==0"), ("reruns.solid_continued", "<default"))}),
    Row("shape_coop", "ms", (0,), "forms.ms_coop", calls=("ms_collide", "ms_contacts"), expect={0: (("ms_suspended", "!=default"), ("ms_tasks", ">0"))}),
    Row("shape_budget0", "ms", (2, 100000), "forms.ms_budget0", calls=("ms_collide", "ms_contacts"),
        expect={2: (("ms_suspended", ">default"),), 100000: (("ms_suspended", "==0"),)}),
    Row("shape_budget", "ms", (2, 100000), "forms.ms_budget", base={"shape_coop": 0, "shape_budget0": 8}, calls=("ms_collide",),
        expect={2: (("ms_tasks", ">default"),), 100000: (("ms_tasks", "<default"),)}),
    # (a cost above the default's 32 suspends the same 370 queries at this size: no value above it is another form here)
    Row("shape_leaf_cost", "ms", (1, 8), "forms.ms_leaf_cost", calls=("ms_collide",), expect={1: (("ms_suspended", "<default"),), 8: (("ms_suspended", "<default"),)}),
    # (two levels hold every walk of this batch: the same tasks as twelve; one level is the walk in one piece)
    Row("shape_levels", "ms", (1,), (("forms.ms_levels", "forms.ms_split"),), calls=("ms_collide", "ms_contacts"), expect={1: (("ms_tasks", "==0"), ("ms_suspended", "==0"))}),
    # (0, never, is what the default's 350 000 ticks amount to on walks this short)
    Row("shape_cut_ticks", "ms", (15000,), "forms.ms_cut_ticks", base={"shape_budget0": 8}, calls=("ms_collide", "ms_contacts"), expect={15000: (("ms_tasks", ">default"),)}),
    Row("shape_finish_tiers", "ms", (0,), "forms.ms_finish_tiers", calls=("ms_collide", "ms_contacts")),
    Row("shape_finish_aside", "ms", (0,), "forms.ms_finish_aside", calls=("ms_collide",), why=STREAMS),
    Row("shape_walk", "ms", (0,), "forms.ms_rounds", base=WALK, calls=("ms_collide",)),
    Row("shape_walk_sort", "ms", (0,), "forms.ms_perm", base=WALK, calls=("ms_collide",)),
    # (the default's 256 box tests already end all but 17 walks, which suspend on a full list: no larger value is another form here)
    Row("shape_walk_budget", "ms", (16,), "forms.ms_walk_budget", base=WALK, calls=("ms_collide",), expect={16: (("ms_suspended", ">default"),)}),
    Row("shape_walk_min", "ms", threshold=Threshold(512, "min", 100000), witness="forms.ms_rounds", calls=("ms_collide",)),
    Row("shape_dist_budget", "ms", (16, 0, 100000), "forms.msd_budget", calls=("ms_distance", "ties_ms_distance"),
        expect={16: (("reruns.solid_continued", ">default"),), 0: (("reruns.solid_continued", "==0"),), 100000: (("reruns.solid_continued", "==0"),)}),
    Row("shape_dist_pool", "ms", (0,), "forms.msd_pool", base={"shape_dist_budget": 16}, calls=("ms_distance", "ties_ms_distance"), work="reruns.solid_continued",
        expect={0: (("reruns.solid_rerun", "==0"), ("reruns.solid_rerun", "<default"))}),
    Row("shape_dist_leaf_min", "ms", (1, 1000), "forms.msd_leaf_min", base={"shape_dist_budget": 16}, calls=("ms_distance", "ties_ms_distance"), work="reruns.solid_continued"),
    Row("shape_dist_starve", "ms", (1, 1000), "forms.msd_starve", base={"shape_dist_budget": 16}, calls=("ms_distance", "ties_ms_distance"), work="reruns.solid_continued"),
    Row("bvh_force_wide", "ms", (1,), "forms.bvh_wide"),
    # ---- meshes and solids in one library.  The default, 2, follows the batch before: the second of two equal mixed batches runs beside, as
    # with 4; a mixed batch behind a batch of mesh pairs alone runs in line, as with 0 (mixed_after_meshes: through the device entry points --
    # a host call does not leave the counts of its batch behind, so every host batch is a first batch)
    Row("mesh_beside", "mixed", (0, 1, 4), (("forms.mesh_beside", "forms.mm_beside"), "kernels"), calls=("mixed_collide", "mixed_after_meshes")),
    Row("mesh_prio", "mixed", (1,), None, why="read when the mesh streams are created: their priority, nothing else", calls=("mixed_collide",)),
    # ---- the host pipeline (n = 2049): every chunking of the batch, records and guesses
    Row("pipe_chunk", "host", (1, 63, 64, 65, 2048, 2049, 2050), (("forms.host_chunks", "forms.host_packed"),)),
    Row("pipe_trace", "host", (1,), "stderr", base={"pipe_chunk": 64}),
    # ---- held by bytes at small size by the tests of their own units
    Covered("split", "test_gpu_dispatch.py::test_split_batch"),  # (131 072 pairs: the smallest batch that splits, MIN_SPLIT)
    Covered("scene_chunk", "test_scene_gpu.py::test_planner_scene_chunks_straddle_configurations"),
    Covered("scene_cull_chunk", "test_scene_cull_gpu.py::test_cull_equals_the_model"),
    Covered("scene_pairs_small_max", "test_scene_pairs_gpu.py::test_both_forms_write_the_same_bytes"),
    Covered("scene_pairs_sorted", "test_scene_pairs_sorted_gpu.py::test_sorted_and_all_pairs_forms_agree"),
    Covered("scene_pairs_sorted_axis", "test_scene_pairs_sorted_gpu.py::test_list_does_not_depend_on_axis_or_chunks"),
    Covered("scene_env_span", "test_scene_env_gpu.py::test_list_does_not_depend_on_chunks_and_spans"),
    Covered("scene_nearest_env_prune", "test_scene_nearest_env_gpu.py::test_spans_chunks_and_pruning_give_the_same_bytes"),
    Covered("hfield_chunk", "test_hfield_gpu.py::test_device_equals_harness_and_host_equals_device"),
    Covered("hfield_items", "test_hfield_gpu.py::test_device_equals_harness_and_host_equals_device"),
    Covered("octree_chunk", "test_octree_gpu.py::test_device_equals_harness_and_host_equals_device"),
    Covered("octree_items", "test_octree_gpu.py::test_device_equals_harness_and_host_equals_device"),
]

TABLE = {}
for _r in ROWS:
    TABLE.setdefault(_r.key, []).append(_r)

# hfcl_lib_set_option refuses these (include/hppfcl_amd.h: HFCL_ERR_INVALID_ARGUMENT, nothing changed): what is no unsigned decimal number,
# and per key a value above the option's range.  ABOVE[key] is the smallest such value; BELOW[key] the largest one below the range
GARBAGE = ("abc", "", "1x", " 3", "3 ", "-1", "+1", "0x10", "1.0", "1e3", "18446744073709551616")
_FLAGS = ("closed_staged", "epa_cc_staged", "epa_records_aside", "epa_general_staged", "shape_finish_tiers", "shape_finish_aside", "epa64_two_streams",
          "bvh_filter", "bvh_shape_lane", "shape_coop", "bvh_coop", "bvhd_pool", "shape_dist_pool", "bvh_walk_early_coop", "bvh_walk_order", "shape_walk",
          "mesh_prio", "shape_walk_sort", "bvh_force_wide", "pipe_trace", "scene_pairs_sorted", "scene_nearest_env_prune")
_U32 = ("bvh_cut_ticks", "shape_cut_ticks", "bvhd_budget", "shape_walk_budget", "shape_walk_min", "gjk_beside_max", "epa_direct_max",
        "epa_pool_min_refills", "shape_dist_leaf_min", "shape_dist_starve", "bvhd_leaf_min", "bvhd_starve", "bvhd_part_min", "shape_dist_budget",
        "bvh_budget0_coop", "shape_budget0", "shape_budget", "shape_leaf_cost", "climb_min", "bvh_budget", "bvh_budget0", "scene_env_span")
_SIZE = ("epa_general_staged_min", "epa_cc_staged_min", "pipe_chunk", "epa_resume_slots")
ABOVE = dict({k: 2 for k in _FLAGS}, **{k: 1 << 32 for k in _U32}, **{k: (1 << 40) + 1 for k in _SIZE})
ABOVE.update(split=3, pool_rerun=3, mesh_beside=5, epa_pool_share=51, bvh_walk_rounds=5, shape_levels=13, bvh_levels=13, cvx_w=65,
             bvh_task_slots=(1 << 16) + 1, scene_chunk=0xFFFFFFF1, scene_cull_chunk=(1 << 31) + 1, scene_pairs_small_max=65,
             scene_pairs_sorted_axis=4, hfield_chunk=0xFFFFFFF1, hfield_items=(1 << 26) + 1, octree_chunk=0xFFFFFFF1, octree_items=(1 << 26) + 1,
             bvh_walk_k="17", bvh_walk_budget="4294967296")
BELOW = {k: 0 for k in ("shape_dist_leaf_min", "shape_dist_starve", "bvhd_leaf_min", "bvhd_starve", "bvh_budget0_coop", "shape_leaf_cost", "shape_levels",
                        "bvh_levels", "bvh_walk_k")}
INSIDE_BUT_REFUSED = {"mesh_beside": (3,), "cvx_w": (1, 3, 5, 6, 12, 48)}  # holes in an enumeration
LISTS = {"bvh_walk_k": ("1,2,3,4,5", "1,,2", "1,x", ",1", "1,", "1,17", "0,1"),  # too many elements, an empty one, a bad one, one out of range
         "bvh_walk_budget": ("1,2,3,4", "1,,2", "1,x", ",1", "1,", "1,4294967296")}
