"""Mesh x mesh collide(): the plans the dispatcher chooses from the batch size alone (hfcl_host_batch.hip: plan_split; described in hfcl_host.hpp
at hfcl_options::walk_auto), each at the smallest batch that gets it and at the largest that gets the one before.  The batch -- 500 001 queries of
cfg4's 5 000-triangle models -- and its oracle records are made once; a case runs a prefix of it through the device-resident entry point, the only
one that hands plan_split the size itself (hfcl_collide_batch cuts a batch into chunks first), on a fresh library.

Per size: the plan that ran is the documented one (a table below, written from the code and its comment), its path had work, every record is
the oracle's (test_gpu_parity._check_bvh_records, no record excused: the oracle has none within 1e-9 of the boundary), two runs are byte-equal.
Across a switch: the same pair gives the same record under either plan (test_options_gpu._same_decisions).  Then the same pairs in reversed
order, the fp32 instantiation, the host pipeline with two plans in one call, the task-level form across its own switch, and mesh x solid at
255 / 256 queries.

Figures are printed before they are asserted (pytest -s)."""
import ctypes as C
import time

import numpy as np
import pytest

from compare import boundary_band
from test_gpu_parity import _check_bvh_records, _depths
from test_options_gpu import _mmc_batch, _ms_batch, _same_decisions, observe, witness

pytestmark = pytest.mark.gpu

N_ALL = 500_001
SWITCHES = ((255, 256), (120_000, 120_001), (220_000, 220_001), (500_000, 500_001))
SIZES = tuple(n for pair in SWITCHES for n in pair)
WITNESS = ("forms.mm_split", "forms.mm_coop", "forms.mm_rounds", "forms.mm_budget0", "forms.mm_walk_k", "forms.mm_walk_budget", "forms.mm_early_coop")


def _plan(split, coop, rounds, budget0, walk_k, walk_budget, early):
    """A plan as `witness(obs, WITNESS)` shows it: the values noted under each name, in order; None: nothing noted under it."""
    s = lambda v: None if v is None else [str(x) for x in (v if isinstance(v, tuple) else (v,))]
    return [s(split), s(coop), s(rounds), s(budget0), s(walk_k), s(walk_budget), s(early)]


# The plans, read from plan_split and mesh_mesh_collide (not from a run).  Walk tables: mm_split is noted (as 0) only where there are none.
# A round's box tests: round 0 takes the queries' budget (mm_budget0), rounds 1 .. 3 the option bvh_walk_budget's defaults 256, 512, 512; a
# walk lists up to 16 leaves in a round (WALK_K), in round 0 of a two-round plan 6.
NO_TABLES = _plan(0, None, None, None, None, None, 0)
ONE_ROUND_256 = _plan(None, 1, 1, 256, (16, 16, 16, 16), (256, 256, 512, 512), 0)
ONE_ROUND_320 = _plan(None, 1, 1, 320, (16, 16, 16, 16), (320, 256, 512, 512), 0)
TWO_ROUNDS_320 = _plan(None, 1, 2, 320, (6, 16, 16, 16), (320, 256, 512, 512), 1)
TWO_ROUNDS_640 = _plan(None, 1, 2, 640, (6, 16, 16, 16), (640, 256, 512, 512), 1)
LANE_STACK = 26  # min(BVH_STACK, BVH_STACK_FILT), hfcl_dev.hpp: what a lane's stack holds


def expected_plan(n, depth):
    """hfcl_host.hpp, hfcl_options::walk_auto: one round of 256 box tests, 320 above 120 000 queries, up to 220 000; two rounds above, 320 box
    tests in round 0, 640 above 500 000.  Below 256 queries (mesh_mesh_collide) no tables -- unless a walk of the deepest model against itself,
    2 depth + 4 entries, does not fit a lane's stack: then the plan of the sizes from 256 on."""
    if n < 256 and 2 * depth + 4 <= LANE_STACK:
        return NO_TABLES
    if n <= 120_000:
        return ONE_ROUND_256
    if n <= 220_000:
        return ONE_ROUND_320
    return TWO_ROUNDS_320 if n <= 500_000 else TWO_ROUNDS_640


# what switches across each pair, by the table above (for 255 / 256 see test_tables_start_at_256_queries)
SWITCHED = {(120_000, 120_001): ("forms.mm_budget0", "forms.mm_walk_budget"),
            (220_000, 220_001): ("forms.mm_rounds", "forms.mm_walk_k", "forms.mm_early_coop"),
            (500_000, 500_001): ("forms.mm_budget0", "forms.mm_walk_budget")}


def _upload(s1, s2, p1, p2):
    """Shape ids and poses (12 doubles, or the fp32 entry points' 7 floats) as arrays on the device."""
    import torch
    dev = torch.device("cuda:0")
    return [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (s1.astype(np.int32), s2.astype(np.int32), p1, p2)]


def _device_run(pkg, b, req, d, n, entry="collide_device", options=None):
    """A fresh library for batch b with `options`, the first n queries of the device arrays d through the device-resident entry point `entry`,
    twice; the records of the second call, what can be observed after it, and whether the two calls gave the same bytes."""
    import torch
    abi = pkg.abi
    f32 = entry.endswith("_f32")
    lib = pkg.workloads.make_library(pkg, b, options=options)
    pkg.engine.dll().hfcl_debug_note_forms(lib._h, C.c_int(1))
    try:
        outs = []
        for _ in range(2):
            out = torch.zeros(n * (11 if f32 else 24), dtype=torch.int32, device=d[0].device)
            getattr(lib, entry)(*d, n, req, out)
            torch.cuda.synchronize()
            outs.append(out.cpu().numpy().view(abi.RESULT_F32_DTYPE if f32 else abi.RESULT_DTYPE).copy())
        assert not np.any((outs[1]["status"] >> 31) & 1), (entry, n)
        return dict(rec=outs[1], obs=observe(pkg, lib), same=outs[0].tobytes() == outs[1].tobytes())
    finally:
        lib.close()


class Big:
    """The batch, its request, the oracle's records, the arrays on the device (made once, never modified), and the runs kept per size."""

    def __init__(self, pkg, oracle):
        import torch
        abi, wl = pkg.abi, pkg.workloads
        t0 = time.time()
        self.pkg, self.b = pkg, wl.cfg4_mesh_mesh(n=N_ALL, seed=33)
        b = self.b
        assert len(b.meshes) == 8 and all(len(m.triangles) == 5000 for m in b.meshes)
        self.req = wl.make_request(b, abi)
        self.depth = max(1 + int(_depths(m.nodes).max()) for m in b.meshes)  # (hfcl_lib::bvh_max_depth counts the root as level 1)
        t1 = time.time()
        self.ref = oracle.bvh_collide_batch(pkg.bvh_builder.MeshLibrary(b.meshes), b.s1, b.s2, b.tf1, b.tf2, self.req, n_threads=16)
        a = np.abs(self.ref["distance"])
        print("    cfg4_mesh_mesh(n=%d, seed=33): made in %.1f s, the oracle's records in %.1f s; models %d levels deep; %d records within 1e-9 of the "
              "boundary, %d within 1e-6, the nearest %.3g away" % (N_ALL, t1 - t0, time.time() - t1, self.depth, int((a < 1e-9).sum()), int((a < 1e-6).sum()), float(a.min())))
        assert not boundary_band(self.ref, 0.0, allowed=0, name="cfg4-500001").any()  # (no excuse: the checks below are strict)
        self.dev = torch.device("cuda:0")
        self.tf1, self.tf2 = b.tf1, b.tf2
        self.d = self.upload(b.s1, b.s2, self.tf1, self.tf2)
        self.kept = {}

    def upload(self, s1, s2, p1, p2):
        return _upload(s1, s2, p1, p2)

    def run(self, n, options=None, d=None, f32=False):
        return _device_run(self.pkg, self.b, self.req, d or self.d, n, "collide_device_f32" if f32 else "collide_device", options)

    def at(self, n):
        if n not in self.kept:
            self.kept[n] = self.run(n)
        return self.kept[n]


@pytest.fixture(scope="module")
def big(pkg, oracle):
    return Big(pkg, oracle)


def _check_records(pkg, rec, ref, what):
    """(c): every record against the oracle's; no overflow flag, no error bit; a batch that decides both ways."""
    assert not np.any((rec["status"] >> 30) & 1), what + ": overflow flags"
    assert not np.any((rec["status"] >> 31) & 1), what + ": error bits"
    _check_bvh_records(pkg.abi, rec, ref, what)
    frac = float((ref["num_contacts"] > 0).mean())
    print("    %s: %d records held to the oracle's, contact fraction %.3f" % (what, len(rec), frac))
    assert 0.2 < frac < 0.8, frac


@pytest.mark.parametrize("n", SIZES)
def test_plan_work_and_records(pkg, big, n):
    """(a) the plan, (b) its work, (c) its records, (d) two runs."""
    r = big.at(n)
    obs, what = r["obs"], "%d queries" % n
    got, want = witness(obs, WITNESS), expected_plan(n, big.depth)
    print("    %s: plan %s" % (what, dict(zip(WITNESS, got))))
    print("    %s: documented %s" % (what, dict(zip(WITNESS, want))))
    assert got == want, "%s: the plan that ran is not the documented one" % what
    rc = obs["mm_round_counters"]
    rounds = int(want[2][0]) if want[2] else 0
    print("    %s: suspended queries %d, tasks %d; per round (queries that walk on, leaves listed, suspended when the round ended): %s" % (
        what, obs["mm_suspended"], obs["mm_tasks"], [(rc[8 * k + 2], rc[8 * k + 1], rc[8 * k + 3]) for k in range(max(rounds, 1))]))
    if n >= 256:
        assert obs["mm_suspended"] > 0, what + ": no walk outlasted its rounds: the continuation had no work"
    if rounds == 2:
        assert rc[2] > 0 and rc[8 + 1] > 0, what + ": round 1 had no query"
        assert rc[3] > 0, what + ": round 0 handed no query over"
        assert obs["mm_suspended"] >= rc[3]
    _check_records(pkg, r["rec"], big.ref[:n], what)
    assert r["same"], what + ": two runs on one library differ"


@pytest.mark.parametrize("m,n", SWITCHES)
def test_the_plan_switches_and_the_records_do_not(pkg, big, m, n):
    """(a) across a switch at least one component of the plan differs, the documented one; (e) the records of the pairs both runs hold are the
    same decisions byte for byte, the numbers within _same_decisions' bound (another plan may evaluate a leaf through another inlined copy)."""
    a, b = big.at(m), big.at(n)
    wa, wb = witness(a["obs"], WITNESS), witness(b["obs"], WITNESS)
    differ = tuple(p for p, x, y in zip(WITNESS, wa, wb) if x != y)
    print("    %d / %d queries: the components of the plan that differ: %s" % (m, n, differ))
    if (m, n) in SWITCHED:
        assert differ == SWITCHED[(m, n)], (m, n, differ)
    else:
        # 255 / 256: tables from 256 queries on, or where a lane's stack does not hold the walk -- these models' (16 levels: 36 entries against
        # 26) have them at either size.  The switch itself is seen on models whose walks fit: test_tables_start_at_256_queries
        assert 2 * big.depth + 4 > LANE_STACK and differ == (), (m, n, differ)
    _same_decisions(dict(rec=b["rec"][:m]), a, "records [:%d] of the run at %d against the run at %d" % (m, n, m))


def test_tables_start_at_256_queries(pkg):
    """(a) at 255 / 256 where the size decides: the options suite's 200-triangle models, 10 levels deep -- 24 stack entries, a lane holds them.
    No tables at 255 queries, the one-round plan at 256; the records of the first 255 pairs the same."""
    b = _mmc_batch(pkg)
    depth = max(1 + int(_depths(m.nodes).max()) for m in b.meshes)
    assert 2 * depth + 4 <= LANE_STACK, depth
    d = _upload(b.s1, b.s2, b.tf1, b.tf2)
    runs = {}
    for n in (255, 256):
        runs[n] = _device_run(pkg, b, pkg.abi.default_collision_request(), d, n)
        assert runs[n]["same"], n
        got = witness(runs[n]["obs"], WITNESS)
        print("    %d queries of 200-triangle models: plan %s" % (n, dict(zip(WITNESS, got))))
        assert got == expected_plan(n, depth), n
    assert expected_plan(255, depth) == NO_TABLES and expected_plan(256, depth) == ONE_ROUND_256
    _same_decisions(dict(rec=runs[256]["rec"][:255]), runs[255], "200-triangle models, records [:255] of the run at 256 against the run at 255")


def test_reversed_order(pkg, big):
    """(f) the same pairs at other places of the batch: the first 220 001 queries in reversed order, un-reversed, against the forward run."""
    n = 220_001
    b = big.b
    d = big.upload(b.s1[:n][::-1], b.s2[:n][::-1], big.tf1[:n][::-1], big.tf2[:n][::-1])
    r = big.run(n, d=d)
    assert r["same"]
    assert witness(r["obs"], WITNESS) == expected_plan(n, big.depth)
    back = np.ascontiguousarray(r["rec"][::-1])
    fwd = big.at(n)
    _same_decisions(dict(rec=back), fwd, "%d queries in reversed order against the forward run" % n)
    print("    %d queries in reversed order: all bytes equal to the forward run's: %s" % (n, back.tobytes() == fwd["rec"].tobytes()))
    _check_records(pkg, back, big.ref[:n], "%d queries in reversed order" % n)


def test_fp32_two_round_plan(pkg, big):
    """(g) the fp32 instantiations of the same kernels at 220 001 queries, by the criteria of test_gpu_parity.py::test_bvh_collide_forms_agree's
    fp32 leg: the oracle's decisions where |d_ref| > 1e-3; the depth of a contact to 2e-4 in its 0.995 quantile, at most 0.5 % beyond."""
    n = 220_001
    sub = big.b.slice(0, n)
    r = big.run(n, d=big.upload(sub.s1, sub.s2, sub.pose1_f32, sub.pose2_f32), f32=True)
    g32, ref = r["rec"], big.ref[:n]
    print("    fp32, %d queries: plan %s" % (n, dict(zip(WITNESS, witness(r["obs"], WITNESS)))))
    assert witness(r["obs"], WITNESS) == expected_plan(n, big.depth)
    assert r["same"]
    clear = np.abs(ref["distance"]) > 1e-3
    assert np.array_equal(pkg.abi.status_contact(g32["status"])[clear] != 0, ref["num_contacts"][clear] > 0)
    hit = clear & (ref["num_contacts"] > 0)
    err = np.abs(g32["distance"][hit] - ref["distance"][hit])
    print("    fp32, %d queries: %d clear of the boundary, %d contacts among them; depth error: 0.995 quantile %.3g, %d beyond 2e-4" % (
        n, int(clear.sum()), int(hit.sum()), float(np.quantile(err, 0.995)), int((err > 2e-4).sum())))
    assert np.quantile(err, 0.995) < 2e-4 and (err > 2e-4).sum() < 0.005 * hit.sum()


def test_host_pipeline_two_plans_in_one_call(pkg, big):
    """(h) hfcl_collide_batch on all 500 001 queries in chunks of 220 001: two chunks of a size that gets the two-round plan, then 59 999 queries
    under the one-round plan, on ONE set of walk tables -- grown for the first chunk, reused by the smaller one.  The plan and the counters that
    can be read after a call are its LAST chunk's (every chunk notes and zeroes its own), so the call on all 500 001 shows the one-round plan only.
    The two-round plan of a 220 001-query chunk of the pipeline is observed by a call before it on the same library: the first 440 002 queries,
    two such chunks, whose second is that call's last."""
    b, c = big.b, 220_001
    lib = pkg.workloads.make_library(pkg, b)
    pkg.engine.dll().hfcl_debug_note_forms(lib._h, C.c_int(1))
    try:
        lib.set_host_chunk(c)
        first = lib.collide(b.s1[:2 * c], b.s2[:2 * c], big.tf1[:2 * c], big.tf2[:2 * c], big.req)
        obs2 = observe(pkg, lib)
        rec = lib.collide(b.s1, b.s2, big.tf1, big.tf2, big.req)
        obs = observe(pkg, lib)
    finally:
        lib.close()
    for what, o in (("the first %d queries" % (2 * c), obs2), ("all %d queries" % N_ALL, obs)):
        rc = o["mm_round_counters"]
        print("    host pipeline, %s: chunks %s, the largest %s; the last chunk's plan %s; its suspended queries %d; per round (queries that walk on, "
              "leaves listed, suspended when the round ended): %s" % (what, o["forms"].get("host_chunks"), o["forms"].get("host_max_chunk"),
                                                                       dict(zip(WITNESS, witness(o, WITNESS))), o["mm_suspended"], [(rc[8 * k + 2], rc[8 * k + 1], rc[8 * k + 3]) for k in range(2)]))
    assert obs2["forms"]["host_chunks"] == ["2"] and obs2["forms"]["host_max_chunk"] == [str(c)]
    assert witness(obs2, WITNESS) == expected_plan(c, big.depth) == TWO_ROUNDS_320
    rc = obs2["mm_round_counters"]
    assert rc[2] > 0 and rc[8 + 1] > 0 and rc[3] > 0 and obs2["mm_suspended"] > 0  # (round 1 and both continuations had work in that chunk)
    assert obs["forms"]["host_chunks"] == ["3"] and obs["forms"]["host_max_chunk"] == [str(c)]
    assert witness(obs, WITNESS) == expected_plan(N_ALL - 2 * c, big.depth) == ONE_ROUND_256
    rc = obs["mm_round_counters"]
    assert rc[2] == 0 and rc[8 + 1] == 0 and obs["mm_suspended"] > 0  # (no residue of the two-round chunks before it in the last chunk's counters)
    _same_decisions(dict(rec=first), dict(rec=big.at(N_ALL)["rec"][:2 * c]), "host pipeline, two chunks of %d, against the device run at %d" % (c, N_ALL))
    _same_decisions(dict(rec=rec), big.at(N_ALL), "host pipeline in chunks of %d against the device run at %d" % (c, N_ALL))
    _check_records(pkg, first, big.ref[:2 * c], "host pipeline, two chunks of %d" % c)
    _check_records(pkg, rec, big.ref, "host pipeline in chunks of %d" % c)


def test_task_levels_across_their_bound(pkg, big):
    """(i) bvh_coop = 0, the task-level form: a batch that fills the chip's lanes at most 1.5 times (2 n <= 3 * CUs * 512) has its queries cut at
    512 steps and the remainders spread over 12 levels of tasks of 16 steps; a larger one walks on its lanes (the compile-time budgets, 0: a unit
    suspends only when its stack is full; 6 levels)."""
    import torch
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    bound = 3 * n_cus * 512 // 2
    assert 256 <= bound < N_ALL, (n_cus, bound)
    paths = ("forms.mm_coop", "forms.mm_budget0", "forms.mm_budget", "forms.mm_levels", "forms.mm_rounds")
    want = {bound: [["0"], ["512"], ["16"], ["12"], ["0"]], bound + 1: [["0"], ["0"], ["0"], ["6"], ["0"]]}
    runs = {}
    for n in (bound, bound + 1):
        r = runs[n] = big.run(n, options={"bvh_coop": 0})
        got = witness(r["obs"], paths)
        print("    bvh_coop = 0, %d CUs, %d queries: %s; suspended queries %d, tasks %d" % (n_cus, n, dict(zip(paths, got)), r["obs"]["mm_suspended"], r["obs"]["mm_tasks"]))
        assert got == want[n], n
        assert r["same"], n
        _check_records(pkg, r["rec"], big.ref[:n], "bvh_coop = 0, %d queries" % n)
    assert runs[bound]["obs"]["mm_tasks"] > 0
    _same_decisions(dict(rec=runs[bound + 1]["rec"][:bound]), runs[bound], "bvh_coop = 0, records [:%d] of the run at %d against the run at %d" % (bound, bound + 1, bound))


@pytest.mark.parametrize("kind", ["collide", "distance"])
def test_mesh_solid_at_255_and_256(pkg, kind):
    """(j) mesh x solid has its own rules from 256 queries on (the split plan of the one-query-per-lane walk, the EPA queue's size): the options
    suite's mesh x solid batch at 255 and at 256 queries, the records of the first 255 byte for byte (these units are built without contraction)."""
    abi = pkg.abi
    b = _ms_batch(pkg)
    req = abi.default_collision_request() if kind == "collide" else abi.default_distance_request()
    d = _upload(b.s1, b.s2, b.tf1, b.tf2)
    runs = {}
    for n in (255, 256):
        runs[n] = _device_run(pkg, b, req, d, n, kind + "_device")
        assert runs[n]["same"], n
        print("    mesh x solid %s(), %d queries: ms_lane %s, ms_split %s, ms_coop %s, ms_budget0 %s" % (
            kind, n, *witness(runs[n]["obs"], ("forms.ms_lane", "forms.ms_split", "forms.ms_coop", "forms.ms_budget0"))))
    if kind == "collide":  # (mesh_solid_collide: the split plan from 256 queries on)
        assert witness(runs[255]["obs"], ("forms.ms_lane", "forms.ms_split", "forms.ms_coop")) == [["1"], ["0"], None]
        assert witness(runs[256]["obs"], ("forms.ms_lane", "forms.ms_split", "forms.ms_coop")) == [["1"], None, ["1"]]
    x, y = runs[256]["rec"][:255], runs[255]["rec"]
    differ = int((x.view(np.uint8).reshape(255, -1) != y.view(np.uint8).reshape(255, -1)).any(axis=1).sum())
    print("    mesh x solid %s(): %d of 255 records differ in a byte between the runs at 255 and at 256 queries" % (kind, differ))
    assert differ == 0
