#!/usr/bin/env python3
"""Scene queries against the per-pair calls: time per call and bytes moved, fp64 collide, on cfg5's broadphase scene (~1 M pairs, one
configuration) and on workloads.scene_planner at ~1 M queries.

  A  hfcl_collide_batch on host-expanded arrays (host clock; the host expansion is timed separately)
  B  hfcl_scene_collide, records and summaries (host clock)        C  ... summaries only
  D  hfcl_collide_batch_device on pre-expanded resident arrays (device events)
  E  hfcl_scene_collide_device, records and summaries (device events)   F  ... summaries only
  G  hfcl_scene_cull_device alone: boxes, mark, scan, emit (device events)
  H  hfcl_scene_collide_culled, summaries only (host clock; against C)
  I  hfcl_scene_cull_device, the count read back, hfcl_scene_collide_listed_device with records and summaries (device events; against E)
  J  the same through the fp32 path (against K)          K  hfcl_scene_collide_device_f32, records and summaries (device events)
  L  hfcl_scene_distance, summaries only (host clock)               M  hfcl_scene_nearest, summaries only (host clock; against L)
  N  hfcl_scene_distance_device, summaries only (device events)     O  hfcl_scene_nearest_device, summaries only (device events; against N)
  P, Q, R, S  the same four through the fp32 path
  T  the narrow phase of nearest's pass 1 alone: hfcl_scene_distance_listed_device on that list, summaries only (device events)
  U  ... of pass 2          V, W  the same two through the fp32 path
  X  hfcl_scene_self_pairs_device alone: boxes, count, scan, emit of ALL pairs of every configuration, no list (device events)
  Y  hfcl_scene_collide_self, summaries only (host clock)
  Z  what a caller had before X: per configuration engine.world_aabbs + engine.broadphase_self_pairs on the host, hfcl_scene_set_pairs,
     hfcl_scene_collide summaries only, all timed together (host clock; one-configuration workloads only; against Y)
  a  hfcl_scene_self_pairs_device, the count read back, hfcl_scene_collide_pairs_device with records and summaries (device events)
  b  the same list by the route that existed: a scene whose own list is all n (n - 1) / 2 pairs, hfcl_scene_cull_device, the count read
     back, hfcl_scene_collide_listed_device with records and summaries (device events; against a; scenes of at most 256 objects)
  c  hfcl_scene_self_pairs_device with the workload's object groups set (device events; robot workloads)
  d  hfcl_scene_collide_self with the groups set, summaries only (host clock)
  e  the same pairs as an explicit list: hfcl_scene_collide_culled on the workload's pair list, summaries only (host clock; against d;
     where the call is refused -- the list's workspace does not fit -- the row holds the refusal instead of a time)
  f  X on the same table without groups (device events; against c: what the skipping saves)
  g  hfcl_scene_nearest_self with the groups set, summaries only: the clearance from the poses and the groups alone (host clock)
  h  hfcl_scene_nearest_self_device, summaries only (device events)            i, j  the same two through the fp32 path
  k  the same answer from the explicit list: hfcl_scene_nearest on the workload's pair list, summaries only (host clock; against g; a
     refusal is kept in the place of a time, as in e)        l  hfcl_scene_nearest_device (device events; against h)
  m, n  the same two through the fp32 path
  o  the same answer from a guessed box filter: hfcl_scene_distance_self with the groups set, summaries only, `inflate` = the scene's true
     clearance taken from g -- the best possible guess (host clock; against g)        p  the same through the fp32 path
  q  o on the device: hfcl_scene_self_pairs_device at that inflate, the count read back, hfcl_scene_distance_pairs_device, summaries only
     (device events; against h)        r  the same through the fp32 path
  s  hfcl_scene_env_pairs_device with the groups set: the list from the links' poses alone, the obstacles an environment set once (device
     events; against c)
  t  hfcl_scene_collide_env, summaries only (host clock; against d)        u  hfcl_scene_distance_env, summaries only (host clock)
  v  t on the device: hfcl_scene_env_pairs_device, the count read back, hfcl_scene_collide_env_pairs_device, summaries only (device events)
  w  the same with hfcl_scene_distance_env_pairs_device
     s .. w report the bytes of the table a call takes against those of the full table, and whether the list is that of c.  Workloads
     whose name ends in "s" have the obstacles in engine.spatial_order; robot32x65536x4096 (4 096 configurations: a full table of 25.8 GB)
     runs s .. w alone.
  x  hfcl_scene_nearest_env with the groups set, clearances only: g from the links' poses alone (host clock; against g and k)
  y  hfcl_scene_nearest_env_device, clearances only (device events; against h and l)        z, 1  the same two through the fp32 path
  2, 3, 4, 5  x, y, z, 1 with scene_nearest_env_prune=0: no environment tile dropped by its distance
     x .. 5 report the pairs each pass evaluates, whether the clearances are those of g and -- from tests/nearest_env_model.py, with
     the thresholds recomputed on the host -- the (16 rows, tile) cells each pass drops by distance.  robot32x65536x4096 runs them too.
X .. b ignore the workload's pair list.  --options key=value,... sets library options in the worker (scene_pairs_small_max=0: the tiled form;
scene_pairs_sorted=1: the list of X, Y, a by sort and sweep -- profiles/r24_a_pairs_sorted.md; the row reports the form that ran).
cfg5x4 / cfg5x16: cfg5's scene with 4 / 16 times the objects at the same density (400 000 / 1 600 000 objects, 4 M / 16 M pairs);
cfg5n1000 .. cfg5n50000: with that many objects.
The culled forms run at --inflate (default 0: the reference's manager).  planner2048: scene_planner(2048, 16), 215 040 queries;
planner2048x32: scene_planner(2048, 32), 952 320 queries.  robot16x4096 / robot32x65536: workloads.scene_robot_env, 16 links and 4 096
obstacles in 256 configurations / 32 links and 65 536 obstacles in 8; rows c .. 5 run on these alone, and c .. e only in a library that
has object groups, g .. r only in one that has hfcl_scene_nearest_self, x .. 5 only in one that has hfcl_scene_nearest_env.  They report, from tests/groups_model.py, the share of column tiles the sweep skips and of row blocks that leave at once.  L .. W report the share of the queries each pass of nearest evaluates.
Rows L .. W import the numpy model of the selection from tests/nearest_model.py: the lists of T .. W (the library keeps its own in its
workspace) and the fp32 (lb - d_f32) / M come from it; no other row depends on tests/.

Every measurement runs in a child process.  Up to three arms, each a library selected with HFCL_LIB_PATH in the child, run every row that
--forms names, in an order that rotates from round to round: "parent", a library built from the parent commit's sources (--parent-lib,
when the file is there); "new", the build under test; "control", a copy of the build under test (--control-lib) -- the same code loaded
from another file, so what it loses against "new" is the noise of the run.  Warm-up calls first, then --calls timed calls: median, min, max.

  python tools/scene_bench.py [--parent-lib build/ab/lib_parent.so] [--control-lib build/ab/lib_control.so] [--calls 12] [--rounds 2] [--out profiles/x.json]
  python tools/scene_bench.py --worker --workload cfg5 --forms A,D     (one child; prints one JSON line)
  python tools/scene_bench.py --workloads planner2048,planner2048x32 --forms L,M,N,O,P,Q,R,S,T,U,V,W     (the pruned minimum distance)"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


ROBOTS = {"robot16x4096": (256, 16, 4096), "robot32x65536": (8, 32, 65536)}  # (configurations, links, obstacles)
ROBOTS.update({k + "s": v for k, v in list(ROBOTS.items())})  # ... the obstacles in spatial order
ENV_ONLY = {"robot32x65536x4096": (4096, 32, 65536), "robot32x65536x4096s": (4096, 32, 65536)}  # (no full table: the env forms alone)
ENV_FORMS = "stuvwxyz12345"
CFG5_SIZES = {"cfg5": 100_000, "cfg5x4": 400_000, "cfg5x16": 1_600_000}
CFG5_SIZES.update({"cfg5n%d" % n: n for n in (1000, 2000, 5000, 10000, 20000, 50000)})  # (the crossover of the two ways to the self pairs)
NENV_FORMS = "xyz12345"


def _workload(pkg, name):
    wl = pkg.workloads
    if name in ROBOTS or name in ENV_ONLY:
        if "split" not in wl.scene_robot_env.__code__.co_varnames:  # (a parent build's package: the rows that exist there)
            sc, groups, pairs = wl.scene_robot_env(*ROBOTS[name])
            return sc.lib, sc.obj_shape, pairs, sc.obj_tf, groups, None
        sc, groups, pairs, split, split32 = wl.scene_robot_env(*(ROBOTS.get(name) or ENV_ONLY[name]), split=True, spatial=name.endswith("s"),
                                                         full=name in ROBOTS)
        return sc.lib, sc.obj_shape, pairs, sc.obj_tf, groups, split + split32
    if name in CFG5_SIZES:  # (cfg5's scene with other numbers of objects in a cube of the same density: ten touching pairs an object)
        b = wl.cfg5_broadphase_scene(n_objects=CFG5_SIZES[name], target_pairs=10 * CFG5_SIZES[name])
        sc = b.scene
        return b.lib, sc["obj_shape"], sc["pairs"], sc["obj_tf"].reshape(1, -1, 12), None, None
    if name == "planner2048x32":
        ps = wl.scene_planner(n_conf=2048, n_objects=32)
    elif name == "planner256x64":
        ps = wl.scene_planner(n_conf=256, n_objects=64)
    else:
        ps = wl.scene_planner(n_conf=2048 if name == "planner2048" else 9984, n_objects=16)
    return ps.lib, ps.obj_shape, ps.pairs, ps.obj_tf, None, None


def _dropped_cells(pkg, lib, obj_shape, groups, boxes, table, n_moving, f32):
    """The (16 rows, environment tile) cells each pass of nearest_env drops by distance at upper_bound = inf, from the boxes: the seed and
    pass 1 by the numpy model's bound, the thresholds from the per-pair distance call on pass 1's pairs."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import nearest_env_model as nem
    import nearest_model
    r = nearest_model.R32 if f32 else nearest_model.R64
    n_conf, n = boxes.shape[:2]
    cand = nem.candidates(n_moving, n, groups)
    seed, thr = np.zeros(n_conf, dtype=np.uint64), np.zeros(n_conf)
    dreq = pkg.abi.default_distance_request()
    for c in range(n_conf):
        L = nearest_model.bound(boxes[c, :n_moving, None, :], boxes[c, None, :, :], r)
        first = int(np.where(cand, L, np.inf).argmin())
        seed[c] = (first // n) << 32 | (first % n)
        in1 = cand & np.isneginf(L)
        in1[first // n, first % n] = True
        i, j = np.nonzero(in1)
        fn = lib.distance_f32 if f32 else lib.distance
        rec = fn(obj_shape[i], obj_shape[j], np.ascontiguousarray(table[c, i]), np.ascontiguousarray(table[c, j]), dreq)
        d = rec["distance"].astype(np.float64)
        thr[c] = d[~np.isnan(d)].min() if len(d) else np.inf
    drop1, drop2, _ = nem.dropped_cells({"seed": seed, "thr": thr}, boxes, n_moving, r)
    return {"cells": int(drop1.size), "dropped_pass1": int(drop1.sum()), "dropped_pass2": int(drop2.sum())}


def _stats(ms):
    ms = sorted(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": ms[0], "max_ms": ms[-1], "calls": len(ms)}


def worker(args):
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_pkg()
    abi = pkg.abi
    L, obj_shape, pairs, table, groups, split = _workload(pkg, args.workload)
    n_conf, G, P = table.shape[0], table.shape[1], len(pairs)
    n = n_conf * P
    i, j = pairs[:, 0], pairs[:, 1]
    lib = pkg.Library(L, options=dict(kv.split("=") for kv in args.options.split(",") if kv))
    req = abi.default_collision_request()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    out = {"workload": args.workload, "lib": os.path.relpath(os.environ["HFCL_LIB_PATH"], ROOT) if "HFCL_LIB_PATH" in os.environ else "in-tree", "n_conf": n_conf, "n_objects": G, "n_pairs": P, "queries": n,
           "forms": {}}

    def expand():
        return (np.tile(obj_shape[i], n_conf), np.tile(obj_shape[j], n_conf), np.ascontiguousarray(table[:, i].reshape(n, 12)),
                np.ascontiguousarray(table[:, j].reshape(n, 12)))

    def host_clock(fn):
        for _ in range(args.warmup):
            fn()
        ms = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            fn()
            ms.append(1e3 * (time.perf_counter() - t0))
        return _stats(ms)

    def device_clock(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(float(e0.elapsed_time(e1)))
        return _stats(ms)

    forms = args.forms.split(",")
    if args.workload in ENV_ONLY:  # (the table holds configuration 0 alone)
        forms = [f for f in forms if f in ENV_FORMS]
    scene = lib.scene(obj_shape, pairs if args.workload not in ENV_ONLY else pairs[:0]) if set(forms) & set("BCEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz12345") else None
    if "A" in forms or "D" in forms:
        t0 = time.perf_counter()
        s1, s2, tf1, tf2 = expand()
        out["host_expansion_ms"] = 1e3 * (time.perf_counter() - t0)
    if "A" in forms:
        out["forms"]["A"] = host_clock(lambda: lib.collide(s1, s2, tf1, tf2, req))
    if "B" in forms:
        out["forms"]["B"] = host_clock(lambda: scene.collide(table, req))
    if "C" in forms:
        out["forms"]["C"] = host_clock(lambda: scene.collide(table, req, records=False))
    if "D" in forms:
        d = [torch.from_numpy(x).to(dev) for x in (s1.astype(np.int32), s2.astype(np.int32), tf1, tf2)]
        d_out = torch.zeros(n * 24, dtype=torch.int32, device=dev)
        out["forms"]["D"] = device_clock(lambda: lib.collide_device(*d, n, req, d_out, stream=st))
    if "E" in forms or "F" in forms:
        d_tab = torch.from_numpy(np.ascontiguousarray(table)).to(dev)
        d_sum = torch.zeros(n_conf * 6, dtype=torch.int32, device=dev)
    if "E" in forms:
        d_rec = torch.zeros(n * 24, dtype=torch.int32, device=dev)
        out["forms"]["E"] = device_clock(lambda: scene.collide_device(d_tab, n_conf, req, d_rec, d_sum, stream=st))
    if "F" in forms:
        out["forms"]["F"] = device_clock(lambda: scene.collide_device(d_tab, n_conf, req, None, d_sum, stream=st))
    if set(forms) & set("GHIJK"):
        ids, _ = scene.cull(table, args.inflate)
        out["inflate"] = args.inflate
        out["n_listed"] = int(len(ids))
        # the cull's byte model: the pose table in, 8 B of pair list per query, 8 B per survivor out (boxes and pair rows: cached)
        out["cull_model_bytes"] = 96.0 * n_conf * G + 8.0 * n + 8.0 * len(ids)
        d_tab64 = torch.from_numpy(np.ascontiguousarray(table)).to(dev)
        d_ids = torch.zeros(max(len(ids), 1), dtype=torch.int64, device=dev)
        d_cb = torch.zeros(n_conf + 1, dtype=torch.int64, device=dev)
        d_n = torch.zeros(1, dtype=torch.int64, device=dev)
        d_sum2 = torch.zeros(n_conf * 6, dtype=torch.int32, device=dev)

        def culled_device(d_table, d_records, f32):
            scene.cull_device(d_table, n_conf, args.inflate, d_ids, len(d_ids), d_cb, d_n, f32=f32, stream=st)
            k = int(d_n.item())  # the one read-back: 8 bytes
            fn = scene.collide_listed_device_f32 if f32 else scene.collide_listed_device
            fn(d_table, n_conf, d_ids, min(k, len(d_ids)), d_cb, req, d_records, d_sum2, stream=st)
    if "G" in forms:
        out["forms"]["G"] = device_clock(lambda: scene.cull_device(d_tab64, n_conf, args.inflate, d_ids, len(d_ids), d_cb, d_n, stream=st))
    if "H" in forms:
        out["forms"]["H"] = host_clock(lambda: scene.collide_culled(table, args.inflate, req, records=False, want_ids=False))
    if "I" in forms:
        d_rec2 = torch.zeros(max(len(ids), 1) * 24, dtype=torch.int32, device=dev)
        out["forms"]["I"] = device_clock(lambda: culled_device(d_tab64, d_rec2, False))
    if set(forms) & set("JKPQRSVWijmnpr"):
        # 7-float poses of the same table: quaternions from the rotation matrices (w from the trace; the planner's and cfg5's rotations are
        # generic, no w near 0)
        R = pkg.geometry.pose_R(table.reshape(-1, 12))
        w4 = np.sqrt(np.maximum(1.0 + R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2], 1e-12)) * 2.0
        quat = np.stack([0.25 * w4, (R[:, 2, 1] - R[:, 1, 2]) / w4, (R[:, 0, 2] - R[:, 2, 0]) / w4, (R[:, 1, 0] - R[:, 0, 1]) / w4], axis=1)
        pose = pkg.geometry.pose_f32_from_quat(quat / np.linalg.norm(quat, axis=1, keepdims=True), table.reshape(-1, 12)[:, 9:]).reshape(n_conf, G, 7)
        d_pose = torch.from_numpy(np.ascontiguousarray(pose)).to(dev)
    if "K" in forms:
        d_rec32 = torch.zeros(n * 11, dtype=torch.int32, device=dev)
        out["forms"]["K"] = device_clock(lambda: scene.collide_device_f32(d_pose, n_conf, req, d_rec32, d_sum2, stream=st))
    if "J" in forms:
        ids32, _ = scene.cull(pose, args.inflate)
        d_ids = torch.zeros(max(len(ids32), len(ids), 1), dtype=torch.int64, device=dev)
        d_rec32c = torch.zeros(len(d_ids) * 11, dtype=torch.int32, device=dev)
        out["forms"]["J"] = device_clock(lambda: culled_device(d_pose, d_rec32c, True))
    if set(forms) & set("LMNOPQRSTUVW"):  # the pruned minimum distance against the unculled summaries-only call
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import nearest_model
        dreq = abi.default_distance_request()
        d_sum3 = torch.zeros(n_conf * 6, dtype=torch.int32, device=dev)
        for f32, letters in ((False, "LMNOTU"), (True, "PQRSVW")):
            if not set(forms) & set(letters):
                continue
            tab = pose if f32 else table
            d_t = d_pose if f32 else torch.from_numpy(np.ascontiguousarray(table)).to(dev)
            host_full = scene.distance_f32 if f32 else scene.distance
            host_near = scene.nearest_f32 if f32 else scene.nearest
            dev_full = scene.distance_device_f32 if f32 else scene.distance_device
            dev_near = scene.nearest_device_f32 if f32 else scene.nearest_device
            listed = scene.distance_listed_device_f32 if f32 else scene.distance_listed_device
            summ, _, n_eval = host_near(tab, dreq, records=False)
            rec, full = host_full(tab, dreq)
            key = "nearest_f32" if f32 else "nearest"
            out[key] = {"evaluated": list(n_eval), "share_pct": [100.0 * k / n for k in n_eval],
                        "equal_to_unculled": bool(summ["min_distance"].tobytes() == full["min_distance"].tobytes() and
                                                  summ["min_pair"].tobytes() == full["min_pair"].tobytes())}
            if f32:  # what the fp32 rounding term of the bound has to cover
                boxes = scene.world_aabbs(tab)
                lb, _, M = nearest_model.raw_bound(boxes[:, pairs[:, 0]], boxes[:, pairs[:, 1]])
                ok = (np.isfinite(lb) & (lb > 0)).reshape(-1)
                out[key]["max_lb_minus_d_over_M"] = float(((lb.reshape(-1) - rec["distance"].astype(np.float64)) / M.reshape(-1))[ok].max())
            if letters[0] in forms:
                out["forms"][letters[0]] = host_clock(lambda: host_full(tab, dreq, records=False))
            if letters[1] in forms:
                out["forms"][letters[1]] = host_clock(lambda: host_near(tab, dreq, records=False))
            if letters[2] in forms:
                out["forms"][letters[2]] = device_clock(lambda: dev_full(d_t, n_conf, dreq, None, d_sum3, stream=st))
            if letters[3] in forms:
                out["forms"][letters[3]] = device_clock(lambda: dev_near(d_t, n_conf, dreq, d_sum3, None, stream=st))
            if letters[4] in forms or letters[5] in forms:
                L_ = nearest_model.query_bounds(scene.world_aabbs(tab), pairs, nearest_model.R32 if f32 else nearest_model.R64)
                sel = nearest_model.select(abi, L_, rec, np.inf)
                assert (len(sel["ids1"]), len(sel["ids2"])) == tuple(n_eval)
                for letter, k in ((letters[4], "1"), (letters[5], "2")):
                    if letter not in forms:
                        continue
                    d_l = torch.from_numpy(sel["ids" + k].view(np.int64)).to(dev)
                    d_c = torch.from_numpy(sel["conf_begin" + k].view(np.int64)).to(dev)
                    m = len(sel["ids" + k])
                    out["forms"][letter] = device_clock(lambda: listed(d_t, n_conf, d_l, m, d_c, dreq, None, d_sum3, stream=st))
    if set(forms) & set("XYZab"):  # the pairs made on the device, no list
        d_tab_p = torch.from_numpy(np.ascontiguousarray(table)).to(dev)
        sp, sp_cb = scene.self_pairs(table, args.inflate)
        out["self_pairs"] = {"n_listed": int(len(sp)), "box_tests": n_conf * G * (G - 1) // 2, "options": args.options}
        if hasattr(scene, "last_pairs_form"):  # (0 tiled, 1 wave per configuration, 2 sort and sweep: option scene_pairs_sorted)
            out["self_pairs"]["form"] = scene.last_pairs_form()
        if args.workload.startswith("cfg5") and args.inflate == 0.0:
            out["self_pairs"]["equals_host_broadphase"] = bool(sp.tobytes() == np.ascontiguousarray(pairs.astype(np.uint32)).tobytes())
        cap = max(len(sp), 1)
        d_sp = torch.zeros(2 * cap, dtype=torch.int32, device=dev)
        d_spcb = torch.zeros(n_conf + 1, dtype=torch.int64, device=dev)
        d_spn = torch.zeros(1, dtype=torch.int64, device=dev)
        d_sum4 = torch.zeros(n_conf * 6, dtype=torch.int32, device=dev)
    if "X" in forms:
        out["forms"]["X"] = device_clock(lambda: scene.self_pairs_device(d_tab_p, n_conf, args.inflate, d_sp, cap, d_spcb, d_spn, stream=st))
    if "Y" in forms:
        out["forms"]["Y"] = host_clock(lambda: scene.collide_self(table, req, args.inflate, records=False))
    if "Z" in forms and n_conf == 1:
        def host_route():
            boxes = pkg.engine.world_aabbs(L, obj_shape, table[0])
            scene.set_pairs(pkg.engine.broadphase_self_pairs(boxes))
            return scene.collide(table, req, records=False)
        summ_host = host_route()
        out["self_pairs"]["host_route_equal"] = bool(summ_host.tobytes() == scene.collide_self(table, req, 0.0, records=False)[3].tobytes()) if args.inflate == 0.0 else None
        out["forms"]["Z"] = host_clock(host_route)
        scene.set_pairs(pairs)
    if "a" in forms:
        d_rec_p = torch.zeros(cap * 24, dtype=torch.int32, device=dev)

        def self_device():
            scene.self_pairs_device(d_tab_p, n_conf, args.inflate, d_sp, cap, d_spcb, d_spn, stream=st)
            k = int(d_spn.item())  # the one read-back: 8 bytes
            scene.collide_pairs_device(d_tab_p, n_conf, d_sp, min(k, cap), d_spcb, req, d_rec_p, d_sum4, stream=st)
        out["forms"]["a"] = device_clock(self_device)
    if "b" in forms and G <= 256:
        ti, tj = np.triu_indices(G, 1)
        every = lib.scene(obj_shape, np.stack([ti, tj], axis=1).astype(np.uint32))
        d_ids_b = torch.zeros(cap, dtype=torch.int64, device=dev)
        d_rec_b = torch.zeros(cap * 24, dtype=torch.int32, device=dev)

        def culled_all_pairs():
            every.cull_device(d_tab_p, n_conf, args.inflate, d_ids_b, cap, d_spcb, d_spn, stream=st)
            k = int(d_spn.item())
            every.collide_listed_device(d_tab_p, n_conf, d_ids_b, min(k, cap), d_spcb, req, d_rec_b, d_sum4, stream=st)
        out["forms"]["b"] = device_clock(culled_all_pairs)
        torch.cuda.synchronize()
        every.close()
    if set(forms) & set("cdef") and groups is not None:  # object groups on the device-made lists, against the explicit list and no groups
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import groups_model
        d_tab_g = torch.from_numpy(np.ascontiguousarray(table)).to(dev)
        d_gcb = torch.zeros(n_conf + 1, dtype=torch.int64, device=dev)
        d_gn = torch.zeros(1, dtype=torch.int64, device=dev)
        has_groups = hasattr(pkg.engine.dll(), "hfcl_scene_set_groups") and hasattr(scene, "set_groups")
        skips, tiles, early, blocks = groups_model.skipped(*groups)
        out["groups"] = {"n_groups": int(len(groups[1])), "tiles_skipped_pct": 100.0 * skips / max(tiles, 1), "blocks_left_early_pct": 100.0 * early / blocks,
                         "box_tests": n_conf * G * (G - 1) // 2, "allowed_pairs": n_conf * P}

        def count_only():
            scene.self_pairs_device(d_tab_g, n_conf, args.inflate, None, 0, d_gcb, d_gn, stream=st)
            return int(d_gn.item())
        if has_groups and set(forms) & set("cde"):
            scene.set_groups(*groups)
            cap_g = max(count_only(), 1)
            out["groups"]["n_listed"] = cap_g
            d_gp = torch.zeros(2 * cap_g, dtype=torch.int32, device=dev)
            if "c" in forms:
                out["forms"]["c"] = device_clock(lambda: scene.self_pairs_device(d_tab_g, n_conf, args.inflate, d_gp, cap_g, d_gcb, d_gn, stream=st))
            if "d" in forms:
                summ_d = scene.collide_self(table, req, args.inflate, records=False)[3]
                out["forms"]["d"] = host_clock(lambda: scene.collide_self(table, req, args.inflate, records=False))
            del d_gp
            scene.clear_groups()
            if "e" in forms:
                try:
                    summ_e = scene.collide_culled(table, args.inflate, req, records=False, want_ids=False)[3]
                    out["forms"]["e"] = host_clock(lambda: scene.collide_culled(table, args.inflate, req, records=False, want_ids=False))
                    if "d" in forms:
                        out["groups"]["d_equals_e"] = bool(all(summ_d[k].tobytes() == summ_e[k].tobytes() for k in ("min_distance", "n_contacts", "n_skipped")))
                except pkg.EngineError as err:
                    out["groups"]["e_refused"] = str(err)
        if "f" in forms:
            cap_f = max(count_only(), 1)
            out["groups"]["n_listed_without_groups"] = cap_f
            d_fp = torch.zeros(2 * cap_f, dtype=torch.int32, device=dev)
            out["forms"]["f"] = device_clock(lambda: scene.self_pairs_device(d_tab_g, n_conf, args.inflate, d_fp, cap_f, d_gcb, d_gn, stream=st))
    if set(forms) & set("ghijklmnopqr") and groups is not None and hasattr(scene, "nearest_self"):  # the clearance on device-made pairs
        dreq = abi.default_distance_request()
        d_clear = torch.zeros(n_conf * 6, dtype=torch.int32, device=dev)
        d_sum5 = torch.zeros(n_conf * 6, dtype=torch.int32, device=dev)
        d_ncb = torch.zeros(n_conf + 1, dtype=torch.int64, device=dev)
        d_nn = torch.zeros(1, dtype=torch.int64, device=dev)
        info = out["nearest_self"] = {"candidates": n_conf * P}
        for f32, letters in ((False, "ghkloq"), (True, "ijmnpr")):
            if not set(forms) & set(letters):
                continue
            tab = pose if f32 else table
            d_t = d_pose if f32 else torch.from_numpy(np.ascontiguousarray(table)).to(dev)
            tag = "f32" if f32 else "f64"
            scene.set_groups(*groups)
            clear, _, n_eval = scene.nearest_self(tab, dreq, records=False)
            info["evaluated_" + tag] = list(n_eval)
            true_clearance = float(max(clear["min_distance"].max(), 0.0))
            info["inflate_" + tag] = true_clearance
            if letters[0] in forms:
                out["forms"][letters[0]] = host_clock(lambda: scene.nearest_self(tab, dreq, records=False))
            if letters[1] in forms:
                fn = scene.nearest_self_device_f32 if f32 else scene.nearest_self_device
                out["forms"][letters[1]] = device_clock(lambda: fn(d_t, n_conf, dreq, d_clear, None, stream=st))
            if letters[4] in forms:
                summ_o = scene.distance_self(tab, dreq, true_clearance, records=False)[3]
                info["o_equal_" + tag] = bool(summ_o["min_distance"].tobytes() == clear["min_distance"].tobytes())
                out["forms"][letters[4]] = host_clock(lambda: scene.distance_self(tab, dreq, true_clearance, records=False))
            if letters[5] in forms:
                def count_at():
                    scene.self_pairs_device(d_t, n_conf, true_clearance, None, 0, d_ncb, d_nn, f32=f32, stream=st)
                    return int(d_nn.item())
                cap_q = max(count_at(), 1)
                info["listed_at_inflate_" + tag] = cap_q
                d_qp = torch.zeros(2 * cap_q, dtype=torch.int32, device=dev)
                pairs_fn = scene.distance_pairs_device_f32 if f32 else scene.distance_pairs_device

                def filtered_device():
                    scene.self_pairs_device(d_t, n_conf, true_clearance, d_qp, cap_q, d_ncb, d_nn, f32=f32, stream=st)
                    k = int(d_nn.item())  # the one read-back: 8 bytes
                    pairs_fn(d_t, n_conf, d_qp, min(k, cap_q), d_ncb, dreq, None, d_sum5, stream=st)
                out["forms"][letters[5]] = device_clock(filtered_device)
                del d_qp
            scene.clear_groups()
            try:  # the explicit list
                summ_k, _, n_k = (scene.nearest_f32 if f32 else scene.nearest)(tab, dreq, records=False)
                info["k_equal_" + tag] = bool(summ_k["min_distance"].tobytes() == clear["min_distance"].tobytes() and tuple(n_k) == tuple(n_eval))
                if letters[2] in forms:
                    near = scene.nearest_f32 if f32 else scene.nearest
                    out["forms"][letters[2]] = host_clock(lambda: near(tab, dreq, records=False))
                if letters[3] in forms:
                    near_d = scene.nearest_device_f32 if f32 else scene.nearest_device
                    out["forms"][letters[3]] = device_clock(lambda: near_d(d_t, n_conf, dreq, d_sum5, None, stream=st))
            except pkg.EngineError as err:
                info["k_refused_" + tag] = str(err)
    if set(forms) & set(ENV_FORMS) and split is not None and hasattr(scene, "set_environment"):  # a static environment kept on the device
        moving_tf, env_tf = split[:2]
        m_conf, n_links = moving_tf.shape[:2]
        dreq = abi.default_distance_request()
        scene.set_groups(*groups)
        t0 = time.perf_counter()
        scene.set_environment(n_links, env_tf)
        info = out["env"] = {"n_conf": m_conf, "n_moving": n_links, "n_env": int(len(env_tf)), "set_environment_ms": 1e3 * (time.perf_counter() - t0),
                             "table_bytes": int(moving_tf.nbytes), "full_table_bytes": 96 * m_conf * (n_links + len(env_tf)), "options": args.options}
        d_mov = torch.from_numpy(np.ascontiguousarray(moving_tf)).to(dev)
        d_ecb = torch.zeros(m_conf + 1, dtype=torch.int64, device=dev)
        d_en = torch.zeros(1, dtype=torch.int64, device=dev)
        d_esum = torch.zeros(m_conf * 6, dtype=torch.int32, device=dev)
        scene.env_pairs_device(d_mov, m_conf, args.inflate, None, 0, d_ecb, d_en, stream=st)
        cap_e = max(int(d_en.item()), 1)
        info["n_listed"] = cap_e
        d_ep = torch.zeros(2 * cap_e, dtype=torch.int32, device=dev)
        if args.workload in ROBOTS:  # the list is the groups sweep's
            ep, ecb = scene.env_pairs(moving_tf, args.inflate)
            gp, gcb = scene.self_pairs(table, args.inflate)
            info["equal_to_groups_list"] = bool(ep.tobytes() == gp.tobytes() and ecb.tobytes() == gcb.tobytes())
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import env_model
            skipped, cells, _ = env_model.skipped_by_box(scene.world_aabbs(table), n_links, args.inflate)
            info["cells_skipped_by_box_pct"] = 100.0 * float(skipped.sum()) / max(m_conf * cells, 1)

        def env_device(fn, req_):
            scene.env_pairs_device(d_mov, m_conf, args.inflate, d_ep, cap_e, d_ecb, d_en, stream=st)
            k = int(d_en.item())  # the one read-back: 8 bytes
            fn(d_mov, m_conf, d_ep, min(k, cap_e), d_ecb, req_, None, d_esum, stream=st)
        if "s" in forms:
            out["forms"]["s"] = device_clock(lambda: scene.env_pairs_device(d_mov, m_conf, args.inflate, d_ep, cap_e, d_ecb, d_en, stream=st))
        if "t" in forms:
            out["forms"]["t"] = host_clock(lambda: scene.collide_env(moving_tf, req, args.inflate, records=False))
        if "u" in forms:
            out["forms"]["u"] = host_clock(lambda: scene.distance_env(moving_tf, dreq, args.inflate, records=False))
        if "v" in forms:
            out["forms"]["v"] = device_clock(lambda: env_device(scene.collide_env_pairs_device, req))
        if "w" in forms:
            out["forms"]["w"] = device_clock(lambda: env_device(scene.distance_env_pairs_device, dreq))
        if set(forms) & set(NENV_FORMS) and hasattr(scene, "nearest_env") and hasattr(pkg.engine.dll(), "hfcl_scene_nearest_env"):  # the clearance from the links' poses alone
            ninfo = out["nearest_env"] = {"candidates": m_conf * P}
            d_nclear = torch.zeros(m_conf * 6, dtype=torch.int32, device=dev)
            for f32, letters in ((False, "xy23"), (True, "z145")):
                if not set(forms) & set(letters):
                    continue
                tag = "f32" if f32 else "f64"
                mov = split[2] if f32 else moving_tf
                scene.set_environment(n_links, split[3] if f32 else env_tf)
                d_m = torch.from_numpy(np.ascontiguousarray(mov)).to(dev)
                fn_d = scene.nearest_env_device_f32 if f32 else scene.nearest_env_device
                clear = {}
                for prune, (host_letter, dev_letter) in ((1, letters[:2]), (0, letters[2:])):
                    lib.set_option("scene_nearest_env_prune", prune)
                    clear[prune], _, n_eval = scene.nearest_env(mov, dreq, records=False)
                    ninfo["evaluated_" + tag] = list(n_eval)
                    if host_letter in forms:
                        out["forms"][host_letter] = host_clock(lambda: scene.nearest_env(mov, dreq, records=False))
                    if dev_letter in forms:
                        out["forms"][dev_letter] = device_clock(lambda: fn_d(d_m, m_conf, dreq, d_nclear, None, stream=st))
                lib.set_option("scene_nearest_env_prune", 1)
                ninfo["prune_off_equal_" + tag] = bool(clear[0].tobytes() == clear[1].tobytes())
                if args.workload in ROBOTS:  # the same answer from the full table; the cells each pass drops
                    tab = table
                    if f32:
                        tab = np.ascontiguousarray(np.concatenate([mov, np.broadcast_to(split[3][None], (m_conf,) + split[3].shape)], axis=1))
                    want, _, n_want = scene.nearest_self(tab, dreq, records=False)
                    ninfo["equal_to_nearest_self_" + tag] = bool(want.tobytes() == clear[1].tobytes() and tuple(n_want) == tuple(n_eval))
                    ninfo["cells_" + tag] = _dropped_cells(pkg, lib, obj_shape, groups, scene.world_aabbs(tab), tab, n_links, f32)
        scene.clear_groups()
        scene.clear_environment()
    torch.cuda.synchronize()
    if scene is not None:
        scene.close()
    lib.close()
    print("SCENE_BENCH " + json.dumps(out), flush=True)


def bytes_moved(n_conf, G, P):
    """Bytes per query over the host link (in / out) and through HBM by the expansion and the fold, from the shapes."""
    n = n_conf * P
    table = 96.0 * n_conf * G
    ids = 8.0 * P + 4.0 * G
    return {
        "A": {"link_in": 200.0, "link_out": 96.0},
        "B": {"link_in": (table + ids) / n, "link_out": 96.0 + 24.0 * n_conf / n},
        "C": {"link_in": (table + ids) / n, "link_out": 24.0 * n_conf / n},
        "expand_hbm": 8.0 + 2 * 96.0 + 8.0,       # pair list in (read once per configuration), two pose rows and two ids out (rows come from cache)
        "fold_hbm": 12.0,                         # distance and status of a record (the lines they sit in: up to 2 x 64 B of a 96-B record)
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--workload", default="cfg5", choices=sorted(CFG5_SIZES) + ["planner", "planner2048", "planner2048x32", "planner256x64"] + sorted(ROBOTS) + sorted(ENV_ONLY))
    ap.add_argument("--workloads", default="cfg5,planner", help="the workloads of a full run, comma-separated")
    ap.add_argument("--inflate", type=float, default=0.0)
    ap.add_argument("--options", default="", help="library options of the worker: key=value,...")
    ap.add_argument("--forms", default="A,B,C,D,E,F")
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "build", "ab", "lib_parent.so"))
    ap.add_argument("--control-lib", default=None, help="a copy of the library under test: the control arm")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    arms = [("new", None)]
    if os.path.exists(args.parent_lib):
        arms.insert(0, ("parent", os.path.abspath(args.parent_lib)))
    if args.control_lib:
        if not os.path.exists(args.control_lib):
            sys.exit("--control-lib %s: no such file" % args.control_lib)
        arms.append(("control", os.path.abspath(args.control_lib)))
    results = []
    for workload in args.workloads.split(","):
        for rnd in range(args.rounds):
            for which, lib_path in arms[rnd % len(arms):] + arms[:rnd % len(arms)]:
                env = dict(os.environ)
                env.pop("HFCL_LIB_PATH", None)
                if lib_path:
                    env["HFCL_LIB_PATH"] = lib_path
                cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--workload", workload, "--calls", str(args.calls), "--warmup",
                       str(args.warmup), "--inflate", str(args.inflate), "--forms", args.forms, "--options", args.options]
                r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
                line = [x for x in r.stdout.splitlines() if x.startswith("SCENE_BENCH ")]
                if r.returncode != 0 or not line:  # a child that failed ends the run: nothing more is started on the device
                    print(r.stdout[-2000:], r.stderr[-4000:])
                    sys.exit("worker failed (%s, %s): exit status %d" % (workload, which, r.returncode))
                res = json.loads(line[0][len("SCENE_BENCH "):])
                res["build"] = which
                results.append(res)
                print(json.dumps(res), flush=True)
    for workload in args.workloads.split(","):
        rs = [r for r in results if r["workload"] == workload]
        if not rs:
            continue
        r0 = rs[0]
        print("\n%s: %d configurations x %d pairs = %d queries, %d objects" % (workload, r0["n_conf"], r0["n_pairs"], r0["queries"], r0["n_objects"]))
        print("| form | build | median ms | min .. max ms (over the runs) |")
        print("|---|---|---|---|")
        for which in ("parent", "new", "control"):
            for f in "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz12345":
                runs = [r["forms"][f] for r in rs if r["build"] == which and f in r["forms"]]
                if runs:
                    print("| %s | %s | %s | %.3f .. %.3f |" % (f, which, " / ".join("%.3f" % x["median_ms"] for x in runs),
                                                          min(x["min_ms"] for x in runs), max(x["max_ms"] for x in runs)))
        print("host expansion for A: %s ms" % " / ".join("%.1f" % r["host_expansion_ms"] for r in rs if "host_expansion_ms" in r))
        print("bytes per query: " + json.dumps(bytes_moved(r0["n_conf"], r0["n_objects"], r0["n_pairs"])))
        for key in ("nearest", "nearest_f32"):
            if key in r0:
                k = r0[key]
                print("%s: %d + %d queries evaluated (%.2f %% + %.2f %%), min_distance / min_pair equal to the unculled call: %s%s" % (
                    key, k["evaluated"][0], k["evaluated"][1], k["share_pct"][0], k["share_pct"][1], k["equal_to_unculled"],
                    "; largest (lb - d_f32) / M = %.3g" % k["max_lb_minus_d_over_M"] if "max_lb_minus_d_over_M" in k else ""))
        if "self_pairs" in r0:
            k = r0["self_pairs"]
            print("self pairs at inflate %g: %d pairs listed of %d box tests (%.3f %%)" % (args.inflate, k["n_listed"], k["box_tests"],
                                                                                          100.0 * k["n_listed"] / max(k["box_tests"], 1)))
        gs = [r["groups"] for r in rs if "n_listed" in r.get("groups", {})] or [r["groups"] for r in rs if "groups" in r]
        if gs:
            k = gs[0]
            print("object groups: %d groups; %.1f %% of the column tiles skipped, %.1f %% of the row blocks leave at once; %s listed with groups, %s without, of "
                  "%d box tests; %d allowed pairs in the explicit list; summaries of d equal those of e: %s%s" % (
                      k["n_groups"], k["tiles_skipped_pct"], k["blocks_left_early_pct"], k.get("n_listed", "-"), k.get("n_listed_without_groups", "-"),
                      k["box_tests"], k["allowed_pairs"], k.get("d_equals_e", "-"), "; e refused: " + k["e_refused"] if "e_refused" in k else ""))
        ns = [r["nearest_self"] for r in rs if "nearest_self" in r]
        if ns:
            print("clearance on device-made pairs: " + json.dumps(ns[-1]))
        es = [r["env"] for r in rs if "env" in r]
        if es:
            print("environment: " + json.dumps(es[-1]))
        ne = [r["nearest_env"] for r in rs if "nearest_env" in r]
        if ne:
            print("clearance among the environment: " + json.dumps(ne[-1]))
        if "n_listed" in r0:
            print("cull at inflate %g: %d of %d queries survive (%.2f %%); byte model of the cull alone: %.0f bytes" % (
                r0["inflate"], r0["n_listed"], r0["queries"], 100.0 * r0["n_listed"] / r0["queries"], r0["cull_model_bytes"]))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
