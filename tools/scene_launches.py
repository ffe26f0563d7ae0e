#!/usr/bin/env python3
"""What the scene entry points launch and compute, for comparing two builds of the library (HFCL_LIB_PATH selects one): every family of
hfcl_scene_* once -- scene (host and device), boxes, cull, listed, culled, nearest (host and device), the self pairs without groups
(host, device, collide_self / distance_self) --, fp64 then fp32, on
workloads.scene_planner(64, 16): 6720 queries, far below the size at which a chunk runs split.  scene_chunk and scene_cull_chunk are set
so that every call runs in three chunks (the listed, culled and nearest forms: a third of their list, read from a call before).

  python tools/scene_launches.py --out DIR [--nearest-env] [--made-lists]
      every output of every call as DIR/<nn>_<name>.npy: records, summaries, boxes, lists, conf_begin, counts, min records, n_evaluated,
      and last_bucket_counts() after every host form.  --nearest-env adds, behind all of these, the clearance among a kept environment
      (hfcl_scene_set_environment* with the first 6 bodies moving, hfcl_scene_nearest_env* host and device, moving rows in three chunks
      and spans of one tile): a run without it is what a build without those calls runs.  --made-lists adds, behind those, the other
      calls on lists made on the device, fp64 then fp32, each in three chunks: under hfcl_scene_set_groups with a matrix that forbids some
      pairs the self pairs and hfcl_scene_nearest_self* (host and device), then hfcl_scene_clear_groups; with the environment set
      hfcl_scene_env_pairs* (host and device), hfcl_scene_{collide,distance}_env_pairs_device* on that list and
      hfcl_scene_{collide,distance}_env*; and hfcl_scene_set_terrain on the smallest field workloads.scene_robot_terrain makes, then
      hfcl_scene_collide_terrain (host and device, with summaries and contacts; fp64: the call has no other form)
  rocprofv3 --kernel-trace --output-format csv -d TRACE -- python tools/scene_launches.py --out DIR [switches]     (one fresh process per build)
  python tools/scene_launches.py --compare DIR_A TRACE_A DIR_B TRACE_B
      the .npy files byte for byte, and the kernel traces: per queue, in dispatch order, (kernel name, grid size, workgroup size)"""
import argparse
import csv
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(out_dir, nearest_env=False, made_lists=False):
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_pkg()
    abi = pkg.abi
    os.makedirs(out_dir, exist_ok=True)
    ps = pkg.workloads.scene_planner(n_conf=64, n_objects=16)
    table = np.ascontiguousarray(ps.obj_tf)
    n_conf, G, P = table.shape[0], table.shape[1], len(ps.pairs)
    total = n_conf * P
    # 7-float poses of the same table: quaternions from the rotation matrices (generic rotations, no w near 0)
    R = pkg.geometry.pose_R(table.reshape(-1, 12))
    w4 = np.sqrt(np.maximum(1.0 + R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2], 1e-12)) * 2.0
    quat = np.stack([0.25 * w4, (R[:, 2, 1] - R[:, 1, 2]) / w4, (R[:, 0, 2] - R[:, 2, 0]) / w4, (R[:, 1, 0] - R[:, 0, 1]) / w4], axis=1)
    pose = np.ascontiguousarray(pkg.geometry.pose_f32_from_quat(quat / np.linalg.norm(quat, axis=1, keepdims=True),
                                                                table.reshape(-1, 12)[:, 9:]).reshape(n_conf, G, 7))
    lib = pkg.Library(ps.lib)
    scene = lib.scene(ps.obj_shape, ps.pairs)
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    creq, dreq = abi.default_collision_request(), abi.default_distance_request()
    seq = [0]

    def dump(name, *arrays, host=False):
        for k, a in enumerate(arrays):
            if a is None:
                continue
            if hasattr(a, "cpu"):
                torch.cuda.synchronize()
                a = a.cpu().numpy()
            np.save(os.path.join(out_dir, "%02d_%s_%d.npy" % (seq[0], name, k)), np.ascontiguousarray(a))
        if host:
            np.save(os.path.join(out_dir, "%02d_%s_buckets.npy" % (seq[0], name)), np.array(list(lib.last_bucket_counts().values()), dtype=np.int64))
        seq[0] += 1

    def d_zeros(n, dtype=torch.int32):
        return torch.zeros(max(int(n), 1), dtype=dtype, device=dev)

    def thirds(work):
        lib.set_option("scene_chunk", max(1, -(-work // 3)))

    lib.set_option("scene_cull_chunk", -(-total // 3))
    for f32 in (False, True):
        p = "f32_" if f32 else "f64_"
        tab = pose if f32 else table
        d_tab = torch.from_numpy(tab).to(dev)
        words = 11 if f32 else 24  # 32-bit words of a record
        sfx = "_f32" if f32 else ""

        thirds(total)
        # scene: host, device
        for kind, req in (("collide", creq), ("distance", dreq)):
            dump(p + kind, *getattr(scene, kind + sfx)(tab, req), host=True)
            d_rec, d_sum = d_zeros(total * words), d_zeros(n_conf * 6)
            getattr(scene, kind + "_device" + sfx)(d_tab, n_conf, req, d_rec, d_sum, stream=st)
            dump(p + kind + "_device", d_rec, d_sum)
        if not f32:  # guesses in and out
            rec, summ, g = scene.collide(tab, creq, want_guess=True)
            dump(p + "collide_guess_out", rec, summ, g, host=True)
            dump(p + "collide_guess_in", *scene.collide(tab, creq, guess_in=g), host=True)
        # boxes
        dump(p + "boxes", scene.world_aabbs(tab))
        d_box = d_zeros(n_conf * G * 6, torch.float64)
        scene.world_aabbs_device(d_tab, n_conf, d_box, f32=f32, stream=st)
        dump(p + "boxes_device", d_box)
        # cull: host, device
        ids, conf_begin = scene.cull(tab, 0.0)
        dump(p + "cull", ids, conf_begin)
        d_ids, d_cb, d_n = d_zeros(total, torch.int64), d_zeros(n_conf + 1, torch.int64), d_zeros(1, torch.int64)
        scene.cull_device(d_tab, n_conf, 0.0, d_ids, total, d_cb, d_n, f32=f32, stream=st)
        dump(p + "cull_device", d_ids, d_cb, d_n)
        n_listed = len(ids)
        thirds(n_listed)
        # listed (device), culled (host)
        for kind, req in (("collide", creq), ("distance", dreq)):
            d_rec, d_sum = d_zeros(n_listed * words), d_zeros(n_conf * 6)
            getattr(scene, kind + "_listed_device" + sfx)(d_tab, n_conf, d_ids, n_listed, d_cb, req, d_rec, d_sum, stream=st)
            dump(p + kind + "_listed_device", d_rec, d_sum)
            dump(p + kind + "_culled", *getattr(scene, kind + "_culled")(tab, 0.0, req, capacity=total), host=True)
        # nearest: host, device
        near = scene.nearest_f32 if f32 else scene.nearest
        _, _, n_eval = near(tab, dreq)
        thirds(max(n_eval))
        summ, rec, n_eval = near(tab, dreq)
        dump(p + "nearest", summ, rec, np.array(n_eval, dtype=np.int64), host=True)
        d_sum, d_min = d_zeros(n_conf * 6), d_zeros(n_conf * words)
        n_eval = (scene.nearest_device_f32 if f32 else scene.nearest_device)(d_tab, n_conf, dreq, d_sum, d_min, stream=st)
        dump(p + "nearest_device", d_sum, d_min, np.array(n_eval, dtype=np.int64))
        # the pairs made on the device, no list and no groups: host, device, and the narrow phase on them (rows in three chunks)
        lib.set_option("scene_cull_chunk", -(-n_conf * G // 3))
        sp, sp_cb = scene.self_pairs(tab, 0.25)
        dump(p + "self_pairs", sp, sp_cb)
        d_sp, d_cb, d_n = d_zeros(2 * len(sp)), d_zeros(n_conf + 1, torch.int64), d_zeros(1, torch.int64)
        scene.self_pairs_device(d_tab, n_conf, 0.25, d_sp, len(sp), d_cb, d_n, f32=f32, stream=st)
        dump(p + "self_pairs_device", d_sp, d_cb, d_n)
        thirds(len(sp))
        for kind, req in (("collide", creq), ("distance", dreq)):
            dump(p + kind + "_self", *getattr(scene, kind + "_self")(tab, req, 0.25), host=True)
        lib.set_option("scene_cull_chunk", -(-total // 3))
    if nearest_env:  # behind every call a build without it has: the clearance among a kept environment
        K = 6
        lib.set_option("scene_cull_chunk", -(-n_conf * K // 3))
        lib.set_option("scene_env_span", 1)
        for f32 in (False, True):
            p = "f32_" if f32 else "f64_"
            tab = pose if f32 else table
            words = 11 if f32 else 24
            moving = np.ascontiguousarray(tab[:, :K])
            scene.set_environment(K, np.ascontiguousarray(tab[0, K:]))
            boxes, tiles = scene.environment_aabbs()
            dump(p + "environment", boxes, tiles)
            _, _, n_eval = scene.nearest_env(moving, dreq)
            thirds(max(max(n_eval), 1))
            clear, rec, n_eval = scene.nearest_env(moving, dreq)
            dump(p + "nearest_env", clear, rec, np.array(n_eval, dtype=np.int64), host=True)
            d_clear, d_min = d_zeros(n_conf * 6), d_zeros(n_conf * words)
            n_eval = (scene.nearest_env_device_f32 if f32 else scene.nearest_env_device)(torch.from_numpy(moving).to(dev), n_conf, dreq, d_clear, d_min, stream=st)
            dump(p + "nearest_env_device", d_clear, d_min, np.array(n_eval, dtype=np.int64))
        scene.clear_environment()
        lib.set_option("scene_env_span", 0)
    if made_lists:
        _made_lists(pkg, lib, scene, table, pose, dump, d_zeros, thirds, dev, st)
    torch.cuda.synchronize()
    scene.close()
    lib.close()
    print("scene_launches: %d calls dumped to %s (%d queries; lists: %d entries)" % (seq[0], out_dir, total, n_listed))


def _made_lists(pkg, lib, scene, table, pose, dump, d_zeros, thirds, dev, st):
    """--made-lists: groups over the self pairs and nearest_self, the env lists and their narrow phases, the terrain"""
    import torch
    abi = pkg.abi
    creq, dreq = abi.default_collision_request(), abi.default_distance_request()
    n_conf, G = table.shape[:2]
    third = lambda n: max(1, -(-n // 3))
    # groups: three, by object index; objects of group 0 never pair with each other, nor group 1 with group 2
    scene.set_groups(np.arange(G) % 3, np.array([[0, 1, 1], [1, 1, 0], [1, 0, 1]], dtype=bool))
    for f32 in (False, True):
        p = "groups_f32_" if f32 else "groups_f64_"
        tab = pose if f32 else table
        d_tab = torch.from_numpy(tab).to(dev)
        words = 11 if f32 else 24
        lib.set_option("scene_cull_chunk", third(n_conf * G))
        sp, sp_cb = scene.self_pairs(tab, 0.25)
        dump(p + "self_pairs", sp, sp_cb)
        d_sp, d_cb, d_n = d_zeros(2 * len(sp)), d_zeros(n_conf + 1, torch.int64), d_zeros(1, torch.int64)
        scene.self_pairs_device(d_tab, n_conf, 0.25, d_sp, len(sp), d_cb, d_n, f32=f32, stream=st)
        dump(p + "self_pairs_device", d_sp, d_cb, d_n)
        _, _, n_eval = scene.nearest_self(tab, dreq)
        thirds(max(max(n_eval), 1))
        clear, rec, n_eval = scene.nearest_self(tab, dreq)
        dump(p + "nearest_self", clear, rec, np.array(n_eval, dtype=np.int64), host=True)
        d_clear, d_min = d_zeros(n_conf * 6), d_zeros(n_conf * words)
        n_eval = (scene.nearest_self_device_f32 if f32 else scene.nearest_self_device)(d_tab, n_conf, dreq, d_clear, d_min, stream=st)
        dump(p + "nearest_self_device", d_clear, d_min, np.array(n_eval, dtype=np.int64))
    scene.clear_groups()
    # the environment: the first K bodies move, the others stand where configuration 0 has them
    K = 6
    lib.set_option("scene_cull_chunk", third(n_conf * K))
    lib.set_option("scene_env_span", 1)
    for f32 in (False, True):
        p = "env_f32_" if f32 else "env_f64_"
        tab = pose if f32 else table
        sfx = "_f32" if f32 else ""
        words = 11 if f32 else 24
        moving = np.ascontiguousarray(tab[:, :K])
        d_moving = torch.from_numpy(moving).to(dev)
        scene.set_environment(K, np.ascontiguousarray(tab[0, K:]))
        ep, ep_cb = scene.env_pairs(moving, 0.25)
        dump(p + "env_pairs", ep, ep_cb)
        d_ep, d_cb, d_n = d_zeros(2 * len(ep)), d_zeros(n_conf + 1, torch.int64), d_zeros(1, torch.int64)
        scene.env_pairs_device(d_moving, n_conf, 0.25, d_ep, len(ep), d_cb, d_n, f32=f32, stream=st)
        dump(p + "env_pairs_device", d_ep, d_cb, d_n)
        thirds(max(len(ep), 1))
        for kind, req in (("collide", creq), ("distance", dreq)):
            d_rec, d_sum = d_zeros(len(ep) * words), d_zeros(n_conf * 6)
            getattr(scene, kind + "_env_pairs_device" + sfx)(d_moving, n_conf, d_ep, len(ep), d_cb, req, d_rec, d_sum, stream=st)
            dump(p + kind + "_env_pairs_device", d_rec, d_sum)
            dump(p + kind + "_env", *getattr(scene, kind + "_env")(moving, req, 0.25), host=True)
    scene.clear_environment()
    lib.set_option("scene_env_span", 0)
    # the terrain: a library and a scene of its own (the workload's solids), every link listed, queries in three chunks
    w = pkg.workloads.scene_robot_terrain(n_conf=16, n_links=6, side=2)
    t = w.terrain
    tlib = pkg.Library(t.lib)
    field = tlib.add_hfield(t.x_dim, t.y_dim, t.heights, t.min_height)
    tscene = tlib.scene(w.object_shape, np.zeros((0, 2), dtype=np.uint32))
    tscene.set_terrain(field, w.tf_terrain)
    n_conf_t, n_links = w.moving_tf.shape[:2]
    n_q = n_conf_t * n_links
    tlib.set_option("hfield_chunk", third(n_q))
    treq = abi.default_collision_request()
    treq.num_max_contacts = 4
    cap = 4 * n_q
    rec, dlb, summ, con, n_con = tscene.collide_terrain(w.moving_tf, treq, max_contacts=cap)
    dump("terrain", rec, dlb, summ, con, np.array([n_con], dtype=np.int64))
    d_rec, d_dlb, d_sum = d_zeros(n_q * 24), d_zeros(n_q, torch.float64), d_zeros(n_conf_t * 6)
    d_con = torch.zeros(cap * abi.CONTACT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    n_con = tscene.collide_terrain_device(torch.from_numpy(w.moving_tf).to(dev), n_conf_t, treq, d_rec, d_dlb, d_sum, d_con, cap, want_count=True, stream=st)
    dump("terrain_device", d_rec, d_dlb, d_sum, d_con[:n_con * abi.CONTACT_DTYPE.itemsize], np.array([n_con], dtype=np.int64))
    torch.cuda.synchronize()
    tscene.close()
    tlib.close()


def _launches(trace_dir):
    """[(kernel name, grid, workgroup), ...] per queue in dispatch order; the queues in the order of their first dispatch."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        sys.exit("%s: %d kernel traces" % (trace_dir, len(files)))
    queues = {}
    with open(files[0]) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Dispatch_Id"]))
    for r in rows:
        q = (r.get("Agent_Id"), r.get("Queue_Id"))
        queues.setdefault(q, []).append((r["Kernel_Name"], tuple(int(r["Grid_Size_" + a]) for a in "XYZ"), tuple(int(r["Workgroup_Size_" + a]) for a in "XYZ")))
    return list(queues.values())


def compare(dir_a, trace_a, dir_b, trace_b):
    names_a, names_b = (sorted(os.path.basename(x) for x in glob.glob(os.path.join(d, "*.npy"))) for d in (dir_a, dir_b))
    bad = 0
    if names_a != names_b or not names_a:
        print("DIFFERENT file lists: %d against %d files" % (len(names_a), len(names_b)))
        bad += 1
    for name in names_a:
        if name in names_b and open(os.path.join(dir_a, name), "rb").read() != open(os.path.join(dir_b, name), "rb").read():
            print("DIFFERENT bytes: " + name)
            bad += 1
    print("outputs: %d files, %s" % (len(names_a), "byte-identical" if not bad else "%d differences" % bad))
    la, lb = _launches(trace_a), _launches(trace_b)
    print("launches: %s against %s per queue" % ([len(q) for q in la], [len(q) for q in lb]))
    if la != lb:
        bad += 1
        for k, (qa, qb) in enumerate(zip(la, lb)):
            for i, (a, b) in enumerate(zip(qa, qb)):
                if a != b:
                    print("queue %d, launch %d: %s against %s" % (k, i, a, b))
                    break
    print("launches: " + ("identical (kernel name, grid size, workgroup size; in order within each queue)" if la == lb else "DIFFERENT"))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--nearest-env", action="store_true", help="add the hfcl_scene_nearest_env* calls behind the others")
    ap.add_argument("--made-lists", action="store_true",
                    help="add, behind the others, the calls under groups, on env lists and on a terrain (see the text above)")
    ap.add_argument("--compare", nargs=4, metavar=("DIR_A", "TRACE_A", "DIR_B", "TRACE_B"))
    a = ap.parse_args()
    if a.compare:
        compare(*a.compare)
    elif a.out:
        run(a.out, a.nearest_env, a.made_lists)
    else:
        ap.error("--out DIR or --compare ...")
