#!/usr/bin/env python
"""OcTree x BVHModel<OBBRSS> collide() (hfcl_octree_mesh_collide_batch*): --n link-sized meshes near the surface of the map of
tools/octree_bench.py (a rolling terrain of 102 400 occupied voxels at depth 16), once with a mesh of a few hundred triangles and once
with one of 5 000, num_max_contacts = 1.  The device form (resident inputs, HIP events around the call) and the host form (wall clock,
copies included), median and spread of --reps calls after a warm-up; the kernels of a call run as one chunk through the pipeline's
timing slots; the listed items per query from the host build of the device header (tests/octree_mesh_harness) on the first --sample
queries, whose records must equal the device's bytes.

Beside it, what a caller without this call must do for the same question: for the first --flat queries, every occupied leaf as an
explicit Box x mesh pair through hfcl_collide_batch_device (inputs made on the device), then a fold per query on the host (any
contact).  The pair count is printed; the flags of the two ways are compared.

  tools/octree_mesh_bench.py [--n 20000] [--side 320] [--resolution 0.05] [--reps 8] [--flat 8] [--sample 500] [--few 64]"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from __graft_entry__ import load_pkg  # noqa: E402
from octree_bench import stats, surface  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20_000)
    ap.add_argument("--side", type=int, default=320)
    ap.add_argument("--resolution", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--flat", type=int, default=8)
    ap.add_argument("--sample", type=int, default=500)
    ap.add_argument("--few", type=int, default=64)
    a = ap.parse_args()
    import torch
    import octree_cases as oc
    import octree_mesh_cases as omc
    pkg = load_pkg()
    abi, geo, engine, bb = pkg.abi, pkg.geometry, pkg.engine, pkg.bvh_builder
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(29)
    res, half = a.resolution, 0.5 * a.side * a.resolution
    g = (np.arange(a.side) + 0.5) * res - half
    X, Y = np.meshgrid(g, g)
    pts = np.stack([X.ravel(), Y.ravel(), surface(X, Y).ravel()], axis=1)
    nodes = engine.octree_from_points(pts, res, 16)
    n_leaves = int((~nodes["child"].any(axis=1)).sum())
    meshes = [bb.Mesh(*bb.bumpy_sphere(12, 12, 0.15)), bb.Mesh(*bb.bumpy_sphere(50, 50, 0.3))]
    L = geo.ShapeLibrary()
    links = [L.add_bvh(k, len(m.vertices)) for k, m in enumerate(meshes)]
    voxel = L.add_box(res, res, res)
    lib = pkg.Library(L)
    for m in meshes:
        lib.add_bvh(m)
    tid = lib.add_octree(nodes, res, 16)
    n = a.n
    xy = rng.uniform(-0.9 * half, 0.9 * half, (n, 2))
    tft = np.repeat(geo.make_pose().reshape(1, 12), n, axis=0)
    ot = np.full(n, tid, dtype=np.uint32)
    req = abi.default_collision_request()
    req.num_max_contacts = 1
    print("# octree x mesh collide(): %d nodes, %d occupied voxels of %g at depth 16; %d queries a mesh, num_max_contacts 1, median [min, max] of "
          "%d calls after one warm-up" % (len(nodes), n_leaves, res, n, a.reps))
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    hh = omc.build_harness(tempfile.mkdtemp())
    for k, m in enumerate(meshes):
        radius = float(np.linalg.norm(m.vertices, axis=1).max())
        T = np.column_stack([xy, surface(xy[:, 0], xy[:, 1]) + rng.uniform(0.6 * radius, 1.6 * radius, n)])
        tfm = geo.make_pose(quat=oc.random_rotations(rng, n), T=T)
        sh = np.full(n, links[k], dtype=np.uint32)
        d_ot, d_sh, d_tft, d_tfm = t(ot.view(np.int32)), t(sh.view(np.int32)), t(tft), t(tfm)
        d_out = torch.zeros(n * 24, dtype=torch.int32, device=dev)
        d_dlb = torch.zeros(n, dtype=torch.float64, device=dev)

        def device_call():
            lib.octree_mesh_collide_device(d_ot, d_sh, d_tft, d_tfm, n, req, d_out, d_bound=d_dlb, stream=st)

        lib.set_option("octree_chunk", n)  # one chunk that is not cut down, so that the breakdown is the whole call's
        lib.set_option("octree_items", 1 << 26)
        lib.set_kernel_timing(True)
        device_call()
        torch.cuda.synchronize()
        br = lib.last_kernel_breakdown()
        lib.set_kernel_timing(False)
        lib.set_option("octree_chunk", 0)
        lib.set_option("octree_items", 0)
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            device_call()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        rec = d_out.cpu().numpy().view(abi.RESULT_DTYPE)
        hit = float((rec["num_contacts"] > 0).mean())
        med, lo, hi = stats(ms)
        # ... and with the item cap out of the way: by default a chunk that lists more than 2^20 items is cut down, and every chunk
        # after a cut counts the walks of all the queries still to come again
        lib.set_option("octree_items", 1 << 26)
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            device_call()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        umed, ulo, uhi = stats(ms)
        # few queries with long walks: the first --few queries alone (a lane each; the call lasts as long as its longest walk, twice)
        few = min(a.few, n)
        lib.set_kernel_timing(True)
        lib.octree_mesh_collide_device(d_ot, d_sh, d_tft, d_tfm, few, req, d_out, d_bound=d_dlb, stream=st)
        torch.cuda.synchronize()
        fbr = lib.last_kernel_breakdown()
        lib.set_kernel_timing(False)
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            lib.octree_mesh_collide_device(d_ot, d_sh, d_tft, d_tfm, few, req, d_out, d_bound=d_dlb, stream=st)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        fmed_, flo, fhi = stats(ms)
        lib.set_option("octree_items", 0)
        oct_med = min(med, umed)
        total = sum(v for _, v in br) or 1.0
        leaf_share = sum(v for name, v in br if "leaf" in name) / total
        print("mesh of %d triangles (%d BVH nodes, radius %.2f)" % (len(m.triangles), len(m.nodes), radius))
        print("%-16s %10s %20s %9s %9s   %s" % ("call", "ms", "[min, max]", "k q/s", "contacts", "kernels of one call as one chunk (ms)"))
        print("%-16s %10.3f %20s %9.3f %9.3f   %s   leaf kernel: %.0f %% of the kernel time" % (
            "device", med, "[%.3f, %.3f]" % (lo, hi), n / med, hit, "  ".join("%s %.3f" % kv for kv in br), 100 * leaf_share), flush=True)
        print("%-16s %10.3f %20s %9.3f %9.3f   octree_items = 2^26: one chunk, not cut" % ("device, uncut", umed, "[%.3f, %.3f]" % (ulo, uhi), n / umed, hit))
        print("%-16s %10.3f %20s %9.3f %9s   the first %d queries alone: %s" % ("device, few", fmed_, "[%.3f, %.3f]" % (flo, fhi), few / fmed_, "", few,
                                                                              "  ".join("%s %.3f" % kv for kv in fbr)), flush=True)
        ms = []
        lib.octree_mesh_collide(ot, sh, tft, tfm, req)
        for _ in range(max(3, a.reps // 2)):
            t0 = time.perf_counter()
            out, _, _, _ = lib.octree_mesh_collide(ot, sh, tft, tfm, req)
            ms.append(1e3 * (time.perf_counter() - t0))
        assert out.tobytes() == rec.tobytes(), "host and device records differ"
        med, lo, hi = stats(ms)
        print("%-16s %10.3f %20s %9.3f %9.3f" % ("host", med, "[%.3f, %.3f]" % (lo, hi), n / med, hit), flush=True)
        # the items a query lists, and the device's bytes against the host build of the header
        s = min(a.sample, n)
        if s:
            want, _, _, _, items = omc.harness_collide(pkg, hh, oc.HarnessTrees(pkg, [(nodes, res, 16)]), omc.HarnessMeshes(pkg, [m]),
                                                       np.zeros(s, dtype=np.uint32), np.zeros(s, dtype=np.uint32), tft[:s], tfm[:s], req,
                                                       items_cap=1 << 24)
            per = np.bincount(items[:, 0], minlength=s)
            same = oc.compare_records(rec[:s], want) == []
            print("items per query (first %d queries, host build of the header): mean %.1f, median %d, max %d; its records equal the device's "
                  "bytes: %s" % (s, per.mean(), int(np.median(per)), int(per.max()), same))
        # every occupied leaf as an explicit Box x mesh pair, for a smaller batch
        f = min(a.flat, n)
        if f:
            boxes = pkg.compat.OcTree(nodes, res, 16).toBoxes()
            nb = len(boxes)
            d_centres = t(boxes[:, :3])
            eye = torch.tensor([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0], dtype=torch.float64, device=dev)
            d_tf1 = torch.cat([eye.repeat(nb, 1), d_centres], dim=1).repeat(f, 1).contiguous()
            d_tf2 = d_tfm[:f].repeat_interleave(nb, dim=0).contiguous()
            d_s1 = torch.full((f * nb,), int(voxel), dtype=torch.int32, device=dev)
            d_s2 = d_sh[:f].repeat_interleave(nb).contiguous()
            d_rec = torch.zeros(f * nb * 24, dtype=torch.int32, device=dev)
            one = abi.default_collision_request()
            lib.collide_device(d_s1, d_s2, d_tf1, d_tf2, f * nb, one, d_rec, stream=st)
            torch.cuda.synchronize()
            ms, fold = [], []
            for _ in range(3):  # (wall clock around call and wait: a large batch runs on several streams of the library)
                t0 = time.perf_counter()
                lib.collide_device(d_s1, d_s2, d_tf1, d_tf2, f * nb, one, d_rec, stream=st)
                torch.cuda.synchronize()
                ms.append(1e3 * (time.perf_counter() - t0))
                t0 = time.perf_counter()
                pr = d_rec.cpu().numpy().view(abi.RESULT_DTYPE).reshape(f, nb)
                flags = (abi.status_contact(pr["status"]) != 0).any(axis=1)
                fold.append(1e3 * (time.perf_counter() - t0))
            med, lo, hi = stats(ms)
            fmed = stats(fold)[0]
            agree = int((flags == (rec["num_contacts"][:f] > 0)).sum())
            print("%-16s %10.3f %20s %9.6f %9.3f   %d queries x %d leaves = %d explicit Box x mesh pairs; copy back and fold on the host %.1f ms "
                  "more; per query %.3f ms against %.5f ms of the octree x mesh call (%.0f x); contact flags agree on %d of %d"
                  % ("flat box pairs", med, "[%.3f, %.3f]" % (lo, hi), f / med, float(flags.mean()), f, nb, f * nb, fmed, (med + fmed) / f,
                     oct_med / n, (med + fmed) / f / (oct_med / n), agree, f), flush=True)
    lib.close()


if __name__ == "__main__":
    main()
