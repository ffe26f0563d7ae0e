#!/usr/bin/env python
"""OcTree x BVHModel<OBBRSS> distance() (hfcl_octree_mesh_distance_batch*): --n link-sized meshes over the map of tools/octree_bench.py (a
rolling terrain of 102 400 occupied voxels at depth 16), ONE configuration a run -- the mesh (--mesh 288: a few hundred triangles;
--mesh 5000) and where it is (--where near: at the surface, a part of the queries touching; --where away: 0.5 - 2 above it) -- so that a
job can give every configuration a time limit of its own.  A walk solves its pairs one after the other and can be long: start at the
default --n 1000 and raise it only while a call stays well inside its limit.

The device form (resident inputs, HIP events around the call) and the host form (wall clock, copies included), median and spread of
--reps calls after a warm-up; the pairs a walk solved from n_visited; the first --sample queries through the host build of the device
header (tests/octree_mesh_distance_harness), whose records must equal the device's bytes; the first --few queries alone (a group each:
the call lasts as long as its longest walk).

Beside it (--flat F, default 0: not run), what a caller without this call must do for the same question: for the first F queries, every
occupied leaf as an explicit Box x mesh distance() pair through hfcl_distance_batch_device (inputs made on the device), then the minimum
per query on the host.  The distances of the two ways are compared.

  tools/octree_mesh_distance_bench.py [--mesh 288|5000] [--where near|away] [--n 1000] [--side 320] [--resolution 0.05] [--reps 3]
                                      [--sample 16] [--few 8] [--flat 0]"""
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
    ap.add_argument("--mesh", type=int, default=288, choices=(288, 5000))
    ap.add_argument("--where", default="near", choices=("near", "away"))
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--side", type=int, default=320)
    ap.add_argument("--resolution", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sample", type=int, default=16)
    ap.add_argument("--few", type=int, default=8)
    ap.add_argument("--flat", type=int, default=0)
    a = ap.parse_args()
    import torch
    import octree_cases as oc
    import octree_mesh_distance_cases as omdc
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
    m = bb.Mesh(*bb.bumpy_sphere(12, 12, 0.15)) if a.mesh == 288 else bb.Mesh(*bb.bumpy_sphere(50, 50, 0.3))
    L = geo.ShapeLibrary()
    link = L.add_bvh(0, len(m.vertices))
    voxel = L.add_box(res, res, res)
    lib = pkg.Library(L)
    lib.add_bvh(m)
    tid = lib.add_octree(nodes, res, 16)
    n = a.n
    radius = float(np.linalg.norm(m.vertices, axis=1).max())
    xy = rng.uniform(-0.9 * half, 0.9 * half, (n, 2))
    up = rng.uniform(0.6 * radius, 1.6 * radius, n) if a.where == "near" else radius + rng.uniform(0.5, 2.0, n)
    tfm = geo.make_pose(quat=oc.random_rotations(rng, n), T=np.column_stack([xy, surface(xy[:, 0], xy[:, 1]) + up]))
    tft = np.repeat(geo.make_pose().reshape(1, 12), n, axis=0)
    ot, sh = np.full(n, tid, dtype=np.uint32), np.full(n, link, dtype=np.uint32)
    req = abi.default_distance_request()
    print("# octree x mesh distance(): %d nodes, %d occupied voxels of %g at depth 16; mesh of %d triangles (%d BVH nodes, radius %.2f) %s; %d "
          "queries, median [min, max] of %d calls after one warm-up" % (len(nodes), n_leaves, res, len(m.triangles), len(m.nodes), radius,
                                                                         "at the surface" if a.where == "near" else "0.5 - 2 above the surface", n, a.reps))
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    d_ot, d_sh, d_tft, d_tfm = t(ot.view(np.int32)), t(sh.view(np.int32)), t(tft), t(tfm)
    d_out = torch.zeros(n * 24, dtype=torch.int32, device=dev)
    d_vis = torch.zeros(n, dtype=torch.int32, device=dev)

    def timed(count):
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            lib.octree_mesh_distance_device(d_ot, d_sh, d_tft, d_tfm, count, req, d_out, d_visited=d_vis, stream=st)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return stats(ms)

    t0 = time.perf_counter()
    lib.octree_mesh_distance_device(d_ot, d_sh, d_tft, d_tfm, n, req, d_out, d_visited=d_vis, stream=st)
    torch.cuda.synchronize()
    print("warm-up call: %.1f ms" % (1e3 * (time.perf_counter() - t0)), flush=True)
    med, lo, hi = timed(n)
    rec = d_out.cpu().numpy().view(abi.RESULT_DTYPE).copy()
    vis = d_vis.cpu().numpy().view(np.uint32).copy()
    print("%-14s %10s %22s %9s %9s %10s %9s %12s" % ("call", "ms", "[min, max]", "q/s", "touching", "pairs/q", "max", "M solves/s"))
    print("%-14s %10.3f %22s %9.1f %9.3f %10.1f %9d %12.3f" % ("device", med, "[%.3f, %.3f]" % (lo, hi), 1e3 * n / med, float((rec["distance"] <= 0).mean()),
                                                                  vis.mean(), int(vis.max()), vis.sum() / med / 1e3), flush=True)
    few = min(a.few, n)
    if few:
        fmed, flo, fhi = timed(few)
        print("%-14s %10.3f %22s %9.1f %9s %10.1f %9d %12.3f   the first %d queries alone, a group each" % (
            "device, few", fmed, "[%.3f, %.3f]" % (flo, fhi), 1e3 * few / fmed, "", vis[:few].mean(), int(vis[:few].max()), vis[:few].sum() / fmed / 1e3, few),
            flush=True)
    ms = []
    for _ in range(max(2, a.reps)):
        t0 = time.perf_counter()
        out, hvis = lib.octree_mesh_distance(ot, sh, tft, tfm, req, want_visited=True)
        ms.append(1e3 * (time.perf_counter() - t0))
    assert out.tobytes() == rec.tobytes() and hvis.tobytes() == vis.tobytes(), "host and device records differ"
    hmed, hlo, hhi = stats(ms)
    print("%-14s %10.3f %22s %9.1f" % ("host", hmed, "[%.3f, %.3f]" % (hlo, hhi), 1e3 * n / hmed), flush=True)
    s = min(a.sample, n)
    if s:
        hh = omdc.build_harness(tempfile.mkdtemp())
        t0 = time.perf_counter()
        want, want_vis, _ = omdc.harness_distance(pkg, hh, oc.HarnessTrees(pkg, [(nodes, res, 16)]), omdc.HarnessMeshes(pkg, [m]), np.zeros(s, dtype=np.uint32),
                                                  np.zeros(s, dtype=np.uint32), tft[:s], tfm[:s], req)
        print("host build of the header on the first %d queries: %.1f ms a query on one CPU thread; its records and visited counts equal the "
              "device's bytes: %s" % (s, 1e3 * (time.perf_counter() - t0) / s, oc.compare_records(rec[:s], want) == [] and want_vis.tobytes() == vis[:s].tobytes()),
              flush=True)
    f = min(a.flat, n)
    if f:  # every occupied leaf as an explicit Box x mesh distance() pair
        boxes = pkg.compat.OcTree(nodes, res, 16).toBoxes()
        nb = len(boxes)
        eye = torch.tensor([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0], dtype=torch.float64, device=dev)
        d_tf1 = torch.cat([eye.repeat(nb, 1), t(boxes[:, :3])], dim=1).repeat(f, 1).contiguous()
        d_tf2 = d_tfm[:f].repeat_interleave(nb, dim=0).contiguous()
        d_s1 = torch.full((f * nb,), int(voxel), dtype=torch.int32, device=dev)
        d_s2 = d_sh[:f].repeat_interleave(nb).contiguous()
        d_rec = torch.zeros(f * nb * 24, dtype=torch.int32, device=dev)
        lib.distance_device(d_s1, d_s2, d_tf1, d_tf2, f * nb, req, d_rec, stream=st)
        torch.cuda.synchronize()
        ms, fold = [], []
        for _ in range(2):  # (wall clock around call and wait: a large batch runs on several streams of the library)
            t0 = time.perf_counter()
            lib.distance_device(d_s1, d_s2, d_tf1, d_tf2, f * nb, req, d_rec, stream=st)
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            best = d_rec.cpu().numpy().view(abi.RESULT_DTYPE).reshape(f, nb)["distance"].min(axis=1)
            fold.append(1e3 * (time.perf_counter() - t0))
        bmed, blo, bhi = stats(ms)
        fmed = stats(fold)[0]
        sep = rec["distance"][:f] > 0
        worst = float(np.abs(best[sep] - rec["distance"][:f][sep]).max()) if sep.any() else 0.0
        print("%-14s %10.3f %22s   %d queries x %d leaves = %d explicit Box x mesh distance() pairs; copy back and minimum on the host %.1f ms more; "
              "per query %.3f ms against %.3f ms of the octree x mesh call (%.0f x); separated queries %d, largest difference of their distances %.3g; "
              "touching ones agree in sign: %s" % ("flat box pairs", bmed, "[%.3f, %.3f]" % (blo, bhi), f, nb, f * nb, fmed, (bmed + fmed) / f, med / n,
                                                   (bmed + fmed) / f / (med / n), int(sep.sum()), worst, bool(((best <= 0) == ~sep).all())), flush=True)
    lib.close()


if __name__ == "__main__":
    main()
