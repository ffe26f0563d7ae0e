#!/usr/bin/env python
"""OcTree x solid distance() (hfcl_octree_distance_batch*): the scene of tools/octree_bench.py -- --n solids of the seven kinds over a map
of roughly 10^5 occupied voxels (a rolling terrain sampled at the map's resolution, made by engine.octree_from_points at octomap's depth
of 16) -- once near the surface (-0.05 .. 0.3 above it) and once 0.5 .. 2 away.  Per regime: the device form (resident inputs, HIP
events around the call) and the host form (wall clock, copies included), median and spread of --reps calls after a warm-up; mean and
maximum n_visited (the leaves a walk solved); the kernel's time from last_kernel_breakdown() (one extra call as one chunk); the first
--sample device records against the host build of the device header (tests/octree_distance_harness), byte for byte.

Beside it, what a caller without this call must do: for the first --flat queries, every occupied leaf as an explicit Box pair through
hfcl_distance_batch_device (inputs made on the device), then a minimum fold per query on the host.  That fold is the brute-force minimum,
which the ordered walk equals for six kinds and may exceed for an Ellipsoid: the two are compared per query.

  tools/octree_distance_bench.py [--n 100000] [--side 320] [--resolution 0.05] [--reps 12] [--flat 32] [--sample 2000] [--cpu-only K]
--cpu-only K: no device; the visited counts of the first K queries of each regime from the host build of the header."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from __graft_entry__ import load_pkg  # noqa: E402

REGIMES = (("near the surface", -0.05, 0.3), ("0.5 - 2 away", 0.5, 2.0))


def stats(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[0], ms[-1]


def surface(x, y):
    return 0.6 * np.sin(0.7 * x) * np.cos(0.5 * y) + 0.25 * np.sin(2.1 * x + 0.3) + 0.15 * np.cos(1.7 * y)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--side", type=int, default=320)
    ap.add_argument("--resolution", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--flat", type=int, default=32)
    ap.add_argument("--sample", type=int, default=2000)
    ap.add_argument("--cpu-only", type=int, default=0)
    a = ap.parse_args()
    import octree_cases as oc
    import octree_distance_cases as odc
    pkg = load_pkg()
    abi, geo, engine = pkg.abi, pkg.geometry, pkg.engine
    rng = np.random.default_rng(25)
    res, half = a.resolution, 0.5 * a.side * a.resolution
    g = (np.arange(a.side) + 0.5) * res - half
    X, Y = np.meshgrid(g, g)
    pts = np.stack([X.ravel(), Y.ravel(), surface(X, Y).ravel()], axis=1)
    t0 = time.perf_counter()
    nodes = engine.octree_from_points(pts, res, 16)
    build_s = time.perf_counter() - t0
    n_leaves = int((~nodes["child"].any(axis=1)).sum())
    L, solids = oc.seven_solids(pkg, rng)
    voxel = L.add_box(res, res, res)
    n = a.n
    xy = rng.uniform(-0.95 * half, 0.95 * half, (n, 2))
    quat = oc.random_rotations(rng, n)
    sh = solids[rng.integers(0, len(solids), n)]
    lift = rng.uniform(0.0, 1.0, n)
    tft = np.repeat(geo.make_pose().reshape(1, 12), n, axis=0)
    ot = np.zeros(n, dtype=np.uint32)
    req = abi.default_distance_request()
    print("# octree x solid distance(): %d points -> %d nodes, %d occupied voxels of %g at depth 16 (host build %.2f s); %d queries, signed "
          "distance, median [min, max] of %d calls after one warm-up" % (len(pts), len(nodes), n_leaves, res, build_s, n, a.reps))
    hh = odc.build_harness(tempfile.mkdtemp()) if (a.sample or a.cpu_only) else None
    tables = oc.HarnessTrees(pkg, [(nodes, res, 16)])

    def poses(lo, hi):
        T = np.column_stack([xy, surface(xy[:, 0], xy[:, 1]) + lo + (hi - lo) * lift])
        return np.asarray(geo.make_pose(quat=quat, T=T)).reshape(n, 12)

    if a.cpu_only:
        k = min(a.cpu_only, n)
        for name, lo, hi in REGIMES:
            tfs = poses(lo, hi)
            t0 = time.perf_counter()
            _, vis = odc.harness_distance(pkg, hh, tables, L, ot[:k], sh[:k], tft[:k], tfs[:k], req)
            print("%-18s host build of the header, first %d queries: n_visited mean %.1f, median %d, max %d (%.2f s on one core)" %
                  (name, k, vis.mean(), int(np.median(vis)), vis.max(), time.perf_counter() - t0))
        return

    import torch
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    lib = pkg.Library(L)
    tid = lib.add_octree(nodes, res, 16)
    assert tid == 0
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    d_ot, d_sh, d_tft = t(ot.view(np.int32)), t(sh.view(np.int32)), t(tft)
    d_out = torch.zeros(n * 24, dtype=torch.int32, device=dev)
    d_vis = torch.zeros(n, dtype=torch.int32, device=dev)
    print("%-18s %-8s %10s %22s %9s %10s %8s   %s" % ("regime", "call", "ms", "[min, max]", "M q/s", "visited", "max", "kernel of one call as one chunk (ms)"))
    for name, lo, hi in REGIMES:
        tfs = poses(lo, hi)
        d_tfs = t(tfs)

        def device_call():
            lib.octree_distance_device(d_ot, d_sh, d_tft, d_tfs, n, req, d_out, d_visited=d_vis, stream=st)

        lib.set_option("octree_chunk", n)  # one chunk, so that the breakdown is the whole call's
        lib.set_kernel_timing(True)
        device_call()
        torch.cuda.synchronize()
        br = lib.last_kernel_breakdown()
        lib.set_kernel_timing(False)
        lib.set_option("octree_chunk", 0)
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            device_call()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        rec = d_out.cpu().numpy().view(abi.RESULT_DTYPE).copy()
        vis = d_vis.cpu().numpy().view(np.uint32).copy()
        med, mn, mx = stats(ms)
        dev_med = med
        print("%-18s %-8s %10.3f %22s %9.3f %10.1f %8d   %s" % (name, "device", med, "[%.3f, %.3f]" % (mn, mx), n / med / 1e3, vis.mean(), vis.max(),
                                                               "  ".join("%s %.3f" % kv for kv in br)), flush=True)
        ms = []
        lib.octree_distance(ot, sh, tft, tfs, req)
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out = lib.octree_distance(ot, sh, tft, tfs, req)
            ms.append(1e3 * (time.perf_counter() - t0))
        assert out.tobytes() == rec.tobytes(), "host and device records differ"
        med, mn, mx = stats(ms)
        print("%-18s %-8s %10.3f %22s %9.3f" % (name, "host", med, "[%.3f, %.3f]" % (mn, mx), n / med / 1e3), flush=True)
        pct = np.percentile(vis, [50, 90, 99, 99.9])
        print("%-18s n_visited: median %d, 90 %% %d, 99 %% %d, 99.9 %% %d, max %d; separated %.3f; the slowest wave's four walks against the mean "
              "of a wave's longest: %d / %.1f" % (name, pct[0], pct[1], pct[2], pct[3], vis.max(), float((rec["distance"] > 0).mean()), vis.max(),
                                                  vis[:n - n % 4].reshape(-1, 4).max(axis=1).mean()))
        k = min(a.sample, n)
        if k:
            want, want_vis = odc.harness_distance(pkg, hh, tables, L, ot[:k], sh[:k], tft[:k], tfs[:k], req)
            same = oc.compare_records(rec[:k], want) == [] and want_vis.tobytes() == vis[:k].tobytes()
            print("%-18s first %d records and visited counts equal the bytes of the host build of the header: %s" % (name, k, same))
        # every occupied leaf as an explicit Box pair, for a smaller batch
        m = min(a.flat, n)
        if m:
            boxes = pkg.compat.OcTree(nodes, res, 16).toBoxes()
            nb = len(boxes)
            d_centres = t(boxes[:, :3])
            eye = torch.tensor([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0], dtype=torch.float64, device=dev)
            d_tf1 = torch.cat([eye.repeat(nb, 1), d_centres], dim=1).repeat(m, 1).contiguous()
            d_tf2 = d_tfs[:m].repeat_interleave(nb, dim=0).contiguous()
            d_s1 = torch.full((m * nb,), int(voxel), dtype=torch.int32, device=dev)
            d_s2 = d_sh[:m].repeat_interleave(nb).contiguous()
            d_rec = torch.zeros(m * nb * 24, dtype=torch.int32, device=dev)
            lib.distance_device(d_s1, d_s2, d_tf1, d_tf2, m * nb, req, d_rec, stream=st)
            torch.cuda.synchronize()
            ms, fold = [], []
            for _ in range(max(3, a.reps // 4)):  # (wall clock around call and wait: a large batch runs on several streams of the library)
                t0 = time.perf_counter()
                lib.distance_device(d_s1, d_s2, d_tf1, d_tf2, m * nb, req, d_rec, stream=st)
                torch.cuda.synchronize()
                ms.append(1e3 * (time.perf_counter() - t0))
                t0 = time.perf_counter()
                pr = d_rec.cpu().numpy().view(abi.RESULT_DTYPE).reshape(m, nb)
                nearest = pr["distance"].min(axis=1)
                fold.append(1e3 * (time.perf_counter() - t0))
            med, mn, mx = stats(ms)
            fmed = stats(fold)[0]
            sep = nearest > 0
            types = L.shapes_array()["type"][sh[:m]]
            # (the explicit boxes are key * resolution cubes, the walk's are halved down from the root: equal up to rounding, not in bits)
            diff = rec["distance"][:m][sep] - nearest[sep]
            equal = int((np.abs(diff) <= 1e-9).sum())
            above = int((diff > 1e-9).sum())
            below = int((diff < -1e-9).sum())
            worst = float(diff.max()) if len(diff) else 0.0
            print("%-18s %-8s %10.3f %22s %9.6f   %d queries x %d leaves = %d explicit Box pairs; copy back and fold on the host %.1f ms more; per "
                  "query %.3f ms against %.6f ms of the octree call; of %d separated queries the walk equals the brute-force minimum within 1e-9 in "
                  "%d, exceeds it in %d (by up to %.4f) and lies below it in %d (Ellipsoids among the %d: %d)" %
                  (name, "flat", med, "[%.3f, %.3f]" % (mn, mx), m / med / 1e3, m, nb, m * nb, fmed, (med + fmed) / m, dev_med / n, int(sep.sum()), equal,
                   above, worst, below, m, int((types == 19).sum())), flush=True)
            del d_tf1, d_tf2, d_s1, d_s2, d_rec
    lib.close()


if __name__ == "__main__":
    main()
