#!/usr/bin/env python
"""OcTree x solid collide() (hfcl_octree_collide_batch*): --n solids of the seven kinds near the surface of a map of roughly 10^5
occupied voxels (a rolling terrain sampled at the map's resolution, made by engine.octree_from_points at octomap's depth of 16).  The
device form (resident inputs, HIP events around the call) and the host form (wall clock, copies included), median and spread of
--reps calls after a warm-up; the kernels of a call run as one chunk; the listed items per query from the host build of the device
header (tests/octree_harness) on the first --sample queries, whose records must equal the device's bytes.

Beside it, what a caller without this call must do for the same answers: for the first --flat queries, every occupied leaf as an
explicit Box pair through hfcl_collide_batch_device (inputs made on the device), then a fold per query on the host (any contact, the
smallest distance).  The pair count is printed; the flags of the two ways are compared.

  tools/octree_bench.py [--n 100000] [--side 320] [--resolution 0.05] [--reps 12] [--flat 32] [--sample 2000] [--max-contacts 1]"""
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
    ap.add_argument("--max-contacts", type=int, default=1)
    a = ap.parse_args()
    import torch
    import octree_cases as oc
    pkg = load_pkg()
    abi, geo, engine = pkg.abi, pkg.geometry, pkg.engine
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
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
    lib = pkg.Library(L)
    tid = lib.add_octree(nodes, res, 16)
    n = a.n
    xy = rng.uniform(-0.95 * half, 0.95 * half, (n, 2))
    T = np.column_stack([xy, surface(xy[:, 0], xy[:, 1]) + rng.uniform(-0.05, 0.3, n)])
    tfs = geo.make_pose(quat=oc.random_rotations(rng, n), T=T)
    tft = np.repeat(geo.make_pose().reshape(1, 12), n, axis=0)
    sh = solids[rng.integers(0, len(solids), n)]
    ot = np.full(n, tid, dtype=np.uint32)
    req = abi.default_collision_request()
    req.num_max_contacts = a.max_contacts
    print("# octree x solid collide(): %d points -> %d nodes, %d occupied voxels of %g at depth 16 (host build %.2f s); %d queries, "
          "num_max_contacts %d, median [min, max] of %d calls after one warm-up" % (len(pts), len(nodes), n_leaves, res, build_s, n, a.max_contacts, a.reps))
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    d_ot, d_sh, d_tft, d_tfs = t(ot.view(np.int32)), t(sh.view(np.int32)), t(tft), t(tfs)
    d_out = torch.zeros(n * 24, dtype=torch.int32, device=dev)
    d_dlb = torch.zeros(n, dtype=torch.float64, device=dev)

    def device_call():
        lib.octree_collide_device(d_ot, d_sh, d_tft, d_tfs, n, req, d_out, d_bound=d_dlb, stream=st)

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
    oct_med = med
    print("%-16s %10s %20s %9s %9s   %s" % ("call", "ms", "[min, max]", "M q/s", "contacts", "kernels of one call as one chunk (ms)"))
    print("%-16s %10.3f %20s %9.3f %9.3f   %s" % ("octree device", med, "[%.3f, %.3f]" % (lo, hi), n / med / 1e3, hit,
                                                 "  ".join("%s %.3f" % kv for kv in br)), flush=True)
    ms = []
    lib.octree_collide(ot, sh, tft, tfs, req)
    for _ in range(a.reps):
        t0 = time.perf_counter()
        out, _, _, _ = lib.octree_collide(ot, sh, tft, tfs, req)
        ms.append(1e3 * (time.perf_counter() - t0))
    assert out.tobytes() == rec.tobytes(), "host and device records differ"
    med, lo, hi = stats(ms)
    print("%-16s %10.3f %20s %9.3f %9.3f" % ("octree host", med, "[%.3f, %.3f]" % (lo, hi), n / med / 1e3, hit), flush=True)

    # the items a query lists, and the device's bytes against the host build of the header
    k = min(a.sample, n)
    if k:
        hh = oc.build_harness(tempfile.mkdtemp())
        want, _, _, _, n_items = oc.harness_collide(pkg, hh, oc.HarnessTrees(pkg, [(nodes, res, 16)]), L, np.zeros(k, dtype=np.uint32), sh[:k], tft[:k],
                                                    tfs[:k], req)
        same = oc.compare_records(rec[:k], want) == []
        print("items per query (first %d queries, host build of the header): %.2f; its records equal the device's bytes: %s" % (k, n_items / k, same))

    # every occupied leaf as an explicit Box pair, for a smaller batch
    m = min(a.flat, n)
    if m:
        fcl_tree = pkg.compat.OcTree(nodes, res, 16)
        boxes = fcl_tree.toBoxes()
        nb = len(boxes)
        d_centres = t(boxes[:, :3])
        eye = torch.tensor([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0], dtype=torch.float64, device=dev)
        d_tf1 = torch.cat([eye.repeat(nb, 1), d_centres], dim=1).repeat(m, 1).contiguous()
        d_tf2 = d_tfs[:m].repeat_interleave(nb, dim=0).contiguous()
        d_s1 = torch.full((m * nb,), int(voxel), dtype=torch.int32, device=dev)
        d_s2 = d_sh[:m].repeat_interleave(nb).contiguous()
        d_rec = torch.zeros(m * nb * 24, dtype=torch.int32, device=dev)
        one = abi.default_collision_request()
        lib.collide_device(d_s1, d_s2, d_tf1, d_tf2, m * nb, one, d_rec, stream=st)
        torch.cuda.synchronize()
        ms, fold = [], []
        for _ in range(max(3, a.reps // 4)):  # (wall clock around call and wait: a large batch runs on several streams of the library)
            t0 = time.perf_counter()
            lib.collide_device(d_s1, d_s2, d_tf1, d_tf2, m * nb, one, d_rec, stream=st)
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            pr = d_rec.cpu().numpy().view(abi.RESULT_DTYPE).reshape(m, nb)
            flags = (abi.status_contact(pr["status"]) != 0).any(axis=1)
            nearest = pr["distance"].min(axis=1)
            fold.append(1e3 * (time.perf_counter() - t0))
        med, lo, hi = stats(ms)
        fmed = stats(fold)[0]
        agree = int((flags == (rec["num_contacts"][:m] > 0)).sum())
        print("%-16s %10.3f %20s %9.6f %9.3f   %d queries x %d leaves = %d explicit Box pairs; copy back and fold on the host %.1f ms more; "
              "per query %.3f ms against %.6f ms of the octree call; contact flags agree on %d of %d (smallest distance of query 0: %.6f)"
              % ("flat box pairs", med, "[%.3f, %.3f]" % (lo, hi), m / med / 1e3, float(flags.mean()), m, nb, m * nb, fmed, (med + fmed) / m,
                 oct_med / n, agree, m, float(nearest[0])), flush=True)
    lib.close()


if __name__ == "__main__":
    main()
