#!/usr/bin/env python
"""HeightField<AABB> x solid collide() (hfcl_hfield_collide_batch*) on workloads.hfield_terrain: the device form (resident inputs,
HIP events around the call) and the host form (wall clock, copies included), median and spread of --reps calls after a warm-up, the
kernels of the last chunk of a call, and beside them the same terrain triangulated as a BVHModel<OBBRSS> through
hfcl_collide_batch_device -- the only way a caller has without height fields.  That row answers ANOTHER question: the mesh is the
terrain's top surface, a height field is solid down to min_height (a solid below the surface collides with the field, not with the
mesh), so the two rows are not the same computation and their contact shares differ.

  tools/hfield_bench.py [--n 100000] [--sides 256,1024] [--reps 12] [--no-mesh] [--max-contacts 1]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_pkg  # noqa: E402


def stats(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--sides", default="256,1024")
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--no-mesh", action="store_true")
    ap.add_argument("--max-contacts", type=int, default=1)
    a = ap.parse_args()
    import torch
    pkg = load_pkg()
    abi, wl = pkg.abi, pkg.workloads
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    print("# height field x solid collide(), %d queries, num_max_contacts %d, median [min, max] of %d calls after one warm-up" % (a.n, a.max_contacts, a.reps))
    print("%-12s %-22s %10s %20s %9s %9s   %s" % ("terrain", "call", "ms", "[min, max]", "M q/s", "contacts", "kernels of the last chunk (ms)"))
    for side in [int(s) for s in a.sides.split(",")]:
        w = wl.hfield_terrain(a.n, side, side)
        req = abi.default_collision_request()
        req.num_max_contacts = a.max_contacts
        lib = pkg.Library(w.lib)
        hid = lib.add_hfield(w.x_dim, w.y_dim, w.heights, w.min_height)
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
        d_hf, d_sh = t((w.hfield + hid).view(np.int32)), t(w.shape.view(np.int32))
        d_tfh, d_tfs, d_sw = t(w.tf_hfield), t(w.tf_shape), t(w.swapped)
        d_out = torch.zeros(a.n * 24, dtype=torch.int32, device=dev)
        d_dlb = torch.zeros(a.n, dtype=torch.float64, device=dev)

        def device_call():
            lib.hfield_collide_device(d_hf, d_sh, d_tfh, d_tfs, a.n, req, d_out, d_swapped=d_sw, d_bound=d_dlb, stream=st)

        lib.set_kernel_timing(True)
        device_call()
        torch.cuda.synchronize()
        br = lib.last_kernel_breakdown()
        lib.set_kernel_timing(False)
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
        ks = "  ".join("%s %.3f" % kv for kv in br)
        name = "%dx%d" % (side, side)
        print("%-12s %-22s %10.3f %20s %9.3f %9.3f   %s" % (name, "hfield device", med, "[%.3f, %.3f]" % (lo, hi), a.n / med / 1e3, hit, ks), flush=True)
        ms = []
        lib.hfield_collide(w.hfield + hid, w.shape, w.tf_hfield, w.tf_shape, req, swapped=w.swapped)
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out, _, _, _ = lib.hfield_collide(w.hfield + hid, w.shape, w.tf_hfield, w.tf_shape, req, swapped=w.swapped)
            ms.append(1e3 * (time.perf_counter() - t0))
        assert out.tobytes() == rec.tobytes(), "host and device records differ"
        med, lo, hi = stats(ms)
        print("%-12s %-22s %10.3f %20s %9.3f %9.3f" % (name, "hfield host", med, "[%.3f, %.3f]" % (lo, hi), a.n / med / 1e3, hit), flush=True)
        lib.close()
        if a.no_mesh:
            continue
        # the same terrain as a triangle mesh (its top surface): a different question, see the module docstring
        t0 = time.perf_counter()
        verts, tris = w.triangulation()
        mesh = pkg.bvh_builder.Mesh(verts, tris)
        build_s = time.perf_counter() - t0
        L2 = w.lib.copy()  # the solids under the same ids, plus the mesh
        mid = L2.add_bvh(0, len(verts))
        lib2 = pkg.Library(L2)
        lib2.add_bvh(mesh)
        s_mesh, s_solid = np.full(a.n, mid, dtype=np.uint32), w.shape
        s1, s2 = np.where(w.swapped == 1, s_solid, s_mesh), np.where(w.swapped == 1, s_mesh, s_solid)
        tf1, tf2 = np.where(w.swapped[:, None] == 1, w.tf_shape, w.tf_hfield), np.where(w.swapped[:, None] == 1, w.tf_hfield, w.tf_shape)
        d_s1, d_s2, d_tf1, d_tf2 = t(s1.astype(np.int32)), t(s2.astype(np.int32)), t(tf1), t(tf2)
        lib2.set_kernel_timing(False)
        lib2.collide_device(d_s1, d_s2, d_tf1, d_tf2, a.n, req, d_out, stream=st)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            lib2.collide_device(d_s1, d_s2, d_tf1, d_tf2, a.n, req, d_out, stream=st)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        rec2 = d_out.cpu().numpy().view(abi.RESULT_DTYPE)
        med, lo, hi = stats(ms)
        print("%-12s %-22s %10.3f %20s %9.3f %9.3f   (another question: the surface alone; %d triangles, host build %.1f s)" % (
            name, "mesh device", med, "[%.3f, %.3f]" % (lo, hi), a.n / med / 1e3, float((rec2["num_contacts"] > 0).mean()), len(tris), build_s), flush=True)
        lib2.close()


if __name__ == "__main__":
    main()
