#!/usr/bin/env python
"""Cost of the contact-patch pass against the collide() pass that made its records, on resting contacts (device-resident
buffers, one stream, HIP events around each kernel).  usage: tools/contact_patch_bench.py [--n 1000000] [--steps 10] [--warmup 3]
Scenes: box x box, 32-vertex hulls on a halfspace, cylinder x box, and the mix of every kind (workloads.resting_contacts).
Prints one JSON line per scene: ms per step of the collide pass and of the patch pass (median), and the patch kernels' split."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def scene(pkg, name, n, seed=1):
    wl, abi = pkg.workloads, pkg.abi
    # a resting batch tiled to n pairs (the generator is host Python: ~0.5 ms per pair)
    base = wl.resting_contacts(n=40_000, seed=seed)
    k1, k2 = base.shapes["type"][base.s1], base.shapes["type"][base.s2]
    want = {"box_box": (abi.GEOM_BOX, abi.GEOM_BOX), "cylinder_box": (abi.GEOM_CYLINDER, abi.GEOM_BOX)}.get(name)
    if name == "mix":
        sel = np.ones(len(base), bool)
    elif want:
        sel = ((k1 == want[0]) & (k2 == want[1])) | ((k1 == want[1]) & (k2 == want[0]))
    else:  # hull32_halfspace: 32-vertex hulls against a halfspace
        npts = base.shapes["num_points"]
        sel = (((k1 == abi.GEOM_HALFSPACE) & (k2 == abi.GEOM_CONVEX) & (npts[base.s2] == 32)) |
               ((k2 == abi.GEOM_HALFSPACE) & (k1 == abi.GEOM_CONVEX) & (npts[base.s1] == 32)))
    idx = np.flatnonzero(sel)
    idx = np.resize(idx, n)
    base.s1, base.s2, base.tf1, base.tf2 = base.s1[idx], base.s2[idx], base.tf1[idx], base.tf2[idx]
    return base


def kernel_source_sha():
    """Fingerprint of the device code (bench.py's): the numbers belong to the code they were taken on."""
    h = hashlib.sha256()
    d = os.path.join(ROOT, "hpp-fcl_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".hpp")) or f == "Makefile":
            h.update(f.encode())
            h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scenes", default="box_box,hull32_halfspace,cylinder_box,mix")
    args = ap.parse_args()
    import torch
    pkg = ge.load_pkg()
    abi = pkg.abi
    dev = torch.device("cuda:0")
    sha = kernel_source_sha()
    for name in args.scenes.split(","):
        b = scene(pkg, name, args.n)
        lib = pkg.Library(b.lib, device=0)
        for sid, (off, ids) in b.graphs().items():
            lib.set_convex_neighbors(sid, off, ids)
        n = len(b)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).to(dev)  # noqa: E731
        d_s1, d_s2, d_tf1, d_tf2 = t(b.s1), t(b.s2), t(b.tf1), t(b.tf2)
        d_rec = torch.zeros(n * abi.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_g = torch.zeros(n * abi.GUESS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        preq = abi.default_patch_request()
        cap = lib.contact_patch_max_points(preq)
        d_out = torch.zeros(n * abi.PATCH_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_pts = torch.zeros(n * cap * 2, dtype=torch.float64, device=dev)
        creq = abi.default_collision_request()
        col_ms, pat_ms, split = [], [], {}
        for step in range(args.warmup + args.steps):
            lib.collide_device(d_s1, d_s2, d_tf1, d_tf2, n, creq, d_rec, None, d_g)
            c = sum(ms for _, ms in lib.last_kernel_breakdown())
            lib.contact_patch_device(d_s1, d_s2, d_tf1, d_tf2, d_rec, n, preq, cap, d_out, d_pts, d_guesses=d_g)
            br = lib.last_kernel_breakdown()
            if step >= args.warmup:
                col_ms.append(c)
                pat_ms.append(sum(ms for _, ms in br))
                for k, ms in br:
                    split.setdefault(k, []).append(ms)
        out = d_out.cpu().numpy().view(abi.PATCH_DTYPE)
        cls = out["status"] & 3
        print(json.dumps({"scene": name, "pairs": n, "source_sha": sha, "collide_ms": round(float(np.median(col_ms)), 4),
                          "patch_ms": round(float(np.median(pat_ms)), 4),
                          "patch_kernels_ms": {k: round(float(np.median(v)), 4) for k, v in split.items()},
                          "classes": {c: int((cls == i).sum()) for i, c in enumerate(("none", "point", "onesided", "clipped"))},
                          "mean_points": round(float(out["num_points"][cls >= 2].mean()) if (cls >= 2).any() else 0.0, 3)}),
              flush=True)
        lib.close()


if __name__ == "__main__":
    main()
