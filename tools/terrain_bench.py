#!/usr/bin/env python
"""A height-field terrain under a scene's moving objects (hfcl_scene_collide_terrain*) on workloads.scene_robot_terrain: the device
form (resident table, HIP events around the call) and the host form (wall clock, copies included), each with records + bounds +
summaries and with summaries only, against the SAME queries through hfcl_hfield_collide_batch_device / hfcl_hfield_collide_batch with
the expansion done by the caller (for the host form the caller's numpy expansion is timed separately and NOT included in its row: the
row is the call alone, 200 B per query in and 104 B out).  Median and [min, max] of --reps calls after one warm-up, in one build.

  tools/terrain_bench.py [--sizes 4096x24,16384x24] [--side 256] [--reps 12]"""
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
    ap.add_argument("--sizes", default="4096x24,16384x24", help="n_conf x n_links, comma separated")
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--reps", type=int, default=12)
    a = ap.parse_args()
    import torch
    pkg = load_pkg()
    abi, wl = pkg.abi, pkg.workloads
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    print("# terrain %d x %d, median [min, max] of %d calls after one warm-up" % (a.side, a.side, a.reps))
    print("%-12s %-34s %10s %20s %9s   %s" % ("scene", "call", "ms", "[min, max]", "M q/s", "notes"))

    def timed_device(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return stats(ms)

    def timed_host(fn):
        fn()
        ms = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            ms.append(1e3 * (time.perf_counter() - t0))
        return stats(ms)

    for size in a.sizes.split(","):
        n_conf, n_links = (int(x) for x in size.split("x"))
        w = wl.scene_robot_terrain(n_conf, n_links, a.side)
        n = n_conf * n_links
        req = abi.default_collision_request()
        lib = pkg.Library(w.terrain.lib)
        lib.set_kernel_timing(False)
        hid = lib.add_hfield(w.terrain.x_dim, w.terrain.y_dim, w.terrain.heights, w.terrain.min_height)
        sc = lib.scene(w.object_shape, np.zeros((0, 2), dtype=np.uint32))
        sc.set_terrain(hid, w.tf_terrain)
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
        d_table = t(w.moving_tf)
        d_out = torch.zeros(n * 24, dtype=torch.int32, device=dev)
        d_dlb = torch.zeros(n, dtype=torch.float64, device=dev)
        d_sum = torch.zeros(n_conf * 6, dtype=torch.int32, device=dev)
        t0 = time.perf_counter()
        hf, sh, tfh, tfs = w.explicit()
        expand_ms = 1e3 * (time.perf_counter() - t0)
        hf = hf + np.uint32(hid)
        d_hf, d_sh, d_tfh, d_tfs = t(hf.view(np.int32)), t(sh.view(np.int32)), t(tfh), t(tfs)
        d_out2 = torch.zeros(n * 24, dtype=torch.int32, device=dev)
        d_dlb2 = torch.zeros(n, dtype=torch.float64, device=dev)
        name = "%dx%d" % (n_conf, n_links)

        def row(call, s, notes=""):
            print("%-12s %-34s %10.3f %20s %9.3f   %s" % (name, call, s[0], "[%.3f, %.3f]" % (s[1], s[2]), n / s[0] / 1e3, notes), flush=True)

        s = timed_device(lambda: sc.collide_terrain_device(d_table, n_conf, req, d_out, d_dlb, d_sum, stream=st))
        rec = d_out.cpu().numpy().view(abi.RESULT_DTYPE)
        summ = d_sum.cpu().numpy().view(abi.SCENE_SUMMARY_DTYPE)
        row("terrain device, records+summaries", s, "links touching %.3f, configurations touching %.3f" % (
            float((rec["num_contacts"] > 0).mean()), float((summ["n_contacts"] > 0).mean())))
        row("terrain device, summaries only", timed_device(lambda: sc.collide_terrain_device(d_table, n_conf, req, None, None, d_sum, stream=st)))
        assert d_sum.cpu().numpy().view(abi.SCENE_SUMMARY_DTYPE).tobytes() == summ.tobytes(), "summaries-only call differs"
        row("explicit device (hfield_collide)", timed_device(lambda: lib.hfield_collide_device(d_hf, d_sh, d_tfh, d_tfs, n, req, d_out2, d_bound=d_dlb2, stream=st)))
        assert d_out2.cpu().numpy().view(abi.RESULT_DTYPE).tobytes() == rec.tobytes(), "terrain and explicit records differ"
        row("terrain host, records+summaries", timed_host(lambda: sc.collide_terrain(w.moving_tf, req)))
        row("terrain host, summaries only", timed_host(lambda: sc.collide_terrain(w.moving_tf, req, records=False, bounds=False)))
        row("explicit host (hfield_collide)", timed_host(lambda: lib.hfield_collide(hf, sh, tfh, tfs, req)),
            "+ %.3f ms of numpy expansion by the caller, not included" % expand_ms)
        sc.close()
        lib.close()


if __name__ == "__main__":
    main()
