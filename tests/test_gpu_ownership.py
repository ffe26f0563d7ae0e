"""A library, a scene gives back every device buffer, pinned buffer, stream and event it took (csrc/hfcl_own.hpp: the owning handles
count themselves per kind; hfcl_debug_live_handles reads the four counts).  Every case runs twice on libraries built from the same
inputs: the counts return to the baseline exactly after close(), each of the four was above it while the objects lived, and the
records of one call per family are the same bytes both times -- results do not depend on the state of the handles."""
import ctypes as C
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _live(pkg):
    out = (C.c_int64 * 4)()
    pkg.engine.dll().hfcl_debug_live_handles(out)
    return tuple(out)  # device buffers, pinned buffers, streams, events


class _Watch:
    """Baseline at construction (after gc.collect()); see() after calls keeps the peak; closed() holds the two claims."""

    def __init__(self, pkg):
        gc.collect()
        self.pkg, self.base = pkg, _live(pkg)
        self.peak = self.base

    def see(self):
        self.peak = tuple(max(a, b) for a, b in zip(self.peak, _live(self.pkg)))

    def closed(self, what):
        gc.collect()
        assert _live(self.pkg) == self.base, (what, "live handles after close()", _live(self.pkg), "baseline", self.base)
        assert all(p > b for p, b in zip(self.peak, self.base)), (what, "some kind of handle was never taken", self.peak, self.base)


def _twice(pkg, what, run):
    """run(watch) -> {family: records}: twice, the ownership claims each time, the records byte for byte between the two"""
    got = []
    for _ in range(2):
        w = _Watch(pkg)
        got.append(run(w))
        w.closed(what)
    assert got[0].keys() == got[1].keys() and len(got[0]) > 0
    for k in got[0]:
        a, b = np.ascontiguousarray(got[0][k]), np.ascontiguousarray(got[1][k])
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (what, k)


def _device_calls(torch, pkg, lib, b, n, w):
    """collide and distance in both precisions on the first n pairs, device-resident, with penetration data; the four record arrays"""
    abi = pkg.abi
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    s1, s2 = t(b.s1[:n].astype(np.int32)), t(b.s2[:n].astype(np.int32))
    tf1, tf2, p1, p2 = t(b.tf1[:n]), t(b.tf2[:n]), t(b.pose1_f32[:n]), t(b.pose2_f32[:n])
    creq, dreq = abi.default_collision_request(), abi.default_distance_request()
    assert creq.enable_contact and dreq.enable_signed_distance
    out = {}
    for name, f32, call in (("collide", False, lambda o: lib.collide_device(s1, s2, tf1, tf2, n, creq, o)),
                            ("distance", False, lambda o: lib.distance_device(s1, s2, tf1, tf2, n, dreq, o)),
                            ("collide_f32", True, lambda o: lib.collide_device_f32(s1, s2, p1, p2, n, creq, o)),
                            ("distance_f32", True, lambda o: lib.distance_device_f32(s1, s2, p1, p2, n, dreq, o))):
        o = torch.zeros(n * (11 if f32 else 24), dtype=torch.int32, device=dev)
        call(o)
        torch.cuda.synchronize()
        w.see()
        out["device_%s_%d" % (name, n)] = o.cpu().numpy().view(abi.RESULT_F32_DTYPE if f32 else abi.RESULT_DTYPE)
    return out


def test_mixed_library_gives_back_every_buffer_family(pkg, torch_cuda):
    """Workspace and EPA buffers (and their grow path), the packed small host path, the pipeline's slots, the contact list, the
    patch workspace, the forced re-size behind option epa_resume_slots."""
    abi, wl = pkg.abi, pkg.workloads
    b = wl.cfg5_mixed(n=20000, seed=7)
    creq, dreq = abi.default_collision_request(), abi.default_distance_request()

    def run(w):
        lib = pkg.Library(b.lib, device=0)
        w.see()
        got = _device_calls(torch_cuda, pkg, lib, b, 2048, w)
        got.update(_device_calls(torch_cuda, pkg, lib, b, 6000, w))  # (past 2048 + 2048 / 8 + 1024: every workspace buffer grows)
        for n in (2048, 20000):  # the packed small path (<= 4096 pairs); five pipeline chunks of 8192
            lib.set_host_chunk(8192)
            s1, s2 = b.s1[:n], b.s2[:n]
            rec, g = lib.collide(s1, s2, b.tf1[:n], b.tf2[:n], creq, want_guess=True)
            got["host_collide_%d" % n] = rec
            rec, g2 = lib.collide(s1, s2, b.tf1[:n], b.tf2[:n], creq, guess_in=g, want_guess=True)
            got["host_collide_guess_%d" % n] = rec
            got["host_distance_%d" % n] = lib.distance(s1, s2, b.tf1[:n], b.tf2[:n], dreq, guess_in=g, want_guess=True)[0]
            got["host_collide_qt_%d" % n] = lib.collide_qt(s1, s2, b.pose1_qt[:n], b.pose2_qt[:n], creq, guess_in=g, want_guess=True)[0]
            got["host_distance_qt_%d" % n] = lib.distance_qt(s1, s2, b.pose1_qt[:n], b.pose2_qt[:n], dreq, guess_in=g, want_guess=True)[0]
            w.see()
        n = 2048
        rec, contacts, produced = lib.collide_contacts(b.s1[:n], b.s2[:n], b.tf1[:n], b.tf2[:n], creq, 4 * n)
        got["contacts_records"] = rec  # (the list itself in a canonical order: its entries are appended by atomics)
        got["contacts"] = np.frombuffer(b"".join(sorted(c.tobytes() for c in contacts)), dtype=np.uint8)
        assert produced == len(contacts)
        rec, g = lib.collide(b.s1[:n], b.s2[:n], b.tf1[:n], b.tf2[:n], creq, want_guess=True)
        patches, pts = lib.contact_patch(b.s1[:n], b.s2[:n], b.tf1[:n], b.tf2[:n], rec, g)
        got["patches"], got["patch_points"] = patches, pts
        w.see()
        for slots in (1, 64, 0):  # the EPA hand-over area is sized again by the next batch
            lib.set_option("epa_resume_slots", slots)
            got["resume_slots_%d" % slots] = lib.collide(b.s1[:6000], b.s2[:6000], b.tf1[:6000], b.tf2[:6000], creq)
            w.see()
        lib.close()
        return got

    _twice(pkg, "mixed library", run)


def test_mesh_library_gives_back_walk_and_split_tables(pkg, torch_cuda):
    """Walk tables, split tables, the mesh streams, the node / vertex images of the models."""
    abi, wl = pkg.abi, pkg.workloads
    b = wl.mesh_vs_shapes(n=2048)

    def run(w):
        lib = wl.make_library(pkg, b, device=0)
        got = {"collide": lib.collide(b.s1, b.s2, b.tf1, b.tf2, abi.default_collision_request())}
        w.see()
        got["distance"] = lib.distance(b.s1, b.s2, b.tf1, b.tf2, abi.default_distance_request())
        w.see()
        lib.close()
        return got

    _twice(pkg, "mesh library", run)


def test_split_batch_helper_and_set_shapes(pkg, torch_cuda):
    """131072 pairs: the smallest batch that runs as two halves -- the helper library, the side stream, the fork / join events;
    hfcl_lib_set_shapes repoints the helper's view of the tables, and the batch after it computes the same records."""
    abi, wl = pkg.abi, pkg.workloads
    b = wl.cfg5_mixed(n=131072, seed=11)
    assert all(int(k) != abi.BV_OBBRSS for k in b.shapes["type"])
    creq = abi.default_collision_request()

    torch = torch_cuda
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d = (t(b.s1.astype(np.int32)), t(b.s2.astype(np.int32)), t(b.tf1), t(b.tf2))

    def batch(lib):
        o = torch.zeros(len(b) * 24, dtype=torch.int32, device=dev)
        lib.collide_device(*d, len(b), creq, o)
        torch.cuda.synchronize()
        assert lib.last_split_parts() == 2
        return o.cpu().numpy().view(abi.RESULT_DTYPE)

    def run(w):
        lib = pkg.Library(b.lib, device=0)
        lib.set_split(2)
        got = {"split": batch(lib)}
        w.see()
        shapes, verts = np.ascontiguousarray(b.shapes), np.ascontiguousarray(b.verts, dtype=np.float64)
        assert pkg.engine.dll().hfcl_lib_set_shapes(lib._h, abi.ptr(shapes), C.c_size_t(len(shapes)), abi.ptr(verts), C.c_size_t(len(verts))) == abi.OK
        got["split_after_set_shapes"] = batch(lib)
        assert got["split_after_set_shapes"].tobytes() == got["split"].tobytes()
        w.see()
        lib.close()
        return got

    _twice(pkg, "split batch", run)


def test_scene_gives_back_its_lists_and_the_scene_workspace(pkg, torch_cuda):
    """8 objects, all 28 pairs: host, device, culled and listed calls in both precisions, one hfcl_scene_set_pairs."""
    torch = torch_cuda
    abi, wl = pkg.abi, pkg.workloads
    ps = wl.scene_planner(16, 8, seed=3)
    i, j = np.triu_indices(8, 1)
    pairs = np.stack([i, j], axis=1).astype(np.uint32)
    assert len(pairs) == 28
    tf, pose = ps.obj_tf, ps.obj_pose_f32
    n_conf, total = len(tf), len(tf) * 28
    creq, dreq = abi.default_collision_request(), abi.default_distance_request()
    dev = torch.device("cuda", 0)

    def run(w):
        lib = pkg.Library(ps.lib, device=0)
        scene = lib.scene(ps.obj_shape, ps.pairs)
        scene.set_pairs(pairs)
        w.see()
        got = {}
        got["collide"], got["collide_summary"], g = scene.collide(tf, creq, want_guess=True)
        got["distance"], got["distance_summary"] = scene.distance(tf, dreq, guess_in=g)
        got["collide_f32"], _ = scene.collide_f32(pose, creq)
        got["distance_f32"], _ = scene.distance_f32(pose, dreq)
        w.see()
        for kind, culled in (("collide", scene.collide_culled), ("distance", scene.distance_culled)):
            for f32, table in ((False, tf), (True, pose)):
                rec, ids, conf_begin, summ = culled(table, 0.05)[:4]
                got["culled_%s_%d" % (kind, f32)], got["culled_ids_%s_%d" % (kind, f32)] = rec, ids
        w.see()
        for f32, table in ((False, tf), (True, pose)):  # device forms: the whole range, then the cull and the calls on its list
            d_tab = torch.from_numpy(np.ascontiguousarray(table)).to(dev)
            words = 11 if f32 else 24
            d_ids = torch.zeros(total, dtype=torch.int64, device=dev)
            d_cb = torch.zeros(n_conf + 1, dtype=torch.int64, device=dev)
            d_n = torch.zeros(1, dtype=torch.int64, device=dev)
            scene.cull_device(d_tab, n_conf, 0.05, d_ids, total, d_cb, d_n, f32=f32)
            torch.cuda.synchronize()
            n_listed = int(d_n.cpu().numpy()[0])
            assert 0 < n_listed <= total
            for kind, req in (("collide", creq), ("distance", dreq)):
                o = torch.zeros(total * words, dtype=torch.int32, device=dev)
                getattr(scene, "%s_device%s" % (kind, "_f32" if f32 else ""))(d_tab, n_conf, req, o)
                ol = torch.zeros(n_listed * words, dtype=torch.int32, device=dev)
                getattr(scene, "%s_listed_device%s" % (kind, "_f32" if f32 else ""))(d_tab, n_conf, d_ids, n_listed, d_cb, req, ol)
                torch.cuda.synchronize()
                got["device_%s_%d" % (kind, f32)], got["listed_%s_%d" % (kind, f32)] = o.cpu().numpy(), ol.cpu().numpy()
            w.see()
        scene.close()
        lib.close()
        return got

    _twice(pkg, "scene", run)


def test_retired_adjacency_images_are_given_back(pkg, torch_cuda):
    """Convex neighbours registered twice between batches: the image the first batch used is retired, not freed, by the second
    registration's upload -- and given back at close()."""
    abi, wl = pkg.abi, pkg.workloads
    b = wl.large_convex(n=2048, kind="distance")
    dreq = abi.default_distance_request()

    def run(w):
        lib = pkg.Library(b.lib, device=0)
        got = {}
        for k in range(3):
            assert wl.register_adjacency(lib, b.shapes, b.verts) == b.n_large
            got["distance_%d" % k] = lib.distance(b.s1, b.s2, b.tf1, b.tf2, dreq)
            w.see()
        assert got["distance_1"].tobytes() == got["distance_0"].tobytes() == got["distance_2"].tobytes()
        lib.close()
        return got

    _twice(pkg, "retired adjacency images", run)
