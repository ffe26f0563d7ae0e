"""k_epa_loop<float, 8, 17>: the trip as a loop of its own, with a shorter instruction chain (profiles/r33_a_epa_loop_trip.md).

Without a GPU: the resources its residency rests on, and the static instruction counts of the unit as the Makefile builds it held
against the counts of the kernel before the trip loop was split off (tools/kernel_insts.py: 841 scalar instructions, 285 register
copies, 66 lane spills of SGPRs, 18 of them inside the trip).  The test pins "below those", and no lane spill inside the trip loop;
what the tree reaches is in the profile.

On the GPU: the records at the batch sizes at which the kernel takes another path -- no polytope at all, one, a wave of eight one
short / full / one over, eight waves' worth one short / full / one over, 500 (with polytopes that outgrow the block), and what 200 000
pairs give (about 60 000).  Pairs of hulls of 4, 5, 16, 17, 31 and 32 vertices (the library of tests/test_gjk_occupancy.py) from one
library, the batches composed by the status of one run as tests/test_epa_pool_gpu.py composes its own.  Every batch: a second run,
its pairs alone in slices of 8 and of 70, the pool at shares 10 / 20 / 50 against share 0 -- records byte for byte, bucket and
hand-over counts equal -- and every record against the fp64 oracle in the envelope of test_fp32_device_path, none excused.  The
natural batch is sliced where a carried-over state would show, not 28 000 times (a batch per slice: ten seconds): its first 1 000
slices of 8 and 200 of 70, and every slice that holds a polytope that was handed over."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from compare import check_parity, check_properties

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "k_epa_loop<float, 8, 17>"
PARENT = {"SALU": 841, "v_mov_b32": 285, "lane_spill": 66}  # tools/kernel_insts.py epa32 k_epa_loop on the kernel before this change

VERTS = [4, 5, 16, 17, 31, 32]
HULLS_PER_COUNT = 11
N_NATURAL = 200000
SEED = 7
COUNTS = [0, 1, 7, 8, 9, 63, 64, 65, 500]  # penetrating pairs (the kernel's cnt): a wave holds 8 polytopes, a round of refills of a wave up to 64
N_FREE = 300                               # separated pairs beside them
SHARES = (10, 20, 50)
COUNT_KEYS = ("closed", "prim", "cc", "pc", "cp", "unsupported", "large", "epa_queue", "epa_overflow")
SMALL = {"epa_cc_staged_min": 0, "epa_pool_min_refills": 0}  # a small batch takes the staged tier, and draws from the pool
NATURAL_FIRST = {8: 1000, 70: 200}


def test_resources():
    """At most 168 VGPRs, no AGPRs, no scratch, 12 544 B of LDS: three waves per SIMD."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "epa32"], capture_output=True, text=True,
                         check=True).stdout
    rows = [tuple(int(x) for x in m.groups()) for m in re.finditer(r"^%s\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s*$" % re.escape(KERNEL), out, re.M)]
    assert len(rows) == 1, out
    vgpr, agpr, scratch, lds, occ = rows[0]
    print(KERNEL, "VGPR", vgpr, "AGPR", agpr, "scratch", scratch, "LDS", lds, "occupancy", occ)
    assert vgpr <= 168 and agpr == 0 and scratch == 0 and lds == 12544 and occ == 3, rows[0]


def test_instruction_counts_below_parent():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_insts.py"), "epa32", "k_epa_loop", "--json"], capture_output=True,
                         text=True, check=True).stdout
    r = json.loads(out)
    assert r["kernel"].startswith("void " + KERNEL), r["kernel"]
    whole, trip = r["whole"], r["trip_loop"]
    print("whole kernel:", {k: whole[k] for k in ("total", "VALU", "SALU", "v_mov_b32", "lane_spill", "mask_b64")})
    print("trip loop   :", {k: trip[k] for k in ("total", "VALU", "SALU", "v_mov_b32", "lane_spill", "mask_b64")})
    for k, parent in PARENT.items():
        assert whole[k] < parent, (k, whole[k], parent)
    # the trip loop is the one loop of the kernel that holds the expansion: by far the largest one without a memory instruction
    assert trip["total"] > 1000 and trip["LDS"] > 100, trip
    assert trip["lane_spill"] == 0, trip


# ---------------------------------------------------------------------------------------------------------------------------------


class _Dev:
    """A batch's inputs on the device, or the rows `idx` of them; run(lo, hi): that slice alone."""

    def __init__(self, torch, b, idx=None):
        dev = torch.device("cuda:0")
        pick = (lambda a: a) if idx is None else (lambda a: a[idx])
        self.torch = torch
        self.n = len(b) if idx is None else len(idx)
        self.s1 = torch.from_numpy(np.ascontiguousarray(pick(b.s1).astype(np.int32))).to(dev)
        self.s2 = torch.from_numpy(np.ascontiguousarray(pick(b.s2).astype(np.int32))).to(dev)
        self.p1 = torch.from_numpy(np.ascontiguousarray(pick(b.pose1_f32))).to(dev)
        self.p2 = torch.from_numpy(np.ascontiguousarray(pick(b.pose2_f32))).to(dev)

    def run(self, lib, req, lo=0, hi=None):
        """Records as (n, 11) int32, the bucket counts and the hand-over count of the call."""
        torch = self.torch
        hi = self.n if hi is None else hi
        d_out = torch.zeros((hi - lo) * 11, dtype=torch.int32, device=self.s1.device)
        lib.distance_device_f32(self.s1[lo:hi].contiguous(), self.s2[lo:hi].contiguous(), self.p1[lo:hi].contiguous(), self.p2[lo:hi].contiguous(),
                                hi - lo, req, d_out, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        counts = lib.last_bucket_counts()
        return d_out.cpu().numpy().reshape(hi - lo, 11), {k: counts[k] for k in COUNT_KEYS}, lib.last_epa_handed_over()


def _same(got, want, what):
    differ = np.flatnonzero((got != want).any(axis=1))
    assert differ.size == 0, "%s: %d records differ, first %s" % (what, differ.size, differ[:10])


def _batch(pkg):
    """N_NATURAL cfg3 pairs over one library of hulls of every vertex count of VERTS."""
    wl = pkg.workloads
    rng = wl._rng(SEED, 3)
    lib = pkg.geometry.ShapeLibrary()
    for v in VERTS:
        base = wl.fibonacci_sphere(v)
        for radii in rng.uniform(0.1, 1.0, (HULLS_PER_COUNT, 3)):
            lib.add_convex(base * radii)
    nlib = len(VERTS) * HULLS_PER_COUNT
    s1, s2 = rng.integers(0, nlib, N_NATURAL), rng.integers(0, nlib, N_NATURAL)
    q1, T1, q2, T2 = wl._poses(rng, N_NATURAL, 1.0)
    return wl.Batch("cfg3_mixed_vertex_counts", lib, s1, s2, q1, T1, q2, T2, "distance", {"gjk_variant": pkg.abi.NesterovAcceleration})


@pytest.fixture(scope="module")
def natural(pkg, oracle, torch_cuda):
    """The 200 000 pairs, their records at share 0 and the oracle's: computed once, left unchanged."""
    abi, wl = pkg.abi, pkg.workloads
    b = _batch(pkg)
    req = wl.make_request(b, abi)
    lib = pkg.Library(b.lib, options={"epa_pool_share": 0})
    d = _Dev(torch_cuda, b)
    d.run(lib, req)
    rec, counts, over = d.run(lib, req)
    assert "k_epa_prepare" in [k for k, _ in lib.last_kernel_breakdown()]
    lib.close()
    rec.setflags(write=False)
    queued = abi.status_epa(rec[:, 10].view(np.uint32)) != abi.EPA_DidNotRun
    assert int(queued.sum()) == counts["epa_queue"], (int(queued.sum()), counts)
    tf1, tf2 = b.tf_from_f32()
    ref = oracle.distance_batch(b.shapes, b.verts, b.s1, b.s2, tf1, tf2, req, n_threads=8)
    ref.setflags(write=False)
    print("natural batch: %d polytopes, %d handed over" % (counts["epa_queue"], over))
    return {"b": b, "req": req, "rec": rec, "counts": counts, "over": over, "queued": queued, "ref": ref}


def _against_oracle(pkg, rec, ref, name):
    abi = pkg.abi
    got = np.ascontiguousarray(rec).view(abi.RESULT_F32_DTYPE).reshape(-1)
    st = check_parity(abi, got, ref, dist_tol=1e-4, point_tol=5e-4, flag_band=1e-4, name=name, fp32=True)  # no record excused
    check_properties(abi, got, tol=2e-4, name=name)
    print(name, "n=%d max_dd=%.3g max_dsep=%.3g" % (len(got), st["max_dd"], st["max_dsep"]))


def _check_batch(pkg, torch, natural, idx, options, what, slices):
    """All the checks of one batch (rows `idx` of the natural one, None: all of it); slices: [(width, lo, hi)] run alone.  Returns share 0's
    records, counts and hand-over count."""
    b, req = natural["b"], natural["req"]
    d = _Dev(torch, b, idx)
    lib = pkg.Library(b.lib, options=dict(options, epa_pool_share=0))
    d.run(lib, req)  # (cold workspace)
    rec0, counts0, over0 = d.run(lib, req)
    rec1, counts1, over1 = d.run(lib, req)
    _same(rec1, rec0, what + ": second run")
    assert counts1 == counts0 and over1 == over0, (what, counts1, counts0, over1, over0)
    if counts0["epa_queue"]:
        assert "k_epa_prepare" in [k for k, _ in lib.last_kernel_breakdown()], "%s: the batch does not take the staged EPA tier" % what
    for share in SHARES:
        lib.set_option("epa_pool_share", share)
        rec, counts, over = d.run(lib, req)
        _same(rec, rec0, "%s: share %d against share 0" % (what, share))
        assert counts == counts0 and over == over0, (what, share, counts, counts0, over, over0)
    lib.set_option("epa_pool_share", 0)
    lib.set_option("epa_cc_staged_min", 0)  # (the slices are small batches: they take the staged tier all the same)
    lib.set_option("epa_pool_min_refills", 0)
    queued_total = over_total = 0
    for w, lo, hi in slices:
        rec, counts, over = d.run(lib, req, lo, hi)
        _same(rec, rec0[lo:hi], "%s: pairs [%d, %d) alone" % (what, lo, hi))
        if w == 8:
            queued_total += counts["epa_queue"]
            over_total += over
    lib.close()
    ref = natural["ref"] if idx is None else natural["ref"][idx]
    _against_oracle(pkg, rec0, ref, what)
    return rec0, counts0, over0, queued_total, over_total


def _all_slices(n):
    return [(w, lo, min(lo + w, n)) for w in (8, 70) for lo in range(0, n, w)]


@pytest.mark.gpu
@pytest.mark.parametrize("n_pen", COUNTS)
def test_composed_batch(pkg, torch_cuda, natural, n_pen):
    pen_idx, free_idx = np.flatnonzero(natural["queued"]), np.flatnonzero(~natural["queued"])
    rng = np.random.default_rng(1)
    idx = np.concatenate([rng.choice(pen_idx, n_pen, replace=False), rng.choice(free_idx, N_FREE, replace=False)])
    rng.shuffle(idx)
    what = "cnt_%d" % n_pen
    rec0, counts0, over0, queued_sl, over_sl = _check_batch(pkg, torch_cuda, natural, idx, SMALL, what, _all_slices(len(idx)))
    print("%s: %d pairs, cnt %d, handed over %d" % (what, len(idx), counts0["epa_queue"], over0))
    assert counts0["epa_queue"] == n_pen, (counts0, n_pen)
    _same(rec0, natural["rec"][idx], what + " against the natural batch's records")
    # the slices of 8 hold the same polytopes, and hand over the same ones
    assert queued_sl == n_pen and over_sl == over0, (queued_sl, over_sl, over0)
    if n_pen == 500:
        assert over0 > 0, "no polytope of the 500 outgrows the block: another seed"


@pytest.mark.gpu
def test_natural_batch(pkg, torch_cuda, natural):
    n = len(natural["b"])
    # a polytope that ran more iterations than the block holds was handed over
    handed = np.flatnonzero(natural["queued"] & (pkg.abi.status_epa_iters(natural["rec"][:, 10].view(np.uint32)) > 17))
    assert handed.size > 0
    slices = []
    for w in (8, 70):
        starts = sorted(set(list(range(0, NATURAL_FIRST[w] * w, w)) + [int(i) // w * w for i in handed]))
        slices += [(w, lo, min(lo + w, n)) for lo in starts]
    rec0, counts0, over0, _, _ = _check_batch(pkg, torch_cuda, natural, None, {}, "natural", slices)
    _same(rec0, natural["rec"], "natural batch: share 0 again")
    assert counts0 == natural["counts"] and over0 == natural["over"]
    assert over0 > 0, "no polytope of the natural batch outgrows the block: another seed"


@pytest.mark.gpu
@pytest.mark.parametrize("max_iterations", [1, 5, 17, 18, 64])
def test_iteration_limits_staged_equals_one_kernel_form(pkg, torch_cuda, natural, max_iterations):
    """step()'s exits: the request's limit before the block's capacity (17), at it and behind it.  The staged form against the one-kernel
    form (k_epa_stream<.., CC>: the same arithmetic in the kernel this change leaves alone), byte for byte, on the 500-polytope batch."""
    b = natural["b"]
    req = pkg.workloads.make_request(b, pkg.abi)
    req.q.epa_max_iterations = max_iterations
    pen_idx, free_idx = np.flatnonzero(natural["queued"]), np.flatnonzero(~natural["queued"])
    rng = np.random.default_rng(1)
    idx = np.concatenate([rng.choice(pen_idx, 500, replace=False), rng.choice(free_idx, N_FREE, replace=False)])
    rng.shuffle(idx)
    d = _Dev(torch_cuda, b, idx)
    recs, counts, overs = {}, {}, {}
    for staged in ("0", "1"):
        lib = pkg.Library(b.lib, options=dict(SMALL, epa_cc_staged=staged))
        d.run(lib, req)
        recs[staged], counts[staged], overs[staged] = d.run(lib, req)
        assert ("k_epa_prepare" in [k for k, _ in lib.last_kernel_breakdown()]) == (staged == "1")
        lib.close()
    print("max_iterations %d: cnt %d, handed over %d (staged)" % (max_iterations, counts["1"]["epa_queue"], overs["1"]))
    assert counts["0"]["epa_queue"] == counts["1"]["epa_queue"] == 500
    _same(recs["1"], recs["0"], "epa_max_iterations %d: staged against one-kernel form" % max_iterations)
    if max_iterations > 17:
        assert overs["1"] > 0
