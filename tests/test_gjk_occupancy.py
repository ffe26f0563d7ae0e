"""k_gjk_cvx<2, 0, *>, the fp32 convex x convex GJK kernel of 2-lane groups: the resources that decide how many of its single-wave
workgroups are resident (three per SIMD by registers, twelve per CU by LDS), and its records at the smallest shapes at which it can go
wrong -- hulls that fill one lane of a pair, both, or neither exactly; batches of a lone pair, a wave one short of full, full, one
over, three workgroups, and 65 workgroups with the last one nearly empty."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from compare import check_parity, check_properties

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VERTS = [4, 5, 16, 17, 31, 32]  # <= 16: the second lane of a pair holds padding only (copies of vertex 0)
SIZES = [1, 31, 32, 33, 65, 2049]
SEED = 21
LONE_SEEDS = (21, 22)  # a batch of one pair holds one class only: at every vertex count the first is separated, the second penetrates
HALF_WIDTH = 0.6  # hulls of radii U[0.1, 1] with centres in [-0.6, 0.6]^3: about half of the pairs penetrate


def test_resource_pin():
    """The figures the residency of k_gjk_cvx<2, 0, *> rests on, from the compiler's own report of the unit as the Makefile builds it:
    at most 168 VGPRs with no AGPRs and no scratch (three waves per SIMD) and at most 12 800 B of LDS, ten allocation units of 1 280 B
    (twelve single-wave workgroups per CU).  A later compiler whose allocator takes more fails here instead of halving the occupancy."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "gjk32"], capture_output=True, text=True,
                         check=True).stdout
    rows = {}
    for line in out.splitlines():
        m = re.match(r"(k_gjk_cvx<2, 0, (?:true|false)>)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s*$", line)
        if m:
            rows[m.group(1)] = tuple(int(x) for x in m.groups()[1:])
    assert sorted(rows) == ["k_gjk_cvx<2, 0, false>", "k_gjk_cvx<2, 0, true>"], out
    for name, (vgpr, agpr, scratch, lds, occ) in rows.items():
        print(name, "VGPR", vgpr, "AGPR", agpr, "scratch", scratch, "LDS", lds, "occupancy", occ)
        assert vgpr <= 168 and agpr == 0 and scratch == 0, (name, vgpr, agpr, scratch)
        assert lds <= 12800, (name, lds)
        assert occ == 3, (name, occ)


def _batch(pkg, n, v, seed=SEED):
    return pkg.workloads.cfg3_convex_convex(n, seed, nlib=64, half_width=HALF_WIDTH, nverts=v)


def _request(pkg, b, bvg):
    req = pkg.workloads.make_request(b, pkg.abi)
    if bvg:
        req.q.gjk_initial_guess = pkg.abi.BoundingVolumeGuess
    return req


class _Device:
    """One batch on the device: the whole of it or a slice [lo, hi) through the fp32 device-resident entry point."""

    def __init__(self, pkg, torch, b, req):
        self.pkg, self.torch, self.n, self.req = pkg, torch, len(b), req
        dev = torch.device("cuda:0")
        self.lib = pkg.Library(b.lib)
        self.s1 = torch.from_numpy(b.s1.astype(np.int32)).to(dev)
        self.s2 = torch.from_numpy(b.s2.astype(np.int32)).to(dev)
        self.p1 = torch.from_numpy(b.pose1_f32).to(dev)
        self.p2 = torch.from_numpy(b.pose2_f32).to(dev)

    def run(self, lo=0, hi=None):
        torch = self.torch
        hi = self.n if hi is None else hi
        out = torch.zeros((hi - lo) * 11, dtype=torch.int32, device=self.s1.device)
        self.lib.distance_device_f32(self.s1[lo:hi].contiguous(), self.s2[lo:hi].contiguous(), self.p1[lo:hi].contiguous(),
                                     self.p2[lo:hi].contiguous(), hi - lo, self.req, out, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return out.cpu().numpy().reshape(hi - lo, 11)

    def close(self):
        self.lib.close()


def _against_oracle(pkg, oracle, torch, b, req, name):
    abi = pkg.abi
    tf1, tf2 = b.tf_from_f32()
    ref = oracle.distance_batch(b.shapes, b.verts, b.s1, b.s2, tf1, tf2, req, n_threads=8)
    d = _Device(pkg, torch, b, req)
    try:
        got = d.run().view(abi.RESULT_F32_DTYPE).reshape(-1)
    finally:
        d.close()
    st = check_parity(abi, got, ref, dist_tol=1e-4, point_tol=5e-4, flag_band=1e-4, name=name, fp32=True)  # no record excused
    check_properties(abi, got, tol=2e-4, name=name)
    print(name, "n=%d max_dd=%.3g max_dsep=%.3g contacts=%d" % (len(b), st["max_dd"], st["max_dsep"], int(abi.status_contact(ref["status"]).sum())))
    return abi.status_contact(ref["status"]).astype(bool)


@pytest.mark.gpu
@pytest.mark.parametrize("bvg", [False, True], ids=["default_guess", "bv_guess"])
@pytest.mark.parametrize("v", VERTS)
def test_records_against_oracle(pkg, oracle, torch_cuda, v, bvg):
    """Every record of every batch size against the fp64 oracle fed with the fp32-rounded poses, in the envelope of
    test_fp32_device_path (test_gpu_parity.py) with no excused record; bvg: the k_gjk_cvx<2, 0, true> instantiation."""
    for n in SIZES:
        if n == 1:
            both = []
            for seed in LONE_SEEDS:
                b = _batch(pkg, 1, v, seed)
                both.append(_against_oracle(pkg, oracle, torch_cuda, b, _request(pkg, b, bvg), "v%d-n1-seed%d" % (v, seed))[0])
            assert both == [False, True], both  # a separated lone pair, then a penetrating one
        else:
            b = _batch(pkg, n, v)
            contact = _against_oracle(pkg, oracle, torch_cuda, b, _request(pkg, b, bvg), "v%d-n%d" % (v, n))
            assert contact.any() and not contact.all(), "v=%d n=%d: one class only (%d contacts)" % (v, n, contact.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("bvg", [False, True], ids=["default_guess", "bv_guess"])
@pytest.mark.parametrize("v", VERTS)
def test_record_independent_of_partners(pkg, torch_cuda, v, bvg):
    """A pair's record depends neither on the pairs it runs in lockstep with nor on where the simplex payload is stored: the 2 049-pair
    batch equals, byte for byte, a second run of itself, its first 70 pairs each as a batch of one, and its slices of 32 pairs."""
    b = _batch(pkg, 2049, v)
    d = _Device(pkg, torch_cuda, b, _request(pkg, b, bvg))
    try:
        whole = d.run()
        assert np.array_equal(d.run(), whole), "a second run differs"
        for k in range(70):
            assert np.array_equal(d.run(k, k + 1), whole[k:k + 1]), "pair %d alone differs from its record in the batch" % k
        for lo in range(0, 2049, 32):
            hi = min(lo + 32, 2049)
            differ = np.flatnonzero((d.run(lo, hi) != whole[lo:hi]).any(axis=1))
            assert differ.size == 0, "slice [%d, %d): records %s differ" % (lo, hi, lo + differ[:10])
    finally:
        d.close()
