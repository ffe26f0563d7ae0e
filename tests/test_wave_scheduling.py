"""How work is handed to the waves of the fp32 convex x convex path: k_gjk_cvx<2, 0> runs in workgroups of one wave, one per round of
32 pairs, placed by the dispatcher as waves end; k_epa_loop strides its blocks over one round of resident waves.  That changes no
arithmetic of a pair or a polytope, so every record must be what any other schedule gives -- here: the same pairs submitted in slices
of 1 000."""
import numpy as np
import pytest


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: records against the same pairs in slices of 1 000
# ---------------------------------------------------------------------------------------------------------------------------------
COUNT_KEYS = ("closed", "prim", "cc", "pc", "cp", "unsupported", "large", "epa_queue", "epa_overflow")


class _Dev:
    """A batch's inputs on the device, or the rows `idx` of them."""

    def __init__(self, torch, b, idx=None):
        dev = torch.device("cuda:0")
        pick = (lambda a: a) if idx is None else (lambda a: a[idx])
        self.torch, self.kind = torch, b.kind
        self.n = len(b) if idx is None else len(idx)
        self.s1 = torch.from_numpy(np.ascontiguousarray(pick(b.s1).astype(np.int32))).to(dev)
        self.s2 = torch.from_numpy(np.ascontiguousarray(pick(b.s2).astype(np.int32))).to(dev)
        self.p1 = torch.from_numpy(np.ascontiguousarray(pick(b.pose1_f32))).to(dev)
        self.p2 = torch.from_numpy(np.ascontiguousarray(pick(b.pose2_f32))).to(dev)

    def run(self, lib, req, lo=0, hi=None, out=None):
        """Records of the pairs [lo, hi) as (hi - lo, 11) int32, the bucket counts and the hand-over count of the call."""
        torch = self.torch
        hi = self.n if hi is None else hi
        d_out = torch.zeros((hi - lo) * 11, dtype=torch.int32, device=self.s1.device) if out is None else out[lo * 11:hi * 11]
        fn = lib.distance_device_f32 if self.kind == "distance" else lib.collide_device_f32
        fn(self.s1[lo:hi], self.s2[lo:hi], self.p1[lo:hi], self.p2[lo:hi], hi - lo, req, d_out, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        counts = lib.last_bucket_counts()
        return d_out, {k: counts[k] for k in COUNT_KEYS}, lib.last_epa_handed_over()

    def sliced(self, lib, req, step=1000):
        torch = self.torch
        out = torch.zeros(self.n * 11, dtype=torch.int32, device=self.s1.device)
        sums, over = dict.fromkeys(COUNT_KEYS, 0), 0
        for lo in range(0, self.n, step):  # (1 000 rows of 28 / 44 bytes keep every slice 16-byte aligned)
            _, c, o = self.run(lib, req, lo, min(lo + step, self.n), out=out)
            for k in COUNT_KEYS:
                sums[k] += c[k]
            over += o
        return out.cpu().numpy().reshape(self.n, 11), sums, over


def _same(got, want, what):
    differ = np.flatnonzero((got != want).any(axis=1))
    assert differ.size == 0, "%s: %d records differ, first %s" % (what, differ.size, differ[:10])


@pytest.mark.gpu
@pytest.mark.parametrize("case,n", [("cfg3_convex_convex", 300000), ("cfg5_mixed", 120000)])
def test_records_do_not_depend_on_the_schedule(pkg, torch_cuda, case, n):
    """cfg3 at 300 000 pairs and the mixed fp32 batch of test_fp32_staged_epa_equals_one_kernel_form: the whole batch against the
    one-kernel EPA form, against itself in slices of 1 000 and against a second run; queue lengths and the hand-over count against the
    slices' sums."""
    abi, wl = pkg.abi, pkg.workloads
    b = getattr(wl, case)(n=n, seed=3)
    req = wl.make_request(b, abi)
    d = _Dev(torch_cuda, b)
    lib = pkg.Library(b.lib, options={"epa_cc_staged_min": 0, "epa_cc_staged": "1"})
    d.run(lib, req)  # (cold workspace)
    out1, counts1, over1 = d.run(lib, req)
    names = [k for k, _ in lib.last_kernel_breakdown()]
    assert "k_epa_prepare" in names, names
    rec1 = out1.cpu().numpy().reshape(n, 11).copy()
    out2, counts2, over2 = d.run(lib, req)
    rec2 = out2.cpu().numpy().reshape(n, 11)
    want, sums, over = d.sliced(lib, req)
    lib.close()
    one = pkg.Library(b.lib, options={"epa_cc_staged_min": 0, "epa_cc_staged": "0"})
    out0, counts0, _ = d.run(one, req)
    rec0 = out0.cpu().numpy().reshape(n, 11)
    one.close()
    print("%s: counts %s handed over %d (slices: %d)" % (case, counts1, over1, over))
    _same(rec1, rec2, "two runs")
    _same(rec1, want, "whole batch against slices of 1 000")
    _same(rec1, rec0, "staged against the one-kernel form")
    assert counts1 == counts2 == sums, (counts1, counts2, sums)
    assert counts0["epa_queue"] == counts1["epa_queue"] > 0
    assert over1 == over2 == over, (over1, over2, over)
    if case == "cfg3_convex_convex":
        assert over1 > 0  # (the batch does exercise the hand-over)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 31, 33, 127])
def test_small_batches(pkg, torch_cuda, n):
    abi, wl = pkg.abi, pkg.workloads
    b = wl.cfg3_convex_convex(n=n, seed=5)
    req = wl.make_request(b, abi)
    d = _Dev(torch_cuda, b)
    lib = pkg.Library(b.lib, options={"epa_cc_staged_min": 0, "epa_cc_staged": "1"})
    out, counts, over = d.run(lib, req)
    got = out.cpu().numpy().reshape(n, 11)
    want, sums, over_s = d.sliced(lib, req, step=4)  # (four rows: the smallest slice that stays 16-byte aligned)
    lib.close()
    _same(got, want, "n = %d" % n)
    assert counts == sums and over == over_s


@pytest.mark.gpu
def test_penetrating_pairs_few_none_many(pkg, torch_cuda):
    """Batches composed from cfg3 pairs so that the number of polytopes (cnt) is 0, below the grid of k_epa_loop (one round of resident
    waves: 3 072 on 256 CUs), and several blocks for every wave of it."""
    torch = torch_cuda
    abi, wl = pkg.abi, pkg.workloads
    b = wl.cfg3_convex_convex(n=300000, seed=7)
    req = wl.make_request(b, abi)
    lib = pkg.Library(b.lib, options={"epa_cc_staged_min": 0, "epa_cc_staged": "1"})
    full = _Dev(torch, b)
    want_full, _, _ = full.sliced(lib, req)
    cases = [(0, 40000), (500, 40000), (50000, 20000)]
    pen = abi.status_contact(want_full[:, 10].view(np.uint32)).astype(bool)  # (a pair in contact is a pair GJK hands to EPA)
    rng = np.random.default_rng(1)
    pen_idx, free_idx = np.flatnonzero(pen), np.flatnonzero(~pen)
    for n_pen, n_free in cases:
        idx = np.concatenate([rng.choice(pen_idx, n_pen, replace=False), rng.choice(free_idx, n_free, replace=False)])
        rng.shuffle(idx)
        d = _Dev(torch, b, idx)
        out, counts, over = d.run(lib, req)
        got = out.cpu().numpy().reshape(len(idx), 11)
        print("n_pen %d n_free %d: epa_queue %d handed over %d" % (n_pen, n_free, counts["epa_queue"], over))
        _same(got, want_full[idx], "%d penetrating pairs among %d" % (n_pen, len(idx)))
        out2, counts2, over2 = d.run(lib, req)
        _same(out2.cpu().numpy().reshape(len(idx), 11), got, "second run, %d penetrating pairs" % n_pen)
        assert counts == counts2 and over == over2
        if n_pen == 0:
            assert counts["epa_queue"] == 0
    lib.close()
