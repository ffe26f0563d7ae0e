"""k_epa_loop<float, 8, 17> draws the last share of a batch's polytopes by ticket from a pool (option epa_pool_share; hfcl_epa_pool.hpp).
Which wave steps a polytope changes no arithmetic of it, so the records at shares 10, 20 and 50 must be the bytes of share 0 -- the static
schedule --, with the same bucket counts and hand-over count, run after run.  Batches composed from cfg3 pairs by the status of one
reference run at share 0, as tests/test_wave_scheduling.py composes its own, so that the number of polytopes (cnt) is 0, a few hundred
(most waves find every range dry at once), on either side of the threshold below which a batch keeps the static schedule (two full
refills per wave: 16 x the grid of one round of resident waves), and what 200 000 natural pairs give (the pool engages with the default
options; some fifteen hundred polytopes outgrow the block, so groups that end in a hand-over are refilled from the pool).  Every batch has
at least 32 768 pairs: smaller ones take the one-kernel EPA form and never reach k_epa_loop."""
import numpy as np
import pytest

COUNT_KEYS = ("closed", "prim", "cc", "pc", "cp", "unsupported", "large", "epa_queue", "epa_overflow")
SHARES = (10, 20, 50)
N_NATURAL = 200000
WAVES_PER_CU = 12  # k_epa_loop: three waves per SIMD, one round of resident waves


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

    def run(self, lib, req):
        """Records as (n, 11) int32, the bucket counts and the hand-over count of the call."""
        torch = self.torch
        d_out = torch.zeros(self.n * 11, dtype=torch.int32, device=self.s1.device)
        fn = lib.distance_device_f32 if self.kind == "distance" else lib.collide_device_f32
        fn(self.s1, self.s2, self.p1, self.p2, self.n, req, d_out, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        counts = lib.last_bucket_counts()
        return d_out.cpu().numpy().reshape(self.n, 11), {k: counts[k] for k in COUNT_KEYS}, lib.last_epa_handed_over()


def _same(got, want, what):
    differ = np.flatnonzero((got != want).any(axis=1))
    assert differ.size == 0, "%s: %d records differ, first %s" % (what, differ.size, differ[:10])


def _shares_equal_share0(pkg, d, req, shape_lib, options, what):
    """Share 0, then 10 / 20 / 50, each twice, on one library; returns share 0's records, counts and hand-over count."""
    lib = pkg.Library(shape_lib, options=dict(options, epa_pool_share=0))
    d.run(lib, req)  # (cold workspace)
    rec0, counts0, over0 = d.run(lib, req)
    assert "k_epa_prepare" in [k for k, _ in lib.last_kernel_breakdown()], "%s: the batch does not take the staged EPA tier" % what
    for share in SHARES:
        lib.set_option("epa_pool_share", share)
        rec, counts, over = d.run(lib, req)
        _same(rec, rec0, "%s: share %d against share 0" % (what, share))
        assert counts == counts0 and over == over0, (what, share, counts, counts0, over, over0)
        rec2, counts2, over2 = d.run(lib, req)
        _same(rec2, rec, "%s: share %d, second run" % (what, share))
        assert counts2 == counts0 and over2 == over0, (what, share, counts2, over2)
    lib.close()
    return rec0, counts0, over0


@pytest.fixture(scope="module")
def natural(pkg, torch_cuda):
    """200 000 cfg3 pairs and their records at share 0: the reference run the composed batches are chosen from (left unchanged)."""
    abi, wl = pkg.abi, pkg.workloads
    b = wl.cfg3_convex_convex(n=N_NATURAL, seed=7)
    req = wl.make_request(b, abi)
    lib = pkg.Library(b.lib, options={"epa_pool_share": 0})
    d = _Dev(torch_cuda, b)
    d.run(lib, req)
    rec, counts, over = d.run(lib, req)
    lib.close()
    rec.setflags(write=False)
    # a pair EPA ran on is a polytope of the convex x convex queue: the count k_epa_loop reads
    queued = abi.status_epa(rec[:, 10].view(np.uint32)) != abi.EPA_DidNotRun
    contact = abi.status_contact(rec[:, 10].view(np.uint32)).astype(bool)
    print("reference run: %d pairs EPA ran on, %d in contact, epa_queue %d" % (int(queued.sum()), int(contact.sum()), counts["epa_queue"]))
    assert int(queued.sum()) == counts["epa_queue"], (int(queued.sum()), counts)
    grid = torch_cuda.cuda.get_device_properties(0).multi_processor_count * WAVES_PER_CU
    return {"b": b, "req": req, "rec": rec, "counts": counts, "over": over, "queued": queued, "grid": grid}


@pytest.mark.gpu
def test_pool_engages_with_default_options(pkg, torch_cuda, natural):
    """The natural batch: enough polytopes for the default epa_pool_min_refills, and hand-overs among them."""
    b, req = natural["b"], natural["req"]
    cnt = natural["counts"]["epa_queue"]
    print("natural batch: cnt %d, grid %d, handed over %d" % (cnt, natural["grid"], natural["over"]))
    assert cnt >= 16 * natural["grid"], (cnt, natural["grid"])  # (past the threshold: the pool is on)
    assert natural["over"] > 0
    rec0, counts0, over0 = _shares_equal_share0(pkg, _Dev(torch_cuda, b), req, b.lib, {}, "natural batch")
    _same(rec0, natural["rec"], "natural batch: share 0 again")
    assert counts0 == natural["counts"] and over0 == natural["over"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["cnt_0", "cnt_500_min_refills_0", "below_threshold", "at_threshold"])
def test_composed_batches(pkg, torch_cuda, natural, case):
    b, req, grid = natural["b"], natural["req"], natural["grid"]
    n_pen, n_free, options = {
        "cnt_0": (0, 40000, {}),
        "cnt_500_min_refills_0": (500, 40000, {"epa_pool_min_refills": 0}),
        "below_threshold": (16 * grid - 1, 2000, {}),
        "at_threshold": (16 * grid, 2000, {}),
    }[case]
    pen_idx, free_idx = np.flatnonzero(natural["queued"]), np.flatnonzero(~natural["queued"])
    assert len(pen_idx) >= n_pen and n_pen + n_free >= 32768
    rng = np.random.default_rng(1)
    idx = np.concatenate([rng.choice(pen_idx, n_pen, replace=False), rng.choice(free_idx, n_free, replace=False)])
    rng.shuffle(idx)
    rec0, counts0, over0 = _shares_equal_share0(pkg, _Dev(torch_cuda, b, idx), req, b.lib, options, case)
    print("%s: %d pairs, cnt %d (grid %d), handed over %d" % (case, len(idx), counts0["epa_queue"], grid, over0))
    assert counts0["epa_queue"] == n_pen, (case, counts0, n_pen)
    _same(rec0, natural["rec"][idx], "%s against the natural batch's records" % case)


@pytest.mark.gpu
def test_other_kernels_never_see_the_pool(pkg, torch_cuda):
    """The mixed fp32 batch through collide(): share 20 against share 0."""
    abi, wl = pkg.abi, pkg.workloads
    b = wl.cfg5_mixed(n=120000, seed=3)
    req = wl.make_request(b, abi)
    d = _Dev(torch_cuda, b)
    lib = pkg.Library(b.lib, options={"epa_pool_share": 0})
    d.run(lib, req)
    rec0, counts0, over0 = d.run(lib, req)
    lib.set_option("epa_pool_share", 20)
    rec, counts, over = d.run(lib, req)
    rec2, counts2, over2 = d.run(lib, req)
    lib.close()
    _same(rec, rec0, "cfg5_mixed: share 20 against share 0")
    _same(rec2, rec, "cfg5_mixed: second run")
    assert counts == counts2 == counts0 and over == over2 == over0
    assert counts0["epa_queue"] > 0
