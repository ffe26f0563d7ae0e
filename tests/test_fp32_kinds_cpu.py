"""fp32 records of EVERY pair kind against the fp64 oracle, on the host build of the device headers (tests/hostsim: the GJK / EPA
core the HIP kernels are made of, the consistency marks of the fp32 runs and the fp64 redo of the marked pairs as
sim_batch_f32 mirrors them).  The judge is tests/fp32_judge.py; tests/test_fp32_kinds_gpu.py runs the same batches on the kernels."""
import numpy as np
import pytest

import fp32_judge

N = 40000
# (workload, keyword arguments, distinct ordered kind pairs the batch must hold)
BATCHES = [
    ("all_primitives", dict(seed=1, kind="collide"), 49),
    ("all_primitives", dict(seed=2, kind="collide"), 49),
    ("all_primitives", dict(seed=1, kind="distance"), 49),
    ("all_primitives", dict(seed=2, kind="distance"), 49),
    ("cfg5_mixed", dict(seed=1), 25),
    ("cfg5_mixed", dict(seed=2), 25),
    ("triangle_pairs", dict(), 15),
    ("flat_pairs", dict(kind="collide"), 32),
    ("flat_pairs", dict(kind="distance"), 32),
    ("cfg1_sphere_sphere", dict(), 1),
    ("large_convex", dict(), None),
]
IDS = ["%s-%s" % (w, "-".join("%s%s" % kv for kv in sorted(kw.items())) or "default") for w, kw, _ in BATCHES]


def make_batch(wl, workload, kw):
    return getattr(wl, workload)(n=N, **kw)


def oracle_records(oracle, b, req, tf1, tf2):
    fn = oracle.distance_batch if b.kind == "distance" else oracle.collide_batch
    return fn(b.shapes, b.verts, b.s1, b.s2, tf1, tf2, req, n_threads=8)


def check_batch_content(pkg, b, ref, workload, n_kind_pairs):
    """The batch holds every ordered kind pair it is meant to, none of them rare, and a fair share of each outcome."""
    abi = pkg.abi
    pairs, rarest = fp32_judge.kind_pairs(b)
    if n_kind_pairs is not None:
        assert pairs == n_kind_pairs, (workload, pairs)
        assert rarest >= 500, (workload, rarest)
    else:  # large_convex: a hull above 32 vertices on at least one side of every pair
        npts = b.shapes["num_points"]
        assert (np.maximum(npts[b.s1], npts[b.s2]) > 32).all()
    contact = abi.status_contact(ref["status"]).mean()
    assert 0.2 <= contact <= 0.7, (workload, contact)


@pytest.mark.parametrize("workload,kw,n_kind_pairs", BATCHES, ids=IDS)
def test_fp32_kinds_against_oracle(pkg, oracle, hostsim, workload, kw, n_kind_pairs):
    abi, wl = pkg.abi, pkg.workloads
    b = make_batch(wl, workload, kw)
    req = wl.make_request(b, abi)
    tf1, tf2 = b.tf_from_f32()
    ref = oracle_records(oracle, b, req, tf1, tf2)
    check_batch_content(pkg, b, ref, workload, n_kind_pairs)
    got = hostsim.batch_f32(abi, b.shapes, b.verts, b.s1, b.s2, b.pose1_f32, b.pose2_f32, req)
    print("%s: %d of %d records marked and solved again in fp64: %s" % (b.name, hostsim.redo_count(), len(b), hostsim.redo_reasons()))
    fp32_judge.judge(pkg, b, req, got, ref, tf1, tf2, name=b.name)


@pytest.mark.parametrize("workload", ["cfg3_convex_convex", "cfg2_box_capsule"])
def test_fp32_marks_spare_the_plain_batches(pkg, hostsim, workload):
    """Pairs of hulls and Box x Capsule pairs run consistently in fp32: none of 200 000 is handed to the fp64 redo."""
    abi, wl = pkg.abi, pkg.workloads
    b = getattr(wl, workload)(n=200000)
    req = wl.make_request(b, abi)
    hostsim.batch_f32(abi, b.shapes, b.verts, b.s1, b.s2, b.pose1_f32, b.pose2_f32, req)
    assert hostsim.redo_count() == 0


def test_fp32_judge_catches_unrepaired_records(pkg, oracle, hostsim):
    """The judge is not vacuous: with the redo switched off the marked records stay as the fp32 run left them, and step a fails."""
    abi, wl = pkg.abi, pkg.workloads
    b = make_batch(wl, "all_primitives", dict(seed=1, kind="distance"))
    req = wl.make_request(b, abi)
    tf1, tf2 = b.tf_from_f32()
    ref = oracle_records(oracle, b, req, tf1, tf2)
    hostsim.set_redo(False)
    try:
        got = hostsim.batch_f32(abi, b.shapes, b.verts, b.s1, b.s2, b.pose1_f32, b.pose2_f32, req)
    finally:
        hostsim.set_redo(True)
    with pytest.raises(AssertionError, match="outside the envelope|decision band|NaN patterns"):
        fp32_judge.judge(pkg, b, req, got, ref, tf1, tf2, name=b.name + "-no-redo")
