"""fp32 records of EVERY pair kind from the HIP kernels against the fp64 oracle: the batches and the judge of
tests/test_fp32_kinds_cpu.py (tests/fp32_judge.py) through Library.distance_f32 / collide_f32 -- the host forms, which run the same
run_batch as the device forms and every scene form -- plus request variants, byte identity across batch shapes (the same pair must be
marked and solved again in fp64 identically wherever it stands), and the batches that must hand nothing to the fp64 redo."""
import numpy as np
import pytest

import fp32_judge
from test_fp32_kinds_cpu import BATCHES, IDS, check_batch_content, make_batch, oracle_records

pytestmark = pytest.mark.gpu


def run_f32(lib, b, req):
    fn = lib.distance_f32 if b.kind == "distance" else lib.collide_f32
    return fn(b.s1, b.s2, b.pose1_f32, b.pose2_f32, req)


@pytest.mark.parametrize("workload,kw,n_kind_pairs", BATCHES, ids=IDS)
def test_fp32_kinds_against_oracle(pkg, oracle, torch_cuda, workload, kw, n_kind_pairs):
    abi, wl = pkg.abi, pkg.workloads
    b = make_batch(wl, workload, kw)
    req = wl.make_request(b, abi)
    tf1, tf2 = b.tf_from_f32()
    ref = oracle_records(oracle, b, req, tf1, tf2)
    check_batch_content(pkg, b, ref, workload, n_kind_pairs)
    lib = pkg.Library(b.lib)
    got = run_f32(lib, b, req)
    print("%s: buckets %s" % (b.name, lib.last_bucket_counts()))
    fp32_judge.judge(pkg, b, req, got, ref, tf1, tf2, name=b.name + "-gpu")
    lib.close()


def test_fp32_kinds_margin_and_upper_bound(pkg, oracle, torch_cuda):
    """collide() with a security margin and an early stop: marked pairs are solved again under the same request."""
    abi, wl = pkg.abi, pkg.workloads
    b = make_batch(wl, "cfg5_mixed", dict(seed=1))
    req = wl.make_request(b, abi, security_margin=0.05, distance_upper_bound=0.2)
    tf1, tf2 = b.tf_from_f32()
    ref = oracle_records(oracle, b, req, tf1, tf2)
    assert (abi.status_gjk(ref["status"]) == 2).mean() > 0.1  # early stops do occur
    lib = pkg.Library(b.lib)
    got = run_f32(lib, b, req)
    print("%s: buckets %s" % (b.name, lib.last_bucket_counts()))
    fp32_judge.judge(pkg, b, req, got, ref, tf1, tf2, name=b.name + "-margin-gpu")
    lib.close()


def test_fp32_kinds_bounding_volume_guess(pkg, oracle, torch_cuda):
    abi, wl = pkg.abi, pkg.workloads
    b = make_batch(wl, "all_primitives", dict(seed=1, kind="distance"))
    req = wl.make_request(b, abi)
    req.q.gjk_initial_guess = abi.BoundingVolumeGuess
    tf1, tf2 = b.tf_from_f32()
    ref = oracle_records(oracle, b, req, tf1, tf2)
    lib = pkg.Library(b.lib)
    got = run_f32(lib, b, req)
    print("%s: buckets %s" % (b.name, lib.last_bucket_counts()))
    fp32_judge.judge(pkg, b, req, got, ref, tf1, tf2, name=b.name + "-bvg-gpu")
    lib.close()


def test_fp32_record_independent_of_batch_shape(pkg, torch_cuda):
    """A 2 049-pair all_primitives batch against its pairs 0..69 run alone, its slices of 32, and a second run: byte for byte.  The
    batch holds marked pairs, so this also pins that marking and the fp64 redo do not depend on a pair's partners or its slot."""
    abi, wl = pkg.abi, pkg.workloads
    b = wl.all_primitives(n=2049, seed=1, kind="distance")
    req = wl.make_request(b, abi)
    lib = pkg.Library(b.lib)
    whole = run_f32(lib, b, req)
    assert lib.last_bucket_counts()["redo"] > 0
    again = run_f32(lib, b, req)
    assert whole.tobytes() == again.tobytes()
    for k in range(70):
        one = run_f32(lib, b.slice(k, k + 1), req)
        assert one.tobytes() == whole[k:k + 1].tobytes(), k
    for lo in range(0, 2049, 32):
        part = run_f32(lib, b.slice(lo, min(lo + 32, 2049)), req)
        assert part.tobytes() == whole[lo:lo + 32].tobytes(), lo
    lib.close()


@pytest.mark.parametrize("workload", ["cfg3_convex_convex", "cfg2_box_capsule"])
def test_fp32_plain_batches_hand_nothing_to_the_redo(pkg, torch_cuda, workload):
    abi, wl = pkg.abi, pkg.workloads
    b = getattr(wl, workload)(n=200000)
    req = wl.make_request(b, abi)
    lib = pkg.Library(b.lib)
    run_f32(lib, b, req)
    counts = lib.last_bucket_counts()
    assert counts["redo"] == 0, counts
    lib.close()
