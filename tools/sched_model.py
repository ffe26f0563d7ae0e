#!/usr/bin/env python3
"""Scheduling model of the two big kernels of the fp32 convex x convex path (cfg3), from the oracle's iteration counts.  No GPU needed.

  k_gjk_cvx<2, 0>   a wave steps 32 pairs in lockstep: a round lasts set-up + the trips of its slowest pair (a pair's trips = its GJK
                    iterations + 1).  256-thread form: block b owns the rounds of its four waves (it += groups) and frees its slots when
                    the slowest of the four has ended; single-wave form: every round is a workgroup, placed as slots fall free.
  k_epa_loop        a wave steps 8 polytopes in lockstep and refills when two groups are idle (a refill = 0.25 trip); blocks strided
                    over one round of resident waves, and the last share of them (option epa_pool_share, SHIPPED_SHARE percent by
                    default) drawn by ticket from a pool of 16 counters: csrc/hfcl_epa_pool.hpp is the arithmetic the kernel runs,
                    model_epa the same on the oracle's iteration counts -- keep the two in step.  The model looks at every counter
                    in front of a draw, as the form of round 7 did; the kernel in the tree does not (profiles/r15_a_epa_pool.md: the
                    look cost more than the pool gained), which changes the model's count of atomics at a wave's end, not its trips.

Times are in trips (one lockstep iteration of a wave) and say nothing about waves that share a SIMD speeding up when a partner leaves:
for k_gjk_cvx the device shows less than the model (profiles/r07_a_wave_scheduling.md has both); for k_epa_loop's pool it shows as much
or more, levelling off at 20 % as here (profiles/r15_a_epa_pool.md).  model_gjk's number of resident waves per CU is an argument (8 until
round 20, 12 since); gjk_forecast turns its ends at two residencies into a time, pricing a trip by how many independent waves share a
SIMD's issue slots: 0.531 ms forecast for 0.457 measured (profiles/r21_a_gjk_occupancy.md section 5).

usage: tools/sched_model.py [--pairs 1000000] [--seed 1] [--cus 256] [--threads 16] [--gjk-waves-per-cu 12]"""
import argparse
import heapq
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

EPA_BLOCK_CAP = 17   # EPA_FAST_CAP: a polytope that needs more iterations leaves k_epa_loop (hand-over)
REFILL = 0.25        # trips per refill (reproduces HFCL_EPA_LOOP_REFILL_MIN 1 ~ 2, 3 = +4 %; profiles/r05_a)
REFILL_MIN = 2
SHIPPED_SHARE = 20   # percent: the default of option epa_pool_share (csrc/hfcl_host.hpp)


def oracle_counts(n, seed, threads):
    import __graft_entry__ as ge
    import oracle_binding as ob
    pkg = ge.load_pkg()
    abi, wl = pkg.abi, pkg.workloads
    ob.build()
    b = wl.cfg3_convex_convex(n=n, seed=seed)
    req = wl.make_request(b, abi)
    ref = ob.distance_batch(b.shapes, b.verts, b.s1, b.s2, b.tf1, b.tf2, req, n_threads=threads)
    s = ref["status"]
    pen = abi.status_epa(s) != 15  # HFCL_EPA_DID_NOT_RUN
    return abi.status_gjk_iters(s).astype(np.int64), abi.status_epa_iters(s)[pen].astype(np.int64)


def greedy(durations, slots):
    """Units placed in order on `slots` servers as they fall free: the time the last one ends, and the busy share of the slots."""
    free = [0.0] * min(slots, len(durations))
    heapq.heapify(free)
    end = 0.0
    for d in durations:
        t = heapq.heappop(free) + d
        end = max(end, t)
        heapq.heappush(free, t)
    return end, float(np.sum(durations)) / (slots * end) if end > 0 else 0.0


def model_gjk(iters, cus, setup, waves_per_cu=8):
    """waves_per_cu: resident waves of the kernel per CU (8 = two per SIMD, the form of rounds 2 to 20; 12 = three per SIMD).  The ends are in
    trips of a wave, and a trip lasts longer the more waves share a SIMD's issue slots: compare ends of different residencies through
    gjk_forecast, not directly."""
    trips = iters + 1
    pad = (-len(trips)) % 32
    rounds = np.concatenate([trips, np.zeros(pad, dtype=trips.dtype)]).reshape(-1, 32).max(axis=1) + setup
    wave_slots = cus * waves_per_cu
    # 256-thread blocks, grid = 16 per CU: wave w of block b owns the rounds (4 b + w) + k * (4 * grid)
    grid = min(cus * 16, (len(rounds) + 3) // 4)
    waves = np.zeros(grid * 4)
    idx = np.arange(len(rounds)) % (grid * 4)
    np.add.at(waves, idx, rounds)
    blocks = waves.reshape(grid, 4).max(axis=1)
    end_block, _ = greedy(blocks, wave_slots // 4)
    held = float(blocks.sum() * 4) / wave_slots
    used = float(rounds.sum()) / wave_slots
    end_wave, _ = greedy(rounds, wave_slots)
    return {"trips_per_pair": float(trips.mean()), "round_mean": float(rounds.mean() - setup), "round_sd": float(rounds.std()),
            "rounds_per_wave": len(rounds) / (grid * 4.0), "held": held, "used": used, "end_256": end_block, "end_64": end_wave}


def gjk_forecast(ms_ref, end_ref, end_new, waves_ref, waves_new, issue_ref):
    """k_gjk_cvx<2, 0> at another residency, from a measured time.  A wave issues a VALU instruction in the share issue_ref / waves_ref of its
    SIMD's cycles when waves_ref waves share the SIMD (issue_ref: measured SQ_INSTS_VALU over the issue peak) and waits for the rest; with
    more waves the waits overlap and the issue slots are shared, so the SIMD's issue share rises to at most 1 - (1 - issue_ref / waves_ref) ** waves_new
    (independent waves) and a trip takes waves_new / waves_ref * issue_ref / that as long.  Returns (ms, issue share)."""
    p = issue_ref / waves_ref
    issue_new = 1.0 - (1.0 - p) ** waves_new
    trip = (waves_new / waves_ref) * (issue_ref / issue_new)
    return ms_ref * (end_new / end_ref) * trip, issue_new


def model_epa(lengths, grid, pool_share, k, min_refills, groups=8):
    """Event-driven: every wave at its next refill, in time order.  pool_share = 0: every block strided; > 0: that share drawn by ticket."""
    cnt = len(lengths)
    L = np.minimum(lengths, EPA_BLOCK_CAP)
    S = cnt
    rng_len = 0
    if pool_share > 0 and cnt >= grid * groups * min_refills:
        S = int((cnt - int(cnt * pool_share)) // grid * grid)
        rng_len = (cnt - S + k - 1) // k
    counters = [0] * k
    atomics = 0
    ends = []
    heap = [(0.0, w) for w in range(grid)]
    state = {w: {"next": w, "at": w % k, "dry": set() if rng_len else set(range(k)), "live": []} for w in range(grid)}
    while heap:
        t, w = heapq.heappop(heap)
        st = state[w]
        want = groups - len(st["live"])
        got = []
        if st["next"] < S:
            got = [b for b in range(st["next"], st["next"] + want * grid, grid) if b < S]
            st["next"] += want * grid
        elif len(st["dry"]) < k:
            for j in range(k):
                if counters[j] >= max(0, min(rng_len, cnt - S - j * rng_len)):
                    st["dry"].add(j)
            while len(st["dry"]) < k and not got:
                j = next((st["at"] + s) % k for s in range(k) if (st["at"] + s) % k not in st["dry"])
                ticket = counters[j]
                counters[j] += want
                atomics += 1
                length = max(0, min(rng_len, cnt - S - j * rng_len))
                left = length - ticket
                if left <= want:
                    st["dry"].add(j)
                if left > 0:
                    got = list(range(S + j * rng_len + ticket, S + j * rng_len + ticket + min(want, left)))
                st["at"] = j
        t += REFILL
        st["live"] += [int(L[b]) for b in got]
        more = st["next"] < S or len(st["dry"]) < k
        if not st["live"]:
            if more:
                heapq.heappush(heap, (t, w))
            else:
                ends.append(t - REFILL)
            continue
        # trips until the refill condition holds again
        live = sorted(st["live"])
        if more:
            idle_now = groups - len(live)
            need = max(0, REFILL_MIN - idle_now)  # groups that have to end first
            steps = live[need - 1] if need > 0 else live[0]
            steps = max(steps, 1)
        else:
            steps = live[-1]
        st["live"] = [x - steps for x in live if x - steps > 0]
        if not more and not st["live"]:
            ends.append(t + steps)
            continue
        heapq.heappush(heap, (t + steps, w))
    ends = np.array(ends)
    return {"S": S, "mean_end": float(ends.mean()), "last_end": float(ends.max()), "atomics": atomics}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--cus", type=int, default=256)
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--gjk-waves-per-cu", type=int, default=12, help="resident waves of k_gjk_cvx<2, 0> per CU (registers and LDS: DESIGN.md section 3)")
    ap.add_argument("--gjk-ref-ms", type=float, default=0.596, help="measured k_gjk_cvx<2, 0> time at 8 waves per CU (profiles/r15_a section 5)")
    ap.add_argument("--gjk-ref-issue", type=float, default=0.50, help="its SQ_INSTS_VALU over the issue peak (profiles/traffic_cfg3.json of that build)")
    a = ap.parse_args()
    gjk_iters, epa_len = oracle_counts(a.pairs, a.seed, a.threads)
    print("oracle: %d pairs, %.2f GJK iterations per pair, %d polytopes, %.2f EPA iterations each (%d past the block's %d)" % (
        len(gjk_iters), gjk_iters.mean(), len(epa_len), epa_len.mean(), int((epa_len > EPA_BLOCK_CAP).sum()), EPA_BLOCK_CAP))
    for setup in (2, 3, 4):
        g = model_gjk(gjk_iters, a.cus, setup)
        print("k_gjk_cvx<2,0>  set-up %d trips: round %.1f +- %.1f trips (%.1f per pair), %.2f rounds per wave; 256-thread blocks hold %.0f "
              "wave-trips per slot for %.0f used and end at %.0f; single-wave workgroups end at %.0f (-%.1f %%)" % (
                  setup, g["round_mean"], g["round_sd"], g["trips_per_pair"], g["rounds_per_wave"], g["held"], g["used"], g["end_256"],
                  g["end_64"], 100 * (1 - g["end_64"] / g["end_256"])))
    if a.gjk_waves_per_cu != 8:
        g8, gn = model_gjk(gjk_iters, a.cus, 3, 8), model_gjk(gjk_iters, a.cus, 3, a.gjk_waves_per_cu)
        ms, issue = gjk_forecast(a.gjk_ref_ms, g8["end_64"], gn["end_64"], 2.0, a.gjk_waves_per_cu / 4.0, a.gjk_ref_issue)
        print("k_gjk_cvx<2,0>  %d waves per CU against 8: single-wave workgroups end at %.0f trips against %.0f; issue share %.2f -> %.2f, "
              "a trip %.2f times as long: %.3f ms -> forecast %.3f ms" % (a.gjk_waves_per_cu, gn["end_64"], g8["end_64"], a.gjk_ref_issue, issue,
                                                                        ms / a.gjk_ref_ms * g8["end_64"] / gn["end_64"], a.gjk_ref_ms, ms))
    grid = a.cus * 12
    base = model_epa(epa_len, grid, 0.0, 16, 2)
    print("k_epa_loop  static: waves end at %.0f trips on average, the last at %.0f" % (base["mean_end"], base["last_end"]))
    print("k_epa_loop  the tree draws the last %d %% by ticket (option epa_pool_share)" % SHIPPED_SHARE)
    for share, k in ((0.1, 1), (0.1, 16), (0.1, 32), (SHIPPED_SHARE / 100.0, 16), (0.05, 16)):
        m = model_epa(epa_len, grid, share, k, 2)
        print("k_epa_loop  pool = last %.0f %% (S = %d), %2d counters: mean %.0f, last %.0f (%+.1f %%), %d atomics (%.0f per counter)" % (
            100 * share, m["S"], k, m["mean_end"], m["last_end"], 100 * (m["last_end"] / base["last_end"] - 1), m["atomics"], m["atomics"] / k))


if __name__ == "__main__":
    main()
