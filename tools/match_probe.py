#!/usr/bin/env python3
"""Gallery match (top-1), wall time per frp_match call and identity of results: persistent running-best kernel vs the per-tile kernel
(FRP_MATCH_V1=1), N = 100k / 1M rows, M = 32 / 320 / 512 queries.
    tools/match_probe.py within [N ...]
the radius match instead: wall ms per call, copies included, of frp_match_within (cap 64, the bound of tolerance 0.6; every query
is a noisy copy of a gallery row, so it has about one hit) against frp_match(topk=64), frp_match_scores and the plain top-1, M = 320,
N = 100k / 1M; under `rocprofv3 --kernel-trace --stats` the same run gives match_top1_kernel against match_top1_within_kernel.
    tools/match_probe.py --groups [N ...]
gallery groups: wall ms per call of the grouped top-1 (frp_match_groups, the mask patterns of tests/groups_cases.py) against the plain
top-1 on the same gallery and queries, M = 320, N = 100k / 1M, in one process, alternating round by round; per size the median of the
rounds, the plain kernel's run-to-run spread (max - min of its rounds over their median) and the ratio grouped / plain."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import frp_amd_loader  # noqa
from frp_amd import native
eng = native.Engine(0)
rng = np.random.default_rng(0)


def within_mode(sizes):
    from frp_amd.face_service import within_min_cos
    M, cap, bound = 320, 64, within_min_cos(0.6)

    def wall(fn, reps):
        fn()
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        return (time.perf_counter() - t) / reps * 1e3

    for N in sizes:
        G = rng.standard_normal((N, 512)).astype(np.float32)
        eng.gallery_set(G)
        q = G[rng.integers(0, N, size=M)] + 0.3 * rng.standard_normal((M, 512)).astype(np.float32)
        del G
        idx, cos, n = eng.match_within(q, bound, cap)
        i1, c1 = eng.match(q)
        ik, ck = eng.match(q, topk=cap)
        cut = ck >= np.float32(bound)
        same = (np.array_equal(idx[:, 0], i1) and np.array_equal(n, cut.sum(1)) and np.array_equal(idx[cut], ik[cut])
                and np.array_equal(cos[cut], ck[cut]))
        t_w = wall(lambda: eng.match_within(q, bound, cap), 20)
        t_1 = wall(lambda: eng.match(q), 20)
        t_k = wall(lambda: eng.match(q, topk=cap), 3)
        t_s = wall(lambda: eng.match_scores(q), 3)
        print(f"N={N:8d} M={M}: match_within {t_w:8.3f} ms | top-1 {t_1:8.3f} ms | match(topk=64) {t_k:9.2f} ms | match_scores {t_s:9.2f} ms"
              f" | hits per query {n.mean():.2f} (max {n.max()}) | lists equal top-k cut at the bound: {same}")


def groups_mode(sizes):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import groups_cases as gc
    M, rounds, reps = 320, 7, 20
    for N in sizes:
        G = rng.standard_normal((N, 512)).astype(np.float32)
        eng.gallery_set(G)
        q = G[rng.integers(0, N, size=M)] + 0.3 * rng.standard_normal((M, 512)).astype(np.float32)
        del G
        eng.gallery_set_groups(gc.row_groups(N))
        qg = gc.query_groups(M)
        ig, cg = eng.match(q, groups=qg)
        i1, c1 = eng.match(q)
        P = (qg & gc.row_groups(N)[np.maximum(ig, 0)]) != 0
        consistent = bool(np.all(P[ig >= 0]) and np.all(cg[ig >= 0] <= c1[ig >= 0]) and np.array_equal(ig[qg == gc.ALL], i1[qg == gc.ALL]))
        t = {"plain": [], "grouped": []}
        for _ in range(rounds):
            for name, fn in (("plain", lambda: eng.match(q)), ("grouped", lambda: eng.match(q, groups=qg))):
                fn()
                t0 = time.perf_counter()
                for _ in range(reps):
                    fn()
                t[name].append((time.perf_counter() - t0) / reps * 1e3)
        mp, mg = float(np.median(t["plain"])), float(np.median(t["grouped"]))
        spread = (max(t["plain"]) - min(t["plain"])) / mp
        print(f"N={N:8d} M={M}: plain top-1 {mp:7.3f} ms | grouped top-1 {mg:7.3f} ms | ratio {mg / mp:6.3f} | plain spread over {rounds} rounds "
              f"{100 * spread:5.1f} % | winners permitted, never above the plain winner's score, equal for ALL queries: {consistent}")


if len(sys.argv) > 1 and sys.argv[1] == "--groups":
    groups_mode([int(a) for a in sys.argv[2:]] or [100_000, 1_000_000])
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "within":
    within_mode([int(a) for a in sys.argv[2:]] or [100_000, 1_000_000])
    sys.exit(0)
for N in (100_000, 1_000_000):
    eng.gallery_set(rng.standard_normal((N, 512)).astype(np.float32))
    for M in (32, 320, 512):
        q = rng.standard_normal((M, 512)).astype(np.float32)
        res = {}
        for v1 in (False, True):
            if v1:
                os.environ["FRP_MATCH_V1"] = "1"
            else:
                os.environ.pop("FRP_MATCH_V1", None)
            idx, cos = eng.match(q)
            t = time.perf_counter()
            for _ in range(20):
                eng.match(q)
            res[v1] = ((time.perf_counter() - t) / 20 * 1e3, idx, cos)       # wall ms per call (incl. query upload / result fetch)
        same = np.array_equal(res[False][1], res[True][1]) and np.array_equal(res[False][2], res[True][2])
        a, b = res[False][0], res[True][0]
        print(f"N={N:8d} M={M:3d}: running-best {a*1e3:7.1f} us per call | per-tile {b*1e3:7.1f} us per call | identical results {same}")
