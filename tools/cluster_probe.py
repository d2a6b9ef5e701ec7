#!/usr/bin/env python3
"""Gallery clustering: FaceService.cluster_faces on the device (Engine.gallery_cluster: rows, score tiles and labels stay there, one
int per name comes back) against the route it replaces (use_device_cluster = False: the gallery fetched to the host, CLUSTER_TILE
candidate rows uploaded and a CLUSTER_TILE x N score block downloaded per gallery pass, the sweep in numpy), on one engine and the
same galleries.
Cases: N in {10,000, 100,000} x {fp16 rows, exact float64 rows} x {planted clusters of about 20 rows, all singletons - the worst
case, N / 64 passes}.  One JSON line per case: wall time of either route (one run each behind a warm-up at N = 2,000; the host
route's run is minutes long at N = 100,000), gallery passes, and the bytes either route moves over PCIe (counted from the calls the
host route makes and from the sweep's tiles - not measured on the bus).  The clusters of both routes are compared on the way.
Every case is a child process under its own time limit; the first one that fails ends the run.
    python tools/cluster_probe.py [--sizes 10000,100000] [--kinds planted,singletons] [--rows fp16,exact] [--timeout 900]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR = 0.9
PER_IDENTITY = 20


def gallery(n, kind, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    out = np.empty((n, 512), np.float32)
    centres = rng.standard_normal(((n + PER_IDENTITY - 1) // PER_IDENTITY, 512)).astype(np.float32)
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    ident = rng.integers(0, centres.shape[0], n)
    for i0 in range(0, n, 8192):
        m = min(8192, n - i0)
        v = rng.standard_normal((m, 512)).astype(np.float32)
        if kind == "planted":                      # cos of two rows of an identity ~ 0.83: d ~ 0.58 < THR; strangers: d ~ 1.41
            v = centres[ident[i0:i0 + m]] + np.float32(0.02) * v
        out[i0:i0 + m] = v / np.linalg.norm(v, axis=1, keepdims=True)
    return out


def sweep_tiles(seed_pos, tile):
    """(gallery passes, candidates over all passes) of the tiled sweep that ended in these labels"""
    import numpy as np
    n = len(seed_pos)
    assigned = np.zeros(n, bool)
    cursor = passes = cands = 0
    while cursor < n:
        cand = (cursor + np.nonzero(~assigned[cursor:])[0])[:tile]
        if cand.size == 0:
            break
        passes += 1
        cands += int(cand.size)
        assigned |= np.isin(seed_pos, cand[seed_pos[cand] == cand])
        cursor = int(cand[-1]) + 1
    return passes, cands


def run_case(n, kind, rows):
    import numpy as np
    os.environ["FRP_EXACT_COMPAT"] = "1" if rows == "exact" else "0"
    sys.path.insert(0, ROOT)
    import frp_amd_loader  # noqa: F401
    from frp_amd import native
    from frp_amd.face_service import CLUSTER_TILE, FaceService
    eng = native.Engine(0)
    fs = FaceService(engine=eng)
    assert fs.ENCODINGS.exact == (rows == "exact")
    moved = {"up": 0, "down": 0, "passes": 0}

    def counted(fn, up_per_query, down_per_score):
        def call(q):
            out = fn(q)
            moved["passes"] += 1
            moved["up"] += len(q) * up_per_query
            moved["down"] += out.size * down_per_score
            return out
        return call

    def fetched(fn, row_bytes):
        def call(*a):
            out = fn(*a)
            moved["down"] += len(out) * row_bytes
            return out
        return call

    def both_routes(count):
        names = [f"id{i}" for i in range(len(fs.ENCODINGS))]
        res = {}
        for route, on in (("device", True), ("host", False)):
            fs.use_device_cluster = on
            t0 = time.perf_counter()
            res[route] = fs.cluster_faces(THR)
            res[route + "_s"] = time.perf_counter() - t0
        assert res["device"] == res["host"], "the two routes disagree"
        if not count:
            return None
        pos_of = {nm: p for p, nm in enumerate(names)}
        seed_pos = np.empty(len(names), np.int64)
        for members in res["device"].values():
            seed_pos[[pos_of[m] for m in members]] = pos_of[members[0]]
        res["clusters"] = len(res["device"])
        res["tiles"] = sweep_tiles(seed_pos, min(CLUSTER_TILE, 64))
        return res

    fs.ENCODINGS.set_bulk([f"id{i}" for i in range(2000)], gallery(2000, kind, 1))          # warm-up: allocations, first launches
    both_routes(False)
    fs.ENCODINGS.set_bulk([f"id{i}" for i in range(n)], gallery(n, kind, 2))
    eng.match_scores = counted(eng.match_scores, 512 * 4, 4)
    eng.gallery_distances = counted(eng.gallery_distances, 512 * 8, 8)
    eng.gallery_get = fetched(eng.gallery_get, 512 * 2)
    eng.gallery_get_exact = fetched(eng.gallery_get_exact, 512 * 8)
    launches = eng.counters()["match_launches"]
    res = both_routes(True)
    launches = eng.counters()["match_launches"] - launches - (0 if rows == "exact" else moved["passes"])      # the device route's alone
    passes, cands = res["tiles"]
    assert moved["passes"] == passes and (rows == "exact" or launches == passes), (moved, passes, launches)
    print(json.dumps({"case": f"{kind}-{rows}-{n}", "n": n, "rows": rows, "gallery": kind, "threshold": THR, "clusters": res["clusters"],
                      "device_s": round(res["device_s"], 4), "host_s": round(res["host_s"], 4),
                      "speedup": round(res["host_s"] / res["device_s"], 1), "passes": passes,
                      "device_pcie_bytes": n * 4 + n * 4 + passes * 8 + 4, "host_pcie_bytes": moved["up"] + moved["down"]}), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,100000")
    ap.add_argument("--kinds", default="planted,singletons")
    ap.add_argument("--rows", default="fp16,exact")
    ap.add_argument("--timeout", type=int, default=900, help="seconds per case")
    ap.add_argument("--case", nargs=3, metavar=("N", "KIND", "ROWS"), help="(internal) run one case in this process")
    a = ap.parse_args()
    if a.case:
        run_case(int(a.case[0]), a.case[1], a.case[2])
        return 0
    for n in a.sizes.split(","):
        for kind in a.kinds.split(","):
            for rows in a.rows.split(","):
                rc = subprocess.call(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--case", n, kind, rows])
                if rc != 0:
                    print(f"cluster_probe: case {kind}-{rows}-{n} ended with status {rc}: stopping", file=sys.stderr)
                    return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
