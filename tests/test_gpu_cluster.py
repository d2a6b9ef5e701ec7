"""GPU: gallery clustering on the device (frp_gallery_cluster / Engine.gallery_cluster / FaceService.cluster_faces) against the host
model of the sweep (tests/cluster_model.py) over the very scores the host route reads - frp_match_scores of the rows as queries,
frp_gallery_distances of the exact rows - so every comparison is an equality of integers."""
import json
import math
import os

import numpy as np
import pytest

import frp_amd.face_service as fsmod
from cluster_model import cluster_tiled_fast
from frp_amd import native
from frp_amd.face_service import FaceService, cluster_min_cos

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
D = native.EMB_DIM
THR = 0.9                                   # distance threshold of the synthetic galleries: cos >= ~0.595
SIZES = (1, 2, 65, 129, 200, 1000)          # cross the tile (64), the matcher's 32-query padding and its 128-row workgroup
TILES = (1, 3, 64)


@pytest.fixture(autouse=True)
def _exact_rows_and_clean_gallery(engine):
    engine.gallery_exact(True)
    yield
    engine.gallery_exact(True)
    engine.gallery_set(np.zeros((0, D), np.float32))


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _singletons(n, rng):
    return _unit(rng.standard_normal((n, D)))


def _planted(n, rng, per=5):
    """identities of about `per` rows; the noise level differs per row, so that pairs fall on both sides of THR"""
    centres = _unit(rng.standard_normal(((n + per - 1) // per, D)))
    ident = rng.integers(0, centres.shape[0], n)
    sigma = rng.uniform(0.01, 0.04, (n, 1))
    return _unit(centres[ident] + sigma * rng.standard_normal((n, D)))


def _chain(rng):
    """A~B, B~C, A!~C: unit rows at 0, 45 and 90 degrees in one plane (cos 45 = 0.707 passes THR, cos 90 = 0 does not)"""
    e = np.linalg.qr(rng.standard_normal((D, 2)))[0].T
    ang = np.deg2rad([0.0, 45.0, 90.0])
    return np.cos(ang)[:, None] * e[0] + np.sin(ang)[:, None] * e[1]


def _mixed(n, rng):
    """a chain, a zero row, exact duplicates, planted clusters and singletons, interleaved"""
    if n < 16:
        return _planted(n, rng)
    rows = np.concatenate([_planted(n // 2, rng), _singletons(n - n // 2, rng)])
    rows = rows[rng.permutation(n)]
    rows[2:5] = _chain(rng)
    rows[7] = 0.0
    rows[n - 3] = rows[1]                    # exact duplicates, far apart and next to each other
    rows[11] = rows[10]
    return rows


def _expected(engine, order, exact, tile):
    """the host model over the scores of the present route: the rows as queries against the gallery, columns taken in `order`"""
    order = np.asarray(order)
    if exact:
        passes = engine.gallery_distances(engine.gallery_get_exact()[order])[:, order] <= THR
    else:
        passes = engine.match_scores(engine.gallery_get().astype(np.float32)[order])[:, order] >= np.float32(cluster_min_cos(THR))
    return cluster_tiled_fast(passes, tile)


def _bound(exact):
    return {"max_dist": THR} if exact else {"min_cos": cluster_min_cos(THR)}


def _check_all_tiles(engine, order, exact, what):
    exp_pos, exp_n = _expected(engine, order, exact, 64)
    for tile in TILES:
        pos, k = engine.gallery_cluster(order, tile=tile, **_bound(exact))
        assert pos.dtype == np.int32 and np.array_equal(pos, exp_pos) and k == exp_n, (what, tile, np.nonzero(pos != exp_pos)[0][:8])
    pos, k = engine.gallery_cluster(order, **_bound(exact))                  # tile 0: the largest
    assert np.array_equal(pos, exp_pos) and k == exp_n, what
    return exp_pos, exp_n


@pytest.mark.parametrize("exact", [False, True], ids=["fp16", "exact"])
@pytest.mark.parametrize("n", SIZES)
def test_parity_with_the_host_model_over_device_scores(engine, n, exact):
    rng = np.random.default_rng(100 * n + exact)
    # --- all singletons (n / tile passes), the whole gallery in enrolment order
    engine.gallery_set(_singletons(n, rng))
    before = engine.counters()["match_launches"]
    pos, k = engine.gallery_cluster(np.arange(n), tile=64, **_bound(exact))
    assert k == n and np.array_equal(pos, np.arange(n))
    assert engine.counters()["match_launches"] - before == (0 if exact else math.ceil(n / 64))      # the fp16 route's passes are counted
    _check_all_tiles(engine, np.arange(n), exact, "singletons")
    # --- one cluster of everything
    engine.gallery_set(_unit(_unit(rng.standard_normal((1, D))) + 0.01 * rng.standard_normal((n, D))))
    pos, k = _check_all_tiles(engine, np.arange(n), exact, "one")
    assert k == 1 and not pos.any()
    # --- mixed rows; rows removed in the middle and one enrolled again (a permuted order), two names left out (a strict subset)
    extra = 3 if n >= 16 else 0
    rows = _mixed(n + extra, rng)
    if exact and n >= 16:
        rows[13] = np.nan                                                    # a NaN row is a cluster of one and joins nobody
    engine.gallery_set(rows)
    names = list(range(n + extra))                                           # names[p]: the enrolment id at position p (dict order)
    row_of = {i: i for i in names}
    if extra:
        for victim in (names[(n + extra) // 2], names[5]):                   # the last row moves into the freed one
            r, last = row_of.pop(victim), engine.gallery_size() - 1
            names.remove(victim)
            engine.gallery_remove_row(r)
            for i, ri in row_of.items():
                if ri == last:
                    row_of[i] = r
        engine.gallery_update_row(engine.gallery_size(), _unit(rng.standard_normal(D)))
        row_of[-1] = engine.gallery_size() - 1
        names.append(-1)
        assert engine.gallery_size() == n + 2
        names = names[:5] + names[6:-4] + names[-3:]                         # n of the n + 2 names (the chain and the zero row stay)
    order = np.array([row_of[i] for i in names])
    assert order.size == n and (extra == 0 or not np.array_equal(order, np.sort(order)))
    exp_pos, _ = _check_all_tiles(engine, order, exact, "mixed")
    if extra:
        assert exp_pos[np.nonzero(order == 7)[0][0]] == np.nonzero(order == 7)[0][0]      # the zero row seeds itself


@pytest.mark.parametrize("exact", [False, True], ids=["fp16", "exact"])
def test_chain_depends_on_the_enrolment_order(engine, exact):
    rng = np.random.default_rng(5)
    a, b, c = _chain(rng)
    rest = _singletons(140, rng)
    for first, want in (((a, b, c), [0, 0, 2]), ((b, a, c), [0, 0, 0]), ((c, b, a), [0, 0, 2]), ((a, c, b), [0, 1, 0])):
        rows = np.concatenate([np.stack(first), rest])
        engine.gallery_set(rows)
        exp_pos, exp_n = _check_all_tiles(engine, np.arange(rows.shape[0]), exact, "chain")
        assert exp_pos[:3].tolist() == want and exp_n == 140 + len(set(want))
        # the same rows enrolled behind two tiles of singletons
        engine.gallery_set(np.concatenate([rest, np.stack(first)]))
        exp_pos, _ = _check_all_tiles(engine, np.arange(rows.shape[0]), exact, "chain at the end")
        assert (exp_pos[140:] - 140).tolist() == want


def test_boundary_fp16_route(engine):
    """min_cos equal to a real score takes the row; the next float32 up does not"""
    rng = np.random.default_rng(11)
    rows = _singletons(70, rng)
    rows[40] = _unit(rows[3] + 0.03 * rng.standard_normal(D))
    engine.gallery_set(rows)
    s = engine.match_scores(engine.gallery_get().astype(np.float32))[3, 40]
    assert 0.5 < s < 0.999
    order = np.arange(70)
    pos, k = engine.gallery_cluster(order, min_cos=float(s))
    assert pos[40] == 3 and k == 69 and (np.delete(pos, 40) == np.delete(order, 40)).all()
    pos, k = engine.gallery_cluster(order, min_cos=float(np.nextafter(s, np.float32(np.inf))))
    assert np.array_equal(pos, order) and k == 70
    pos, k = engine.gallery_cluster(order, min_cos=float("nan"))             # a bound no score reaches
    assert np.array_equal(pos, order) and k == 70
    pos, k = engine.gallery_cluster(order, min_cos=float("-inf"))
    assert not pos.any() and k == 1


def test_boundary_exact_route(engine):
    """max_dist equal to a real distance takes the row; the next float64 down does not"""
    rng = np.random.default_rng(12)
    rows = _singletons(70, rng)
    rows[40] = rows[3] + 0.01 * rng.standard_normal(D)                       # not a unit vector: the exact rows are as enrolled
    engine.gallery_set(rows)
    d = float(engine.gallery_distances(engine.gallery_get_exact())[3, 40])
    assert 0.05 < d < 0.6
    order = np.arange(70)
    pos, k = engine.gallery_cluster(order, max_dist=d)
    assert pos[40] == 3 and k == 69 and (np.delete(pos, 40) == np.delete(order, 40)).all()
    pos, k = engine.gallery_cluster(order, max_dist=float(np.nextafter(d, -np.inf)))
    assert np.array_equal(pos, order) and k == 70
    pos, k = engine.gallery_cluster(order, max_dist=float("nan"))
    assert np.array_equal(pos, order) and k == 70


def test_larger_gallery_is_deterministic(engine):
    n = 4096
    rng = np.random.default_rng(13)
    engine.gallery_set(_planted(n, rng, per=20).astype(np.float32))
    order = np.arange(n)
    exp_pos, exp_n = _expected(engine, order, False, 64)
    assert 100 < exp_n < n // 2                                              # (the gallery is what it is meant to be: planted clusters)
    pos1, k1 = engine.gallery_cluster(order, min_cos=cluster_min_cos(THR))
    pos2, k2 = engine.gallery_cluster(order, min_cos=cluster_min_cos(THR))
    assert np.array_equal(pos1, pos2) and k1 == k2
    assert np.array_equal(pos1, exp_pos) and k1 == exp_n


def _golden():
    meta = json.load(open(os.path.join(HERE, "golden", "plumbing_golden.json")))
    return meta, np.load(os.path.join(HERE, "golden", "plumbing_golden.npz"))


def _spy(engine, monkeypatch):
    calls, orig = [], engine.gallery_cluster
    monkeypatch.setattr(engine, "gallery_cluster", lambda *a, **kw: (calls.append(kw), orig(*a, **kw))[1], raising=False)
    return calls


def test_service_device_route_on_exact_rows_vs_reference_golden(engine, monkeypatch):
    meta, arrays = _golden()
    calls = _spy(engine, monkeypatch)
    for case in meta["cases"]:                                               # the 128-d cases too
        fs = FaceService(engine=engine)
        assert fs.ENCODINGS.exact and fs.use_device_cluster
        fs.ENCODINGS.clear()
        for name, g in zip(case["names"], arrays[f"case{case['id']}_G"]):
            assert fs.store_face(name, g)["success"]
        for t, exp in case["clusters"].items():
            calls.clear()
            assert fs.cluster_faces(float(t)) == exp, (case["id"], t)
            assert len(calls) == 1 and calls[0]["max_dist"] == float(t) and calls[0]["tile"] == 64
        fs.ENCODINGS.clear()


def test_service_device_route_equals_host_route_on_fp16_rows(engine, monkeypatch):
    meta, arrays = _golden()
    calls = _spy(engine, monkeypatch)
    for tile in (64, 3):
        monkeypatch.setattr(fsmod, "CLUSTER_TILE", tile)
        for case in meta["cases"]:
            if case["D"] != 512:
                continue
            fs = FaceService(engine=engine)
            fs.ENCODINGS.clear()
            fs.ENCODINGS.exact = False                                       # the compat calls on the unit fp16 rows
            for name, g in zip(case["names"], arrays[f"case{case['id']}_G"]):
                assert fs.store_face(name, g)["success"]
            # a removal in the middle: rows are no longer in dict order
            assert fs.delete_face(case["names"][2])["success"]
            names = fs.ENCODINGS.names()
            assert not np.array_equal(fs.ENCODINGS.rows_of(names), np.arange(len(names)))
            for t in case["clusters"]:
                calls.clear()
                fs.use_device_cluster = True
                dev = fs.cluster_faces(float(t))
                assert len(calls) == 1 and calls[0]["tile"] == tile and calls[0]["min_cos"] == cluster_min_cos(float(t))
                fs.use_device_cluster = False
                host = fs.cluster_faces(float(t))
                assert len(calls) == 1 and dev == host, (case["id"], t, tile)
            fs.ENCODINGS.clear()


def test_argument_checks(engine):
    rows = _singletons(10, np.random.default_rng(3))
    engine.gallery_set(rows)
    ok = np.arange(10)

    def refused(code, *args, **kw):
        with pytest.raises(native.FrpError) as e:
            engine.gallery_cluster(*args, **kw)
        assert e.value.code == code and len(str(e.value)) > len(f"frp error {code}: ")
    refused(-1, [0, 1, 1], min_cos=0.5)                                      # a duplicate row
    refused(-1, [0, 10], min_cos=0.5)                                        # a row out of range
    refused(-1, [0, -1], min_cos=0.5)
    refused(-1, ok, min_cos=0.5, tile=65)
    refused(-1, ok, min_cos=0.5, tile=-1)
    refused(-1, [], min_cos=0.5)
    with pytest.raises(ValueError):
        engine.gallery_cluster(ok)
    with pytest.raises(ValueError):
        engine.gallery_cluster(ok, min_cos=0.5, max_dist=0.5)
    engine.gallery_exact(False)
    refused(-1, ok, max_dist=0.5)                                            # FRP_CLUSTER_EXACT without exact rows
    pos, k = engine.gallery_cluster(ok, min_cos=0.5)                         # ... the fp16 route does not need them
    assert np.array_equal(pos, ok) and k == 10
    engine.gallery_exact(True)
    engine.gallery_set(np.zeros((0, D), np.float32))
    refused(-4, [0], min_cos=0.5)                                            # an empty gallery
    refused(-4, [0], max_dist=0.5)
