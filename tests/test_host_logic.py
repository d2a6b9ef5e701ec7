"""CPU tests of the host side: FaceService bookkeeping against the reference-derived golden
vectors (through a float64 test double of the engine), BatchNorm folding against the oracle,
layer tables, blob layout, and the C-ABI export list."""
import json
import os
import re
import struct

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fake_engine import FakeEngine
from frp_amd import native, netspec, weights
from frp_amd.face_service import FaceService, box_to_location, calibrate_confidence, confidence_level
from oracle import network as onet

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def golden():
    meta = json.load(open(os.path.join(HERE, "golden", "plumbing_golden.json")))
    arrays = np.load(os.path.join(HERE, "golden", "plumbing_golden.npz"))
    return meta, arrays


def _same(a, b, tol=1e-6):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert list(x.keys()) == list(y.keys())
        for k in x:
            if isinstance(y[k], float):
                assert abs(x[k] - y[k]) <= (0.011 if k == "confidence_score" else tol), (k, x[k], y[k])
            else:
                assert x[k] == y[k], (k, x[k], y[k])


def test_abi_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "frp.h")).read()
    declared = sorted(set(re.findall(r"\b(frp_[a-z0-9_]+)\s*\(", hdr)))
    assert declared, "no declarations parsed"
    lib = native.load_library()          # fails loudly if libfrp.so is not built
    for name in declared:
        assert hasattr(lib, name), f"libfrp.so does not export {name}"
    assert set(declared) == set(native.ABI_SYMBOLS)
    assert lib.frp_version().startswith(b"frp ")
    assert not hasattr(lib, "upload_jpeg_device")          # an ingest helper the library once exported by accident
    # the shipped library carries no tuning hooks: those live in the FRP_LAB build (include/frp_lab.h, libfrp_lab.so)
    lab = sorted(set(re.findall(r"\b(frp_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", "frp_lab.h")).read())))
    assert lab == ["frp_conv_bench", "frp_kstep_lab", "frp_mfma_peak"] and not any(hasattr(lib, n) for n in lab)


def test_no_gpu_means_loud_failure_not_fallback():
    import torch as _t
    if _t.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(native.FrpError):
        native.Engine(0)
    fs = FaceService()
    r = fs.encode_face(np.zeros((32, 32, 3), np.uint8))
    assert r["success"] is False and r["face_count"] == 0 and "frp error" in r["message"]   # reference error convention
    assert list(r.keys()) == ["success", "face_count", "encodings", "message", "processing_time"]


def test_service_matches_reference_golden(golden):
    meta, arrays = golden
    assert [confidence_level(r["d"]) for r in meta["confidence"]] == [r["level"] for r in meta["confidence"]]
    assert [calibrate_confidence(r["d"]) for r in meta["confidence"]] == [r["score"] for r in meta["confidence"]]
    for case in meta["cases"]:
        G, Q = arrays[f"case{case['id']}_G"], arrays[f"case{case['id']}_Q"]     # unit rows
        fs = FaceService(engine=FakeEngine())
        fs.tolerance = case["tolerance"]
        for n, g in zip(case["names"], G):
            assert fs.store_face(n, g)["success"]
        assert fs.get_all_targets() == case["names"]
        for q, exp, knn in zip(Q, case["compare"], case["knn"]):
            _same(fs.compare_faces(q), exp)
            for k, e in knn.items():
                _same(fs.find_k_nearest(q, int(k)), e)
        for g_, e in zip(fs.batch_compare_faces(list(Q)), case["batch"]):
            _same(g_, e)
        _same(fs.compare_faces(Q[1], target_names=case["subset"]["target_names"]), case["subset"]["result"])
        _same(fs.compare_faces(Q[1], return_distances=False), case["no_dist"])
        for t, exp in case["clusters"].items():
            assert fs.cluster_faces(float(t)) == exp
        dup = arrays[f"case{case['id']}_dup"]
        assert fs.store_face("new_person", dup) == case["store_dup"]      # as the reference got it: not a unit vector
        assert fs.store_face(case["names"][0], G[0]) == case["store_update"]
        assert fs.get_all_targets() == case["targets_after"]
        m = fs.get_performance_metrics()
        assert sorted(m.keys()) == meta["metrics_keys"]
    fs = FaceService(engine=FakeEngine())
    assert fs.compare_faces(np.zeros(4)) == [] and fs.find_k_nearest(np.zeros(4), 3) == []
    assert fs.batch_compare_faces([np.zeros(4), np.ones(4)]) == meta["empty_batch"]
    assert fs.cluster_faces() == meta["empty_clusters"]
    assert fs.health_check() == meta["health_empty"]


def test_gallery_name_table_survives_delete_and_update():
    rng = np.random.default_rng(1)
    fs = FaceService(engine=FakeEngine())
    E = rng.standard_normal((6, 512))
    E /= np.linalg.norm(E, axis=1, keepdims=True)
    for i in range(6):
        fs.store_face(f"p{i}", E[i])
    assert fs.delete_face("p1")["success"] and not fs.delete_face("p1")["success"]
    assert fs.get_all_targets() == ["p0", "p2", "p3", "p4", "p5"]           # dict order kept (device row of p5 moved)
    for i in (0, 2, 3, 4, 5):
        top = fs.find_k_nearest(E[i], 1)[0]
        assert top["target"] == f"p{i}" and top["distance"] < 1e-6
    assert np.allclose(fs.ENCODINGS["p5"], E[5]) and "p1" not in fs.ENCODINGS and len(fs.ENCODINGS) == 5
    fs.store_face("p2", E[1])                                                # overwrite
    assert fs.find_k_nearest(E[1], 1)[0]["target"] == "p2"


def test_delete_between_match_and_lookup_cannot_misattribute():
    """store/delete move device rows (swap-remove).  A delete that lands between the device match and the row -> name
    lookup must not attribute the face to the identity that was moved into its row (the reference builds names and
    matrix in one call, face_service.py:403-411): readers hold the gallery lock across both."""
    import threading
    rng = np.random.default_rng(3)
    E = rng.standard_normal((6, 512))
    E /= np.linalg.norm(E, axis=1, keepdims=True)

    class SlowEngine(FakeEngine):
        """lets a deleter run while the 'device' call is in flight"""
        def __init__(self):
            super().__init__()
            self.in_call = threading.Event()
            self.go = threading.Event()

        def match(self, q, topk=1):
            r = super().match(q, topk)
            self.in_call.set()
            self.go.wait(2.0)
            return r

        def gallery_distances(self, q):      # (the exact compat rows: find_k_nearest's device call by default)
            r = super().gallery_distances(q)
            self.in_call.set()
            self.go.wait(2.0)
            return r

    eng = SlowEngine()
    fs = FaceService(engine=eng)
    for i in range(6):
        fs.store_face(f"p{i}", E[i])
    out = {}
    t = threading.Thread(target=lambda: out.setdefault("r", fs.find_k_nearest(E[1], 1)))
    t.start()
    assert eng.in_call.wait(2.0)
    d = threading.Thread(target=lambda: out.setdefault("d", fs.delete_face("p1")))   # row 1 <- p5 (swap-remove)
    d.start()
    d.join(0.2)
    assert d.is_alive()                      # the delete waits for the reader's lock instead of racing the lookup
    eng.go.set()
    t.join()
    d.join()
    assert out["r"][0]["target"] == "p1" and out["d"]["success"]
    assert fs.find_k_nearest(E[5], 1)[0]["target"] == "p5"


def test_match_scores_buffer_follows_gallery_growth():
    """native.Engine.match_scores sizes its output from gallery_size(); the library refuses (and the binding
    retries) when the gallery changed in between - exercised here through the same retry loop on a stub library"""
    from frp_amd import native

    class Lib:
        def __init__(self):
            self.n = 5
            self.calls = 0

        def frp_gallery_size(self, h):
            return self.n

        def frp_match_scores(self, h, q, m, out, n_cols):
            self.calls += 1
            if self.calls == 1:
                self.n = 6                   # a store_face slipped in: capacity no longer matches
            return 0 if n_cols == self.n else -1

        def frp_last_error(self, h):
            return b"match_scores: output sized for another gallery size"

    eng = native.Engine.__new__(native.Engine)
    eng._lib, eng._h = Lib(), None
    out = eng.match_scores(np.zeros((2, 512), np.float32))
    assert out.shape == (2, 6) and eng._lib.calls == 2


def test_quality_matches_reference_geometry_and_formulas(golden):
    meta, _ = golden
    fs = FaceService(engine=FakeEngine())
    img = np.zeros((480, 640, 3), np.uint8)
    for q in meta["quality"]:
        got = fs.assess_face_quality(img, tuple(q["loc"]))
        for k in ("size_score", "position_score", "aspect_score"):
            assert got[k] == q["result"][k]
    # blur / lighting on a known pattern: checkerboard of 0/255 -> Laplacian variance and std are closed-form
    yy, xx = np.mgrid[0:64, 0:64]
    cb = (((yy + xx) % 2) * 255).astype(np.uint8)
    g = fs.assess_face_quality(np.stack([cb] * 3, -1), (0, 64, 64, 0))
    assert g["blur_score"] == 100.0 and abs(g["lighting_score"] - (100.0 - 0.5 / 128 * 100 + 100.0) / 2) < 0.5
    flat = fs.assess_face_quality(np.full((64, 64, 3), 128, np.uint8), (0, 64, 64, 0))
    assert flat["blur_score"] == 0.0 and "Image is blurry - use better focus or steady camera" in flat["issues"]
    assert fs.get_quality_statistics()["total_assessments"] == len(meta["quality"]) + 2


def test_encode_and_stream_formatting_from_device_results():
    eng = FakeEngine()
    B, K = 1, 4
    emb = np.zeros((B, K, 512), np.float32)
    emb[0, 0, 0] = emb[0, 1, 1] = 1.0
    eng.canned = dict(boxes=np.array([[[10.7, 20.2, 110.9, 140.1], [-5.0, 3.0, 700.0, 500.0], [0] * 4, [0] * 4]], np.float32),
                      kps=np.zeros((B, K, 5, 2), np.float32), scores=np.array([[0.9, 0.8, 0, 0]], np.float32),
                      counts=np.array([2], np.int32), emb=emb,
                      match_idx=np.array([[1, 0, -1, -1]], np.int32), match_cos=np.array([[0.98, 0.5, -1, -1]], np.float32))
    fs = FaceService(engine=eng)
    r = fs.encode_face(np.zeros((480, 640, 3), np.uint8), return_locations=True)
    assert r["success"] and r["face_count"] == 2 and r["message"] == "Successfully encoded 2 face(s)"
    assert r["locations"] == [(20, 110, 140, 10), (3, 640, 480, 0)]           # (top,right,bottom,left), clipped
    assert r["encodings"][0].dtype == np.float64 and r["encodings"][0].shape == (512,)
    assert box_to_location([1.9, 2.9, 3.9, 4.9], 100, 100) == (2, 3, 4, 1)
    fs.store_face("alice", emb[0, 0])
    fs.store_face("bob", emb[0, 1])
    faces = fs.process_frames(np.zeros((1, 480, 640, 3), np.uint8), max_faces=K)[0]
    assert [f["target"] for f in faces] == ["bob", "alice"]
    assert faces[0]["match"] and faces[0]["confidence"] == "high" and abs(faces[0]["distance"] - 0.2) < 1e-6
    assert not faces[1]["match"] and faces[1]["confidence"] == "low"
    eng.canned["counts"] = np.array([0], np.int32)
    r = fs.encode_face(np.zeros((480, 640, 3), np.uint8))
    assert r == {"success": False, "face_count": 0, "encodings": [], "message": "No faces detected in image",
                 "processing_time": r["processing_time"]}
    assert fs.encode_face(12345)["message"] == "Invalid input type"
    m = fs.get_performance_metrics()
    assert m["total_encodings"] == 4 and m["failed_encodings"] == 1


# ------------------------------------------------------------------ layer tables / folding / blob
def test_layer_tables_match_published_work():
    emb = netspec.iresnet_layers()
    macs, _ = netspec.layer_macs(emb, 112, 112, "emb.in")
    assert macs == 12_089_606_144                      # 12,089.6 MMAC = 24.18 GFLOP per face
    det = netspec.detector_layers()
    dm, per = netspec.layer_macs(det, 1088, 1920, "det.in")
    assert dm == 72_956_405_760
    assert netspec.num_anchors(1088, 1920) == 85680 and netspec.num_anchors(640, 640) == 16800
    r50, _ = netspec.layer_macs(netspec.iresnet_layers((3, 4, 14, 3)), 112, 112, "emb.in")
    assert abs(r50 * 2 / 1e9 - 12.62) < 0.05


def _apply_folded(x_nchw, w16, bias, slope, l):
    """fp32 evaluation of a folded layer exactly as the kernel defines it."""
    w = torch.from_numpy(w16.astype(np.float32)).permute(0, 3, 1, 2)
    y = F.conv2d(x_nchw, w, None, stride=l.stride, padding=l.k // 2)
    _, _, Ho, Wo = y.shape
    if l.flags & netspec.FLAG_BORDER_BIAS:
        cy = np.where(np.arange(Ho) == 0, 0, np.where(np.arange(Ho) == Ho - 1, 2, 1))
        cx = np.where(np.arange(Wo) == 0, 0, np.where(np.arange(Wo) == Wo - 1, 2, 1))
        b = torch.from_numpy(bias[cy[:, None] * 3 + cx[None, :]]).permute(2, 0, 1)[None]
    else:
        b = torch.from_numpy(bias)[None, :, None, None]
    y = y + b
    return y


def test_bn_folding_including_border_bias_equals_oracle_block():
    raw = weights.make_synthetic_raw(3, (1, 1, 1, 1), (1, 1, 1, 1), want_det=False)
    layers = {l.name: l for l in netspec.iresnet_layers((1, 1, 1, 1))}
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.standard_normal((2, 64, 9, 11)).astype(np.float32))
    p = "emb.layer2.0"
    # oracle: bn1 -> conv1 -> bn2 -> prelu
    t = onet._bn(raw, f"{p}.bn1", x)
    t = onet._conv(raw, f"{p}.conv1", t, 1)
    t = F.prelu(onet._bn(raw, f"{p}.bn2", t), onet._t(raw, f"{p}.prelu.weight"))
    l = layers[f"{p}.conv1"]
    w16, bias, slope = weights.fold_layer(raw, l)
    assert bias.shape == (9, 128)
    y = _apply_folded(x, w16, bias, slope, l)
    y = torch.where(y > 0, y, y * torch.from_numpy(slope)[None, :, None, None])
    assert float((y - t).abs().max()) < 5e-3 * float(t.abs().max())       # only the fp16 weight rounding differs
    # without the border classes the frame of the map would be wrong: prove the classes matter
    y_mid = _apply_folded(x, w16, np.broadcast_to(bias[4], bias.shape).copy(), slope, l)
    assert float((y_mid - _apply_folded(x, w16, bias, slope, l)).abs().max()) > 1e-3


def test_fc_folding_permutes_to_nhwc():
    raw = weights.make_synthetic_raw(5, (1, 1, 1, 1), (1, 1, 1, 1), want_det=False)
    l = [q for q in netspec.iresnet_layers((1, 1, 1, 1)) if q.name == "emb.fc"][0]
    w16, bias, _ = weights.fold_layer(raw, l)
    rng = np.random.default_rng(1)
    x = rng.standard_normal((3, 512, 7, 7)).astype(np.float32)
    xt = torch.from_numpy(x)
    ref = onet._bn(raw, "emb.bn2", xt).flatten(1)
    ref = F.linear(ref, onet._t(raw, "emb.fc.weight"), onet._t(raw, "emb.fc.bias"))
    ref = F.batch_norm(ref, onet._t(raw, "emb.features.running_mean"), onet._t(raw, "emb.features.running_var"),
                       onet._t(raw, "emb.features.weight"), onet._t(raw, "emb.features.bias"), False, 0.0, 1e-5).numpy()
    nhwc = np.transpose(x, (0, 2, 3, 1)).reshape(3, -1)
    got = nhwc @ w16.reshape(512, -1).astype(np.float32).T + bias[None]
    assert np.abs(got - ref).max() < 5e-3 * np.abs(ref).max()


def test_blob_layout_and_buffer_liveness():
    raw = weights.make_synthetic_raw(7, (1, 1, 1, 1), (1, 1, 1, 1))
    blob = weights.pack_blob(raw, (1, 1, 1, 1), (1, 1, 1, 1))
    hdr = struct.unpack(weights.HEADER_FMT, blob[:weights.HEADER_BYTES])
    assert hdr[0] == b"FRPBLOB1" and hdr[1] == weights.BLOB_VERSION == 2 and hdr[2] == 128
    n_det, n_det_bufs = hdr[3], hdr[4]
    det_off, emb_off, data_off, data_bytes = hdr[19], hdr[20], hdr[21], hdr[22]
    assert data_off % 256 == 0 and data_off + data_bytes == len(blob)
    ob = weights.OP_BYTES
    ops = [struct.unpack(weights.OP_FMT, blob[det_off + i * ob: det_off + (i + 1) * ob]) for i in range(n_det)]
    layers = netspec.detector_layers((1, 1, 1, 1))
    assert len(ops) == len(layers)
    # replay liveness: a physical buffer may only be overwritten once its previous tensor is dead
    holder, last_use = {}, {}
    for i, l in enumerate(layers):
        last_use[l.src] = i
        if l.res:
            last_use[l.res] = i
    for i, (l, op) in enumerate(zip(layers, ops)):
        in_buf, out_buf, res_buf = op[0], op[1], op[2]
        assert holder.get(in_buf, l.src) == l.src and in_buf != out_buf and res_buf != out_buf
        if l.res:
            assert holder[res_buf] == l.res
        prev = holder.get(out_buf)
        assert prev is None or last_use.get(prev, -1) < i, f"{l.name} overwrites live {prev}"
        holder[out_buf] = l.dst
        holder.setdefault(in_buf, l.src)
        assert op[10] % 16 == 0 and op[11] % 16 == 0 and 0 <= out_buf < n_det_bufs


def test_buffer_plan_keeps_the_block_input_for_the_k_concat_consumer():
    """K-concat (csrc/net_program.cpp: plan_kconcat folds a strided block's 1x1 shortcut conv into the 3x3 conv that adds
    it): the fused conv reads the shortcut's INPUT, so the packer must keep that tensor alive until then and must not hand
    its buffer to the conv's output - the runtime refuses the fusion otherwise (and the four launches stay separate)."""
    for blocks in ((1, 1, 1, 1), (3, 13, 30, 3)):
        layers = netspec.iresnet_layers(blocks)
        phys, n = weights.assign_buffers(layers, ["emb.in", "emb.out"])
        prod = {l.dst: l for l in layers}
        fused = 0
        for j, l in enumerate(layers):
            sc = prod.get(l.res) if l.res else None
            if sc is None or sc.k != 1:
                continue
            fused += 1
            assert l.k == 3 and l.stride == sc.stride == 2
            assert phys[l.dst] != phys[sc.src] and phys[l.src] != phys[sc.src]
            # nobody writes into the shortcut input's buffer between the shortcut op and its consumer
            i = layers.index(sc)
            for q in layers[i + 1: j]:
                assert phys[q.dst] != phys[sc.src], q.name
        assert fused == 4
        assert n <= 9                                   # (liveness still recycles: a handful of buffers whatever the depth)


def test_arcface_checkpoint_loader_roundtrip(tmp_path):
    """a checkpoint in the public arcface_torch naming loads into the raw dict pack_blob consumes"""
    raw = weights.make_synthetic_raw(11, (1, 1, 1, 1), (1, 2, 1, 1), want_det=False)
    sd = {"module." + k[4:]: torch.from_numpy(v) for k, v in raw.items()}
    sd["module.bn1.num_batches_tracked"] = torch.tensor(5)
    path = str(tmp_path / "backbone.pth")
    torch.save({"state_dict": sd}, path)
    got = weights.load_arcface_state_dict(path)
    assert set(got) == set(raw) and all(np.array_equal(got[k], raw[k]) for k in raw)
    assert weights.emb_blocks_of(got) == (1, 2, 1, 1)
    det = weights.make_synthetic_raw(11, (1, 1, 1, 1), (1, 2, 1, 1), want_emb=False)
    blob = weights.pack_blob({**det, **got}, (1, 1, 1, 1), weights.emb_blocks_of(got))
    assert blob[:8] == b"FRPBLOB1"


def test_fp8_activation_scales_are_calibrated():
    """BASELINE config 5: the fp8-mfma blob carries per-tensor activation scales from a calibration pass of the fp16
    program (weights.calibrate_fp8) - not 1.0.  (1) every fp8 tensor's writer and reader agree on its scale; (2) scales
    are powers of two that put the observed |max| inside (448 / 4, 448 / 2]; (3) an embedder whose inner activations are
    64 x larger or smaller (same function: conftest.rescaled_embedder_raw) gets scales moved by exactly that factor."""
    import struct
    from conftest import rescaled_embedder_raw
    from frp_amd import netspec as ns, weights as wts
    blocks = (1, 2, 2, 1)
    raw = wts.make_synthetic_raw(19, (1, 1, 1, 1), blocks)
    layers = ns.iresnet_layers(blocks)
    plan = wts.plan_fp8(layers)
    chips = wts.default_calibration_chips(3)
    sc = wts.calibrate_fp8(raw, layers, plan, chips)
    _, amax = wts.run_program_fp32(raw, layers, wts.emb_input_blob(chips), True, want_amax=True)
    assert sc and set(sc) == {l.dst for l, pl in zip(layers, plan) if pl["out8"] or pl["dst2"]}
    for name, s in sc.items():
        assert np.log2(s) == np.round(np.log2(s))
        assert 448 / 4 < amax[name] / s * wts.FP8_HEADROOM <= 448 * 1.0001, (name, amax[name], s)
    for f in (64.0, 1.0 / 64):
        sc2 = wts.calibrate_fp8(rescaled_embedder_raw(raw, blocks, f), layers, plan, chips)
        for name in sc:
            assert sc2[name] == sc[name] * (f if name.endswith(".t") else 1.0), (name, f)
    blob = wts.pack_blob(raw, (1, 1, 1, 1), blocks, weight_format="fp8-mfma", calib_chips=chips)
    hdr = struct.unpack(wts.HEADER_FMT, blob[:wts.HEADER_BYTES])
    n_emb, emb_off = hdr[11], hdr[20]
    ops = [dict(zip(wts.OP_FIELDS, struct.unpack(wts.OP_FMT, blob[emb_off + i * wts.OP_BYTES: emb_off + (i + 1) * wts.OP_BYTES])))
           for i in range(n_emb)]
    written = {}                                  # physical buffer -> scale of the fp8 tensor last written there
    n_checked = 0
    for op, l, pl in zip(ops, layers, plan):
        if pl["f8"]:
            assert op["flags"] & wts.OPFLAG_FP8_MFMA and op["in_scale"] == written[op["in_buf"]] == sc[l.src]
            n_checked += 1
        if pl["out8"]:
            written[op["out_buf"]] = op["out_scale"]
        elif pl["dst2"]:
            written[op["out2_buf"]] = op["out_scale"]
        if pl["out8"] or pl["dst2"]:
            assert op["out_scale"] == sc[l.dst] != 1.0
    assert n_checked == sum(pl["f8"] for pl in plan) > 0
    unit = wts.pack_blob(raw, (1, 1, 1, 1), blocks, weight_format="fp8-mfma", calibrate=False)
    assert len(unit) == len(blob) and unit != blob


def test_fp8_weight_codec_and_blob():
    """BASELINE config 5 storage format: E4M3FN codec properties and the fp8 blob layout"""
    import struct
    from frp_amd import netspec as ns, weights as wts
    t = wts.FP8_E4M3
    assert t[0] == 0 and t[1] == 2.0 ** -9 and t[0x7E] == 448.0 and np.isnan(t[0x7F]) and t[0x80 | 0x7E] == -448.0
    assert np.all(np.diff(t[:127]) > 0)                                   # codes 0..126 ascend
    codes = np.arange(256, dtype=np.uint8)
    ok = ~np.isnan(t)
    back = wts.fp8_e4m3_encode(t[ok])
    assert np.array_equal(t[back], t[ok])                                  # every representable value encodes to itself
    assert wts.fp8_e4m3_encode(np.array([-0.0], np.float32))[0] == 0      # no negative zero codes
    rng = np.random.default_rng(0)
    x = rng.uniform(-448, 448, 20000).astype(np.float32)
    q = t[wts.fp8_e4m3_encode(x)]
    assert np.all(np.abs(q - x) <= np.maximum(np.abs(x) * 2.0 ** -4, 2.0 ** -10))     # half an ulp of a 3-bit mantissa
    mid = (t[8:126] + t[9:127]) / 2                                        # exact ties go to the even code
    assert np.all(wts.fp8_e4m3_encode(mid.astype(np.float32)) % 2 == 0)
    w = (rng.standard_normal((6, 3, 3, 16)) * 0.1).astype(np.float16)
    w[2] = 0
    c, s = wts.fp8_quantize_rows(w)
    d = wts.fp8_dequantize_rows(c, s)
    assert d.dtype == np.float16 and np.all(d[2] == 0) and s[2] == 1.0
    assert np.abs(d.astype(np.float32) - w.astype(np.float32)).max() <= np.abs(w.astype(np.float32)).max() * 2.0 ** -4 * 1.01
    # blob: same program, weights at one byte per element + scales, flag 16 on every op
    raw = wts.make_synthetic_raw(3, (1, 1, 1, 1), (1, 1, 1, 1))
    b16 = wts.pack_blob(raw, (1, 1, 1, 1), (1, 1, 1, 1))
    b8 = wts.pack_blob(raw, (1, 1, 1, 1), (1, 1, 1, 1), weight_format="fp8")
    assert len(b8) < 0.56 * len(b16)
    hdr = struct.unpack(wts.HEADER_FMT, b8[:wts.HEADER_BYTES])
    n_det, det_off = hdr[3], hdr[19]
    op_size = struct.calcsize(wts.OP_FMT)
    for i in range(n_det):
        op = struct.unpack(wts.OP_FMT, b8[det_off + i * op_size: det_off + (i + 1) * op_size])
        assert op[8] & wts.OPFLAG_W_FP8
    with pytest.raises(ValueError):
        wts.pack_blob(raw, (1, 1, 1, 1), (1, 1, 1, 1), weight_format="int4")


def test_lanes_keep_submission_order_and_surface_errors(monkeypatch):
    """lanes.Lanes host logic without a GPU: batches are spread over the lanes' threads, results come back in submission
    order even when a later batch finishes first, the look-ahead is bounded, errors of the iterator and of a lane reach
    the consumer, an abandoned generator stops its workers"""
    import threading
    import time
    from frp_amd import lanes as lanes_mod

    class SlowEngine:
        made = []

        def __init__(self, device, **kw):
            self.calls = []
            self.closed = False
            SlowEngine.made.append(self)

        def process_frames(self, frames, **kw):
            t = int(frames[0])
            if t < 0:
                raise RuntimeError("lane failure")
            time.sleep(0.03 if t % 2 == 0 else 0.001)       # even batches are slow: odd ones overtake them
            self.calls.append((t, threading.get_ident()))
            return {"t": t, "kw": kw}

        def close(self):
            self.closed = True

    monkeypatch.setattr(lanes_mod.native, "Engine", SlowEngine)
    L = lanes_mod.Lanes(0, 2, max_batch=4)
    assert len(SlowEngine.made) == 2
    pulled = []

    def src(n):
        for t in range(n):
            pulled.append(t)
            yield np.array([t])
    got = []
    for out in L.run(src(12), max_faces=3, flags=1):
        got.append(out["t"])
        assert len(pulled) - len(got) <= 2 * 2             # at most 2 x n_lanes batches taken ahead of the consumer
        assert out["kw"]["max_faces"] == 3 and out["kw"]["flags"] == 1
    assert got == list(range(12))
    assert all(e.calls for e in SlowEngine.made)            # both lanes worked, each on its own thread
    assert len({tid for e in SlowEngine.made for _, tid in e.calls}) == 2
    assert list(L.run(iter(()))) == []

    def bad_iter():
        yield np.array([0])
        raise KeyError("camera gone")
    with pytest.raises(KeyError):
        list(L.run(bad_iter()))
    with pytest.raises(RuntimeError):
        list(L.run([np.array([0]), np.array([-1]), np.array([2])]))
    before = threading.active_count()
    g = L.run(src(50))
    next(g)
    g.close()
    assert threading.active_count() <= before
    L.close()
    assert all(e.closed for e in SlowEngine.made)
    with pytest.raises(ValueError):
        lanes_mod.Lanes(0, 0)


def test_abandoned_stream_with_full_look_ahead_does_not_deadlock(monkeypatch):
    """a consumer SLOWER than the device that stops early: the workers are parked on the look-ahead throttle when the
    generator is closed and must leave (they used to wait there forever and close() hung in join()).  Unbounded source;
    close() runs under a watchdog."""
    import itertools
    import threading
    import time
    from frp_amd import lanes as lanes_mod

    def watchdog(fn, seconds=10.0):
        th = threading.Thread(target=fn, daemon=True)
        th.start()
        th.join(seconds)
        assert not th.is_alive(), "generator close() hung: workers parked on the throttle never woke up"

    g = lanes_mod.run_ordered((np.array([t]) for t in itertools.count()), [lambda x: int(x[0])] * 2)
    assert next(g) == 0
    time.sleep(0.2)                      # both workers run ahead until the look-ahead (2 x 2 items) is full and park
    watchdog(g.close)
    # ... and when the consumer's loop body raises
    def body():
        with pytest.raises(ZeroDivisionError):
            for out in lanes_mod.run_ordered((np.array([t]) for t in itertools.count()), [lambda x: int(x[0])] * 3):
                time.sleep(0.1)
                1 / 0
    watchdog(body)
    with pytest.raises(ValueError):
        next(lanes_mod.run_ordered([1], []))


def test_run_ordered_deferred_results_are_finished_under_the_next_item_or_at_once():
    """lanes.Deferred (FaceService.process_stream builds a batch's result dicts while the lane's next batch is on the device):
    finish() runs on the worker's own thread - inside its next call, where that call invokes take_next.idle(), when a next item
    had been claimed; immediately when none had - every result arrives exactly once, in order, also when the source is
    slower than the workers (nothing claimed ahead: nothing may be held back) and when a worker never calls idle()."""
    import itertools
    import threading
    import time
    from frp_amd import lanes as lanes_mod

    for slow_source, calls_idle in ((False, True), (True, True), (False, False)):
        log = []
        lock = threading.Lock()

        def src(n):
            for t in range(n):
                if slow_source:
                    time.sleep(0.004)
                yield t

        def make(w):
            def fn(item, take_next):
                time.sleep(0.001)
                nxt = take_next()
                if calls_idle:
                    take_next.idle()
                me = threading.get_ident()

                def finish():
                    assert threading.get_ident() == me                 # the lane's own thread
                    with lock:
                        log.append(("finish", item, nxt))
                    return item * 10
                return lanes_mod.Deferred(finish)
            return fn

        outs = list(lanes_mod.run_ordered(src(30), [make(0), make(1)], prefetch=True))
        assert outs == [t * 10 for t in range(30)], (slow_source, calls_idle)
        assert sorted(x[1] for x in log) == list(range(30))
        if slow_source:
            assert any(x[2] is None for x in log)                      # finished at once: no next item was in hand

    # a failing finish() surfaces in the consumer like any worker error
    def bad(item, take_next):
        take_next()
        def finish():
            raise RuntimeError("boom")
        return lanes_mod.Deferred(finish)
    with pytest.raises(RuntimeError, match="boom"):
        list(lanes_mod.run_ordered(iter(range(5)), [bad, bad], prefetch=True))

    # abandoning the generator with deferred results pending does not hang
    g = lanes_mod.run_ordered(itertools.count(), [make(0), make(1)], prefetch=True)
    assert next(g) == 0
    g.close()


def test_run_ordered_prefetch_hands_every_item_to_exactly_one_worker_in_order():
    """prefetch mode (FaceService.process_stream: the next batch's upload overlaps the running one): a worker may claim
    its NEXT item while it works; every item is processed once, by the worker that claimed it, results stay in
    submission order, the look-ahead bound holds, an abandoned stream ends"""
    import itertools
    import threading
    import time
    from frp_amd import lanes as lanes_mod
    seen, staged_hits, lock = [], [0], threading.Lock()

    def make(wid):
        staged = {}

        def fn(item, take_next):
            t = int(item[0])
            if staged.pop("t", None) == t:
                with lock:
                    staged_hits[0] += 1
            time.sleep(0.002 if t % 3 else 0.01)
            nxt = take_next()
            assert take_next() is nxt or nxt is None                       # a second call returns the same claim
            if nxt is not None:
                staged["t"] = int(nxt[0])
            with lock:
                seen.append((t, wid))
            return t * 10
        return fn

    pulled = []

    def src(n):
        for t in range(n):
            pulled.append(t)
            yield np.array([t])
    got = []
    for out in lanes_mod.run_ordered(src(40), [make(0), make(1)], prefetch=True):
        got.append(out)
        assert len(pulled) - len(got) <= 5       # 2 x workers ahead of what the consumer has been HANDED (this item: not appended yet when the feeder pulled)
    assert got == [t * 10 for t in range(40)]
    assert sorted(t for t, _ in seen) == list(range(40)) and len({w for _, w in seen}) == 2
    assert staged_hits[0] >= 20                                            # most items arrived at their worker already staged
    g = lanes_mod.run_ordered((np.array([t]) for t in itertools.count()), [make(0), make(1)], prefetch=True)
    assert next(g) == 0
    time.sleep(0.1)
    th = threading.Thread(target=g.close, daemon=True)
    th.start()
    th.join(10)
    assert not th.is_alive()


def test_run_ordered_slow_source_never_blocks_a_worker_or_its_locks():
    """a LIVE source (a camera that sleeps for its fps limit and blocks in read: mixer.StreamMixer) is read by the
    pipeline's feeder thread: take_next() returns at once whether or not the next batch exists, so a worker that calls it
    while holding a lock (process_stream holds the gallery's shared lock there) never parks that lock on the source, a
    batch's result is delivered before the source has produced the next one, and a source that takes an exclusive lock
    of the caller's (a generator that enrols an identity) cannot deadlock against the workers' shared sections"""
    import threading
    import time
    from frp_amd import lanes as lanes_mod
    from frp_amd.gallery import Gallery
    eng_ = FakeEngine()
    G = Gallery(lambda: eng_)
    waits, produced_at, delivered_at = [], {}, {}

    def src(n):
        for t in range(n):
            time.sleep(0.15)                                   # fps limit / cap.read
            with G.locked():                                   # the source enrols someone: exclusive gallery section
                G.put(f"seen{t}", np.full(512, float(t + 1), np.float32))
            produced_at[t] = time.perf_counter()
            yield np.array([t])

    def make():
        def fn(item, take_next):
            with G.reading():                                  # process_stream's guard around process + take_next + fetch
                t0 = time.perf_counter()
                take_next()
                waits.append(time.perf_counter() - t0)
                time.sleep(0.01)                               # the device pass
            return int(item[0])
        return fn

    def run():
        for out in lanes_mod.run_ordered(src(6), [make(), make()], prefetch=True):
            delivered_at[out] = time.perf_counter()
    th = threading.Thread(target=run, daemon=True)
    th.start()
    th.join(20)
    assert not th.is_alive(), "slow source + gallery writer deadlocked against the lanes' shared sections"
    assert sorted(delivered_at) == list(range(6)) and len(G) == 6
    assert max(waits) < 0.05, waits                            # never waited for the source (it sleeps 0.15 s per item)
    for t in range(5):                                         # batch t is out before batch t + 1 even exists
        assert delivered_at[t] < produced_at[t + 1], (t, delivered_at[t], produced_at[t + 1])


def test_gallery_rw_lock_and_mirrors():
    """Gallery host logic for two lanes: updates reach every mirror, mirrors only join an empty gallery, shared readers
    run together while a writer waits for them and keeps later readers out"""
    import threading
    import time
    from frp_amd.gallery import Gallery
    a, b = FakeEngine(), FakeEngine()
    G = Gallery(lambda: a)
    G.add_mirror(b)
    rng = np.random.default_rng(3)
    E = rng.standard_normal((5, 512)).astype(np.float32)
    for i in range(4):
        G.put(f"p{i}", E[i])
    G.remove("p1")                                   # swap-remove on both copies
    G.put("p0", E[4])                                # overwrite on both copies
    assert np.array_equal(a.G, b.G) and len(a.G) == 3 and G.names() == ["p0", "p2", "p3"]
    G.set_bulk(["x", "y"], E[:2])
    assert np.array_equal(a.G, b.G) and len(b.G) == 2
    with pytest.raises(ValueError):
        G.add_mirror(FakeEngine())                   # not into a filled gallery
    G.clear()
    assert len(a.G) == len(b.G) == 0

    log = []
    inside = threading.Barrier(2, timeout=5)

    def reader(tag):
        with G.reading():
            inside.wait()                            # both readers are inside together
            log.append(("r-in", tag))
            time.sleep(0.05)
            log.append(("r-out", tag))

    def writer():
        with G.locked():
            with G.locked():                         # re-entrant
                with G.reading():                    # and may read inside its own exclusive section
                    log.append(("w", 0))
    r = [threading.Thread(target=reader, args=(i,)) for i in range(2)]
    for t in r:
        t.start()
    time.sleep(0.01)
    w = threading.Thread(target=writer)
    w.start()
    time.sleep(0.01)
    late = threading.Thread(target=lambda: (G.reading().__enter__(), log.append(("late", 0)), G._lock.release_read()))
    late.start()
    for t in r + [w, late]:
        t.join(timeout=5)
        assert not t.is_alive()
    order = [e[0] for e in log]
    assert order.index("w") > max(i for i, e in enumerate(order) if e == "r-out")      # the writer waited for both readers
    assert order.index("late") > order.index("w")                                      # and went before the late reader


def test_process_stream_two_lanes_host_logic():
    """FaceService.process_stream with two (fake) engines: results in submission order, equal to process_frames batch by
    batch, both engines used, enrolment during the stream reaches both gallery copies"""
    import time
    a, b = FakeEngine(), FakeEngine()
    svc = FaceService(engine=a, second_engine=b)
    rng = np.random.default_rng(11)
    E = rng.standard_normal((6, 512)).astype(np.float32)
    for i in range(4):
        assert svc.store_face(f"id{i}", E[i].tolist())["success"]
    assert np.array_equal(a.G, b.G)
    used = []

    def canned_for(eng, tag):
        def pf(frames, max_faces=10, det_thresh=0.5, nms_iou=0.4, flags=0):
            t = int(frames[0, 0, 0, 0])
            used.append(tag)
            time.sleep(0.02 if t % 2 == 0 else 0.001)
            q = E[t % 4][None]
            idx, cos = eng.match(q)
            return {"counts": np.array([1]), "boxes": np.zeros((1, 1, 4), np.float32) + t, "kps": np.zeros((1, 1, 10), np.float32),
                    "scores": np.ones((1, 1), np.float32), "emb": q[None].astype(np.float32),
                    "match_idx": np.array([[idx[0]]], np.int32), "match_cos": np.array([[cos[0]]], np.float32)}
        return pf
    a.process_frames = canned_for(a, "a")
    b.process_frames = canned_for(b, "b")
    batches = [np.full((1, 4, 4, 3), t, np.uint8) for t in range(10)]
    got = list(svc.process_stream(batches, max_faces=1))
    assert [g[0][0]["bbox"][0] for g in got] == list(range(10))                      # submission order
    assert [g[0][0]["target"] for g in got] == [f"id{t % 4}" for t in range(10)]
    assert set(used) == {"a", "b"}
    want = [svc.process_frames(f, max_faces=1) for f in batches]
    for g, w_ in zip(got, want):
        assert g[0][0]["target"] == w_[0][0]["target"] and g[0][0]["distance"] == w_[0][0]["distance"]
    # enrol while a stream is running: both copies get the row, later batches can match it
    gen = svc.process_stream(batches, max_faces=1)
    next(gen)
    assert svc.store_face("late", E[5].tolist())["success"]
    list(gen)
    assert np.array_equal(a.G, b.G) and len(a.G) == 5
    # a service whose gallery was filled before the second lane could join streams on one lane
    solo = FaceService(engine=FakeEngine())
    solo._eng().process_frames = canned_for(solo._eng(), "solo")
    assert solo.store_face("id0", E[0].tolist())["success"]
    assert len(list(solo.process_stream(batches[:3], max_faces=1))) == 3


def test_native_allgather_helper_hands_every_rank_its_own_rows(monkeypatch):
    """dist.native_allgather_gallery (the library-owned RCCL collective: include/frp.h frp_dist_* / frp_gallery_allgather), host side,
    against recording engines: rank 0 mints the id and every rank gets it through the control channel, each rank builds exactly
    rows shard_range(N, r, R) - contiguous ceil(N / R) blocks, the last ranks short or empty -, the first lane gathers and the
    other lanes of the GPU copy its snapshot.  (The collective itself: tests/test_gpu_service.py, one rank; bench.py --gpus N.)"""
    from frp_amd import dist as fdist, native

    class Rec:
        def __init__(self):
            self.calls = []
            self._dist = None

        def dist_init(self, uid, rank, world):
            self.calls.append(("init", uid, rank, world))
            self._dist = (rank, world)

        def gallery_allgather(self, rows, n_total):
            self.calls.append(("gather", rows.copy(), n_total))

        def gallery_device_ptr(self):
            return 0xABC0

        def gallery_set_device(self, ptr, n):
            self.calls.append(("copy", ptr, n))

    monkeypatch.setattr(native.Engine, "dist_unique_id", staticmethod(lambda: b"\x07" * 128))
    N, R = 1001, 4
    table = np.arange(N * 512, dtype=np.float32).reshape(N, 512)
    shared = {}

    def channel(payload):
        if payload is not None:
            shared["id"] = payload
        return shared["id"]
    seen = []
    for rank in range(R):
        lanes = [Rec(), Rec()]
        n = fdist.native_allgather_gallery(lanes, N, lambda first, cnt: table[first:first + cnt], rank, R, channel)
        assert n == N
        kind, uid, r_, w_ = lanes[0].calls[0]
        assert (kind, uid, r_, w_) == ("init", b"\x07" * 128, rank, R)
        kind, rows, n_total = lanes[0].calls[1]
        first, cnt = fdist.shard_range(N, rank, R)
        assert kind == "gather" and n_total == N and rows.shape == (cnt, 512) and np.array_equal(rows, table[first:first + cnt])
        assert lanes[1].calls == [("copy", 0xABC0, N)]
        seen.append((first, cnt))
        # a second gather on the same engines reuses the communicator
        fdist.native_allgather_gallery(lanes, N, lambda first, cnt: table[first:first + cnt], rank, R, channel)
        assert [c[0] for c in lanes[0].calls] == ["init", "gather", "gather"]
    assert seen == [(0, 251), (251, 251), (502, 251), (753, 248)]
