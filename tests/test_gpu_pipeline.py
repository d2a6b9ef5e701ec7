"""GPU end-to-end parity of detect -> align -> embed -> match against the fp32 oracle."""
import os

import numpy as np
import pytest

import align_model
from conftest import get_raw_and_blob
from oracle import network as onet

pytestmark = pytest.mark.gpu


def _frames(rng, B, H, W):
    base = rng.normal(110, 12, size=(B, H, W, 3))
    yy, xx = np.mgrid[0:H, 0:W]
    for b in range(B):
        for _ in range(3):
            cx, cy, r = rng.uniform(30, W - 30), rng.uniform(30, H - 30), rng.uniform(15, 40)
            m = ((xx - cx) / r) ** 2 + ((yy - cy) / (1.3 * r)) ** 2 < 1
            base[b][m] += rng.uniform(30, 80)
    return np.clip(base, 0, 255).astype(np.uint8)


def _threshold_with_margin(raw, frames, canvas, lo_cnt=3, hi_cnt=12):
    """Pick a score threshold in the widest logit gap (over all frames) that leaves between
    lo_cnt and hi_cnt candidates per frame, so the candidate set is stable under the
    fp16-vs-fp32 deviation of the head maps."""
    maps = onet.det_forward(raw, onet.det_blob(frames, canvas))
    per = [np.concatenate([m[b][..., [0, 15]].reshape(-1) for m in maps]) for b in range(frames.shape[0])]
    allv = np.sort(np.concatenate(per))[::-1][: 40 * len(per)]
    best = None
    for hi, lo in zip(allv[:-1], allv[1:]):
        t = 0.5 * (hi + lo)
        cnts = [int((p >= t).sum()) for p in per]
        if min(cnts) >= lo_cnt and max(cnts) <= hi_cnt and (best is None or hi - lo > best[0]):
            best = (hi - lo, t)
    assert best is not None and best[0] > 0.02, "no stable threshold for these seeds"
    return 1.0 / (1.0 + np.exp(-best[1])), maps


def test_process_frames_end_to_end(engine):
    rng = np.random.default_rng(123)
    raw, blob = get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))
    engine.load_weights(blob)
    B, H, W = 2, 192, 256
    frames = _frames(rng, B, H, W)
    K = 10
    G = rng.standard_normal((500, 512)).astype(np.float32)
    G /= np.linalg.norm(G, axis=1, keepdims=True)
    total = 0
    for b in range(B):      # one threshold per frame (synthetic weights: score statistics differ per frame)
        fr = frames[b:b + 1]
        thr, _ = _threshold_with_margin(raw, fr, (H, W))
        r = onet.process_frames(raw, fr, None, (H, W), score_thresh=thr, nms_iou=0.4, max_faces=K)[0]
        n = len(r["boxes"])
        assert n >= 2
        # gallery: the oracle's embeddings of its own faces planted among distractors
        slots = rng.choice(500, size=n, replace=False)
        Gb = G.copy()
        Gb[slots] = r["emb"]
        engine.gallery_set(Gb)
        out = engine.process_frames(fr, max_faces=K, det_thresh=float(thr), nms_iou=0.4)
        assert out["counts"][0] == n
        # same faces in the same order, boxes/landmarks within 0.5 px
        assert np.abs(out["boxes"][0, :n] - r["boxes"]).max() < 0.5
        assert np.abs(out["kps"][0, :n] - r["kps"]).max() < 0.5
        assert np.abs(out["scores"][0, :n] - r["scores"]).max() < 2e-3
        for k in range(n):
            cos = float((out["emb"][0, k] * r["emb"][k]).sum())
            assert cos > 1 - 1e-3, cos                          # north_star: within 1e-3 cosine
            assert out["match_idx"][0, k] == slots[k]           # identical top-1 identity
            assert abs(out["match_cos"][0, k] - 1.0) < 2e-3
        assert np.all(out["match_idx"][0, n:] == -1) and np.all(out["emb"][0, n:] == 0)
        total += n
    assert total >= 4


def test_full_size_end_to_end_1080p_r100_vs_oracle(engine):
    """The whole path at the headline size, not piecewise: ONE 1920 x 1080 frame through the full detector (1088 x 1920 canvas,
    85,680 anchors), threshold + NMS, 5-point alignment, IResNet-100 and a 3,000-row gallery, against the fp32 oracle's
    whole chain (`oracle/network.py: process_frames`) on the same frame and weights: same face count and order, boxes and
    landmarks within 0.5 px, scores 2e-3, embeddings cos >= 1 - 1e-3, identical top-1, match cosine 2e-3.  (A call of
    this size takes the direct kernels in quarter tiles for the embedder and the default tiles for the detector.)"""
    rng = np.random.default_rng(4242)
    raw, blob = get_raw_and_blob((1, 2, 2, 2), (3, 13, 30, 3))
    engine.load_weights(blob)
    H, W, K = 1080, 1920, 10
    fr = _frames(rng, 1, H, W)
    thr, _ = _threshold_with_margin(raw, fr, (1088, 1920), lo_cnt=2, hi_cnt=40)
    r = onet.process_frames(raw, fr, None, (1088, 1920), score_thresh=thr, nms_iou=0.4, max_faces=K)[0]
    n = len(r["boxes"])
    assert 2 <= n <= K
    G = rng.standard_normal((3000, 512)).astype(np.float32)
    G /= np.linalg.norm(G, axis=1, keepdims=True)
    slots = rng.choice(3000, size=n, replace=False)
    G[slots] = r["emb"]
    engine.gallery_set(G)
    out = engine.process_frames(fr, max_faces=K, det_thresh=float(thr), nms_iou=0.4)
    assert out["counts"][0] == n
    assert np.abs(out["boxes"][0, :n] - r["boxes"]).max() < 0.5
    assert np.abs(out["kps"][0, :n] - r["kps"]).max() < 0.5
    assert np.abs(out["scores"][0, :n] - r["scores"]).max() < 2e-3
    cos = (out["emb"][0, :n] * r["emb"]).sum(1)
    assert cos.min() > 1 - 1e-3, cos
    assert np.array_equal(out["match_idx"][0, :n], slots)
    assert np.abs(out["match_cos"][0, :n] - 1.0).max() < 2e-3
    print("full-size end to end:", n, "faces, 1 - cos max", float(1 - cos.min()), "box err", float(np.abs(out["boxes"][0, :n] - r["boxes"]).max()))


def _head_blame(g32, r32, bound):
    """where a head map leaves its reference: count over the bound, the worst element and the 8 x 30 tile / wave pair of the
    Winograd kernel's 2-D tiles it would belong to (one record must convict)"""
    d = np.abs(g32 - r32)
    n, y, x, c = np.unravel_index(int(d.argmax()), d.shape)
    return (f"{int((d > bound).sum())} elements over the bound {bound:.4f}; worst {float(d.max()):.4f} at image {n}, y {y}, x {x}, channel {c} "
            f"(8 x 30 tile row {y // 8}, column {x // 30}; row {y % 8} of the tile: waves {2 * ((y % 8) // 2)} / {2 * ((y % 8) // 2) + 1})")


def _emulated_heads(raw, frames):
    """the detector PROGRAM (folded fp16 weights, fp16 storage between layers, fp32 accumulation) on the CPU, one frame at a time"""
    from frp_amd import netspec as ns
    from test_gpu_kernels import _emulate_program_fp16
    B, H, W, _ = frames.shape
    Hc, Wc = (H + 31) // 32 * 32, (W + 31) // 32 * 32
    outs = None
    for b in range(B):
        x = np.zeros((1, Hc, Wc, 8), np.float16)
        x[0, :H, :W, :3] = ((frames[b, :, :, ::-1].astype(np.float32) - 127.5) / 128.0).astype(np.float16)     # exact in fp16
        x[0, H:, :, :3] = np.float16(-127.5 / 128.0)                                                           # letterbox: u8 zero
        x[0, :H, W:, :3] = np.float16(-127.5 / 128.0)
        emu = _emulate_program_fp16(raw, ns.detector_layers((1, 2, 2, 2)), x, ["det.out3", "det.out4", "det.out5"])
        outs = [[e] for e in emu] if outs is None else [o + [e] for o, e in zip(outs, emu)]
    return [np.concatenate(o, 0).astype(np.float32) for o in outs]


@pytest.mark.parametrize("B,unique,with_oracle", [(4, 4, True), (32, 8, False)])
def test_detector_families_vs_fp16_emulation_and_oracle_at_1080p(fresh_engine, monkeypatch, B, unique, with_oracle):
    """Both kernel families of the detector at camera size, EACH against references that do not depend on the other: the fp32
    emulation of the fp16 program (direct family <= 4 fp16 ulps of a map's scale - the bar of the small-image test -, Winograd
    family <= 6: its packed-fp16 input transform rounds once more per layer; mean <= 1/4 ulp) and, at four frames, the fp32
    oracle (2e-2 of the scale: the fp16-vs-fp32 budget of the head maps).  From four 1080p frames per call on the default
    program runs the Winograd kernel's 2-D tiles on the 136 x 240 x 128 layers, from eight on also on the 68 x 120 x 256 ones
    (frp_api.cpp: det_wino, conv3x3_wino.hip: wino_2d_pays): B = 4 and B = 32 (eight distinct frames, each four times: the
    bench's launch geometry) cover both.  A failure names the family, the element and its tile (round 4's verdict: the
    cross-family comparison could say neither which side was wrong nor where)."""
    engine = fresh_engine
    rng = np.random.default_rng(77)
    raw, blob = get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))
    uniq = _frames(rng, unique, 1080, 1920)
    fr = np.concatenate([uniq] * (B // unique), 0)
    emu = _emulated_heads(raw, uniq)
    ref = onet.det_forward(raw, onet.det_blob(uniq, (1088, 1920))) if with_oracle else None
    maps = {}
    for family, env, ulps in (("direct", "1", 4), ("winograd 2-D tiles", None, 6)):
        if env:
            monkeypatch.setenv("FRP_NO_WINO", env)
        else:
            monkeypatch.delenv("FRP_NO_WINO", raising=False)
        engine.load_weights(blob)
        engine.reset_counters()
        engine.detect(fr, max_faces=4, det_thresh=0.5)
        heads = [h.astype(np.float32) for h in engine.head_maps()]
        maps[family] = heads
        for lv, g in enumerate(heads):
            for rep in range(B // unique):                       # every slot of the batch against the emulation of its frame
                gs = g[rep * unique:(rep + 1) * unique]
                e = emu[lv]
                scale = max(1.0, float(np.abs(e).max()))
                bound = ulps * 2.0 ** -10 * scale
                assert np.abs(gs - e).max() <= bound, f"{family}, stride {8 << lv}, slots {rep * unique}..: vs the fp16 emulation: " + _head_blame(gs, e, bound)
                assert np.abs(gs - e).mean() <= 2.0 ** -12 * scale, (family, lv)
                if ref is not None:
                    r = ref[lv]
                    rs = max(1.0, float(np.abs(r).max()))
                    assert np.abs(gs[..., :30] - r).max() < 2e-2 * rs, f"{family}, stride {8 << lv}: vs the oracle: " + _head_blame(gs[..., :30], r, 2e-2 * rs)
        print(f"[{family}] B={B}: max deviation from the fp16 emulation (ulps of the scale, per stride):",
              [round(float(np.abs(g[:unique] - e).max() / (2.0 ** -10 * max(1.0, float(np.abs(e).max())))), 2) for g, e in zip(heads, emu)])
    # the other family did run: not the same bits
    assert any(not np.array_equal(a, b) for a, b in zip(maps["direct"], maps["winograd 2-D tiles"]))


@pytest.mark.parametrize("family,passes", [("direct", 1500), ("winograd", 800)])
def test_detector_pass_is_bit_reproducible(fresh_engine, monkeypatch, family, passes):
    """The same four resident 1080p frames through the whole detector `passes` times: every op's output (a 64-bit hash taken right
    behind the op, frp_debug_det_hashes) and the head maps repeat bit for bit.  Round 5: the fused stem kernel zero-filled its LDS
    patch without a barrier in front of the first tile's staging - one tile of a workgroup's first ones off by a few per cent once
    in ~350 passes, inside every tolerance against the oracle; it surfaced as round 4's red cross-family comparison."""
    engine = fresh_engine
    if family == "direct":
        monkeypatch.setenv("FRP_NO_WINO", "1")
    else:
        monkeypatch.delenv("FRP_NO_WINO", raising=False)
    rng = np.random.default_rng(77)
    raw, blob = get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))
    fr = _frames(rng, 4, 1080, 1920)
    engine.load_weights(blob)
    engine.upload_frames(fr)
    engine.det_hashes(True, fetch=False)
    try:
        engine.detect_resident((1080, 1920), max_faces=8, det_thresh=0.5)
        first = engine.det_hashes()
        heads = [h.copy() for h in engine.head_maps()]
        assert len(set(first[1:34].tolist())) == 33                     # (34 ops, the fused stems share slot 1: every slot was written)
        for r in range(passes):
            engine.detect_resident((1080, 1920), max_faces=8, det_thresh=0.5)
            got = engine.det_hashes()
            diff = [i + 1 for i in range(64) if first[i] != got[i]]
            assert not diff, f"{family}: pass {r}: the outputs of ops {diff} differ from the first pass (first: op {diff[0]})"
        for a, b in zip(heads, engine.head_maps()):
            assert np.array_equal(a.view(np.uint16), b.view(np.uint16))
    finally:
        engine.det_hashes(False, fetch=False)


@pytest.mark.selfcheck
def test_detector_on_winograd_2d_tiles_agrees_with_the_direct_family_at_1080p(fresh_engine, monkeypatch):
    """From four 1080p frames per call on, the detector's wide 128 / 256-channel 3x3 layers take the Winograd kernel's 2-D tiles
    (frp_api.cpp: det_wino; conv3x3_wino.hip: wino_2d_pays).  The same four frames with FRP_NO_WINO=1 (direct family, the one the
    oracle test above pins) give: head maps within 6 fp16 ulps of their scale (and NOT the same bits: the other family did
    run), the same detections in the same order, boxes / landmarks within 0.25 px (half the bar against the oracle), scores 2e-3, embeddings of the (slightly differently) aligned chips cos >= 0.98;
    one frame alone (direct family either way) is bit for bit its slot of the FRP_NO_WINO batch."""
    engine = fresh_engine
    rng = np.random.default_rng(77)
    raw, blob = get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))
    H, W, K = 1080, 1920, 16
    fr = _frames(rng, 4, H, W)
    G = rng.standard_normal((2000, 512)).astype(np.float32)
    thr, _ = _threshold_with_margin(raw, fr, (1088, 1920), lo_cnt=1, hi_cnt=60)       # a logit gap over all four frames
    monkeypatch.setenv("FRP_NO_WINO", "1")
    engine.load_weights(blob)
    engine.gallery_set(G)
    a = engine.process_frames(fr, max_faces=K, det_thresh=float(thr), nms_iou=0.4)
    ha = [h.astype(np.float32) for h in engine.head_maps()]
    one = engine.process_frames(fr[2:3], max_faces=K, det_thresh=float(thr), nms_iou=0.4)
    monkeypatch.delenv("FRP_NO_WINO")
    engine.load_weights(blob)
    engine.gallery_set(G)
    b = engine.process_frames(fr, max_faces=K, det_thresh=float(thr), nms_iou=0.4)
    hb = [h.astype(np.float32) for h in engine.head_maps()]
    one_b = engine.process_frames(fr[2:3], max_faces=K, det_thresh=float(thr), nms_iou=0.4)
    differs = False
    for x, y in zip(ha, hb):
        scale = max(1.0, float(np.abs(x).max()))
        assert np.abs(x - y).max() <= 6 * 2.0 ** -10 * scale, "direct vs Winograd family: " + _head_blame(y, x, 6 * 2.0 ** -10 * scale)
        differs = differs or not np.array_equal(x, y)
    assert differs
    assert np.array_equal(a["counts"], b["counts"]) and int(a["counts"].sum()) >= 4
    for i, n in enumerate(a["counts"]):
        if not n:
            continue
        # the same faces; their order (descending score) may differ where two scores are closer than the families' 1e-3
        d = np.abs(a["boxes"][i, :n, None, :] - b["boxes"][i, None, :n, :]).max(-1)
        j = d.argmin(1)
        assert sorted(j.tolist()) == list(range(n)), (i, j)
        assert d[np.arange(n), j].max() < 0.25                              # (an fp16 ulp of a stride-32 offset is 0.06 px)
        assert np.abs(a["kps"][i, :n] - b["kps"][i, j]).max() < 0.25
        assert np.abs(a["scores"][i, :n] - b["scores"][i, j]).max() < 2e-3
        # (downstream of landmarks that moved by up to 0.1 px: a seeded random embedder on noise-like chips is far more sensitive to
        # that than a trained one on faces)
        assert (a["emb"][i, :n] * b["emb"][i, j]).sum(1).min() > 0.98
    for k in ("boxes", "kps", "scores", "counts", "emb", "match_idx"):
        assert np.array_equal(one[k][0], a[k][2]), k                        # a frame's result in the direct family: independent of the batch
        assert np.array_equal(one[k], one_b[k]), k                          # and a call of one frame never takes the 2-D tiles


def test_threshold_mode_face_count_stays_on_the_device(engine, monkeypatch):
    """Threshold mode (routes/camera.py:232-259: the reference's loop) without the mid-pipeline host round trip: align,
    embedder, l2norm and matcher read the face count from device memory.  Bit for bit the results of the former path
    (FRP_HOST_COUNT=1: copy the count, wait, launch for exactly n), on the small net and on IResNet-100, with ragged
    counts, frames without faces, a batch without any face, and a batch whose slots exceed the top-1 matcher's 512
    (falls back to the host count); the counters see the real face count and FLOPs."""
    rng = np.random.default_rng(314)
    G = rng.standard_normal((3000, 512)).astype(np.float32)
    ragged = False
    for emb_blocks, B, H, W, K in (((1, 1, 1, 1), 5, 128, 160, 6), ((3, 13, 30, 3), 3, 160, 192, 10)):
        raw, blob = get_raw_and_blob((1, 2, 2, 2), emb_blocks)
        engine.load_weights(blob)
        engine.gallery_set(G)
        frames = _frames(rng, B, H, W)
        frames[1] = 0                                                     # a frame without structure
        for thr in (0.5, 0.3, 0.9, 1.0):
            monkeypatch.setenv("FRP_HOST_COUNT", "1")
            want = engine.process_frames(frames, max_faces=K, det_thresh=thr)
            monkeypatch.delenv("FRP_HOST_COUNT")
            engine.reset_counters()
            got = engine.process_frames(frames, max_faces=K, det_thresh=thr)
            ctr = engine.counters()
            for key in ("counts", "boxes", "kps", "scores", "emb", "match_idx", "match_cos"):
                assert np.array_equal(got[key], want[key]), (emb_blocks, thr, key)
            n = int(got["counts"].sum())
            ragged |= int(want["counts"].max()) > int(want["counts"].min())
            assert ctr["faces"] == n
            if thr == 1.0:
                assert n == 0 and abs(ctr["emb_conv_flops"]) < 1.0
            # resident form: the count is resolved by fetch_results
            engine.upload_frames(frames)
            engine.process_resident(max_faces=K, det_thresh=thr)
            res = engine.fetch_results()
            for key in ("counts", "emb", "match_idx", "match_cos"):
                assert np.array_equal(res[key], want[key]), key
    assert ragged                                                         # some batch had a ragged face count
    # > 512 slots: host-count fallback, same results either way
    raw, blob = get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))
    engine.load_weights(blob)
    frames = _frames(rng, 9, 96, 128)
    a = engine.process_frames(frames, max_faces=64, det_thresh=0.3)
    monkeypatch.setenv("FRP_HOST_COUNT", "1")
    b = engine.process_frames(frames, max_faces=64, det_thresh=0.3)
    for key in ("counts", "emb", "match_idx"):
        assert np.array_equal(a[key], b[key])


def _small_resident_batch(eng):
    """The small nets, a gallery of 300 random rows and B = 3 resident frames of 128 x 160 for K = 6 (18 slots: a threshold pass
    keeps its face count on the device).  Seed 93 was chosen with oracle/network.py on the CPU: its decode_nms keeps 6 + 6 + 6 faces
    at 0.3 - every frame has over 60 candidates - and 0 + 6 + 6 at 0.5, where frame 0 has no candidate at all."""
    rng = np.random.default_rng(93)
    frames = _frames(rng, 3, 128, 160)
    _, blob = get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))
    eng.load_weights(blob)
    eng.gallery_set(rng.standard_normal((300, 512)).astype(np.float32))
    eng.upload_frames(frames)
    return 6


_RESULT_KEYS = ("counts", "boxes", "kps", "scores", "emb", "match_idx", "match_cos")


def _lone_threshold_pass(eng, K, thr):
    """one fetched threshold pass on the resident frames -> (results, faces, embedder FLOPs) by the counters"""
    eng.reset_counters()
    eng.process_resident(max_faces=K, det_thresh=thr)
    res = eng.fetch_results()
    ctr = eng.counters()
    assert ctr["faces"] == int(res["counts"].sum())
    return res, ctr["faces"], ctr["emb_conv_flops"]


def test_queued_threshold_passes_settle_each_other(engine):
    """Two threshold passes queued with nothing between them: the second settles the first one's face count, which is still on
    the device, before it reuses the count's slots.  The fetch gives the second pass alone, the counters hold both."""
    K = _small_resident_batch(engine)
    _, n3, f3 = _lone_threshold_pass(engine, K, 0.3)
    want, n5, f5 = _lone_threshold_pass(engine, K, 0.5)
    assert n3 != n5 and n3 + n5 > 0
    engine.reset_counters()
    engine.process_resident(max_faces=K, det_thresh=0.3)
    engine.process_resident(max_faces=K, det_thresh=0.5)
    got = engine.fetch_results()
    for key in _RESULT_KEYS:
        assert np.array_equal(got[key], want[key]), key
    ctr = engine.counters()
    assert ctr["faces"] == n3 + n5
    assert abs(ctr["emb_conv_flops"] - (f3 + f5)) <= 1e-9 * (f3 + f5)      # (the same double arithmetic in another order)


def test_overflowed_hit_list_is_not_rebuilt_from_replaced_queries(fresh_engine):
    """A hit list that overflowed is rebuilt at fetch time from the queries the pass left on the device: refused once a later
    match has replaced them, equal to the top-k of the fetched embeddings otherwise.  Rows and hit counts equal match(emb, topk).
    The cosines are compared bit for bit with the matcher's score rows of the pass's own queries: the l2norm stores a unit
    embedding e as fp32 and fp16(e) as the query, so emb.astype(float16) is that query, match_f16 takes it without normalising, and
    a host top-k by (cosine desc, row asc) over its score matrix is the list.  (match() divides the fetched e by |e| = 1 +- a few
    ulps first, which moves single fp16 roundings: its cosines agree only to about 1e-7.)"""
    from frp_amd import native
    engine = fresh_engine
    K, cap = _small_resident_batch(engine), 4
    engine.set_within(-2.0, cap)                                            # every gallery row is a hit: every face overflows
    flags = native.FLAG_FORCED_K | native.FLAG_WITHIN
    engine.process_resident(max_faces=K, flags=flags)
    emb = engine.fetch_results()["emb"]
    engine.match(emb[0, :1])
    with pytest.raises(native.FrpError, match="replaced the pass's embeddings"):
        engine.fetch_within()
    engine.process_resident(max_faces=K, flags=flags)                       # a new pass after the refusal fetches normally
    idx, cos, n = engine.fetch_within()
    emb = engine.fetch_results()["emb"].reshape(-1, 512)
    idx, cos = idx.reshape(-1, cap), cos.reshape(-1, cap)
    assert np.all(n == 300)
    assert np.array_equal(idx, engine.match(emb, topk=cap)[0])
    S = engine.match_f16(emb.astype(np.float16), scores=True)[2]
    want_idx = np.stack([np.lexsort((np.arange(300), -row))[:cap] for row in S]).astype(np.int32)
    assert np.array_equal(idx, want_idx)
    assert np.array_equal(cos.view(np.uint32), np.take_along_axis(S, want_idx, axis=1).view(np.uint32))
    # a detect-only call begins a pass of its own: it has no lists, whatever the pass before it was flagged with
    engine.detect_resident((128, 160), max_faces=K)
    with pytest.raises(native.FrpError, match="without FRP_FLAG_WITHIN"):
        engine.fetch_within()


@pytest.mark.parametrize("thr", [0.3, 0.5])
def test_discarded_pending_pass_still_reaches_the_counters(engine, thr):
    """A threshold pass that is queued and never fetched, then discarded by a detect-only call: its faces and the FLOPs of its real
    face count reach the counters all the same.  (Before the pending count was settled by every entry point that discards a pass,
    this sequence showed faces == 0 and the embedder's FLOPs of the capacity B x K.)  At 0.3 every slot holds a face, so only the
    face count tells; at 0.5 frame 0 is empty and the FLOPs of 12 faces differ from those of the 18 slots."""
    K = _small_resident_batch(engine)
    _, n, f = _lone_threshold_pass(engine, K, thr)
    assert n > 0
    engine.reset_counters()
    engine.process_resident(max_faces=K, det_thresh=thr)
    engine.detect_resident((128, 160), max_faces=K)
    engine.synchronize()
    ctr = engine.counters()
    assert ctr["faces"] == n
    assert abs(ctr["emb_conv_flops"] - f) <= 1e-9 * f


def test_forced_k_and_resident_path(engine):
    rng = np.random.default_rng(77)
    raw, blob = get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))
    engine.load_weights(blob)
    B, H, W, K = 3, 128, 160, 4
    frames = _frames(rng, B, H, W)
    G = rng.standard_normal((300, 512)).astype(np.float32)
    engine.gallery_set(G)
    engine.upload_frames(frames)
    engine.process_resident(max_faces=K, flags=1)
    a = engine.fetch_results()
    assert np.all(a["counts"] == K)
    engine.process_resident(max_faces=K, flags=1)            # idempotent on resident frames
    b = engine.fetch_results()
    for key in ("boxes", "kps", "emb", "match_idx", "match_cos"):
        assert np.array_equal(a[key], b[key]), key
    c = engine.process_frames(frames, max_faces=K, flags=1)
    assert np.array_equal(a["emb"], c["emb"])
    assert np.abs(np.linalg.norm(a["emb"], axis=-1) - 1).max() < 1e-4
    # embeddings of the forced faces equal the stage API on the same landmarks
    e = engine.embed_faces(frames[1], a["kps"][1])
    assert np.abs(e - a["emb"][1]).max() < 1e-6
    # RGB flag == BGR input with channels swapped
    d = engine.process_frames(np.ascontiguousarray(frames[..., ::-1]), max_faces=K, flags=1 | 2)
    assert np.array_equal(a["emb"], d["emb"])


def test_two_batches_in_flight_equal_one_at_a_time(engine):
    """lanes.Lanes (two handles = two streams, one host thread each; batch t+1 runs while batch t is on the device):
    every batch gets bit for bit the result of a plain call on a single engine, in submission order, also with ragged
    batch shapes and in threshold mode; an error in the caller's iterator or in a lane surfaces in the consumer"""
    from frp_amd.lanes import Lanes
    rng = np.random.default_rng(909)
    raw, blob = get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))
    engine.load_weights(blob)
    G = rng.standard_normal((700, 512)).astype(np.float32)
    engine.gallery_set(G)
    lanes = Lanes(0, 2, max_batch=4, max_faces=4, max_h=160, max_w=192)
    lanes.load_weights(blob)
    lanes.gallery_set(G)
    shapes = [(3, 128, 160), (4, 160, 192), (1, 96, 128), (3, 128, 160), (2, 160, 192), (4, 128, 160), (1, 160, 192)]
    batches = [_frames(rng, *s_) for s_ in shapes]
    for flags, thr in ((1, 0.5), (0, 0.3)):
        want = [engine.process_frames(f, max_faces=4, det_thresh=thr, flags=flags) for f in batches]
        got = list(lanes.run(batches, max_faces=4, det_thresh=thr, flags=flags))
        assert len(got) == len(want)
        for g, w_ in zip(got, want):
            for key in ("counts", "boxes", "kps", "scores", "emb", "match_idx", "match_cos"):
                assert np.array_equal(g[key], w_[key]), key
    assert list(lanes.run([], max_faces=4)) == []

    def broken():
        yield batches[0]
        raise KeyError("camera gone")
    with pytest.raises(KeyError):
        list(lanes.run(broken(), max_faces=4, flags=1))
    with pytest.raises(ValueError):                                 # a lane's own failure (bad frame shape)
        list(lanes.run([batches[0], np.zeros((1, 8, 8, 4), np.uint8)], max_faces=4, flags=1))
    # an abandoned generator stops its workers
    gen = lanes.run(batches, max_faces=4, flags=1)
    next(gen)
    gen.close()
    lanes.close()


def test_overlapped_ingest_equals_plain_calls(engine):
    """upload_async(t+1) | process(t) | fetch(t) | swap: every batch gives exactly the results of a plain
    process_frames call, also when the batch shape changes and when the staged copy is still running
    at swap time (pinned source) or was a blocking copy (pageable source)."""
    rng = np.random.default_rng(99)
    raw, blob = get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))
    engine.load_weights(blob)
    engine.gallery_set(rng.standard_normal((200, 512)).astype(np.float32))
    K = 3
    shapes = [(4, 128, 160), (4, 128, 160), (2, 96, 224), (4, 128, 160), (1, 160, 128)]
    batches = [_frames(rng, *s) for s in shapes]
    want = [engine.process_frames(f, max_faces=K, flags=1) for f in batches]
    pinned = {}
    def staged(i):
        f = batches[i]
        if i % 2 == 0:                                   # even batches go through page-locked memory
            buf = pinned.setdefault(f.shape, engine.host_frames(*f.shape[:3]))
            buf[...] = f
            return buf
        return f
    engine.upload_frames_async(staged(0))
    engine.swap_frames()
    for i in range(len(batches)):
        if i + 1 < len(batches):
            engine.upload_frames_async(staged(i + 1))    # overlaps the processing of batch i
        engine.process_resident(max_faces=K, flags=1)
        got = engine.fetch_results()
        for key in ("boxes", "kps", "scores", "counts", "emb", "match_idx", "match_cos"):
            assert np.array_equal(got[key], want[i][key]), (i, key)
        if i + 1 < len(batches):
            engine.swap_frames()
    from frp_amd.native import FrpError
    with pytest.raises(FrpError):
        engine.swap_frames()                              # nothing staged


def test_mixed_ingest_kinds_back_to_back_equal_plain_calls(engine):
    """The overlapped loop of the test above with a different INGEST KIND for every consecutive batch - raw frames from page-locked
    and from pageable memory, JPEG stills with the entropy decode on host threads (no restart markers) and on the device (one
    interval per MCU) - so that every kind stages behind every other one on the same handle.  The sizes grow (3 x 96 x 160: every
    staging buffer is regrown while a pass is in flight) and shrink again (4 x 64 x 96: nothing grows, both page-locked JPEG turns
    are reused at a smaller size), and one batch is refused by the call (an image cut inside a restart interval) before a good batch
    of each JPEG kind.  Every accepted batch gives exactly the results of a plain process_frames call on the same pixels (for a JPEG
    batch: the PIL-decoded BGR frames), and the device-decode counter advances by exactly the accepted device-path batches."""
    import io
    from PIL import Image
    from frp_amd import native
    from frp_amd.native import FrpError
    assert os.environ.get("FRP_JPEG_DEVICE_HUFFMAN") == "1"
    rng = np.random.default_rng(77)
    raw, blob = get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))
    engine.load_weights(blob)
    engine.gallery_set(rng.standard_normal((200, 512)).astype(np.float32))
    K, flags = 3, native.FLAG_FORCED_K

    def stills(B, H, W, **kw):
        out = []
        for _ in range(B):
            img = np.clip(rng.normal(120, 55, (H // 8 + 1, W // 8 + 1, 3)).repeat(8, 0).repeat(8, 1)[:H, :W] + rng.normal(0, 7, (H, W, 3)), 0, 255)
            b = io.BytesIO()
            Image.fromarray(img.astype(np.uint8)).save(b, "JPEG", quality=88, subsampling=2, **kw)
            out.append(b.getvalue())
        return out

    def pil_bgr(jpegs):
        return np.stack([np.ascontiguousarray(np.array(Image.open(io.BytesIO(d)).convert("RGB"))[..., ::-1]) for d in jpegs])

    small, large = (4, 64, 96), (3, 96, 160)
    kinds = [("pinned", small), ("jpeg-host", small), ("jpeg-device", small), ("pageable", small), ("jpeg-device", small), ("jpeg-host", small),
             ("jpeg-device", large), ("jpeg-host", large), ("jpeg-device", small), ("jpeg-host", small),
             ("refused", small), ("jpeg-device", small), ("jpeg-host", small)]
    assert all(a[0] != b[0] for a, b in zip(kinds[:-1], kinds[1:]))
    batches = []                                        # (kind, what the upload call gets, the frames process_frames gets)
    for kind, shape in kinds:
        if kind in ("pinned", "pageable"):
            f = _frames(rng, *shape)
            batches.append((kind, f, f))
        elif kind == "refused":
            good = stills(*shape, restart_marker_blocks=1)
            d = good[2]
            sos = d.find(b"\xff\xda")
            rst = [i for i in range(sos, len(d) - 1) if d[i] == 0xFF and 0xD0 <= d[i + 1] <= 0xD7]
            assert len(rst) == 23                       # 24 MCUs, one interval each
            cut = d[:rst[3] + 2 + (rst[4] - rst[3]) // 2] + d[rst[4]:]          # half of interval 4 is missing
            batches.append((kind, good[:2] + [cut] + good[3:], None))
        else:
            j = stills(*shape, **(dict(restart_marker_blocks=1) if kind == "jpeg-device" else {}))
            assert native.jpeg_info(j[0])["restart_interval"] == (1 if kind == "jpeg-device" else 0)
            batches.append((kind, j, pil_bgr(j)))
    want = [None if f is None else engine.process_frames(f, max_faces=K, flags=flags) for _, _, f in batches]
    n0 = engine.jpeg_device_batches()
    pinned = engine.host_frames(*small)
    accepted_on_device = 0

    def upload(i):
        """stage batch i by its kind; the refused batch raises, leaves nothing staged, and the batch behind it goes in its place"""
        nonlocal accepted_on_device
        kind, src, _ = batches[i]
        if kind == "refused":
            with pytest.raises(FrpError, match="JPEG 2"):
                engine.upload_jpeg_async(src)
            return upload(i + 1)
        if kind == "pinned":
            pinned[...] = src
            engine.upload_frames_async(pinned)
        elif kind == "pageable":
            engine.upload_frames_async(src)
        else:
            engine.upload_jpeg_async(src)
            accepted_on_device += kind == "jpeg-device"
        assert engine.jpeg_device_batches() == n0 + accepted_on_device, (i, kind)
        return i

    cur = upload(0)
    engine.swap_frames()
    checked = 0
    while cur is not None:
        nxt = upload(cur + 1) if cur + 1 < len(batches) else None          # overlaps the processing of batch `cur`
        engine.process_resident(max_faces=K, flags=flags)
        got = engine.fetch_results()
        for key in ("boxes", "kps", "scores", "counts", "emb", "match_idx", "match_cos"):
            assert np.array_equal(got[key], want[cur][key]), (cur, batches[cur][0], key)
        checked += 1
        if nxt is not None:
            engine.swap_frames()
        cur = nxt
    assert checked == len(batches) - 1
    assert engine.jpeg_device_batches() == n0 + 5


def test_no_faces_and_no_gallery(engine):
    raw, blob = get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))
    engine.load_weights(blob)
    engine.gallery_set(np.zeros((0, 512), np.float32))
    frames = np.full((1, 96, 96, 3), 127, np.uint8)
    o = engine.process_frames(frames, max_faces=5, det_thresh=0.999999)
    assert o["counts"][0] == 0 and np.all(o["emb"] == 0) and np.all(o["match_idx"] == -1)
    o = engine.process_frames(frames, max_faces=5, flags=1)      # faces but empty gallery
    assert o["counts"][0] == 5 and np.all(o["match_idx"] == -1)


def test_full_size_properties_1080p_r100(engine):
    """BASELINE-sized run (32 x 1080p frames, full detector, IResNet-100, 100k gallery) checked
    through size-independent properties: exact face counts, unit embeddings, idempotence,
    frame-permutation equivariance, planted identities found at cosine ~1, tie-free top-1
    consistent with a float64 recomputation on a sample."""
    from frp_amd import native
    raw, blob = get_raw_and_blob((1, 2, 2, 2), (3, 13, 30, 3))
    engine.load_weights(blob)
    rng = np.random.default_rng(2025)
    B, H, W, K = 32, 1080, 1920, 10
    frames = rng.integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)
    G = rng.standard_normal((100_000, 512)).astype(np.float32)
    G /= np.linalg.norm(G, axis=1, keepdims=True)
    engine.gallery_set(G)
    a = engine.process_frames(frames, max_faces=K, flags=native.FLAG_FORCED_K)
    assert np.all(a["counts"] == K)
    assert np.abs(np.linalg.norm(a["emb"], axis=-1) - 1).max() < 1e-4
    assert np.all(np.diff(a["scores"], axis=1) <= 0)                      # detector order = score descending
    b = engine.process_frames(frames, max_faces=K, flags=native.FLAG_FORCED_K)
    for key in ("boxes", "kps", "scores", "emb", "match_idx", "match_cos"):
        assert np.array_equal(a[key], b[key]), key                          # idempotent / deterministic
    perm = rng.permutation(B)
    c = engine.process_frames(frames[perm], max_faces=K, flags=native.FLAG_FORCED_K)
    for key in ("boxes", "kps", "emb", "match_idx"):
        assert np.array_equal(a[key][perm], c[key]), key                    # frames never interact
    # top-1 against float64 on a sample of faces (fp16 gallery: allow only near-ties to differ)
    sample = a["emb"][::8, ::3].reshape(-1, 512).astype(np.float64)
    S = sample @ G.T.astype(np.float64)
    ref_idx = S.argmax(1)
    got_idx = a["match_idx"][::8, ::3].reshape(-1)
    got_cos = a["match_cos"][::8, ::3].reshape(-1)
    ref_cos = S.max(1)
    assert np.abs(got_cos - ref_cos).max() < 1e-3
    differ = got_idx != ref_idx
    assert np.all(np.abs(S[np.arange(len(S)), got_idx] - ref_cos)[differ] < 5e-4)
    # plant the produced embeddings as identities: every face must find itself
    rows = rng.choice(100_000, size=B * K, replace=False)
    G2 = G.copy()
    G2[rows] = a["emb"].reshape(-1, 512)
    engine.gallery_set(G2)
    d = engine.process_frames(frames, max_faces=K, flags=native.FLAG_FORCED_K)
    assert np.array_equal(d["match_idx"].reshape(-1), rows)
    assert d["match_cos"].min() > 0.999
    engine.gallery_set(np.zeros((0, 512), np.float32))


def test_headline_step_is_bit_reproducible(fresh_engine):
    """The bench's step - 32 resident 1080p frames, forced 10 faces per frame, IResNet-100, 100 k gallery - 150 times: boxes,
    landmarks, scores, all 320 embeddings, match ids and cosines repeat BIT FOR BIT, and so do the detector's per-op hashes.  Every
    kernel of the headline path takes part with the launch geometry the bench times (persistent grids, the 2-D Winograd tiles on
    the detector, the Winograd family on the embedder, the running-best matcher).  A wrong result that comes and goes - as the stem
    kernel's in rounds 2-4 - shows here whatever tolerance an oracle comparison would have forgiven it."""
    from frp_amd import native
    engine = fresh_engine
    raw, blob = get_raw_and_blob((1, 2, 2, 2), (3, 13, 30, 3))
    engine.load_weights(blob)
    rng = np.random.default_rng(31)
    B, H, W, K = 32, 1080, 1920, 10
    engine.upload_frames(_frames(rng, B, H, W))
    G = rng.standard_normal((100_000, 512)).astype(np.float32)
    engine.gallery_set(G)
    engine.det_hashes(True, fetch=False)
    try:
        engine.process_resident(K, flags=native.FLAG_FORCED_K)
        first = engine.fetch_results()
        h0 = engine.det_hashes()
        assert np.all(first["counts"] == K)
        for r in range(150):
            engine.process_resident(K, flags=native.FLAG_FORCED_K)
            got = engine.fetch_results()
            hr = engine.det_hashes()
            diff = [i + 1 for i in range(64) if h0[i] != hr[i]]
            assert not diff, f"step {r}: detector ops {diff} differ from the first step"
            for key in ("boxes", "kps", "scores", "counts", "emb", "match_idx", "match_cos"):
                if not np.array_equal(first[key], got[key]):
                    bad = np.argwhere(first[key] != got[key])
                    raise AssertionError(f"step {r}: {key} differs in {len(bad)} elements; first at {bad[0].tolist()} (frame, face, ...)")
    finally:
        engine.det_hashes(False, fetch=False)


def test_network_passes_replayed_from_captured_graphs_give_the_same_bits_and_counters(fresh_engine):
    """A detector / embedder pass asked for a second time with the same shapes, buffers and switches is captured as a hipGraph and from
    then on replayed by one call (net_program.cpp: run_net).  Forced-K and threshold mode (device-side face count): the first call (launch
    by launch), the capturing call and four replays return the same bits and charge the same counters; replays are counted; a weight
    reload and a changed batch size retire the stale graphs (results then equal a fresh handle's first, uncaptured call)."""
    from frp_amd import native
    engine = fresh_engine
    raw, blob = get_raw_and_blob((1, 1, 1, 1), (1, 1, 1, 1))
    raw2, blob2 = get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))
    rng = np.random.default_rng(41)
    B, H, W, K = 6, 720, 1280, 5
    frames = _frames(rng, B, H, W)
    G = rng.standard_normal((3000, 512)).astype(np.float32)
    keys = ("boxes", "kps", "scores", "counts", "emb", "match_idx", "match_cos")
    ckeys = ("det_conv_flops", "det_conv_launches", "emb_conv_flops", "emb_conv_launches", "faces", "frames")

    def run(e, flags, thresh, n=B):
        e.reset_counters()
        e.process_resident(K, det_thresh=thresh, flags=flags)
        r = e.fetch_results()
        c = e.counters()
        return r, {k: c[k] for k in ckeys}

    engine.load_weights(blob)
    engine.gallery_set(G)
    engine.upload_frames(frames)
    probe = engine.detect_resident((H, W), max_faces=64, det_thresh=1e-6, nms_iou=0.4)
    thr = float(np.clip(np.median(np.sort(probe["scores"], axis=1)[:, ::-1][:, 2]), 1e-4, 0.9999))      # ~3 faces per frame survive
    for flags, thresh in ((native.FLAG_FORCED_K, 0.5), (0, thr)):
        replays0 = engine.graph_replays()
        first, c_first = run(engine, flags, thresh)
        for i in range(5):
            got, c_got = run(engine, flags, thresh)
            for k in keys:
                assert np.array_equal(first[k], got[k]), f"call {i + 2} (flags {flags}): {k} differs from the first call"
            assert c_got == c_first, f"call {i + 2}: counters {c_got} != {c_first}"
        assert engine.graph_replays() - replays0 >= 2 * 4          # detector + embedder pass of calls 3 .. 6
        if not flags:
            assert 0 < first["counts"].sum() < B * K
    # stale graphs: another program in the same allocation, then another batch size - against a handle that has never captured anything
    other = native.Engine(0)
    try:
        other.load_weights(blob2)
        other.gallery_set(G)
        engine.load_weights(blob2)
        for n in (B, 3, B):
            engine.upload_frames(frames[:n])
            other.upload_frames(frames[:n])
            want, _ = run(other, native.FLAG_FORCED_K, 0.5)
            for _ in range(3):
                got, _ = run(engine, native.FLAG_FORCED_K, 0.5)
                for k in keys:
                    assert np.array_equal(want[k], got[k]), f"{n} frames after the reload: {k} differs from a fresh handle's"
    finally:
        other.close()


def test_other_config_shapes_4k_720p_and_million_gallery(engine):
    """Shapes of BASELINE configs 4 and 5 through the same path: one 3840x2160 frame (340,320 anchors,
    canvas 2176 rows), a mixed batch of 1280x720 frames, and a 1M-identity gallery (1.02 GB fp16)."""
    from frp_amd import native
    raw, blob = get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))
    engine.load_weights(blob)
    rng = np.random.default_rng(31)
    K = 6
    f4k = rng.integers(0, 256, size=(1, 2160, 3840, 3), dtype=np.uint8)
    a = engine.detect(f4k, max_faces=K, flags=native.FLAG_FORCED_K)
    heads = engine.head_maps()
    assert [h.shape[1:3] for h in heads] == [(272, 480), (136, 240), (68, 120)]
    ob, ok, osc, oa = onet.decode_nms([h[0] for h in heads], 0.0, 2.0, K)
    assert np.array_equal(a["anchor_idx"][0], oa) and np.array_equal(a["boxes"][0], ob)      # exact at 4K too
    f720 = rng.integers(0, 256, size=(5, 720, 1280, 3), dtype=np.uint8)
    o = engine.process_frames(f720, max_faces=K, flags=native.FLAG_FORCED_K | native.FLAG_NO_MATCH)
    assert np.all(o["counts"] == K) and np.abs(np.linalg.norm(o["emb"], axis=-1) - 1).max() < 1e-4
    single = engine.process_frames(f720[3:4], max_faces=K, flags=native.FLAG_FORCED_K | native.FLAG_NO_MATCH)
    assert np.array_equal(single["emb"][0], o["emb"][3])                  # batch position does not matter
    # 1M gallery: planted rows found, cosine within 1e-3 of float64
    N = 1_000_000
    G = rng.standard_normal((N, 512)).astype(np.float32)
    G /= np.linalg.norm(G, axis=1, keepdims=True)
    engine.gallery_set(G)
    rows = rng.choice(N, size=9, replace=False)
    Q = G[rows] + 0.02 * rng.standard_normal((9, 512)).astype(np.float32)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    idx, cos = engine.match(Q)
    assert np.array_equal(idx, rows)
    assert np.abs(cos - (Q.astype(np.float64) * G[rows].astype(np.float64)).sum(1)).max() < 1e-3
    engine.gallery_set(np.zeros((0, 512), np.float32))


def test_resize_and_pyramid_merge(engine):
    """Config-4 pyramid: the device resize is bit-exact vs the oracle's rule, per-scale detections equal
    the oracle decode of the GPU's own head maps, and the cross-scale merge + NMS equals the oracle's
    independent (scalar-loop) restatement; faces are then embedded from the full-resolution frame."""
    from frp_amd import native, pyramid
    raw, blob = get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))
    engine.load_weights(blob)
    rng = np.random.default_rng(99)
    H, W = 360, 500
    frames = _frames(rng, 2, H, W)
    scales = (1.0, 0.5, 0.25)
    engine.upload_frames(frames)
    thr = 0.30
    per, head_sets = [], []
    for s in scales:
        hw = pyramid.scaled_size(H, W, s)
        d = engine.detect_resident(hw, max_faces=64, det_thresh=thr, nms_iou=0.4)
        heads = engine.head_maps()
        head_sets.append(heads)
        per.append((hw, d))
        # the resized image the detector saw: check through the oracle on frame 0 (fp16 heads within tolerance)
        if s != 1.0:
            img = onet.resize_bilinear_u8(frames[0], hw)
            ref = onet.det_forward(raw, onet.det_blob(img[None], ((hw[0] + 31) // 32 * 32, (hw[1] + 31) // 32 * 32)))
            for g, r in zip(heads, ref):
                assert np.abs(g[0, ..., :30].astype(np.float32) - r[0]).max() < 2e-2 * max(1.0, float(np.abs(r).max()))
    boxes, kps, scores, counts = pyramid.merge_scales(per, (H, W), 8, 0.4)
    for b in range(2):
        ob, ok, osc = onet.detect_pyramid(raw, frames[b], scales, thr, 0.4, 8, 64,
                                          head_maps_per_scale=[[h[b] for h in hs] for hs in head_sets])
        n = len(ob)
        assert counts[b] == n and n >= 2
        assert np.array_equal(boxes[b, :n], ob) and np.array_equal(kps[b, :n], ok)
        assert np.abs(scores[b, :n] - osc).max() < 1e-6
    # whole call: same detections, embeddings from the full-resolution frame
    G = rng.standard_normal((64, 512)).astype(np.float32)
    engine.gallery_set(G)
    out = engine.process_frames_pyramid(frames, scales, max_faces=8, det_thresh=thr, nms_iou=0.4)
    assert np.array_equal(out["counts"], counts) and np.array_equal(out["boxes"], boxes)
    for b in range(2):
        n = counts[b]
        e = engine.embed_faces(frames[b], kps[b, :n])
        assert np.abs(e - out["emb"][b, :n]).max() < 1e-6
        assert np.all(out["match_idx"][b, :n] >= 0) and np.all(out["match_idx"][b, n:] == -1)
    engine.gallery_set(np.zeros((0, 512), np.float32))


def test_config4_full_size_4k_pyramid_million_gallery(engine):
    """BASELINE config 4 at full size, end to end through one call: 1 x 3840x2160 frame, pyramid scales {1, .5, .25},
    1M-identity gallery.  Per scale the device's detections equal the oracle's decode of the GPU's own head maps;
    the cross-scale merge + NMS equals the oracle's independent restatement; embeddings come from the full-resolution
    frame; top-1 over the 1M gallery is the planted identity with the cosine within 1e-3 of float64."""
    from frp_amd import pyramid
    raw, blob = get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))
    engine.load_weights(blob)
    rng = np.random.default_rng(404)
    H, W = 2160, 3840
    frame = _frames(rng, 1, 540, 960)                                   # structure at 1/4 scale ...
    frame = np.repeat(np.repeat(frame, 4, axis=1), 4, axis=2)           # ... blown up, plus pixel noise
    frame = np.clip(frame.astype(np.int16) + rng.integers(-6, 7, size=frame.shape), 0, 255).astype(np.uint8)
    scales, K, thr = (1.0, 0.5, 0.25), 8, 0.30
    engine.upload_frames(frame)
    per, head_sets = [], []
    for sc in scales:
        hw = pyramid.scaled_size(H, W, sc)
        d = engine.detect_resident(hw, max_faces=64, det_thresh=thr, nms_iou=0.4)
        heads = engine.head_maps()
        assert heads[0].shape[1:3] == ((hw[0] + 31) // 32 * 4, (hw[1] + 31) // 32 * 4)
        ob, ok, osc, oa = onet.decode_nms([h[0] for h in heads], thr, 0.4, 64)
        n = len(oa)
        assert d["counts"][0] == n and np.array_equal(d["anchor_idx"][0, :n], oa) and np.array_equal(d["boxes"][0, :n], ob)
        head_sets.append(heads)
        per.append((hw, d))
    boxes, kps, scores, counts = pyramid.merge_scales(per, (H, W), K, 0.4)
    ob, ok, osc = onet.detect_pyramid(raw, frame[0], scales, thr, 0.4, K, 64,
                                      head_maps_per_scale=[[h[0] for h in hs] for hs in head_sets])
    n = len(ob)
    assert counts[0] == n and n >= 1
    assert np.array_equal(boxes[0, :n], ob) and np.array_equal(kps[0, :n], ok)
    # 1M gallery with the frame's own identities planted
    N = 1_000_000
    G = rng.standard_normal((N, 512)).astype(np.float32)
    G /= np.linalg.norm(G, axis=1, keepdims=True)
    e = engine.embed_faces(frame[0], kps[0, :n])
    rows = rng.choice(N, size=n, replace=False)
    G[rows] = e
    engine.gallery_set(G)
    out = engine.process_frames_pyramid(frame, scales, max_faces=K, det_thresh=thr, nms_iou=0.4)
    assert out["counts"][0] == n and np.array_equal(out["boxes"][0, :n], ob)
    assert np.abs(out["emb"][0, :n] - e).max() < 1e-6
    assert np.array_equal(out["match_idx"][0, :n], rows)
    want = (e.astype(np.float64) * G[rows].astype(np.float64)).sum(1)
    assert np.abs(out["match_cos"][0, :n] - want).max() < 1e-3
    # aligned chips of the full-resolution frame against the oracle's warp
    chips = engine.align(frame[0], kps[0, :n])
    for i in range(n):                                     # float64 reference and its derived per-pixel bound (tests/align_model.py)
        blob, tol = align_model.reference(frame[0], kps[0, i])
        assert align_model.within(chips[i, ..., :3], blob, tol), (i, align_model.worst(chips[i, ..., :3], blob, tol))
    engine.gallery_set(np.zeros((0, 512), np.float32))


def test_resize_bit_exact(engine):
    """device bilinear resize == the oracle's rule, bit for bit (down- and up-scaling, odd sizes)"""
    raw, blob = get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))
    engine.load_weights(blob)
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, size=(2, 128, 192, 3), dtype=np.uint8)
    engine.upload_frames(img)
    for hw in [(64, 96), (37, 51), (128, 192), (200, 300), (32, 33)]:
        engine.detect_resident(hw, max_faces=4, flags=1)
        got = engine.det_source()
        assert got.shape == (2, hw[0], hw[1], 3)
        for b in range(2):
            ref = img[b] if hw == (128, 192) else onet.resize_bilinear_u8(img[b], hw)
            assert np.array_equal(got[b], ref), hw


def test_fp8_weight_blob(engine):
    """BASELINE config 5 (fp8 weight storage).  (1) The loader's E4M3 -> fp16 expansion is exact: an fp8 blob
    and an fp16 blob holding the same dequantised weights give bit-identical results.  (2) Accuracy bar of
    SURVEY 8c for fp8: top-1 identity unchanged, embedding cosine vs the fp16 weights >= 0.99 (measured with
    tools/fp8_cosine.py on seeded weights: min 0.9975 for IResNet-100, 0.9977 for R50 and the small net)."""
    from frp_amd import weights as wts
    rng = np.random.default_rng(55)
    frames = _frames(rng, 2, 160, 192)
    chips = rng.integers(0, 256, size=(6, 112, 112, 3), dtype=np.uint8)
    for det_blocks, emb_blocks in [((1, 2, 2, 2), (1, 1, 1, 1)), ((1, 1, 1, 1), (3, 13, 30, 3))]:
        raw = wts.make_synthetic_raw(17, det_blocks, emb_blocks)
        rt = lambda l, w16: wts.fp8_dequantize_rows(*wts.fp8_quantize_rows(w16))     # noqa: E731
        blobs = {"fp8": wts.pack_blob(raw, det_blocks, emb_blocks, weight_format="fp8"),
                 "fp16_of_fp8": wts.pack_blob(raw, det_blocks, emb_blocks, w16_hook=rt),
                 "fp16": wts.pack_blob(raw, det_blocks, emb_blocks)}
        out = {}
        for name, blob in blobs.items():
            engine.load_weights(blob)
            engine.detect(frames, max_faces=4, det_thresh=0.5)
            out[name] = ([h.copy() for h in engine.head_maps()], engine.embed_aligned(chips))
        for a, b in zip(out["fp8"][0], out["fp16_of_fp8"][0]):
            assert np.array_equal(a, b)
        assert np.array_equal(out["fp8"][1], out["fp16_of_fp8"][1])
        e8, e16 = out["fp8"][1], out["fp16"][1]
        cos = (e8 * e16).sum(1)
        assert cos.min() > 0.99, cos
        # top-1 against a gallery that contains the fp16 embeddings among 5000 distractors
        G = rng.standard_normal((5000, 512)).astype(np.float32)
        G[100:100 + len(e16)] = e16
        engine.gallery_set(G)
        idx, _ = engine.match(e8)
        assert np.array_equal(idx, np.arange(100, 100 + len(e16)))


def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def test_fp8_mfma_embedder(engine):
    """BASELINE config 5 ("fp8 ArcFace weights (CDNA4 fp8 MFMA)"): the embedder blob packed with weight_format
    "fp8-mfma" runs every eligible 3x3 conv of stages 2-4 on E4M3 ACTIVATIONS and WEIGHTS through the block-scaled fp8
    MFMA kernel (the residual stream stays fp16; fp8 copies are written by the producing epilogues; per-tensor activation
    scales from the calibration pass in weights.calibrate_fp8).  Compared with
      (a) the program in fp32 on the fp8-DEQUANTISED weights of exactly those layers (weights.fp8_dequantized_weights;
          the other layers keep their fp16-rounded weights): what is left is the E4M3 rounding of the activations;
      (b) the fp32 oracle network on the original weights (weights + activations);
      (c) the fp16 path of the library.
    Bars: top-1 identity identical among 5,000 distractors; cosine >= 0.99 against all three
    (measured on the seeded R100: see the assertion message / DESIGN.md; E4M3 carries 3 mantissa bits and the error
    of ~90 fp8 layers accumulates in the residual stream - decisions near the thresholds: test_fp8_decision_flips)."""
    from frp_amd import weights as wts
    rng = np.random.default_rng(58)
    chips = rng.integers(0, 256, size=(8, 112, 112, 3), dtype=np.uint8)
    floors = {}
    for det_blocks, emb_blocks in [((1, 1, 1, 1), (1, 2, 2, 1)), ((1, 1, 1, 1), (3, 13, 30, 3))]:
        raw = wts.make_synthetic_raw(19, det_blocks, emb_blocks)
        layers = wts.ns.iresnet_layers(emb_blocks)
        plan = wts.plan_fp8(layers)
        blob8 = wts.pack_blob(raw, det_blocks, emb_blocks, weight_format="fp8-mfma")
        engine.load_weights(wts.pack_blob(raw, det_blocks, emb_blocks))
        e16 = engine.embed_aligned(chips)
        engine.load_weights(blob8)
        engine.reset_counters()
        e8 = engine.embed_aligned(chips)
        ctr = engine.counters()
        n_f8 = sum(1 for pl in plan if pl["f8"])
        assert ctr["f8_conv_launches"] == n_f8 > 0                     # the fp8 kernel really ran, on every planned layer
        assert np.abs(np.linalg.norm(e8, axis=1) - 1).max() < 1e-4
        ref_dq = _unit(wts.run_program_fp32(raw, layers, wts.emb_input_blob(chips), fp16_storage=False,
                                            weights_of=wts.fp8_dequantized_weights(layers, plan)))
        ref = onet.emb_forward(raw, onet.emb_blob(chips))
        # the dequantised-weight reference really differs from the plain one (it did not, when it was a plain copy)
        assert 1e-5 < 1 - (ref_dq * ref).sum(1).min() < 2e-2
        cos_dq, cos_ref, cos16 = (e8 * ref_dq).sum(1), (e8 * ref).sum(1), (e8 * e16).sum(1)
        floors[emb_blocks] = (float(cos_dq.min()), float(cos_ref.min()), float(cos16.min()))
        assert min(floors[emb_blocks]) > 0.99, floors
        assert cos_dq.min() >= cos_ref.min() - 2e-3, floors           # weight rounding removed: not further away
        G = rng.standard_normal((5000, 512)).astype(np.float32)
        G[200:200 + len(e16)] = e16
        engine.gallery_set(G)
        idx, _ = engine.match(e8)
        assert np.array_equal(idx, np.arange(200, 200 + len(e16)))       # identical top-1 identity
    print("fp8-mfma cosine floors (vs dequantised-weight fp32 program, vs fp32 oracle, vs fp16 path):", floors)
    engine.gallery_set(np.zeros((0, 512), np.float32))


def test_fp8_activation_scales_follow_the_tensor_range(engine):
    """The calibration has teeth: the SAME embedder function with its inner activations 1024 x larger / smaller
    (conftest.rescaled_embedder_raw: bn2 scaled, conv2 divided).  Calibrated blobs: the fp8 tensors hold the same codes, the
    embedding does not move (cos >= 1 - 1e-3 against the unscaled fp8 run; not bit-exact only because the rescaled conv
    weights become fp16 subnormals).  Uncalibrated blobs (unit scales, what pack_blob wrote before): 1024 x saturates the
    tail of the tensor at E4M3's 448, 1/1024 x flushes most of it to zero - the embedding leaves."""
    from conftest import rescaled_embedder_raw
    from frp_amd import weights as wts
    rng = np.random.default_rng(59)
    chips = rng.integers(0, 256, size=(6, 112, 112, 3), dtype=np.uint8)
    blocks = (2, 3, 4, 2)
    raw = wts.make_synthetic_raw(23, (1, 1, 1, 1), blocks)
    engine.load_weights(wts.pack_blob(raw, (1, 1, 1, 1), blocks, weight_format="fp8-mfma"))
    base = engine.embed_aligned(chips)
    engine.load_weights(wts.pack_blob(raw, (1, 1, 1, 1), blocks))
    e16 = engine.embed_aligned(chips)
    assert (base * e16).sum(1).min() > 0.985
    moved = {}
    for f in (1024.0, 1.0 / 1024):
        raw_f = rescaled_embedder_raw(raw, blocks, f)
        engine.load_weights(wts.pack_blob(raw_f, (1, 1, 1, 1), blocks))
        assert (engine.embed_aligned(chips) * e16).sum(1).min() > 1 - 1e-4        # the same function (fp16 path)
        engine.load_weights(wts.pack_blob(raw_f, (1, 1, 1, 1), blocks, weight_format="fp8-mfma"))
        cal = engine.embed_aligned(chips)
        engine.load_weights(wts.pack_blob(raw_f, (1, 1, 1, 1), blocks, weight_format="fp8-mfma", calibrate=False))
        unc = engine.embed_aligned(chips)
        moved[f] = (float((cal * base).sum(1).min()), float((unc * base).sum(1).min()))
    print("calibrated / uncalibrated cosine vs the unscaled fp8 run:", moved)
    for f, (c_cal, c_unc) in moved.items():
        assert c_cal > 1 - 1e-3, moved
        assert c_unc < 0.99, moved


def _planted_rows(e, dists, rng):
    """unit rows at exact Euclidean distances `dists` [M, R] from the unit vectors e [M, 512] (random directions)"""
    M, R = dists.shape
    u = rng.standard_normal((M, R, 512))
    u -= (u * e[:, None, :]).sum(-1, keepdims=True) * e[:, None, :]
    u /= np.linalg.norm(u, axis=-1, keepdims=True)
    c = 1.0 - dists.astype(np.float64) ** 2 / 2.0
    return (c[..., None] * e[:, None, :] + np.sqrt(1.0 - c ** 2)[..., None] * u).astype(np.float32)


def test_fp8_decision_flips_near_thresholds(engine):
    """What the fp8 path's embedding drift means for the reference's DECISIONS (face_service.py:43,411 match d <= 0.6;
    :486-492 buckets at 0.4 / 0.6; :352-364 duplicate gate d < 0.3): for 48 faces, gallery rows planted at distance
    threshold -+ delta of the fp16 embedding, delta in {0.01, 0.02, 0.05, 0.1}; a decision FLIPS when the fp8 embedding
    puts the row on the other side of the threshold.  Bar: no flip at delta >= 0.05 (the measured drift of a distance is
    below 0.03); the flip counts at 0.01 / 0.02 are printed (DESIGN.md quotes them)."""
    from frp_amd import weights as wts
    rng = np.random.default_rng(61)
    chips = rng.integers(0, 256, size=(48, 112, 112, 3), dtype=np.uint8)
    blocks = (3, 13, 30, 3)
    raw = wts.make_synthetic_raw(19, (1, 1, 1, 1), blocks)
    engine.load_weights(wts.pack_blob(raw, (1, 1, 1, 1), blocks))
    e16 = engine.embed_aligned(chips)
    engine.load_weights(wts.pack_blob(raw, (1, 1, 1, 1), blocks, weight_format="fp8-mfma"))
    e8 = engine.embed_aligned(chips)
    deltas = np.array([0.01, 0.02, 0.05, 0.1])
    thr = np.array([0.3, 0.4, 0.6])
    signed = np.concatenate([-deltas[::-1], deltas])                                   # 8 offsets per threshold
    dists = np.tile((thr[:, None] + signed[None, :]).reshape(1, -1), (len(chips), 1))    # [M, 24]
    rows = _planted_rows(e16.astype(np.float64), dists, rng).reshape(-1, 512)
    engine.gallery_set(rows)
    stored = engine.gallery_get(0, len(rows)).astype(np.float64)                        # the unit fp16 rows the device matches
    R = dists.shape[1]
    flips = np.zeros((len(thr), len(signed)), int)
    drift = []
    for q, name in ((e16, "fp16"), (e8, "fp8")):
        cos = engine.match_scores(q)                                                     # [M, M*R]
        d = onet.cos_to_distance(np.stack([cos[i, i * R:(i + 1) * R] for i in range(len(chips))]))
        if name == "fp16":
            d16 = d
            # the planted geometry survives the fp16 gallery: every row is on the side it was planted on
            assert np.all((d16 < np.repeat(thr, len(signed))[None]) == (dists < np.repeat(thr, len(signed))[None]))
        else:
            drift = np.abs(d - d16)
            for ti, t in enumerate(thr):
                sl = slice(ti * len(signed), (ti + 1) * len(signed))
                flips[ti] = ((d[:, sl] < t) != (d16[:, sl] < t)).sum(0)       # 0.3: dup gate, 0.4: bucket; 0.6 below
                if t == 0.6:
                    flips[ti] = ((d[:, sl] <= t) != (d16[:, sl] <= t)).sum(0)  # match = d <= tolerance (:411)
    report = {f"thr {t}": {f"{s:+.2f}": int(n) for s, n in zip(signed, flips[ti])} for ti, t in enumerate(thr)}
    print(f"fp8 decision flips of {len(chips)} faces per planted offset:", report, "max |distance drift|", float(drift.max()),
          "mean", float(drift.mean()), "cos(e8, e16) min", float((e8 * e16).sum(1).min()))
    far = np.abs(signed) >= 0.05
    assert flips[:, far].sum() == 0, report
    assert drift.max() < 0.03, float(drift.max())
    engine.gallery_set(np.zeros((0, 512), np.float32))


def test_config5_end_to_end_720p_two_streams_fp8(engine):
    """BASELINE configs[4] end to end: two synthetic 720p streams mixed into one batch per GPU (frame t of stream 0,
    frame t of stream 1, ...), detector fp16, embedder on the fp8 matrix path, match against a 20 k gallery holding the
    faces' own fp16 embeddings.  Against the fp16 blob on the same batch: boxes / landmarks / scores / counts identical
    (the detector does not change), top-1 rows identical, embedding cosine above the fp8 bar; and the batch gives every
    frame the result it gets alone (mixing streams into a batch changes nothing)."""
    from frp_amd import native, weights as wts
    rng = np.random.default_rng(62)
    det_blocks, emb_blocks = (1, 2, 2, 2), (3, 13, 30, 3)
    raw = wts.make_synthetic_raw(7, det_blocks, emb_blocks)
    streams = [_frames(np.random.default_rng(100 + s), 3, 720, 1280) for s in range(2)]
    batch = np.stack([streams[s][t] for t in range(3) for s in range(2)])             # interleaved: 6 x 720p
    K = 5
    engine.load_weights(wts.pack_blob(raw, det_blocks, emb_blocks))
    engine.gallery_set(np.zeros((0, 512), np.float32))
    o16 = engine.process_frames(batch, max_faces=K, flags=native.FLAG_FORCED_K | native.FLAG_NO_MATCH)
    assert np.all(o16["counts"] == K)
    G = _unit(rng.standard_normal((20000, 512))).astype(np.float32)
    rows = rng.choice(len(G), size=batch.shape[0] * K, replace=False).reshape(batch.shape[0], K)
    G[rows.reshape(-1)] = o16["emb"].reshape(-1, 512)
    engine.gallery_set(G)
    o16 = engine.process_frames(batch, max_faces=K, flags=native.FLAG_FORCED_K)
    assert np.array_equal(o16["match_idx"], rows)
    engine.load_weights(wts.pack_blob(raw, det_blocks, emb_blocks, weight_format="fp8-mfma"))
    o8 = engine.process_frames(batch, max_faces=K, flags=native.FLAG_FORCED_K)
    for k in ("boxes", "kps", "scores", "counts"):
        assert np.array_equal(o8[k], o16[k]), k
    assert np.array_equal(o8["match_idx"], rows)                                     # identical top-1 identity
    cos = (o8["emb"] * o16["emb"]).sum(-1)
    assert cos.min() > 0.99, float(cos.min())
    assert np.abs(o8["match_cos"] - cos).max() < 2e-3                                # the matcher saw these embeddings
    alone = engine.process_frames(streams[1][2][None], max_faces=K, flags=native.FLAG_FORCED_K)
    for k in ("boxes", "kps", "scores", "match_idx"):
        assert np.array_equal(alone[k][0], o8[k][5]), k                              # frame 2 of stream 1 = batch slot 5
    assert np.abs(alone["emb"][0] - o8["emb"][5]).max() < 1e-6                        # (the FC's split-K follows the batch size)
    print("config-5 end to end: cos(fp8, fp16) min", float(cos.min()), "mean", float(cos.mean()))
    engine.gallery_set(np.zeros((0, 512), np.float32))


def test_malformed_blobs_are_rejected_not_executed(engine):
    """frp_load_weights / the planner validate everything a kernel would otherwise trust: every corruption
    below must come back as an error (never a launch), and the engine must stay usable afterwards."""
    import struct
    from frp_amd import weights as wts
    from frp_amd.native import FrpError
    raw, blob = get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))
    hdr = list(struct.unpack(wts.HEADER_FMT, blob[:wts.HEADER_BYTES]))
    n_det, det_off, emb_off, data_off, data_bytes = hdr[3], hdr[19], hdr[20], hdr[21], hdr[22]
    op_size = struct.calcsize(wts.OP_FMT)

    def with_header(**kw):
        h2 = list(hdr)
        for k, v in kw.items():
            h2[int(k[1:])] = v
        return struct.pack(wts.HEADER_FMT, *h2) + blob[wts.HEADER_BYTES:]

    def with_op(i, **kw):
        names = wts.OP_FIELDS
        off = det_off + i * op_size
        op = list(struct.unpack(wts.OP_FMT, blob[off:off + op_size]))
        for k, v in kw.items():
            op[names.index(k)] = v
        return blob[:off] + struct.pack(wts.OP_FMT, *op) + blob[off + op_size:]

    ops = [struct.unpack(wts.OP_FMT, blob[det_off + i * op_size: det_off + (i + 1) * op_size]) for i in range(n_det)]
    res_i = next(i for i, o in enumerate(ops) if o[2] >= 0 and not (o[8] & 4))        # a block conv with a plain residual
    frames = np.zeros((1, 64, 64, 3), np.uint8)
    load_time = {
        "truncated": blob[:len(blob) // 2],
        "tiny": blob[:40],
        "magic": b"XRPBLOB1" + blob[8:],
        "version": with_header(f1=99),
        "data beyond file": with_header(f22=data_bytes + 4096),
        "op table beyond file": with_header(f19=len(blob) - 8),
        "head buffer id": with_header(f8=10 ** 6),
        "buffer id": with_op(3, out_buf=10 ** 6),
        "in == out": with_op(3, out_buf=ops[3][0]),
        "weight offset": with_op(3, w_off=data_bytes - 16),
        "bias offset": with_op(3, bias_off=data_bytes + 256),
        "kernel size": with_op(3, ksize=5),
        "stride": with_op(3, stride=3),
        "activation": with_op(3, act=7),
        "fp8 flag without room for the scales": with_op(n_det - 1, flags=ops[n_det - 1][8] | 16, w_off=data_bytes - 256),
        "op table offset that wraps in 64 bits": with_header(f19=2 ** 64 - 64),
        "upsampled residual without a residual": with_op(3, res_buf=-1, flags=ops[3][8] | 4),
        "residual id below -1": with_op(res_i, res_buf=-7),
    }
    for name, bad in load_time.items():
        with pytest.raises(FrpError):
            engine.load_weights(bad)
        with pytest.raises(FrpError):                     # a failed load leaves no half-loaded program behind
            engine.detect(frames, max_faces=2)
    # plan-time corruptions: walk the program as the planner does (physical buffers are recycled) to pick
    # buffers that are GUARANTEED inconsistent at that op
    def dims_before(i, H=64, W=64):
        d = {hdr[5]: (H, W, 8)}
        for o in ops[:i]:
            h, w, _ = d[o[0]]
            k, st = o[5], o[6]
            d[o[1]] = ((h + 2 * (k // 2) - k) // st + 1, (w + 2 * (k // 2) - k) // st + 1, o[4])
        return d
    d_res = dims_before(res_i)
    h, w, _ = d_res[ops[res_i][0]]
    want = (h, w, ops[res_i][4])                                         # stride-1 3x3: output dims = input dims
    wrong_res = next(b for b, dd in d_res.items() if dd != want and b != ops[res_i][1])
    unwritten = next(b for b in range(hdr[4]) if b not in dims_before(2) and b != ops[2][1])
    plan_time = {
        "channel chain": with_op(4, cin=ops[4][3] * 2),
        "residual shape": with_op(res_i, res_buf=wrong_res),
        "reads an unwritten buffer": with_op(2, in_buf=unwritten),
    }
    for name, bad in plan_time.items():
        try:
            engine.load_weights(bad)
        except FrpError:
            continue                                       # rejected at load: fine too
        with pytest.raises(FrpError):
            engine.detect(frames, max_faces=2)
    engine.load_weights(blob)                              # and a good blob still works
    out = engine.detect(frames, max_faces=2)
    assert out["counts"].shape == (1,)


def test_c_abi_rejects_bad_arguments(engine):
    """every entry point returns a negative status (and a message) on null / out-of-range arguments
    instead of touching memory"""
    import ctypes as C
    lib, h = engine._lib, engine._h
    raw, blob = get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))
    engine.load_weights(blob)
    f = np.zeros((1, 64, 64, 3), np.uint8)
    o = engine._alloc(1, 4)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)     # noqa: E731
    outs = [ptr(o["boxes"]), ptr(o["kps"]), ptr(o["scores"]), ptr(o["counts"]), ptr(o["emb"]), ptr(o["match_idx"]), ptr(o["match_cos"])]
    G0 = np.random.default_rng(5).standard_normal((8, 512)).astype(np.float32)
    engine.gallery_set(G0)
    engine.process_frames(f, max_faces=4, flags=1)     # leaves results of shape (B=1, K=4) and one resident frame on the handle
    bad_calls = [
        lambda: lib.frp_process_frames(h, None, 1, 64, 64, 192, 4, 0.5, 0.4, 0, *outs),
        lambda: lib.frp_process_frames(h, ptr(f), 0, 64, 64, 192, 4, 0.5, 0.4, 0, *outs),
        lambda: lib.frp_process_frames(h, ptr(f), 1, 64, 64, 100, 4, 0.5, 0.4, 0, *outs),          # row stride < W*3
        lambda: lib.frp_process_frames(h, ptr(f), 1, 64, 64, 192, 0, 0.5, 0.4, 0, *outs),          # max_faces 0
        lambda: lib.frp_process_frames(h, ptr(f), 1, 64, 64, 192, 1000, 0.5, 0.4, 0, *outs),       # max_faces > cap
        lambda: lib.frp_process_frames(h, ptr(f), 5000, 64, 64, 192, 4, 0.5, 0.4, 0, *outs),       # batch too large
        lambda: lib.frp_upload_frames(h, None, 1, 64, 64, 192),
        lambda: lib.frp_upload_frames_async(h, ptr(f), 1, -3, 64, 192),
        lambda: lib.frp_match(h, None, 1, 1, ptr(o["match_idx"]), ptr(o["match_cos"])),
        lambda: lib.frp_match_scores(h, ptr(o["emb"]), 1, None, engine.gallery_size()),
        # caller-sized buffers that no longer match the handle's state (a concurrent caller changed it): refused under
        # the handle mutex, nothing written
        lambda: lib.frp_match_scores(h, ptr(o["emb"]), 1, ptr(o["emb"]), engine.gallery_size() + 1),
        lambda: lib.frp_fetch_results(h, 7, 4, *outs),
        lambda: lib.frp_fetch_results(h, 1, 3, *outs),
        lambda: lib.frp_finish_faces(h, 9, ptr(o["boxes"]), ptr(o["kps"]), ptr(o["scores"]), ptr(o["counts"]), 4, 0, ptr(o["emb"]),
                                     ptr(o["match_idx"]), ptr(o["match_cos"])),
        lambda: lib.frp_detect_resident(h, 9, 64, 64, 4, 0.5, 0.4, 0, ptr(o["boxes"]), ptr(o["kps"]), ptr(o["scores"]), ptr(o["counts"]), None),
        lambda: lib.frp_gallery_set(h, None, 5, 512, 0),
        lambda: lib.frp_gallery_set(h, ptr(o["emb"]), 1, 128, 0),                                 # wrong dimension
        lambda: lib.frp_gallery_remove_row(h, 10 ** 9),
        lambda: lib.frp_load_weights(h, None, 100),
        lambda: lib.frp_embed_aligned(h, None, 3, ptr(o["emb"])),
        lambda: lib.frp_conv2d_nhwc(h, ptr(f), 1, 8, 8, 24, ptr(f), 32, 3, 1, ptr(o["scores"]), None, None, 0, 0, 0, 0, ptr(o["emb"])),
        lambda: lib.frp_process_frames(None, ptr(f), 1, 64, 64, 192, 4, 0.5, 0.4, 0, *outs),      # null handle
        lambda: lib.frp_gallery_reserve(h, 0, C.byref(C.c_void_p())),
        lambda: lib.frp_gallery_commit(h, 5),                                                      # nothing reserved
    ]
    for i, call in enumerate(bad_calls):
        assert call() < 0, i
    assert lib.frp_last_error(h)                      # a message is kept for the last failure on this handle
    from frp_amd.native import FrpError
    with pytest.raises(FrpError):                     # the failed frp_load_weights above unloaded the program
        engine.process_frames(f, max_faces=4)
    engine.load_weights(blob)
    res = engine.process_frames(f, max_faces=4)       # still alive
    assert res["counts"].shape == (1,)


def test_one_handle_shared_by_threads(engine):
    """the reference calls the service from a 4-thread pool (routes/camera.py:30,277-279): concurrent callers
    of ONE handle are serialised by its mutex and every caller gets its own, correct result"""
    import threading
    rng = np.random.default_rng(31)
    raw, blob = get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))
    engine.load_weights(blob)
    engine.gallery_set(rng.standard_normal((500, 512)).astype(np.float32))
    jobs = [(_frames(rng, 2, 96 + 32 * (i % 2), 160), rng.integers(0, 256, (3, 112, 112, 3), dtype=np.uint8)) for i in range(4)]
    want = [(engine.process_frames(f, max_faces=3, flags=1), engine.embed_aligned(c)) for f, c in jobs]
    got = [None] * 4
    errs = []

    def worker(i):
        try:
            for _ in range(5):
                a = engine.process_frames(jobs[i][0], max_faces=3, flags=1)
                b = engine.embed_aligned(jobs[i][1])
                got[i] = (a, b)
        except Exception as e:              # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=worker, args=(i,)) for i in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    for i in range(4):
        for key in ("boxes", "kps", "emb", "match_idx", "match_cos", "counts"):
            assert np.array_equal(got[i][0][key], want[i][0][key]), (i, key)
        assert np.array_equal(got[i][1], want[i][1])


def test_full_size_detector_vs_oracle_one_frame(engine):
    """the full detector on true 1080p frames (maps 544x960 ... 34x60: every wide-image path of the row-patch
    kernel, the XCD tile walk, the fused stems at full size) against the fp32 oracle, frame 0 of a batch of 3"""
    raw, blob = get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))
    engine.load_weights(blob)
    rng = np.random.default_rng(77)
    frames = rng.integers(0, 256, size=(3, 1080, 1920, 3), dtype=np.uint8)
    frames[1:] = frames[0]                                   # batch entries 1, 2 repeat frame 0
    engine.detect(frames, max_faces=4, det_thresh=0.5)
    heads = engine.head_maps()
    ref = onet.det_forward(raw, onet.det_blob(frames[:1], (1088, 1920)))
    for g, r in zip(heads, ref):
        assert g.shape[1:3] == r.shape[1:3]
        scale = max(1.0, float(np.abs(r).max()))
        err = np.abs(g[0, ..., :30].astype(np.float32) - r[0]).max()
        assert err < 2e-2 * scale, (err, scale)
        assert np.array_equal(g[0], g[1]) and np.array_equal(g[0], g[2])     # position in the batch does not matter


EMB_ONNX_LAYOUTS = [dict(named=True), dict(named=False), dict(named=False, fuse_bn=True),
                    dict(named=False, fuse_bn=True, shortcut_first=True, matmul_fc=True, raw_data=False),
                    dict(named=False, eps=2e-5, shortcut_first=True, matmul_fc=True)]
DET_ONNX_LAYOUTS = [dict(named=True), dict(named=False), dict(named=False, fuse_bn=True),
                    dict(named=False, eps=2e-5, shortcut_first=True, laterals_first=True, raw_data=False),
                    dict(named=False, fuse_bn=True, split_heads=True, sigmoid_scores=True)]


@pytest.mark.parametrize("layout", range(5))
def test_onnx_packs_reach_the_device(engine, layout):
    """SURVEY.md 8(f-3) on the device: ONNX files as exporters write them (five embedder layouts: named / anonymous initializers,
    BatchNorms folded into Conv / Gemm, MXNet epsilon, shortcut-first order, MatMul + Add FC, typed instead of raw tensor
    payloads; five detector layouts: + laterals-first order, SCRFD-style split heads behind a Sigmoid) -> onnx_pack ->
    weight blob -> frp_load_weights -> the HIP kernels, against the fp32 oracle on the SOURCE raw dict (the weights the files
    were written from): embeddings cos >= 1 - 1e-3, head maps <= 2e-2 x scale, decode / NMS on those maps exact."""
    from frp_amd import onnx_pack, weights
    det_blocks, emb_blocks = (1, 2, 1, 1), (2, 1, 2, 1)
    src = weights.make_synthetic_raw(31, det_blocks, emb_blocks)
    det_file = onnx_pack.detector_to_onnx(src, **DET_ONNX_LAYOUTS[layout])
    emb_file = onnx_pack.iresnet_to_onnx(src, **EMB_ONNX_LAYOUTS[layout])
    blob = onnx_pack.pack_from_onnx(det_file, emb_file)
    engine.load_weights(blob)
    rng = np.random.default_rng(40 + layout)
    # embedder
    chips = rng.integers(0, 256, (6, 112, 112, 3), dtype=np.uint8)
    got = engine.embed_aligned(chips)
    ref = onet.emb_forward(src, onet.emb_blob(chips))
    cos = (got * ref).sum(1)
    assert cos.min() >= 1 - 1e-3, cos
    # detector: head maps, then decode / NMS of the device's own maps
    B, H, W = 2, 150, 200
    canvas = ((H + 31) // 32 * 32, (W + 31) // 32 * 32)
    frames = rng.integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)
    det = engine.detect(frames, max_faces=6, det_thresh=0.5)
    heads = engine.head_maps()
    for g, r in zip(heads, onet.det_forward(src, onet.det_blob(frames, canvas))):
        scale = max(1.0, float(np.abs(r).max()))
        assert g.shape[:3] == r.shape[:3] and np.abs(g[..., :30].astype(np.float32) - r).max() < 2e-2 * scale
    for b in range(B):
        ob, ok, osc, oa = onet.decode_nms([h[b] for h in heads], 0.5, 0.4, 6)
        n = len(oa)
        assert det["counts"][b] == n and np.array_equal(det["anchor_idx"][b, :n], oa) and np.array_equal(det["boxes"][b, :n], ob)
    # the whole path on the loaded pack: detect -> align -> embed -> match against a gallery enrolled from its own embeddings
    out = engine.process_frames(frames, max_faces=3, flags=1)
    G = out["emb"].reshape(-1, 512)
    engine.gallery_set(G)
    again = engine.process_frames(frames, max_faces=3, flags=1)
    assert np.array_equal(again["match_idx"].reshape(-1), np.arange(len(G))) and again["match_cos"].min() > 0.995
    engine.gallery_set(np.zeros((0, 512), np.float32))


def test_jpeg_stills_decode_on_the_device(engine):
    """baseline JPEG stills -> frp_upload_jpeg_async (entropy decoding on host threads, dequantisation /
    inverse DCT / chroma upsampling / YCbCr -> BGR by HIP kernels on the copy stream) -> the resident frame buffer, against
    the decode the reference performs (PIL: face_recognition.load_image_file, face_service.py:139): EQUAL, bit for bit, on the
    committed stills (4:2:0 / 4:2:2 / 4:4:4 / grayscale, odd sizes, optimised tables, restart intervals) and on camera-size
    stills written on the spot; mixed geometry and files outside the decoder's scope are refused."""
    import glob
    import io
    import os
    from PIL import Image
    from frp_amd.native import FrpError
    raw, blob = get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))
    engine.load_weights(blob)

    def device_decode(jpegs):
        engine.upload_jpeg_async(jpegs)
        engine.swap_frames()
        info = __import__("frp_amd").native.jpeg_info(jpegs[0])
        engine.detect_resident((info["height"], info["width"]), max_faces=2, det_thresh=0.5)
        return engine.det_source()

    def pil_bgr(data):
        return np.array(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1]

    here = os.path.dirname(os.path.abspath(__file__))
    stills = sorted(glob.glob(os.path.join(here, "golden", "stills", "*.jpg")))
    assert len(stills) == 8
    for path in stills:
        data = open(path, "rb").read()
        got = device_decode([data, data, data])                              # a batch of three: every image of it
        ref = pil_bgr(data)
        assert got.shape == (3,) + ref.shape
        for b in range(3):
            assert np.array_equal(got[b], ref), (os.path.basename(path), int(np.abs(got[b].astype(int) - ref).max()))
    rng = np.random.default_rng(9)
    for (h, w, kw) in ((1080, 1920, dict(quality=88)), (720, 1280, dict(quality=95, subsampling=0)), (481, 643, dict(quality=70, subsampling=1))):
        imgs = []
        for i in range(2):
            base = rng.normal(120, 50, (h // 16 + 1, w // 16 + 1, 3)).repeat(16, 0).repeat(16, 1)[:h, :w]
            b = io.BytesIO()
            Image.fromarray(np.clip(base + rng.normal(0, 5, (h, w, 3)), 0, 255).astype(np.uint8)).save(b, "JPEG", **kw)
            imgs.append(b.getvalue())
        got = device_decode(imgs)
        for b in range(2):
            assert np.array_equal(got[b], pil_bgr(imgs[b])), (h, w, kw)
    # awkward sizes (not a multiple of the MCU in either direction, a single MCU column, one pixel more than whole MCUs), every
    # sampling, grayscale, restart intervals, no Huffman tables in the file (Motion-JPEG frames: the Annex K tables implied)
    def strip_dht(d):
        out, i = bytearray(d[:2]), 2
        while True:
            m_, L = d[i + 1], (d[i + 2] << 8) | d[i + 3]
            if m_ == 0xDA:
                return bytes(out + d[i:])
            if m_ != 0xC4:
                out += d[i:i + 2 + L]
            i += 2 + L
    for (h, w) in ((33, 47), (64, 66), (65, 64), (97, 16), (129, 255)):
        img = np.clip(rng.normal(120, 60, (h // 4 + 1, w // 4 + 1, 3)).repeat(4, 0).repeat(4, 1)[:h, :w] + rng.normal(0, 8, (h, w, 3)), 0, 255).astype(np.uint8)
        for kw in (dict(quality=90, subsampling=0), dict(quality=80, subsampling=1), dict(quality=85, subsampling=2),
                   dict(quality=75, subsampling=2, restart_marker_blocks=2), dict(quality=92, gray=True), dict(quality=85, subsampling=2, bare=True)):
            kw = dict(kw)
            gray, bare = kw.pop("gray", False), kw.pop("bare", False)
            b = io.BytesIO()
            (Image.fromarray(img).convert("L") if gray else Image.fromarray(img)).save(b, "JPEG", **kw)
            data = strip_dht(b.getvalue()) if bare else b.getvalue()
            got = device_decode([data, data])
            assert np.array_equal(got[0], pil_bgr(data)) and np.array_equal(got[1], got[0]), (h, w, kw, gray, bare)
    # refused, nothing staged: mixed geometry, a progressive file, not a JPEG
    small = open(stills[0], "rb").read()
    with pytest.raises(FrpError, match="geometry"):
        engine.upload_jpeg_async([imgs[0], small])
    b = io.BytesIO()
    Image.fromarray(np.zeros((32, 32, 3), np.uint8)).save(b, "JPEG", progressive=True)
    with pytest.raises(FrpError, match="progressive"):
        engine.upload_jpeg_async([b.getvalue()])
    with pytest.raises(FrpError):
        engine.upload_jpeg_async([b"not a jpeg at all"])


def test_jpeg_entropy_decode_on_the_device_for_restart_interval_streams(fresh_engine):
    # (the path is opt-in - FRP_JPEG_DEVICE_HUFFMAN=1, read once per process: tests/conftest.py sets it for the GPU session; the
    # host-decoder tests above use frames without restart intervals or too few of them, which never take it)
    """frames that carry restart intervals (RSTn every MCU row - what most Motion-JPEG cameras emit -
    or every few MCUs) have their ENTROPY decode on the device too: one thread per interval (jpeg_huffman_kernel), the compressed
    scans over PCIe instead of coefficients.  Against PIL, bit for bit: every sampling, grayscale, frames without a DHT segment,
    intervals of whole MCU rows / a few MCUs / one MCU, sizes that are no multiple of the MCU, 1080p; the path really ran
    (`jpeg_device_batches`); a frame without intervals in the batch, or too few intervals to fill a wave, takes the host decoder
    (same pixels); damaged streams - a truncated interval, a flipped byte, a marker out of sequence - are refused BY THIS CALL,
    nothing staged."""
    import io
    from PIL import Image
    from frp_amd import native
    from frp_amd.native import FrpError
    engine = fresh_engine
    raw, blob = get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))
    engine.load_weights(blob)
    rng = np.random.default_rng(21)

    def device_decode(jpegs):
        engine.upload_jpeg_async(jpegs)
        engine.swap_frames()
        info = native.jpeg_info(jpegs[0])
        engine.detect_resident((info["height"], info["width"]), max_faces=2, det_thresh=0.5)
        return engine.det_source()

    def pil_bgr(data):
        return np.array(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1]

    def still(h, w, gray=False, **kw):
        img = np.clip(rng.normal(120, 55, (h // 8 + 1, w // 8 + 1, 3)).repeat(8, 0).repeat(8, 1)[:h, :w] + rng.normal(0, 7, (h, w, 3)), 0, 255).astype(np.uint8)
        b = io.BytesIO()
        (Image.fromarray(img).convert("L") if gray else Image.fromarray(img)).save(b, "JPEG", **kw)
        return b.getvalue()

    def strip_dht(d):
        out, i = bytearray(d[:2]), 2
        while True:
            m_, L = d[i + 1], (d[i + 2] << 8) | d[i + 3]
            if m_ == 0xDA:
                return bytes(out + d[i:])
            if m_ != 0xC4:
                out += d[i:i + 2 + L]
            i += 2 + L

    assert os.environ.get("FRP_JPEG_DEVICE_HUFFMAN") == "1"
    n0 = engine.jpeg_device_batches()
    ran = 0
    cases = [(1080, 1920, 4, dict(quality=88, restart_marker_rows=1)), (720, 1280, 6, dict(quality=93, subsampling=0, restart_marker_rows=1)),
             (481, 643, 5, dict(quality=70, subsampling=1, restart_marker_rows=2)), (243, 517, 8, dict(quality=80, subsampling=2, restart_marker_blocks=3)),
             (97, 130, 3, dict(quality=90, subsampling=2, restart_marker_blocks=1)), (360, 640, 4, dict(quality=85, gray=True, restart_marker_rows=1)),
             (360, 640, 4, dict(quality=85, subsampling=2, restart_marker_rows=1, bare=True))]
    for (h, w, B, kw) in cases:
        kw = dict(kw)
        bare = kw.pop("bare", False)
        imgs = [still(h, w, **kw) for _ in range(B)]
        if bare:
            imgs = [strip_dht(d) for d in imgs]
        assert all(native.jpeg_info(d)["restart_interval"] > 0 for d in imgs)
        got = device_decode(imgs)
        for b in range(B):
            ref = pil_bgr(imgs[b])
            assert np.array_equal(got[b], ref), (h, w, kw, b, int(np.abs(got[b].astype(int) - ref).max()))
        ran += 1
        assert engine.jpeg_device_batches() == n0 + ran, (h, w, kw)
    # not this path: one frame of the batch without intervals; a batch with fewer than 64 intervals in all
    mixed = [still(360, 640, quality=85, restart_marker_rows=1), still(360, 640, quality=85)]
    got = device_decode(mixed)
    assert all(np.array_equal(got[b], pil_bgr(mixed[b])) for b in range(2)) and engine.jpeg_device_batches() == n0 + ran
    few = [still(64, 64, quality=85, restart_marker_rows=1)]
    assert np.array_equal(device_decode(few)[0], pil_bgr(few[0])) and engine.jpeg_device_batches() == n0 + ran
    # damaged streams are refused by the call (the flags of the device decode are read before it returns)
    good = [still(360, 640, quality=85, restart_marker_rows=1) for _ in range(4)]
    d = good[2]
    sos = d.find(b"\xff\xda")
    rst = [i for i in range(sos, len(d) - 1) if d[i] == 0xFF and 0xD0 <= d[i + 1] <= 0xD7]
    assert len(rst) >= 10
    cut = d[:rst[3] + 2 + (rst[4] - rst[3]) // 2] + d[rst[4]:]                  # half of interval 4 is missing
    swapped = bytearray(d)
    swapped[rst[5] + 1], swapped[rst[6] + 1] = d[rst[6] + 1], d[rst[5] + 1]      # RST5 and RST6 exchanged
    for bad in (cut, bytes(swapped), d[:rst[8] + 2 + 5]):
        with pytest.raises(FrpError):
            engine.upload_jpeg_async(good[:2] + [bad] + good[3:])
    # ... and a byte flipped inside an interval gives either an error or a decode - never a hang or a fault; the engine keeps working
    for _ in range(20):
        flip = bytearray(d)
        i = int(rng.integers(rst[0] + 2, len(d) - 4))
        if flip[i] == 0xFF or flip[i - 1] == 0xFF:
            continue
        flip[i] ^= int(rng.integers(1, 256))
        if flip[i] == 0xFF:
            continue
        try:
            engine.upload_jpeg_async(good[:3] + [bytes(flip)])
        except FrpError:
            pass
    got = device_decode(good)
    assert all(np.array_equal(got[b], pil_bgr(good[b])) for b in range(4))


def test_staged_ingest_takes_the_device_decoder_for_jpeg_batches(engine):
    """ingest.StagedIngest: full batches of baseline JPEG stills are decoded on the way to the device, the short last batch and
    a PNG batch by PIL on the host - and every batch gives the results of process_frames on the PIL-decoded frames"""
    import io
    from PIL import Image
    from frp_amd import native
    from frp_amd.ingest import StagedIngest
    raw, blob = get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))
    engine.load_weights(blob)
    rng = np.random.default_rng(23)
    engine.gallery_set(rng.standard_normal((200, 512)).astype(np.float32))
    H, W, B = 120, 168, 3
    srcs, decoded = [], []
    for i in range(8):
        img = np.clip(rng.normal(120, 40, (H // 8, W // 8, 3)).repeat(8, 0).repeat(8, 1) + rng.normal(0, 4, (H, W, 3)), 0, 255).astype(np.uint8)
        b = io.BytesIO()
        Image.fromarray(img).save(b, "PNG" if 3 <= i < 6 else "JPEG", quality=90)
        srcs.append(b.getvalue())
        decoded.append(np.array(Image.open(io.BytesIO(b.getvalue())).convert("RGB")))
    ing = StagedIngest(engine, B, H, W)
    got = list(ing.run([srcs[0:3], srcs[3:6], srcs[6:8]], max_faces=4, flags=native.FLAG_FORCED_K))
    assert [n for n, _ in got] == [3, 3, 2] and ing.device_decoded == 1            # JPEG x 3 on the device; PNG x 3 and the short JPEG batch on the host
    k = 0
    for n, out in got:
        ref = engine.process_frames(np.stack(decoded[k:k + n]), max_faces=4, flags=native.FLAG_FORCED_K | native.FLAG_RGB)
        for key in ("boxes", "kps", "emb", "match_idx", "match_cos", "counts"):
            assert np.array_equal(out[key][:n], ref[key]), key
        k += n
    engine.gallery_set(np.zeros((0, 512), np.float32))
