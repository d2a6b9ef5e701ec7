"""CPU half of the decode kernel's planted cases (tests/decode_cases.py): shown with the host model alone - oracle.network.decode_nms,
the reference the kernel is held to, and tests/decode_model.py, the integer restatement of the selection - that every case is what
its name says, that the list covers the digits the radix select walks, that the predicate of tests/test_gpu_decode_exact.py
rejects every mutant of the model on at least one case, and that poisoning the values the kernel must not read changes nothing."""
import numpy as np
import pytest

import decode_cases as dc
import decode_model as dm
from decode_cases import CAP, CASES, case, reference
from test_gpu_decode_exact import same_detections

f16, f32 = np.float16, np.float32
CANVASES = (dc.SMALL, dc.ODD, dc.OVER, dc.WIDE, dc.DIGITS)


def _logits(c, b=0):
    return dm.anchor_values(c["heads"], b, c["canvas_hw"])[:, 0]


def _n_candidates(c, b=0):
    return len(dm.candidates(_logits(c, b), dm.thresholds(c)[0]))


def _out(c, b=0):
    r = reference(c)
    return r["anchor_idx"][b, :r["counts"][b]].tolist()


def _iou64(a, b):
    """the +1-pixel IoU of box arrays [n, 4] x [m, 4] in float64 (the planted coordinates are exact in it)"""
    a, b = np.asarray(a, np.float64)[:, None, :], np.asarray(b, np.float64)[None, :, :]
    w = np.maximum(0, np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0]) + 1)
    h = np.maximum(0, np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1]) + 1)
    area = lambda t: (t[..., 2] - t[..., 0] + 1) * (t[..., 3] - t[..., 1] + 1)
    return w * h / (area(a) + area(b) - w * h)


def _over_cap_frames():
    """(case, frame, cut key) of every frame with more than 1024 candidates"""
    out = []
    for c in CASES:
        for b in range(c["heads"][0].shape[0]):
            T = dm.cut_key(_logits(c, b), dm.thresholds(c)[0])
            if T is not None:
                out.append((c, b, T))
    return out


def test_case_list_is_small_and_well_formed():
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names)
    for c in CASES:
        H, W = c["canvas_hw"]
        assert c["canvas_hw"] in CANVASES and H % 32 == 0 and W % 32 == 0
        B = c["heads"][0].shape[0]
        assert 1 <= B <= 6 and 1 <= c["K"] <= 128 and isinstance(c["det_thresh"], f32) and isinstance(c["nms_iou"], f32)
        for h, s in zip(c["heads"], dc.STRIDES):
            assert h.dtype == f16 and h.shape == (B, H // s, W // s, 32) and not h.flags.writeable
            assert not h[..., 30:].any()                       # as the detector leaves them
    assert [dc.n_anchors(hw) for hw in CANVASES] == [42, 252, 1050, 4158, 12852]
    assert sum(1 for i in range(4158) if i >= 4096) == 62 and dc.level_dims(dc.WIDE) == [(36, 44), (18, 22), (9, 11)]
    assert sum(c["canvas_hw"] == dc.DIGITS for c in CASES) == 2            # the one larger canvas: the two cases that need it


@pytest.mark.parametrize("hw", CANVASES)
def test_anchor_slot_is_the_models_order(hw):
    """anchor_slot and anchor_index invert each other, and a marker planted through them alone comes back from the oracle under
    that index, with the box marker_box states"""
    A = dc.n_anchors(hw)
    st = dc.level_starts(hw)
    assert all(dc.anchor_index(hw, *dc.anchor_slot(hw, i)) == i for i in range(A))
    assert [dc.anchor_slot(hw, st[l]) for l in range(3)] == [(l, 0, 0, 0) for l in range(3)]
    for l, (h, w) in enumerate(dc.level_dims(hw)):
        assert dc.anchor_slot(hw, st[l + 1] - 1) == (l, h - 1, w - 1, 1)
    picks = sorted({0, st[1] - 1, st[1], st[2] - 1, st[2], A - 1, A // 3, A // 2 + 1})
    heads = dc.quiet_heads(1, hw)
    for j, i in enumerate(picks):
        dc.plant_marker(heads, 0, i, f16(1 + j))
    boxes, _, _, idx = dc.onet.decode_nms([h[0] for h in heads], 0.5, 0.4, 16)
    assert idx.tolist() == picks[::-1]
    assert np.array_equal(boxes, np.array([dc.marker_box(hw, i) for i in picks[::-1]], f32))


def test_the_two_kinds_of_box_are_what_the_docstring_says():
    """bulk boxes overlap each other far above every bound used, markers are disjoint from each other and all but disjoint from a
    bulk box - on whole canvases, not only for the planted anchors"""
    for hw in (dc.OVER, dc.WIDE):
        A = dc.n_anchors(hw)
        m = np.array([dc.marker_box(hw, i) for i in range(A)])
        for lo in range(0, A, 512):
            ov = _iou64(m[lo:lo + 512], m)
            ov[np.arange(len(ov)), lo + np.arange(len(ov))] = 0
            assert not ov.any()
    for hw in CANVASES:
        A = dc.n_anchors(hw)
        st = dc.level_starts(hw)
        corners = [0, st[1] - 1, st[1], st[2] - 1, st[2], A - 1, dc.anchor_index(hw, 0, 0, hw[1] // 8 - 1, 0), dc.anchor_index(hw, 0, hw[0] // 8 - 1, 0, 1)]
        bulk = np.array([dc.bulk_box(hw, i) for i in corners])
        assert _iou64(bulk, bulk).min() > 0.7 > max(float(c["nms_iou"]) for c in CASES) + 0.2
        assert _iou64(bulk, np.array([dc.marker_box(hw, i) for i in corners])).max() < 1e-6
    for c in CASES:                                            # every planted marker has the box the rule gives
        if c["markers"]:
            r = reference(c)
            for b in range(len(r["counts"])):
                for k in range(r["counts"][b]):
                    i = int(r["anchor_idx"][b, k])
                    if i in c["markers"]:
                        assert np.array_equal(r["boxes"][b, k], np.array(dc.marker_box(c["canvas_hw"], i), f32))


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_the_model_equals_the_reference(c):
    assert same_detections(dm.decode(c), reference(c)) == []


def test_levels():
    c = case("levels")
    st = dc.level_starts(dc.WIDE)
    assert st == [0, 3168, 3960, 4158] and {0, 3167, 3168, 3959, 3960, 4157} <= set(c["markers"]) and len(c["markers"]) == 14
    slots = [dc.anchor_slot(dc.WIDE, i) for i in c["markers"]]
    for l, (h, w) in enumerate(dc.level_dims(dc.WIDE)):
        assert h != w
        assert any(s[0] == l and s[2] == w - 1 and 0 < s[1] < h - 1 for s in slots)        # last column, an inner row
        assert any(s[0] == l and s[1] == h - 1 and 0 < s[2] < w - 1 for s in slots)        # last row, an inner column
    assert (1, 5, 7, 0) in slots and (1, 5, 7, 1) in slots
    out = _out(c)
    assert _n_candidates(c) == 14 and sorted(out) == c["markers"] and out != sorted(out) and out != sorted(out, reverse=True)
    lg = [float(dc.logit_of(c["heads"], 0, i)) for i in out]
    assert len(set(lg)) == 14 and lg == sorted(lg, reverse=True)
    vals = dm.anchor_values(c["heads"], 0, dc.WIDE)[c["markers"]].astype(f32)
    assert (vals[:, 1:5] < 0).any() and (vals[:, 5:] < 0).any() and (vals[:, 5:] > 0).any()
    assert all(v[1] != v[3] and v[2] != v[4] and abs(v[1]) != abs(v[3]) and abs(v[2]) != abs(v[4]) for v in vals)   # asymmetric distances
    assert len({v[1:].tobytes() for v in vals}) == 14


def test_cap_boundaries():
    exact, unique, tied = case("cap_exact"), case("cap_plus_one_unique"), case("cap_plus_one_tied")
    assert [_n_candidates(c) for c in (exact, unique, tied)] == [1024, 1025, 1025]
    lt = dm.thresholds(exact)[0]
    for c in (exact, unique, tied):
        cand = set(dm.candidates(_logits(c), lt).tolist())
        assert 0 not in cand and 1049 not in cand and len(cand) < dc.n_anchors(dc.OVER)
    assert dm.cut_key(_logits(exact), lt) is None
    bulk = _out(exact)[1]
    assert _out(exact) == [1037, bulk, 900, 5] and bulk not in exact["markers"]
    assert _out(unique) == [1037, _out(unique)[1], 900]                      # 5, alone at the bottom and at a low index, is cut
    lg = _logits(unique)
    assert lg[5] < lg[900] == np.sort(lg[dm.candidates(lg, lt)])[1]
    assert _out(tied) == [1037, _out(tied)[1], 20, 5, 300]                   # of 5, 300, 900 at the bottom the highest index is cut
    lg = _logits(tied)
    assert lg[5] == lg[300] == lg[900] == lg[dm.candidates(lg, lt)].min() and (lg[dm.candidates(lg, lt)] == lg[5]).sum() == 3


def test_tie_cuts():
    c = case("tie_cut")
    lg = _logits(c)
    assert _n_candidates(c) == 4158 and len(set(lg.tolist())) == 1 and c["markers"] == list(range(1020, 1028))
    assert _out(c) == [0, 1020, 1021, 1022, 1023]
    assert 0xFFFFF - (dm.cut_key(lg, dm.thresholds(c)[0]) & 0xFFFFF) == 1023
    c = case("ulp_above_4096")
    lg = _logits(c)
    assert set(lg[:4096].tolist()) == {2.0} and set(lg[4096:].view(np.uint16).tolist()) == {0x4001}
    assert 0xFFFFF - (dm.cut_key(lg, dm.thresholds(c)[0]) & 0xFFFFF) == 961
    assert c["markers"] == [960, 961, 962, 963, 4096, 4100] and _out(c) == [4096, 4097, 4100, 960, 961]


def test_negative_over_cap():
    c = case("negative_over_cap")
    lt = dm.thresholds(c)[0]
    lg = _logits(c)
    cand = dm.candidates(lg, lt)
    assert c["det_thresh"] == f32(0.05) and lt < -2.9 and len(cand) == 1500 and (lg[cand] < 0).all()
    bits = lg[cand].view(np.uint16)
    assert set(bits.tolist()) == set(range(0xBC00, 0xBC05)) and min(np.bincount(bits - 0xBC00)) > 100      # ulp steps, ties in each
    order = cand[np.argsort(-dm.keys_of(lg[cand], cand), kind="stable")]
    assert c["markers"] == sorted(order[CAP - 3:CAP + 3].tolist())
    assert lg[order[CAP - 1]] == lg[order[CAP]] and order[CAP - 1] < order[CAP]          # the cut falls inside a tie group
    assert _out(c)[1:] == order[CAP - 3:CAP].tolist() and _out(c)[0] == order[0]
    assert dm.digits_of(dm.cut_key(lg, lt))[0] < 0x800


@pytest.mark.parametrize("name", ["digits_a", "digits_b", "digits_c", "digits_d"])
def test_digits_cases(name):
    c = case(name)
    lg = _logits(c)
    T = dm.cut_key(lg, dm.thresholds(c)[0])
    cut = c["cut_idx"]
    assert 0xFFFFF - (T & 0xFFFFF) == cut and _n_candidates(c) > CAP
    tie = [i for i in c["markers"] if i > cut and lg[i] == lg[cut]]
    low = [i for i in c["markers"] if i < cut and lg[i] < lg[cut]]
    high = [i for i in c["markers"] if lg[i] > lg[cut]]
    assert len(tie) == len(low) == len(high) == 1
    out = _out(c)
    assert out[1:] == high + [cut] and out[0] not in c["markers"]


def test_coverage_of_the_radix_select():
    """the cut's digit in every pass takes all four residues mod 4 (a thread's four bins h3..h0); pass 0 sees cuts in both halves
    (negative and non-negative logits); pass 2 sees a cut in the first wave's bins and one in the last wave's.  With the
    literal three-pass walk giving the cut key on every such frame."""
    frames = _over_cap_frames()
    assert len(frames) >= 12
    digits = [dm.digits_of(T) for _, _, T in frames]
    for p in range(3):
        assert {d[p] % 4 for d in digits} == {0, 1, 2, 3}, p
    assert any(d[0] < 0x800 for d in digits) and any(d[0] >= 0x800 for d in digits)
    assert any(d[2] < 256 for d in digits) and any(d[2] >= 3840 for d in digits)
    assert any(d[1] % 256 != 255 for d in digits)                 # anchors from 4096 on: bits 12..19 of 0xFFFFF - index move
    for c, b, T in frames:
        lg = _logits(c, b)
        cand = dm.candidates(lg, dm.thresholds(c)[0])
        assert dm.radix_select(dm.keys_of(lg[cand], cand)) == T, c["name"]


def test_nms_cases():
    c = case("chain")
    ia, ib, ic = c["planted"]
    assert dm.iou(dc.CHAIN_A, dc.CHAIN_B) == dm.iou(dc.CHAIN_B, dc.CHAIN_C) == f32(275) / f32(525)
    assert dm.iou(dc.CHAIN_A, dc.CHAIN_C) == f32(150) / f32(650)
    assert f32(150) / f32(650) < c["nms_iou"] - f32(0.1) and c["nms_iou"] + f32(0.1) < f32(275) / f32(525)
    d = dm.decode_frame(c, 0, detail=True)
    assert d["order"].tolist() == [ia, ib, ic] and _out(c) == [ia, ic]
    assert np.array_equal(d["all_boxes"], np.array([dc.CHAIN_A, dc.CHAIN_B, dc.CHAIN_C], f32))
    c = case("second_keeper")
    ia, idd, ie, iff = c["planted"]
    d = dm.decode_frame(c, 0, detail=True)
    assert d["order"].tolist() == [ia, idd, ie, iff] and _out(c) == [ia, idd, iff]
    assert np.array_equal(d["all_boxes"], np.array([dc.KEEP_A, dc.KEEP_D, dc.KEEP_E, dc.KEEP_F], f32))
    assert dm.iou(dc.KEEP_A, dc.KEEP_E) == 0 and dm.iou(dc.KEEP_A, dc.KEEP_D) == 0 and dm.iou(dc.KEEP_D, dc.KEEP_E) == f32(280) / f32(520)
    assert all(dm.iou(k, dc.KEEP_F) == 0 for k in (dc.KEEP_A, dc.KEEP_D, dc.KEEP_E))
    c = case("iou_zero")
    ip, iq, ir, is_ = c["planted"]
    assert c["nms_iou"] == 0 and dm.iou(dc.IOU0_P, dc.IOU0_Q) == f32(1) / f32(241) and dm.iou(dc.IOU0_R, dc.IOU0_S) == 0
    assert dc.IOU0_Q[0] == dc.IOU0_P[2] and dc.IOU0_S[0] == dc.IOU0_R[2] + 1
    assert dm.decode_frame(c, 0, detail=True)["order"].tolist() == [ip, iq, ir, is_] and _out(c) == [ip, ir, is_]


def test_the_loop_ends():
    c = case("full_cap_kth_is_last")
    d = dm.decode_frame(c, 0, detail=True)
    assert _n_candidates(c) == CAP and c["K"] == 128 and d["count"] == 128 and d["keep"][-1] == CAP - 1 and d["keep"][0] == 0
    assert dm.decode_frame(c, 0, K=CAP)["count"] == 128                       # exactly 128 boxes are keepable
    assert d["order"][0] == c["first_bulk"] and d["order"][-1] == c["last_pair"][1]
    c = case("full_cap_one_short")
    d = dm.decode_frame(c, 0, detail=True)
    assert _n_candidates(c) == CAP and c["K"] == 128 and d["count"] == 127 == reference(c)["counts"][0] and d["keep"][-1] == CAP - 2
    assert dm.decode_frame(c, 0, K=CAP)["count"] == 127
    assert tuple(d["order"][-2:]) == c["last_pair"] and dm.iou(d["all_boxes"][-2], d["all_boxes"][-1]) == 1
    assert all(dm.iou(d["all_boxes"][k], d["all_boxes"][-1]) == 0 for k in d["keep"][1:-1])   # only candidate 1022 kills 1023
    c = case("k_one")
    assert c["K"] == 1 and _n_candidates(c) == 1050 > CAP and _out(c) == [1037] and _logits(c).argmax() == 1037
    c = case("k_cap_disjoint")
    d = dm.decode_frame(c, 0, detail=True)
    assert _n_candidates(c) == CAP and c["K"] == 128 == reference(c)["counts"][0] and d["keep"].tolist() == list(range(128))
    assert dm.decode_frame(c, 0, K=CAP)["count"] == CAP


def test_signed_zeros():
    c = case("signed_zero")
    lt = dm.thresholds(c)[0]
    assert c["det_thresh"] == f32(0.5) and lt == 0 and not np.signbit(lt)
    bits = _logits(c).view(np.uint16)
    neg, pos = np.flatnonzero(bits == 0x8000), np.flatnonzero(bits == 0x0000)
    assert sorted(neg.tolist() + pos.tolist()) == c["markers"] == _out(c)
    assert neg.min() < pos.min() and neg.max() < pos.max() and neg.max() > pos.min()     # -0.0 low, +0.0 high, and interleaved
    assert (reference(c)["scores"][0, :8] == 0.5).all()
    c = case("signed_zero_at_the_cut")
    lg = _logits(c)
    zeros = np.flatnonzero(lg == 0)
    assert _n_candidates(c) == 1050 and len(zeros) == 50 and (lg[lg != 0] > 0).all()
    assert np.signbit(lg[zeros[:25]]).all() and not np.signbit(lg[zeros[25:]]).any()
    out = _out(c)
    assert out[1:] == zeros[:24].tolist() and out[0] not in zeros                        # 1000 positive logits + 24 zeros by index
    # the keys: equal for the two zeros; the kernel before this list existed keyed +0.0 above -0.0
    assert dm.sortable16([0x0000, 0x8000]).tolist() == [0x8000, 0x8000]
    assert dm.sortable16([0x0000, 0x8000], split_zeros=True).tolist() == [0x8000, 0x7FFF]
    assert dm.sortable16([0x7C00, 0x3C00, 0x0001, 0x8001, 0xBC00, 0xFC00, 0x7E00, 0xFE00]).tolist() == sorted(
        dm.sortable16([0x7C00, 0x3C00, 0x0001, 0x8001, 0xBC00, 0xFC00, 0x7E00, 0xFE00]).tolist(), reverse=True)
    lg = np.array([-0.0, 0.0, 0.0, 0.0], f16)
    assert dm.select(lg, f32(0)).tolist() == [0, 1, 2, 3] and dm.select(lg, f32(0), "signed_zeros_split").tolist() == [1, 2, 3, 0]


def test_nonfinite_boxes():
    c = case("nonfinite_boxes")
    iy, iw, iv, ix, iz = c["planted"]
    r = reference(c)
    assert dm.decode_frame(c, 0, detail=True)["order"].tolist() == [iy, iw, iv, ix, iz] and _out(c) == [iy, iw, ix, iz]
    assert np.isnan(r["boxes"][0, 0]).sum() == 1 and np.isposinf(r["boxes"][0, 2]).sum() == 1 and np.isnan(r["kps"][0, 3]).sum() == 1
    assert np.isfinite(r["boxes"][0, [1, 3]]).all() and np.isfinite(r["kps"][0, :3]).all()
    lg = _logits(c)
    assert np.isnan(lg).sum() == 1 and np.isneginf(lg).sum() == 1 and _n_candidates(c) == 5


def test_mixed_batch():
    c = case("mixed_batch")
    B = c["heads"][0].shape[0]
    assert B == 6 and [_n_candidates(c, b) for b in range(B)] == [0, 1, 1024, 4158, 3, 3000] == c["frame_candidates"]
    assert reference(c)["counts"].tolist() == [0, 1, 6, 5, 2, 4]
    assert _out(c, 1) == [4157] and _out(c, 3) == [0, 1020, 1021, 1022, 1023]
    assert set(_out(c, 2)) >= set(c["frame_markers"][2]) and _out(c, 5)[1:] == [i for i in _out(c, 5) if i in c["frame_markers"][5]]
    assert len(_out(c, 5)) == 4 and len(c["frame_markers"][5]) == 6
    # frame 0 differs from every other frame: a kernel that selected on frame 0's logits would return nothing anywhere
    assert same_detections(dm.decode(c, "frame_offset_ignored"), reference(c)) != []


def test_forced_cases():
    c = case("forced_short")
    r = reference(c)
    assert c["forced"] and c["K"] == 64 > dc.n_anchors(c["canvas_hw"]) == 42 == r["counts"][0]
    out = _out(c)
    assert sorted(out) == list(range(42)) and out[-4:] == [3, 17, 33, 40] and out[-7:-4] == [0, 12, 41]
    assert np.isnan(r["scores"][0, 38:42]).all() and (r["scores"][0, 35:38] == 0).all() and (r["anchor_idx"][0, 42:] == -1).all()
    assert out.index(7) + 1 == out.index(30) and out.index(9) + 2 == out.index(21) + 1 == out.index(35)      # ties by index
    c = case("forced_mixed")
    r = reference(c)
    assert c["forced"] and r["counts"].tolist() == [16, 16, 16] and c["heads"][0].shape[0] == 3
    assert np.isnan(_logits(c, 0)).all() and _out(c, 0) == list(range(16)) and np.isnan(r["scores"][0]).all()
    assert np.isnan(_logits(c, 1)).sum() == 126 and _out(c, 1)[0] == 197 and r["scores"][1, 0] == 1.0 and np.isfinite(r["scores"][1]).all()
    assert np.isfinite(_logits(c, 2)).all()


_MUTANT_RESULTS = {}


def _rejections(mutant):
    if mutant not in _MUTANT_RESULTS:
        _MUTANT_RESULTS[mutant] = [c["name"] for c in CASES if same_detections(dm.decode(c, mutant), reference(c)) != []]
    return _MUTANT_RESULTS[mutant]


@pytest.mark.parametrize("mutant", dm.MUTANTS)
def test_every_mutant_is_rejected(mutant):
    hit = _rejections(mutant)
    print(mutant, "rejected by", hit)
    assert hit
    if mutant == "signed_zeros_split":                    # the kernel as it was: these two cases and no other
        assert hit == ["signed_zero", "signed_zero_at_the_cut"]


def test_the_predicate_sees_dead_slots_and_scores():
    c = case("chain")
    want = reference(c)
    for key, slot, value in (("boxes", (0, 5, 2), 1e-30), ("kps", (0, 7, 4, 1), -0.0 + 1e-30), ("scores", (0, 2), 1e-30), ("anchor_idx", (0, 2), 0),
                             ("scores", (0, 0), float(want["scores"][0, 0]) + 3e-6), ("counts", (0,), 3)):
        got = {k: v.copy() for k, v in want.items()}
        got[key][slot] = value
        assert same_detections(got, want) != [], (key, slot)
    c = case("signed_zero")
    got = {k: v.copy() for k, v in reference(c).items()}
    got["scores"][0, 0] = np.nextafter(f32(0.5), f32(1))                   # within 1e-6, but a zero logit's score is exactly 0.5
    assert same_detections(got, reference(c)) == ["scores (0.5 / 1 / 0)"]
    c = case("forced_short")
    got = {k: v.copy() for k, v in reference(c).items()}
    got["scores"][0, 41] = 0.0                                             # NaN in the model
    assert same_detections(got, reference(c)) == ["scores (NaN)"]


@pytest.mark.parametrize("name", dc.POISONED)
def test_poison_changes_nothing(name):
    c = case(name)
    p = dc.poison(c)
    lt = dm.thresholds(c)[0]
    total = 0
    for b in range(c["heads"][0].shape[0]):
        clean, dirty = dm.anchor_values(c["heads"], b, c["canvas_hw"]), dm.anchor_values(p["heads"], b, c["canvas_hw"])
        live = dm.select(clean[:, 0], lt)
        dead = np.setdiff1d(np.arange(len(clean)), live)
        assert clean[:, 0].tobytes() == dirty[:, 0].tobytes() and clean[live].tobytes() == dirty[live].tobytes()
        assert np.isnan(dirty[dead, 1:]).all()
        total += len(dead)
    assert total > 1000 and all(np.isnan(h[..., 30:]).all() for h in p["heads"])
    with np.errstate(all="ignore"):
        want, got = reference(c), reference(p)
    for k in want:
        assert want[k].tobytes() == got[k].tobytes(), k
