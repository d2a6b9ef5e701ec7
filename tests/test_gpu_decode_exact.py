"""The detection decode on the device (gather_logits_kernel + decode_nms_kernel through engine.decode_heads) held to
oracle.network.decode_nms on the planted cases of tests/decode_cases.py: every K slot of every frame, dead slots included.

tests/test_decode_inputs.py shows without a GPU what the cases reach - the radix select's boundaries and digits, negative and
signed-zero logits at the cut, the NMS loop's ends, forced top-K above the anchor count, frames of one call on different paths -
and that same_detections, the one predicate used here, rejects every mutant of tests/decode_model.py on at least one case.
Nothing device-specific is imported at module level: the host test imports the predicate from here."""
import numpy as np
import pytest

from decode_cases import CASES, POISONED, case as case_named, frame_of, logit_of, poison, reference

pytestmark = pytest.mark.gpu

SCORE_TOL = 1e-6        # the project's bound for the device's sigmoid against the model's (test_decode_nms_parity)


def same_detections(got, want):
    """the differences between two decode results over ALL K slots, as a list of strings (empty: the same detections).
    counts and anchor_idx equal (-1 from the count on); boxes and kps equal as values with NaN equal to NaN (zeros from the count
    on); scores within SCORE_TOL of the model where the model is finite, NaN where it is NaN, exactly the model's where the model
    gives exactly 0.5, 1.0 or 0.0 (the logits +-0.0, +inf and -inf of the cases), zeros from the count on."""
    diff = []
    for k in ("counts", "anchor_idx"):
        if not np.array_equal(np.asarray(got[k]), np.asarray(want[k])):
            diff.append(k)
    for k in ("boxes", "kps"):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if g.dtype != w.dtype or g.shape != w.shape or not np.array_equal(g, w, equal_nan=True):
            diff.append(k)
    g, w = np.asarray(got["scores"]), np.asarray(want["scores"])
    if g.dtype != w.dtype or g.shape != w.shape:
        return diff + ["scores (shape)"]
    live = np.arange(w.shape[1])[None, :] < np.asarray(want["counts"])[:, None]
    if np.any(g[~live] != 0):
        diff.append("scores (dead slots)")
    nan = live & np.isnan(w)
    if not np.all(np.isnan(g[nan])):
        diff.append("scores (NaN)")
    exact = live & ((w == 0.5) | (w == 1.0) | (w == 0.0))
    if np.any(g[exact] != w[exact]):
        diff.append("scores (0.5 / 1 / 0)")
    fin = live & np.isfinite(w)
    with np.errstate(invalid="ignore"):
        if not np.all(np.abs(g[fin].astype(np.float64) - w[fin].astype(np.float64)) <= SCORE_TOL):
            diff.append("scores")
    return diff


def run(engine, c):
    from frp_amd import native
    return engine.decode_heads(c["heads"], c["canvas_hw"], max_faces=c["K"], det_thresh=float(c["det_thresh"]), nms_iou=float(c["nms_iou"]),
                               flags=native.FLAG_FORCED_K if c["forced"] else 0)


def score_ulps(got, c):
    """the largest distance, in float32 steps, of a live device score from the float64 sigmoid of its anchor's fp16 logit
    (rounded to float32); None without a finite live score.  A record, not a check."""
    worst = None
    for b in range(len(got["counts"])):
        for k in range(int(got["counts"][b])):
            lg = float(logit_of(c["heads"], b, int(got["anchor_idx"][b, k])))
            if not np.isfinite(lg):
                continue
            ref = np.float32(1.0 / (1.0 + np.exp(-lg)))
            d = abs(int(np.float32(got["scores"][b, k]).view(np.int32)) - int(ref.view(np.int32)))
            worst = d if worst is None else max(worst, d)
    return worst


_ULPS = {}


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_decode_equals_the_model(engine, c):
    got = run(engine, c)
    _ULPS[c["name"]] = score_ulps(got, c)
    assert same_detections(got, reference(c)) == []


@pytest.mark.parametrize("name", ["mixed_batch", "forced_mixed"])
def test_frames_of_a_batch_alone_and_again(engine, name):
    """every frame run alone gives its row of the batch's result bit for bit; the batch run twice gives the same bits (the atomic
    gather fills its slots in any order, the sort behind it must not let that show)"""
    c = case_named(name)
    got = run(engine, c)
    assert same_detections(got, reference(c)) == []
    again = run(engine, c)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k
    for b in range(c["heads"][0].shape[0]):
        alone = run(engine, frame_of(c, b))
        for k in got:
            assert alone[k][0].tobytes() == got[k][b].tobytes(), (b, k)


@pytest.mark.parametrize("name", POISONED)
def test_dead_values_are_never_read(engine, name):
    """NaN in channels 30 and 31 and in the 14 box values of every anchor that is no candidate or below the cut: the clean case's bits"""
    c = case_named(name)
    clean, dirty = run(engine, c), run(engine, poison(c))
    for k in clean:
        assert clean[k].tobytes() == dirty[k].tobytes(), k
    assert same_detections(dirty, reference(c)) == []


def test_refusals(engine):
    from frp_amd.native import FrpError
    c = case_named("chain")
    for K in (0, 129):
        with pytest.raises(FrpError):
            engine.decode_heads(c["heads"], c["canvas_hw"], max_faces=K, det_thresh=0.5, nms_iou=0.4)
    for hw in ((64, 100), (72, 96)):
        with pytest.raises(FrpError):
            engine.decode_heads(c["heads"], hw, max_faces=8, det_thresh=0.5, nms_iou=0.4)
    assert same_detections(run(engine, c), reference(c)) == []          # the handle still works


def test_score_ulps_record(engine):
    """prints the largest float32-step distance of the device's scores from the float64 sigmoid over the cases (no bound: the
    bound is SCORE_TOL against the model, in same_detections)"""
    if len(_ULPS) < len(CASES):
        for c in CASES:
            _ULPS.setdefault(c["name"], score_ulps(run(engine, c), c))
    seen = {n: u for n, u in _ULPS.items() if u is not None}
    print(f"decode score ulps vs float64 sigmoid: max {max(seen.values())} ({max(seen, key=seen.get)}) over {len(seen)} cases")
