"""The self-synchronising JPEG entropy decoder on the device (csrc/jpeg_selfsync.hip; frp.h: frp_set_jpeg_selfsync,
frp_jpeg_selfsync_coefficients): scans WITHOUT restart markers decoded by thousands of threads, equal to the serial decode.  Coefficients
against the host decoder, pixels through the product path against PIL, damaged files against the host decoder's verdict, and the staging
discipline next to the other ingest kinds.  The same routines on the CPU, under sanitizers: tests/test_jpeg_selfsync_host.py."""
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_selfsync_cases as cases
from conftest import get_raw_and_blob
from frp_amd import native
from frp_amd.native import FrpError

pytestmark = pytest.mark.gpu

# (kind, B): B = 3 .. 8 per geometry, all small
BATCHES = [("cam420", 4), ("cam444", 3), ("cam422", 5), ("gray", 8), ("flat", 3), ("noise420", 3), ("noise444", 3), ("optimized", 4), ("no_dht", 6), ("tiny", 8)]
_REF = {}


def batch_and_reference(kind, B):
    """(files, host decoder's coefficients [B, n], blocks of an image) - decoded once per session"""
    if kind not in _REF:
        files = cases.stills_with_scan_length() if kind == "lengths" else cases.batch(kind, B)
        ref = [native.jpeg_coefficients(d) for d in files]
        assert all(r[0] == ref[0][0] and r[0]["restart_interval"] == 0 for r in ref)
        _REF[kind] = (files, np.stack([r[1] for r in ref]), ref[0][1].size // 64)
    return _REF[kind]


def pil_bgr(jpegs):
    return np.stack([np.ascontiguousarray(np.array(Image.open(io.BytesIO(d)).convert("RGB"))[..., ::-1]) for d in jpegs])


def decode_through_the_product_path(engine, jpegs):
    engine.upload_jpeg_async(jpegs)
    engine.swap_frames()
    info = native.jpeg_info(jpegs[0])
    engine.detect_resident((info["height"], info["width"]), max_faces=2, det_thresh=0.5)
    return engine.det_source()


@pytest.mark.parametrize("subseq_bytes", [16, 128, 0])
def test_coefficients_equal_the_host_decoders(fresh_engine, subseq_bytes):
    """every generated still kind (camera-like 4:2:0 / 4:4:4 / 4:2:2, grayscale, flat, dense noise, optimised tables, no DHT segment, a scan
    shorter than one subsequence, scan lengths = 0, 1, 15 mod 16) at the smallest, a middle and the product's subsequence size: the
    coefficients of every image equal the host decoder's, every block was counted, no flag, rounds <= subsequences.  Dense noise at S = 16
    synchronises so late (hundreds of rounds, several workgroups) that the loop of launches across workgroups has to carry it."""
    engine = fresh_engine
    for kind, B in BATCHES + [("lengths", 3)]:
        files, ref, blocks = batch_and_reference(kind, B)
        coef, stats = engine.jpeg_selfsync_coefficients(files, subseq_bytes)
        print(kind, subseq_bytes, stats.tolist())
        assert coef.shape == ref.shape and np.array_equal(coef, ref), (kind, np.argwhere(coef != ref)[:4].tolist())
        S = subseq_bytes
        assert stats[:, 0].tolist() == [max(1, -(-cases.scan_bytes(d) // S)) for d in files] if subseq_bytes else (stats[:, 0] >= 1).all()
        assert (stats[:, 1] <= stats[:, 0]).all() and (stats[:, 2] == blocks).all() and (stats[:, 3] == 0).all(), (kind, stats.tolist())
        if kind == "noise444" and subseq_bytes == 16:
            assert (stats[:, 0] > 2 * 256).all() and (stats[:, 1] > 64).all(), stats.tolist()


def test_parity_entry_refuses_what_it_does_not_cover(fresh_engine):
    engine = fresh_engine
    files, _, _ = batch_and_reference("cam420", 4)
    rst = cases.encode(cases.camera_like(np.random.default_rng(1), 97, 130), quality=88, subsampling=2, restart_marker_rows=1)
    for bad in (17, 8, 2048, -16):
        with pytest.raises(FrpError, match="subseq_bytes"):
            engine.jpeg_selfsync_coefficients(files, bad)
    with pytest.raises(FrpError, match="restart intervals"):
        engine.jpeg_selfsync_coefficients([rst, rst])
    with pytest.raises(FrpError, match="restart intervals"):
        engine.jpeg_selfsync_coefficients([files[0], rst])
    with pytest.raises(FrpError, match="JPEG 1"):
        engine.jpeg_selfsync_coefficients([files[0], cases.still("cam444")])              # another geometry
    with pytest.raises(FrpError, match="JPEG 0"):
        engine.jpeg_selfsync_coefficients([b"not a jpeg at all"])
    assert engine.jpeg_selfsync_batches() == 0 and engine.jpeg_device_batches() == 0


def test_pixels_through_the_product_path_equal_pil(fresh_engine):
    """set_jpeg_selfsync(True): upload_jpeg_async -> swap_frames -> the detector's source equals PIL's BGR bit for bit, for the generated
    geometries and one batch of 4 x 1080p; its own counter advances by one per batch and the restart-interval counter does not move.  Off
    (the default): the same pixels from the host decoder, neither counter moves.  Batches with restart intervals and mixed batches route as
    before under either setting."""
    engine = fresh_engine
    raw, blob = get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))
    engine.load_weights(blob)
    rng = np.random.default_rng(31)
    hd = [cases.encode(cases.camera_like(rng, 1080, 1920), quality=88, subsampling=2) for _ in range(4)]
    batches = [batch_and_reference(kind, B)[0] for kind, B in BATCHES] + [hd]
    want = [pil_bgr(j) for j in batches]
    assert engine.jpeg_selfsync_batches() == 0 and engine.jpeg_device_batches() == 0
    for j, w in zip(batches, want):                                                       # the default: the host decoder
        assert np.array_equal(decode_through_the_product_path(engine, j), w)
    assert engine.jpeg_selfsync_batches() == 0 and engine.jpeg_device_batches() == 0
    engine.set_jpeg_selfsync(True)
    for n, (j, w) in enumerate(zip(batches, want)):
        got = decode_through_the_product_path(engine, j)
        assert np.array_equal(got, w), (n, int(np.abs(got.astype(int) - w).max()))
        assert engine.jpeg_selfsync_batches() == n + 1 and engine.jpeg_device_batches() == 0
    done = len(batches)
    # restart intervals (189 of them: the one-thread-per-interval decoder takes the batch), and a mixed batch (the host decoder)
    img = [cases.camera_like(rng, 97, 130) for _ in range(3)]
    with_rst = [cases.encode(i, quality=88, subsampling=2, restart_marker_blocks=1) for i in img]
    mixed = [with_rst[0], cases.encode(img[1], quality=88, subsampling=2)]
    mixed2 = mixed[::-1]
    for on, base in ((True, 0), (False, 1)):
        engine.set_jpeg_selfsync(on)
        assert np.array_equal(decode_through_the_product_path(engine, with_rst), pil_bgr(with_rst))
        assert engine.jpeg_device_batches() == base + 1 and engine.jpeg_selfsync_batches() == done
        for m in (mixed, mixed2):
            assert np.array_equal(decode_through_the_product_path(engine, m), pil_bgr(m))
        assert engine.jpeg_device_batches() == base + 1 and engine.jpeg_selfsync_batches() == done


def test_damaged_files_get_the_host_decoders_verdict(fresh_engine):
    """about 40 seeded truncations, bit flips and injected FF xx pairs in the SCAN of one small still - files the sanitizer harness has
    decoded without a report (tests/test_jpeg_selfsync_host.py: the same corpus) - as image 2 of a batch of 4: the call accepts or refuses as
    the host decoder does on that file; a refusal names "JPEG 2", stages nothing, and the good batch behind it decodes bit for bit."""
    engine = fresh_engine
    raw, blob = get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))
    engine.load_weights(blob)
    engine.set_jpeg_selfsync(True)
    good = cases.stills_with_scan_length()
    want = pil_bgr(good)
    first = cases.scan_start(cases.small_still())
    corpus = [(w, d) for w, d in cases.damaged_corpus() if w != "good" and int(w.split("@")[1]) >= first + 2]
    pick = np.random.default_rng(12).choice(len(corpus), 40, replace=False)
    verdicts = []
    for n in pick:
        what, bad = corpus[int(n)]
        try:
            native.jpeg_coefficients(bad)
            host_accepts = True
        except FrpError:
            host_accepts = False
        verdicts.append(host_accepts)
        files = good[:2] + [bad] + good[2:]
        n0 = engine.jpeg_selfsync_batches()
        if host_accepts:
            got = decode_through_the_product_path(engine, files)
            assert np.array_equal(got[[0, 1, 3]], want), what
            assert engine.jpeg_selfsync_batches() == n0 + 1
            coef, stats = engine.jpeg_selfsync_coefficients(files, 16)
            assert np.array_equal(coef[2], native.jpeg_coefficients(bad)[1]) and (stats[:, 3] == 0).all(), what
        else:
            with pytest.raises(FrpError, match="JPEG 2"):
                engine.upload_jpeg_async(files)
            with pytest.raises(FrpError, match="no staged frames"):
                engine.swap_frames()
            with pytest.raises(FrpError, match="JPEG 2") as e:
                engine.jpeg_selfsync_coefficients(files, 16)
            assert e.value.stats[:, 3].tolist() == [0, 0, 1, 0], what
            assert engine.jpeg_selfsync_batches() == n0
            assert np.array_equal(decode_through_the_product_path(engine, good), want), what
    assert verdicts.count(True) >= 3 and verdicts.count(False) >= 10, verdicts
    assert engine.jpeg_device_batches() == 0


def test_selfsync_batches_stage_next_to_every_other_ingest_kind(fresh_engine):
    """The overlapped loop upload(t + 1) / process(t) with another ingest kind for every consecutive batch - raw frames, JPEG on host threads
    (the setting off), restart-interval JPEG on the device, self-synchronising decode (the setting on) - in two sizes, so that every
    buffer grows while a pass is in flight and is reused at the smaller size, with one refused self-sync batch on the way.  Every accepted
    batch gives the results of a plain process_frames call on PIL's pixels; both counters advance by exactly their own batches."""
    engine = fresh_engine
    rng = np.random.default_rng(78)
    raw, blob = get_raw_and_blob((1, 2, 2, 2), (1, 1, 1, 1))
    engine.load_weights(blob)
    engine.gallery_set(rng.standard_normal((200, 512)).astype(np.float32))
    K, flags = 3, native.FLAG_FORCED_K

    def stills(B, H, W, **kw):
        return [cases.encode(cases.camera_like(rng, H, W), quality=88, subsampling=2, **kw) for _ in range(B)]

    small, large = (4, 64, 96), (3, 96, 160)
    kinds = [("raw", small), ("selfsync", small), ("jpeg-host", small), ("selfsync", small), ("jpeg-device", small), ("selfsync", large), ("jpeg-host", large),
             ("jpeg-device", large), ("selfsync", small), ("raw", small), ("refused", small), ("selfsync", small), ("jpeg-host", small), ("selfsync", large)]
    assert all(a[0] != b[0] for a, b in zip(kinds[:-1], kinds[1:]))
    batches = []
    for kind, shape in kinds:
        if kind == "raw":
            f = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
            batches.append((kind, f, f))
        elif kind == "refused":
            j = stills(*shape)
            cut = j[2][:cases.scan_start(j[2]) + cases.scan_bytes(j[2]) // 2] + b"\xff\xd9"          # half of the scan is missing
            batches.append((kind, j[:2] + [cut] + j[3:], None))
        else:
            j = stills(*shape, **(dict(restart_marker_blocks=1) if kind == "jpeg-device" else {}))
            assert native.jpeg_info(j[0])["restart_interval"] == (1 if kind == "jpeg-device" else 0)
            batches.append((kind, j, pil_bgr(j)))
    want = [None if f is None else engine.process_frames(f, max_faces=K, flags=flags) for _, _, f in batches]
    d0, s0 = engine.jpeg_device_batches(), engine.jpeg_selfsync_batches()
    counted = {"jpeg-device": 0, "selfsync": 0}

    def upload(i):
        kind, src, _ = batches[i]
        engine.set_jpeg_selfsync(kind in ("selfsync", "refused"))
        if kind == "refused":
            with pytest.raises(FrpError, match="JPEG 2"):
                engine.upload_jpeg_async(src)
            return upload(i + 1)
        if kind == "raw":
            engine.upload_frames_async(src)
        else:
            engine.upload_jpeg_async(src)
            if kind in counted:
                counted[kind] += 1
        assert (engine.jpeg_device_batches(), engine.jpeg_selfsync_batches()) == (d0 + counted["jpeg-device"], s0 + counted["selfsync"]), (i, kind)
        return i

    cur = upload(0)
    engine.swap_frames()
    checked = 0
    while cur is not None:
        nxt = upload(cur + 1) if cur + 1 < len(batches) else None                        # overlaps the processing of batch `cur`
        engine.process_resident(max_faces=K, flags=flags)
        got = engine.fetch_results()
        for key in ("boxes", "kps", "scores", "counts", "emb", "match_idx", "match_cos"):
            assert np.array_equal(got[key], want[cur][key]), (cur, batches[cur][0], key)
        checked += 1
        if nxt is not None:
            engine.swap_frames()
        cur = nxt
    assert checked == len(batches) - 1
    assert (engine.jpeg_device_batches(), engine.jpeg_selfsync_batches()) == (d0 + 2, s0 + 6)
