"""Inputs of the self-synchronising JPEG decoder's tests (tests/test_jpeg_selfsync_host.py on the CPU, tests/test_gpu_jpeg_selfsync.py
on the device): stills written on the spot with PIL - none carries restart markers - and a corpus of damaged files.  Everything is seeded:
both test files see the same bytes."""
import io

import numpy as np
from PIL import Image


def camera_like(rng, h, w):
    """blocky content + sensor noise, as the other JPEG tests draw it"""
    return np.clip(rng.normal(120, 55, (h // 8 + 1, w // 8 + 1, 3)).repeat(8, 0).repeat(8, 1)[:h, :w] + rng.normal(0, 7, (h, w, 3)), 0, 255).astype(np.uint8)


def encode(img, gray=False, **kw):
    b = io.BytesIO()
    (Image.fromarray(img).convert("L") if gray else Image.fromarray(img)).save(b, "JPEG", **kw)
    return b.getvalue()


def strip_dht(d: bytes) -> bytes:
    """the same frame without its DHT segments (Motion-JPEG sources leave them out: T.81 Annex K tables)"""
    out, i = bytearray(d[:2]), 2
    while True:
        m, L = d[i + 1], (d[i + 2] << 8) | d[i + 3]
        if m == 0xDA:
            return bytes(out + d[i:])
        if m != 0xC4:
            out += d[i:i + 2 + L]
        i += 2 + L


def scan_start(d: bytes) -> int:
    i = d.find(b"\xff\xda")
    return i + 2 + ((d[i + 2] << 8) | d[i + 3])


def scan_bytes(d: bytes) -> int:
    """entropy-coded bytes of a file PIL wrote (one scan, EOI as its last two bytes)"""
    assert d.endswith(b"\xff\xd9")
    return len(d) - 2 - scan_start(d)


# (name, height, width, content, save arguments): the seven kinds of stills the decoder's round counts were modelled on, then the
# special cases
KINDS = [
    ("cam420", 97, 130, "camera", dict(quality=88, subsampling=2)),
    ("cam444", 120, 176, "camera", dict(quality=93, subsampling=0)),
    ("cam422", 96, 160, "camera", dict(quality=70, subsampling=1)),
    ("gray", 120, 160, "camera", dict(quality=85, gray=True)),
    ("flat", 128, 192, "flat", dict(quality=85, subsampling=2)),
    ("noise420", 64, 96, "noise", dict(quality=100, subsampling=2)),
    ("noise444", 64, 96, "noise", dict(quality=100, subsampling=0)),
    ("optimized", 97, 130, "camera", dict(quality=80, subsampling=2, optimize=True)),
    ("no_dht", 72, 104, "camera", dict(quality=85, subsampling=2, bare=True)),
    ("tiny", 8, 8, "flat", dict(quality=85, gray=True)),
]


def still(kind, seed=0):
    name, h, w, content, kw = next(k for k in KINDS if k[0] == kind)
    rng = np.random.default_rng([sum(name.encode()), seed])
    kw = dict(kw)
    bare = kw.pop("bare", False)
    if content == "camera":
        img = camera_like(rng, h, w)
    elif content == "flat":
        img = np.full((h, w, 3), 90 + 7 * (seed % 5), np.uint8)
    else:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    d = encode(img, **kw)
    return strip_dht(d) if bare else d


def batch(kind, B):
    return [still(kind, s) for s in range(B)]


def stills_with_scan_length(residues=(0, 1, 15), mod=16):
    """one small 4:2:0 still per residue of the scan length modulo 16 (0, 1 and S - 1 for every S the decoder takes), found by seed"""
    out, seed = {}, 0
    while len(out) < len(residues):
        rng = np.random.default_rng([77, seed])
        d = encode(camera_like(rng, 40, 56), quality=85, subsampling=2)
        r = scan_bytes(d) % mod
        if r in residues and r not in out:
            out[r] = d
        seed += 1
        assert seed < 2000
    return [out[r] for r in residues]


def all_good_stills():
    """[(name, bytes)]: every generated still of the parity tests, two seeds of the seven kinds"""
    out = [(f"{k[0]}_{s}", still(k[0], s)) for k in KINDS for s in range(2 if k[2] > 8 else 1)]
    out += [(f"len{r}", d) for r, d in zip((0, 1, 15), stills_with_scan_length())]
    return out


def small_still():
    return encode(camera_like(np.random.default_rng(404), 40, 56), quality=85, subsampling=2)


def damaged_corpus():
    """[(what, bytes)] of one small still: cut at every byte, seeded single-byte flips, injected FF xx pairs (about 1,900 files).
    what = "cut@<n>", "flip@<i>", "ff@<i>" - the offset tells whether the headers or the scan took the damage."""
    good = small_still()
    out = [("good", good)]
    out += [(f"cut@{n}", good[:n]) for n in range(len(good))]
    rng = np.random.default_rng(9)
    for _ in range(420):
        bad = bytearray(good)
        i = int(rng.integers(2, len(bad)))
        bad[i] ^= 1 << int(rng.integers(0, 8))
        out.append((f"flip@{i}", bytes(bad)))
    for _ in range(300):
        bad = bytearray(good)
        i = int(rng.integers(2, len(bad) - 2))
        bad[i:i + 2] = bytes([0xFF, int(rng.choice([0x00, 0xC0, 0xC4, 0xD0, 0xD3, 0xD9, 0xDA, 0xDB, 0xDD, 0xFF, 0x01, int(rng.integers(0, 256))]))])
        out.append((f"ff@{i}", bytes(bad)))
    return out
