"""CPU: the model of the encoder's optimised Huffman coding (tests/jpeg_optimize_model.py: symbol histogram, jpeg_gen_optimal_table, file
writer) against Pillow's save(optimize=True) - WHOLE FILES, byte for byte - and the properties of the inputs that make the comparison
mean something."""
import numpy as np
import pytest

import jpeg_encode_model as M
import jpeg_optimize_model as OM

CASES = OM.cases()


@pytest.fixture(scope="module")
def hists():
    out = {}
    for name, (rgb, q, ss, r) in CASES.items():
        info, coef, _ = M.forward(rgb, q, ss)
        out[name] = (info, coef, OM.histogram(info, coef, r))
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_whole_files_equal_pillows(name):
    rgb, q, ss, r = CASES[name]
    want = OM.pil_encode(rgb, q, ss, r)
    got = OM.encode(rgb, q, ss, r)
    if got != want:                                          # say which half differs
        gs, gscan = M.split_segments(got)
        ws, wscan = M.split_segments(want)
        assert [m for m, _ in gs] == [m for m, _ in ws], name
        for m in (0xE0, 0xDB, 0xC0, 0xC4, 0xDD, 0xDA):
            assert M.segments_of(gs, m) == M.segments_of(ws, m), (name, hex(m))
        assert gscan == wscan, (name, "scan", len(gscan), len(wscan))
    assert got == want, name
    segs, _ = M.split_segments(got)
    assert [m for m, _ in segs] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4] + ([0xDD] if r else []) + [0xDA]
    assert got != M.pil_encode(rgb, q, ss, r)               # not the Annex K file


def test_the_case_list_is_the_issue_s():
    assert len(CASES) >= 9
    shapes = {n: (c[0].shape[1], c[0].shape[0], c[1], c[2], c[3]) for n, c in CASES.items()}
    for want in [(37, 53, 85, "4:2:0", 0), (64, 48, 95, "4:4:4", 0), (16, 16, 85, "4:2:0", 0), (40, 72, 20, "4:2:0", 3), (33, 17, 100, "4:4:4", 0),
                 (48, 48, 85, "4:2:0", 0), (640, 480, 85, "4:2:0", 0)]:
        assert want in shapes.values(), want
    assert sum(w * h > 64 * 72 for w, h, _, _, _ in shapes.values()) >= 3


def test_inputs_exercise_the_special_symbols(hists):
    def ac(name, t):
        return hists[name][2][OM.AC0 + 256 * t:OM.AC0 + 256 * (t + 1)].astype(np.int64)

    def dc(name, t):
        return hists[name][2][16 * t:16 * t + 16].astype(np.int64)

    # a ZRL is counted somewhere
    assert any(ac(n, t)[0xF0] > 0 for n in CASES for t in (0, 1))
    assert ac("noise_40x72_q20_420_r3", 0)[0xF0] + ac("noise_40x72_q20_420_r3", 1)[0xF0] > 0
    # a block whose coefficient 63 is non-zero has no EOB: fewer EOBs than blocks
    info, coef, h = hists["noise_33x17_q100_444"]
    n_luma = info["mcus_x"] * info["mcus_y"]
    assert dc("noise_33x17_q100_444", 0).sum() == n_luma and ac("noise_33x17_q100_444", 0)[0] < n_luma
    assert (coef[:n_luma * 64].reshape(-1, 64)[:, 63] != 0).any()
    # the flat image: nothing but EOB in both AC tables -> one symbol, a 1-bit code
    for t in (0, 1):
        a = ac("flat_16x16_q85_420", t)
        assert a[0] > 0 and np.count_nonzero(a) == 1
    tabs = OM.tables(hists["flat_16x16_q85_420"][2])
    assert tabs[1] == ([1] + [0] * 15, [0]) and tabs[3] == ([1] + [0] * 15, [0])
    # the grey image: chroma is 128 everywhere -> category 0 and EOB only
    assert np.flatnonzero(dc("grey_48x48_q85_420", 1)).tolist() == [0] and np.flatnonzero(ac("grey_48x48_q85_420", 1)).tolist() == [0]
    assert np.count_nonzero(ac("grey_48x48_q85_420", 0)) > 10
    # the restart interval resets the DC predictions: other DC counts than without it, the same AC counts
    rgb, q, ss, r = CASES["noise_40x72_q20_420_r3"]
    info, coef, h3 = hists["noise_40x72_q20_420_r3"]
    h0 = OM.histogram(info, coef, 0)
    assert r == 3 and not np.array_equal(h3[:32], h0[:32]) and np.array_equal(h3[32:], h0[32:])
    # partial MCUs: a size that is no multiple of 16 at 4:2:0, none of 8 at 4:4:4
    assert any(c[2] == "4:2:0" and (c[0].shape[0] % 16 or c[0].shape[1] % 16) for c in CASES.values())
    assert any(c[2] == "4:4:4" and (c[0].shape[0] % 8 or c[0].shape[1] % 8) for c in CASES.values())
    # every block codes one DC symbol; every block has an EOB or a non-zero last coefficient
    for name in CASES:
        info = hists[name][0]
        blocks = [info["mcus_x"] * info["mcus_y"] * info["h_samp"][0] * info["v_samp"][0], 2 * info["mcus_x"] * info["mcus_y"]]
        for t in (0, 1):
            assert dc(name, t).sum() == blocks[t] and ac(name, t)[0] <= blocks[t], name


def test_optimal_table_invariants_on_the_images(hists):
    for name in CASES:
        h = hists[name][2]
        for k, (bits, vals) in enumerate(OM.tables(h)):
            t = k >> 1
            freq = h[OM.AC0 + 256 * t:OM.AC0 + 256 * (t + 1)] if k & 1 else h[16 * t:16 * t + 16]
            assert sum(bits) == len(vals) == np.count_nonzero(freq), (name, k)
            assert sorted(vals) == np.flatnonzero(freq).tolist(), (name, k)
            # Kraft, the pseudo-symbol's code included: it had the longest length
            longest = max(i + 1 for i in range(16) if bits[i])
            assert sum(b * 2 ** (16 - (i + 1)) for i, b in enumerate(bits)) + 2 ** (16 - longest) <= 2 ** 16, (name, k)


def test_optimal_table_refusals_and_the_smallest_tables():
    with pytest.raises(ValueError):
        OM.gen_optimal_table([0] * 256)
    one = [0] * 256
    one[0x21] = 7
    assert OM.gen_optimal_table(one) == ([1] + [0] * 15, [0x21])
    two = list(one)
    two[3] = 7
    # equal counts: the pseudo-symbol merges with the LARGER symbol first (ties go to the larger index), which gets the longer code
    assert OM.gen_optimal_table(two) == ([1, 1] + [0] * 14, [3, 0x21])
