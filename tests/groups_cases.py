"""Mask patterns of the gallery-group tests over match_cases.exact_case(N, M) (tests/test_gpu_groups.py; their conditions and the mutant
models that must fail on them: tests/test_groups_inputs.py).  Plain numpy, cached, read-only; nothing device-specific is imported.

Row r is PERMITTED for query q iff row_groups[r] & query_groups[q] != 0; the grouped selections are match_model.top1 / topk / within
on masked_scores(): the score matrix with NaN where a row is not permitted.

row_groups(N)     bit r % 3 for every row; additionally bit 5 where r % 64 == 5; additionally bit 6 on row N - 1.
query_groups(M)   bit q % 3; additionally bit 5 for odd q; ALL where q % 11 == 10; only bit 7 (no row has it) where q % 13 == 5; then
                  the first four queries of match_cases (applied last): the anchor query permits bit 2 - row 11, the anchor's copy in the
                  other half-wave, not the anchor row 7 itself -, the negated anchor bit 0, the zero query nothing, the negative query
                  bit 6: row N - 1 alone, the last row of a ragged block, with a score below -0.25 - where a masked element left at 0
                  would win.  M == 1 (the negative query alone): bit 6; query_groups_none(M): every query permits nothing.
"""
import functools

import numpy as np

import match_cases as mc
import match_model as mm

ALL = 0xFFFFFFFF
ANCHOR_COPY = mc.ANCHOR + 4          # row 11: bit 2, where the anchor row 7 has bit 1


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def row_groups(N):
    r = np.arange(N)
    g = (1 << (r % 3)).astype(np.uint32)
    g[r % 64 == 5] |= np.uint32(1 << 5)
    g[N - 1] |= np.uint32(1 << 6)
    return _ro(g)


@functools.lru_cache(maxsize=None)
def query_groups(M):
    if M == 1:
        return _ro(np.array([1 << 6], np.uint32))
    q = np.arange(M)
    g = (1 << (q % 3)).astype(np.uint32)
    g[q % 2 == 1] |= np.uint32(1 << 5)
    g[q % 11 == 10] = np.uint32(ALL)
    g[q % 13 == 5] = np.uint32(1 << 7)
    g[mc.Q_ANCHOR], g[mc.Q_MINUS], g[mc.Q_ZERO], g[mc.Q_NEGATIVE] = 1 << 2, 1 << 0, 0, 1 << 6
    return _ro(g)


@functools.lru_cache(maxsize=None)
def query_groups_none(M):
    return _ro(np.zeros(M, np.uint32))


def permitted(rg, qg):
    """-> bool [M, N]"""
    return (np.asarray(qg, np.uint32)[:, None] & np.asarray(rg, np.uint32)[None, :]) != 0


def masked_scores(S, rg, qg):
    """the score matrix the grouped selections are defined on: NaN where the row is not permitted"""
    return np.where(permitted(rg, qg), np.asarray(S, np.float32), np.float32(np.nan)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def exact_scores(N, M):
    """float32 scores [M, N] of the exact family: the float64 reference rounded once (exact: match_cases)"""
    G, Q = mc.exact_case(N, M)
    return _ro(mm.scores(mc.unit16(G), mc.unit16(Q)).astype(np.float32))
