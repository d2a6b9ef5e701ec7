"""Host model of the device clustering sweep (include/frp.h: frp_gallery_cluster; csrc/cluster_kernels.hip), pure numpy over a given
boolean matrix: passes[s, p] says that seed s takes position p - evaluated by the caller with s as the query and p's gallery row as
the column.  Written tile by tile, as the device runs it: candidates, resolve, assign, advance."""
import numpy as np


def cluster_tiled(passes, tile=64):
    """-> (seed_pos [n] int32: the position of the seed that took each position, == p for a seed; the number of seeds)"""
    passes = np.asarray(passes, dtype=bool)
    n = passes.shape[0]
    assert passes.shape == (n, n) and tile >= 1
    seed_pos = np.full(n, -1, np.int32)
    cursor, n_seeds = 0, 0
    while True:
        # 1. candidates: the first `tile` unassigned positions at or after the cursor, ascending
        cand = [p for p in range(cursor, n) if seed_pos[p] < 0][:tile]
        if not cand:
            break
        # 2. resolve: A[t] = the candidates u that candidate t passes; c_t is a seed iff no earlier seed of this tile passed it
        A = [sum(1 << u for u, cu in enumerate(cand) if passes[ct, cu]) for ct in cand]
        seeds, taken = [], 0
        for t in range(len(cand)):
            if not (taken >> t) & 1:
                seeds.append(t)
                taken |= A[t]
        for t in seeds:                      # a seed always gets itself, whatever its own score is
            seed_pos[cand[t]] = cand[t]
        n_seeds += len(seeds)
        # 3. assign: every unassigned position takes the first seed of the tile, in tile order, that passes it
        for p in range(n):
            if seed_pos[p] >= 0:
                continue
            for t in seeds:
                if passes[cand[t], p]:
                    seed_pos[p] = cand[t]
                    break
        # 4. advance: past the last candidate
        cursor = cand[-1] + 1
    return seed_pos, n_seeds


def cluster_tiled_fast(passes, tile=64):
    """cluster_tiled with step 3 vectorised (the same sweep; for the larger expected matrices of the GPU tests)"""
    passes = np.asarray(passes, dtype=bool)
    n = passes.shape[0]
    seed_pos = np.full(n, -1, np.int32)
    cursor, n_seeds = 0, 0
    while cursor < n:
        cand = (cursor + np.nonzero(seed_pos[cursor:] < 0)[0])[:tile]
        if cand.size == 0:
            break
        sub = passes[np.ix_(cand, cand)]
        seeds, taken = [], np.zeros(cand.size, bool)
        for t in range(cand.size):
            if not taken[t]:
                seeds.append(t)
                taken |= sub[t]
        spos = cand[seeds]
        seed_pos[spos] = spos
        n_seeds += len(seeds)
        block = passes[spos] & (seed_pos < 0)[None, :]
        hit = block.any(axis=0)
        seed_pos[hit] = spos[block.argmax(axis=0)[hit]]
        cursor = int(cand[-1]) + 1
    return seed_pos, n_seeds


def clusters_dict(names, seed_pos):
    """the reference's dict from the labels: cluster k is the k-th seed; the seed, then its members in ascending position"""
    out, key = {}, {}
    for p, s in enumerate(seed_pos):
        if s == p:
            key[p] = f"cluster_{len(out)}"
            out[key[p]] = [names[p]]
    for p, s in enumerate(seed_pos):
        if s != p:
            out[key[int(s)]].append(names[p])
    return out
