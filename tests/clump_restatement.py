"""Dense numpy restatement of LD clumping (gv_ld_clump), written from the definition in include/gvamp.h on top of
ld_restatement and ld_pos_restatement: the adjacency, the clumps as the literal sequential walk, the same clumps by the round scheme of
the device selection (synchronous, counting the rounds), the blocks the launch computes, and the distance of the inputs from the
threshold.  Test infrastructure only."""
import numpy as np

import ld_pos_restatement as lpr


def eligible(p, p1, p2):
    """(E1, E2) as booleans; a NaN p fails both comparisons"""
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return p <= p1, p <= p2


def order_of(p, e):
    """the markers of the boolean set e in ascending p, equal p by ascending index"""
    j = np.nonzero(e)[0]
    return j[np.argsort(np.asarray(p, dtype=np.float64)[j], kind="stable")]


def adjacency(r, poly, pos, radius, chrom, p, p2, r2):
    """M x M booleans: j != k, k in the band of j, both polymorphic, both in E2, r_jk * r_jk >= r2 (fp64 product and comparison)"""
    M = r.shape[0]
    _, e2 = eligible(p, np.inf, p2)
    ok = lpr.in_band_pos(pos, radius, chrom) & ~np.eye(M, dtype=bool)
    ok &= poly[:, None] & poly[None, :] & e2[:, None] & e2[None, :]
    return ok & (r * r >= r2)


def clump_sequential(adj, p, p1, p2):
    """(index_of int64[M], n_index): the definition as a literal loop"""
    M = adj.shape[0]
    e1, e2 = eligible(p, p1, p2)
    index_of = np.full(M, -1, dtype=np.int64)
    n = 0
    for j in order_of(p, e1):
        if index_of[j] != -1:
            continue
        index_of[j] = j
        n += 1
        for k in range(M):
            if e2[k] and adj[j, k] and index_of[k] == -1:
                index_of[k] = j
    return index_of, n


def clump_rounds(adj, p, p1, p2):
    """(index_of, n_index, rounds) by the round scheme, every round reading the states the previous one left: an undecided marker of E1
    becomes claimed if a neighbour of lower rank is an index, an index if every neighbour of lower rank is claimed, and waits otherwise;
    then every marker of E2 takes the index of the lowest rank among its neighbours.  rounds counts the rounds run until one leaves no
    marker waiting (0 with E1 empty)."""
    M = adj.shape[0]
    e1, e2 = eligible(p, p1, p2)
    order = order_of(p, e2)
    rank = np.full(M, -1, dtype=np.int64)
    rank[order] = np.arange(order.size)
    UNDECIDED, INDEX, CLAIMED = 0, 1, 2
    state = np.zeros(M, dtype=np.int64)
    lower = adj & e1[None, :] & (rank[None, :] < rank[:, None])          # [j][k]: k is a neighbour of E1 with a lower rank than j
    rounds = 0
    waiting = bool(e1.any())
    while waiting:
        rounds += 1
        assert rounds <= int(e1.sum()) + 1
        und = e1 & (state == UNDECIDED)
        claimed = und & (lower & (state == INDEX)[None, :]).any(1)
        index = und & ~claimed & ~(lower & (state == UNDECIDED)[None, :]).any(1)
        state[claimed] = CLAIMED
        state[index] = INDEX
        waiting = bool((und & ~claimed & ~index).any())
    index_of = np.full(M, -1, dtype=np.int64)
    is_index = state == INDEX
    for j in np.nonzero(e2)[0]:
        if is_index[j]:
            index_of[j] = j
            continue
        k = np.nonzero(adj[j] & is_index)[0]
        if k.size:
            index_of[j] = k[np.argmin(rank[k])]
    return index_of, int(is_index.sum()), rounds


def blocks_launched(hi, e2):
    """blocks (I, J >= I) of 64 x 64 markers that hold an in-band pair (ld_pos_restatement.block_pairs) and a marker of E2 in both row
    groups"""
    M = hi.size
    nrg = (M + 63) // 64
    holds = [bool(np.asarray(e2)[64 * I:64 * I + 64].any()) for I in range(nrg)]
    n = 0
    for I in range(nrg):
        reach = int(hi[min(64 * I + 63, M - 1)]) // 64 - I
        n += sum(1 for d in range(reach + 1) if holds[I] and holds[I + d])
    return n


def pairs_e2(pos, radius, chrom, e2):
    """the ordered in-band pairs (j, k) with both markers in E2, self included"""
    e2 = np.asarray(e2)
    return int((lpr.in_band_pos(pos, radius, chrom) & e2[:, None] & e2[None, :]).sum())


def margin(r, band, r2):
    """min over the in-band pairs j != k of |r_jk^2 - r2|: how far the inputs are from flipping a comparison"""
    M = r.shape[0]
    ok = band & ~np.eye(M, dtype=bool)
    return float(np.abs(r * r - r2)[ok].min()) if ok.any() else np.inf
