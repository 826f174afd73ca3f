"""What the tests of the batch products in marker-sharded jobs share (tests/test_sharded_products_cpu.py, tests/test_gpu_sharded_products.py,
tests/test_gpu_sharded_drivers.py): the splits of [0, Mt), the offset arithmetic of the output files restated in numpy, the bit
comparisons, a dense long-double / float64 restatement of Z = A W, and the clump-index fixture of the thresholded score.  Pure numpy: no
GPU, nothing of the library.

Splits.  A split is a list of (S, M) per rank.  `even2` is divide_work (host/utilities.cpp) over two ranks; `uneven3` has a shard of one
marker (one partial tile, fewer markers than any PCA block), a shard of exactly one 64-marker row group and a ragged rest; `empty3` has
a rank without markers between two that have some.

Deviation of a score.  An entry of Z = A W is a sum of M terms whose rounding scales with the magnitude of the column, not of the entry
(an entry may cancel to nearly nothing), so the deviation of a column from its reference is max_n |z_n - ref_n| / max_n |ref_n|; a column
whose reference is zero everywhere must be zero everywhere (deviation 0 or inf).  The bar on it is the rule of DESIGN.md section 15: 16 x
the deviation of the same restatement evaluated in plain float64, never less than 1e-12."""
import numpy as np

import bed_fixed_restatement as bx

LD = np.longdouble
MT = 517                                      # the `ragged` shapes of bed_fixed_restatement / pca_restatement
FLOOR = 1e-12


# ---- splits ---------------------------------------------------------------------------------------------------------------------------
def divide_work(Mt, nranks):
    """[(S, M)] per rank as host/utilities.cpp divides Mt markers: the first Mt % nranks ranks hold one marker more"""
    base, extra = divmod(Mt, nranks)
    out, S = [], 0
    for r in range(nranks):
        M = base + (1 if r < extra else 0)
        out.append((S, M))
        S += M
    return out


def splits(Mt=MT):
    assert Mt > 300
    return {"even2": divide_work(Mt, 2),
            "uneven3": [(0, 1), (1, 64), (65, Mt - 65)],
            "empty3": [(0, 300), (300, 0), (300, Mt - 300)]}


def tiles_exactly(split, Mt):
    """True when the shards cover [0, Mt) in rank order without gap or overlap"""
    at = 0
    for S, M in split:
        if S != at or M < 0:
            return False
        at += M
    return at == Mt


def owner(split, m):
    """the rank whose shard holds marker m"""
    for r, (S, M) in enumerate(split):
        if S <= m < S + M:
            return r
    raise ValueError(m)


# ---- the file layout: column c of rank (S, M) at value offset c * Mt + S --------------------------------------------------------------
def assemble(split, Mt, parts, shift=None):
    """What the ranks of a job leave in an output file of C columns of Mt float64 values: a file of zeros into which rank r writes its
    M values of column c at value offset c * Mt + S (mpi_store_vec_to_file).  parts[r]: C x M of rank r.  shift: {rank: d} moves that
    rank's S by d values, the defect the layout tests must see.  Returns the C * Mt values of the file"""
    C = len(parts[0])
    out = np.zeros(C * Mt)
    for r, (S, M) in enumerate(split):
        P = np.asarray(parts[r], dtype=np.float64).reshape(C, M)
        S = S + (shift or {}).get(r, 0)
        for c in range(C):
            out[c * Mt + S:c * Mt + S + M] = P[c]
    return out


def one_rank_layout(full):
    """the same file written by one rank: column after column"""
    return np.asarray(full, dtype=np.float64).reshape(-1).copy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    """equal as bit patterns: -0.0 differs from 0.0, a NaN equals only a NaN of the same payload"""
    a, b = bits(a), bits(b)
    return a.shape == b.shape and bool(np.array_equal(a, b))


def first_bit_difference(a, b):
    """(flat index, a, b) of the first entry whose bits differ, or None"""
    a, b = np.ascontiguousarray(a, dtype=np.float64).reshape(-1), np.ascontiguousarray(b, dtype=np.float64).reshape(-1)
    if a.shape != b.shape:
        return ("shape", a.shape, b.shape)
    bad = np.nonzero(bits(a) != bits(b))[0]
    return None if len(bad) == 0 else (int(bad[0]), float(a[bad[0]]), float(b[bad[0]]))


def assert_concatenation_is_the_one_shard_result(split, Mt, parts, full, what):
    """the shards' outputs, written where the drivers write them, are the one-context result bit for bit"""
    diff = first_bit_difference(assemble(split, Mt, parts), one_rank_layout(full))
    assert diff is None, (what, diff)


def assert_same_on_every_rank(per_rank, what):
    """every rank holds the bits of rank 0"""
    for r in range(1, len(per_rank)):
        diff = first_bit_difference(per_rank[r], per_rank[0])
        assert diff is None, (what, "rank %d against rank 0" % r, diff)


# ---- Z = A W restated densely ---------------------------------------------------------------------------------------------------------
def dense_A(bed, N, M, present, dtype=LD):
    """N x M: the matrix of gv_ax_dev / gv_score_dev from its definition.  Per marker over the phenotyped individuals with a present
    genotype: mu their mean, msig = 1 / sqrt(sum (a - mu)^2 / (nonas - 1)), 1 for a marker without variance; entry (a - mu) msig / sqrt(N)
    there, 0 at missing genotypes and at individuals without a phenotype"""
    code = bx.decode(bed, N, M)[:, :N]
    present = np.ones(N, dtype=bool) if present is None else np.asarray(present, dtype=bool)
    a = np.select([code == 0, code == 2, code == 3], [2, 1, 0], 0).astype(dtype)
    have = (code != 1) & present[None, :]
    cnt = have.sum(axis=1).astype(dtype)
    mu = np.where(cnt > 0, np.where(have, a, dtype(0)).sum(axis=1) / np.where(cnt > 0, cnt, dtype(1)), dtype(0))
    d = np.where(have, a - mu[:, None], dtype(0))
    ss = (d * d).sum(axis=1)
    nonas = dtype(int(present.sum()))
    sg = np.where(ss != 0, dtype(1) / np.sqrt(np.where(ss != 0, ss, dtype(1)) / (nonas - dtype(1))), dtype(1))
    return (d * sg[:, None]).T / np.sqrt(dtype(N))


def dense_score(A, W):
    """C x N: row j = A W[j], in the precision of A"""
    return np.asarray(W, dtype=np.float64).astype(A.dtype) @ A.T


def score_deviation(got, ref):
    """the largest column deviation (module docstring) and the per-column figures"""
    got, ref = np.asarray(got, dtype=LD), np.asarray(ref, dtype=LD)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    per = []
    for g, f in zip(got, ref):
        top = np.max(np.abs(f))
        err = np.max(np.abs(g - f))
        per.append(float(err / top) if top > 0 else (0.0 if err == 0 else float("inf")))
    return max(per), per


def score_bound(dev64):
    return max(16.0 * dev64, FLOOR)


def score_columns(cs, mave, msig, C=9):
    """C weight columns of case cs: the four kinds of bx.vector_x for kernel mode 1, cycled (kind 4 is the zero vector)"""
    kinds = [bx.vector_x(cs, k, 1, mave, msig) for k in (1, 2, 3, 4)]
    return np.array([kinds[j % 4] for j in range(C)])


def phenotype_columns(cs, C=9):
    """C N-space columns of case cs: the four kinds of bx.vector_p, cycled (zero at NA and pad slots; kind 4 is the zero vector).  Nine of
    them make a second pass of the batch ATx kernel (at most 8 columns a pass)"""
    kinds = [bx.vector_p(cs, k) for k in (1, 2, 3, 4)]
    return np.array([kinds[j % 4] for j in range(C)])


# ---- the clump index of the thresholded score ---------------------------------------------------------------------------------------
def clump_fixture(Mt, rank_counts=(2, 3), seed=29):
    """(index_of, p, w0, thresholds) over Mt markers, in the format of <out>_clump_index.bin (float64: the index marker of a marker's
    clump, itself for an index marker, -1 for a marker in no clump).  For every rank count of `rank_counts` the first marker s of every
    shard but the first is an index marker with members on both sides of the edge (s - 2, s - 1 in the shard below, s + 1 in its own),
    and the marker s - 5 is an index marker with a member at s + 3, in the shard above.  Those members and index markers carry weights
    a thousand times the others' and p-values under the smallest threshold: a member that contributed, or an index marker that did not,
    moves every score far beyond any rounding."""
    rng = np.random.default_rng(seed)
    idx = np.full(Mt, -1.0)
    own = rng.random(Mt) < 0.3
    last = -1
    for j in range(Mt):                                             # a member belongs to the index marker before it, 20 % to no clump
        if own[j]:
            idx[j], last = j, j
        elif last >= 0 and rng.random() < 0.8:
            idx[j] = last
    p = rng.random(Mt) * 0.1
    w0 = rng.standard_normal(Mt)
    thresholds = [0.001, 0.01, 0.05]
    loud = []
    for n in rank_counts:
        for S, _ in divide_work(Mt, n)[1:]:
            idx[[S - 2, S - 1, S, S + 1]] = S
            idx[S - 5], idx[S + 3] = S - 5, S - 5
            loud += [S - 5, S - 2, S - 1, S, S + 1, S + 3]
    for j in range(Mt):                                             # the edits above must not leave a member of a non-index marker
        if idx[j] >= 0 and idx[int(idx[j])] != idx[j]:
            idx[j] = -1.0
    loud = np.array(sorted(set(loud)))
    w0[loud] = 1000.0 * (1.0 + rng.random(len(loud)))
    p[loud] = 1e-4 * rng.random(len(loud))
    idx[7], p[7] = 7.0, 0.01                                        # a tie exactly at a cut-off is in
    return idx, p, w0, thresholds


def cross_shard_members(idx, split):
    """the members (j, index marker) whose index marker lies in another shard"""
    return [(j, int(g)) for j, g in enumerate(idx) if g >= 0 and g != j and owner(split, j) != owner(split, int(g))]


def shard_first_index_markers(idx, split):
    """the index markers that are the first marker of a shard other than the first"""
    return [S for S, M in split[1:] if M > 0 and idx[S] == S]


def used_markers_global(idx, p, thr):
    """the markers column `thr` uses: index markers (index_of[j] == j) with p_j <= thr"""
    idx, p = np.asarray(idx), np.asarray(p)
    with np.errstate(invalid="ignore"):
        return np.nonzero((idx == np.arange(len(idx))) & (p <= thr))[0]


def used_markers_sharded(idx, p, thr, split):
    """the same set as a sharded job finds it: every rank maps its slice of the global index file to shard-local indices (a marker that
    names itself keeps its own local index, any other marker one outside the shard) and applies the rule to its slice"""
    out = []
    for S, M in split:
        g = np.asarray(idx[S:S + M])
        local = np.where(g == S + np.arange(M), np.arange(M), np.where(g < 0, -1, M + 1))
        with np.errstate(invalid="ignore"):
            out += [S + j for j in range(M) if local[j] == j and p[S + j] <= thr]
    return np.array(out, dtype=np.int64)
