"""Operands of the retrieval tests that are exact in fp32 (tests/test_retrieval_ref.py asserts that they are, the way
tests/test_exact.py does for the conv cases; tests/test_gpu_retrieval.py then demands the specification's bits), and the
host arithmetic that tells where the kernel cuts the gallery into slabs."""
import numpy as np

TILE = 128          # queries per workgroup and gallery rows per score tile (csrc/retrieval.hip: TQ, TG)
SMAX = 64
SLABS = (1, 3, 0)   # every GPU case runs with these `slabs` arguments: one slab, an odd count, the kernel's own choice


def slab_count(nq, ng, slabs):
    """Slabs gca_retrieval_topk uses and gallery rows per slab (make_plan in csrc/retrieval.hip)."""
    qtiles, gtiles = -(-nq // TILE), -(-ng // TILE)
    S = slabs if slabs > 0 else -(-256 // max(qtiles, 1))
    S = max(1, min(S, SMAX, gtiles))
    per = -(-gtiles // S) if gtiles else 1
    return (-(-gtiles // per) if gtiles else 1), per * TILE


def slab_of(j, nq, ng, slabs):
    return np.asarray(j) // slab_count(nq, ng, slabs)[1]


def pm1_rows(rs, n, D, nnz):
    """n rows of D entries: `nnz` of them +-1 (nnz a power of 4: |row|^2 = nnz and 1 / sqrt(nnz) are exact), the rest 0."""
    out = np.zeros((n, D), dtype=np.float32)
    for i in range(n):
        m = nnz[i % len(nnz)] if isinstance(nnz, (tuple, list)) else nnz
        pos = rs.permutation(D)[:m]
        out[i, pos] = rs.choice([-1.0, 1.0], size=m)
    return out


def cosine_case():
    """Entries in {-1, +1}, D = 64: norm 8, r = 0.125, dist = 1 - s / 64.  Gallery rows equal to queries and duplicated
    across the slab boundaries of every slab count in SLABS (rows 128, 256, 512 start slabs)."""
    rs = np.random.RandomState(11)
    q = rs.choice([-1.0, 1.0], size=(33, 64)).astype(np.float32)
    g = rs.choice([-1.0, 1.0], size=(700, 64)).astype(np.float32)
    for i, rows in enumerate(((100, 130, 300, 600), (5, 255, 256, 699), (127, 128, 511, 512))):
        g[list(rows)] = q[i]
    g[[400, 650]] = g[20]
    return q, g


def euclidean_case():
    """Integer entries in [-8, 8], D = 48: every d2 is an integer <= 4 * 48 * 64."""
    rs = np.random.RandomState(12)
    q = rs.randint(-8, 9, size=(70, 48)).astype(np.float32)
    g = rs.randint(-8, 9, size=(1000, 48)).astype(np.float32)
    g[[3, 129, 500, 999]] = q[0]
    g[[640, 641]] = g[7]
    return q, g


def ramp_case(descending):
    """D = 8, gallery row j = (4200 - j) e0 (descending: every later row is nearer than everything before it, so every
    candidate passes every threshold) or the same rows in ascending order (nothing after the first k passes);
    queries c e0, c = 0..4.  Euclidean."""
    v = 4200.0 - np.arange(4096)
    g = np.zeros((4096, 8), dtype=np.float32)
    g[:, 0] = v if descending else v[::-1]
    q = np.zeros((5, 8), dtype=np.float32)
    q[:, 0] = np.arange(5)
    return q, g


def all_equal_case():
    g = np.tile(np.array([[1, -1, 1, 1] * 4], dtype=np.float32), (300, 1))
    q = pm1_rows(np.random.RandomState(13), 5, 16, 16)
    return q, g


def shape_case(nq, ng, D, metric, seed=0):
    """Small exact operands of any shape: integers in [-3, 3] (euclidean), or rows with a power-of-4 count of +-1 (cosine)."""
    rs = np.random.RandomState(1000 * seed + 7 * nq + 13 * ng + D)
    if metric == 'euclidean':
        return (rs.randint(-3, 4, size=(nq, D)).astype(np.float32), rs.randint(-3, 4, size=(ng, D)).astype(np.float32))
    nnz = [m for m in (1, 4, 16, 64, 256, 1024) if m <= D][-2:]
    return pm1_rows(rs, nq, D, nnz), pm1_rows(rs, ng, D, nnz)


def float_case(D):
    rs = np.random.RandomState(2000 + D)
    return rs.standard_normal((70, D)).astype(np.float32), rs.standard_normal((1000, D)).astype(np.float32)
