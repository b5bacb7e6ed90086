"""Numpy (fp64) specification of gca_nnclr_search / gca_nnclr_bwd (csrc/nnclr.hip) and of one NNCLRLoss forward: NNCLR, Dwibedi et
al. 2021, Algorithm 1.

    search   z1, z2 (N, D): the projections of the two views;  Q (K, D): the support set.  Per view v:
             s[v][i,j] = sum_e z_v[i,e] * Q[j,e]          key(s) = s, or -inf where s is NaN
             idx[v][i] = the SMALLEST j with key(s[v][i,j]) = max_j key        sim[v][i] = that key        nn_v[i,:] = Q[idx[v][i],:]
    loss     direction 0 has rows nn1 and columns p2, direction 1 rows nn2 and columns p1: mocov3_ref.direction(q = nn, k = p);
             loss = w (l_0 + l_1), w = 1/2;  lse, rank as there.
    dp       P[i,j] = exp(s[i,j] - lse[i]):   dp[j,:] = g w inv_T / N ( sum_i P[i,j] nn[i,:] - nn[j,:] )
             dp2 comes from direction 0, dp1 from direction 1; nothing flows to nn (nor to z).
    module   search the PRE-enqueue support set, the loss, then Q[(index + i) % K] = z1[i] and index = (index + N) % K.

Dispatch of the kernels:
    search   fast: D <= 256, D % 4 == 0, z1 / z2 / Q 16-byte aligned, 4 waves, groups of 4 row tiles of the two views together
             (G = ceil(2 ceil(N / 32) / 4)); generic: 1 wave, G = 2 ceil(N / 32).  kt = ceil(K / 32) tiles of the support set:
             want = clamp(ceil(256 / G), 1, kt), tps = ceil(kt / want), splits = ceil(kt / tps); split s covers the columns
             [32 tps s, 32 tps (s + 1)).
    backward mocov3_ref.mocov3_path.

Inputs of the tests live here too, so the CPU tests can assert the properties the GPU tests rely on."""
import numpy as np

import mocov3_ref as mr

W = 0.5
SEARCH_EXACT_CASES = [(1, 8, 1), (5, 32, 31), (33, 128, 100), (64, 256, 3075), (33, 130, 200), (4, 1, 40)]       # (N, D, K)
SEARCH_EXACT_PATHS = ['fast', 'fast', 'fast', 'fast', 'generic', 'generic']
NAN_CASE = (33, 128, 100)
SEARCH_FLOAT_CASES = [(5, 32, 31), (33, 128, 100), (64, 256, 3075), (100, 256, 1000), (40, 130, 200)]
GAP = 1e-5                                 # every float-input row's top-2 gap exceeds GAP * max|s|
BWD_EXACT_CASES, BWD_EXACT_PATHS, EXACT_INV_T = mr.EXACT_CASES, mr.EXACT_PATHS, mr.EXACT_INV_T
BWD_FLOAT_TS = (0.1, 0.2)
BWD_FLOAT_CASES = [(N, D) for N in (5, 33, 100, 257) for D in (32, 128, 256)]
HARD_CASES, HARD_T = mr.HARD_CASES, mr.HARD_T


# ----------------------------------------------------------------------------- the specification
def key(s):
    return np.where(np.isnan(s), -np.inf, s)


def search_view(z, Q, last=False):
    """-> dict(s, idx, sim, nn) of one view.  last: the WRONG tie rule (largest index), for the tests that must tell them apart."""
    with np.errstate(invalid='ignore'):
        s = np.asarray(z, dtype=np.float64) @ np.asarray(Q, dtype=np.float64).T
    k = key(s)
    idx = (k.shape[1] - 1 - np.argmax(k[:, ::-1], axis=1)) if last else np.argmax(k, axis=1)        # argmax: the first maximum
    return dict(s=s, idx=idx.astype(np.int64), sim=k[np.arange(k.shape[0]), idx], nn=np.asarray(Q)[idx])


def search(z1, z2, Q, last=False):
    v = [search_view(z1, Q, last), search_view(z2, Q, last)]
    return {name: [v[0][name], v[1][name]] for name in v[0]}


def top2_gap(s):
    """Per row: the largest key minus the second largest (inf for K = 1)."""
    k = np.sort(key(s), axis=1)
    if k.shape[1] == 1:
        return np.full(k.shape[0], np.inf)
    with np.errstate(invalid='ignore'):
        return np.where(np.isinf(k[:, -1]) & (k[:, -1] == k[:, -2]), 0.0, k[:, -1] - k[:, -2])


def nnclr(nn1, nn2, p1, p2, inv_T, w=W, g=1.0):
    """-> dict(s, lse, sp, l, rank, P: [direction 0, direction 1]; loss; dp1, dp2), everything in fp64 from the given values."""
    coef = float(g) * float(w) * float(inv_T)
    d = [mr.direction(nn1, p2, inv_T, coef), mr.direction(nn2, p1, inv_T, coef)]
    out = {name: [d[0][name], d[1][name]] for name in d[0] if name != 'dq'}
    out['loss'] = float(w) * (d[0]['l'] + d[1]['l'])
    N = np.asarray(nn1).shape[0]
    n1, n2 = np.asarray(nn1, dtype=np.float64), np.asarray(nn2, dtype=np.float64)
    out['dp2'] = coef / N * (d[0]['P'].T @ n1 - n1)
    out['dp1'] = coef / N * (d[1]['P'].T @ n2 - n2)
    out['dnn_rows'] = [d[0]['dq'], d[1]['dq']]            # mocov3's gradient (to the rows): NOT what NNCLR wants
    return out


def enqueue(Q, index, rows):
    Q = np.array(Q, copy=True)
    K = Q.shape[0]
    if rows.shape[0] > K:
        raise ValueError('cannot enqueue %d rows into a support set of %d' % (rows.shape[0], K))
    for i in range(rows.shape[0]):
        Q[(index + i) % K] = rows[i]
    return Q, (index + rows.shape[0]) % K


def module_step(z1, z2, p1, p2, Q, index, inv_T, g=1.0):
    """One NNCLRLoss forward -> (search dict, nnclr dict, new Q, new index)."""
    sr = search(z1, z2, Q)
    out = nnclr(sr['nn'][0], sr['nn'][1], p1, p2, inv_T, g=g)
    Q2, index2 = enqueue(Q, index, np.asarray(z1))
    return sr, out, Q2, index2


def search_path(N, D, K, aligned=True):
    """-> (name, waves per workgroup, splits, tiles per split)."""
    fast = D <= mr.FAST_MAX_D and D % 4 == 0 and aligned
    T = -(-N // 32)
    G = -(-2 * T // 4) if fast else 2 * T
    kt = -(-K // 32)
    want = min(max(-(-256 // G), 1), kt)
    tps = -(-kt // want)
    return ('fast' if fast else 'generic', 4 if fast else 1, -(-kt // tps), tps)


def split_boundaries(N, D, K, aligned=True):
    """First columns of the splits 1 .. splits - 1."""
    _, _, splits, tps = search_path(N, D, K, aligned)
    return [32 * tps * s for s in range(1, splits)]


def torch_chain(z1, z2, p1, p2, Q, T):
    """The literal loss of Algorithm 1 as a chain of torch ops (the comparator of tools/nnclr_micro.py and test_nnclr_ref.py)."""
    import torch
    import torch.nn.functional as F
    nn1 = Q.index_select(0, (z1.detach() @ Q.t()).argmax(dim=1))
    nn2 = Q.index_select(0, (z2.detach() @ Q.t()).argmax(dim=1))
    target = torch.arange(p1.shape[0], device=p1.device)
    return 0.5 * (F.cross_entropy(nn1 @ p2.t() / T, target) + F.cross_entropy(nn2 @ p1.t() / T, target))


# ----------------------------------------------------------------------------- inputs
def _sign(row):
    return np.where(row < 0, -1.0, 1.0).astype(np.float32)


def exact_search_inputs(N, D, K, seed=0, nan=False):
    """(z1, z2, Q, plants) fp32 with entries m / 8 in [-1, 1]: every s is a multiple of 1/64 of magnitude at most D <= 2^9, the same
    number in fp32 and fp64 under any order of summation.  For D >= 32 equal maxima are planted (a support row that is the sign
    pattern of a z row scores sum |z|, which nothing else in [-1, 1]^D reaches): `plants` lists (view, row, columns that tie,
    expected idx).  In order, as far as rows and columns last:
        view 0 row 0     columns 0 and K - 1 tie (they differ in one feature, where the z row is 0)
        view 1 row N - 1 that z row with a 1 at that feature: its maximum is the LAST column alone
        view 0 row 1     columns 31 and 32 tie, across a tile edge
        further rows     columns b - 1 and b tie for every split boundary b that search_path reports
    Small D (1, 8) rely on the ties that m / 8 values produce by themselves.  nan: row 5 of Q is NaN and row 3 of z2 is NaN."""
    rng = np.random.RandomState(7919 * N + 31 * D + K + seed)
    z1, z2 = (rng.randint(-8, 9, size=(N, D)).astype(np.float32) / np.float32(8) for _ in range(2))
    Q = rng.randint(-8, 9, size=(K, D)).astype(np.float32) / np.float32(8)
    zs, plants, used = [z1, z2], [], set()

    def plant(view, row, cols):
        g = _sign(zs[view][row])
        for c in cols:
            Q[c] = g
        used.update(cols)
        plants.append((view, row, tuple(cols), min(cols)))

    if D >= 32:
        free = [(v, i) for v in range(2) for i in range(N)]
        if K >= 4 and N >= 2:
            e0 = D // 2
            z1[0, e0] = 0.0
            plant(0, 0, (0, K - 1))
            Q[0, e0], Q[K - 1, e0] = -1.0, 1.0
            z2[N - 1] = z1[0]
            z2[N - 1, e0] = 1.0
            plants.append((1, N - 1, (K - 1,), K - 1))
            free.remove((0, 0)), free.remove((1, N - 1))
        if K >= 40 and N >= 2:
            plant(0, 1, (31, 32))
            free.remove((0, 1))
        for b in split_boundaries(N, D, K):
            if not free:
                break
            if b in used or b - 1 in used or b >= K:
                continue
            v, i = free.pop(0)
            plant(v, i, (b - 1, b))
    if nan:
        Q[5] = np.nan
        z2[3] = np.nan
        plants = [p for p in plants if not (p[0] == 1 and p[1] == 3) and 5 not in p[2]]
    return z1, z2, Q, plants


def float_search_inputs(N, D, K, seed=0):
    """(z1, z2, Q, designated (2, N)) fp32 unit rows: Q random, each z row a perturbed copy (cos about 0.9) of a designated support
    row -- two z rows may share one."""
    rng = np.random.RandomState(131 * N + 17 * D + K + seed)
    Q = rng.randn(K, D)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    des = rng.randint(0, K, size=(2, N))
    zs = []
    for v in range(2):
        x = Q[des[v]] + rng.randn(N, D) * np.sqrt(0.23 / D)
        zs.append(x / np.linalg.norm(x, axis=1, keepdims=True))
    return zs[0].astype(np.float32), zs[1].astype(np.float32), Q.astype(np.float32), des


def bwd_exact_inputs(N, D):
    """(nn1, nn2, p1, p2): mocov3_ref.exact_inputs with nn in the role of q and p in the role of k (its docstring says why the
    random rows are sparse: the backward pass reads an fp32 row_lse)."""
    return mr.exact_inputs(N, D)


BWD_COS = 0.45


def bwd_float_inputs(N, D, seed=0, hard=False):
    """(nn1, nn2, p1, p2) fp32.  hard: mocov3_ref.float_inputs(hard=True) in the roles above -- row norms spread 4x, rows sharing
    a direction, and row 0 of each p equal to its neighbour row.  Otherwise unit rows, each a perturbed copy of its clip's
    direction with cos(nn[i], p[i]) about BWD_COS = 0.45: a neighbour is ANOTHER clip's projection, aligned with the prediction
    far less than the two views of one clip are.  The figure is chosen for the temperatures of the tests, not for the kernel: at
    cos 0.9 and T = 0.1 the positive logit is 9, the softmax of a batch of 5 is saturated (1 - P[j,j] about 5e-4) and the
    rounding of s to fp32 alone (ulp 1e-6) is 2e-3 of dp -- the fp32 torch chain on the CPU misses the 1e-5 bar there by 15x
    (1.5e-4, measured), so no fp32 kernel can be held to it.  At 0.45 the logits at T = 0.1 are those of MoCo v3's tests at
    T = 0.2 (4.5), where fp32 arithmetic leaves the room test_nnclr_ref.py asserts."""
    if hard:
        return mr.float_inputs(N, D, seed=seed, hard=True)
    rng = np.random.RandomState(211 * N + D + seed)
    base = rng.randn(N, D)
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    out = []
    for _ in range(4):
        x = base + rng.randn(N, D) * np.sqrt((1.0 / BWD_COS - 1.0) / D)
        out.append((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32))
    return tuple(out)


def step_inputs(N, D, K, seed=0):
    """(z1, z2, p1, p2, Q) unit rows for the module tests: the search inputs above plus predictions near the projections."""
    z1, z2, Q, _ = float_search_inputs(N, D, K, seed)
    rng = np.random.RandomState(991 * N + D + K + seed)
    ps = []
    for z in (z1, z2):
        x = z.astype(np.float64) + rng.randn(N, D) * np.sqrt(0.3 / D)
        ps.append((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32))
    return z1, z2, ps[0], ps[1], Q
