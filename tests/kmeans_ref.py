"""The specification of pm_kmeans and pm_cluster_search in numpy and the oracle
(include/pacmann.h), restated independently of the library:

start       centroid c = row pick[c]; pick = the first nc entries of a
            Fisher-Yates shuffle of 0 .. n-1 whose i-th swap partner is
            i + hash4(seed, 12, i, 0, 0) % (n - i)
assignment  oracle.knn(centroids, rows, 1): the c minimising (L2Dist, c)
update      members in ascending id order; partial sum p of 16 adds members
            p, p + 16, ... in order in f64 from +0.0; total = partial 0 plus
            partials 1 .. 15 in order; total / size in f64, rounded once to f32;
            an empty cluster keeps its centroid
loop        assign; niter times: update, assign; moved[t] = labels changed by
            assignment t (moved[0] = n); stop when nothing moved
search      probed = oracle.knn(centroids, q, nprobe); result = oracle.knn over
            the ascending-id union of the probed clusters' rows, mapped back to
            original ids, -1 / +inf padded
"""
import numpy as np

DOM_KMEANS_INIT = 12
PARTIALS = 16
M64 = (1 << 64) - 1


def sm64(x: int) -> int:
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def hash4(seed: int, dom: int, a: int, b: int, c: int) -> int:
    h = sm64((seed + dom) & M64)
    h = sm64(h ^ a)
    h = sm64(h ^ b)
    return sm64(h ^ c)


def pick(n: int, nc: int, seed: int) -> list[int]:
    perm: dict[int, int] = {}
    out = []
    for i in range(nc):
        j = i + hash4(seed, DOM_KMEANS_INIT, i, 0, 0) % (n - i)
        vi, vj = perm.get(i, i), perm.get(j, j)
        perm[j], perm[i] = vi, vj
        out.append(vj)
    return out


def assign(rows, cen) -> np.ndarray:
    from oracle import oracle as O
    ids, _ = O.knn(cen, rows, 1)
    return ids[:, 0].astype(np.uint32)


def update(rows, cen, labels) -> np.ndarray:
    new = cen.copy()
    dim = rows.shape[1]
    for c in range(cen.shape[0]):
        members = np.flatnonzero(labels == c)   # ascending id
        if len(members) == 0:
            continue
        part = np.zeros((PARTIALS, dim), dtype=np.float64)
        for i, m in enumerate(members):
            part[i % PARTIALS] = part[i % PARTIALS] + rows[m].astype(np.float64)
        total = part[0].copy()
        for p in range(1, PARTIALS):
            total = total + part[p]
        new[c] = (total / np.float64(len(members))).astype(np.float32)
    return new


def kmeans(rows, nc: int, niter: int, seed: int = 1, init=None):
    """(centroids, labels, sizes, moved) as pm.kmeans returns them."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n = rows.shape[0]
    cen = (rows[pick(n, nc, seed)] if init is None else np.asarray(init, dtype=np.float32)).copy()
    moved = np.zeros(niter + 1, dtype=np.uint64)
    labels = assign(rows, cen)
    moved[0] = n
    for t in range(1, niter + 1):
        cen = update(rows, cen, labels)
        new = assign(rows, cen)
        moved[t] = int((new != labels).sum())
        labels = new
        if moved[t] == 0:
            break
    return cen, labels, np.bincount(labels, minlength=nc).astype(np.uint64), moved


def cluster_search(rows, cen, labels, queries, k: int, nprobe: int):
    """(ids, dists, probed, scanned) as ClusterIndex.search returns them."""
    from oracle import oracle as O
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, rows.shape[1])
    labels = np.asarray(labels)
    probed, _ = O.knn(cen, q, nprobe)
    ids = np.full((len(q), k), -1, dtype=np.int64)
    dists = np.full((len(q), k), np.inf, dtype=np.float32)
    scanned = np.zeros(len(q), dtype=np.uint64)
    for i in range(len(q)):
        union = np.flatnonzero(np.isin(labels, probed[i]))   # ascending id
        scanned[i] = len(union)
        if len(union) == 0:
            continue
        li, ld = O.knn(rows[union], q[i], k)
        ok = li[0] >= 0
        ids[i, ok] = union[li[0][ok]]
        dists[i, ok] = ld[0][ok]
    return ids, dists, probed.astype(np.uint32), scanned


def tied_init_case(dim: int = 6, pairs: int = 20):
    """(rows, init): blob 0 is `pairs` rows a + d and as many a - d (integers), so
    its mean is a exactly; blob 1 lies far away.  init = [a, a, b]: centroids 0
    and 1 are identical and stay so (centroid 0's mean is a, centroid 1 never gets
    a member because every tie goes to the lower index)."""
    rng = np.random.default_rng(4)
    a, b = np.full(dim, 100, np.float32), np.full(dim, 5000, np.float32)
    d = rng.integers(-9, 10, size=(pairs, dim)).astype(np.float32)
    rows = np.vstack([a + d, a - d, b + rng.integers(-9, 10, size=(2 * pairs + 1, dim)).astype(np.float32)])
    rows = rows[rng.permutation(len(rows))]
    return np.ascontiguousarray(rows), np.vstack([a, a, b])


def wide_range_rows(n, dim, seed):
    """Coordinates +-m 2^e, m in [1, 2), e uniform in [-20, 20], where every value of 2^-12 and above is
    cancelled by its negative in another row (an unpaired one is scaled down): the f64 sum of a column
    passes through 2^20 and ends near 2^-9, so the roundings on the way, which depend on the order of the
    additions, reach the f32 mean."""
    rng = np.random.default_rng(seed)
    mant = rng.uniform(1.0, 2.0, size=(n, dim))
    sign = rng.choice([-1.0, 1.0], size=(n, dim))
    x = (sign * mant * np.exp2(rng.integers(-20, 21, size=(n, dim)))).astype(np.float32)
    for j in range(dim):
        perm = rng.permutation(n)
        a, b = perm[0:n - 1:2], perm[1:n:2]
        big = np.abs(x[a, j]) >= 2.0 ** -12
        x[b[big], j] = -x[a[big], j]
        rest = np.concatenate([b[~big], perm[2 * len(a):]])
        big = np.abs(x[rest, j]) >= 2.0 ** -12
        x[rest[big], j] *= np.float32(2.0 ** -32)
    return x
