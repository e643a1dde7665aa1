"""The claim pm_graph_u8.hip rests on, without a GPU: for uint8
rows of up to 256 dimensions the biased int8 identity of tests/knn_u8_ref.py
gives integer distances whose float32 conversion is the oracle's L2Dist bit for
bit, every intermediate fits int32, and the (distance, id) ranking is the
oracle's; and the generators of the GPU tests keep what they promise."""
import numpy as np
import pytest

from tests import knn_u8_ref as U

I32 = 2 ** 31 - 1


def check_against_oracle(oracle, v, q):
    dist, peak = U.biased_distances(q, v)
    assert max(peak.values()) <= I32, peak
    assert 0 <= dist.min() and dist.max() <= U.MAX_DIST < 2 ** 24
    n = len(v)
    oi, od = oracle.knn(v.astype(np.float32), q.astype(np.float32), n)
    ri, rd = U.rank(dist, n)
    assert np.array_equal(ri, oi)
    assert np.array_equal(rd.view(np.uint32), od.view(np.uint32))
    return dist, peak


@pytest.mark.parametrize("dim", [1, 63, 64, 65, 255, 256])
def test_identity_equals_l2dist_on_random_bytes(oracle, dim):
    rng = np.random.default_rng([9, dim])
    v = rng.integers(0, 256, (90, dim), dtype=np.uint8)
    q = rng.integers(0, 256, (7, dim), dtype=np.uint8)
    q[0] = v[3]
    check_against_oracle(oracle, v, q)


def test_all_0_against_all_255_is_the_largest_distance(oracle):
    v = np.stack([np.full(256, 255, np.uint8), np.zeros(256, np.uint8)])
    q = np.zeros((1, 256), np.uint8)
    dist, peak = check_against_oracle(oracle, v, q)
    assert dist[0, 0] == 16_646_400 == U.MAX_DIST and dist[0, 1] == 0
    od = oracle.knn(v.astype(np.float32), q.astype(np.float32), 2)[1]
    assert od[0, 1].view(np.uint32) == np.float32(16_646_400).view(np.uint32)
    assert peak["acc"] == 256 * 128 * 128     # (-128) (-128) and (-128) 127 over 256 coordinates


def test_all_255_against_all_255(oracle):
    v = np.full((3, 256), 255, np.uint8)
    dist, peak = check_against_oracle(oracle, v, v[:1])
    assert (dist == 0).all() and peak["acc"] == 256 * 127 * 127 and peak["norms"] == 2 * 256 * 255 * 255


def test_extreme_rows_reach_both_signs(oracle):
    v, q = U.extreme_rows()
    dist, peak = check_against_oracle(oracle, v, q)
    assert dist.max() == U.MAX_DIST and peak["acc"] == 256 * 128 * 128 and peak["cx"] == 256 * 128 * 128
    qb, vb = q.astype(np.int64) - 128, v.astype(np.int64) - 128
    assert (qb @ vb.T).min() == -256 * 128 * 127 and (qb @ vb.T).max() == 256 * 128 * 128


def test_shape_cases_cover_every_axis():
    cases = U.shape_cases()
    assert 38 <= len(cases) <= 46
    for axis, values in ((0, U.SHAPE_N), (2, U.SHAPE_DIM)):
        for x in values:
            assert len({c[1] for c in cases if c[axis] == x}) >= 2, (axis, x)   # with at least two nq
    for nq in U.SHAPE_NQ:
        assert sum(c[1] == nq for c in cases) >= 2
    assert {U.pad_dim(c[2]) for c in cases} == {64, 128, 192, 256}
    for k in (1, 64, 128):
        assert sum(c[3] == k for c in cases) >= 2, k
    assert sum(c[3] == c[0] + 1 for c in cases) >= 2       # k = n + 1
    assert sum(c[3] > c[0] for c in cases) >= 4            # -1 / +inf padding
    assert all(1 <= c[3] <= U.TOP and 1 <= c[2] <= U.MAX_DIM for c in cases)


def test_generators_keep_their_promises():
    v, q = U.descending_rows()
    d = U.biased_distances(q, v)[0][0]
    assert v.dtype == np.uint8 and len(d) == 1024 and (np.diff(d) < 0).all()
    v, q, ntie = U.identical_rows()
    d = U.biased_distances(q, v)[0]
    assert ((d[:ntie] == 0).sum(1) == 300).all() and ((d[ntie:] == 0).sum(1) == 1).all()
    v, q, ids = U.one_distance_rows()
    d = U.biased_distances(q, v)[0]
    assert (d[0, ids] == 1).all() and len(ids) == 200 and (np.delete(d[0], ids) > 1).all()
    assert ids[:100].max() < 128 and ids[100:].min() >= (len(v) - 1) // 64 * 64 - 64
