"""The k-means reference itself (tests/kmeans_ref.py), on the CPU: the start's
picks, and Lloyd's loop on blobs whose answer is known."""
import numpy as np
import pytest

from tests import kmeans_ref as R


@pytest.mark.parametrize("n,nc,seed", [(1, 1, 0), (10, 10, 1), (1000, 31, 7), (2 ** 32 - 2, 100, 3)])
def test_picks_are_distinct_and_in_range(n, nc, seed):
    p = R.pick(n, nc, seed)
    assert len(p) == nc == len(set(p))
    assert all(0 <= x < n for x in p)
    assert p == R.pick(n, nc, seed)
    if n > 100:
        assert p != R.pick(n, nc, seed + 1)


def test_pick_is_the_shuffle_head():
    """The sparse map gives what the full Fisher-Yates array gives."""
    n, nc, seed = 50, 20, 5
    a = list(range(n))
    for i in range(nc):
        j = i + R.hash4(seed, R.DOM_KMEANS_INIT, i, 0, 0) % (n - i)
        a[i], a[j] = a[j], a[i]
    assert a[:nc] == R.pick(n, nc, seed)


def blobs(nb=5, per=40, dim=6, seed=0):
    rng = np.random.default_rng(seed)
    centre = (np.arange(nb)[:, None] * 1000 + np.zeros((nb, dim))).astype(np.float32)
    gen = np.repeat(np.arange(nb), per)
    rng.shuffle(gen)
    rows = centre[gen] + rng.integers(-5, 6, size=(nb * per, dim)).astype(np.float32)
    return rows, gen, centre


def test_blobs_converge_to_the_generating_labels(oracle):
    rows, gen, centre = blobs()
    cen, labels, sizes, moved = R.kmeans(rows, 5, 20, init=centre + 3)
    assert moved[0] == len(rows)
    t = int(np.flatnonzero(moved == 0)[0])
    assert 1 <= t < 20 and (moved[t:] == 0).all()
    assert int(sizes.sum()) == len(rows) and (sizes == 40).all()
    # equal up to renaming: a bijection between the two labellings
    pairs = set(zip(gen.tolist(), labels.tolist()))
    assert len(pairs) == 5 and len({a for a, _ in pairs}) == 5 and len({b for _, b in pairs}) == 5
    for c in range(5):
        assert np.allclose(cen[c], rows[labels == c].astype(np.float64).mean(0), rtol=1e-6)


def test_blobs_from_picked_rows(oracle):
    """From the hash4 start the loop still ends at a fixed point with every row counted."""
    rows, _, _ = blobs()
    cen, labels, sizes, moved = R.kmeans(rows, 5, 30, seed=2)
    assert (moved == 0).any() and int(sizes.sum()) == len(rows)
    assert np.array_equal(R.assign(rows, cen), labels)
    assert np.array_equal(R.update(rows, cen, labels).view(np.uint32), cen.view(np.uint32))


def test_empty_cluster_keeps_its_centroid(oracle):
    rows, init = R.tied_init_case()
    cen, labels, sizes, moved = R.kmeans(rows, 3, 5, init=init)
    assert sizes[1] == 0 and not (labels == 1).any() and sizes[0] == 40 and sizes[2] == 41
    assert np.array_equal(cen[1], init[1]) and np.array_equal(cen[0], init[0])
    assert moved[1] == 0


def test_addition_order_shows_in_the_wide_range_data():
    """On the GPU tests' wide-range rows the documented order and a plain ascending f64 sum give different
    centroid bits: a kernel that summed in another order would not pass them."""
    rows = R.wide_range_rows(500, 8, 81)
    seq = np.zeros(8)
    for r in rows.astype(np.float64):
        seq = seq + r
    plain = (seq / 500.0).astype(np.float32)
    docs = R.update(rows, np.zeros((1, 8), np.float32), np.zeros(500, np.uint32))[0]
    assert not np.array_equal(docs.view(np.uint32), plain.view(np.uint32))
    assert np.allclose(docs, plain, rtol=1e-4)
