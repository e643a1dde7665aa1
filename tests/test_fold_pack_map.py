"""The packed fold image's index map (k_fold_image through pm.fold_image_map:
host arithmetic, no GPU) against a NumPy restatement of the layout.

A graph DB whose coordinate words (f32) all have zero low halves gets a fold
image without them: coordinate slice s' of the image holds, as 16 consecutive
half-words, the high halves of coordinate words 16 s' .. 16 s' + 15, and the
neighbour-id slices follow whole.  The block layout is the plain image's: one
64 KB block per (slice, 4 chunks), line k = row k of each of the four chunks,
32 B per chunk, rows past the partition's end zero."""
import numpy as np
import pytest

CS = 512


def rows_u32(N, dim, m, seed):
    """[N, dim + m] uint32 entries: integer-valued f32 coordinates, then neighbour ids."""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 256, size=(N, dim)).astype(np.float32).view(np.uint32)
    return np.concatenate([v, rng.integers(0, 2**32, size=(N, m), dtype=np.uint32)], axis=1)


def numpy_image(rows, SS, nsl):
    """The plain image layout over rows of nsl 32-B slices: [nsl, SS / 4, CS, 4, 8] uint32."""
    N = rows.shape[0]
    pad = np.zeros((SS * CS, nsl * 8), dtype=np.uint32)
    pad[:N] = rows[:, :nsl * 8]
    x = pad.reshape(SS // 4, 4, CS, nsl, 8)          # block b, chunk slot c, line k, slice s, word
    return np.ascontiguousarray(x.transpose(3, 0, 2, 1, 4))


def image_by_map(rows, SS, E, dim, packed):
    import pacmann_amd as pm
    N = rows.shape[0]
    row, word, pk, nitems, npk = pm.fold_image_map(CS, SS, E, dim, packed)
    assert len(row) == nitems
    out = np.zeros((nitems, 4), dtype=np.uint32)
    r = row.astype(np.int64)
    live = r < N
    assert r.max() < SS * CS
    for i in range(4):   # four whole words
        sel = live & ~pk
        out[sel, i] = rows[r[sel], word[sel] + i]
    for i in range(4):   # the high halves of eight words, two per image word
        sel = live & pk
        lo, hi = rows[r[sel], word[sel] + 2 * i], rows[r[sel], word[sel] + 2 * i + 1]
        out[sel, i] = (lo >> 16) | (hi & 0xffff0000)
    return out.reshape(-1), npk


@pytest.mark.parametrize("dim,m", [(128, 32), (48, 16), (48, 8), (16, 8)])
def test_packed_image_map(dim, m):
    """dim 128 (SIFT's entries), a dim that is a multiple of 16 but not of 32, the same with
    E % 4 == 2 (tail words outside the image) and the smallest (one packed slice)."""
    N, SS = 3 * CS + 77, 4 + 4      # the last chunks partial and past N
    E = (dim + m) // 2
    rows = rows_u32(N, dim, m, seed=dim + m)
    assert not (rows[:, :dim] & 0xffff).any()
    got, npk = image_by_map(rows, SS, E, dim, True)
    assert npk == dim // 16
    nsl = E // 4 - npk
    halves = (rows[:, :dim] >> 16).astype(np.uint16)                 # 16 per packed slice
    packed_rows = np.concatenate([halves.view(np.uint32), rows[:, dim:]], axis=1)
    want = numpy_image(packed_rows, SS, nsl)
    assert got.size == want.size == nsl * (SS // 4) * CS * 4 * 8
    assert np.array_equal(got, want.reshape(-1))
    # and the plain image of the same entries, through the same map
    plain, npk0 = image_by_map(rows, SS, E, dim, False)
    assert npk0 == 0
    assert np.array_equal(plain, numpy_image(rows, SS, E // 4).reshape(-1))


@pytest.mark.parametrize("cs,E,dim", [
    (512, 16, 24),     # dim % 16 != 0: the coordinates do not fill whole packed slices
    (512, 16, 8),
    (512, 16, 0),      # no coordinate part (a bare PIR engine)
    (512, 10, 32),     # coordinates beyond the folded E & ~3 words
    (1024, 80, 128),   # the CS-1,024 fold has no packed form
])
def test_packed_image_refused(cs, E, dim):
    import pacmann_amd as pm
    with pytest.raises(RuntimeError, match="no packed fold image"):
        pm.fold_image_map(cs, 8, E, dim, True)
    assert pm.fold_image_map(cs, 8, E, dim, False)[4] == 0   # the plain image exists


def test_image_sizes():
    """SIFT1M's partition (62,500 rows x 640 B, SetSize 124): 20 -> 12 slices."""
    import pacmann_amd as pm
    plain = pm.fold_image_map(512, 124, 80, 128, False, n=0)[3]
    packed = pm.fold_image_map(512, 124, 80, 128, True, n=0)[3]
    assert plain == 20 * 31 * 4096 and packed == 12 * 31 * 4096


def test_fold_pack_option_values():
    import pacmann_amd as pm
    for v in (2, -2, 7):
        with pytest.raises(RuntimeError, match="fold_pack"):
            pm.set_option("fold_pack", v)
    for v in (0, 1, -1):
        pm.set_option("fold_pack", v)
