"""loader.load_bvecs_u8 returns load_bvecs' rows as uint8: the same records, the
same truncation and zero fill, the same "Unexpected EOF"."""
import struct

import numpy as np
import pytest

from pacmann_amd import loader


def write_bvecs(path, rows):
    with open(path, "wb") as f:
        for r in rows:
            f.write(struct.pack("<i", len(r)))
            f.write(np.asarray(r, np.uint8).tobytes())


def both(path, n, dim, capsys):
    want = loader.load_bvecs(path, n, dim)
    err_f32 = capsys.readouterr().err
    got = loader.load_bvecs_u8(path, n, dim)
    err_u8 = capsys.readouterr().err
    assert got.dtype == np.uint8 and got.shape == (n, dim) and got.flags.c_contiguous
    assert np.array_equal(got, want.astype(np.uint8)) and np.array_equal(got.astype(np.float32), want)
    assert err_u8 == err_f32
    return got, err_u8


@pytest.fixture
def rows():
    return np.random.default_rng(5).integers(0, 256, (20, 24), dtype=np.uint8)


@pytest.mark.parametrize("dim", [24, 10, 40])
def test_uniform_file(tmp_path, capsys, rows, dim):
    """dim equal to, smaller and larger than the stored dimension."""
    p = tmp_path / "a.bvecs"
    write_bvecs(p, rows)
    got, err = both(p, 20, dim, capsys)
    w = min(dim, 24)
    assert np.array_equal(got[:, :w], rows[:, :w]) and not got[:, w:].any() and err == ""
    got, err = both(p, 7, dim, capsys)
    assert np.array_equal(got[:, :w], rows[:7, :w]) and err == ""


@pytest.mark.parametrize("dim", [24, 10, 40])
def test_fewer_records_than_asked(tmp_path, capsys, rows, dim):
    p = tmp_path / "a.bvecs"
    write_bvecs(p, rows)
    got, err = both(p, 25, dim, capsys)
    assert not got[20:].any() and "Unexpected EOF" in err


@pytest.mark.parametrize("dim", [24, 10, 40])
def test_short_last_record(tmp_path, capsys, rows, dim):
    p = tmp_path / "a.bvecs"
    write_bvecs(p, rows)
    data = p.read_bytes()
    p.write_bytes(data[:-5])
    got, err = both(p, 20, dim, capsys)
    assert not got[19].any() and got[18].any() and "Unexpected EOF" in err


def test_mixed_dimensions_and_empty_file(tmp_path, capsys, rows):
    p = tmp_path / "a.bvecs"
    write_bvecs(p, [rows[0], rows[1][:9], rows[2]])
    got, _ = both(p, 3, 24, capsys)
    assert np.array_equal(got[1, :9], rows[1][:9]) and not got[1, 9:].any()
    p.write_bytes(b"")
    got, err = both(p, 2, 8, capsys)
    assert not got.any() and "Unexpected EOF" in err
