"""Why a region decode may stop at the covering slab (CPU only, the oracle alone): Lorenzo
prediction restarts at every tile, so the codes of a tile-aligned slab of the slowest axis plus the
outlier cells that fall inside it reconstruct, as a field of the slab's own extents, to the bits of
the same slab of the whole field's reconstruction.  The slab units are 1024 elements (1-D), 32 rows
(2-D) and 8 planes (3-D); 16 rows in 2-D is no such unit, which the last test shows.

This pins the table in DESIGN.md §4 "Region decode"; it does not run the region code."""
import numpy as np
import pytest

from cusz_amd import datagen

SHAPES = {  # name: (dims, slab unit on the slow axis)
    "1d-200003": ((200_003, 1, 1), 1024),
    "2d-300x70": ((300, 70, 1), 32),
    "2d-301x70": ((301, 70, 1), 32),
    "3d-96x20x13": ((96, 20, 13), 8),
    "3d-256x20x13": ((256, 20, 13), 8),
}
VARIANTS = [(np.float32, False, 512), (np.float64, False, 64), (np.float32, True, 64), (np.float64, True, 512)]
_cache = {}


def _ndim(dims):
    return 3 if dims[2] != 1 else 2 if dims[1] != 1 else 1


def _full(oracle, dims, dtype, zz, radius):
    """codes, cells and the whole reconstruction, once per (shape, variant)"""
    key = (dims, dtype, zz, radius)
    if key not in _cache:
        n = int(np.prod(dims))
        data = datagen.smooth3d_np(dims, sum(dims), dtype=dtype).reshape(-1)
        rng = np.random.default_rng(n)
        data[rng.integers(0, n, max(8, n // 500))] += dtype(3.0)  # outliers at either radius
        eb = 3e-4
        codes, ov, oi = oracle.lorenzo_c(data, dims, eb, radius, zz)
        assert len(oi) > 0
        _cache[key] = (codes, ov, oi, oracle.lorenzo_x(codes, ov, oi, dims, eb, radius, zz, dtype), eb)
    return _cache[key]


def _slab(oracle, dims, dtype, zz, radius, a, b):
    """(slab reconstructed on its own, the same slab of the whole reconstruction), as bits"""
    codes, ov, oi, full, eb = _full(oracle, dims, dtype, zz, radius)
    nd = _ndim(dims)
    P = int(np.prod(dims[:nd - 1]))
    lo, hi = a * P, b * P
    keep = (oi >= lo) & (oi < hi)
    sdims = list(dims)
    sdims[nd - 1] = b - a
    got = oracle.lorenzo_x(codes[lo:hi], ov[keep], (oi[keep] - lo).astype(np.uint32), tuple(sdims), eb, radius, zz, dtype)
    bits = np.uint32 if dtype == np.float32 else np.uint64
    return got.view(bits), full[lo:hi].view(bits)


def _slabs(length, T):
    """every slab of 1 or 2 units, and every slab that reaches the field's end"""
    units = (length + T - 1) // T
    out = {(u * T, min(length, (u + k) * T)) for u in range(units) for k in (1, 2)}
    out |= {(u * T, length) for u in range(units)}
    return sorted(out)


@pytest.mark.parametrize("dtype,zz,radius", VARIANTS, ids=["f32-r512", "f64-r64", "f32-zz-r64", "f64-zz-r512"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_tile_aligned_slabs_reconstruct_to_the_bits_of_the_field(oracle, shape, dtype, zz, radius):
    dims, T = SHAPES[shape]
    nd = _ndim(dims)
    slabs = _slabs(dims[nd - 1], T)
    if nd == 1:  # 196 tiles: the first, the last and a spread in between
        slabs = slabs[:4] + slabs[len(slabs) // 2:len(slabs) // 2 + 4] + slabs[-6:]
    assert len(slabs) >= 3
    for a, b in slabs:
        if nd > 1 and b - a == 1:
            continue  # (the oracle reads the dimension count off the extents)
        got, want = _slab(oracle, dims, dtype, zz, radius, a, b)
        np.testing.assert_array_equal(got, want, err_msg=f"slab [{a}, {b})")


def test_sixteen_rows_are_no_slab_unit_in_2d(oracle):
    dims = (301, 70, 1)
    differ = 0
    slabs = [s for s in _slabs(70, 16) if s[0] % 32]  # (those at a multiple of 32 start on a tile)
    assert slabs
    for a, b in slabs:
        got, want = _slab(oracle, dims, np.float32, False, 512, a, b)
        differ += int(np.any(got != want))
    assert differ > 0
