"""Fields whose Lorenzo quantization codes are known in closed form (a plain helper module, no
tests): the prediction errors are chosen first and the field is their integral.

delta_field() draws one integer delta per element, uniform on [-(radius - 1), radius - 1], plants
outlier deltas (+-radius, +-(radius + 1), 3 radius) on 2 % of the positions of a field of 50
elements or more, and integrates with np.cumsum along x, then y, then z, restarting at every border
of the Lorenzo tile (edge_fields.tile_of: 8 x 8 x 8, 32 x 32 or 1024).  The Lorenzo differences
inside a tile, with 0 before its first element, undo exactly that, so at eb = 0.5 (prequantization
is a multiplication by 1) the prediction error of every element is its delta:

    plain:   code = delta + radius where |delta| < radius, else 0 and the cell holds delta + radius;
    ZigZag:  code = zz(delta)      where |delta| < radius, else 0 and the cell holds delta;
    the reconstruction is the input, bit for bit.

None of this calls the oracle: test_delta_fields.py holds the oracle to it on the CPU, the GPU
tests hold the kernels to both.

Exactness: the field's values are sums of up to a tile's deltas, and the kernels and the oracle
form up to three successive differences (and partial sums) of them, at most 8 max|field| in
magnitude.  Integers below 2^24 are exact in f32, so delta_field() asserts max|field| < 2^21; the
largest of the shapes in use is 36,415.
"""
import numpy as np

from edge_fields import tile_of

OUTLIER_SHARE = 50   # one position in 50 carries an outlier delta
OUTLIER_FROM = 50    # ... in fields of this many elements or more


def vector_width(dtype, lx):
    """Elements a lane holds in the reference-layout 2-D and 3-D Lorenzo kernels (lorenzo.hip
    lorenzo_geom): f32 4 if lx % 4 == 0, else 2 if lx is even, else 1; f64 2 if lx is even, else 1."""
    if np.dtype(dtype) == np.float32 and lx % 4 == 0:
        return 4
    return 2 if lx % 2 == 0 else 1


def outlier_deltas(radius):
    r = radius
    return (r, -r, r + 1, -(r + 1), 3 * r)


def zigzag(d):
    """composite.hh: (v << 1) ^ (v >> 15) on int16 -> 0, -1, 1, -2, ... map to 0, 1, 2, 3, ..."""
    d = np.asarray(d, np.int64)
    return np.where(d >= 0, 2 * d, -2 * d - 1)


def draw_deltas(dims, radius, seed=None, planted=None):
    """-> int64[n] deltas (x fastest).  planted: {flat index: delta} instead of the 2 % outliers."""
    x, y, z = dims
    n = x * y * z
    rng = np.random.default_rng(1_000_003 * x + 10_007 * y + 101 * z + 7 * radius if seed is None else seed)
    d = rng.integers(-(radius - 1), radius, n)
    if planted is not None:
        for i, v in planted.items():
            d[i] = v
    elif n >= OUTLIER_FROM:
        pos = rng.choice(n, n // OUTLIER_SHARE, replace=False)
        d[pos] = rng.choice(outlier_deltas(radius), pos.size)
    return d


def integrate(deltas, dims):
    """Running sums along x, then y, then z, each restarted at every tile border -> int64[n]."""
    x, y, z = dims
    f = np.asarray(deltas, np.int64).reshape(z, y, x).copy()
    for axis, tile in ((2, tile_of(dims)[0]), (1, tile_of(dims)[1]), (0, tile_of(dims)[2])):
        for lo in range(0, f.shape[axis], tile):
            sl = tuple(slice(lo, lo + tile) if a == axis else slice(None) for a in range(3))
            f[sl] = np.cumsum(f[sl], axis=axis)
    return f.reshape(-1)


def delta_field(dims, radius, dtype, zz, seed=None, planted=None):
    """-> (data, expected_codes u16[n], expected_ol_idx u32[k] ascending, expected_ol_val f32[k]) for
    a compress at eb = 0.5 with this radius and predictor (zz: LorenzoZigZag)."""
    d = draw_deltas(dims, radius, seed, planted)
    f = integrate(d, dims)
    assert np.abs(f).max() < 2 ** 21, "partial differences and sums must stay exact in f32"
    data = f.astype(dtype)
    inside = np.abs(d) < radius
    codes = np.where(inside, zigzag(d) if zz else d + radius, 0).astype(np.uint16)
    idx = np.flatnonzero(~inside)
    val = (d[idx] if zz else d[idx] + radius).astype(np.float32)
    return data, codes, idx.astype(np.uint32), val


# ---- the shapes and radii of test_gpu_lorenzo_matrix.py (test_delta_fields.py checks each on the CPU) ----
# layouts: what to set (None: the default) and what internals().layout must then say (cusz_amd.LAYOUT_*)
BRICK, REF, FORCE = 0, 1, 2
F32, F64 = np.float32, np.float64

# A. the instantiation matrix: reference layout, radius 512; x crosses the x-brick of 64 V
MATRIX_3D = [(260, 9, 9), (130, 9, 9), (65, 9, 9), (66, 17, 9), (33, 17, 9)]
MATRIX_2D = [(260, 33, 1), (130, 33, 1), (65, 33, 1), (35, 40, 1), (45, 37, 1)]
MATRIX_LATTICE = [(33, 17, 9), (66, 17, 9), (130, 9, 9), (35, 40, 1), (45, 37, 1), (65, 33, 1)]

# B. thin and tiny shapes, radius 512: (dims, layout to set, layout expected)
THIN_1D = [((n, 1, 1), lay, {None: BRICK, REF: REF}[lay]) for n in (1, 2, 3, 255, 256, 257, 1023, 1025)
           for lay in (None, REF)]
THIN = THIN_1D + [(d, REF, REF) for d in [(1, 2, 1), (1, 33, 1), (2, 2, 1), (3, 40, 1), (31, 33, 1), (33, 2, 1),
                                          (4, 300, 1)]]
THIN += [(d, FORCE, BRICK) for d in [(256, 2, 1), (260, 3, 1), (256, 9, 1)]]
THIN += [(d, REF, REF) for d in [(1, 1, 2), (1, 1, 9), (1, 2, 2), (2, 2, 2), (2, 1, 3), (1, 9, 9), (40, 1, 9), (7, 9, 8),
                                 (4, 1, 2), (260, 9, 2)]]
THIN += [(d, None, BRICK) for d in [(256, 1, 2), (256, 1, 9), (256, 2, 2), (512, 1, 17)]]

# C. the radius range: (dims, dtype, layout to set, layout expected, radii)
RADII = (1, 2, 3, 100, 127, 128, 129, 255, 300, 511)
RADII_F64_BRICK = (1, 127, 128, 129, 511)
RADIUS_SHAPES = [
    ((66, 17, 9), F32, REF, REF, RADII),
    ((33, 17, 9), F64, REF, REF, RADII),
    ((35, 40, 1), F32, REF, REF, RADII),
    ((16684, 1, 1), F32, None, BRICK, RADII),   # one full linear brick and a ragged one
    ((16684, 1, 1), F32, REF, REF, RADII),
    ((256, 13, 11), F32, None, BRICK, RADII),
    ((256, 13, 11), F64, None, BRICK, RADII_F64_BRICK),
    ((300, 40, 1), F32, FORCE, BRICK, RADII),
]
MODES_DIMS, MODES_RADII = (512, 16, 9), (1, 128, 511)   # codebook modes; fused region decode
REGION_RADII = (1, 129)
FZG_SHAPES, FZG_RADII = [(4097, 1, 1), (40, 24, 17)], (1, 3, 129, 511)
SCAN_DIMS, SCAN_RADIUS = (256, 32, 16), 129
# D. the delta field whose histogram the device codebook is built from at bklen = 2 radius
BOOK_DIMS, BOOK_BKLENS = (66, 17, 9), (2, 4, 6, 200, 254, 256, 258, 600, 1022)


def delta_cases():
    """Every (dims, radius, dtype, zz) a delta field is built for on the GPU."""
    out = set()
    for zz in (False, True):
        for dt in (F32, F64):
            out |= {(d, 512, dt, zz) for d in MATRIX_3D + MATRIX_2D}
            out |= {(d, 512, dt, zz) for d, _, _ in THIN}
        for d, dt, _, _, radii in RADIUS_SHAPES:
            out |= {(d, r, dt, zz) for r in radii}
        out |= {(MODES_DIMS, r, F32, zz) for r in MODES_RADII + REGION_RADII}
        out |= {(d, r, F32, zz) for d in FZG_SHAPES for r in FZG_RADII}
    out.add((SCAN_DIMS, SCAN_RADIUS, F32, False))
    out |= {(BOOK_DIMS, b // 2, F32, False) for b in BOOK_BKLENS}
    return sorted(out, key=lambda c: (c[0], c[1], np.dtype(c[2]).itemsize, c[3]))
