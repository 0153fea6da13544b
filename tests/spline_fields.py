"""Fields for the edges of the spline3 path, built on the CPU (a plain helper module, no tests).

The spline kernels (cusz_amd/csrc/spline.hip) work tile by tile; a field is an edge case for them
through WHERE its outliers fall (which tile, how many per tile, on which face) and through WHAT
its codes are (the quantiser's edges, the range an outlier cell carries).  test_spline_fields.py
checks on the oracle's output that each field here hits what it is meant to and nothing else;
test_gpu_spline_edges.py runs them through the bit-exact chain on the GPU.

Finite values only: an infinite value leaves the spline code domain (include/cusz_amd.h,
PSZ_AMD_ERR_CODE_RANGE) like the too-high spikes of range_spike(); a NaN has no defined result.
"""
import numpy as np

from cusz_amd import datagen

# ---- geometry ----------------------------------------------------------------------------------
TILE = (32, 8, 8)     # spline.hip: kSX - 1, kSY - 1, kSZ - 1 (:33); spline_geom (:563-570)
PREFETCH = 768        # spline.hip k_spline3_x: kEnt * kSplThreads = 3 * 256 entries in registers (:423, :523)
SCAN_CHUNK = 1024     # spline.hip k_spl_bucket_scan: tiles per pass of its carry loop (:372)
CODE_EXACT = 1 << 24  # every int up to here is a float: what an outlier cell carries (spline.hip :39-44)
CODE_LIM = (1 << 31) - 1024  # |code / 2| below this (spline.hip kSplCodeLim, :45)


def slot_cap(dims):
    """Outlier cells a tile's slot holds (pipeline.cc Pipeline::init: spl_cap)."""
    x, y, z = dims
    return min(x, 32) * min(y, 8) * min(z, 8) // 10 + 16


def spill_cap(n):
    """Cells of the shared spill list before any growth (pipeline.cc Pipeline::init: spill_cap)."""
    return n // 10 + 1024


def tile_grid(dims):
    x, y, z = dims
    return (x + 31) // 32, (y + 7) // 8, (z + 7) // 8


def ntiles(dims):
    gx, gy, gz = tile_grid(dims)
    return gx * gy * gz


def tile_of(idx, dims):
    """Tile index (x fastest over tiles) of flat element indices."""
    x, y, _ = dims
    gx, gy, _ = tile_grid(dims)
    idx = np.asarray(idx, np.int64)
    return idx % x // 32 + gx * (idx // x % y // 8 + gy * (idx // (x * y) // 8))


def tile_counts(ol_idx, dims):
    """Outliers per tile."""
    return np.bincount(tile_of(ol_idx, dims), minlength=ntiles(dims))


def group_totals(counts, dims):
    """Per tile: the cells of the tile and its seven upper neighbours, which k_spline3_x walks for
    the tile and its +1 faces (ranges_of, spline.hip :428-437)."""
    gx, gy, gz = tile_grid(dims)
    c = np.zeros((gz + 1, gy + 1, gx + 1), np.int64)
    c[:gz, :gy, :gx] = np.asarray(counts).reshape(gz, gy, gx)
    tot = sum(c[dz:gz + dz, dy:gy + dy, dx:gx + dx] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1))
    return tot.ravel()


def flat(p, dims):
    return p[0] + dims[0] * (p[1] + dims[1] * p[2])


def level_eb(unit, eb):
    """(eb_r, ebx2) of an interpolation level as floats (spl_level_eb, spline.hip :125-136)."""
    eb_r0, ebx20 = np.float32(1.0 / eb), np.float32(eb * 2.0)
    eb_r, ebx2 = eb_r0, ebx20
    t = 1
    while t < unit:
        eb_r = np.float32(np.float64(eb_r) * 1.25)
        ebx2 = np.float32(np.float64(ebx2) / 1.25)
        t *= 2
    if np.float64(ebx2) < np.float64(ebx20) / 2.0:
        ebx2 = np.float32(np.float64(ebx20) / 2.0)
        eb_r = np.float32(np.float64(eb_r0) * 2.0)
    return eb_r, ebx2


# ---- smooth background ---------------------------------------------------------------------------
SMOOTH_EB = 3e-6

# shapes below a tile in some axis, exact tile multiples, last tiles one point thick, ndiv (X or Y
# below 2: k_spline3_x divides instead of multiplying, spline.hip :613)
SHAPES = [
    ((1, 1, 1), None), ((2, 1, 1), None), ((7, 3, 2), None), ((8, 8, 8), None), ((9, 9, 9), None),
    ((31, 7, 7), None), ((32, 8, 8), None), ((64, 16, 16), None), ((65, 17, 17), None),
    ((1, 9, 9), None), ((40, 1, 9), None), ((257, 1, 1), np.float64), ((45, 37, 1), np.float32),
]
# tile counts around the 8 of TileOrder's per-XCD branch (spline.hip :170-180)
GRIDS = {1: (32, 8, 8), 7: (224, 8, 8), 8: (256, 8, 8), 9: (96, 24, 8), 15: (96, 40, 8), 16: (256, 16, 8),
         17: (544, 8, 8)}


def smooth(dims, dtype=np.float32, seed=5):
    return datagen.smooth3d_np(dims, seed, dtype=dtype)


def big_dims(multi_processor_count):
    """A field with more tiles than any grid (the occupancy ceiling of 256-thread blocks is 8 per CU)
    and a tile count that is no multiple of 8, ragged on every axis: (410, 100, 99) = 13^3 tiles on
    up to 274 CUs, a thicker field beyond."""
    x, y, z = 410, 100, 99
    while ntiles((x, y, z)) <= 8 * multi_processor_count or ntiles((x, y, z)) % 8 == 0:
        z += 8
    return x, y, z


# ---- outlier loads -------------------------------------------------------------------------------
NOISE_DIMS = (96, 24, 24)  # 3 x 3 x 3 full tiles
NOISE_EB = 1e-3
NOISE_TILES = {"centre": [(1, 1, 1)], "three": [(0, 0, 0), (2, 2, 0), (0, 2, 2)]}


def noise_on_tiles(dims, tiles, dtype, amp=10.0, seed=11):
    """smooth + uniform(-amp, amp) on the listed tiles ((bx, by, bz); None: everywhere)."""
    x, y, z = dims
    f = smooth(dims, np.float64).reshape(z, y, x)
    rng = np.random.default_rng(seed)
    noise = rng.uniform(-amp, amp, f.shape)
    if tiles is None:
        f = f + noise
    else:
        for bx, by, bz in tiles:
            s = np.s_[bz * 8:bz * 8 + 8, by * 8:by * 8 + 8, bx * 32:bx * 32 + 32]
            f[s] += noise[s]
    return f.astype(dtype).ravel()


def noise_field(kind, dtype):
    """-> data on NOISE_DIMS at NOISE_EB.  "centre": one tile far past its slot (one ranged spill);
    "three": three tiles that touch nowhere (reservations race on the spill counter); "all": every
    tile, past the spill list (the list grows and the compress repeats), every tile group far past
    the prefetched entries."""
    return noise_on_tiles(NOISE_DIMS, None if kind == "all" else NOISE_TILES[kind], dtype)


def scattered_tiles(dims, every=7):
    gx, gy, gz = tile_grid(dims)
    x, y, z = dims
    full = [(t % gx, t // gx % gy, t // (gx * gy)) for t in range(0, gx * gy * gz, every)]
    return [(bx, by, bz) for bx, by, bz in full if bx * 32 < x and by * 8 < y and bz * 8 < z]


SCATTER_EB = 1e-2  # the smooth background alone has no outlier here


def scattered_noise(dims, dtype, every=7):
    """Noise on every 7th tile (ragged ones included): most tiles hold no cell."""
    x, y, z = dims
    f = smooth(dims, np.float64).reshape(z, y, x)
    rng = np.random.default_rng(3)
    for bx, by, bz in scattered_tiles(dims, every):
        s = np.s_[bz * 8:bz * 8 + 8, by * 8:by * 8 + 8, bx * 32:bx * 32 + 32]
        f[s] += rng.uniform(-10, 10, f[s].shape)
    return f.astype(dtype).ravel()


# ---- face cells ------------------------------------------------------------------------------------
FACE_DIMS = (96, 24, 24)
FACE_EB = 0.5
FACE_HEIGHT = 3000.0
# a cell of an upper neighbour on this tile's +1 faces (put, spline.hip :480-491): x face, the
# point before it, an x-y edge, a y face, a y-z edge -- and the same on the last tile's lower faces
_FACE_O = (64, 16, 16)  # origin of the last tile
# (33, 8, 5) and (5, 8, 8) have an odd x: points of the last stage, which a tile that is not the
# last of its axis leaves to the upper neighbour (spl_stage's INCL = false) -- the lower tile takes
# their cell in and never reads it.  (36, 8, 5) and (8, 8, 10) near them are read.
FACE_SPIKES = [(32, 3, 5), (31, 3, 5), (64, 8, 3), (33, 8, 5), (5, 8, 8), (36, 8, 5), (8, 8, 8 + 2),
               (_FACE_O[0], _FACE_O[1] + 3, _FACE_O[2] + 5), (_FACE_O[0] - 1, _FACE_O[1] + 3, _FACE_O[2] + 5),
               (_FACE_O[0], _FACE_O[1], _FACE_O[2] + 3), (_FACE_O[0] + 1, _FACE_O[1], _FACE_O[2] + 5),
               (_FACE_O[0] + 5, _FACE_O[1], _FACE_O[2]), (_FACE_O[0] + 4, _FACE_O[1], _FACE_O[2] + 5),
               (_FACE_O[0] + 10, _FACE_O[1], _FACE_O[2])]


def face_field(dtype):
    f = np.zeros(FACE_DIMS[::-1], dtype)
    for k, (px, py, pz) in enumerate(FACE_SPIKES):
        f[pz, py, px] = FACE_HEIGHT + 16 * k
    return f.ravel()


def lower_tiles(p, dims):
    """Tiles other than its own that hold point p on a +1 face."""
    gx, gy, _ = tile_grid(dims)
    own = (p[0] // 32, p[1] // 8, p[2] // 8)
    out = []
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                if (dx, dy, dz) == (0, 0, 0):
                    continue
                if (dx and p[0] % 32) or (dy and p[1] % 8) or (dz and p[2] % 8):
                    continue
                t = (own[0] - dx, own[1] - dy, own[2] - dz)
                if min(t) >= 0:
                    out.append(t)
    return out


# ---- division ---------------------------------------------------------------------------------------
# (X, Y) of noisy X x Y x 3 fields: powers of two, their neighbours, 2 and 3 for the magic-number
# division of k_spline3_x (spline.hip :605-614)
DIV_XY = [(2, 2), (3, 3), (2, 9), (3, 8), (31, 7), (32, 8), (33, 9), (127, 2), (128, 8), (129, 3), (128, 7)]


# ---- quantiser edges -------------------------------------------------------------------------------
QUANT_EB = 0.5
QUANT_DIMS = (259, 81, 50)  # 8 x 10 x 6 full tiles hold the spikes; ragged tiles beyond them
# one interior point of each of the nine stages (spl_interpolate, spline.hip :139-165), with its unit;
# only the first (unit 4 along z: x and y on the 8-lattice) has to lie on a face of its tile
STAGE_POINTS = [((8, 0, 4), 4), ((8, 4, 4), 4), ((4, 4, 4), 4),
                ((4, 4, 2), 2), ((4, 2, 2), 2), ((2, 2, 2), 2),
                ((2, 2, 1), 1), ((2, 1, 1), 1), ((1, 1, 1), 1)]


def quant_deltas(radius, dtype):
    """Code - radius of the spikes: kept and dropped codes at both ends of [0, 2 radius), and in f64
    the half-integer ties of the truncation with their nextafter neighbours."""
    r = radius
    d = [-(r + 1), -r, -(r - 1), r - 1, r, r + 1]
    if dtype == np.float64:
        for t in (-(r + 0.5), -(r - 0.5), r - 0.5, r + 0.5):
            d += [t, float(np.nextafter(t, 0.0)), float(np.nextafter(t, np.copysign(np.inf, t)))]
    return d


def quant_code(delta, radius):
    """The code of a spike of delta * ebx2 on a zero prediction: |err| * eb_r + 1 = 2 |delta| + 1,
    halved and truncated -> trunc(|delta| + 0.5), signed, + radius."""
    return int(np.copysign(np.floor(abs(delta) + 0.5), delta)) + radius


def quant_field(radius, dtype, stages=range(9)):
    """-> (data, spikes): zeros with one spike per tile; spikes = [(flat index, expected code)].
    A tile and the tile below it in y never both hold a spike (the first stage's point lies on
    that face), so every spike is predicted from zeros.  The expected code is None for a tie above
    unit 1: there eb_r * ebx2 is not exactly 2 (0.8f, 0.64f), the tie is not exactly reachable and
    the oracle alone says on which side the spike falls."""
    x, y, z = QUANT_DIMS
    f = np.zeros((z, y, x), dtype)
    free = [(bx, by, bz) for bz in range(6) for by in (0, 2, 4, 6, 8) for bx in range(8)]
    spikes = []
    k = 0
    for s in stages:
        (px, py, pz), unit = STAGE_POINTS[s]
        _, ebx2 = level_eb(unit, QUANT_EB)
        for d in quant_deltas(radius, dtype):
            bx, by, bz = free[k % len(free)]
            assert k < len(free), "more spikes than tiles"
            k += 1
            h = dtype(np.float64(d) * np.float64(ebx2))
            p = (bx * 32 + px, by * 8 + py, bz * 8 + pz)
            f[p[2], p[1], p[0]] = h
            spikes.append((flat(p, QUANT_DIMS), quant_code(d, radius) if unit == 1 or d == int(d) else None))
    return f.ravel(), spikes


# ---- values -------------------------------------------------------------------------------------------
VALUE_DIMS = (70, 19, 13)


def value_field(kind, dtype):
    """-> (data, eb) on VALUE_DIMS (ragged on every axis)."""
    x, y, z = VALUE_DIMS
    if kind == "constant":
        return np.full(x * y * z, 3.25, dtype), 1e-3
    if kind == "mean1e6":
        # a read of the zero padding outside the field would predict 0 next to 1e6: outliers
        return (1e6 + smooth(VALUE_DIMS, np.float64)).astype(dtype), 1e-2
    if kind == "zeros":
        f = np.zeros((z, y, x), dtype)
        tiny = np.finfo(dtype).smallest_subnormal
        f[2:5, 3:9, 10:40] = -0.0
        f[6:12, 7:15, 30:66] = tiny
        f[9:13, 15:19, 60:70] = -tiny * 3
        return f.ravel(), 1e-3
    if kind == "pow23":
        # f32 integers around 2^23, where the spacing of floats goes from 0.5 to 1
        assert dtype == np.float32
        rng = np.random.default_rng(9)
        f = 2.0 ** 23 - 1500 + np.round(2000 * smooth(VALUE_DIMS, np.float64)) + rng.integers(-3, 4, x * y * z)
        return f.astype(np.float32), 256.0
    raise ValueError(kind)


# ---- the code range ------------------------------------------------------------------------------------
RANGE_DIMS = (40, 9, 9)
RANGE_POINT = (5, 3, 3)  # a last-stage point (odd x): code = height + 512 at eb 0.5, radius 512
# (height, accepted in f32, accepted in f64): both sides of 2^24 and of the int limit, both signs
RANGE_SPIKES = [
    (CODE_EXACT - 512, True, True),            # code 2^24: the last int every float step reaches
    (CODE_EXACT - 511, True, False),           # 2^24 + 1: (float)code is 2^24
    (2 * CODE_EXACT + 2, True, False),
    (-CODE_EXACT - 512, True, True),           # code -2^24
    (-CODE_EXACT - 513, True, False),
    (CODE_LIM - 128 - 512, True, True),        # code 2^31 - 1152: a float, |code / 2| under the limit
    (CODE_LIM - 128, True, True),              # f32's last height under the limit; code + radius is an int
    (CODE_LIM - 127, True, False),             # (f32 rounds the height to the one above)
    (CODE_LIM, False, False),
    (-CODE_LIM + 128, True, True),
    (-CODE_LIM, False, False),
    (1 << 31, False, False),
    (-(1 << 31), False, False),
]


def range_spike(height, dtype):
    f = np.zeros(RANGE_DIMS[::-1], dtype)
    f[RANGE_POINT[2], RANGE_POINT[1], RANGE_POINT[0]] = height
    return f.ravel()


def range_noise(dtype=np.float64):
    """standard_normal * 1e3 on VALUE_DIMS: at eb 1e-5 codes reach 3e8, at 1e-6 they leave int."""
    return (np.random.default_rng(0).standard_normal(int(np.prod(VALUE_DIMS))) * 1e3).astype(dtype)
