"""Fields for the edges of the brick path, built on the CPU (a plain helper module, no tests).

Outlier bursts (burst_field): a smooth field with noise on a part of it, so that one brick's
outlier slot (10 % of its elements + 16), one y-step's share of it (the single-pass mode gives each
of a brick's eight y-steps an eighth) or the field's spill list (10 % of its elements + 1024)
overflows.  test_edge_fields.py checks on the oracle's output that each kind overflows what it is
meant to and nothing else.

Lattice values (lattice_field): fields whose prequantised values sit on the edges of the number
format and of the quantiser -- deltas exactly at +-(radius - 1), +-radius, +-(radius + 1), rounding
ties and their float neighbours, -0.0, a denormal, magnitudes from 2^23 (f64: 2^52) up where the
differences and partial sums stop being exact -- placed at the structural seams of the kernels:
x in {0, 7, 8, 63, 64, 255, 256, last}, y and z in {0, 7, 8, last}.

Finite values only, and every in * ebx2_r stays finite: NaN and Inf are out of scope (the reference
gives them no defined result either).
"""
import numpy as np

from cusz_amd import datagen

# ---- brick geometry (cusz_amd/csrc/brick_scan.hip brick_geom, pipeline.cc Pipeline::init) ----------------------
BRICK_X, BRICK_Y, BRICK_Z = 256, 8, 8       # a 3-D brick
BRICK_ELEMS = BRICK_X * BRICK_Y * BRICK_Z   # also a linear (1-D, 2-D) brick's consecutive elements
STREAM_SLOTS = 8                            # single-pass mode: one slot per y-step of a brick


def slot_cap(brick_elems=BRICK_ELEMS):
    """Outlier cells a brick's slot holds before any growth."""
    return brick_elems // 10 + 16


def stream_slot_cap(brick_elems=BRICK_ELEMS):
    """... and one y-step's share of it in the single-pass mode."""
    return slot_cap(brick_elems) // STREAM_SLOTS


def spill_cap(n):
    """Cells of the shared spill list before any growth."""
    return n // 10 + 1024


def brick_counts(ol_idx, dims):
    """Outliers per brick -> (per_brick[nbricks], per_ystep[nbricks, 8]); brick index
    (bz * nby + by) * nbx + bx.  Fields with y == 1 or z == 1 lie on linear bricks of BRICK_ELEMS
    consecutive elements, which have no y-steps: per_ystep is None."""
    x, y, z = dims
    idx = np.asarray(ol_idx, np.int64)
    if z == 1:
        nb = (x * y + BRICK_ELEMS - 1) // BRICK_ELEMS
        return np.bincount(idx // BRICK_ELEMS, minlength=nb), None
    gx, gy, gz = idx % x, idx // x % y, idx // (x * y)
    nbx, nby, nbz = x // BRICK_X, (y + BRICK_Y - 1) // BRICK_Y, (z + BRICK_Z - 1) // BRICK_Z
    b = (gz // BRICK_Z * nby + gy // BRICK_Y) * nbx + gx // BRICK_X
    per_step = np.bincount(b * 8 + gy % 8, minlength=8 * nbx * nby * nbz).reshape(-1, 8)
    return per_step.sum(1), per_step


# ---- outlier bursts ----------------------------------------------------------------------------
BURST_DIMS = (512, 24, 17)   # 2 x 3 x 3 bricks, the last z layer one plane thick
BURST_EB, BURST_RADIUS = 1e-3, 512
BURST_BRICK = (0, 1, 1)      # (bx, by, bz) of the brick that "brick" saturates
BURST2D_DIMS = (300, 97, 1)  # two linear bricks (the second ragged)


def smooth_field(dtype=np.float32):
    """The burst fields' background alone: a handful of outliers, no slot anywhere near full."""
    return datagen.smooth3d_np(BURST_DIMS, 7, dtype=dtype)


def burst_field(kind, dtype=np.float32):
    """-> (data, dims, eb, radius).  kind:
    "ystep":   noise on z 8:12, y 11, x 256:356 -- two y-steps of one brick pass their eighth of
               the slot, the brick as a whole stays inside it;
    "brick":   noise on one whole brick -- far past its slot, the field total below the spill list;
    "all":     uniform(-1e3, 1e3) everywhere -- every slot and the spill list overflow;
    "brick2d": 300 x 97 (linear bricks when forced), noise on rows 10:20 of the first brick: about
               twice its slot (the brick slots share a buffer with the reference layout's, sized
               by the larger: they must outgrow those for the growth to show in the capacity)."""
    rng = np.random.default_rng(1)
    if kind == "brick2d":
        x, y, _ = BURST2D_DIMS
        f = datagen.cesm2d_np((x, y), 7, dtype=np.float64).reshape(y, x)
        f[10:20, :] += rng.standard_normal((10, x)) * 50
        return f.astype(dtype).ravel(), BURST2D_DIMS, BURST_EB, BURST_RADIUS
    x, y, z = BURST_DIMS
    f = datagen.smooth3d_np(BURST_DIMS, 7, dtype=np.float64).reshape(z, y, x)
    if kind == "ystep":
        f[8:12, 11, 256:356] += rng.standard_normal((4, 100)) * 50
    elif kind == "brick":
        bx, by, bz = BURST_BRICK
        f[8 * bz:8 * bz + 8, 8 * by:8 * by + 8, 256 * bx:256 * bx + 256] += rng.standard_normal((8, 8, 256)) * 50
    elif kind == "all":
        f = rng.uniform(-1e3, 1e3, (z, y, x))
    else:
        raise ValueError(kind)
    return f.astype(dtype).ravel(), BURST_DIMS, BURST_EB, BURST_RADIUS


# ---- lattice values ----------------------------------------------------------------------------
SEAMS_X = (0, 7, 8, 63, 64, 255, 256)
SEAMS_YZ = (0, 7, 8)
SEAMS_1D = (1023, 1024, 16383, 16384)  # 1-D fields also: the tile's and the linear brick's border
FLAVOURS = ("exact", "ties", "near_ties", "order")


def lattice_eb(flavour):
    return 1e-3 if flavour == "near_ties" else 0.5


def seam_positions(extent, seams):
    """The seam positions that exist on an axis of this extent (the last element among them)."""
    return sorted({s for s in seams if s < extent} | {extent - 1})


def tile_of(dims):
    """The Lorenzo tile, inside which prediction runs: 8^3, 32^2 or 1024 (lrz_c.cuhip.inl)."""
    x, y, z = dims
    return (8, 8, 8) if z > 1 else (32, 32, 1) if y > 1 else (1024, 1, 1)


def spike_heights(radius):
    r = radius
    return (r - 1, -(r - 1), r, -r, r + 1, -(r + 1), 2 * r, -3 * r)


def lattice_spikes(dims, radius=512):
    """-> [(x, y, z, height)]: point spikes on the cross product of the axes' seam positions.  Two
    seam positions that are neighbours inside one tile (x = 7 and 8 in a 1-D or 2-D tile) form a
    plateau: the later spike takes the height of the one it touches, so that with the background
    zeroed in the tile every delta around the spikes is 0 or +-height exactly."""
    x, y, z = dims
    tx, ty, tz = tile_of(dims)
    sx = seam_positions(x, SEAMS_X + (SEAMS_1D if y == 1 and z == 1 else ()))
    sy, sz = seam_positions(y, SEAMS_YZ), seam_positions(z, SEAMS_YZ)
    hs = spike_heights(radius)
    placed, fresh = [], 0  # fresh: spikes so far that did not join a plateau
    for iz, gz in enumerate(sz):
        for iy, gy in enumerate(sy):
            for ix, gx in enumerate(sx):
                p = (gx, gy, gz)
                touched = {q[3] for q in placed
                           if (p[0] // tx, p[1] // ty, p[2] // tz) == (q[0] // tx, q[1] // ty, q[2] // tz)
                           and all(abs(a - b) <= 1 for a, b in zip(p, q))}
                assert len(touched) <= 1, "a spike touches plateaus of two heights"
                if touched:
                    placed.append(p + (touched.pop(),))
                else:
                    placed.append(p + (hs[(fresh + 3 * iy + 5 * iz) % len(hs)],))
                    fresh += 1
    return placed


def _walk(n, rng, dtype):
    return np.cumsum(rng.integers(-3, 4, n)).astype(dtype)


def _big_spikes(dtype):
    if np.dtype(dtype) == np.float32:
        return (2.0 ** 23 + 1, -(2.0 ** 24 + 2), 3e9)
    return (2.0 ** 52 + 1, -(2.0 ** 53 + 2), 1e19)


def round_half_away(v):
    """roundf / round in the array's own type: the fraction v - trunc(v) is exact."""
    t = np.trunc(v)
    return np.where(np.abs(v - t) >= 0.5, t + np.copysign(1, v).astype(v.dtype), t).astype(v.dtype)


def lorenzo_deltas(data, dims, eb, order):
    """The Lorenzo prediction errors of a field in plain numpy, every operation one IEEE operation
    in the array's type: prequantise, then difference along the axes in `order` (e.g. "zxy", the
    reference's for 3-D; "yx" for 2-D), each inside its tile with 0 before the tile's first element."""
    x, y, z = dims
    dtype = data.dtype.type
    p = round_half_away(data * dtype(1.0 / (2 * eb))).reshape(z, y, x)
    for ax in order:
        axis, tile = {"x": (2, tile_of(dims)[0]), "y": (1, tile_of(dims)[1]), "z": (0, tile_of(dims)[2])}[ax]
        prev = np.roll(p, 1, axis)
        first = np.arange(p.shape[axis]) % tile == 0
        prev[tuple(first if a == axis else slice(None) for a in range(3))] = 0
        p = p - prev
    return p.reshape(-1)


def lattice_field(dims, dtype, flavour, radius=512):
    """-> flat array of dims (x fastest), for compression at lattice_eb(flavour).
    "exact":     integers (a +-3 random walk) with the point spikes of lattice_spikes(); the walk is
                 zeroed in each spike's tile, so the deltas around it are +-height exactly and
                 every |p| < 2^23: all arithmetic exact, the round trip returns the input;
    "ties":      small integers k, k +- 0.5 and the float neighbours of those ties on either side
                 (around 0: 0.49999997, 0.50000006), with -0.0 and a denormal sprinkled in;
    "near_ties": (k + 0.5) * 2 eb at eb = 1e-3 and its two float neighbours, k a slow walk;
    "order":     "exact" plus spikes of 2^23 + 1, -(2^24 + 2), 3e9 (f64: 2^52 + 1, -(2^53 + 2),
                 1e19): differences and partial sums round, so the operation order shows."""
    x, y, z = dims
    n = x * y * z
    dtype = np.dtype(dtype).type
    seed = 7919 * x + 31 * y + z + FLAVOURS.index(flavour)
    rng = np.random.default_rng(seed)
    if flavour in ("exact", "order"):
        f = _walk(n, rng, dtype).reshape(z, y, x)
        tx, ty, tz = tile_of(dims)
        spikes = lattice_spikes(dims, radius)
        for gx, gy, gz, _ in spikes:
            f[gz // tz * tz:(gz // tz + 1) * tz, gy // ty * ty:(gy // ty + 1) * ty, gx // tx * tx:(gx // tx + 1) * tx] = 0
        for gx, gy, gz, h in spikes:
            f[gz, gy, gx] = h
        f = f.reshape(-1)
        if flavour == "order":
            big = _big_spikes(dtype)
            # in pairs along x, the second with an odd offset: the difference of two such values
            # (and 3e9 +- anything odd) has no exact representation
            pos = np.concatenate(([0, n - 2], rng.choice(n - 1, 12, replace=False)))
            for i, p in enumerate(pos):
                f[p] += dtype(big[i % 3])
                f[p + 1] += dtype(big[(i + 1) % 3]) + dtype(3)
            # and 2 x 2 clusters {0, -+3; B, B} across the axis differenced first (3-D: z, 2-D: y)
            # and x: B - -+3 rounds before the other B cancels it, so the small delta that is left
            # -- a quant code -- is 2 or 4 in one order and 3 in the other
            if y > 1:
                f = f.reshape(z, y, x)
                tx, ty, tz = tile_of(dims)
                for i in range(9):
                    gx = int(rng.integers(0, x // tx)) * tx + int(rng.integers(1, min(tx, x)))
                    gy = int(rng.integers(0, y))
                    gz = int(rng.integers(0, z))
                    if z > 1:
                        gz = min(z - 1, gz // tz * tz + int(rng.integers(1, tz)))
                        lo = (gz - 1, gy)
                    else:
                        gy = min(y - 1, gy // ty * ty + int(rng.integers(1, ty)))
                        lo = (gz, gy - 1)
                    if gx >= x or (z > 1 and gz % tz == 0) or (z == 1 and gy % ty == 0):
                        continue
                    b = dtype(big[i % 3])
                    f[lo[0], lo[1], gx - 1], f[lo[0], lo[1], gx] = 0, -3 * np.sign(b)
                    f[gz, gy, gx - 1], f[gz, gy, gx] = b, b
                f = f.reshape(-1)
        return f
    if flavour == "ties":
        k = rng.integers(-8, 9, n).astype(dtype)
        sign = np.where(rng.random(n) < 0.5, -1, 1).astype(dtype)
        sign = np.where(k != 0, np.sign(k), sign).astype(dtype)
        tie = sign * (np.abs(k) + dtype(0.5))
        cat = rng.integers(0, 4, n)
        f = np.select([cat == 0, cat == 1, cat == 2], [k, tie, np.nextafter(tie, dtype(0))],
                      np.nextafter(tie, sign * dtype(np.inf))).astype(dtype)
        tiny = dtype(1e-40) if dtype == np.float32 else dtype(1e-310)
        special = rng.choice(n, min(64, n // 4), replace=False)
        f[special[0::4]] = dtype(-0.0)
        f[special[1::4]] = tiny
        f[special[2::4]] = -tiny
        f[special[3::4]] = dtype(0.0)
        f[0], f[n - 1] = dtype(-0.0), tiny
        return f
    if flavour == "near_ties":
        k = np.cumsum(rng.integers(-1, 2, n)).astype(np.float64)
        tie = ((k + 0.5) * (2 * lattice_eb(flavour))).astype(dtype)
        cat = rng.integers(0, 3, n)
        return np.select([cat == 0, cat == 1], [tie, np.nextafter(tie, dtype(-np.inf))],
                         np.nextafter(tie, dtype(np.inf))).astype(dtype)
    raise ValueError(flavour)

