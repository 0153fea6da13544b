"""The edge fields do what the GPU tests need them to (CPU only, on the oracle's output): each
burst overflows exactly what it is meant to, the lattice reaches the code extremes, the outlier
predicate's edge, every seam, and -- for "order" -- the regime where the arithmetic is inexact.
Without these conditions test_gpu_outlier_burst.py and test_gpu_lattice.py could pass while
testing nothing."""
import numpy as np
import pytest

import edge_fields as ef

SLOT = ef.slot_cap()            # 10 % of a brick's elements + 16
STEP = ef.stream_slot_cap()     # an eighth of it: one y-step's slot in the single-pass mode

LATTICE_SHAPES = [(512, 16, 9), (256, 13, 11), (40, 24, 17), (300, 40, 1), (70, 45, 1), (33068, 1, 1)]
ids = lambda s: "x".join(map(str, s))  # noqa: E731


def test_slot_geometry():
    assert ef.BRICK_ELEMS == 256 * 8 * 8 and SLOT == ef.BRICK_ELEMS // 10 + 16 and STEP == SLOT // 8
    assert (SLOT, STEP) == (1654, 206)  # the figures DESIGN.md quotes (pipeline.hh brick_slot_cap, kStreamSlots)


@pytest.fixture(scope="module")
def bursts(oracle):
    out = {}
    for kind in ("smooth", "ystep", "brick", "all"):
        for dtype in (np.float32, np.float64):
            if kind == "smooth":
                data, (dims, eb, radius) = ef.smooth_field(dtype), (ef.BURST_DIMS, ef.BURST_EB, ef.BURST_RADIUS)
            else:
                data, dims, eb, radius = ef.burst_field(kind, dtype)
            _, _, oi = oracle.lorenzo_c(data, dims, eb, radius)
            out[kind, dtype] = (data.size, *ef.brick_counts(oi, dims))
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_smooth_background_is_far_from_every_slot(bursts, dtype):
    n, per_brick, per_step = bursts["smooth", dtype]
    assert 0 < per_brick.sum() < 200 and per_step.max() < STEP // 4


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_ystep_burst_overflows_a_ystep_slot_only(bursts, dtype):
    n, per_brick, per_step = bursts["ystep", dtype]
    assert per_brick.max() <= SLOT, "no brick may pass its slot"
    b = int(np.argmax(per_step.max(1)))
    assert per_step[b].max() > STEP and per_brick[b] <= SLOT
    assert np.count_nonzero(per_step[b] > STEP) >= 2  # the noisy row and the row it predicts


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_brick_burst_overflows_one_slot_not_the_spill_list(bursts, dtype):
    n, per_brick, per_step = bursts["brick", dtype]
    bx, by, bz = ef.BURST_BRICK
    x, y, z = ef.BURST_DIMS
    sat = (bz * ((y + 7) // 8) + by) * (x // 256) + bx
    assert per_brick[sat] > SLOT and per_brick[sat] == per_brick.max()
    assert per_brick.sum() < n // 10
    assert per_brick[sat] - SLOT < ef.spill_cap(n)  # what overflows the slot fits the spill list


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_all_burst_overflows_every_slot_and_the_spill_list(bursts, dtype):
    n, per_brick, per_step = bursts["all", dtype]
    assert per_brick.sum() > ef.spill_cap(n) == n // 10 + 1024
    assert per_brick.min() > SLOT
    assert (per_brick - SLOT).sum() > ef.spill_cap(n)  # the spill list itself overflows


def test_2d_burst_pushes_one_linear_brick_past_its_slot(oracle):
    data, dims, eb, radius = ef.burst_field("brick2d")
    _, _, oi = oracle.lorenzo_c(data, dims, eb, radius)
    per_brick, per_step = ef.brick_counts(oi, dims)
    assert per_step is None and per_brick.size == 2
    assert per_brick[0] > SLOT and per_brick[1] <= SLOT and per_brick.sum() < data.size // 10 + 1024


@pytest.mark.parametrize("dims", LATTICE_SHAPES, ids=ids)
def test_lattice_spikes_cover_every_seam(dims):
    spikes = ef.lattice_spikes(dims)
    tile = ef.tile_of(dims)
    for axis, seams in enumerate((ef.SEAMS_X, ef.SEAMS_YZ, ef.SEAMS_YZ)):
        want = {s for s in seams if s < dims[axis]} | {dims[axis] - 1}
        assert want <= {p[axis] for p in spikes}, (axis, want)
    # first and last element, every height; spikes of one tile that touch share a height (a plateau)
    assert {(0, 0, 0), tuple(d - 1 for d in dims)} <= {p[:3] for p in spikes}
    assert {p[3] for p in spikes} == set(ef.spike_heights(512))
    for i, p in enumerate(spikes):
        for q in spikes[:i]:
            if all(a // t == b // t for a, b, t in zip(p, q, tile)) and \
                    max(abs(a - b) for a, b in zip(p[:3], q[:3])) <= 1:
                assert p[3] == q[3], (p, q)


@pytest.mark.parametrize("radius", [512, 64])
@pytest.mark.parametrize("zigzag", [False, True], ids=["plain", "zigzag"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("dims", LATTICE_SHAPES, ids=ids)
def test_exact_lattice_reaches_the_code_extremes_and_round_trips(oracle, dims, dtype, zigzag, radius):
    r = radius
    data = ef.lattice_field(dims, dtype, "exact", r)
    assert np.all(data == np.round(data)) and np.abs(data).max() < 2 ** 23
    codes, ov, oi = oracle.lorenzo_c(data, dims, 0.5, r, zigzag)
    hist = oracle.histogram(codes, 2 * r)
    # delta = -(r - 1) and r - 1: the smallest and largest code a quantised delta takes
    lo, hi = (2 * r - 3, 2 * r - 2) if zigzag else (1, 2 * r - 1)
    assert hist[lo] > 0 and hist[hi] > 0
    # |delta| == r is the first outlier (the predicate is |delta| < r); cells hold delta (+ r)
    delta = ov - (0 if zigzag else r)
    assert np.any(delta == r) and np.any(delta == -r)
    assert {r + 1, -(r + 1), 2 * r, -3 * r} <= set(delta.tolist())
    assert np.all(codes[oi] == 0)
    out = oracle.lorenzo_x(codes, ov, oi, dims, 0.5, r, zigzag, dtype)
    np.testing.assert_array_equal(out.view(np.uint8), data.view(np.uint8))  # bit for bit


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("dims", LATTICE_SHAPES, ids=ids)
def test_ties_lattice_reconstructs_to_round_half_away(oracle, dims, dtype):
    data = ef.lattice_field(dims, dtype, "ties")
    frac = np.abs(data - np.trunc(data))
    half = dtype(0.5)
    for v in (half, np.nextafter(half, dtype(0)), np.nextafter(half, dtype(1)), dtype(0)):
        assert np.any(frac == v), v
    assert np.any(np.signbit(data) & (data == 0)) and np.any((data != 0) & (np.abs(data) < np.finfo(dtype).tiny))
    if dtype == np.float32:  # the literals the rounding shortcut is built around
        assert {np.float32(0.49999997), np.float32(-0.49999997), np.float32(0.50000006)} <= set(data.tolist())
    codes, ov, oi = oracle.lorenzo_c(data, dims, 0.5)
    out = oracle.lorenzo_x(codes, ov, oi, dims, 0.5, dtype=dtype)
    want = ef.round_half_away(data)
    assert np.any(want != np.rint(data))  # half-away differs from half-even on this field
    np.testing.assert_array_equal(out, want)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("dims", LATTICE_SHAPES, ids=ids)
def test_near_ties_lattice_straddles_the_tie(oracle, dims, dtype):
    eb = ef.lattice_eb("near_ties")
    data = ef.lattice_field(dims, dtype, "near_ties")
    scaled = data * dtype(1.0 / (2 * eb))  # what the kernels round, in their own type
    frac = np.abs(scaled - np.trunc(scaled))
    assert np.any(frac == 0.5) and np.any(frac < 0.5) and np.any(frac > 0.5)
    assert np.all(np.abs(frac - 0.5) < 1e-3)
    codes, ov, oi = oracle.lorenzo_c(data, dims, eb)
    assert len(oi) < data.size // 10
    out = oracle.lorenzo_x(codes, ov, oi, dims, eb, dtype=dtype)
    assert np.max(np.abs(out.astype(np.float64) - data)) <= 1.001 * eb


@pytest.mark.parametrize("zigzag", [False, True], ids=["plain", "zigzag"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("dims", LATTICE_SHAPES, ids=ids)
def test_order_lattice_is_in_the_inexact_regime(oracle, dims, dtype, zigzag):
    data = ef.lattice_field(dims, dtype, "order")
    assert np.all(np.isfinite(data)) and np.abs(data).max() >= (2.0 ** 23 if dtype == np.float32 else 2.0 ** 52)
    codes, ov, oi = oracle.lorenzo_c(data, dims, 0.5, 512, zigzag)
    out = oracle.lorenzo_x(codes, ov, oi, dims, 0.5, 512, zigzag, dtype)
    assert np.all(np.isfinite(out))
    assert np.count_nonzero(out != data) >= 1, "every sum exact: the field cannot tell one order from another"


@pytest.mark.parametrize("zigzag", [False, True], ids=["plain", "zigzag"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("dims", [d for d in LATTICE_SHAPES if d[1] > 1], ids=ids)
def test_order_lattice_tells_the_difference_orders_apart(oracle, dims, dtype, zigzag):
    """Predicting with the axes differenced in another order changes quant codes of the "order"
    field -- not only outlier values, which f32 cells would hide for f64 -- while on the "exact"
    field every order gives the oracle's codes."""
    ref_order, others = ("zxy", ("xzy", "yxz", "xyz")) if dims[2] > 1 else ("yx", ("xy",))
    r = 512

    def codes_of(delta):
        q = np.abs(delta) < r
        d = np.where(q, delta, 0).astype(np.int64)
        return np.where(q, (d << 1) ^ (d >> 63) if zigzag else d + r, 0).astype(np.uint16)

    for flavour in ("exact", "order"):
        data = ef.lattice_field(dims, dtype, flavour)
        codes, _, _ = oracle.lorenzo_c(data, dims, 0.5, r, zigzag)
        np.testing.assert_array_equal(codes_of(ef.lorenzo_deltas(data, dims, 0.5, ref_order)), codes)
        for o in others:
            differ = np.count_nonzero(codes_of(ef.lorenzo_deltas(data, dims, 0.5, o)) != codes)
            assert (differ == 0) if flavour == "exact" else (differ >= 1), (flavour, o, differ)
