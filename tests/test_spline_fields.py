"""The spline edge fields do what the GPU tests need them to (CPU only, on the oracle's output):
each lands its outliers where it is meant to -- over or under a tile's slot, the spill list, the
entries k_spline3_x prefetches -- its spikes get the intended codes, and the oracle's own round
trip holds the bound for every field the GPU is expected to accept.  Without these conditions
test_gpu_spline_edges.py could pass while testing nothing."""
import numpy as np
import pytest

import spline_fields as sf

DTYPES = [np.float32, np.float64]
dt_ids = ["f32", "f64"]
TOL = {np.float32: 1.005, np.float64: 1.001}  # the bound up to the float parameters (test_gpu_spline.py)


def roundtrip(oracle, data, dims, eb, radius=512):
    """-> (codes, ol_val, ol_idx, lost, max |error| / eb) of the oracle's own compress + decompress."""
    c, a, ov, oi, lost = oracle.spline3_c(data, dims, eb, radius, count_lost=True)
    x = oracle.spline3_x(c, a, ov, oi, dims, eb, radius)
    return c, ov, oi, lost, float(np.abs(x.astype(np.float64) - data).max()) / eb


def in_domain(oracle, data, dims, eb, radius=512):
    c, ov, oi, lost, err = roundtrip(oracle, data, dims, eb, radius)
    assert lost == 0 and err <= TOL[data.dtype.type], (lost, err)
    return c, ov, oi


def test_geometry():
    assert sf.slot_cap((96, 24, 24)) == 220 and sf.slot_cap((7, 3, 2)) == 20 and sf.slot_cap((1, 1, 1)) == 16
    assert sf.spill_cap(96 * 24 * 24) == 6553
    assert sf.ntiles((410, 100, 99)) == 13 ** 3 and sf.ntiles((32, 8, 8)) == 1 and sf.ntiles((33, 9, 9)) == 8
    assert [sf.ntiles(d) for d in sf.GRIDS.values()] == list(sf.GRIDS)
    # a tile's group: itself and the seven tiles above it
    c = np.arange(27)
    g = sf.group_totals(c, (96, 24, 24))
    assert g[26] == 26 and g[0] == 0 + 1 + 3 + 4 + 9 + 10 + 12 + 13 and g[13] == 13 + 14 + 16 + 17 + 22 + 23 + 25 + 26
    np.testing.assert_array_equal(sf.tile_of([0, 31, 32, 96 * 8, 96 * 24 * 8], (96, 24, 24)), [0, 0, 1, 3, 9])
    # level bounds at eb 0.5: (eb_r, ebx2) = (2, 1), (2.5, 0.8f), (3.125, 0.64f)
    assert [tuple(map(float, sf.level_eb(u, 0.5))) for u in (1, 2, 4)] == [
        (2.0, 1.0), (2.5, float(np.float32(0.8))), (3.125, float(np.float32(np.float64(np.float32(0.8)) / 1.25)))]


def test_big_field_outgrows_every_grid():
    assert sf.big_dims(256) == (410, 100, 99)
    for cus in (64, 256, 304, 1024):
        d = sf.big_dims(cus)
        assert sf.ntiles(d) > 8 * cus and sf.ntiles(d) % 8 and sf.ntiles(d) > sf.SCAN_CHUNK
        assert d[0] % 32 and d[1] % 8 and d[2] % 8


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_ids)
def test_smooth_shapes(oracle, dtype):
    """Every shape is in the domain; between them they have tiles over and under the slot and tile
    groups over and under the prefetched entries; none passes the spill list."""
    over = under = gover = gunder = 0
    for dims, only in sf.SHAPES + [(d, None) for d in sf.GRIDS.values()]:
        if only not in (None, dtype):
            continue
        _, _, oi = in_domain(oracle, sf.smooth(dims, dtype), dims, sf.SMOOTH_EB)
        tc = sf.tile_counts(oi, dims)
        over += int(np.count_nonzero(tc > sf.slot_cap(dims)))
        under += int(np.count_nonzero((tc > 0) & (tc <= sf.slot_cap(dims))))
        g = sf.group_totals(tc, dims)
        gover, gunder = gover + int(np.count_nonzero(g > sf.PREFETCH)), gunder + int(np.count_nonzero((g > 0) & (g <= sf.PREFETCH)))
        assert np.maximum(tc - sf.slot_cap(dims), 0).sum() <= sf.spill_cap(int(np.prod(dims)))
        if dims in ((1, 9, 9), (40, 1, 9)):
            assert oi.size > 0, "the ndiv shapes need outliers"
    assert over >= 10 and under >= 10 and gover >= 10 and gunder >= 10


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_ids)
def test_noise_fields(oracle, dtype):
    slot, n = sf.slot_cap(sf.NOISE_DIMS), int(np.prod(sf.NOISE_DIMS))
    tid = lambda t: t[0] + 3 * (t[1] + 3 * t[2])  # noqa: E731

    _, ov, oi = in_domain(oracle, sf.noise_field("centre", dtype), sf.NOISE_DIMS, sf.NOISE_EB)
    tc = sf.tile_counts(oi, sf.NOISE_DIMS)
    assert tc[13] > sf.PREFETCH > slot and np.all(np.delete(tc, 13) <= slot)  # one ranged spill
    assert np.count_nonzero(tc == 0) >= 20 and np.count_nonzero(tc) > 1  # the lower neighbours' faces
    assert tc.sum() - slot < sf.spill_cap(n)
    assert np.abs(ov).max() < sf.CODE_EXACT

    _, _, oi = in_domain(oracle, sf.noise_field("three", dtype), sf.NOISE_DIMS, sf.NOISE_EB)
    tc = sf.tile_counts(oi, sf.NOISE_DIMS)
    noisy = [tid(t) for t in sf.NOISE_TILES["three"]]
    assert all(tc[t] > slot for t in noisy) and np.all(np.delete(tc, noisy) <= slot)
    assert np.maximum(tc - slot, 0).sum() < sf.spill_cap(n)  # three reservations, the list holds them
    for a in sf.NOISE_TILES["three"]:
        for b in sf.NOISE_TILES["three"]:
            assert a == b or max(abs(p - q) for p, q in zip(a, b)) >= 2

    _, _, oi = in_domain(oracle, sf.noise_field("all", dtype), sf.NOISE_DIMS, sf.NOISE_EB)
    tc = sf.tile_counts(oi, sf.NOISE_DIMS)
    assert np.all(tc > sf.PREFETCH)
    assert np.maximum(tc - slot, 0).sum() > sf.spill_cap(n)  # the list overflows and grows
    assert sf.group_totals(tc, sf.NOISE_DIMS).min() > sf.PREFETCH

    # the background a manager compresses afterwards: nothing spills
    _, _, oi = in_domain(oracle, sf.smooth(sf.NOISE_DIMS, dtype), sf.NOISE_DIMS, sf.NOISE_EB)
    assert sf.tile_counts(oi, sf.NOISE_DIMS).max() <= slot


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_ids)
def test_face_spikes_reach_the_lower_tiles(oracle, dtype):
    """Every spike is an outlier cell; each of the face spikes lies on a +1 face of at least one
    lower tile, and dropping its cell changes what that tile reconstructs -- unless it is a point
    of the last stage (odd x), which the lower tile takes in and never reads."""
    data = sf.face_field(dtype)
    c, a, ov, oi, lost = oracle.spline3_c(data, sf.FACE_DIMS, sf.FACE_EB, count_lost=True)
    x = oracle.spline3_x(c, a, ov, oi, sf.FACE_DIMS, sf.FACE_EB)
    assert lost == 0 and np.abs(x.astype(np.float64) - data).max() <= TOL[dtype] * sf.FACE_EB
    X, Y, _ = sf.FACE_DIMS
    on_face = 0
    for p in sf.FACE_SPIKES:
        k = np.flatnonzero(oi == sf.flat(p, sf.FACE_DIMS))
        assert k.size == 1, p
        lower = sf.lower_tiles(p, sf.FACE_DIMS)
        on_face += bool(lower)
        keep = np.ones(oi.size, bool)
        keep[k] = False
        y = oracle.spline3_x(c, a, ov[keep], oi[keep], sf.FACE_DIMS, sf.FACE_EB)
        changed = np.flatnonzero(x != y)
        tiles = set(sf.tile_of(changed, sf.FACE_DIMS).tolist())
        for bx, by, bz in lower:
            assert (bx + 3 * (by + 3 * bz) in tiles) == (p[0] % 2 == 0), (p, (bx, by, bz))
    assert on_face == 12
    faces = [(p[0] % 32 == 0, p[1] % 8 == 0, p[2] % 8 == 0) for p in sf.FACE_SPIKES]
    assert {(True, False, False), (True, True, False), (False, True, False), (False, True, True)} <= set(faces)


def test_division_shapes_are_all_outliers(oracle):
    xs, ys = {x for x, _ in sf.DIV_XY}, {y for _, y in sf.DIV_XY}
    assert {2, 3, 31, 32, 33, 127, 128, 129} <= xs and {2, 3, 7, 8, 9} <= ys
    for x, y in sf.DIV_XY:
        dims = (x, y, 3)
        for dtype in DTYPES:
            _, _, oi = in_domain(oracle, sf.noise_on_tiles(dims, None, dtype), dims, sf.NOISE_EB)
            assert set((oi % x).tolist()) == set(range(x)) and set((oi // x % y).tolist()) == set(range(y))


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_ids)
def test_scattered_noise_leaves_most_tiles_empty(oracle, dtype):
    dims = sf.big_dims(256)
    _, _, oi = in_domain(oracle, sf.scattered_noise(dims, dtype), dims, sf.SCATTER_EB)
    tc = sf.tile_counts(oi, dims)
    assert 0.1 * tc.size < np.count_nonzero(tc) < 0.2 * tc.size
    assert tc[sf.SCAN_CHUNK:].sum() > 1000 and tc[2 * sf.SCAN_CHUNK:].sum() > 1000  # two carries of the scan


@pytest.mark.parametrize("radius", [512, 256, 64])
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_ids)
def test_quantiser_spikes_get_their_codes(oracle, dtype, radius):
    data, spikes = sf.quant_field(radius, dtype)
    c, ov, oi, lost, err = roundtrip(oracle, data, sf.QUANT_DIMS, sf.QUANT_EB, radius)
    assert lost == 0 and err <= 1.0  # exact arithmetic on this lattice: the plain bound
    cell = dict(zip(oi.tolist(), ov.tolist()))
    assert len(spikes) == 9 * (6 if dtype == np.float32 else 18)
    got = set()
    for idx, want in spikes:
        code = int(cell[idx]) if idx in cell else int(c[idx])
        assert (idx in cell) == (not 0 <= code < 2 * radius)
        if want is not None:
            assert code == want, (idx, code, want)
        got.add(code)
    # kept and dropped codes at both ends, the kept 0 (the placeholder's value) among them
    assert {-1, 0, 1, 2 * radius - 1, 2 * radius, 2 * radius + 1} <= got
    assert any(int(c[i]) == 0 and i not in cell for i, _ in spikes)
    tiles = sf.tile_of([i for i, _ in spikes], sf.QUANT_DIMS)
    assert np.unique(tiles).size == len(spikes), "one spike per tile"


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_ids)
def test_value_fields(oracle, dtype):
    c, _, oi = in_domain(oracle, *_vf("constant", dtype))
    assert oi.size == 0 and np.all(c == 512)
    c, _, oi = in_domain(oracle, *_vf("mean1e6", dtype))
    assert oi.size == 0 and np.unique(c).size > 8  # a zero read in place of 1e6 would be an outlier
    data, dims, eb = _vf("zeros", dtype)
    assert np.count_nonzero(np.signbit(data) & (data == 0)) > 100 and np.count_nonzero(data) > 1000
    assert np.abs(data).max() < np.finfo(dtype).tiny
    c, _, oi = in_domain(oracle, data, dims, eb)
    assert oi.size == 0 and np.all(c == 512)
    if dtype == np.float32:
        data, dims, eb = _vf("pow23", dtype)
        assert data.min() < 2.0 ** 23 - 1000 and data.max() > 2.0 ** 23 + 1000 and np.all(data == np.round(data))
        in_domain(oracle, data, dims, eb)


def _vf(kind, dtype):
    data, eb = sf.value_field(kind, dtype)
    return data, sf.VALUE_DIMS, eb


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_ids)
def test_range_spikes(oracle, dtype):
    """The spike table: which heights the oracle counts as lost, the code each accepted one gets,
    and what ignoring the count costs (the defect the status closes)."""
    for h, ok32, ok64 in sf.RANGE_SPIKES:
        data = sf.range_spike(h, dtype)
        c, ov, oi, lost, err = roundtrip(oracle, data, sf.RANGE_DIMS, 0.5)
        ok = ok32 if dtype == np.float32 else ok64
        assert (lost == 0) == ok, (h, lost)
        idx = sf.flat(sf.RANGE_POINT, sf.RANGE_DIMS)
        if ok:
            assert oi.tolist() == [idx] or abs(h) < 512
            # the code is height + 512, in the arithmetic of the dtype (spl_stage's COMP branch)
            code = np.abs(dtype(h)) * dtype(2) + dtype(1)
            want = int(np.copysign(np.floor(code / dtype(2)), h)) + 512
            assert want == h + 512 or dtype == np.float32
            assert float(ov[0]) == float(np.float32(want)), (h, ov)
            assert err * 0.5 <= max(0.5, float(np.spacing(dtype(abs(h))))), (h, err)
        elif dtype == np.float64 and abs(h) < sf.CODE_LIM:
            assert err >= 2.0, (h, err)  # the bound breaks silently: 2 eb and more
    heights = [h for h, _, _ in sf.RANGE_SPIKES]
    assert sf.CODE_EXACT - 512 in heights and sf.CODE_EXACT - 511 in heights and 1 << 31 in heights
    assert any(h < 0 for h in heights)


def test_range_noise_is_out_of_domain(oracle):
    data = sf.range_noise()
    _, ov, _, lost, err = roundtrip(oracle, data, sf.VALUE_DIMS, 1e-5)
    assert lost > 0 and sf.CODE_EXACT < np.abs(ov).max() < sf.CODE_LIM and err > 10
    _, _, _, lost, err = roundtrip(oracle, data, sf.VALUE_DIMS, 1e-6)
    assert lost > 0 and err > 1e9  # codes leave int
    # the same field in its domain
    in_domain(oracle, data, sf.VALUE_DIMS, 1.0)
