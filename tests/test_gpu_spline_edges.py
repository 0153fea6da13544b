"""The spline3 path at its edges on the GPU: tile and grid shapes, outlier loads past a tile's slot,
the spill list and the prefetched entries, cells on the +1 faces, the quantiser's edges, value
kinds, modes and decoders -- every case through gpu_util.spline_roundtrip (codes, anchors, cells in
order, histogram, Huffman segment and the decompressed field, bit for bit against the CPU oracle) --
and the code range: a field whose codes an outlier cell cannot carry is refused by status
(PSZ_AMD_ERR_CODE_RANGE) exactly when the oracle counts such a code.

spline_fields.py builds the fields; test_spline_fields.py proves on the oracle that each hits the
edge it is meant to, and that the oracle's own round trip holds the error bound for every field
accepted here (the GPU result is the oracle's, bit for bit).
"""
import ctypes as C

import numpy as np
import pytest

import cusz_amd as cz
import spline_fields as sf
from gpu_util import d2h, empty_device, parse_archive, sync, to_device
from gpu_util import spline_roundtrip as _roundtrip

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
dt_ids = ["f32", "f64"]
name = lambda d: "x".join(map(str, d)) if isinstance(d, tuple) else getattr(d, "__name__", str(d))  # noqa: E731


def _resource(dtype, dims):
    return cz.Resource(cz.F4 if dtype == np.float32 else cz.F8, dims, cz.Spline)


# ---- shapes and grids -------------------------------------------------------------------------------
SHAPE_CASES = [(dims, dt) for dims, only in sf.SHAPES for dt in DTYPES if only in (None, dt)]


@pytest.mark.parametrize("dims,dtype", SHAPE_CASES, ids=[f"{name(d)}-{name(t)}" for d, t in SHAPE_CASES])
def test_shapes(oracle, dims, dtype):
    """Below a tile in some axis, exact tile multiples, last tiles one point thick, X or Y of 1."""
    _roundtrip(oracle, dims, dtype, sf.SMOOTH_EB)


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_ids)
@pytest.mark.parametrize("tiles", list(sf.GRIDS))
def test_small_grids(oracle, tiles, dtype):
    """Fewer tiles than any grid: TileOrder's per-XCD ranges from 8 tiles up, the strided walk below
    and for grids that are no multiple of 8."""
    _roundtrip(oracle, sf.GRIDS[tiles], dtype, sf.SMOOTH_EB)


@pytest.fixture(scope="module")
def big_dims():
    import torch

    dims = sf.big_dims(torch.cuda.get_device_properties(0).multi_processor_count)
    assert sf.ntiles(dims) > 8 * torch.cuda.get_device_properties(0).multi_processor_count
    return dims


def test_more_tiles_than_the_grid(oracle, big_dims):
    """Every workgroup walks more than one tile, the per-XCD ranges are ragged (ntiles % 8 != 0),
    the finalize scan and the bucket bounds cross 1024 tiles: all codes and cells, not two slabs."""
    assert sf.ntiles(big_dims) % 8 and sf.ntiles(big_dims) > sf.SCAN_CHUNK
    _, _, _, nol = _roundtrip(oracle, big_dims, np.float64, sf.SMOOTH_EB)
    assert nol > 10 * sf.ntiles(big_dims)


# ---- outlier paths ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_ids)
@pytest.mark.parametrize("kind", ["centre", "three", "all"])
def test_outlier_loads(oracle, kind, dtype):
    """One ranged spill, three racing reservations, the spill list's overflow and regrowth (with
    more than 768 entries per tile group): the archive is the oracle's, a repeat on the manager
    gives the same bytes, and the manager afterwards compresses a smooth field as a fresh one does."""
    dims, eb = sf.NOISE_DIMS, sf.NOISE_EB
    data = sf.noise_field(kind, dtype)
    r = _resource(dtype, dims)
    first, again, after, fresh = {}, {}, {}, {}
    _roundtrip(oracle, dims, dtype, eb, data=data, resource=r, keep=first)
    d_in = to_device(data)
    ptr, nbytes, st = r.compress(d_in.data_ptr(), eb)
    assert st == cz.PSZ_SUCCESS and d2h(ptr, nbytes).tobytes() == first["archive"]
    _roundtrip(oracle, dims, dtype, eb, data=data, resource=r, keep=again)  # and decompresses again
    assert again["archive"] == first["archive"]
    _roundtrip(oracle, dims, dtype, eb, resource=r, keep=after)
    r.close()
    _roundtrip(oracle, dims, dtype, eb, keep=fresh)
    assert after["archive"] == fresh["archive"]


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_ids)
def test_face_cells(oracle, dtype):
    """Cells of an upper neighbour on a tile's +1 faces (lx == 32, ly == 8, lz == 8, edges), around
    an inner tile and the last one: the lower tile's reconstruction is the oracle's."""
    data, x, ebx, nol = _roundtrip(oracle, sf.FACE_DIMS, dtype, sf.FACE_EB, data=sf.face_field(dtype))
    assert nol >= len(sf.FACE_SPIKES)
    f, g = data.reshape(sf.FACE_DIMS[::-1]), x.reshape(sf.FACE_DIMS[::-1])
    for px, py, pz in sf.FACE_SPIKES:  # the spike and the points before it, in the lower tiles
        for q in ((px, py, pz), (px - 1, py, pz), (px, py - 1, pz), (px, py, pz - 1)):
            assert abs(float(g[q[2], q[1], q[0]]) - float(f[q[2], q[1], q[0]])) <= ebx, q


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_ids)
@pytest.mark.parametrize("xy", sf.DIV_XY, ids=[name(p) for p in sf.DIV_XY])
def test_index_division(oracle, xy, dtype):
    """k_spline3_x splits a cell's index by multiply-high: cells in every row and column of
    X x Y x 3 fields with X, Y at powers of two, their neighbours, 2 and 3."""
    dims = (*xy, 3)
    _roundtrip(oracle, dims, dtype, sf.NOISE_EB, data=sf.noise_on_tiles(dims, None, dtype))


@pytest.mark.parametrize("order", ["reversed_in_tile", "shuffled"])
def test_reordered_cells_on_many_tiles(oracle, big_dims, order):
    """Cells in another order decompress identically on more than 2048 tiles of which most hold
    no cell: the bucket scan carries across its 1024-tile passes, empty tiles get empty ranges."""
    import torch

    dims, dtype = big_dims, np.float32
    n = int(np.prod(dims))
    r = _resource(dtype, dims)
    keep = {}
    _, x0, _, nol = _roundtrip(oracle, dims, dtype, sf.SCATTER_EB, data=sf.scattered_noise(dims, dtype), resource=r,
                               keep=keep)
    arch = bytearray(keep["archive"])
    h = parse_archive(bytes(arch))["header"]
    cells = np.frombuffer(bytes(arch[h.entry[3]:h.entry[4]]), np.uint64).copy()
    assert cells.size == nol > 10000
    gid = (cells >> np.uint64(32)).astype(np.int64)
    tile = sf.tile_of(gid, dims)
    assert np.count_nonzero(np.bincount(tile, minlength=sf.ntiles(dims))) < sf.ntiles(dims) // 4
    if order == "shuffled":
        cells = cells[np.random.default_rng(1).permutation(cells.size)]
    else:
        cells = cells[np.lexsort((-gid, tile))]  # tile order kept, descending inside a tile
    arch[h.entry[3]:h.entry[4]] = cells.tobytes()
    d_arch = torch.tensor(np.frombuffer(bytes(arch), np.uint8)).cuda()
    out = empty_device(n, torch.float32)
    out.fill_(float("nan"))
    r.decompress(d_arch.data_ptr(), len(arch), out.data_ptr())
    sync()
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), x0.view(np.uint32))
    r.close()


# ---- quantiser edges, values, modes -----------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_ids)
@pytest.mark.parametrize("radius", [512, 256, 64])
def test_quantiser_edges(oracle, radius, dtype):
    """Kept and dropped codes of -1, 0, 1, 2r - 1, 2r, 2r + 1 (a kept 0 has the outlier placeholder's
    value), ties of the truncation and their neighbours, at a point of each of the nine stages."""
    data, spikes = sf.quant_field(radius, dtype)
    _, _, _, nol = _roundtrip(oracle, sf.QUANT_DIMS, dtype, sf.QUANT_EB, data=data, radius=radius)
    assert nol >= len(spikes) // 3


VALUE_CASES = [(k, dt) for k in ("constant", "mean1e6", "zeros") for dt in DTYPES] + [("pow23", np.float32)]


@pytest.mark.parametrize("kind,dtype", VALUE_CASES, ids=[f"{k}-{name(t)}" for k, t in VALUE_CASES])
def test_value_kinds(oracle, kind, dtype):
    """A constant, a large mean (a read of the zero padding would show as outliers), -0.0 and
    denormals, f32 integers around 2^23, on a field ragged in every axis."""
    data, eb = sf.value_field(kind, dtype)
    _, _, _, nol = _roundtrip(oracle, sf.VALUE_DIMS, dtype, eb, data=data)
    assert nol == 0


def test_rel_mode_f32(oracle):
    data, x, ebx, _ = _roundtrip(oracle, (96, 40, 24), np.float32, 1e-4, mode=cz.Rel)
    assert ebx == pytest.approx(1e-4 * (float(data.max()) - float(data.min())), rel=1e-9)
    assert np.max(np.abs(x.astype(np.float64) - data)) <= 1.005 * ebx


def test_lane_and_wave_decoders(oracle):
    """Every Huffman decoder on a spline archive (ragged, outlier-bearing)."""
    _, _, _, nol = _roundtrip(oracle, (70, 19, 13), np.float32, sf.SMOOTH_EB,
                              decoders=(cz.DECODER_AUTO, cz.DECODER_LANE, cz.DECODER_WAVE))
    assert nol > 100


# ---- the code range -----------------------------------------------------------------------------------
def _compress_raw(r, d_in, eb):
    """psz_compress_* -> (status, archive pointer or None)."""
    out, nbytes = C.c_void_p(), C.c_size_t()
    f = cz.lib().psz_compress_float if r.dtype == cz.F4 else cz.lib().psz_compress_double
    st = f(r._h, cz.psz_rc2(cz.Abs, eb, 512), C.c_void_p(d_in.data_ptr()), C.byref(r.header), C.byref(out),
           C.byref(nbytes))
    return st, out.value


def _scan_finish_raw(r, d_in, eb):
    """psz_amd_compress_scan_* + psz_amd_compress_finish -> (status, archive pointer or None)."""
    import torch

    d_hist = torch.zeros(1025, dtype=torch.int32, device="cuda")
    r.compress_scan(d_in.data_ptr(), eb, d_hist.data_ptr())
    out, nbytes = C.c_void_p(), C.c_size_t()
    st = cz.lib().psz_amd_compress_finish(r._h, None, C.byref(r.header), C.byref(out), C.byref(nbytes))
    return st, out.value


def _refused_iff_lost(oracle, data, dims, eb, dtype):
    """Both entry points refuse the field exactly when the oracle counts a lost code; a refusal
    hands back no pointer and leaves the manager usable."""
    lost = oracle.spline3_c(data, dims, eb, count_lost=True)[4]
    r = _resource(dtype, dims)
    d_in = to_device(data)
    for call in (_compress_raw, _scan_finish_raw):
        st, ptr = call(r, d_in, eb)
        if lost:
            assert st == cz.PSZ_AMD_ERR_CODE_RANGE and ptr is None, (call.__name__, st, ptr)
        else:
            assert st == cz.PSZ_SUCCESS and ptr, (call.__name__, st)
    after, fresh = {}, {}
    _roundtrip(oracle, dims, dtype, 1e-3, resource=r, keep=after)
    r.close()
    _roundtrip(oracle, dims, dtype, 1e-3, keep=fresh)
    assert after["archive"] == fresh["archive"]
    return lost


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_ids)
@pytest.mark.parametrize("height,ok32,ok64", sf.RANGE_SPIKES, ids=[str(h) for h, _, _ in sf.RANGE_SPIKES])
def test_code_range_spikes(oracle, height, ok32, ok64, dtype):
    """One spike of code height + 512 on zeros, on both sides of 2^24 (the ints a cell's float
    holds: f64 only) and of the int limit (both dtypes), both signs.  Accepted ones are bit-exact."""
    data = sf.range_spike(height, dtype)
    lost = _refused_iff_lost(oracle, data, sf.RANGE_DIMS, 0.5, dtype)
    assert (lost == 0) == (ok32 if dtype == np.float32 else ok64)
    if not lost:
        _, x, _, _ = _roundtrip(oracle, sf.RANGE_DIMS, dtype, 0.5, data=data)
        err = np.max(np.abs(x.astype(np.float64) - data))
        assert err <= max(0.5, float(np.spacing(dtype(abs(height)))))  # eb, or one ulp of the value in f32


@pytest.mark.parametrize("eb", [1e-5, 1e-6])
def test_code_range_noise_is_refused(oracle, eb):
    """standard_normal * 1e3 in f64: codes of 3e8 (error 44 eb if accepted) and beyond int."""
    assert _refused_iff_lost(oracle, sf.range_noise(), sf.VALUE_DIMS, eb, np.float64) > 0


def test_code_range_noise_in_domain(oracle):
    """The same field at a bound that keeps its codes in the domain, and in f32 where codes past
    2^24 are consistent on both sides."""
    assert _refused_iff_lost(oracle, sf.range_noise(), sf.VALUE_DIMS, 1.0, np.float64) == 0
    _roundtrip(oracle, sf.VALUE_DIMS, np.float64, 1.0, data=sf.range_noise())
    data = sf.range_noise(np.float32)
    assert _refused_iff_lost(oracle, data, sf.VALUE_DIMS, 1e-5, np.float32) == 0
    _, _, _, nol = _roundtrip(oracle, sf.VALUE_DIMS, np.float32, 1e-5, data=data)
    assert nol > data.size // 2
