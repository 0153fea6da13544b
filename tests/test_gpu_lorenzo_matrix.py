"""Lorenzo at every vector width, on thin and tiny shapes and over the radius range.

A. The reference-layout kernels k_lorenzo_c2d/c3d/x2d/x3d<T, V, ZZ> (lorenzo.hip DISPATCH_V) take
   V from the dtype and the parity of lx; every instantiation differs in its row loads, code loads
   and the shuffle path of hs_step.  Each is run by (at least) the case named here, plain and ZigZag,
   compress and reconstruct:

       instantiation          case (radius 512, LAYOUT_REFERENCE)
       3-D f32 V = 4          260 x 9 x 9
       3-D f32 V = 2          130 x 9 x 9, 66 x 17 x 9
       3-D f32 V = 1           65 x 9 x 9, 33 x 17 x 9
       3-D f64 V = 2          260 x 9 x 9, 130 x 9 x 9, 66 x 17 x 9
       3-D f64 V = 1           65 x 9 x 9, 33 x 17 x 9
       2-D f32 V = 4          260 x 33
       2-D f32 V = 2          130 x 33
       2-D f32 V = 1           65 x 33, 35 x 40, 45 x 37
       2-D f64 V = 2          260 x 33, 130 x 33
       2-D f64 V = 1           65 x 33, 35 x 40, 45 x 37

   (x crosses the x-brick of 64 V elements; y and z are ragged.)  Three kinds of field each: a delta
   field (delta_fields.py), a smooth one at a small eb (non-integer arithmetic), and the lattice
   flavours "order" and "near_ties" (edge_fields.py), which pin the scan order under rounding.
B. Thin and tiny shapes: extents of 1 on x or y, fields smaller than a wave's row, brick fields
   with ly == 1, forced 2-D bricks below a chunk row pair, fields of 1 to 3 elements; and
   psz_amd_value_range on 1 to 17 elements at an aligned and an element-aligned pointer.
C. Radii 1 .. 511: bklen = 2 radius in the histogram, the books and the decode tables, the byte-row
   base c0 = max(radius - 127, 0) of the brick path at its seam, FZG's transform, the codebook
   modes, the fused region decode and a scan / finish pair.
D. The device codebook at odd lengths against its restatement in the oracle.

Every Lorenzo case is run_roundtrip's contract (codes, outlier set, histogram, Huffman segment and
the reconstruction by all three decoders against the oracle, bit for bit) and asserts the layout it
took.  Delta-field cases are also held to the closed form, which does not involve the oracle: the
decoded codes, the archive's cells sorted by index, and the field decompressed by a manager made
from the header alone, as bits.

Measured on an MI355X when the module was added: 505 cases in 3.9 s, about 8 ms a case (the
largest field has 131,072 elements; a compress or decompress of these shapes takes 0.1 to 0.2 ms).
Two cases stand out against the 0.01 s of the slowest case of test_gpu_lattice.py in the same run:
the first case of the session (0.26 s: the runtime starts up), and
test_radius[256x13x11-float32-default-r1-zigzag] with 0.08 s in every run, also when it is run
nearly alone.  The library is not where that goes -- each of its calls on this field takes 0.15 ms,
the stage times show no repeat, and the test's own function called outside pytest takes 5 ms -- so
the shape stays as it is; what pytest does for 75 ms around this one case was not found.
"""
import numpy as np
import pytest
import torch

import cusz_amd as cz
import delta_fields as df
import edge_fields as ef
from cusz_amd import datagen
from gpu_util import d2h, parse_archive, sync, to_device
from test_gpu_book import device_book
from test_gpu_fzg import check_fzg_archive
from test_gpu_lattice import _decompress
from test_gpu_parity import run_roundtrip
from test_gpu_region import full_decompress, region
from test_gpu_sampled import sampled_roundtrip

pytestmark = pytest.mark.gpu

assert (df.BRICK, df.REF, df.FORCE) == (cz.LAYOUT_BRICK, cz.LAYOUT_REFERENCE, cz.LAYOUT_BRICK_FORCE)
F32, F64 = np.float32, np.float64
BITS = {F32: np.uint32, F64: np.uint64}
DTYPES = pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
PREDICTORS = pytest.mark.parametrize("zz", [False, True], ids=["plain", "zigzag"])
LAYOUT_NAMES = {None: "default", cz.LAYOUT_REFERENCE: "reference", cz.LAYOUT_BRICK_FORCE: "forced"}


def _dims_id(d):
    return "x".join(map(str, d))


def _ctype(dtype):
    return cz.F4 if dtype == F32 else cz.F8


def compress_checked(data, dims, eb, dtype, zz, radius, layout, expect, closed=None, codebook=None):
    """One compress that asserts the layout it took and, for a delta field (closed = the expected
    codes, outlier indices and values), holds codes, cells and the decompressed field to the closed
    form -> the archive's bytes."""
    n = data.size
    r = cz.Resource(_ctype(dtype), dims, cz.LorenzoZigZag if zz else cz.Lorenzo)
    if layout is not None:
        r.set_layout(layout)
    if codebook is not None:
        r.set_codebook(codebook)
    d_in = to_device(data)
    ptr, nbytes, st = r.compress(d_in.data_ptr(), eb, cz.Abs, radius)
    assert st == cz.PSZ_SUCCESS
    ino = r.internals()
    assert ino.layout == expect, f"layout {ino.layout}, meant to take {expect}"
    assert ino.bklen == 2 * radius
    arch = d2h(ptr, nbytes).tobytes()
    if closed is not None:
        codes, idx, val = closed
        if ino.layout == cz.LAYOUT_BRICK:  # codes never reach HBM: decode them
            r.decode_codes(ptr)
            sync()
        codes_g = d2h(ino.d_quant_codes, 2 * n, np.uint16)
        bad = np.flatnonzero(codes_g != codes)
        assert bad.size == 0, f"{bad.size} codes differ from the closed form, first at {bad[:5]}: " \
                              f"{codes_g[bad[:5]]} vs {codes[bad[:5]]}"
        a = parse_archive(arch)
        assert a["bklen"] == 2 * radius and a["header"].splen == idx.size
        order = np.argsort(a["ol_idx"], kind="stable")
        np.testing.assert_array_equal(a["ol_idx"][order], idx)
        np.testing.assert_array_equal(a["ol_val"][order].view(np.uint32), val.view(np.uint32))
    r.close()
    if closed is not None:
        got = _decompress(arch, n, dtype)
        bad = np.flatnonzero(got.view(BITS[dtype]) != data.view(BITS[dtype]))
        assert bad.size == 0, f"{bad.size} values differ from the input, first at {bad[:5]}: {got[bad[:5]]} vs {data[bad[:5]]}"
    return arch


def delta_case(oracle, dims, radius, dtype, zz, layout, expect, codebook=None, planted=None):
    data, codes, idx, val = df.delta_field(dims, radius, dtype, zz, planted=planted)
    arch = compress_checked(data, dims, 0.5, dtype, zz, radius, layout, expect, (codes, idx, val), codebook)
    again, a = run_roundtrip(oracle, data, dims, 0.5, dtype, zz, radius, layout=layout, codebook=codebook)
    assert again == arch, "two managers, one field: the same archive"
    return arch, a


# ---- A. the instantiation matrix ------------------------------------------------------------------------
MATRIX = [(d, dt, zz) for d in df.MATRIX_3D + df.MATRIX_2D for dt in (F32, F64) for zz in (False, True)]
MATRIX_IDS = [f"{_dims_id(d)}-{np.dtype(dt).name}-{'zigzag' if zz else 'plain'}" for d, dt, zz in MATRIX]
_covered = {(3 if d[2] > 1 else 2, np.dtype(dt).name, df.vector_width(dt, d[0]), zz) for d, dt, zz in MATRIX}
_wanted = {(nd, t, v, zz) for nd in (2, 3) for t, v in (("float32", 4), ("float32", 2), ("float32", 1), ("float64", 2),
                                                        ("float64", 1)) for zz in (False, True)}
assert _covered == _wanted and len(_wanted) == 20, sorted(_wanted - _covered)


@pytest.mark.parametrize("dims,dtype,zz", MATRIX, ids=MATRIX_IDS)
def test_matrix_delta(oracle, dims, dtype, zz):
    delta_case(oracle, dims, 512, dtype, zz, cz.LAYOUT_REFERENCE, cz.LAYOUT_REFERENCE)


@pytest.mark.parametrize("dims,dtype,zz", MATRIX, ids=MATRIX_IDS)
def test_matrix_smooth(oracle, dims, dtype, zz):
    data = datagen.smooth3d_np(dims, sum(dims), dtype=dtype) if dims[2] > 1 else datagen.cesm2d_np(dims, sum(dims), dtype=dtype)
    eb = 1e-4 if dtype == F32 else 1e-5
    arch = compress_checked(data, dims, eb, dtype, zz, 512, cz.LAYOUT_REFERENCE, cz.LAYOUT_REFERENCE)
    again, _ = run_roundtrip(oracle, data, dims, eb, dtype, zz, layout=cz.LAYOUT_REFERENCE)
    assert again == arch


@PREDICTORS
@DTYPES
@pytest.mark.parametrize("flavour", ["order", "near_ties"])
@pytest.mark.parametrize("dims", df.MATRIX_LATTICE, ids=_dims_id)
def test_matrix_lattice(oracle, dims, flavour, dtype, zz):
    data = ef.lattice_field(dims, dtype, flavour)
    eb = ef.lattice_eb(flavour)
    arch = compress_checked(data, dims, eb, dtype, zz, 512, cz.LAYOUT_REFERENCE, cz.LAYOUT_REFERENCE)
    again, _ = run_roundtrip(oracle, data, dims, eb, dtype, zz, check_bound=flavour != "order", layout=cz.LAYOUT_REFERENCE)
    assert again == arch


# ---- B. thin and tiny shapes ------------------------------------------------------------------------------
@PREDICTORS
@DTYPES
@pytest.mark.parametrize("dims,layout,expect", df.THIN, ids=[f"{_dims_id(d)}-{LAYOUT_NAMES[l]}" for d, l, _ in df.THIN])
def test_thin(oracle, dims, layout, expect, dtype, zz):
    delta_case(oracle, dims, 512, dtype, zz, layout, expect)


@PREDICTORS
@DTYPES
@pytest.mark.parametrize("layout,expect", [(None, cz.LAYOUT_BRICK), (cz.LAYOUT_REFERENCE, cz.LAYOUT_REFERENCE)],
                         ids=["default", "reference"])
def test_one_element_that_is_an_outlier(oracle, layout, expect, dtype, zz):
    arch, a = delta_case(oracle, (1, 1, 1), 512, dtype, zz, layout, expect, planted={0: 3 * 512})
    assert a["header"].splen == 1 and a["ol_idx"].tolist() == [0]


VR_LENGTHS = (1, 2, 3, 4, 5, 7, 8, 15, 16, 17)


@DTYPES
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "one_element_in"])
def test_value_range_tiny(dtype, offset):
    """psz_amd_value_range (k_extrema_partial): 16-B groups when the pointer is 16-B aligned, element
    by element otherwise; the extrema on the first and the last element, values past both ends
    that would win if they were read.  Exact against numpy."""
    es = np.dtype(dtype).itemsize
    rng = np.random.default_rng(es + offset)
    r = cz.Resource(_ctype(dtype), (32, 1, 1))
    out = torch.zeros(2, dtype=torch.float64, device="cuda")
    for n in VR_LENGTHS:
        data = rng.uniform(-1, 1, n).astype(dtype)
        data[0], data[-1] = dtype(-3.5), dtype(7.25)
        if n == 1:
            data[0] = dtype(0.1)
        fence = np.array([-1e30, 1e30, -1e30], dtype)
        buf = to_device(np.concatenate((fence[:offset], data, fence[1:])))
        assert buf.data_ptr() % 16 == 0
        out.fill_(float("nan"))
        r.value_range(buf.data_ptr() + offset * es, out.data_ptr(), n)
        sync()
        got = out.cpu().numpy()
        assert got.tolist() == [float(data.min()), float(data.max())], (n, got)
    r.close()


# ---- C. the radius range ----------------------------------------------------------------------------------
RADIUS_CASES = [(d, dt, lay, exp, r) for d, dt, lay, exp, radii in df.RADIUS_SHAPES for r in radii]


@PREDICTORS
@pytest.mark.parametrize("dims,dtype,layout,expect,radius", RADIUS_CASES,
                         ids=[f"{_dims_id(d)}-{np.dtype(dt).name}-{LAYOUT_NAMES[l]}-r{r}" for d, dt, l, _, r in RADIUS_CASES])
def test_radius(oracle, dims, dtype, layout, expect, radius, zz):
    arch, a = delta_case(oracle, dims, radius, dtype, zz, layout, expect)
    assert a["header"].rc.radius == radius


@PREDICTORS
@pytest.mark.parametrize("radius", df.MODES_RADII)
@pytest.mark.parametrize("mode", [cz.CODEBOOK_EXACT, cz.CODEBOOK_SAMPLED, cz.CODEBOOK_STREAM], ids=["exact", "sampled", "stream"])
def test_radius_codebook_modes(oracle, mode, radius, zz):
    dims = df.MODES_DIMS
    if mode == cz.CODEBOOK_EXACT:
        delta_case(oracle, dims, radius, F32, zz, None, cz.LAYOUT_BRICK, codebook=mode)
        return
    data, codes, idx, val = df.delta_field(dims, radius, F32, zz)
    arch = compress_checked(data, dims, 0.5, F32, zz, radius, None, cz.LAYOUT_BRICK, (codes, idx, val), mode)
    assert sampled_roundtrip(oracle, data, dims, F32, 0.5, zz, radius, mode) == arch


@pytest.mark.parametrize("radius", df.REGION_RADII)
def test_radius_fused_region(radius):
    dims, o, e = df.MODES_DIMS, (250, 7, 7), (13, 9, 2)
    data, _, _, _ = df.delta_field(dims, radius, F32, False)
    r = cz.Resource(cz.F4, dims)
    ptr, nb, _ = r.compress(to_device(data).data_ptr(), 0.5, cz.Abs, radius)
    assert r.internals().layout == cz.LAYOUT_BRICK
    d_arch = to_device(d2h(ptr, nb).copy())
    full = full_decompress(r, d_arch, nb, data.size, F32)
    np.testing.assert_array_equal(full, data.view(np.uint32))
    got, guards = region(r, d_arch, nb, o, e, F32)
    want = full.reshape(dims[::-1])[o[2]:o[2] + e[2], o[1]:o[1] + e[1], o[0]:o[0] + e[0]].reshape(-1)
    np.testing.assert_array_equal(got, want)
    assert guards, "written outside the box"
    assert r.last_region().path == cz.REGION_FUSED
    r.close()


@PREDICTORS
@pytest.mark.parametrize("radius", df.FZG_RADII)
@pytest.mark.parametrize("dims", df.FZG_SHAPES, ids=_dims_id)
def test_radius_fzg(oracle, dims, radius, zz):
    data, codes, idx, val = df.delta_field(dims, radius, F32, zz)
    n = data.size
    r = cz.Resource(cz.F4, dims, cz.LorenzoZigZag if zz else cz.Lorenzo, codec=cz.FZCodec)
    ptr, nb, st = r.compress(to_device(data).data_ptr(), 0.5, cz.Abs, radius)
    assert st == cz.PSZ_SUCCESS
    ino = r.internals()
    assert ino.layout == cz.LAYOUT_REFERENCE
    arch = d2h(ptr, nb).tobytes()
    h, codes_o, xo = check_fzg_archive(oracle, arch, data, dims, F32, zz, radius)
    np.testing.assert_array_equal(codes_o, codes)
    np.testing.assert_array_equal(d2h(ino.d_quant_codes, 2 * n, np.uint16), codes)
    cells = np.frombuffer(arch[h.entry[3]:h.entry[4]], np.uint32).reshape(-1, 2)
    order = np.argsort(cells[:, 1], kind="stable")
    np.testing.assert_array_equal(cells[order, 1], idx)
    np.testing.assert_array_equal(cells[order, 0], val.view(np.uint32))
    r.close()
    got = _decompress(arch, n, F32)
    np.testing.assert_array_equal(got.view(np.uint32), data.view(np.uint32))
    np.testing.assert_array_equal(xo.view(np.uint32), data.view(np.uint32))


def test_radius_scan_then_finish(oracle):
    """compress_scan, then compress_finish with the histogram the scan exported (test_gpu_shard.py):
    the device book of the full histogram at bklen 258."""
    dims, radius = df.SCAN_DIMS, df.SCAN_RADIUS
    data, codes, idx, val = df.delta_field(dims, radius, F32, False)
    r = cz.Resource(cz.F4, dims)
    d_in = to_device(data)
    hist = torch.zeros(2 * radius + 1, dtype=torch.int32, device="cuda")
    r.compress_scan(d_in.data_ptr(), 0.5, hist.data_ptr(), radius=radius)
    ptr, nb, _ = r.compress_finish(hist.data_ptr())
    assert r.internals().layout == cz.LAYOUT_BRICK
    arch = d2h(ptr, nb).tobytes()
    r.close()
    h = hist.cpu().numpy().view(np.uint32)
    want = np.bincount(codes, minlength=2 * radius).astype(np.uint32)
    np.testing.assert_array_equal(h[:2 * radius], want)
    assert h[2 * radius] == 0, "no outlier overflow"
    np.testing.assert_array_equal(want, oracle.histogram(codes, 2 * radius))
    _, rv = oracle.book_twoqueue(want, 2 * radius, smooth=0)
    a = parse_archive(arch)
    np.testing.assert_array_equal(a["revbook"], rv)
    order = np.argsort(a["ol_idx"], kind="stable")
    np.testing.assert_array_equal(a["ol_idx"][order], idx)
    np.testing.assert_array_equal(a["ol_val"][order].view(np.uint32), val.view(np.uint32))
    xo = oracle.lorenzo_x(codes, val, idx, dims, 0.5, radius, False, F32)
    got = _decompress(arch, data.size, F32)
    np.testing.assert_array_equal(got.view(np.uint32), xo.view(np.uint32))
    np.testing.assert_array_equal(got.view(np.uint32), data.view(np.uint32))


# ---- D. the device codebook at odd lengths ----------------------------------------------------------------
@pytest.mark.parametrize("smooth", [0, 1])
@pytest.mark.parametrize("bklen", df.BOOK_BKLENS)
def test_device_book_odd_lengths(oracle, bklen, smooth):
    rng = np.random.default_rng(bklen)
    _, codes, _, _ = df.delta_field(df.BOOK_DIMS, bklen // 2, F32, False)
    single = np.zeros(bklen, np.uint32)
    single[bklen // 3] = 54321
    hists = {"delta": np.bincount(codes, minlength=bklen), "uniform": rng.integers(0, 1000, bklen),
             "ties": np.full(bklen, 7), "single": single}
    for name, h in hists.items():
        h = np.asarray(h, np.uint32)
        assert h.size == bklen
        b_d, r_d = device_book(h, bklen, smooth)
        b_o, r_o = oracle.book_twoqueue(h, bklen, smooth)
        np.testing.assert_array_equal(b_d, b_o, err_msg=f"{name} bklen={bklen} smooth={smooth}: book")
        np.testing.assert_array_equal(r_d, r_o, err_msg=f"{name} bklen={bklen} smooth={smooth}: revbook")
