"""Region decode in PSZ_AMD_REGION_MODE_COVER: a 1-D brick-layout archive decodes only the tiles of
1024 that cover the range, in one fused kernel (path FUSED, k_brick1_region); every other Lorenzo
archive off the fused 3-D path decodes only the tile-aligned slab of its slowest axis that covers
the box (path SLAB).  Every box equals, bit for
bit, the same box of psz_decompress_* of that archive by a default manager (whose parity with the
oracle other tests pin); nothing around the box is written; `chunks` is the closed-form count of
include/cusz_amd.h, written out again here; and the manager's code buffer shows that nothing outside
those chunks was decoded.

The fused 1-D launch gives every wave at most one unit of 64 tiles (launch_brick1_region sizes the
grid by the units), so there is no grid-stride round to test.

As in test_gpu_region.py the output box sits between two poisoned 4 KiB guard bands.
"""
import functools
import subprocess

import numpy as np
import pytest

import cusz_amd as cz
from cusz_amd import datagen
from gpu_util import H2D, d2h, hip, parse_archive, sync, to_device

pytestmark = pytest.mark.gpu

GUARD = 4096
POISON = {np.float32: np.uint32(0x7FC0DEAD), np.float64: np.uint64(0x7FF8DEADBEEF0BAD)}
BITS = {np.float32: np.uint32, np.float64: np.uint64}
SENTINEL = np.uint16(0xABCD)  # no quant code: codes are below 2 radius <= 1024
WHOLE, COVER = cz.REGION_MODE_WHOLE, cz.REGION_MODE_COVER
N1 = 200_003  # 1-D: 195 tiles of 1024 and one of 323; three units of 64 tiles and a fourth, ragged one; a short last chunk


def ndim(dims):
    return 3 if dims[2] != 1 else 2 if dims[1] != 1 else 1


def slab(dims, o, e):
    """(a P, b P): the code range of the covering slab (include/cusz_amd.h, PSZ_AMD_REGION_SLAB)"""
    nd = ndim(dims)
    T = {1: 1024, 2: 32, 3: 8}[nd]
    P = int(np.prod(dims[:nd - 1]))
    a = o[nd - 1] // T * T
    b = min(dims[nd - 1], -(-(o[nd - 1] + e[nd - 1]) // T) * T)
    return a * P, b * P


def chunk_range(dims, o, e, sublen, pardeg):
    lo, hi = slab(dims, o, e)
    return lo // sublen, min(pardeg, -(-hi // sublen))


def field_1d(dtype, spikes=True):
    """Small and smooth: no outlier at a tile's first element, so cells lie only where they are planted."""
    i = np.arange(N1, dtype=np.float64)
    d = (0.02 * np.sin(i * 1e-3) + 0.005 * np.cos(i * 0.017)).astype(dtype)
    if spikes:
        d[1030:1054:2] += dtype(3)      # 12 spikes in chunk 4 (tile 1, before the box that starts in phase 3)
        d[1930:1966:3] += dtype(3)      # 12 in chunk 7 (inside that box)
        d[[3120, 65_530, 70_001, 199_700, N1 - 1]] += dtype(3)
    return d                             # (tile 0 and tile 2 hold no cell)


def field_nd(dims, dtype, spikes=()):
    d = datagen.smooth3d_np(dims, sum(dims), dtype=dtype).reshape(-1).copy()
    for s in spikes:
        d[s] += dtype(3)
    return d


class Archive:
    """One field compressed once and decompressed once in full (by the compressing manager, in its
    default mode): the reference for every box."""

    def __init__(self, dims, dtype, data, eb=1e-4, radius=512, pred=cz.Lorenzo, codec=cz.Huffman, layout=None,
                 sublen=None):
        self.dims, self.dtype = dims, dtype
        self.n = int(np.prod(dims))
        self.ctype = cz.F4 if dtype == np.float32 else cz.F8
        self.r = cz.Resource(self.ctype, dims, pred, codec=codec)
        if layout is not None:
            self.r.set_layout(layout)
        if sublen is not None:
            self.r.set_sublen(sublen)
        ptr, self.nbytes, _ = self.r.compress(to_device(data).data_ptr(), eb, cz.Abs, radius)
        self.bytes = d2h(ptr, self.nbytes).tobytes()
        self.d_arch = to_device(np.frombuffer(self.bytes, np.uint8).copy())
        self.header = cz.psz_header.from_buffer_copy(self.bytes[:176])
        self.unit = 4096 if codec == cz.FZCodec else self.header.vle_sublen
        out = to_device(np.full(self.n, POISON[dtype]).view(dtype))
        self.r.decompress(self.d_arch.data_ptr(), self.nbytes, out.data_ptr())
        sync()
        self.full = d2h(out.data_ptr(), self.n * np.dtype(dtype).itemsize, BITS[dtype]).reshape(dims[::-1])

    def box(self, o, e):
        return np.ascontiguousarray(self.full[o[2]:o[2] + e[2], o[1]:o[1] + e[1], o[0]:o[0] + e[0]]).reshape(-1)

    def manager(self, mode=COVER, decoder=None):
        r = cz.Resource(self.ctype, None, header=self.header)
        r.set_region_mode(mode)
        if decoder is not None:
            r.set_decoder(decoder)
        return r

    def cells(self):
        return parse_archive(self.bytes, 2 * self.header.rc.radius)["ol_idx"].astype(np.int64)


def region(r, a, o, e, d_arch=None):
    """Region decode into a poisoned, guarded buffer -> (box bits, guards intact)."""
    es = np.dtype(a.dtype).itemsize
    g, nb = GUARD // es, int(np.prod(e))
    buf = to_device(np.full(2 * g + nb, POISON[a.dtype]).view(a.dtype))
    r.decompress_region((d_arch if d_arch is not None else a.d_arch).data_ptr(), a.nbytes, o, e, buf.data_ptr() + GUARD)
    sync()
    bits = d2h(buf.data_ptr(), (2 * g + nb) * es, BITS[a.dtype])
    return bits[g:g + nb], bool(np.all(bits[:g] == POISON[a.dtype]) and np.all(bits[g + nb:] == POISON[a.dtype]))


def check_slab(r, a, o, e, d_arch=None, bounded=False):
    """One box on manager r: bits, guards, path SLAB, chunks; bounded: the code buffer outside the
    covering chunks keeps a sentinel written beforehand, and the codes inside it are decoded."""
    o, e = (tuple(o) + (0, 0, 0))[:3], (tuple(e) + (1, 1, 1))[:3]
    c0, c1 = chunk_range(a.dims, o, e, a.unit, a.header.vle_pardeg)
    if bounded:
        d_codes = r.internals().d_quant_codes
        fill = np.full(a.n, SENTINEL)
        assert hip().hipMemcpy(d_codes, fill.ctypes.data, 2 * a.n, H2D) == 0
    got, guards = region(r, a, o, e, d_arch)
    np.testing.assert_array_equal(got, a.box(o, e))
    assert guards, "written outside the box"
    info = r.last_region()
    assert info.path == cz.REGION_SLAB and info.bricks == 0 and info.elems == int(np.prod(e))
    assert (info.brick_lo.x, info.brick_lo.y, info.brick_lo.z, info.brick_n.x, info.brick_n.y, info.brick_n.z) == (0,) * 6
    assert info.chunks == c1 - c0
    lo, hi = slab(a.dims, o, e)
    if lo >= a.unit or a.n - hi >= a.unit:  # a whole chunk lies before or after the slab: not everything is decoded
        assert info.chunks < a.header.vle_pardeg
    if bounded:
        codes = d2h(d_codes, 2 * a.n, np.uint16)
        lo, hi = c0 * a.unit, min(a.n, c1 * a.unit)
        assert np.all(codes[:lo] == SENTINEL) and np.all(codes[hi:] == SENTINEL), "decoded outside the covering chunks"
        assert np.all(codes[lo:hi] < 2 * a.header.rc.radius)
    return info


def check_fused1(r, a, o, e, d_arch=None):
    """One range of a 1-D archive on manager r: bits, guards, path FUSED, tiles and chunks."""
    got, guards = region(r, a, (o, 0, 0), (e, 1, 1), d_arch)
    np.testing.assert_array_equal(got, a.box((o, 0, 0), (e, 1, 1)))
    assert guards, "written outside the box"
    info = r.last_region()
    t0, t1 = o // 1024, -(-(o + e) // 1024)
    assert info.path == cz.REGION_FUSED and info.elems == e
    assert (info.brick_lo.x, info.brick_lo.y, info.brick_lo.z, info.brick_n.x, info.brick_n.y, info.brick_n.z) == (t0, 0, 0, t1 - t0, 1, 1)
    assert info.bricks == t1 - t0 and info.chunks == min(4 * t1, a.header.vle_pardeg) - 4 * t0
    if t1 - t0 < -(-a.n // 1024):
        assert info.chunks < a.header.vle_pardeg
    return info


# ---- 1-D ------------------------------------------------------------------------------------------
BOXES_1D = {
    "whole": (0, N1),
    "element": (70_001, 1),
    "in_chunk": (3_100, 50),
    "chunk_border": (1_200, 200),     # within a tile: the carry
    "phase3": (1_900, 300),           # starts in the tile's fourth chunk, ends in the next tile
    "tile_border": (1_000, 100),
    "unit_border": (65_500, 100),     # 64 tiles
    "to_end": (N1 - 777, 777),
    "last_tile": (199_700, 100),      # inside the partial tile
    "no_cells": (2_100, 900),         # tile 2
}


@functools.lru_cache(maxsize=None)
def arch_1d(dtype, spikes=True, pred=cz.Lorenzo, layout=None, sublen=None):
    return Archive((N1, 1, 1), dtype, field_1d(dtype, spikes), pred=pred, layout=layout, sublen=sublen)


def test_1d_field_is_what_the_boxes_assume():
    a = arch_1d(np.float32)
    assert a.header.vle_sublen == 256 and a.header.vle_pardeg == (N1 + 255) // 256
    idx = a.cells()
    per_chunk = np.bincount(idx // 256, minlength=a.header.vle_pardeg)
    assert per_chunk[4] >= 12 and per_chunk[7] >= 12          # before / inside the "phase3" box, tile 1
    assert not np.any((idx >= 0) & (idx < 1024)) and not np.any((idx >= 2048) & (idx < 3072))  # tiles without cells
    assert np.any(idx >= N1 - 323)                            # a cell in the last, partial tile
    assert np.all(np.diff(idx) > 0)                           # in index order, as written
    assert arch_1d(np.float32, spikes=False).header.splen == 0


@pytest.mark.parametrize("box", list(BOXES_1D))
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_1d_boxes(dtype, box):
    a = arch_1d(dtype)
    o, e = BOXES_1D[box]
    check_fused1(a.manager(), a, o, e)


def test_1d_ranges_one_after_another_on_one_manager():
    a = arch_1d(np.float32)
    r = a.manager()
    for box in ("phase3", "whole", "element", "phase3", "last_tile"):
        check_fused1(r, a, *BOXES_1D[box])
    for o, e in [(1024, 1024), (1023, 1), (1024, 1), (2047, 2), (65_535, 2), (0, 1), (N1 - 1, 1), (199_679, 2)]:
        check_fused1(r, a, o, e)  # tile, chunk and unit borders, element by element


def test_1d_without_outliers():
    a = arch_1d(np.float32, spikes=False)
    r = a.manager()  # (no cells: the call reads nothing back)
    for o, e in (BOXES_1D["phase3"], BOXES_1D["unit_border"], BOXES_1D["to_end"], BOXES_1D["whole"]):
        check_fused1(r, a, o, e)


@pytest.mark.parametrize("variant", ["zigzag", "lane", "wave", "reversed_cells", "reference_layout", "sublen512"])
def test_1d_demotions_to_the_slab(variant):
    """What the fused 1-D kernel does not take: ZigZag and another chunk length by the header, a
    forced decoder and cells out of index order by the manager's checks."""
    kw = dict(zigzag=dict(pred=cz.LorenzoZigZag), reference_layout=dict(layout=cz.LAYOUT_REFERENCE), sublen512=dict(sublen=512))
    a = arch_1d(np.float32, **kw.get(variant, {}))
    if variant == "sublen512":
        assert a.header.vle_sublen == 512
    r = a.manager(decoder=dict(lane=cz.DECODER_LANE, wave=cz.DECODER_WAVE).get(variant))
    d_arch = None
    if variant == "reversed_cells":
        raw = np.frombuffer(a.bytes, np.uint8).copy()
        cells = raw[a.header.entry[3]:a.header.entry[4]].view(np.uint32).reshape(-1, 2)
        assert len(cells) > 1
        cells[:] = cells[::-1].copy()
        d_arch = to_device(raw)
    o, e = BOXES_1D["phase3"]
    plan = cz.region_plan(a.header, (o,), (e,), COVER).path
    assert plan == (cz.REGION_SLAB if variant in ("zigzag", "sublen512") else cz.REGION_FUSED) or variant == "reference_layout"
    if variant == "reference_layout" and plan == cz.REGION_FUSED and np.all(np.diff(a.cells()) > 0):
        # chunks of 256 and cells in index order: the header and the cells are a brick archive's
        for box in ("phase3", "unit_border", "last_tile", "element"):
            check_fused1(r, a, *BOXES_1D[box])
        return
    for box in ("phase3", "unit_border", "last_tile", "element"):
        o, e = BOXES_1D[box]
        check_slab(r, a, (o,), (e,), d_arch=d_arch, bounded=box == "phase3")
    if variant == "reversed_cells":  # the same manager then takes the fused path for the archive as written
        check_fused1(r, a, *BOXES_1D["phase3"])


# ---- 2-D ------------------------------------------------------------------------------------------
# rows 32..63 of 300 x 70 are codes [9600, 19200): a spike on either side of both faces of that slab
FACES = (9_599, 9_600, 19_199, 19_200)
FIELDS_2D = {
    "300x70": dict(dims=(300, 70, 1), dtype=np.float32, spikes=FACES, sublen=256),       # V = 4
    "300x70-s2048": dict(dims=(300, 70, 1), dtype=np.float32, spikes=FACES, sublen=2048),
    "300x70-s8192": dict(dims=(300, 70, 1), dtype=np.float32, spikes=FACES, sublen=8192),
    "301x70": dict(dims=(301, 70, 1), dtype=np.float32, sublen=256),                     # V = 1
    "302x40-f64": dict(dims=(302, 40, 1), dtype=np.float64, sublen=256),                 # V = 2
    "512x70-bricks": dict(dims=(512, 70, 1), dtype=np.float32, layout=cz.LAYOUT_BRICK_FORCE),
}


def boxes_2d(lx, ly):
    return {
        "in_slab": ((17, 5), (lx - 50, 20)),
        "across_32": ((10, 20), (100, 15)),
        "to_last_row": ((0, ly - 7), (lx, 7)),
        "row": ((0, 33), (lx, 1)),
        "element": ((lx - 1, ly - 1), (1, 1)),
        "second_slab": ((5, 33), (7, 3)),
    }


@functools.lru_cache(maxsize=None)
def arch_nd(name):
    f = dict({**FIELDS_2D, **FIELDS_3D, **FIELDS_FZG}[name])
    dims, dtype = f.pop("dims"), f.pop("dtype")
    return Archive(dims, dtype, field_nd(dims, dtype, f.pop("spikes", ())), **f)


@pytest.mark.parametrize("name", list(FIELDS_2D))
def test_2d_boxes(name):
    a = arch_nd(name)
    want = FIELDS_2D[name].get("sublen")
    assert want is None or a.header.vle_sublen == want
    r = a.manager()
    for box, (o, e) in boxes_2d(*a.dims[:2]).items():
        check_slab(r, a, o, e, bounded=box in ("across_32", "second_slab", "to_last_row"))


def test_outliers_at_the_faces_of_the_slab():
    a = arch_nd("300x70")
    assert set(FACES) <= set(a.cells().tolist())
    check_slab(a.manager(), a, (0, 32), (300, 32), bounded=True)   # the slab itself: two of the four are inside
    check_slab(a.manager(), a, (299, 63), (1, 1))
    check_slab(a.manager(), a, (0, 0), (300, 32))                  # its neighbours: one each
    check_slab(a.manager(), a, (0, 64), (300, 6))


def test_a_tail_slab_one_step_thick():
    """len % T == 1: the last slab is one row (2-D) or one plane (3-D) and reconstructs with the
    field's own kernel."""
    a = Archive((300, 65, 1), np.float32, field_nd((300, 65, 1), np.float32, spikes=(19_200, 19_499)), sublen=256)
    r = a.manager()
    for o, e in [((0, 64), (300, 1)), ((299, 64), (1, 1)), ((0, 64), (1, 1)), ((5, 60), (20, 5))]:
        check_slab(r, a, o, e, bounded=True)
    a = Archive((64, 20, 9), np.float32, field_nd((64, 20, 9), np.float32, spikes=(64 * 20 * 8, 64 * 20 * 9 - 1)))
    r = a.manager()
    for o, e in [((0, 0, 8), (64, 20, 1)), ((63, 19, 8), (1, 1, 1)), ((3, 2, 5), (20, 10, 4))]:
        check_slab(r, a, o, e, bounded=True)
    a = Archive((96, 20, 9), np.float64, field_nd((96, 20, 9), np.float64), pred=cz.LorenzoZigZag, radius=64, eb=3e-4)
    check_slab(a.manager(), a, (0, 0, 8), (96, 20, 1), bounded=True)


# ---- 3-D ------------------------------------------------------------------------------------------
FIELDS_3D = {
    "96x64x40": dict(dims=(96, 64, 40), dtype=np.float32),
    "96x20x13": dict(dims=(96, 20, 13), dtype=np.float32),                               # ragged y and z
    "512x24x24-zz": dict(dims=(512, 24, 24), dtype=np.float32, eb=1e-3, pred=cz.LorenzoZigZag),
    "512x24x24": dict(dims=(512, 24, 24), dtype=np.float32, eb=1e-3),                    # a fused candidate
    "64x20x13-f64": dict(dims=(64, 20, 13), dtype=np.float64, eb=3e-4, radius=64),
}


def boxes_3d(lx, ly, lz):
    return {
        "across_plane_8": ((5, 7, 6), (lx - 16, 10, 5)),
        "in_slab": ((0, 0, 9), (lx, ly, 3)),
        "to_last_plane": ((3, 2, lz - 4), (20, 10, 4)),
        "element": ((lx - 1, ly - 1, lz - 1), (1, 1, 1)),
    }


@pytest.mark.parametrize("name", [n for n in FIELDS_3D if n != "512x24x24"])
def test_3d_boxes(name):
    a = arch_nd(name)
    r = a.manager()
    for box, (o, e) in boxes_3d(*a.dims).items():
        check_slab(r, a, o, e, bounded=box != "element")


def test_3d_fused_candidate_with_a_forced_decoder_takes_the_slab():
    a = arch_nd("512x24x24")
    o, e = boxes_3d(*a.dims)["across_plane_8"]
    assert cz.region_plan(a.header, o, e, COVER).path == cz.REGION_FUSED
    check_slab(a.manager(decoder=cz.DECODER_LANE), a, o, e, bounded=True)
    check_slab(a.manager(decoder=cz.DECODER_WAVE), a, *boxes_3d(*a.dims)["to_last_plane"])
    r = a.manager()  # the default decoder stays fused under COVER
    got, guards = region(r, a, o, e)
    np.testing.assert_array_equal(got, a.box(o, e))
    assert guards and r.last_region().path == cz.REGION_FUSED


# ---- FZG ------------------------------------------------------------------------------------------
FIELDS_FZG = {
    "fzg-1d": dict(dims=(50_000, 1, 1), dtype=np.float32, codec=cz.FZCodec),
    "fzg-3d": dict(dims=(96, 64, 40), dtype=np.float32, codec=cz.FZCodec, radius=64, eb=3e-4),
    "fzg-3d-zz-f64": dict(dims=(96, 20, 13), dtype=np.float64, codec=cz.FZCodec, pred=cz.LorenzoZigZag),
}


@pytest.mark.parametrize("name", list(FIELDS_FZG))
def test_fzg_boxes(name):
    a = arch_nd(name)
    r = a.manager()
    if name == "fzg-1d":
        assert check_slab(r, a, (5_000,), (50,), bounded=True).chunks == 1    # tile [4096, 5120): inside block 1
        assert check_slab(r, a, (8_000,), (400,), bounded=True).chunks == 2   # tiles [7168, 9216): blocks 1 and 2
        check_slab(r, a, (49_990,), (10,), bounded=True)                      # the last, short block
        check_slab(r, a, (0,), (50_000,))
    else:
        for box, (o, e) in boxes_3d(*a.dims).items():
            check_slab(r, a, o, e, bounded=box != "element")


# ---- what stays ------------------------------------------------------------------------------------
def test_spline_keeps_the_fallback():
    dims = (33, 9, 9)
    a = Archive(dims, np.float32, field_nd(dims, np.float32), eb=3e-6, pred=cz.Spline)
    r = a.manager()
    o, e = (3, 2, 1), (29, 6, 7)
    got, guards = region(r, a, o, e)
    np.testing.assert_array_equal(got, a.box(o, e))
    info = r.last_region()
    assert guards and info.path == cz.REGION_FALLBACK and info.chunks == a.header.vle_pardeg


def test_modes_alternate_on_one_manager():
    a = arch_nd("96x64x40")
    o, e = boxes_3d(*a.dims)["across_plane_8"]
    r = a.manager()
    first = check_slab(r, a, o, e)
    r.set_region_mode(WHOLE)
    got, guards = region(r, a, o, e)
    np.testing.assert_array_equal(got, a.box(o, e))
    info = r.last_region()
    assert guards and info.path == cz.REGION_FALLBACK and info.chunks == a.header.vle_pardeg and info.bricks == 0
    with pytest.raises(cz.PszError) as ei:
        r.set_region_mode(2)
    assert ei.value.status == cz.PSZ_AMD_ERR_INVALID_ARG
    got, _ = region(r, a, o, e)
    assert r.last_region().path == cz.REGION_FALLBACK  # the refused value left the mode alone
    r.set_region_mode(COVER)
    out = to_device(np.full(a.n, POISON[a.dtype]).view(a.dtype))
    r.decompress(a.d_arch.data_ptr(), a.nbytes, out.data_ptr())  # a full decompress in between
    sync()
    np.testing.assert_array_equal(d2h(out.data_ptr(), a.n * 4, np.uint32).reshape(a.full.shape), a.full)
    assert check_slab(r, a, o, e).chunks == first.chunks
    check_slab(r, a, o, e, bounded=True)  # and once more: the same bits


def test_a_default_manager_still_reports_the_fallback():
    a = arch_nd("300x70")
    r = a.manager(mode=WHOLE)
    got, guards = region(r, a, (5, 40, 0), (7, 3, 1))
    np.testing.assert_array_equal(got, a.box((5, 40, 0), (7, 3, 1)))
    assert guards and r.last_region().path == cz.REGION_FALLBACK
    a = arch_1d(np.float32)  # 1-D: fused under COVER, the fallback again once set back
    r = a.manager()
    check_fused1(r, a, *BOXES_1D["phase3"])
    r.set_region_mode(WHOLE)
    got, guards = region(r, a, (1_900, 0, 0), (300, 1, 1))
    np.testing.assert_array_equal(got, a.box((1_900, 0, 0), (300, 1, 1)))
    info = r.last_region()
    assert guards and info.path == cz.REGION_FALLBACK and info.bricks == 0 and info.chunks == a.header.vle_pardeg


@pytest.mark.parametrize("name,o,e", [("1d", (1_900,), (300,)), ("300x70", (10, 20), (100, 15))])
def test_cli_region_mode(tmp_path, name, o, e):
    a = arch_1d(np.float32) if name == "1d" else arch_nd(name)
    f = tmp_path / "field.f32.cusza"
    f.write_bytes(a.bytes)
    o3, e3 = (tuple(o) + (0, 0, 0))[:3], (tuple(e) + (1, 1, 1))[:3]
    api, _ = region(a.manager(), a, o3, e3)
    flag = ",".join(map(str, o)) + ":" + ",".join(map(str, e))
    c0, c1 = chunk_range(a.dims, o3, e3, a.unit, a.header.vle_pardeg)
    cover = f"fused, {-(-(o[0] + e[0]) // 1024) - o[0] // 1024} bricks" if name == "1d" else f"slab, {c1 - c0} chunks"
    for extra, word in ((["--region-mode", "cover"], cover),
                        (["--region-mode", "whole"], f"fallback, {a.header.vle_pardeg} chunks"), ([], "fallback")):
        x = subprocess.run([cz.CLI_PATH, "-x", "-i", str(f), "--region", flag] + extra, capture_output=True, text=True,
                           timeout=120)
        assert x.returncode == 0 and word in x.stdout, x.stdout + x.stderr
        np.testing.assert_array_equal(np.fromfile(tmp_path / "field.f32.cuszx", dtype=np.uint32), api)
        (tmp_path / "field.f32.cuszx").unlink()
    x = subprocess.run([cz.CLI_PATH, "-x", "-i", str(f), "--region", flag, "--region-mode", "some"], capture_output=True,
                       text=True, timeout=120)
    assert x.returncode != 0
