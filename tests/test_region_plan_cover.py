"""psz_amd_region_plan_mode (host only, no GPU).  WHOLE is psz_amd_region_plan field by field; COVER
gives every Lorenzo archive off the fused path the covering slab: the path and the chunk count
against the formulas of include/cusz_amd.h written out again here, and against a brute-force
marking of the chunks that hold a code of the slab.  The arithmetic itself (region_cover.hh) is
also compiled with g++ alone and checked value by value."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import cusz_amd as cz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHOLE, COVER = cz.REGION_MODE_WHOLE, cz.REGION_MODE_COVER


def _header(dims, dtype=cz.F4, predictor=cz.Lorenzo, sublen=256, radius=512, codec=cz.Huffman):
    h = cz.psz_header()
    x, y, z = (tuple(dims) + (1, 1, 1))[:3]
    h.dtype = dtype
    h.pipeline.predictor = predictor
    h.pipeline.codec1 = codec
    h.rc.radius = radius
    h.vle_sublen = sublen
    h.vle_pardeg = (x * y * z + sublen - 1) // sublen
    h.len = cz.psz_len(x, y, z)
    return h


# name: (dims, header keywords, path under COVER)
FIELDS = {
    "1d-50000": ((50_000, 1, 1), {}, cz.REGION_FUSED),    # 1-D, chunks of 256: the fused 1-D path
    "1d-200003": ((200_003, 1, 1), {}, cz.REGION_FUSED),
    "1d-200003-f64": ((200_003, 1, 1), dict(dtype=cz.F8, radius=64), cz.REGION_FUSED),
    "1d-200003-zz": ((200_003, 1, 1), dict(predictor=cz.LorenzoZigZag), cz.REGION_SLAB),
    "1d-200003-s512": ((200_003, 1, 1), dict(sublen=512), cz.REGION_SLAB),
    "2d-300x70-s256": ((300, 70, 1), dict(sublen=256), cz.REGION_SLAB),
    "2d-300x70-s2048": ((300, 70, 1), dict(sublen=2048), cz.REGION_SLAB),
    "2d-300x70-s8192": ((300, 70, 1), dict(sublen=8192), cz.REGION_SLAB),
    "2d-3600x1800-s256": ((3600, 1800, 1), dict(sublen=256), cz.REGION_SLAB),
    "2d-3600x1800-s2048": ((3600, 1800, 1), dict(sublen=2048), cz.REGION_SLAB),
    "2d-3600x1800-s8192": ((3600, 1800, 1), dict(sublen=8192), cz.REGION_SLAB),
    "3d-96x64x40": ((96, 64, 40), {}, cz.REGION_SLAB),
    "3d-256x20x13-zz": ((256, 20, 13), dict(predictor=cz.LorenzoZigZag), cz.REGION_SLAB),
    "3d-96x64x40-f64-zz": ((96, 64, 40), dict(predictor=cz.LorenzoZigZag, dtype=cz.F8, radius=64), cz.REGION_SLAB),
    "3d-512x24x24-s1024": ((512, 24, 24), dict(sublen=1024), cz.REGION_SLAB),
    "fzg-96x64x40": ((96, 64, 40), dict(codec=cz.FZCodec, sublen=4096), cz.REGION_SLAB),
    "fzg-1d-50000": ((50_000, 1, 1), dict(codec=cz.FZCodec, sublen=4096, predictor=cz.LorenzoZigZag), cz.REGION_SLAB),
    "spline": ((96, 64, 40), dict(predictor=cz.Spline), cz.REGION_FALLBACK),
    "codec-lc": ((96, 64, 40), dict(codec=2), cz.REGION_FALLBACK),  # psz_codec LC: no decoder here
    "3d-512x24x24": ((512, 24, 24), {}, cz.REGION_FUSED),
}


def _ndim(dims):
    return 3 if dims[2] != 1 else 2 if dims[1] != 1 else 1


def _slab(dims, o, e):
    """(a P, b P): the code range of the covering slab, by the header comment's formulas"""
    nd = _ndim(dims)
    T = {1: 1024, 2: 32, 3: 8}[nd]
    P = int(np.prod(dims[:nd - 1], dtype=np.int64))
    ln, os_, es = dims[nd - 1], o[nd - 1], e[nd - 1]
    a = os_ // T * T
    b = min(ln, -(-(os_ + es) // T) * T)
    return a * P, b * P


def _chunks_formula(dims, o, e, sublen, pardeg):
    lo, hi = _slab(dims, o, e)
    return min(pardeg, -(-hi // sublen)) - lo // sublen


def _chunks_brute(dims, o, e, sublen, pardeg):
    """chunks holding a code of the slab, by marking every code of the slab"""
    lo, hi = _slab(dims, o, e)
    mark = np.zeros(pardeg * sublen, bool)
    mark[lo:hi] = True
    return int(mark.reshape(pardeg, sublen).any(axis=1).sum())


def _boxes(dims, count, rng):
    out = [((0, 0, 0), tuple(dims)),                                        # the whole field
           (tuple(d - 1 for d in dims), (1, 1, 1)), ((0, 0, 0), (1, 1, 1)),  # one element: last, first
           (tuple(d // 2 for d in dims), (1, 1, 1)),
           (tuple(d // 3 for d in dims), tuple(d - d // 3 for d in dims))]   # ending at the far faces
    for _ in range(count):
        o = [int(rng.integers(0, d)) for d in dims]
        e = [int(rng.integers(1, d - a + 1)) for d, a in zip(dims, o)]
        if rng.random() < 0.4:  # small boxes
            e = [min(x, int(rng.integers(1, 40))) for x in e]
        out.append((tuple(o), tuple(e)))
    return out


def _fields(r):
    return (r.path, r.brick_lo.x, r.brick_lo.y, r.brick_lo.z, r.brick_n.x, r.brick_n.y, r.brick_n.z, r.bricks, r.chunks,
            r.elems)


@pytest.mark.parametrize("name", list(FIELDS))
def test_whole_is_region_plan_and_cover_follows_the_formulas(name):
    dims, kw, path = FIELDS[name]
    h = _header(dims, **kw)
    sublen, pardeg = h.vle_sublen, h.vle_pardeg
    brute = int(np.prod(dims)) <= 1 << 20  # (marking 3600 x 1800 for every box would take seconds)
    rng = np.random.default_rng(sum(dims) + sublen)
    nd = _ndim(dims)
    for o, e in _boxes(dims, 100, rng):
        old = cz.psz_amd_region_info()
        assert cz.lib().psz_amd_region_plan(h, cz.psz_len(*o), cz.psz_len(*e), old) == cz.PSZ_SUCCESS
        whole, cover = cz.region_plan(h, o, e, WHOLE), cz.region_plan(h, o, e, COVER)
        assert _fields(old) == _fields(whole) == _fields(cz.region_plan(h, o, e)), (o, e)
        assert cover.path == path and cover.elems == int(np.prod(e)), (o, e)
        if path == cz.REGION_SLAB:
            assert whole.path == cz.REGION_FALLBACK and whole.chunks == pardeg
            assert _fields(cover)[1:8] == (0,) * 7, (o, e)
            assert cover.chunks == _chunks_formula(dims, o, e, sublen, pardeg), (o, e)
            if brute:
                assert cover.chunks == _chunks_brute(dims, o, e, sublen, pardeg), (o, e)
            if o[nd - 1] == 0 and e[nd - 1] == dims[nd - 1]:
                assert cover.chunks == pardeg
        elif nd == 1:  # fused 1-D: the brick fields count tiles of 1024
            t0, t1 = o[0] // 1024, -(-(o[0] + e[0]) // 1024)
            assert whole.path == cz.REGION_FALLBACK and whole.chunks == pardeg
            assert _fields(cover)[1:8] == (t0, 0, 0, t1 - t0, 1, 1, t1 - t0), (o, e)
            assert cover.chunks == min(4 * t1, pardeg) - 4 * t0, (o, e)
            hit = np.zeros(pardeg * 256, bool)  # and by marking the covering tiles' elements
            hit[t0 * 1024:min(t1 * 1024, dims[0])] = True
            assert cover.chunks == int(hit.reshape(pardeg, 256).any(axis=1).sum()), (o, e)
        else:  # 3-D FUSED candidates and FALLBACK archives: the mode changes nothing
            assert _fields(cover) == _fields(whole), (o, e)


def test_chunk_counts_at_chosen_boxes():
    """Closed-form cases: a P no multiple of the chunk length, and a chunk longer than the slab."""
    h = _header((300, 70, 1), sublen=2048)  # rows 32..63 are codes 9600..19199: chunks 4..9
    assert cz.region_plan(h, (5, 40, 0), (7, 3, 1), COVER).chunks == 6
    h = _header((300, 70, 1), sublen=8192)  # rows 64..69 are codes 19200..20999: inside chunk 2
    assert cz.region_plan(h, (0, 69, 0), (300, 1, 1), COVER).chunks == 1
    h = _header((3600, 1800, 1), sublen=8192)  # rows 992..1023: codes 3571200..3686399
    assert cz.region_plan(h, (0, 1000, 0), (1, 1, 1), COVER).chunks == (3686400 + 8191) // 8192 - 3571200 // 8192
    h = _header((200_003, 1, 1))  # fused 1-D; the last tile: 323 elements, two chunks
    p = cz.region_plan(h, (200_002, 0, 0), (1, 1, 1), COVER)
    assert (p.path, p.brick_lo.x, p.bricks, p.chunks) == (cz.REGION_FUSED, 195, 1, 2)
    p = cz.region_plan(h, (1023, 0, 0), (2, 1, 1), COVER)
    assert (p.path, p.brick_lo.x, p.brick_n.x, p.bricks, p.chunks) == (cz.REGION_FUSED, 0, 2, 2, 8)
    h = _header((200_003, 1, 1), sublen=512)  # another chunk length: the slab
    assert cz.region_plan(h, (1023, 0, 0), (2, 1, 1), COVER).chunks == 4
    h = _header((96, 64, 40), codec=cz.FZCodec, sublen=4096)  # planes 8..15: 49152 codes = 12 blocks
    assert cz.region_plan(h, (3, 3, 9), (2, 2, 2), COVER).chunks == 12


def test_bad_mode_and_bad_boxes():
    h = _header((300, 70, 1))
    out = cz.psz_amd_region_info()
    L = cz.lib()
    for mode in (-1, 2, 7):
        assert L.psz_amd_region_plan_mode(h, cz.psz_len(0, 0, 0), cz.psz_len(1, 1, 1), mode, out) == cz.PSZ_AMD_ERR_INVALID_ARG
        with pytest.raises(cz.PszError):
            cz.region_plan(h, (0, 0, 0), (1, 1, 1), mode)
    for mode in (WHOLE, COVER):  # the box is validated as before
        for o, e in [((0, 0, 0), (0, 1, 1)), ((300, 0, 0), (1, 1, 1)), ((0, 69, 0), (1, 2, 1)), ((0, 0, 1), (1, 1, 1))]:
            assert L.psz_amd_region_plan_mode(h, cz.psz_len(*o), cz.psz_len(*e), mode, out) == cz.PSZ_AMD_ERR_INVALID_ARG


# ---- region_cover.hh with g++ alone ---------------------------------------------------------------
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("region_plan") / "libregionshim.so"
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "cusz_amd", "csrc"), "-o", str(out),
           os.path.join(ROOT, "tests", "host", "region_plan_shim.cc")]
    if shutil.which("g++") is None:
        pytest.skip("g++ unavailable")
    try:
        subprocess.run(cmd, check=True, capture_output=True, timeout=120)
    except subprocess.CalledProcessError as e:
        pytest.fail(f"region_cover.hh does not compile with g++ alone:\n{e.stderr.decode()}")
    lib = C.CDLL(str(out))
    lib.region_shim_cover.restype = None
    lib.region_shim_cover.argtypes = [C.c_int] + [C.c_size_t] * 7 + [C.c_void_p]
    lib.region_shim_tiles1.restype = C.c_size_t
    lib.region_shim_tiles1.argtypes = [C.c_size_t] * 3 + [C.c_void_p]
    return lib


def test_cover_header_alone(shim):
    out = np.zeros(6, np.uint64)
    rng = np.random.default_rng(11)
    for name in ("1d-200003", "2d-300x70-s2048", "2d-3600x1800-s8192", "3d-96x64x40"):
        dims, kw, _ = FIELDS[name]
        h = _header(dims, **kw)
        nd = _ndim(dims)
        for o, e in _boxes(dims, 50, rng):
            shim.region_shim_cover(nd, *dims, o[nd - 1], e[nd - 1], h.vle_sublen, h.vle_pardeg, out.ctypes.data)
            T, P, a, b, c0, c1 = (int(v) for v in out)
            lo, hi = _slab(dims, o, e)
            assert (a * P, b * P) == (lo, hi) and T == {1: 1024, 2: 32, 3: 8}[nd]
            assert (c0, c1) == (lo // h.vle_sublen, min(h.vle_pardeg, -(-hi // h.vle_sublen)))
            assert c1 - c0 == cz.region_plan(h, o, e, COVER).chunks
    # offsets past 2^32 stay exact: 2^31 + 2^24 rows of 4 elements, a box at row 2^31 + 5
    rows = 2**31 + 2**24
    shim.region_shim_cover(2, 4, rows, 1, 2**31 + 5, 40, 256, 4 * rows // 256, out.ctypes.data)
    assert [int(v) for v in out] == [32, 4, 2**31, 2**31 + 64, 2**33 // 256, 2**33 // 256 + 1]
    # the fused 1-D path's tiles
    n, nchunks = 200_003, (200_003 + 255) // 256
    for o, e in [(0, n), (70_001, 1), (1_200, 200), (1_900, 300), (65_500, 100), (n - 777, 777), (n - 1, 1)]:
        chunks = shim.region_shim_tiles1(o, e, nchunks, out.ctypes.data)
        t0, t1 = o // 1024, -(-(o + e) // 1024)
        assert (int(out[0]), int(out[1]), chunks) == (t0, t1, min(4 * t1, nchunks) - 4 * t0)
    assert shim.region_shim_tiles1(2**32 - 6, 1, 2**24, out.ctypes.data) == 4 and int(out[0]) == 2**22 - 1
