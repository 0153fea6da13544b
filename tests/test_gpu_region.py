"""Region-of-interest decompression (psz_amd_decompress_region_*): a box of an archive decodes to
exactly the bits that the same box of psz_decompress_* of that archive holds (whose own parity
with the oracle the other GPU tests pin), nothing around the box is written, and the fused path
decodes only the covering bricks.

The output box sits between two 4 KiB guard bands; bands and box are filled with a NaN pattern
beforehand, the bands must keep it.
"""
import functools
import subprocess

import numpy as np
import pytest

import cusz_amd as cz
from cusz_amd import datagen
from gpu_util import d2h, parse_archive, sync, to_device

pytestmark = pytest.mark.gpu

GUARD = 4096  # bytes on each side of the box
POISON = {np.float32: np.uint32(0x7FC0DEAD), np.float64: np.uint64(0x7FF8DEADBEEF0BAD)}
BITS = {np.float32: np.uint32, np.float64: np.uint64}

# name: dims, dtype, eb, radius, predictor
FIELDS = {
    "A": ((512, 24, 24), np.float32, 1e-3, 512, cz.Lorenzo),  # 2 x 3 x 3 bricks, some without outliers
    # ragged y and z; eb chosen so that its bricks hold both <= 128 and > 128 outlier cells (the
    # values in LDS / read from the archive): test_field_b_has_both_kinds_of_brick checks it
    "B": ((256, 20, 13), np.float32, 3e-4, 64, cz.Lorenzo),
    "C": ((512, 16, 16), np.float64, 3e-4, 64, cz.Lorenzo),
    "Azz": ((512, 24, 24), np.float32, 1e-3, 512, cz.LorenzoZigZag),
    "1d": ((50_000, 1, 1), np.float32, 1e-4, 512, cz.Lorenzo),
    "2d": ((300, 40, 1), np.float32, 1e-4, 512, cz.Lorenzo),
    "ref3d": ((96, 64, 40), np.float32, 1e-4, 512, cz.Lorenzo),  # x no multiple of 256: reference layout
    # (the smallest 3-D spline shape of test_gpu_spline.py: one tile plus its faces)
    "spline": ((33, 9, 9), np.float32, 3e-6, 512, cz.Spline),
}

BOXES = {
    "A": {
        "whole": ((0, 0, 0), (512, 24, 24)),
        "brick": ((256, 8, 8), (256, 8, 8)),         # the interior brick (1, 1, 1) exactly
        "unaligned": ((250, 7, 7), (13, 10, 10)),    # crosses brick borders on all three axes
        "element": ((301, 13, 9), (1, 1, 1)),
        "xcolumn": ((0, 5, 11), (512, 1, 1)),
        "zplane": ((0, 0, 13), (512, 24, 1)),
        "left": ((10, 3, 2), (200, 17, 20)),         # x < 256: blocks right of the box are not decoded
        "left_1blk": ((3, 9, 9), (40, 3, 3)),        # ... three of the four
        "right": ((300, 2, 1), (150, 20, 22)),       # x >= 256: blocks left of the box decode, store nothing
        "right_last": ((480, 0, 0), (32, 24, 24)),
    },
    "B": {
        "whole": ((0, 0, 0), (256, 20, 13)),
        "brick": ((0, 8, 0), (256, 8, 8)),
        "unaligned": ((60, 6, 6), (10, 5, 4)),       # crosses the 64-column block and the y, z brick borders
        "element": ((77, 17, 11), (1, 1, 1)),
        "xcolumn": ((0, 19, 12), (256, 1, 1)),
        "zplane": ((0, 0, 8), (256, 20, 1)),
        "corner": ((200, 15, 9), (56, 5, 4)),        # hugs the ragged far corner
        "right": ((130, 1, 1), (100, 18, 11)),       # outlier cells of the skipped left blocks carry on
    },
    "C": {
        "whole": ((0, 0, 0), (512, 16, 16)),
        "brick": ((256, 8, 8), (256, 8, 8)),
        "unaligned": ((250, 7, 7), (13, 3, 3)),
        "element": ((333, 9, 5), (1, 1, 1)),
        "xcolumn": ((0, 3, 14), (512, 1, 1)),
        "zplane": ((0, 0, 7), (512, 16, 1)),
        "right": ((400, 2, 3), (100, 12, 10)),
    },
}
CASES = [(f, b) for f in BOXES for b in BOXES[f]]


class Archive:
    """One field compressed once and decompressed once in full: the reference for every box."""

    def __init__(self, name):
        self.dims, self.dtype, eb, radius, pred = FIELDS[name]
        n = int(np.prod(self.dims))
        data = datagen.smooth3d_np(self.dims, sum(self.dims), dtype=self.dtype).reshape(-1)
        self.ctype = cz.F4 if self.dtype == np.float32 else cz.F8
        self.r = cz.Resource(self.ctype, self.dims, pred)
        d_in = to_device(data)
        ptr, self.nbytes, _ = self.r.compress(d_in.data_ptr(), eb, cz.Abs, radius)
        self.bytes = d2h(ptr, self.nbytes).tobytes()
        self.d_arch = to_device(np.frombuffer(self.bytes, np.uint8).copy())  # (the manager reuses its own buffer)
        self.header = cz.psz_header.from_buffer_copy(self.bytes[:176])
        self.full = full_decompress(self.r, self.d_arch, self.nbytes, n, self.dtype).reshape(self.dims[::-1])

    def box(self, o, e):
        return np.ascontiguousarray(self.full[o[2]:o[2] + e[2], o[1]:o[1] + e[1], o[0]:o[0] + e[0]]).reshape(-1)


def full_decompress(r, d_arch, nbytes, n, dtype):
    out = to_device(np.full(n, POISON[dtype]).view(dtype))
    r.decompress(d_arch.data_ptr(), nbytes, out.data_ptr())
    sync()
    return d2h(out.data_ptr(), n * np.dtype(dtype).itemsize, BITS[dtype])


@functools.lru_cache(maxsize=None)
def archive(name):
    return Archive(name)


def region(r, d_arch, nbytes, o, e, dtype, expect_status=None):
    """Region decode into a poisoned, guarded buffer -> (box bits, guards intact)."""
    es = np.dtype(dtype).itemsize
    g, nb = GUARD // es, max(1, int(np.prod(e)))
    buf = to_device(np.full(2 * g + nb, POISON[dtype]).view(dtype))
    d_box = buf.data_ptr() + GUARD
    if expect_status is None:
        r.decompress_region(d_arch.data_ptr(), nbytes, o, e, d_box)
    else:
        with pytest.raises(cz.PszError) as ei:
            r.decompress_region(d_arch.data_ptr(), nbytes, o, e, d_box)
        assert ei.value.status == expect_status
    sync()
    bits = d2h(buf.data_ptr(), (2 * g + nb) * es, BITS[dtype])
    guards = bool(np.all(bits[:g] == POISON[dtype]) and np.all(bits[g + nb:] == POISON[dtype]))
    return bits[g:g + nb], guards


def covering(o, e):
    lo = (o[0] // 256, o[1] // 8, o[2] // 8)
    hi = ((o[0] + e[0] - 1) // 256, (o[1] + e[1] - 1) // 8, (o[2] + e[2] - 1) // 8)
    return lo, tuple(int(h - l + 1) for h, l in zip(hi, lo))


@pytest.mark.parametrize("field,box", CASES, ids=[f"{f}-{b}" for f, b in CASES])
def test_region_equals_the_box_of_the_full_decompress(field, box):
    a = archive(field)
    o, e = BOXES[field][box]
    got, guards = region(a.r, a.d_arch, a.nbytes, o, e, a.dtype)
    info = a.r.last_region()
    np.testing.assert_array_equal(got, a.box(o, e))
    assert guards, "written outside the box"
    lo, n = covering(o, e)
    assert info.path == cz.REGION_FUSED
    assert (info.brick_lo.x, info.brick_lo.y, info.brick_lo.z) == lo
    assert (info.brick_n.x, info.brick_n.y, info.brick_n.z) == n
    assert info.bricks == int(np.prod(n)) and info.chunks == 64 * info.bricks and info.elems == int(np.prod(e))
    if box == "brick":
        assert info.bricks == 1 and info.chunks == 64


def test_field_b_has_both_kinds_of_brick():
    """The boxes of B touch a brick whose outlier values fit the decoder's LDS (1 .. 128 cells) and
    one whose values it reads from the archive (> 128 cells)."""
    a = archive("B")
    idx = parse_archive(a.bytes, 128)["ol_idx"].astype(np.int64)
    x, y, z = a.dims
    gx, gy, gz = idx % x, idx // x % y, idx // (x * y)
    nbx, nby = x // 256, (y + 7) // 8
    per = np.bincount((gz // 8 * nby + gy // 8) * nbx + gx // 256, minlength=nbx * nby * ((z + 7) // 8))
    touched = set()
    for o, e in BOXES["B"].values():
        lo, n = covering(o, e)
        touched |= {((lo[2] + k) * nby + lo[1] + j) * nbx + lo[0] + i
                    for k in range(n[2]) for j in range(n[1]) for i in range(n[0])}
    counts = per[sorted(touched)]
    assert np.any((counts >= 1) & (counts <= 128)), counts
    assert np.any(counts > 128), counts


def test_region_waves_take_a_second_brick():
    """More covering bricks than the launch has waves (min(CUs, bricks) workgroups of 8): a wave
    hands over to its next brick -- fetched during the last block, prefetched at its reconstruction
    -- in the box walk as it does in the field walk; every other box of this file has at most 18
    bricks.  512 x 256 x 260 f32: 2 x 32 x 33 = 2112 bricks, the last z layer 4 planes deep, some
    with outlier cells.  The whole field as a box; the box from x = 300 on; and the box from x = 400
    on, where each brick's first two blocks lie left of the box (they store nothing, and their zero
    codes still consume the rows' cells).  Field, reference and boxes stay on the device."""
    import torch

    dims, eb, radius = (512, 256, 260), 1e-3, 512
    n = int(np.prod(dims))
    bricks = (dims[0] // 256) * ((dims[1] + 7) // 8) * ((dims[2] + 7) // 8)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert bricks > 8 * cus, (bricks, cus)
    r = cz.Resource(cz.F4, dims, cz.Lorenzo)
    d_in = datagen.smooth3d_torch(dims, seed=sum(dims))
    ptr, nbytes, _ = r.compress(d_in.data_ptr(), eb, cz.Abs, radius)
    raw = d2h(ptr, nbytes)
    del d_in
    h = cz.psz_header.from_buffer_copy(raw[:176].tobytes())
    idx = raw[h.entry[3]:h.entry[4]].view(np.uint32).reshape(-1, 2)[:, 1].astype(np.int64)
    of_brick = (idx // (dims[0] * dims[1]) // 8 * 32 + idx // dims[0] % dims[1] // 8) * 2 + idx % dims[0] // 256
    print(f"{len(np.unique(of_brick))} of {bricks} bricks hold outlier cells ({len(idx)} cells)")
    assert len(idx) > 0 and of_brick.max() < bricks
    d_arch = to_device(raw)
    poison = int(POISON[np.float32])
    full = torch.full((n,), poison, dtype=torch.int32, device="cuda")
    r.decompress(d_arch.data_ptr(), nbytes, full.data_ptr())
    sync()
    full = full.view(dims[2], dims[1], dims[0])
    g = GUARD // 4
    for ox, nbr in ((0, bricks), (300, bricks // 2), (400, bricks // 2)):
        o, e = (ox, 0, 0), (dims[0] - ox, dims[1], dims[2])
        nb = int(np.prod(e))
        buf = torch.full((2 * g + nb,), poison, dtype=torch.int32, device="cuda")
        r.decompress_region(d_arch.data_ptr(), nbytes, o, e, buf.data_ptr() + GUARD)
        sync()
        info = r.last_region()
        assert info.path == cz.REGION_FUSED and info.bricks == nbr
        assert torch.equal(buf[g:g + nb].view(e[2], e[1], e[0]), full[:, :, ox:]), ox
        assert bool((buf[:g] == poison).all()) and bool((buf[g + nb:] == poison).all()), "written outside the box"


FALLBACK_BOXES = {
    "1d": ((12_345, 0, 0), (20_001, 1, 1)),
    "2d": ((17, 5, 0), (250, 30, 1)),
    "ref3d": ((5, 7, 9), (80, 50, 30)),
    "Azz": ((250, 7, 7), (13, 10, 10)),
    "spline": ((3, 2, 1), (29, 6, 7)),
}


@pytest.mark.parametrize("field", list(FALLBACK_BOXES))
def test_fallback_paths(field):
    a = archive(field)
    o, e = FALLBACK_BOXES[field]
    got, guards = region(a.r, a.d_arch, a.nbytes, o, e, a.dtype)
    np.testing.assert_array_equal(got, a.box(o, e))
    assert guards
    info = a.r.last_region()
    assert info.path == cz.REGION_FALLBACK and info.bricks == 0 and info.elems == int(np.prod(e))


def test_forced_lane_decoder_falls_back():
    a = archive("A")
    r = cz.Resource(cz.F4, None, header=a.header)
    r.set_decoder(cz.DECODER_LANE)
    o, e = BOXES["A"]["unaligned"]
    got, guards = region(r, a.d_arch, a.nbytes, o, e, a.dtype)
    np.testing.assert_array_equal(got, a.box(o, e))
    assert guards and r.last_region().path == cz.REGION_FALLBACK


def test_cells_in_another_order_fall_back():
    """The archive's outlier cells reversed: still a valid archive (the full decompress scatters
    them), but not in brick order, which the region call learns from its one read-back."""
    a = archive("B")
    h = a.header
    raw = np.frombuffer(a.bytes, np.uint8).copy()
    cells = raw[h.entry[3]:h.entry[4]].view(np.uint32).reshape(-1, 2)
    assert len(cells) > 1
    cells[:] = cells[::-1].copy()
    d_arch = to_device(raw)
    r = cz.Resource(cz.F4, None, header=h)
    o, e = BOXES["B"]["unaligned"]
    got, guards = region(r, d_arch, a.nbytes, o, e, a.dtype)
    np.testing.assert_array_equal(got, a.box(o, e))
    assert guards and r.last_region().path == cz.REGION_FALLBACK
    # the same manager then takes the fused path for the archive as written
    got, guards = region(r, a.d_arch, a.nbytes, o, e, a.dtype)
    np.testing.assert_array_equal(got, a.box(o, e))
    assert guards and r.last_region().path == cz.REGION_FUSED


def test_repeat_with_a_full_decompress_in_between():
    a = archive("B")
    o, e = BOXES["B"]["corner"]
    first, g1 = region(a.r, a.d_arch, a.nbytes, o, e, a.dtype)
    full = full_decompress(a.r, a.d_arch, a.nbytes, int(np.prod(a.dims)), a.dtype)
    second, g2 = region(a.r, a.d_arch, a.nbytes, o, e, a.dtype)
    np.testing.assert_array_equal(first, second)
    np.testing.assert_array_equal(first, a.box(o, e))
    np.testing.assert_array_equal(full.reshape(a.full.shape), a.full)
    assert g1 and g2 and a.r.last_region().path == cz.REGION_FUSED


@pytest.mark.parametrize("o,e", [
    ((0, 0, 0), (0, 1, 1)), ((512, 0, 0), (1, 1, 1)), ((0, 24, 0), (1, 1, 1)), ((0, 0, 24), (1, 1, 1)),
    ((500, 0, 0), (13, 1, 1)), ((0, 20, 0), (4, 5, 4)), ((0, 0, 23), (8, 8, 2)),
])
def test_boxes_outside_the_field_are_rejected_and_write_nothing(o, e):
    a = archive("A")
    got, guards = region(a.r, a.d_arch, a.nbytes, o, e, a.dtype, expect_status=cz.PSZ_AMD_ERR_INVALID_ARG)
    assert guards and np.all(got == POISON[a.dtype])


def test_dtype_mismatch_and_truncated_archive():
    a = archive("A")
    buf = to_device(np.full(64, POISON[np.float64]).view(np.float64))
    st = cz.lib().psz_amd_decompress_region_double(a.r._h, a.d_arch.data_ptr(), a.nbytes, cz.psz_len(0, 0, 0),
                                                   cz.psz_len(4, 1, 1), buf.data_ptr())
    assert st == cz.PSZ_ABORT_UNSUPPORTED_TYPE
    got, guards = region(a.r, a.d_arch, a.nbytes - 8, (0, 0, 0), (4, 1, 1), a.dtype,
                         expect_status=cz.PSZ_AMD_ERR_BAD_ARCHIVE)
    assert guards and np.all(got == POISON[a.dtype])
    sync()
    assert np.all(d2h(buf.data_ptr(), 64 * 8, np.uint64) == POISON[np.float64])


def test_cli_region(tmp_path):
    a = archive("A")
    f = tmp_path / "field.f32.cusza"
    f.write_bytes(a.bytes)
    o, e = BOXES["A"]["unaligned"]
    flag = ",".join(map(str, o)) + ":" + ",".join(map(str, e))
    x = subprocess.run([cz.CLI_PATH, "-x", "-i", str(f), "--region", flag], capture_output=True, text=True, timeout=120)
    assert x.returncode == 0, x.stderr
    got = np.fromfile(tmp_path / "field.f32.cuszx", dtype=np.uint32)
    api, _ = region(a.r, a.d_arch, a.nbytes, o, e, a.dtype)
    np.testing.assert_array_equal(got, api)
    x = subprocess.run([cz.CLI_PATH, "-x", "-i", str(f)], capture_output=True, text=True, timeout=120)
    assert x.returncode == 0, x.stderr
    np.testing.assert_array_equal(np.fromfile(tmp_path / "field.f32.cuszx", dtype=np.uint32), a.full.reshape(-1))
    x = subprocess.run([cz.CLI_PATH, "-x", "-i", str(f), "--region", "500,0,0:13,1,1"], capture_output=True, text=True,
                       timeout=120)
    assert x.returncode != 0
