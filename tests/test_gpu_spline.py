"""cuSZ-i spline3 path on the GPU, through the C-ABI, against the CPU oracle.

Parity with the reference itself is UNPINNED (the reference has no test and no wired
pipeline for spline3, compressor.inl:358-361/:495-497); the oracle restates spline3.inl.
Bit-exact here: quant codes, anchors, outlier cells (value bits, index AND order: tile order,
then (z,y,x) inside the 32x8x8 tile), histogram, Huffman segment, and the decompressed field.
"""
import numpy as np
import pytest

import cusz_amd as cz
from cusz_amd import datagen
from gpu_util import d2h, empty_device, parse_archive, sync, to_device
from gpu_util import spline_roundtrip as _roundtrip

pytestmark = pytest.mark.gpu

CASES = [
    ((64, 32, 16), np.float32, 1e-3),
    ((64, 32, 16), np.float64, 1e-3),
    ((70, 19, 13), np.float32, 3e-6),   # ragged tiles, ~5 % outliers
    ((70, 19, 13), np.float64, 5e-6),
    ((45, 37, 1), np.float64, 3e-6),    # 2-D
    ((1000, 1, 1), np.float32, 3e-6),   # 1-D
    ((33, 9, 9), np.float32, 3e-6),     # one tile plus its faces
    ((160, 96, 72), np.float64, 3e-6),
]


@pytest.mark.parametrize("dims,dtype,eb", CASES)
def test_spline_parity(oracle, dims, dtype, eb):
    data, x, ebx, nol = _roundtrip(oracle, dims, dtype, eb)
    err = np.max(np.abs(x.astype(np.float64) - data))
    # the reference quantises with float eb parameters (FP = float, spline3.cu:36) and, for f32,
    # reconstructs in f32: the bound holds up to those roundings.  Measured worst over these
    # cases (scripts/spline_err.py, round 2): f32 1.00334 eb, f64 1.00031 eb.
    tol = 1.001 if dtype == np.float64 else 1.005
    assert err <= tol * ebx, (err / ebx, nol)


def test_spline_beyond_ten_percent_outliers():
    """More than the reference's 10 % outliers (buf_comp.hh:55): the capacity grows, the archive
    is valid and decompresses within the bound (float rounding: spline f32 tolerance)."""
    import torch

    dims = (70, 19, 13)
    data = datagen.smooth3d_np(dims, 5)
    r = cz.Resource(cz.F4, dims, cz.Spline)
    d_in = to_device(data)
    ptr, nb, st = r.compress(d_in.data_ptr(), 1e-6, cz.Abs)
    assert st == cz.PSZ_SUCCESS
    assert r.header.splen > data.size // 10
    out = torch.empty(data.size, dtype=torch.float32, device="cuda")
    r.decompress(ptr, nb, out.data_ptr())
    sync()
    err = np.abs(out.cpu().numpy().astype(np.float64) - data).max()
    # eb = 1e-6 is ~8 f32 ulps of these values: the float reconstruction's rounding adds a few
    assert err <= 1e-6 + 4 * 2.0 ** -23 * np.abs(data).max(), err
    r.close()


def test_spline_rel_mode(oracle):
    _roundtrip(oracle, (96, 40, 24), np.float64, 1e-6, mode=cz.Rel)


def test_spline_fullsize_512(oracle):
    """BASELINE config 5 size (512^3 f64, r2r 1e-6): error bound and anchors on every element,
    codes of two tile-aligned slabs against the oracle (tiles are independent)."""
    import torch

    dims = (512, 512, 512)
    n = 512 ** 3
    d_in = datagen.smooth3d_torch(dims, seed=5, device="cuda").double()
    r = cz.Resource(cz.F8, dims, cz.Spline)
    ptr, nbytes, _ = r.compress(d_in.data_ptr(), 1e-6, cz.Rel)
    ebx = r.header.rc.eb
    out = torch.empty(n, dtype=torch.float64, device="cuda")
    r.decompress(ptr, nbytes, out.data_ptr())
    sync()
    err = (out - d_in).abs().max().item()
    assert err <= 1.001 * ebx, err / ebx
    ino = r.internals()
    codes = d2h(ino.d_quant_codes, 2 * n, np.uint16).reshape(512, 512, 512)
    host = d_in.cpu().numpy().reshape(512, 512, 512)
    for z0 in (0, 256):  # slab of 8 planes (+1 face plane for the predictor)
        sub = np.ascontiguousarray(host[z0:z0 + 9])
        co, _, _, _ = oracle.spline3_c(sub, (512, 512, 9), ebx)
        np.testing.assert_array_equal(codes[z0:z0 + 8].ravel(), co.reshape(9, 512, 512)[:8].ravel())
    r.close()


@pytest.mark.parametrize("order", ["reversed_in_tile", "shuffled"])
def test_spline_decompress_reordered_outliers(order):
    """Outlier cells in any order decompress identically: tile-sorted but not (z, y, x) inside a
    tile (read as the per-tile lists directly), and fully shuffled (the bucket kernels rebuild
    the per-tile lists)."""
    import torch

    dims, dtype, eb = (70, 19, 13), np.float32, 3e-6
    n = int(np.prod(dims))
    data = datagen.smooth3d_np(dims, 5, dtype=dtype)
    r = cz.Resource(cz.F4, dims, cz.Spline)
    d_in = to_device(data)
    ptr, nbytes, _ = r.compress(d_in.data_ptr(), eb, cz.Abs)
    arch = bytearray(d2h(ptr, nbytes).tobytes())
    out0 = empty_device(n, torch.float32)
    r.decompress(ptr, nbytes, out0.data_ptr())
    sync()
    h = parse_archive(bytes(arch))["header"]
    cells = np.frombuffer(bytes(arch[h.entry[3]:h.entry[4]]), np.uint64).copy()
    assert cells.size > 100
    if order == "shuffled":
        cells = cells[np.random.default_rng(1).permutation(cells.size)]
    else:
        gid = (cells >> np.uint64(32)).astype(np.int64)
        gx, gy, gz = gid % dims[0], (gid // dims[0]) % dims[1], gid // (dims[0] * dims[1])
        gdx, gdy = (dims[0] + 31) // 32, (dims[1] + 7) // 8
        tile = gx // 32 + gdx * (gy // 8 + gdy * (gz // 8))
        cells = cells[np.lexsort((-gid, tile))]  # tile order kept, descending inside a tile
    arch[h.entry[3]:h.entry[4]] = cells.tobytes()
    d_arch = torch.tensor(np.frombuffer(bytes(arch), np.uint8)).cuda()
    out1 = empty_device(n, torch.float32)
    r.decompress(d_arch.data_ptr(), nbytes, out1.data_ptr())
    sync()
    np.testing.assert_array_equal(out1.cpu().numpy().view(np.uint32), out0.cpu().numpy().view(np.uint32))
    r.close()
