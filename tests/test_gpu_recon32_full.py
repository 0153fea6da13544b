"""The 32-column reconstruction's full-brick path (`recon_block32<..., FULL>`, brick3_decode.hip):
bricks with all 8 rows and all 8 planes inside the field are reconstructed in one straight line,
without row or plane tests; ragged bricks keep the guarded body.  The launcher takes 32-column
blocks for f32 fields of at least 12 bricks per CU (3072 on MI355X), so the shapes here are the
smallest that select it.  Every case decompresses into a NaN-filled buffer and must equal the
oracle's reconstruction bit for bit (lrz_x.cuhip.inl:271-360 order).

  * 512 x 512 x 192: exactly 3072 bricks, all full.  Spikes give outliers; brick 0 holds the dense
    head block of 256 * 8 * 3 elements, far more cells than a brick stages in LDS (128).
    Lorenzo takes them as ranked cells; ZigZag, and Lorenzo with the archive's cells shuffled
    (the bounds pass then reports them unsorted), read them from the scattered field.
  * 512 x 508 x 192 (ragged in y only) and 768 x 512 x 132 (ragged in z only): full and ragged
    bricks in one launch.
  * all +0.0, all -0.0 and a constant: the y running sum starts from -0.0 in the lower lane half
    and from the lower half's sum in the upper, so the signed zeros and a lone outlier at the
    field's first element pin the start value."""
import functools

import numpy as np
import pytest
import torch

import cusz_amd as cz
from gpu_util import d2h, empty_device, parse_archive, sync, to_device

pytestmark = pytest.mark.gpu

EB = 1e-4
FULL_DIMS = (512, 512, 192)
KCELLCAP = 128  # outlier values of a brick kept in LDS (brick3_decode.hip)


def _field(dims, seed, spikes):
    """test_gpu_brick32.py's recipe."""
    x, y, z = dims
    rng = np.random.default_rng(seed)
    xs = np.arange(x, dtype=np.float64)
    ys = np.arange(y, dtype=np.float64)[:, None]
    plane = np.sin(0.05 * xs)[None, :] * np.cos(0.07 * ys)
    out = np.empty((z, y, x), np.float32)
    for k in range(z):
        out[k] = plane + 0.5 * np.sin(0.03 * k + 0.01 * xs)[None, :]
    f = out.ravel()
    f += (1e-3 * rng.standard_normal(f.size)).astype(np.float32)
    if spikes:
        idx = rng.choice(f.size, size=spikes, replace=False)
        f[idx] += rng.uniform(-50, 50, size=spikes).astype(np.float32)
        f[: 256 * 8 * 3] += rng.uniform(-50, 50, size=256 * 8 * 3).astype(np.float32)
    return f


@functools.lru_cache(maxsize=2)
def _spiked():
    data = _field(FULL_DIMS, sum(FULL_DIMS), 20000)
    data.setflags(write=False)
    return data


@functools.lru_cache(maxsize=2)
def _reference(oracle, kind, zigzag):
    """(field, oracle reconstruction, outlier indices), computed once per field and predictor."""
    dims = FULL_DIMS
    if kind == "spiked":
        data = _spiked()
    else:
        value = {"+0": 0.0, "-0": -0.0, "const": 1.5}[kind]
        data = np.full(int(np.prod(dims)), value, np.float32)
    codes, ov, oi = oracle.lorenzo_c(data, dims, EB, 512, zigzag)
    want = oracle.lorenzo_x(codes, ov, oi, dims, EB, 512, zigzag, np.float32)
    want.setflags(write=False)
    return data, want, oi


def _nbricks(dims):
    return (dims[0] // 256) * -(-dims[1] // 8) * -(-dims[2] // 8)


def _decompress_and_compare(r, ptr, nbytes, want):
    out = empty_device(want.size, torch.float32)
    out.fill_(float("nan"))
    r.decompress(ptr, nbytes, out.data_ptr())
    sync()
    xg = out.cpu().numpy()
    bad = np.flatnonzero(xg.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, f"{bad.size} mismatches, first {bad[:5]}: {xg[bad[:5]]} vs {want[bad[:5]]}"


def _roundtrip(data, dims, zigzag, want, shuffle_cells=False):
    r = cz.Resource(cz.F4, dims, cz.LorenzoZigZag if zigzag else cz.Lorenzo)
    d_in = to_device(data)
    ptr, nbytes, _ = r.compress(d_in.data_ptr(), EB)
    assert r.internals().layout == cz.LAYOUT_BRICK
    if shuffle_cells:
        arch = bytearray(d2h(ptr, nbytes).tobytes())
        h = parse_archive(bytes(arch))["header"]
        cells = np.frombuffer(bytes(arch[h.entry[3]:h.entry[4]]), np.uint64).copy()
        assert cells.size > 1000
        arch[h.entry[3]:h.entry[4]] = cells[np.random.default_rng(3).permutation(cells.size)].tobytes()
        d_arch = to_device(np.frombuffer(bytes(arch), np.uint8).copy())
        _decompress_and_compare(r, d_arch.data_ptr(), nbytes, want)
    else:
        _decompress_and_compare(r, ptr, nbytes, want)
    r.close()


@pytest.mark.parametrize("zigzag,shuffle_cells", [(False, False), (True, False), (False, True)],
                         ids=["ranked_cells", "zigzag_scatter", "shuffled_cells_scatter"])
def test_full_bricks_with_outliers(oracle, zigzag, shuffle_cells):
    dims = FULL_DIMS
    assert _nbricks(dims) == 12 * 256 and dims[1] % 8 == 0 and dims[2] % 8 == 0  # 32-column mode, all full
    data, want, oi = _reference(oracle, "spiked", zigzag)
    assert oi.size > 1000
    # brick 0 (x < 256, y < 8, z < 8) holds the dense head block: past the LDS cell stage
    xi, yi, zi = oi % dims[0], oi // dims[0] % dims[1], oi // (dims[0] * dims[1])
    assert np.count_nonzero((xi < 256) & (yi < 8) & (zi < 8)) > KCELLCAP
    _roundtrip(data, dims, zigzag, want, shuffle_cells)


@pytest.mark.parametrize("dims,spikes", [
    ((512, 508, 192), 20000),  # 2 x 64 x 24 = 3072 bricks, the last brick row 4 rows high
    ((768, 512, 132), 0),      # 3 x 64 x 17 = 3264 bricks, the last brick plane 4 planes deep
], ids=["ragged_y", "ragged_z"])
def test_full_and_ragged_bricks_in_one_launch(oracle, dims, spikes):
    assert _nbricks(dims) >= 12 * 256
    assert (dims[1] % 8 != 0) != (dims[2] % 8 != 0)
    data = _field(dims, sum(dims), spikes)
    codes, ov, oi = oracle.lorenzo_c(data, dims, EB, 512, False)
    if spikes:
        assert oi.size > 1000
    want = oracle.lorenzo_x(codes, ov, oi, dims, EB, 512, False, np.float32)
    _roundtrip(data, dims, False, want)


@pytest.mark.parametrize("kind", ["+0", "-0", "const"])
def test_full_bricks_signed_zeros_and_constant(oracle, kind):
    dims = FULL_DIMS
    assert _nbricks(dims) == 12 * 256
    data, want, oi = _reference(oracle, kind, False)
    if kind == "const":
        assert oi.size >= 1  # the field's first element: its start value comes from a cell
    _roundtrip(data, dims, False, want)
