"""The 3-D decoder's 32-column mode (12 waves per CU, `recon_block32`), which the launcher picks
for f32 fields of at least 12 bricks per CU (3072 on MI355X): parity needs fields that large.
Each case decompresses through the fused decoder into a NaN-poisoned buffer and must equal the
oracle's reconstruction bit for bit (lrz_x.cuhip.inl:271-360 order).  Ragged y and z extents
exercise the partial bricks, whose rows past the field sit in the upper lane half; spikes give
outliers, ranked per lane half (ZigZag off) or read from the scattered field (ZigZag on).

The last case hands it a reference-format archive with a crafted deep book (crafted_books.py,
test_gpu_deep_codes.py): one brick row in 16 holds 256 codes of 27 bits, the rest 1-bit codes."""
import numpy as np
import pytest
import torch

import crafted_books as cb
import cusz_amd as cz
from archive_util import oracle_archive
from gpu_util import d2h, empty_device, sync, to_device

pytestmark = pytest.mark.gpu


def _field(dims, seed, spikes):
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
    if spikes:  # outliers: clustered in some bricks (more cells than a brick stages in LDS)
        idx = rng.choice(f.size, size=spikes, replace=False)
        f[idx] += rng.uniform(-50, 50, size=spikes).astype(np.float32)
        f[: 256 * 8 * 3] += rng.uniform(-50, 50, size=256 * 8 * 3).astype(np.float32)
    return f


@pytest.mark.parametrize("dims,zigzag,spikes", [
    ((512, 500, 196), False, 20000),  # 2 x 63 x 25 = 3150 bricks, partial in y and z
    ((512, 512, 200), True, 5000),    # 3200 bricks, full; ZigZag: outliers from the scatter
    ((768, 504, 132), False, 0),      # 3 x 63 x 17 = 3213 bricks, partial in z only
])
def test_brick32_decoder_bit_exact(oracle, dims, zigzag, spikes):
    data = _field(dims, sum(dims), spikes)
    nbricks = (dims[0] // 256) * -(-dims[1] // 8) * -(-dims[2] // 8)
    assert nbricks >= 12 * 256  # the 32-column mode (on MI355X's 256 CUs)
    eb = 1e-4
    r = cz.Resource(cz.F4, dims, cz.LorenzoZigZag if zigzag else cz.Lorenzo)
    d_in = to_device(data)
    ptr, nbytes, _ = r.compress(d_in.data_ptr(), eb)
    assert r.internals().layout == cz.LAYOUT_BRICK
    codes_o, ov_o, oi_o = oracle.lorenzo_c(data, dims, eb, 512, zigzag)
    if spikes:
        assert oi_o.size > 1000
    xo = oracle.lorenzo_x(codes_o, ov_o, oi_o, dims, eb, 512, zigzag, np.float32)
    out = empty_device(data.size, torch.float32)
    out.fill_(float("nan"))
    r.decompress(ptr, nbytes, out.data_ptr())
    sync()
    xg = out.cpu().numpy()
    bad = np.flatnonzero(xg.view(np.uint32) != xo.view(np.uint32))
    assert bad.size == 0, f"{bad.size} mismatches, first {bad[:5]}: {xg[bad[:5]]} vs {xo[bad[:5]]}"
    r.close()


def test_brick32_decoder_deep_sparse_rows(oracle):
    """deep27 x sparse16 on (512, 512, 192): 2 x 64 x 24 = 3072 bricks, the fewest the 32-column
    mode runs from.  A dense row is 6912 bits against 256 for the others, so a lane that holds one
    outruns its ring refills while its neighbours idle; the archive stays near 16 MB.  The decoded
    codes equal the input, the reconstruction the oracle's, bit for bit."""
    dims = (512, 512, 192)
    n = int(np.prod(dims))
    assert (dims[0] // 256) * (dims[1] // 8) * (dims[2] // 8) == 12 * 256
    eb = 1e-3
    b = cb.book_of("deep27")
    codes = cb.place(b, n, "sparse16", 1)
    none_v, none_i = np.zeros(0, np.float32), np.zeros(0, np.uint32)
    arch = oracle_archive(oracle, codes, none_v, none_i, dims, eb, b.book, b.revbook, sublen=256)
    assert len(arch) < 20 << 20
    want = oracle.lorenzo_x(codes, none_v, none_i, dims, eb)
    h = cz.psz_header.from_buffer_copy(arch[:176])
    r = cz.Resource(cz.F4, None, header=h)
    d_arch = to_device(np.frombuffer(arch, np.uint8).copy())
    poison = np.full(n, 0xFFFF, np.uint16)  # (kept alive across the copy)
    cz.hip_memcpy(r.internals().d_quant_codes, poison.ctypes.data, 2 * n, 1)
    del poison
    r.decode_codes(d_arch.data_ptr())
    sync()
    got = d2h(r.internals().d_quant_codes, 2 * n, np.uint16)
    bad = np.flatnonzero(got != codes)
    assert bad.size == 0, (f"{bad.size} codes differ; first at {bad[0]}: chunk {bad[0] // 256} "
                           f"({'dense' if bad[0] // 256 % 16 == 7 else 'sparse'} row)")
    del got
    out = empty_device(n, torch.float32)
    out.fill_(float("nan"))
    r.decompress(d_arch.data_ptr(), len(arch), out.data_ptr())
    sync()
    xg = out.cpu().numpy()
    badx = np.flatnonzero(xg.view(np.uint32) != want.view(np.uint32))
    assert badx.size == 0, f"{badx.size} values differ; first at {badx[0]}: chunk {badx[0] // 256}"
    r.close()
