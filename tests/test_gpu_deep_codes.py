"""Every Huffman decoder on deep and dense codes: reference-format archives whose canonical book
is crafted (crafted_books.py) rather than the shallow optimal book of a small field, so that runs
of 27-bit codes, codes just past the tables (17 bits), windows past the second table's cap and
chunks many times the average reach the decoders -- what a 512^3 field's archive can hold and a
200k-element field's own book never does.  test_crafted_books.py checks on the CPU that the
streams reach those paths.

Each case: codes from crafted_books.place (or a real field's codes under crafted_books.relabel),
the archive from archive_util.oracle_archive, want = oracle.lorenzo_x; then psz_amd_decode_codes
must return the input codes exactly, and decompress into a NaN-poisoned buffer must equal want bit
for bit.

Which kernel a row runs (hf_decode.hip launch_hf_decode, the one chooser behind decode_codes: AUTO
and sublen a multiple of 64, at most 8192 -> k_chunk_decode; else LANE (k_hf_decode_win) when
sublen % 16 == 0 and the knob says LANE or, under AUTO, pardeg >= 64 per CU; else WAVE
(k_hf_decode).  decompress: AUTO, a brick-shaped field that is not 2-D and sublen 256 -> the
fused brick decoders, whose reconstruction is then what the decompress checks):

| Kernel                  | Dims                                          | sublen          | Decoder                   |
|-------------------------|-----------------------------------------------|-----------------|---------------------------|
| k_brick3_decode<64>     | (512, 24, 17): 2 x 3 x 3 bricks, ragged z     | 256             | AUTO                      |
| k_brick3_region         | same archive; boxes: one interior brick, a box across a brick seam in all three axes, the ragged last z layer | 256 | AUTO |
| k_brick1_decode         | (16384 * 3 + 77, 1, 1)                        | 256             | AUTO                      |
| k_chunk_decode          | (300, 200, 1) and (64, 48, 40)                | 2048, 4864      | AUTO                      |
| k_hf_decode (wave)      | all of the above                              | 256, 1000, 2048 | WAVE; AUTO at sublen 1000 (no multiple of 64) |
| k_hf_decode_win (lane)  | all of the above                              | 256, 2048       | LANE                      |

(The AUTO rows' decode_codes also runs k_chunk_decode on the 3-D and 1-D brick fields.)

Every profile runs with the bands and iid patterns on every row; period3, period5 and sparse16
with deep27 and long17 (and period5 with l2over) on the 3-D fused, 1-D fused and wave rows; a real
field with outliers, relabelled anti-optimally with deep27's lengths, on the 3-D fused, region and
wave rows.  The q75 pattern (three 16-bit codes, then a 27-bit one, 75 bits a quarter) runs with
every and deep27 on every row: a long code ends a lane's quarter, so rows of nothing but long codes
move 27 bits a quarter and never outrun the ring refills of the compact decoder (64 bits a
quarter), whereas every q75 row must (test_crafted_books.py test_q75_outruns_the_ring_refills) --
the stall branch of decode_chunks4.  The fields are the smallest that still span more than one brick, a ragged brick, a
ragged last chunk and more than 64 chunks per wave unit.

On a mismatch the message names the first differing chunk and its par_nbit.
"""
import functools

import numpy as np
import pytest

import crafted_books as cb
import cusz_amd as cz
import edge_fields as ef
from archive_util import oracle_archive
from gpu_util import d2h, sync, to_device

pytestmark = pytest.mark.gpu

SEED = 1   # the seed test_crafted_books.py checks the census conditions for
EB = 1e-3
DIMS = {
    "b3": (512, 24, 17),
    "b1": (16384 * 3 + 77, 1, 1),
    "c2": (300, 200, 1),
    "c3": (64, 48, 40),
}
AUTO, LANE, WAVE = cz.DECODER_AUTO, cz.DECODER_LANE, cz.DECODER_WAVE
DEC_NAME = {AUTO: "auto", LANE: "lane", WAVE: "wave"}

# (kernel, dims, sublen, decoder)
FUSED3 = [("brick3", "b3", 256, AUTO)]
REGION = [("region", "b3", 256, AUTO)]
FUSED1 = [("brick1", "b1", 256, AUTO)]
CHUNK = [("chunk", d, s, AUTO) for d in ("c2", "c3") for s in (2048, 4864)]
WAVES = [("wave", d, s, WAVE) for d in DIMS for s in (256, 1000, 2048)] + [("wave", d, 1000, AUTO) for d in DIMS]
LANES = [("lane", d, s, LANE) for d in DIMS for s in (256, 2048)]
ALL_ROWS = FUSED3 + REGION + FUSED1 + CHUNK + WAVES + LANES

BOXES = {
    "brick": ((256, 8, 8), (256, 8, 8)),        # the interior brick (1, 1, 1) exactly
    "seam": ((250, 7, 7), (13, 10, 10)),        # across a brick seam on all three axes
    "last_z": ((0, 0, 16), (512, 24, 1)),       # the ragged last z layer (one plane thick)
}
GUARD = 4096
POISON = np.uint32(0x7FC0DEAD)


def _row_id(row):
    k, d, s, dec = row
    return f"{k}-{d}-{s}-{DEC_NAME[dec]}"


def _cases():
    out = []
    for name in cb.PROFILES:
        for pattern in ("bands", "iid"):
            out += [(name, pattern, row) for row in ALL_ROWS]
    for name, patterns in (("deep27", ("period3", "period5", "sparse16")),
                           ("long17", ("period3", "period5", "sparse16")), ("l2over", ("period5",))):
        for pattern in patterns:
            out += [(name, pattern, row) for row in FUSED3 + FUSED1 + WAVES]
    for name in cb.Q75_PROFILES:
        out += [(name, "q75", row) for row in ALL_ROWS]
    return out


CASES = _cases()


@functools.lru_cache(maxsize=None)
def _stream(oracle, name, pattern, dkey):
    """-> (book, codes, ol_val, ol_idx, want): computed once per stream, shared by its rows."""
    dims = DIMS[dkey]
    n = int(np.prod(dims))
    b = cb.book_of(name)
    codes = cb.place(b, n, pattern, SEED)
    # symbol 0 is the outlier marker: a stream that uses it (flat10) comes with a cell per zero code
    oi = np.flatnonzero(codes == 0).astype(np.uint32)
    ov = (np.random.default_rng(SEED).integers(-3000, 3000, oi.size) + 512).astype(np.float32)
    if dkey == "b3":
        order = cb.brick_order(oi, dims)
        ov, oi = ov[order], oi[order]
    want = oracle.lorenzo_x(codes, ov, oi, dims, EB)
    for a in (codes, ov, oi, want):
        a.setflags(write=False)
    return b, codes, ov, oi, want


@functools.lru_cache(maxsize=None)
def _relabelled(oracle):
    """The outlier burst field of edge_fields.py (one brick far past its slot, a handful of cells
    elsewhere) with deep27's lengths dealt anti-optimally: the commonest code takes 27 bits."""
    data, dims, eb, radius = ef.burst_field("brick")
    assert dims == DIMS["b3"] and radius == 512
    codes, ov, oi = oracle.lorenzo_c(data, dims, eb, radius)
    assert oi.size > 1000 and np.count_nonzero(codes == 0) == oi.size
    b = cb.relabel(codes, "deep27")
    assert b.lens[np.bincount(codes, minlength=1024).argmax()] == 27
    order = cb.brick_order(oi, dims)
    ov, oi = ov[order], oi[order]
    want = oracle.lorenzo_x(codes, ov, oi, dims, eb, radius)
    for a in (codes, ov, oi, want):
        a.setflags(write=False)
    return b, codes, ov, oi, want, eb


def _region(r, d_arch, nbytes, o, e):
    """Region decode into a poisoned, guarded buffer -> (box bits, guards intact)."""
    g, nb = GUARD // 4, int(np.prod(e))
    buf = to_device(np.full(2 * g + nb, POISON).view(np.float32))
    r.decompress_region(d_arch.data_ptr(), nbytes, o, e, buf.data_ptr() + GUARD)
    sync()
    bits = d2h(buf.data_ptr(), (2 * g + nb) * 4, np.uint32)
    return bits[g:g + nb], bool(np.all(bits[:g] == POISON) and np.all(bits[g + nb:] == POISON))


def _check(oracle, row, b, codes, ov, oi, want, eb):
    kernel, dkey, sublen, decoder = row
    dims = DIMS[dkey]
    n = codes.size
    arch = oracle_archive(oracle, codes, ov, oi, dims, eb, b.book, b.revbook, sublen=sublen)
    h = cz.psz_header.from_buffer_copy(arch[:176])
    r = cz.Resource(cz.F4, None, header=h)
    try:
        r.set_decoder(decoder)
        d_arch = to_device(np.frombuffer(arch, np.uint8).copy())
        # (a fresh manager's code buffer may be the block that the previous case's freed: poison it)
        poison = np.full(n, 0xFFFF, np.uint16)  # (kept alive across the copy)
        cz.hip_memcpy(r.internals().d_quant_codes, poison.ctypes.data, 2 * n, 1)
        r.decode_codes(d_arch.data_ptr())
        sync()
        got = d2h(r.internals().d_quant_codes, 2 * n, np.uint16)
        bad = np.flatnonzero(got != codes)
        if bad.size:
            c = int(bad[0]) // sublen
            nbit = oracle.hf_encode(codes, b.book, sublen)[0]
            pytest.fail(f"{bad.size} codes differ; first at {int(bad[0])} (got {int(got[bad[0]])}, want "
                        f"{int(codes[bad[0]])}): chunk {c}, symbol {int(bad[0]) - c * sublen} of it, "
                        f"par_nbit {int(nbit[c])}")
        out = to_device(np.full(n, np.nan, np.float32))
        r.decompress(d_arch.data_ptr(), len(arch), out.data_ptr())
        sync()
        full = d2h(out.data_ptr(), 4 * n, np.uint32)
        badx = np.flatnonzero(full != want.view(np.uint32))
        assert badx.size == 0, f"{badx.size} values differ; first at {int(badx[0])}: chunk {int(badx[0]) // sublen}"
        if kernel == "region":
            x, y, z = dims
            cube = full.reshape(z, y, x)
            for o, e in BOXES.values():
                box, guards = _region(r, d_arch, len(arch), o, e)
                assert r.last_region().path == cz.REGION_FUSED
                crop = cube[o[2]:o[2] + e[2], o[1]:o[1] + e[1], o[0]:o[0] + e[0]].reshape(-1)
                np.testing.assert_array_equal(box, crop)
                assert guards, "written outside the box"
    finally:
        r.close()


@pytest.mark.parametrize("name,pattern,row", CASES, ids=[f"{n}-{p}-{_row_id(r)}" for n, p, r in CASES])
def test_crafted_stream_decodes(oracle, name, pattern, row):
    b, codes, ov, oi, want = _stream(oracle, name, pattern, row[1])
    _check(oracle, row, b, codes, ov, oi, want, EB)


RELABEL_ROWS = FUSED3 + REGION + [w for w in WAVES if w[1] == "b3"]


@pytest.mark.parametrize("row", RELABEL_ROWS, ids=[_row_id(r) for r in RELABEL_ROWS])
def test_real_outliers_under_an_anti_optimal_book(oracle, row):
    """Real outlier cells (code 0 present, more than 128 of them in one brick and a few in others)
    at deep27's bit rate; Lorenzo without ZigZag, so the fused decoders rank the cells themselves."""
    b, codes, ov, oi, want, eb = _relabelled(oracle)
    _check(oracle, row, b, codes, ov, oi, want, eb)
