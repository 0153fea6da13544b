"""Every Huffman encoder on deep and dense codebooks.  The books that the suite's small fields
produce are shallow (longest code 19 bits, no lane whose four codewords pass 64 bits), so the
encoders' general packer, the switch between it and the fast one, rows next to the flush threshold
and archives near the capacity never ran.  Here the book is dictated and the codes are placed:

  compress_scan(field) ; compress_finish(dyadic histogram)

where the field is deep_books.field_of_codes of a crafted_books.place stream (its Lorenzo codes at
eb = 0.5 are the stream, in closed form) and the histogram is deep_books.dyadic_hist of the
profile's book, from which both codebook builders -- the device book (default) and the host heap
(CODEBOOK_EXACT) -- return that book word for word.  test_deep_books.py checks both facts and what
each stream does to the packers on the CPU.

| Encoder                                        | Dims                                   | Knobs                                  |
|------------------------------------------------|----------------------------------------|----------------------------------------|
| k_brick_plan + k_brick3_pack<4, 3>             | b3 (512, 24, 17): 2 x 3 x 3 bricks, ragged z | default; f32, deep27-bands also f64 |
| k_brick3_pack<4, 1>                            | b1 (16384 * 3 + 77, 1, 1): ragged last brick, short last chunk | default      |
| the same on 2-D linear bricks                  | b2 (300, 200, 1)                       | LAYOUT_BRICK_FORCE                     |
| k_hf_pack -> k_hf_tile_sums -> k_hf_gather     | c2 (300, 200, 1), c3 (64, 48, 40)      | LAYOUT_REFERENCE; sublen 256 (4 codes a lane: pack_words only), 512, 1024 (the first with full rounds), 2048, 8192, the tuned default |
| k_brick3_scan's sample + k_brick3_pack; k_brick3_sample + k_brick3_stream | 768 x 128 x 128: the sample-blind fields | CODEBOOK_SAMPLED; CODEBOOK_STREAM |

bands, iid and sparse16 (deep27, long17) run on every row, q75 with every and deep27, period3 and
period5 with deep27 and long17 on the brick rows; flat10 brings code-0 cells; the relabelled burst
field (more than 128 cells in one brick, the commonest code 27 bits long) runs on b3.  One stream
per row also runs under CODEBOOK_EXACT.

Each case asserts: PSZ_SUCCESS; the archive within the manager's capacity; the histogram pass 1
exported; the outlier cells equal to the closed form (3-D bricks: in brick order); the Huffman
segment against archive_util.oracle_archive with the profile's book -- reference layout byte for
byte, brick layouts revbook, par_nbit, every chunk's cells, zero gaps and the totals
(gpu_util.check_phf_against_oracle); and the field decompressed into a NaN-poisoned buffer by a
manager made from the header, bit for bit the input.  A mismatch names the first differing chunk,
its par_nbit and the census of its row.

The refusal: a caller's histogram with a zero bin where the slab's own is nonzero makes
psz_amd_compress_finish return PSZ_AMD_ERR_INVALID_ARG with no archive (the book of such a
histogram has no codeword for a symbol the slab uses); a zero bin for an unused symbol is accepted.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import crafted_books as cb
import cusz_amd as cz
import deep_books as db
from archive_util import oracle_archive
from cusz_amd import datagen
from gpu_util import check_phf_against_oracle, chunk_cells, d2h, parse_archive, to_device
from test_gpu_lattice import _decompress
from test_gpu_sampled import sampled_roundtrip

pytestmark = pytest.mark.gpu

RADIUS = cb.BKLEN // 2
BRICK, REF, FORCE = cz.LAYOUT_BRICK, cz.LAYOUT_REFERENCE, cz.LAYOUT_BRICK_FORCE
# (dims key, layout to set, sublen to set)
BRICK_ROWS = [("b3", None, None), ("b1", None, None), ("b2", FORCE, None)]
REF_ROWS = [(k, REF, s) for k in db.REF_KEYS for s in db.REF_SUBLENS]
ROWS = BRICK_ROWS + REF_ROWS
MODE_NAME = {None: "device", cz.CODEBOOK_EXACT: "exact"}


def _row_id(row):
    k, _, s = row
    return k if k in db.BRICK_KEYS else f"{k}-{s or 'tuned'}"


def _cases():
    out = [(n, p, row, None) for row in ROWS for n, p in db.streams_of(row[0])]
    out += [(*db.EXACT_STREAM, row, cz.CODEBOOK_EXACT) for row in ROWS]
    return out


CASES = _cases()
assert all(s in db.streams_of(r[0]) for s in (db.SWITCHING, db.EXACT_STREAM) for r in ROWS)


def _manager(row, dtype=np.float32, codebook=None):
    dkey, layout, sublen = row
    r = cz.Resource(cz.F4 if dtype == np.float32 else cz.F8, db.DIMS[dkey])
    if layout is not None:
        r.set_layout(layout)
    if sublen is not None:
        r.set_sublen(sublen)
    if codebook is not None:
        r.set_codebook(codebook)
    return r


def _dev(a):
    return to_device(np.array(a))   # (a copy: the streams are cached read-only)


def _hist_dev(h):
    assert h.size == cb.BKLEN + 1 and h.dtype == np.uint32
    return to_device(h.view(np.int32))


def _scan_finish(r, d_in, d_hist, codes, may_grow=False):
    """compress_scan, then compress_finish with the caller's histogram -> the archive's bytes.
    may_grow: a brick past its outlier slot warns once and the repeat succeeds (cusz_amd.h)."""
    own = torch.full((cb.BKLEN + 1,), -1, dtype=torch.int32, device="cuda")
    for _ in range(3 if may_grow else 1):
        r.compress_scan(d_in.data_ptr(), 0.5, own.data_ptr(), radius=RADIUS)
        try:
            ptr, nbytes, st = r.compress_finish(d_hist.data_ptr())
        except cz.PszError as e:
            if not (may_grow and e.status == cz.PSZ_WARN_OUTLIER_TOO_MANY):
                raise
            continue
        assert st == cz.PSZ_SUCCESS
        got = own.cpu().numpy().view(np.uint32)
        np.testing.assert_array_equal(got[:cb.BKLEN], np.bincount(codes, minlength=cb.BKLEN))
        assert r.header.entry[5] == nbytes <= r.internals().archive_capacity
        return d2h(ptr, nbytes).tobytes()
    pytest.fail("the compress kept warning")


def _first_chunk_mismatch(a, want, codes, lens, dims, brick):
    """None, or a message naming the first chunk whose bit count or cells differ."""
    s = a["sublen"]
    c = None
    bad = np.flatnonzero(a["par_nbit"] != want["par_nbit"]) if a["par_nbit"].size == want["par_nbit"].size else np.array([0])
    if bad.size:
        c, what = int(bad[0]), "par_nbit"
    else:
        ours, _ = chunk_cells(a["par_nbit"], a["par_entry"], a["bitstream"])
        ref, _ = chunk_cells(want["par_nbit"], want["par_entry"], want["bitstream"])
        badc = np.flatnonzero(ours != ref)
        if badc.size:
            ends = np.cumsum((want["par_nbit"].astype(np.int64) + 31) >> 5)
            c, what = int(np.searchsorted(ends, badc[0], side="right")), f"{badc.size} cells, first at cell {int(badc[0])}"
    if c is None:
        return None
    census = db.encoder_census(codes, lens, dims, brick, s if not brick else db.ROW)
    return (f"chunk {c} of {s} codes differs ({what}): par_nbit {int(a['par_nbit'][min(c, a['par_nbit'].size - 1)])}, want "
            f"{int(want['par_nbit'][c])}; its first row: {db.census_line(census, c * s // db.ROW)}")


def _check_archive(oracle, arch, row, book, rv, lens, codes, data, oi, ov, layout):
    dkey, _, sublen = row
    dims, n = db.DIMS[dkey], codes.size
    a = parse_archive(arch)
    h = a["header"]
    assert a["bklen"] == cb.BKLEN and h.splen == oi.size
    assert a["sublen"] == (db.ROW if layout == BRICK else sublen or a["sublen"])
    # the outlier cells: the closed form; 3-D bricks write them in brick order
    order = cb.brick_order(oi, dims) if dkey == "b3" else np.arange(oi.size)
    got_order = np.arange(oi.size) if dkey == "b3" else np.argsort(a["ol_idx"], kind="stable")
    np.testing.assert_array_equal(a["ol_idx"][got_order], oi[order])
    np.testing.assert_array_equal(a["ol_val"][got_order].view(np.uint32), ov[order].view(np.uint32))
    # the Huffman segment: the oracle's encoding with the dictated book
    want_arch = oracle_archive(oracle, codes, ov, oi, dims, 0.5, book, rv, sublen=a["sublen"])
    want = parse_archive(want_arch)
    np.testing.assert_array_equal(a["revbook"], rv, err_msg="the codebook builder did not return the dictated book")
    msg = _first_chunk_mismatch(a, want, codes, lens, dims, layout == BRICK)
    assert msg is None, msg
    check_phf_against_oracle(a, want, want["phf"], layout)
    got = _decompress(arch, n, data.dtype.type)
    bits = np.uint32 if data.dtype == np.float32 else np.uint64
    bad = np.flatnonzero(got.view(bits) != data.view(bits))
    assert bad.size == 0, f"{bad.size} values differ from the input, first at {int(bad[0])}: chunk {int(bad[0]) // a['sublen']}"


def _encode_case(oracle, row, b, codes, data, oi, ov, codebook=None, may_grow=False):
    r = _manager(row, data.dtype.type, codebook)
    try:
        arch = _scan_finish(r, _dev(data), _hist_dev(db.dyadic_hist(b)), codes, may_grow)
        layout = r.internals().layout
        assert layout == (BRICK if row[0] in db.BRICK_KEYS else REF)
    finally:
        r.close()
    _check_archive(oracle, arch, row, b.book, b.revbook, b.lens, codes, data, oi, ov, layout)


@pytest.mark.parametrize("name,pattern,row,codebook", CASES,
                         ids=[f"{n}-{p}-{_row_id(r)}-{MODE_NAME[m]}" for n, p, r, m in CASES])
def test_crafted_stream_encodes(oracle, name, pattern, row, codebook):
    b, codes, data, oi, ov = db.stream(name, pattern, row[0])
    _encode_case(oracle, row, b, codes, data, oi, ov, codebook)


def test_deep27_bands_f64(oracle):
    b, codes, data, oi, ov = db.stream("deep27", "bands", "b3", np.float64)
    _encode_case(oracle, BRICK_ROWS[0], b, codes, data, oi, ov)


def test_real_outliers_under_an_anti_optimal_book(oracle):
    """More than 128 outlier cells in one brick (past its slot: the first compress warns and grows
    it) while the brick's rows run at 27 bits a code."""
    b, codes, data, oi, ov = db.relabelled_stream(oracle)
    _encode_case(oracle, BRICK_ROWS[0], b, codes, data, oi, ov, may_grow=True)


@pytest.mark.parametrize("mode,scheme", [(cz.CODEBOOK_SAMPLED, "bricks"), (cz.CODEBOOK_STREAM, "units")], ids=["sampled", "stream"])
def test_sample_blind_field(oracle, mode, scheme):
    """The single-process paths take no histogram: a field whose sample misses the symbols the rest
    of it is made of, so the sampled book gives them 23 (19) bits and most lanes pass 64 bits."""
    data, codes, book, rv = db.blind_case(oracle, scheme)
    arch = sampled_roundtrip(oracle, np.array(data), db.BLIND_DIMS, np.float32, 0.5, False, RADIUS, mode)
    a = parse_archive(arch)
    np.testing.assert_array_equal(a["revbook"], rv)
    assert a["total_nbit"] == int((book >> 27).astype(np.int64)[codes].sum()) and a["header"].splen == 0


# ---- the refusal -------------------------------------------------------------------------------------------
REFUSAL_ROWS = [BRICK_ROWS[0], ("c3", REF, 2048)]
SENTINEL_PTR, SENTINEL_LEN = 0xDEAD0, 12345


def _finish_raw(r, d_hist):
    """psz_amd_compress_finish with sentinels in the outputs -> (status, pointer, length)."""
    out, nbytes = C.c_void_p(SENTINEL_PTR), C.c_size_t(SENTINEL_LEN)
    st = cz.lib().psz_amd_compress_finish(r._h, C.c_void_p(d_hist.data_ptr()), C.byref(r.header), C.byref(out), C.byref(nbytes))
    return st, out.value, nbytes.value


@pytest.mark.parametrize("codebook", [None, cz.CODEBOOK_EXACT], ids=["device", "exact"])
@pytest.mark.parametrize("row", REFUSAL_ROWS, ids=_row_id)
def test_a_histogram_without_a_used_bin_is_refused(oracle, row, codebook):
    b, codes, data, oi, ov = db.stream("every", "iid", row[0])
    good = db.dyadic_hist(b)
    rare = int(b.longest[0])
    assert 0 < np.count_nonzero(codes == rare) < 10_000 and good[rare] == 1
    bad = good.copy()
    bad[rare] = 0
    r = _manager(row, codebook=codebook)
    try:
        d_in = _dev(data)
        own = torch.zeros(cb.BKLEN + 1, dtype=torch.int32, device="cuda")
        r.compress_scan(d_in.data_ptr(), 0.5, own.data_ptr(), radius=RADIUS)
        st, ptr, nbytes = _finish_raw(r, _hist_dev(bad))
        assert st == cz.PSZ_AMD_ERR_INVALID_ARG
        assert (ptr, nbytes) == (SENTINEL_PTR, SENTINEL_LEN), "no archive is handed out"
        st, ptr, nbytes = _finish_raw(r, _hist_dev(good))
        assert st == cz.PSZ_AMD_ERR_STATE and ptr == SENTINEL_PTR, "the refusal consumed the scan"
        # the manager is usable: the true histogram gives the usual archive
        arch = _scan_finish(r, d_in, _hist_dev(good), codes)
        layout = r.internals().layout
    finally:
        r.close()
    _check_archive(oracle, arch, row, b.book, b.revbook, b.lens, codes, data, oi, ov, layout)


@pytest.mark.parametrize("codebook", [None, cz.CODEBOOK_EXACT], ids=["device", "exact"])
@pytest.mark.parametrize("row", REFUSAL_ROWS, ids=_row_id)
def test_a_histogram_without_an_unused_bin_is_accepted(oracle, row, codebook):
    """Any relation but "zero where the slab counted" is allowed: counts smaller than the slab's own
    (every dyadic histogram here), and a zero bin for a symbol the slab does not use."""
    b, codes, _, _, _ = db.stream("every", "iid", row[0])
    gone, other = int(b.longest[0]), int(b.longest[1])
    codes = np.where(codes == gone, other, codes).astype(np.uint16)
    data, oi, ov = db.field_of_codes(codes, db.DIMS[row[0]])
    hist = db.dyadic_hist(b)
    hist[gone] = 0
    build = oracle.codebook if codebook == cz.CODEBOOK_EXACT else lambda h, n: oracle.book_twoqueue(h, n, 0)
    book, rv = build(hist[:cb.BKLEN], cb.BKLEN)
    lens = np.where(book == 0xFFFFFFFF, 0, book >> 27).astype(np.uint8)
    assert lens[gone] == 0 and np.all(lens[codes] > 0)
    r = _manager(row, codebook=codebook)
    try:
        arch = _scan_finish(r, to_device(data), _hist_dev(hist), codes)
        layout = r.internals().layout
    finally:
        r.close()
    _check_archive(oracle, arch, row, book, rv, lens, codes, data, oi, ov, layout)


def test_spline_is_checked_and_fzg_exempt():
    """Spline builds its book from the same histogram and goes through the check; FZG builds no
    book (of the caller's histogram only the overflow word counts) and is exempt."""
    dims = (64, 32, 24)
    data = datagen.smooth3d_np(dims, 11)
    d_in = to_device(data)
    for predictor, codec, refused in ((cz.Spline, cz.Huffman, True), (cz.Lorenzo, cz.FZCodec, False)):
        r = cz.Resource(cz.F4, dims, predictor, codec=codec)
        try:
            own = torch.zeros(cb.BKLEN + 1, dtype=torch.int32, device="cuda")
            r.compress_scan(d_in.data_ptr(), 1e-3, own.data_ptr(), radius=RADIUS)
            h = own.cpu().numpy().view(np.uint32).copy()
            assert h[cb.BKLEN] == 0
            bad = h.copy()
            bad[np.flatnonzero(h[:cb.BKLEN])[0]] = 0
            st, ptr, nbytes = _finish_raw(r, _hist_dev(bad))
            if refused:
                assert st == cz.PSZ_AMD_ERR_INVALID_ARG and ptr == SENTINEL_PTR
                r.compress_scan(d_in.data_ptr(), 1e-3, own.data_ptr(), radius=RADIUS)
                st, ptr, nbytes = _finish_raw(r, _hist_dev(h))
            assert st == cz.PSZ_SUCCESS and ptr != SENTINEL_PTR
            arch = d2h(ptr, nbytes).tobytes()
        finally:
            r.close()
        got = _decompress(arch, data.size, np.float32)
        assert float(np.abs(got.astype(np.float64) - data).max()) <= 1.001e-3
