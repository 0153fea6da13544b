"""deep_books.py on the CPU: the two closed forms that let a test dictate an encoder's book and its
codes, checked against the oracle, and the conditions on every stream that test_gpu_deep_encode.py
relies on -- asserted on the census of the streams themselves, not measured on a GPU.

`pytest -s` prints the census: per stream and dims the lane groups above and at 64 bits and the
longest row, and for the sample-blind fields the share of wide groups.
"""
import functools

import numpy as np
import pytest

import crafted_books as cb
import deep_books as db
from edge_fields import slot_cap, spill_cap

STREAM_CASES = [(n, p, k) for k in db.DIMS for n, p in db.streams_of(k)]


@functools.lru_cache(maxsize=None)
def _census(name, pattern, dkey, sublen=db.ROW):
    b, codes, _, _, _ = db.stream(name, pattern, dkey)
    return db.encoder_census(codes, b.lens, db.DIMS[dkey], dkey in db.BRICK_KEYS, sublen)


# ---- 1. the dyadic histogram dictates the book -------------------------------------------------------
@pytest.mark.parametrize("name", list(cb.PROFILES))
def test_dyadic_histogram_gives_the_profiles_book(oracle, name):
    b = cb.book_of(name)
    h = db.dyadic_hist(b)
    assert h.size == cb.BKLEN + 1 and h[cb.BKLEN] == 0 and int(h.astype(np.int64).sum()) == 1 << cb.LMAX
    assert np.all((h[:cb.BKLEN] == 0) == (b.lens == 0))
    for builder in (lambda: oracle.book_twoqueue(h[:cb.BKLEN], cb.BKLEN, 0), lambda: oracle.codebook(h[:cb.BKLEN], cb.BKLEN)):
        book, rv = builder()
        assert book.tobytes() == b.book.tobytes()
        assert rv.tobytes() == b.revbook.tobytes()


def test_dyadic_histogram_of_the_relabelled_book(oracle):
    b = db.relabelled_stream(oracle)[0]
    h = db.dyadic_hist(b)
    for book, rv in (oracle.book_twoqueue(h[:cb.BKLEN], cb.BKLEN, 0), oracle.codebook(h[:cb.BKLEN], cb.BKLEN)):
        assert book.tobytes() == b.book.tobytes() and rv.tobytes() == b.revbook.tobytes()


# ---- 2. the field of a code stream ---------------------------------------------------------------------
def _check_field(oracle, codes, data, oi, ov, dims):
    codes_o, ov_o, oi_o = oracle.lorenzo_c(data, dims, 0.5, cb.BKLEN // 2)
    np.testing.assert_array_equal(codes_o, codes)
    np.testing.assert_array_equal(oi_o, oi)
    np.testing.assert_array_equal(ov_o.view(np.uint32), ov.view(np.uint32))
    x = oracle.lorenzo_x(codes, ov, oi, dims, 0.5, cb.BKLEN // 2, False, data.dtype.type)
    np.testing.assert_array_equal(x.view(np.uint8), data.view(np.uint8))


@pytest.mark.parametrize("name,pattern,dkey", STREAM_CASES, ids=[f"{n}-{p}-{k}" for n, p, k in STREAM_CASES])
def test_field_of_codes_is_the_oracles(oracle, name, pattern, dkey):
    b, codes, data, oi, ov = db.stream(name, pattern, dkey)
    assert np.all(b.lens[codes] > 0)
    np.testing.assert_array_equal(oi, np.flatnonzero(codes == 0))
    assert (oi.size > 0) == (name == "flat10")
    _check_field(oracle, codes, data, oi, ov, db.DIMS[dkey])


def test_field_of_codes_f64_and_relabelled(oracle):
    b, codes, data, oi, ov = db.stream("deep27", "bands", "b3", np.float64)
    assert data.dtype == np.float64
    _check_field(oracle, codes, data, oi, ov, db.DIMS["b3"])
    b, codes, data, oi, ov = db.relabelled_stream(oracle)
    _check_field(oracle, codes, data, oi, ov, db.DIMS["b3"])
    per_brick = np.bincount(_brick_of(oi, db.DIMS["b3"]))
    assert per_brick.max() > 128 and np.count_nonzero(per_brick) > 1
    assert b.lens[np.bincount(codes, minlength=cb.BKLEN).argmax()] == 27


def _brick_of(idx, dims):
    x, y, z = dims
    idx = np.asarray(idx, np.int64)
    return (idx // (x * y) // 8 * ((y + 7) // 8) + idx // x % y // 8) * (x // 256) + idx % x // 256


def test_field_of_codes_bound():
    """The worst stream stays exact in f32: a whole 1024-element tile of the largest delta."""
    codes = np.full(4096, 1023, np.uint16)
    data, _, _ = db.field_of_codes(codes, (4096, 1, 1))
    assert np.abs(data).max() == 1024 * 511 < 2 ** 21
    with pytest.raises(AssertionError):   # (a tile of outlier deltas at a radius no book has: past 2^21)
        db.field_of_codes(np.zeros(4096, np.uint16), (4096, 1, 1), radius=4096)


# ---- the census against the oracle's encoder -----------------------------------------------------------
@pytest.mark.parametrize("dkey", ["b3", "b1"])
def test_census_rows_are_the_oracles_chunks(oracle, dkey):
    b, codes, _, _, _ = db.stream("every", "iid", dkey)
    c = _census("every", "iid", dkey)
    np.testing.assert_array_equal(c["row_bits"], oracle.hf_encode(codes, b.book, 256)[0])
    assert np.all(c["wide"] + c["exact"] + c["narrow"] == 64)
    # every chunk of the field exactly once, in bricks of at most 64
    rows = np.concatenate([r for r, _ in c["bricks"]])
    np.testing.assert_array_equal(np.sort(rows), np.arange(c["row_bits"].size))


@pytest.mark.parametrize("sublen", [1024, 2048, 8192])
def test_census_chunks_are_the_oracles(oracle, sublen):
    b, codes, _, _, _ = db.stream("deep27", "sparse16", "c2")
    c = _census("deep27", "sparse16", "c2", sublen)
    np.testing.assert_array_equal(c["chunk_bits"], oracle.hf_encode(codes, b.book, sublen)[0])
    assert len(c["rounds"]) == c["chunk_bits"].size
    assert sum(r.size for r in c["rounds"]) == -(-codes.size // db.ROUND)
    assert not c["rounds"][-1][-1], "the short last round is never fast"


def test_packing_order():
    o3 = db.brick_packing_order((512, 24, 17))
    assert len(o3) == 18 and sum(f for _, f in o3) == 12
    # brick (bx 1, by 2, bz 1): first row y = 16, z = 8, then z = 9 of the same y
    rows, full = o3[(1 * 3 + 2) * 2 + 1]
    assert full and rows[0] == (8 * 24 + 16) * 2 + 1 and rows[1] == (9 * 24 + 16) * 2 + 1 and rows[8] == (8 * 24 + 17) * 2 + 1
    assert o3[-1][0].size == 8 and not o3[-1][1]   # one plane thick
    o1 = db.brick_packing_order((16384 * 3 + 77, 1, 1))
    assert [r.size for r, _ in o1] == [64, 64, 64, 1] and [f for _, f in o1] == [True, True, True, False]
    assert o1[1][0][:5].tolist() == [64, 68, 72, 76, 80] and o1[1][0][16] == 65
    o2 = db.brick_packing_order((300, 200, 1))
    assert [r.size for r, _ in o2] == [64, 64, 64, 43]


# ---- 3. what the streams do to the packers -------------------------------------------------------------
def test_print_census(capsys):
    with capsys.disabled():
        print()
        for name, pattern, dkey in STREAM_CASES:
            if dkey in db.BRICK_KEYS:
                c = _census(name, pattern, dkey)
                print(f"census {name}-{pattern}-{dkey}: groups > 64: {int(c['wide'].sum())}, == 64: {int(c['exact'].sum())}, "
                      f"of {c['wide'].size * 64}; longest row {int(c['row_bits'].max())} bits")


@pytest.mark.parametrize("dkey", ["b3", "b1", "b2"])
def test_deep27_has_a_full_length_row(dkey):
    c = _census("deep27", "bands", dkey)
    assert c["row_bits"].max() == 256 * 27 == 6912
    # ... next to the flush threshold of k_brick3_pack: a row of 216 words, kPackRowMax = 218
    assert (c["row_bits"].max() + 31) // 32 == 216


@pytest.mark.parametrize("pattern", ["bands", "iid"])
@pytest.mark.parametrize("dkey", db.BRICK_KEYS)
def test_l2full_is_the_upper_edge_of_the_fast_path(dkey, pattern):
    c = _census("l2full", pattern, dkey)
    assert c["wide"].sum() == 0
    at = c["group_pos"][c["group_bits"] == db.FAST_BITS] & 31
    assert set(at.tolist()) == set(range(32))


@pytest.mark.parametrize("name,pattern", [("long17", "bands"), ("every", "q75"), ("deep27", "q75")])
@pytest.mark.parametrize("dkey", db.BRICK_KEYS)
def test_rows_of_nothing_but_wide_groups(dkey, name, pattern):
    c = _census(name, pattern, dkey)
    full_rows = np.concatenate([r for r, full in c["bricks"] if full])
    assert np.any(c["wide"][full_rows] == 64)


@pytest.mark.parametrize("dkey", db.BRICK_KEYS)
def test_rows_switch_packers_in_every_full_brick(dkey):
    c = _census(*db.SWITCHING, dkey)
    full = [rows for rows, f in c["bricks"] if f]
    assert len(full) >= 3
    for rows in full:
        assert db.switches(c["wide"][rows] > 0) == (True, True)


@pytest.mark.parametrize("name", ["deep27", "long17"])
@pytest.mark.parametrize("dkey", db.REF_KEYS)
def test_rounds_alternate_inside_a_chunk(dkey, name):
    """sparse16: one round in four holds the dense row.  At sublen 2048 it is every chunk's second
    round (fast, then not); at 8192 a chunk holds both orders; at 1024 a chunk is one round, and
    the wave's next chunk is the other kind."""
    assert (name, "sparse16") in db.streams_of(dkey)
    c2, c8, c1 = (_census(name, "sparse16", dkey, s) for s in (2048, 8192, 1024))
    assert any(db.switches(~r)[0] for r in c2["rounds"])
    assert any(db.switches(~r) == (True, True) for r in c8["rounds"])
    kinds = np.array([bool(r[0]) for r in c1["rounds"][:-1]])
    assert kinds.any() and not kinds.all()
    # ... and the other streams' full rounds are all of one kind: never fast, or always
    for other in (("deep27", "bands"), ("every", "iid"), ("every", "q75")):
        assert not any(r.any() for r in _census(*other, dkey, 2048)["rounds"])
    assert all(r[:-1].all() for r in _census("l2full", "bands", dkey, 2048)["rounds"])


def test_archive_near_the_capacity():
    """deep27 q75 and bands run the archive at 18 to 19 bits an element; the capacity is 27."""
    for pattern in ("q75", "bands"):
        c = _census("deep27", pattern, "b3")
        assert c["row_bits"].sum() / (c["row_bits"].size * 256) > 18


# ---- the sample-blind fields ----------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["bricks", "units"])
def test_blind_field(oracle, scheme, capsys):
    data, codes, book, rv = db.blind_case(oracle, scheme)
    dims = db.BLIND_DIMS
    x, y, z = dims
    seen, unseen = db.blind_symbols(scheme)
    hist = oracle.sample_histogram(codes, dims, cb.BKLEN, scheme)
    assert np.all(hist[unseen] == 0) and np.all(hist[seen] > 0) and codes.min() >= 1
    sampled = db.sample_mask(oracle, dims, scheme)
    np.testing.assert_array_equal(np.bincount(codes.reshape(z, y, x)[sampled], minlength=cb.BKLEN), hist)
    share = sampled.mean()
    assert share < 1 and (scheme, round(1 / share)) in (("bricks", 3), ("units", 16)), "the mode really samples"
    lens = (book >> 27).astype(np.int64)
    assert np.all(book != 0xFFFFFFFF), "sample + 1: every symbol has a code"
    assert lens[unseen].min() >= 17 and lens[unseen].min() == {"bricks": 23, "units": 19}[scheme]
    c = db.encoder_census(codes, lens, dims, True)
    wide_share = c["wide"].sum() / c["wide"].size / 64
    assert wide_share >= 0.25
    bricks_sampled = sampled[::8, ::8, ::256].reshape(-1)   # one element per brick, in brick order
    assert any(full and not bricks_sampled[i] and np.all(c["wide"][rows] > 0) for i, (rows, full) in enumerate(c["bricks"]))
    assert any(db.switches(c["wide"][rows] > 0) == (True, True) for rows, _ in c["bricks"])
    assert 0 < spill_cap(codes.size) and 0 < slot_cap()   # (no code 0: no outlier at all)
    codes_o, ov_o, oi_o = oracle.lorenzo_c(data, dims, 0.5, cb.BKLEN // 2)
    np.testing.assert_array_equal(codes_o, codes)
    assert oi_o.size == 0
    with capsys.disabled():
        print(f"\nblind {scheme}: unseen symbols {int(lens[unseen].min())} bits, groups > 64: {wide_share:.1%}, longest row "
              f"{int(c['row_bits'].max())} bits, {c['row_bits'].sum() / codes.size:.1f} bits a code")
