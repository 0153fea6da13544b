"""The crafted books and streams of crafted_books.py, checked on the CPU against the oracle: the
canonisation is the oracle's byte for byte, every profile is a complete code of at most 27 bits,
every profile x pattern stream survives the oracle's own encode -> decode, and the streams reach
the decoder paths that test_gpu_deep_codes.py decodes them for (conditions on the oracle's own
output, not measurements)."""
import functools

import numpy as np
import pytest

import crafted_books as cb

DIMS3 = (512, 24, 17)            # the GPU cases' 3-D field: 816 brick rows
N3 = int(np.prod(DIMS3))
SEED = 1                         # the GPU cases' seed


def _fib(k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f[:k]


def _hist(kind):
    h = np.zeros(1024, np.uint32)
    i = np.arange(1024)
    if kind == "geometric":
        h[:] = np.floor(1e9 * 0.8 ** np.abs(i - 512))
    elif kind == "fib25":        # 26 Fibonacci counts: a chain of depth 25
        h[500:526] = _fib(26)
    elif kind == "limit":        # 45 Fibonacci counts: depth 44, through the 27-bit limit
        h[300:345] = _fib(45)
    return h


@pytest.mark.parametrize("kind,depth", [("geometric", None), ("fib25", 25), ("limit", 27)])
def test_canon_is_the_oracles(oracle, kind, depth):
    h = _hist(kind)
    lens = oracle.huffman_lengths(h)
    if depth:
        assert lens.max() == depth
    book_o, rv_o = oracle.codebook(h)
    book, rv = cb.canon(lens)
    assert book.tobytes() == book_o.tobytes()
    assert rv.tobytes() == rv_o.tobytes()


@pytest.mark.parametrize("name", list(cb.PROFILES))
def test_profiles_are_complete(name):
    lengths = cb.PROFILES[name]
    assert max(lengths) <= cb.LMAX and min(lengths) >= 1
    assert sum(1 << (cb.LMAX - l) for l in lengths) == 1 << cb.LMAX   # Kraft sum exactly 1
    b = cb.book_of(name)
    assert sorted(b.lens[b.lens > 0].tolist()) == sorted(lengths)
    assert (b.lens[0] == 0) == (name != "flat10")
    # the book words are a prefix code: sorted left-justified, no word is a prefix of its successor
    w = b.book[b.used].astype(np.int64)
    l, c = w >> 27, w & 0x07FFFFFF
    lj = np.sort((c << (32 - l)) * 32 + l)
    v, ll = lj >> 5, lj & 31
    assert np.all(v[1:] >> (32 - ll[:-1]) != v[:-1] >> (32 - ll[:-1]))
    first, entry, keys, lens, code = cb.revbook_tables(b.revbook)
    np.testing.assert_array_equal(lens, b.lens)
    np.testing.assert_array_equal(code[b.used], c)


def test_l2over_threshold():
    first = cb.revbook_tables(cb.book_of("l2over").revbook)[0]
    assert first[12] == 256 and first[12] << 4 > max(cb.L2_CAPS)


STREAMS = [(n, p) for n in cb.PROFILES for p in cb.PATTERNS if p != "q75" or n in cb.Q75_PROFILES]


def test_q75_profiles():
    for name, lengths in cb.PROFILES.items():
        assert (name in cb.Q75_PROFILES) == (16 in lengths and max(lengths) > 16)


@pytest.mark.parametrize("sublen", [256, 1000, 2048])
@pytest.mark.parametrize("name,pattern", STREAMS)
def test_streams_round_trip_through_the_oracle(oracle, name, pattern, sublen):
    b = cb.book_of(name)
    n = 256 * 48 + 77
    codes = cb.place(name, n, pattern, SEED)
    assert np.all(b.lens[codes] > 0)
    nbit, entry, bs, tot = oracle.hf_encode(codes, b.book, sublen)
    got = oracle.hf_decode(bs, b.revbook, nbit, entry, sublen, n)
    np.testing.assert_array_equal(got, codes)
    # the census reads its windows from a stream of its own: the oracle's, cell for cell
    nbit_c, entry_c, bs_c = cb.encode_bits(codes, b.revbook, sublen)[:3]
    np.testing.assert_array_equal(nbit_c, nbit)
    np.testing.assert_array_equal(entry_c, entry)
    np.testing.assert_array_equal(bs_c, bs)
    assert tot == int(nbit.astype(np.int64).sum())


@functools.lru_cache(maxsize=None)
def _census(name, pattern, sublen=256):
    b = cb.book_of(name)
    return cb.path_census(cb.place(name, N3, pattern, SEED), b.revbook, sublen)


def test_relabel_is_anti_optimal():
    rng = np.random.default_rng(5)
    codes = np.clip(np.round(512 + 20 * rng.standard_normal(100_000)), 0, 1023).astype(np.uint16)
    codes[::1000] = 0
    b = cb.relabel(codes, "deep27")
    assert cb.kraft_is_one(b.lens[b.lens > 0])
    hist = np.bincount(codes, minlength=1024)
    used = np.flatnonzero(hist)
    assert np.all(b.lens[used] > 0)
    order = used[np.argsort(-hist[used], kind="stable")]
    assert np.all(np.diff(b.lens[order].astype(int)) <= 0)   # rarer symbols never get longer codes
    assert b.lens[order[0]] == 27
    with pytest.raises(AssertionError):
        cb.relabel(np.arange(1024, dtype=np.uint16), "deep27")


# ---- the conditions that keep the GPU cases honest -----------------------------------------------
@pytest.mark.parametrize("name", ["deep27", "long17"])
@pytest.mark.parametrize("pattern", ["bands", "sparse16"])
def test_long_words_come_in_runs(name, pattern):
    c = _census(name, pattern)
    for cap in cb.L2_CAPS:
        assert cb.longest_run(c["klass"][cap] == cb.KLASS_LONG) >= 256
    assert c["len"].max() == cb.book_of(name).max_len > cb.L2_BITS


@pytest.mark.parametrize("pattern", ["bands", "iid", "period5"])
def test_l2over_reaches_the_long_search_with_short_words(pattern):
    """Words of <= 16 bits past the second table's cap.  With 2047 usable entries that is the upper
    half of the 13-bit codes; with 4095 only index 4095 itself is left out (the last slot stays
    0): the highest 13-bit code followed by three 1 bits, which an iid stream does not hold (a
    chance of 516^-4 per word) -- period5 does by construction, bands at a row's end by its seed."""
    c = _census("l2over", pattern)
    assert c["len"].max() == 13
    for cap in cb.L2_CAPS if pattern != "iid" else (2047,):
        assert np.count_nonzero(c["klass"][cap] == cb.KLASS_LONG) > 0
    assert np.count_nonzero(c["klass"][2047] == cb.KLASS_LONG) > np.count_nonzero(c["klass"][2047] == cb.KLASS_L2) // 2


@pytest.mark.parametrize("pattern", ["bands", "iid"])
def test_l2full_stays_in_the_tables(pattern):
    c = _census("l2full", pattern)
    assert c["len"].max() == 16
    for cap in cb.L2_CAPS:
        assert np.count_nonzero(c["klass"][cap] == cb.KLASS_LONG) == 0
    assert cb.longest_run(c["klass"][4095] == cb.KLASS_L2) >= 256


def test_flat10_is_first_table_only():
    c = _census("flat10", "iid")
    assert np.all(c["klass"][2047] == cb.KLASS_L1) and np.all(c["len"] == 10)


def test_every_covers_every_length_and_class():
    c = _census("every", "iid")
    assert set(np.unique(c["len"]).tolist()) == set(range(1, 28))
    for cap in cb.L2_CAPS:
        assert set(np.unique(c["klass"][cap]).tolist()) == {cb.KLASS_L1, cb.KLASS_L2, cb.KLASS_LONG}


@pytest.mark.parametrize("name", ["every", "deep27"])
def test_bands_rows_run_at_the_extreme_rates(oracle, name):
    b = cb.book_of(name)
    nbit = oracle.hf_encode(cb.place(name, N3, "bands", SEED), b.book, 256)[0]
    assert nbit.max() >= 6912 and nbit.min() == 256


@pytest.mark.parametrize("name", ["deep27", "long17"])
def test_sparse16_has_a_chunk_far_above_the_average(oracle, name):
    """deep27: the dense row is more than ten times the mean.  Both profiles: it is past the wave
    decoder's LDS staging (1.5 x the average chunk's cells + 64, rounded up to 16 cells:
    hf_decode.hip launch_hf_decode), so that decoder reads it from global memory."""
    b = cb.book_of(name)
    nbit = oracle.hf_encode(cb.place(name, N3, "sparse16", SEED), b.book, 256)[0].astype(np.int64)
    if name == "deep27":
        assert nbit.max() > 10 * nbit.mean()
    ncell = (nbit + 31) >> 5
    avg = int(ncell.sum()) // ncell.size
    cellcap = (avg + avg // 2 + 64 + 15) // 16 * 16
    assert ncell.max() + 2 > cellcap
    # ... while the bands pattern's longest chunk still fits it
    nb = oracle.hf_encode(cb.place(name, N3, "bands", SEED), b.book, 256)[0].astype(np.int64)
    nc = (nb + 31) >> 5
    avg = int(nc.sum()) // nc.size
    assert nc.max() + 2 <= (avg + avg // 2 + 64 + 15) // 16 * 16


@pytest.mark.parametrize("pattern", ["period3", "period5"])
def test_period_patterns_put_long_words_on_every_step(pattern):
    c = _census("deep27", pattern)
    long_at = np.flatnonzero(c["len"] == 27) % 256
    assert set((long_at % 4).tolist()) == {0, 1, 2, 3}
    if pattern == "period5":
        # a code word longer than a lane's segment of the wave decoder (ceil(nbit / 64) bits):
        # several lanes' segments then hold no code word start
        seg = -(-c["par_nbit"].astype(np.int64) // 64)
        assert seg.min() < 27


@pytest.mark.parametrize("name", cb.Q75_PROFILES)
def test_q75_outruns_the_ring_refills(name):
    """Every row of a q75 stream holds more bits than a lane of the compact decoder has in its ring
    at the start plus what its refills bring in the quarters the row takes: its wave must wait
    for words (decode_chunks4's stall branch)."""
    c = _census(name, "q75")
    rows = np.arange(N3 // 256)
    quarters, bits = cb.quarter_load(c, rows)
    assert np.all(quarters == 64) and np.all(bits == 64 * 75)
    assert np.all(cb.must_stall(quarters, bits))


@pytest.mark.parametrize("name,pattern", [("deep27", "bands"), ("deep27", "sparse16"), ("long17", "bands"),
                                          ("l2full", "bands"), ("deep27", "period3")])
def test_why_q75_a_run_of_long_words_does_not(name, pattern):
    """A long word ends its quarter, so a row of nothing but 27-bit (or 17-bit) words moves 27 (17)
    bits per quarter, and a row of 16-bit words exactly the 64 that the refills bring: none of
    these rows has to wait."""
    c = _census(name, pattern)
    quarters, bits = cb.quarter_load(c, np.arange(0, N3 // 256, 5))
    assert not np.any(cb.must_stall(quarters, bits))


def test_a_wrong_long_threshold_shows(oracle):
    """Sensitivity, on the CPU: with first[17] off by one the oracle's decoder returns other codes
    for a long17 stream, and the same codes for an l2full stream (no code longer than 16 bits)."""
    out = {}
    for name in ("long17", "l2full"):
        b = cb.book_of(name)
        codes = cb.place(name, 256 * 40, "bands", SEED)
        nbit, entry, bs, _ = oracle.hf_encode(codes, b.book, 256)
        rv = b.revbook.copy()
        rv[:128].view(np.int32)[17] += 1
        got = oracle.hf_decode(bs, rv, nbit, entry, 256, codes.size)
        out[name] = bool(np.array_equal(got, codes))
    assert out == {"long17": False, "l2full": True}
