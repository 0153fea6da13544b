"""The FZG segment's numpy model (tests/fzg_model.py) against itself and against hand-computed
vectors: round trips at every unit and block edge, the symbol transform, the segment's size and its
worst case.  CPU-only; tests/test_gpu_fzg.py holds the kernels to this model byte for byte."""
import numpy as np
import pytest

import fzg_model as fm

NS = [1, 255, 256, 257, 4095, 4096, 4097, 65_537]


def _popcount(a):
    return int(np.unpackbits(np.ascontiguousarray(a).view(np.uint8)).sum())


@pytest.mark.parametrize("zigzag", [False, True])
@pytest.mark.parametrize("radius", [64, 512])
@pytest.mark.parametrize("n", NS)
def test_roundtrip_random_codes(n, radius, zigzag):
    rng = np.random.default_rng(n + radius)
    # mostly near the centre, some anywhere in the book, some outlier codes (0)
    codes = np.clip(rng.normal(radius, 3, n).round(), 0, 2 * radius - 1).astype(np.uint16)
    wide = rng.random(n) < 0.05
    codes[wide] = rng.integers(0, 2 * radius, int(wide.sum()))
    codes[rng.random(n) < 0.02] = 0
    seg = fm.encode(codes, radius, zigzag)
    np.testing.assert_array_equal(fm.decode(seg, n, radius), codes)
    s = fm.parse(seg, n)
    units, blocks = fm.counts(n)
    assert s["transform"] == (fm.PLAIN if zigzag else fm.ZIGZAG_DELTA)
    # segment size: 32 + 8 units + 4 (blocks + 1), padded to 8, + 8 popcount(flags)
    fixed = (32 + 8 * units + 4 * (blocks + 1) + 7) // 8 * 8
    assert len(seg) == fixed + 8 * _popcount(s["flags"])
    assert s["total"] == _popcount(s["flags"]) == s["block_off"][-1]
    # worst case: 2 n bytes of payload (whole units) + n / 32 of flags + n / 1024 of offsets
    npad = units * fm.UNIT
    assert len(seg) <= 2 * npad + npad // 32 + 4 * (blocks + 1) + 32 + 8


@pytest.mark.parametrize("n", NS)
def test_worst_case_is_reached_and_bounded(n):
    """Every bit of every symbol set: all 64 words of every whole unit are nonzero."""
    codes = np.full(n, 0xFFFF, np.uint16)
    seg = fm.encode(codes, 512, True)
    s = fm.parse(seg, n)
    units, blocks = fm.counts(n)
    assert s["total"] <= 64 * units
    if n % fm.UNIT == 0:
        assert s["total"] == 64 * units and 8 * s["total"] == 2 * n
    assert len(seg) <= 32 + 8 * units + 4 * (blocks + 1) + 4 + 512 * units
    np.testing.assert_array_equal(fm.decode(seg, n), codes)


@pytest.mark.parametrize("radius", [64, 512])
def test_transform_is_a_bijection_with_small_deltas_low(radius):
    codes = np.arange(2 * radius, dtype=np.uint16)
    t = fm.symbols(codes, radius, False)
    assert sorted(t.tolist()) == list(range(2 * radius))
    assert t[radius] == 0 and t[radius - 1] == 1 and t[radius + 1] == 2 and t[radius - 2] == 3
    assert t[0] == 2 * radius - 1  # the outlier code
    np.testing.assert_array_equal(fm.codes_of(t, radius, fm.ZIGZAG_DELTA), codes)
    np.testing.assert_array_equal(fm.symbols(codes, radius, True), codes)


@pytest.mark.parametrize("n", [1, 300, 4097])
def test_all_codes_at_radius_have_no_payload(n):
    seg = fm.encode(np.full(n, 512, np.uint16), 512, False)
    s = fm.parse(seg, n)
    assert s["total"] == 0 and not s["flags"].any() and not s["block_off"].any()
    assert len(seg) == fm.offsets(n)[2]


def test_symbol_one_at_index_zero():
    sym = np.zeros(256, np.uint16)
    sym[0] = 1
    s = fm.parse(fm.encode(sym, 512, True), 256)
    assert s["flags"].tolist() == [1] and s["payload"].tolist() == [1] and s["block_off"].tolist() == [0, 1]


def test_symbol_high_bit_at_index_255():
    sym = np.zeros(256, np.uint16)
    sym[255] = 0x8000
    s = fm.parse(fm.encode(sym, 512, True), 256)
    assert s["flags"].tolist() == [1 << 63] and s["payload"].tolist() == [1 << 63]


def test_outlier_code_is_the_largest_symbol():
    for radius in (64, 512):
        codes = np.full(256, radius, np.uint16)
        codes[0] = 0
        s = fm.parse(fm.encode(codes, radius, False), 256)
        # lane 0's u64 = 2 radius - 1 in its low field: words 0 .. log2(2 radius) - 1, each with bit 0
        nbits = (2 * radius - 1).bit_length()
        assert s["flags"].tolist() == [(1 << nbits) - 1] and s["payload"].tolist() == [1] * nbits


def test_block_offsets_count_words_before_each_block():
    n = 3 * fm.BLOCK + 17
    sym = np.zeros(n, np.uint16)
    sym[0] = 3                      # block 0: words 0 and 1
    sym[fm.BLOCK + 5] = 1           # block 1: lane 1, field 1 -> word 16
    sym[2 * fm.BLOCK + 256] = 7     # block 2, unit 1: words 0..2
    sym[n - 1] = 1                  # block 3 (17 symbols): lane 4, field 0 -> word 0
    seg = fm.encode(sym, 512, True)
    s = fm.parse(seg, n)
    assert s["block_off"].tolist() == [0, 2, 3, 6, 7]
    assert s["payload"].tolist() == [1, 1, 1 << 1, 1, 1, 1, 1 << 4]
    np.testing.assert_array_equal(fm.decode(seg, n), sym)
