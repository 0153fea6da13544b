"""The reference method of test_gpu_huge.py (huge_fields.py), proved on the CPU at a size the oracle
takes whole: codes, outlier cells and reconstruction assembled from one oracle run per block (per
pair of blocks for spline) equal the oracle's on the whole field; the offsets a 32-bit slip would
produce are no whole number of blocks and move most elements onto another block; the reference
alone keeps the error bound on every block; the noisy case's bitstream lies past 2^31 bytes.
"""
import dataclasses

import numpy as np
import pytest

import huge_fields as hf

# one per predictor, dimensionality, type and mode used by the GPU tests
SMALL = ["f64_4g", "f32_2g", "f32_2g-zigzag", "ref3d", "1d", "2d_under", "2d_over", "spline_over", "noisy", "rel"]


def case_of(name):
    base, _, variant = name.partition("-")
    c = hf.CASES[base]
    return dataclasses.replace(c, zigzag=True) if variant == "zigzag" else c


@pytest.mark.parametrize("name", SMALL)
def test_assembly_equals_the_whole_field_oracle(oracle, name):
    c = case_of(name).small(5)
    exp = hf.expected(c, oracle)
    seq = hf.sequence(c)
    assert len(set(seq.tolist())) >= 2
    ids = exp.ids(seq)
    data = hf.assemble(exp.alphabet, exp.tail, seq)
    assert data.size == c.n and data.dtype == c.dtype
    if c.spline:
        codes, anchors, ov, oi = oracle.spline3_c(data, c.dims, exp.eb, c.radius)
        recon = oracle.spline3_x(codes, anchors, ov, oi, c.dims, exp.eb, c.radius)
        np.testing.assert_array_equal(hf.assemble(exp.anchors, exp.anchors_tail, ids).view(np.uint8),
                                      anchors.view(np.uint8))
    else:
        codes, ov, oi = oracle.lorenzo_c(data, c.dims, exp.eb, c.radius, c.zigzag)
        recon = oracle.lorenzo_x(codes, ov, oi, c.dims, exp.eb, c.radius, c.zigzag, dtype=c.dtype)
    np.testing.assert_array_equal(hf.assemble(exp.codes, exp.codes_tail, ids), codes)
    bits = np.uint32 if c.dtype == np.float32 else np.uint64
    np.testing.assert_array_equal(hf.assemble(exp.recon, exp.recon_tail, ids).view(bits), recon.view(bits))
    idx, val = hf.assemble_cells(exp, seq)
    idx_o, val_o = hf.sort_cells(oi, ov)
    np.testing.assert_array_equal(idx, idx_o)
    np.testing.assert_array_equal(val, val_o)
    # every block has outliers: the huge field's last blocks carry them past element 2^31
    assert all(len(cells[1]) > 0 for cells in exp.cells) and len(exp.cells_tail[1]) > 0


@pytest.mark.parametrize("name", SMALL)
def test_the_reference_alone_keeps_the_bound_on_every_block(oracle, name):
    c = case_of(name)
    exp = hf.expected(c, oracle)
    k = c.k
    src = [i // k if i < k * k else i - k * k for i in range(len(exp.recon))] if c.spline else range(k)
    for i, s in enumerate(src):
        err = np.abs(exp.recon[i].astype(np.float64) - exp.alphabet[s].astype(np.float64)).max()
        assert err <= 1.001 * exp.eb, (i, err / exp.eb)
    err = np.abs(exp.recon_tail.astype(np.float64) - exp.tail.astype(np.float64)).max()
    assert err <= 1.001 * exp.eb, err / exp.eb


@pytest.mark.parametrize("name", list(hf.CASES))
def test_shifts_are_no_whole_blocks_and_the_sequence_is_not_periodic(name):
    c = hf.CASES[name]
    seq = hf.sequence(c)
    alphabet, _ = hf.blocks(c)
    for i in range(c.k):
        for j in range(i):  # distinct nearly everywhere, not in a few elements
            assert np.count_nonzero(alphabet[i] != alphabet[j]) > 0.99 * c.block_elems
    inside = 0
    for s in c.shifts():
        assert s % c.block_elems != 0, s
        d = hf.shift_differs(c, seq, s)
        if d is not None:  # (a shift beyond the field cannot land in it)
            inside += 1
            assert d > 0.4, (s, d)
    # the shapes reach the marks they are there for
    marks = {"f64_4g": 2, "f32_2g": 3, "ref3d": 1, "1d": 3, "2d_under": 0, "2d_over": 1, "spline_over": 3,
             "spline_under": 2, "noisy": 3, "rel": 3}
    assert inside == marks[name]


def test_sizes_sit_on_the_edges_they_are_for():
    c = hf.CASES
    assert 2 ** 32 < c["f64_4g"].n * 8 < 2 ** 32 + 2 ** 25 and c["f64_4g"].n > 2 ** 29
    assert 2 ** 31 < c["f32_2g"].n < 2 ** 31 + 2 ** 21 and c["f32_2g"].n * 4 > 2 ** 33
    assert c["f32_2g"].reps * c["f32_2g"].block_elems >= 2 ** 31, "the tail lies wholly past element 2^31"
    assert c["ref3d"].dims[0] % 256 != 0 and 2 ** 31 < c["ref3d"].n * 4 < 2 ** 31 + 2 ** 23
    assert c["1d"].n == 2 ** 31 + 3 * 16384 + 77 and c["1d"].n % 256 != 0
    assert c["2d_under"].dims == (4096, 131071, 1) and c["2d_under"].n * 4 == 2 ** 31 - 16384
    assert 2 ** 31 < c["2d_over"].n * 8 < 2 ** 31 + 2 ** 22
    assert 2 ** 31 < c["spline_over"].n < 2 ** 31 + 2 ** 21
    assert 2 ** 31 - 2 ** 18 <= c["spline_under"].n < 2 ** 31
    for name in c:
        assert c[name].n < 2 ** 32 and c[name].tail % 8 != 0
    assert c["1d"].block % 16384 == 0 and c["2d_under"].block % 32 == 0 and c["f32_2g"].block % 8 == 0


def test_the_noisy_field_costs_more_than_two_gib_of_bitstream(oracle):
    """Bits of every block under the oracle's book of the whole field's histogram, times R: well
    inside (2^31, 2^32) bytes, so the archive's own book and chunk padding cannot move it out."""
    c = hf.CASES["noisy"]
    exp = hf.expected(c, oracle)
    bits, hist = hf.bit_cost(exp, hf.sequence(c), oracle)
    assert hist.sum() == c.n
    assert 1.12 * 2 ** 31 < bits / 8 < 0.8 * 2 ** 32, bits / 8
    assert hist[0] < c.n // 20  # outliers stay far below the 10 % slots


def test_rel_extremes_sit_in_the_first_block_and_the_tail(oracle):
    c = hf.CASES["rel"]
    alphabet, tail = hf.blocks(c)
    seq = hf.sequence(c)
    assert seq[0] == 0 and alphabet[0].min() == hf.REL_LO and tail.max() == hf.REL_HI
    assert alphabet.max() < hf.REL_HI and tail.min() > hf.REL_LO and alphabet[1:].min() > hf.REL_LO
    assert hf.value_range(c, alphabet, tail) == (hf.REL_LO, hf.REL_HI)
    assert hf.abs_eb(c, alphabet, tail) == c.eb * (hf.REL_HI - hf.REL_LO)
