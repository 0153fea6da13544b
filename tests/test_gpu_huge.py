"""Fields past 2 GiB and 2^31 elements: every 32-bit offset edge of the library, bit for bit.

The fields and what is expected of them come from huge_fields.py: a non-periodic sequence of a few
small blocks plus a ragged tail, assembled on the device, with the oracle run once per block
(test_huge_fields.py proves on the CPU that this equals the oracle on the whole field, and that an
offset wrapped at 2^31, 2^32 or 2^33 bytes or at 2^31 elements lands on other data).  Nothing of
field size crosses to the host: codes and reconstruction are compared on the device, block by
block, as integers, so -0.0 and NaN count; only the outlier cells (a few hundred per block), the
spline anchors and the headers are read back.

Each case names the edge it is the smallest shape for and asserts the layout (or region path) it
is there for.  A case skips only when the device has less free memory than it needs.
"""
import ctypes as C
import dataclasses
import struct

import numpy as np
import pytest
import torch

import cusz_amd as cz
import huge_fields as hf
from gpu_util import d2h, hip, sync
from test_gpu_region import region

pytestmark = pytest.mark.gpu

_expected = {}


def expected(oracle, case):
    """The oracle's per-block results, once per case (shared, never modified)."""
    key = dataclasses.replace(case, reps=0, name="")  # the alphabet does not depend on R
    if key not in _expected:
        _expected[key] = hf.expected(case, oracle)
    return dataclasses.replace(_expected[key], case=case)


def need_memory(case):
    """Field, output and a copy of the codes; the manager's codes, byte codes, slots, spill list and
    an archive sized n * 27 / 8; comparison temporaries.  Skips when the device has less free."""
    need = case.n * (2 * case.itemsize + 2 + 10) + (4 << 30)
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f"needs {need} bytes of device memory, {free} are free")


def codes_tensor(r, n):
    """The manager's quant codes (index order) as a device tensor."""
    t = torch.empty(n, dtype=torch.int16, device="cuda")
    sync()
    assert hip().hipMemcpy(C.c_void_p(t.data_ptr()), C.c_void_p(r.internals().d_quant_codes), 2 * n, 3) == 0
    return t


def archive_parts(ptr, nbytes):
    """Header, Huffman header fields and outlier cells of a device archive (the bitstream stays put)."""
    h = cz.psz_header.from_buffer_copy(d2h(ptr, 176).tobytes())
    assert h.entry[5] == nbytes
    phf = d2h(ptr + h.entry[2], 64).tobytes()
    tnbit, tncell = struct.unpack_from("<QQ", phf, 24)
    pent = struct.unpack_from("<6I", phf, 40)
    cells = d2h(ptr + h.entry[3], h.entry[4] - h.entry[3], np.uint32).reshape(-1, 2)
    return h, dict(total_nbit=tnbit, total_ncell=tncell, bits_off=h.entry[2] + pent[4]), cells


def assert_equal_on_device(case, got, per_block, tail, ids, what):
    count, first = hf.mismatches(case, got, per_block, tail, ids)
    assert count == 0, f"{what}: {count} of {case.n} elements differ, the first at {first} " \
                       f"(block {first // case.block_elems} of {case.reps}, byte {first * got.element_size()})"


class Run:
    """One compress of a huge field, checked against the block-assembled oracle: layout, header,
    outlier cells, anchors, codes, histogram; then check_decompress() as often as needed."""

    r = field = None

    def compress(self, oracle, case, layout=None, codebook=None, expect_layout=cz.LAYOUT_BRICK):
        need_memory(case)
        self.case, self.exp = case, expected(oracle, case)
        self.seq = hf.sequence(case)
        self.ids = self.exp.ids(self.seq)
        self.field = hf.device_field(case, self.exp.alphabet, self.exp.tail, self.seq)
        pred = cz.Spline if case.spline else cz.LorenzoZigZag if case.zigzag else cz.Lorenzo
        self.r = r = cz.Resource(cz.F4 if case.dtype == np.float32 else cz.F8, case.dims, pred)
        if layout is not None:
            r.set_layout(layout)
        if codebook is not None:
            r.set_codebook(codebook)
        self.ptr, self.nbytes, st = r.compress(self.field.data_ptr(), case.eb, case.mode, case.radius)
        assert st == cz.PSZ_SUCCESS
        assert r.internals().layout == expect_layout
        self.brick = expect_layout == cz.LAYOUT_BRICK
        self.header, self.phf, cells = archive_parts(self.ptr, self.nbytes)
        h, exp = self.header, self.exp
        assert (h.len.x, h.len.y, h.len.z) == case.dims and h.rc.eb == exp.eb
        # outlier cells: the same set (the brick layout lists them in brick order), indices >= 2^31 included
        idx_e, val_e = hf.assemble_cells(exp, self.seq)
        assert h.splen == len(idx_e) == len(cells)
        idx_g, val_g = hf.sort_cells(cells[:, 1], cells[:, 0])
        np.testing.assert_array_equal(idx_g, idx_e)
        np.testing.assert_array_equal(val_g, val_e)
        if case.n > hf.MARK_ELEMS:
            assert idx_e[-1] >= hf.MARK_ELEMS
        if case.spline:
            got = d2h(self.ptr + h.entry[1], h.entry[2] - h.entry[1], np.uint32)
            want = hf.assemble(exp.anchors, exp.anchors_tail, self.ids).view(np.uint32)
            np.testing.assert_array_equal(got, want)
        # codes (the fused path keeps them only in the archive), histogram, splen
        if self.brick:
            r.decode_codes(self.ptr)
        codes = codes_tensor(r, case.n)
        assert_equal_on_device(case, codes, exp.codes, exp.codes_tail, self.ids, "codes")
        bklen = 2 * case.radius
        hist = hf.code_histogram(codes, bklen)
        assert hist.sum() == case.n
        if codebook != cz.CODEBOOK_STREAM:  # (the single pass counts only its sample)
            np.testing.assert_array_equal(d2h(r.internals().d_hist, 4 * bklen, np.uint32), hist)
        if not case.zigzag:  # (zigzag: code 0 is a zero delta as well as an outlier's place)
            assert h.splen == hist[0]
        else:
            assert h.splen <= hist[0]
        del codes
        return self

    def check_decode_codes(self, decoder):
        """decode_codes with one decoder into zeroed codes."""
        r, case = self.r, self.case
        r.set_decoder(decoder)
        zero = torch.zeros(1 << 26, dtype=torch.int16, device="cuda")
        base = r.internals().d_quant_codes
        for e0 in range(0, case.n, zero.numel()):
            m = min(zero.numel(), case.n - e0)
            assert hip().hipMemcpy(C.c_void_p(base + 2 * e0), C.c_void_p(zero.data_ptr()), 2 * m, 3) == 0
        r.decode_codes(self.ptr)
        codes = codes_tensor(r, case.n)
        assert_equal_on_device(case, codes, self.exp.codes, self.exp.codes_tail, self.ids, f"codes, decoder {decoder}")

    def check_decompress(self, decoder=None):
        """The whole field into a NaN-poisoned buffer: the oracle's bits, and within the bound."""
        case, exp = self.case, self.exp
        if decoder is not None:
            self.r.set_decoder(decoder)
        out = torch.full((case.n,), float("nan"), dtype=self.field.dtype, device="cuda")
        self.r.decompress(self.ptr, self.nbytes, out.data_ptr())
        sync()
        assert_equal_on_device(case, out, exp.recon, exp.recon_tail, self.ids, f"reconstruction, decoder {decoder}")
        err = hf.max_abs_err(case, out, self.field)
        assert err <= 1.001 * exp.eb, err / exp.eb

    def expected_box(self, o, e):
        """The box of the expected reconstruction (3-D), as bits."""
        case, exp = self.case, self.exp
        x, y = case.row
        planes = []
        for z in range(o[2], o[2] + e[2]):
            b, zz = divmod(z, case.block)
            src = exp.recon[self.ids[b]] if b < case.reps else exp.recon_tail
            planes.append(src.reshape(-1, y, x)[zz, o[1]:o[1] + e[1], o[0]:o[0] + e[0]])
        return np.stack(planes).reshape(-1).view(np.uint32 if case.dtype == np.float32 else np.uint64)

    def close(self):
        if self.r is not None:
            self.r.close()
        self.r = self.field = None


@pytest.fixture
def run(oracle):
    """Run(...) whose manager and tensors are freed when the test ends, however it ends."""
    made = []

    def make(case, **kw):
        made.append(Run())
        return made[-1].compress(oracle, case, **kw)
    yield make
    for a in made:
        a.close()
    torch.cuda.empty_cache()


def test_the_comparison_sees_single_elements_past_every_mark(oracle):
    """The device assembly and the blockwise comparison themselves, at full size: the assembled
    field equals its own alphabet, and one flipped sign bit of a zero, one NaN and one changed
    value -- past 2^31 elements, in the last block and in the tail -- are each counted."""
    case = hf.CASES["f32_2g"]
    need_memory(case)
    alphabet, tail = hf.blocks(case)
    seq = hf.sequence(case)
    field = hf.device_field(case, alphabet, tail, seq)
    assert hf.mismatches(case, field, alphabet, tail, seq) == (0, -1)
    # the blocks sit where the sequence says: first element of a few blocks around the marks
    be = case.block_elems
    for b in (0, 1, 2 ** 29 // be, 2 ** 30 // be, 2 ** 31 // be, case.reps - 1):
        assert field[b * be].item() == alphabet[seq[b], 0] and field[b * be + be - 1].item() == alphabet[seq[b], -1]
    assert field[case.n - 1].item() == tail[-1]
    spots = [2 ** 31 + 5, case.reps * be - 1, case.n - 3]
    field[spots[0]] = 0.0
    assert hf.mismatches(case, field, alphabet, tail, seq) == (1, spots[0])
    want = alphabet.copy()
    want[seq[spots[0] // be], spots[0] % be] = -0.0   # equal as floats, not as bits
    want_tail = tail.copy()
    want_tail[-3] = np.nan
    field[spots[2]] = float("nan")                      # equal as bits, not as floats
    others = np.flatnonzero(seq == seq[spots[0] // be]).size - 1  # the block's other places show -0.0 too
    count, first = hf.mismatches(case, field, want, want_tail, seq)
    assert count == 1 + others and first <= spots[0]
    field[spots[1]] += 1.0
    assert hf.mismatches(case, field, alphabet, tail, seq)[0] == 3
    del field
    torch.cuda.empty_cache()


VARIANTS = [(False, cz.CODEBOOK_SAMPLED), (True, cz.CODEBOOK_STREAM)]
VARIANT_IDS = ["plain-sampled", "zigzag-stream"]


@pytest.mark.parametrize("zigzag,codebook", VARIANTS, ids=VARIANT_IDS)
def test_f64_bricks_past_4_gib(run, zigzag, codebook):
    """(256, 256, 8213) f64: input and output cross the 2^31- and 2^32-byte marks."""
    case = dataclasses.replace(hf.CASES["f64_4g"], zigzag=zigzag)
    assert case.n * 8 > 2 ** 32
    run(case, codebook=codebook).check_decompress()


@pytest.mark.parametrize("zigzag,codebook", [(False, cz.CODEBOOK_STREAM), (True, cz.CODEBOOK_SAMPLED)],
                         ids=["plain-stream", "zigzag-sampled"])
def test_f32_bricks_past_2g_elements(run, zigzag, codebook):
    """(256, 256, 32789) f32: bytes past 2^33, element and outlier indices from 2^31 up."""
    case = dataclasses.replace(hf.CASES["f32_2g"], zigzag=zigzag)
    assert case.n > 2 ** 31
    a = run(case, codebook=codebook)
    a.check_decompress()
    for decoder in (cz.DECODER_LANE, cz.DECODER_WAVE):  # the generic decoders write codes past element 2^31 too
        a.check_decode_codes(decoder)


# origin, extent: wholly past element 2^31 (plane 32768), across the last block's border into the
# ragged tail; and across the 2^32-byte mark (plane 16384)
REGION_BOXES = {"past_2g_elements": ((37, 51, 32770), (150, 90, 17)), "across_4_gib": ((3, 5, 16380), (250, 200, 9))}


def test_f32_region_decodes_past_2g_elements(run):
    case = hf.CASES["f32_2g"]
    a = run(case)
    arch = torch.empty(a.nbytes, dtype=torch.uint8, device="cuda")  # (the manager reuses its own buffer)
    assert hip().hipMemcpy(C.c_void_p(arch.data_ptr()), C.c_void_p(a.ptr), a.nbytes, 3) == 0
    plane = case.unit
    for name, (o, e) in REGION_BOXES.items():
        first, last = o[2] * plane, (o[2] + e[2]) * plane
        assert first >= 2 ** 31 if name == "past_2g_elements" else first * 4 < 2 ** 32 < last * 4
        got, guards = region(a.r, arch, a.nbytes, o, e, case.dtype)
        info = a.r.last_region()
        np.testing.assert_array_equal(got, a.expected_box(o, e), err_msg=name)
        assert guards, "written outside the box"
        assert info.path == cz.REGION_FUSED and info.elems == int(np.prod(e))


def test_f32_reference_layout_past_2_gib(run):
    """250 x 256 planes (x no multiple of 256): the Lorenzo kernels of the reference layout and the
    generic Huffman encoder, every decoder, at byte offsets past 2^31."""
    case = hf.CASES["ref3d"]
    assert case.n * 4 > 2 ** 31
    a = run(case, expect_layout=cz.LAYOUT_REFERENCE)
    for decoder in (cz.DECODER_LANE, cz.DECODER_WAVE, cz.DECODER_AUTO):
        a.check_decode_codes(decoder)
        a.check_decompress(decoder)


@pytest.mark.parametrize("layout", [cz.LAYOUT_BRICK, cz.LAYOUT_REFERENCE], ids=["brick", "reference"])
def test_1d_past_2g_elements(run, layout):
    """n = 2^31 + 3 * 16384 + 77: the blocks around element 2^31 and the ragged tail among all."""
    case = hf.CASES["1d"]
    run(case, layout=layout, expect_layout=layout).check_decompress()


def test_2d_just_under_the_brick_limit(run):
    """(4096, 131071) f32, 16 KiB under 2^31 bytes: linear bricks."""
    case = hf.CASES["2d_under"]
    run(case, layout=cz.LAYOUT_BRICK_FORCE, expect_layout=cz.LAYOUT_BRICK).check_decompress()


def test_2d_just_over_the_brick_limit(run):
    """(4096, 65599) f64, 2 MB over 2 GiB: the reference layout, whatever is asked for, and exact."""
    case = hf.CASES["2d_over"]
    run(case, layout=cz.LAYOUT_BRICK_FORCE, expect_layout=cz.LAYOUT_REFERENCE).check_decompress()


@pytest.mark.parametrize("dtype,dims", [
    (cz.F4, (2 ** 29, 4, 1)), (cz.F8, (2 ** 28, 3, 1)),                     # a 2-D row of 2 GiB
    (cz.F4, (2 ** 32, 1, 1)), (cz.F4, (2048, 2048, 1024)), (cz.F8, (2 ** 16, 2 ** 16, 1)),  # n = 2^32
], ids=["row-f32", "row-f64", "n-1d", "n-3d", "n-2d"])
def test_unsupported_sizes_fail_at_creation_without_allocating(dtype, dims):
    torch.cuda.init()
    sync()
    before = torch.cuda.mem_get_info()[0]
    with pytest.raises(cz.PszError) as ei:
        cz.Resource(dtype, dims)
    assert ei.value.status == cz.PSZ_ABORT_UNSUPPORTED_DIMENSION
    assert torch.cuda.mem_get_info()[0] == before


@pytest.mark.parametrize("name", ["spline_over", "spline_under"])
def test_spline_on_both_sides_of_2g_elements(run, name):
    """X * Y * Z just past 2^31 (the index path without magic divisions) and just below it."""
    case = hf.CASES[name]
    assert (case.n >= 2 ** 31) == (name == "spline_over")
    run(case, expect_layout=cz.LAYOUT_REFERENCE).check_decompress()


def test_bitstream_past_2_gib(run):
    """Noisy blocks: the Huffman bitstream itself ends between 2^31 and 2^32 bytes into the archive."""
    a = run(hf.CASES["noisy"])
    end = a.phf["bits_off"] + 4 * a.phf["total_ncell"]
    assert 2 ** 31 < end < 2 ** 32, end
    a.check_decompress()
    a.check_decompress(cz.DECODER_LANE)


def test_relative_bound_past_2g_elements(run):
    """r2r: the minimum sits in the first block, the maximum in the tail past every mark; range and
    bound in the header are those of the block alphabet."""
    case = hf.CASES["rel"]
    a = run(case)
    assert (a.header.min_val, a.header.max_val) == (hf.REL_LO, hf.REL_HI)
    assert a.header.rc.eb == case.eb * (hf.REL_HI - hf.REL_LO)
    a.check_decompress()
