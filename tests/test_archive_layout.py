"""The archive's host-side layout (cusz_amd/csrc/archive_layout.hh, compiled here with g++ alone:
the header includes no HIP header) against the running sums a reference encoder lays its
segments out by (archive_util.oracle_archive; hf_buf.cc:199-211): the writer's offsets and header
templates, and the decode-side view over an oracle-built archive.  CPU-only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cusz_amd as cz
from archive_util import oracle_archive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PSZ_HEADER_BYTES = 176
ENCODED, END = 2, 5  # psz_header.entry: the phf segment, the archive's end


class phf_header(C.Structure):
    """include/hf.h: bklen:16 @0 | sublen @4 | pardeg @8 | original_len @16 | total_nbit @24 |
    total_ncell @32 | entry[6] @40."""
    _fields_ = [("bklen", C.c_int, 16), ("sublen", C.c_int), ("pardeg", C.c_int), ("original_len", C.c_size_t),
                ("total_nbit", C.c_size_t), ("total_ncell", C.c_size_t), ("entry", C.c_uint32 * 6)]


assert C.sizeof(phf_header) == 64 and phf_header.entry.offset == 40


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("layout") / "liblayoutshim.so"
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "cusz_amd", "csrc"), "-o", str(out), os.path.join(ROOT, "tests", "host", "layout_shim.cc")]
    try:
        subprocess.run(cmd, check=True, capture_output=True, timeout=120)
    except OSError as e:
        pytest.skip(f"g++ unavailable: {e}")
    except subprocess.CalledProcessError as e:
        pytest.fail(f"archive_layout.hh does not compile with g++ alone:\n{e.stderr.decode()}")
    lib = C.CDLL(str(out))
    lib.shim_layout.restype = None
    lib.shim_layout.argtypes = [C.c_size_t, C.c_int, C.c_size_t, C.c_void_p]
    lib.shim_fill.restype = None
    lib.shim_fill.argtypes = [C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p]
    lib.shim_view.restype = None
    lib.shim_view.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p]
    return lib


def _running_sums(sizes):
    ent = [0]
    for s in sizes:
        ent.append(ent[-1] + s)
    return ent


@pytest.mark.parametrize("anchor_bytes", [0, 4 * 27, 8 * 27])
@pytest.mark.parametrize("pardeg", [1, 3, 4097])
@pytest.mark.parametrize("bklen", [2, 128, 1024])
def test_layout_and_templates_equal_running_sums(shim, bklen, pardeg, anchor_bytes):
    # the phf segment's sections as archive_util.oracle_archive sizes them (the bitstream's
    # length is not static: its start is the last static entry)
    rv_bytes = 4 * 32 + 4 * 32 + 2 * bklen  # first i32[32] | entry i32[32] | keys u16[bklen]
    ent = _running_sums([128, rv_bytes, 4 * pardeg, 4 * pardeg])
    phf_off = PSZ_HEADER_BYTES + anchor_bytes

    off = np.zeros(5, np.uint64)
    shim.shim_layout(anchor_bytes, bklen, pardeg, off.ctypes.data)
    assert off.tolist() == [phf_off, rv_bytes, ent[2], ent[3], ent[4]]

    sublen, n = 256, 256 * (pardeg - 1) + 7
    h, ph = cz.psz_header(), phf_header()
    shim.shim_fill(anchor_bytes, bklen, sublen, pardeg, n, C.addressof(h), C.addressof(ph))
    assert list(ph.entry[:5]) == ent[:5]
    assert list(h.entry[:3]) == [0, PSZ_HEADER_BYTES, phf_off]
    # the rest of the static fields, and nothing else: the phf header is zeroed around them, the
    # psz header's other fields are the caller's (0xFF bytes from the shim)
    assert (ph.bklen, ph.sublen, ph.pardeg, ph.original_len) == (bklen, sublen, pardeg, n)
    assert (ph.total_nbit, ph.total_ncell, ph.entry[5]) == (0, 0, 0)
    assert (h.vle_sublen, h.vle_pardeg, h.len.x, h.len.y, h.len.z) == (sublen, pardeg, n, 1, 1)
    assert list(h.entry[3:]) == [0xFFFFFFFF] * 3 and h.dtype == -1 and h.splen == 2 ** 64 - 1


@pytest.fixture(scope="module")
def archive(oracle):
    """A reference-layout archive of a 1-D field of 2,000 elements at sublen 256: 8 chunks, the
    last one short; no outliers, so the bitstream is the archive's last segment.  Returns (bytes,
    ent, pardeg, bitstream words), ent the phf segment's running sums as oracle_archive forms them."""
    n, sublen, eb = 2000, 256, 1e-3
    rng = np.random.default_rng(11)
    data = np.cumsum(rng.normal(0, 4e-3, n)).astype(np.float32)
    codes, ov, oi = oracle.lorenzo_c(data, (n, 1, 1), eb)
    book, rv = oracle.codebook(oracle.histogram(codes))
    arch = oracle_archive(oracle, codes, ov, oi, (n, 1, 1), eb, book, rv, sublen=sublen)
    nbit, _, bs, _ = oracle.hf_encode(codes, book, sublen)
    assert nbit.size == 8 and n % sublen != 0 and oi.size == 0
    ent = _running_sums([oracle.PHF_FORCED_ALIGN, rv.size, 4 * nbit.size, 4 * nbit.size, 4 * bs.size])
    return arch, ent, int(nbit.size), int(bs.size)


def _view(shim, header, arch):
    out = np.zeros(8, np.int64)
    shim.shim_view(C.addressof(header), arch, out.ctypes.data)
    return out.tolist()


def test_view_of_oracle_archive(shim, archive):
    arch, ent, pardeg, bs_words = archive
    h = cz.psz_header.from_buffer_copy(arch[:PSZ_HEADER_BYTES])
    ph = phf_header.from_buffer_copy(arch[h.entry[ENCODED]:h.entry[ENCODED] + 64])
    assert list(ph.entry) == ent  # the archive's own phf header carries the same sums
    bitstream, revbook, par_nbit, par_entry, words, bklen, sublen, pd = _view(shim, h, arch)
    base = h.entry[ENCODED]
    assert (revbook, par_nbit, par_entry, bitstream) == (base + ent[1], base + ent[2], base + ent[3], base + ent[4])
    # (bs_words runs to the archive's end, the range of the decoders' loads: here the bitstream's)
    assert h.entry[END] == len(arch) and h.splen == 0
    assert words == bs_words
    assert (bklen, sublen, pd) == (2 * h.rc.radius, h.vle_sublen, h.vle_pardeg) == (1024, 256, pardeg)


def test_view_bs_words_zero_when_end_before_bitstream(shim, archive):
    arch, ent, _, _ = archive
    h = cz.psz_header.from_buffer_copy(arch[:PSZ_HEADER_BYTES])
    bits_off = h.entry[ENCODED] + ent[4]
    for end in (bits_off, bits_off - 1, 0):
        h.entry[END] = end
        assert _view(shim, h, arch)[4] == 0
    h.entry[END] = bits_off + 4
    assert _view(shim, h, arch)[4] == 1
