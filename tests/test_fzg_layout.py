"""The FZG segment's host-side layout (cusz_amd/csrc/archive_layout.hh FzgLayout / FzgView, compiled
here with g++ alone: the header includes no HIP header) against the numpy model of the format
(tests/fzg_model.py): the writer's offsets and header templates, and the decode side's checks over
model-built archives, whole and corrupt.  CPU-only."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import cusz_amd as cz
import fzg_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = [1, 255, 256, 257, 4095, 4096, 4097, 65_537]
ENCODED, SPFMT, END = 2, 3, 5


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("fzg_layout") / "libfzgshim.so"
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "cusz_amd", "csrc"), "-o", str(out),
           os.path.join(ROOT, "tests", "host", "fzg_layout_shim.cc")]
    try:
        subprocess.run(cmd, check=True, capture_output=True, timeout=120)
    except OSError as e:
        pytest.skip(f"g++ unavailable: {e}")
    except subprocess.CalledProcessError as e:
        pytest.fail(f"archive_layout.hh does not compile with g++ alone:\n{e.stderr.decode()}")
    lib = C.CDLL(str(out))
    lib.fzg_shim_layout.restype = None
    lib.fzg_shim_layout.argtypes = [C.c_size_t, C.c_void_p]
    lib.fzg_shim_fill.restype = None
    lib.fzg_shim_fill.argtypes = [C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.fzg_shim_check.restype = C.c_int
    lib.fzg_shim_check.argtypes = [C.c_void_p, C.c_size_t, C.c_char_p]
    return lib


@pytest.mark.parametrize("n", NS)
def test_layout_and_templates_equal_the_model(shim, n):
    off = np.zeros(6, np.uint64)
    shim.fzg_shim_layout(n, off.ctypes.data)
    units, blocks = fm.counts(n)
    flags_rel, off_rel, payload_rel = fm.offsets(n)
    assert flags_rel == 32
    assert off.tolist() == [176, units, blocks, off_rel, payload_rel, payload_rel + 512 * units]
    # the worst case the pipeline sizes the archive by covers every segment the model can write
    assert len(fm.encode(np.full(n, 0xFFFF, np.uint16), 512, True)) <= payload_rel + 512 * units

    h, fh = cz.psz_header(), (C.c_uint8 * 32)()
    for transform in (fm.PLAIN, fm.ZIGZAG_DELTA):
        shim.fzg_shim_fill(n, transform, C.addressof(h), fh)
        assert fm.HEADER.unpack(bytes(fh)) == (fm.MAGIC, 256, transform, units, blocks, 0, 0)
        # the template is the model's header of an empty payload (all symbols 0); the device fills
        # in the word count
        seg = fm.encode(np.full(n, 0 if transform == fm.PLAIN else 512, np.uint16), 512, transform == fm.PLAIN)
        assert seg[:32] == bytes(fh)
    assert (h.vle_sublen, h.vle_pardeg, h.len.x, h.len.y, h.len.z) == (4096, blocks, n, 1, 1)
    assert list(h.entry[:3]) == [0, 176, 176]
    # nothing else: the psz header's other fields are the caller's (0xFF bytes from the shim)
    assert list(h.entry[3:]) == [0xFFFFFFFF] * 3 and h.dtype == -1 and h.splen == 2 ** 64 - 1


def _archive(n, seed=3):
    """(header, archive bytes) of a model-built FZG archive without outlier cells."""
    rng = np.random.default_rng(seed + n)
    codes = np.clip(rng.normal(512, 4, n).round(), 1, 1023).astype(np.uint16)
    seg = fm.encode(codes, 512, False)
    h = cz.psz_header()
    h.pipeline.codec1 = cz.FZCodec
    h.rc.radius = 512
    h.len = cz.psz_len(n, 1, 1)
    end = 176 + len(seg)
    for k, v in enumerate([0, 176, 176, end, end, end]):
        h.entry[k] = v
    return h, bytes(h) + seg


def _check(shim, h, n, arch):
    return shim.fzg_shim_check(C.addressof(h), n, arch)


@pytest.mark.parametrize("n", NS)
def test_view_accepts_model_archives_and_refuses_corrupt_ones(shim, n):
    h, arch = _archive(n)
    assert _check(shim, h, n, arch) == 0
    _, off_rel, payload_rel = fm.offsets(n)
    units, blocks = fm.counts(n)
    total = struct.unpack_from("<Q", arch, 176 + 24)[0]
    assert total > 0

    def with_entry(k_from, delta):
        g = cz.psz_header.from_buffer_copy(bytes(h))
        for k in range(k_from, 6):
            g.entry[k] += delta
        return g

    # truncated: the last payload word cut off; then cut into the offsets (refused before any read)
    assert _check(shim, with_entry(SPFMT, -8), n, arch[:-8]) == 2
    g = with_entry(SPFMT, 0)
    for k in range(SPFMT, 6):
        g.entry[k] = 176 + payload_rel - 8
    assert _check(shim, g, n, arch[:176 + payload_rel - 8]) == 1
    # entries out of order, a segment that is not 8-byte aligned
    g = with_entry(SPFMT, 0)
    g.entry[SPFMT] = g.entry[ENCODED] - 8
    assert _check(shim, g, n, arch) == 1
    assert _check(shim, with_entry(ENCODED, 4), n, arch[:176] + b"\0" * 4 + arch[176:]) == 1

    def patched(at, fmt, value):
        b = bytearray(arch)
        struct.pack_into(fmt, b, 176 + at, value)
        return bytes(b)

    assert _check(shim, h, n, patched(0, "<I", fm.MAGIC + 1)) == 2
    assert _check(shim, h, n, patched(4, "<I", 128)) == 2
    assert _check(shim, h, n, patched(8, "<I", 2)) == 2
    assert _check(shim, h, n, patched(12, "<I", units + 1)) == 2
    assert _check(shim, h, n, patched(16, "<I", blocks + 1)) == 2
    assert _check(shim, h, n, patched(24, "<Q", total + 1)) == 2
    # block_off[blocks] leaves the archive (or merely disagrees with the header's count)
    assert _check(shim, h, n, patched(off_rel + 4 * blocks, "<I", 0x3FFFFFFF)) == 2
    assert _check(shim, h, n, patched(off_rel + 4 * blocks, "<I", total - 1)) == 2
    # an archive of another length
    assert _check(shim, h, n + fm.BLOCK, arch) != 0
