"""The FZG codec (codec1 = FZCodec) through every public entry point, on the GPU.

For each case: compress succeeds and the header says FZCodec; the segment equals the numpy model's
encoding (tests/fzg_model.py) of the CPU oracle's codes byte for byte, twice; decode_codes gives the
oracle's codes; decompress into a NaN-poisoned buffer is bit-identical to the oracle's
reconstruction and to what the Huffman archive of the same field decompresses to; entry[5] is the
size and splen the oracle's outlier count.  Then the paths around it: empty and incompressible
payloads, outlier-slot growth, scan + finish, region decode (fallback), refused archives, merge and
spline refusals, the command line, the older cusz.h API, and no state leaking between codecs.
"""
import ctypes as C
import struct
import subprocess

import numpy as np
import pytest
import torch

import cusz_amd as cz
import fzg_model as fm
from cusz_amd import datagen
from gpu_util import d2h, sync, to_device
from test_gpu_region import full_decompress, region

pytestmark = pytest.mark.gpu

POISON = {np.float32: np.uint32(0x7FC0DEAD), np.float64: np.uint64(0x7FF8DEADBEEF0BAD)}
BITS = {np.float32: np.uint32, np.float64: np.uint64}
NO_SUCH_CODEC = cz.STATUS_NAMES.index("PSZ_ABORT_NO_SUCH_CODEC")

SHAPES = [(n, 1, 1) for n in (1, 255, 256, 257, 4095, 4096, 4097, 50_000)] + [
    (300, 40, 1), (96, 64, 40), (40, 24, 17),
    (256, 16, 16),  # brick-eligible: must still take the reference layout
]
CASES = [(s, dt, zz, radius, cz.Abs) for s in SHAPES for dt in (np.float32, np.float64) for zz in (False, True)
         for radius in (64, 512)]
CASES += [((96, 64, 40), np.float32, False, 512, cz.Rel), ((300, 40, 1), np.float64, True, 64, cz.Rel)]
# many workgroups, payload offsets past 2^16 words
CASES += [((256, 256, 64), np.float32, False, 512, cz.Abs)]


def _ctype(dtype):
    return cz.F4 if dtype == np.float32 else cz.F8


def _pred(zz):
    return cz.LorenzoZigZag if zz else cz.Lorenzo


def _field(dims, dtype, seed=None):
    return datagen.smooth3d_np(dims, sum(dims) if seed is None else seed, dtype=dtype).reshape(-1)


def _compress(r, d_in, eb, mode=cz.Abs, radius=512):
    ptr, nb, st = r.compress(d_in.data_ptr(), eb, mode, radius)
    assert st == cz.PSZ_SUCCESS
    return d2h(ptr, nb).tobytes()


def _poisoned(n, dtype):
    return to_device(np.full(n, POISON[dtype]).view(dtype))


def _segment(arch):
    h = cz.psz_header.from_buffer_copy(arch[:176])
    return h, arch[h.entry[2]:h.entry[3]]


def check_fzg_archive(oracle, arch, data, dims, dtype, zz, radius):
    """Header, segment and outlier cells of an FZG archive against the oracle + the model.
    -> (header, oracle codes, oracle reconstruction)."""
    n = data.size
    h, seg = _segment(arch)
    assert h.pipeline.codec1 == cz.FZCodec and h.pipeline.predictor == _pred(zz)
    assert (h.len.x, h.len.y, h.len.z) == tuple(dims)
    assert h.entry[5] == len(arch) and list(h.entry[:3]) == [0, 176, 176]
    assert (h.vle_sublen, h.vle_pardeg) == (4096, fm.counts(n)[1])
    ebx = h.rc.eb  # absolute (Rel mode: scaled by the range)
    codes_o, ov_o, oi_o = oracle.lorenzo_c(data.reshape(-1), dims, ebx, radius, zz)
    want = fm.encode(codes_o, radius, zz)
    assert len(seg) == len(want), (len(seg), len(want))
    assert seg == want, f"segment differs from the model at byte {next(i for i in range(len(seg)) if seg[i] != want[i])}"
    cells = np.frombuffer(arch[h.entry[3]:h.entry[4]], np.uint32).reshape(-1, 2)
    assert h.splen == len(oi_o) == cells.shape[0] and h.entry[4] == h.entry[5]
    order = np.argsort(cells[:, 1], kind="stable")
    np.testing.assert_array_equal(cells[order, 1], oi_o)
    np.testing.assert_array_equal(cells[order, 0], ov_o.view(np.uint32))
    xo = oracle.lorenzo_x(codes_o, ov_o, oi_o, dims, ebx, radius, zz, dtype)
    return h, codes_o, xo


def fzg_roundtrip(oracle, data, dims, dtype, eb, zz, radius, mode=cz.Abs):
    n = data.size
    r = cz.Resource(_ctype(dtype), dims, _pred(zz), codec=cz.FZCodec)
    d_in = to_device(data)
    arch = _compress(r, d_in, eb, mode, radius)  # fails without the feature: PSZ_ABORT_NO_SUCH_CODEC
    ino = r.internals()
    assert ino.layout == cz.LAYOUT_REFERENCE
    h, codes_o, xo = check_fzg_archive(oracle, arch, data, dims, dtype, zz, radius)
    # the code buffer keeps the untransformed codes
    np.testing.assert_array_equal(d2h(ino.d_quant_codes, 2 * n, np.uint16), codes_o)
    assert _compress(r, d_in, eb, mode, radius) == arch, "second compress of the same field"

    # decode_codes and decompress by a manager made from the header alone (its code buffer is new)
    d_arch = to_device(np.frombuffer(arch, np.uint8).copy())
    r2 = cz.Resource(None, None, header=h)
    r2.decode_codes(d_arch.data_ptr())
    sync()
    np.testing.assert_array_equal(d2h(r2.internals().d_quant_codes, 2 * n, np.uint16), codes_o)
    for mgr in (r, r2):
        got = full_decompress(mgr, d_arch, len(arch), n, dtype)
        bad = np.flatnonzero(got != xo.view(BITS[dtype]))
        assert bad.size == 0, f"{bad.size} reconstruction mismatches, first {bad[:5]}"
    r2.close()

    # ... and therefore to what the Huffman archive of the same field decompresses to
    rh = cz.Resource(_ctype(dtype), dims, _pred(zz))
    ptr, nb, _ = rh.compress(d_in.data_ptr(), eb, mode, radius)
    out = _poisoned(n, dtype)
    rh.decompress(ptr, nb, out.data_ptr())
    sync()
    np.testing.assert_array_equal(d2h(out.data_ptr(), n * np.dtype(dtype).itemsize, BITS[dtype]), xo.view(BITS[dtype]))
    rh.close()
    r.close()
    return arch


@pytest.mark.parametrize("dims,dtype,zz,radius,mode", CASES,
                         ids=["x".join(map(str, d)) + f"-{np.dtype(t).name}-zz{int(z)}-r{r}-{'rel' if m else 'abs'}"
                              for d, t, z, r, m in CASES])
def test_roundtrip(oracle, dims, dtype, zz, radius, mode):
    data = _field(dims, dtype)
    eb = 2e-4 if mode == cz.Abs else 1e-4
    arch = fzg_roundtrip(oracle, data, dims, dtype, eb, zz, radius, mode)
    if dims == (256, 256, 64):
        _, seg = _segment(arch)
        s = fm.parse(seg, data.size)
        assert s["blocks"] >= 1024 and s["total"] > 1 << 16


@pytest.mark.parametrize("zz", [False, True])
def test_constant_field_has_an_empty_payload(oracle, zz):
    dims = (5000, 1, 1)
    arch = fzg_roundtrip(oracle, np.zeros(5000, np.float32), dims, np.float32, 1e-3, zz, 512)
    _, seg = _segment(arch)
    s = fm.parse(seg, 5000)
    assert s["total"] == 0 and not s["flags"].any() and not s["block_off"].any()
    assert len(arch) == 176 + fm.offsets(5000)[2]
    if not zz:  # a constant that is not 0: only the elements predicted from 0 (one per 1,024) have a symbol
        arch = fzg_roundtrip(oracle, np.full(5000, 0.25, np.float32), dims, np.float32, 1e-3, zz, 512)
        s = fm.parse(_segment(arch)[1], 5000)
        assert 0 < s["total"] <= 5 * 8 and not s["flags"][np.arange(s["units"]) % 4 != 0].any()


NOISE_N = 50_000  # three whole 1-D outlier bricks of 16,384 and a short one
SLOT = 16_384 // 10 + 16


def _noise():
    return np.random.default_rng(77).standard_normal(NOISE_N).astype(np.float32)


def test_noise_spans_all_planes_and_round_trips(oracle):
    """Neighbour differences of sigma 1.41 against a code range of +-512 * 2 eb = +-2.76: codes of
    every magnitude, about 5 % outliers -- under the 10 % slots of every brick (checked here)."""
    data, eb = _noise(), 2.7e-3
    codes_o, _, oi_o = oracle.lorenzo_c(data, (NOISE_N, 1, 1), eb, 512, False)
    per_brick = np.bincount(oi_o // 16_384, minlength=4)
    assert 0 < per_brick.max() <= SLOT and oi_o.size > NOISE_N // 50, per_brick
    assert fm.symbols(codes_o, 512, False).max() >= 512  # the top plane of the book is in use
    r = cz.Resource(cz.F4, (NOISE_N,), codec=cz.FZCodec)
    cap0 = r.internals().archive_capacity
    r.close()
    arch = fzg_roundtrip(oracle, data, (NOISE_N, 1, 1), np.float32, eb, False, 512)
    _, seg = _segment(arch)
    print(f"noise: {2 * NOISE_N} bytes of codes -> segment {len(seg)} bytes, archive {len(arch)} of capacity {cap0}")
    assert len(arch) <= cap0


def test_outliers_past_the_slots_grow_and_give_the_same_archive(oracle):
    data, eb = _noise(), 1.0e-3  # about 30 % outliers: every whole brick is past its slot
    _, _, oi_o = oracle.lorenzo_c(data, (NOISE_N, 1, 1), eb, 512, False)
    assert np.bincount(oi_o // 16_384, minlength=4)[:3].min() > SLOT
    d_in = to_device(data)
    r = cz.Resource(cz.F4, (NOISE_N,), codec=cz.FZCodec)
    cap0 = r.internals().archive_capacity
    first = _compress(r, d_in, eb)  # warns inside, grows, repeats
    cap1 = r.internals().archive_capacity
    assert cap1 > cap0
    check_fzg_archive(oracle, first, data, (NOISE_N, 1, 1), np.float32, False, 512)
    assert _compress(r, d_in, eb) == first, "the grown manager: large enough from the start"
    assert r.internals().archive_capacity == cap1
    # the two-call form does not repeat by itself: warning, then the same archive
    fresh = cz.Resource(cz.F4, (NOISE_N,), codec=cz.FZCodec)
    hist = torch.zeros(1025, dtype=torch.int32, device="cuda")
    fresh.compress_scan(d_in.data_ptr(), eb, hist.data_ptr())
    with pytest.raises(cz.PszError) as ei:
        fresh.compress_finish(0)
    assert ei.value.status == cz.PSZ_WARN_OUTLIER_TOO_MANY
    fresh.compress_scan(d_in.data_ptr(), eb, hist.data_ptr())
    ptr, nb, _ = fresh.compress_finish(0)
    assert d2h(ptr, nb).tobytes() == first
    fresh.close()
    r.close()


@pytest.mark.parametrize("dims", [(96, 64, 40), (256, 16, 16)])
def test_scan_then_finish_with_its_own_histogram(oracle, dims):
    data = _field(dims, np.float32)
    d_in = to_device(data)
    r = cz.Resource(cz.F4, dims, codec=cz.FZCodec)
    whole = _compress(r, d_in, 2e-4)
    hist = torch.zeros(1025, dtype=torch.int32, device="cuda")
    r.compress_scan(d_in.data_ptr(), 2e-4, hist.data_ptr())
    ptr, nb, _ = r.compress_finish(hist.data_ptr())
    assert d2h(ptr, nb).tobytes() == whole
    sync()
    # the histogram is still produced and exported (not used by the codec)
    codes_o, _, _ = oracle.lorenzo_c(data, dims, 2e-4, 512, False)
    np.testing.assert_array_equal(hist[:1024].cpu().numpy().astype(np.uint32), oracle.histogram(codes_o, 1024))
    assert int(hist[1024].item()) == 0
    r.compress_scan(d_in.data_ptr(), 2e-4, hist.data_ptr())
    ptr, nb, _ = r.compress_finish(0)
    assert d2h(ptr, nb).tobytes() == whole
    t = r.stage_times()
    r.close()
    assert t[cz.T_BOOK] == 0


def test_stage_times_have_no_book_stage():
    dims = (96, 64, 40)
    d_in = to_device(_field(dims, np.float32))
    r = cz.Resource(cz.F4, dims, codec=cz.FZCodec)
    r.enable_timing()
    ptr, nb, _ = r.compress(d_in.data_ptr(), 2e-4)
    t = r.stage_times()
    assert t[cz.T_BOOK] == 0 and t[cz.T_ENCODE] > 0 and t[cz.T_PREDICT] > 0 and t[cz.T_COMPRESS] >= t[cz.T_ENCODE]
    out = _poisoned(int(np.prod(dims)), np.float32)
    r.decompress(ptr, nb, out.data_ptr())
    sync()
    t = r.stage_times()
    assert t[cz.T_DECODE] > 0 and t[cz.T_DECOMPRESS] >= t[cz.T_DECODE]
    r.close()


def test_knobs_are_accepted_and_change_nothing(oracle):
    dims = (256, 16, 16)
    data = _field(dims, np.float32)
    d_in = to_device(data)
    plain = cz.Resource(cz.F4, dims, codec=cz.FZCodec)
    want = _compress(plain, d_in, 2e-4)
    n = data.size
    d_arch = to_device(np.frombuffer(want, np.uint8).copy())
    base = full_decompress(plain, d_arch, len(want), n, np.float32)
    plain.close()
    for knob in ("sublen", "decoder", "layout", "codebook"):
        r = cz.Resource(cz.F4, dims, codec=cz.FZCodec)
        if knob == "sublen":
            r.set_sublen(512)
        elif knob == "decoder":
            r.set_decoder(cz.DECODER_WAVE)
        elif knob == "layout":
            r.set_layout(cz.LAYOUT_BRICK_FORCE)
        else:
            r.set_codebook(cz.CODEBOOK_STREAM)
        assert _compress(r, d_in, 2e-4) == want, knob
        assert r.internals().layout == cz.LAYOUT_REFERENCE
        np.testing.assert_array_equal(full_decompress(r, d_arch, len(want), n, np.float32), base, knob)
        r.close()


REGION_DIMS = (256, 16, 16)
REGION_BOXES = [((0, 0, 0), REGION_DIMS), ((250, 7, 7), (6, 3, 9)), ((0, 8, 8), (256, 8, 8)), ((131, 15, 2), (1, 1, 1))]


@pytest.mark.parametrize("dtype,zz", [(np.float32, False), (np.float64, True)])
def test_region_decode_takes_the_fallback(dtype, zz):
    data = _field(REGION_DIMS, dtype)
    r = cz.Resource(_ctype(dtype), REGION_DIMS, _pred(zz), codec=cz.FZCodec)
    arch = _compress(r, to_device(data), 3e-4, radius=64)
    d_arch = to_device(np.frombuffer(arch, np.uint8).copy())
    header = cz.psz_header.from_buffer_copy(arch[:176])
    full = full_decompress(r, d_arch, len(arch), data.size, dtype).reshape(REGION_DIMS[::-1])
    for o, e in REGION_BOXES:
        got, guards = region(r, d_arch, len(arch), o, e, dtype)
        want = np.ascontiguousarray(full[o[2]:o[2] + e[2], o[1]:o[1] + e[1], o[0]:o[0] + e[0]]).reshape(-1)
        np.testing.assert_array_equal(got, want)
        assert guards, "written outside the box"
        info, plan = r.last_region(), cz.region_plan(header, o, e)
        assert info.path == plan.path == cz.REGION_FALLBACK
        assert info.elems == plan.elems == int(np.prod(e)) and info.bricks == plan.bricks == 0
    r.close()


def _refused(r, arch, n, dtype, what):
    """decompress and decode_codes refuse `arch`; the output buffer keeps its poison."""
    d_arch = to_device(np.frombuffer(arch, np.uint8).copy())
    r.set_header(cz.psz_header.from_buffer_copy(arch[:176]))
    out = _poisoned(n, dtype)
    with pytest.raises(cz.PszError) as ei:
        r.decompress(d_arch.data_ptr(), len(arch), out.data_ptr())
    assert ei.value.status == cz.PSZ_AMD_ERR_BAD_ARCHIVE, what
    sync()
    assert np.all(d2h(out.data_ptr(), n * np.dtype(dtype).itemsize, BITS[dtype]) == POISON[dtype]), what
    with pytest.raises(cz.PszError) as ei:
        r.decode_codes(d_arch.data_ptr())
    assert ei.value.status == cz.PSZ_AMD_ERR_BAD_ARCHIVE, what


def test_corrupt_archives_are_refused_before_any_launch():
    dims, dtype = (4097, 3, 1), np.float32
    data = _field(dims, dtype)
    n = data.size
    r = cz.Resource(cz.F4, dims, codec=cz.FZCodec)
    arch = _compress(r, to_device(data), 1e-4, radius=64)
    h, seg = _segment(arch)
    s = fm.parse(seg, n)
    assert s["total"] > 0 and h.splen > 0
    _, off_rel, _ = fm.offsets(n)

    def shifted(delta):
        g = cz.psz_header.from_buffer_copy(arch[:176])
        for k in (3, 4, 5):
            g.entry[k] += delta
        return bytes(g)

    # the segment truncated by one word (the outlier cells move up, the entries say so)
    _refused(r, shifted(-8) + arch[176:h.entry[3] - 8] + arch[h.entry[3]:], n, dtype, "truncated payload")
    # ... and cut inside its offsets (refused from the entries alone)
    cut = off_rel + 4
    g = cz.psz_header.from_buffer_copy(arch[:176])
    g.entry[3] = 176 + cut
    g.entry[4] = g.entry[5] = 176 + cut + 8 * h.splen
    _refused(r, bytes(g) + seg[:cut] + arch[h.entry[3]:], n, dtype, "truncated offsets")

    def patched(at, fmt, value):
        b = bytearray(arch)
        struct.pack_into(fmt, b, 176 + at, value)
        return bytes(b)

    _refused(r, patched(12, "<I", s["units"] + 1), n, dtype, "unit count")
    _refused(r, patched(12, "<I", s["units"] - 1), n, dtype, "unit count")
    _refused(r, patched(0, "<I", fm.MAGIC ^ 1), n, dtype, "magic")
    _refused(r, patched(off_rel + 4 * s["blocks"], "<I", 0x3FFFFFFF), n, dtype, "block_off[blocks] leaves the archive")
    _refused(r, patched(24, "<Q", s["total"] + (1 << 20)), n, dtype, "word count")
    # the manager still decodes the good archive
    d_arch = to_device(np.frombuffer(arch, np.uint8).copy())
    r.set_header(h)
    full_decompress(r, d_arch, len(arch), n, dtype)
    r.close()


def test_merge_refuses_fzg_parts():
    dims = (64, 16, 8)
    parts = []
    for seed in (1, 2):
        r = cz.Resource(cz.F4, dims, codec=cz.FZCodec)
        parts.append(_compress(r, to_device(_field(dims, np.float32, seed)), 1e-3))
        r.close()
    with pytest.raises(cz.PszError) as ei:
        cz.merge_archives(parts, (64, 16, 16))
    assert ei.value.status == NO_SUCH_CODEC


def test_spline_with_fzg_is_refused():
    dims = (33, 9, 9)
    r = cz.Resource(cz.F4, dims, cz.Spline, codec=cz.FZCodec)
    with pytest.raises(cz.PszError) as ei:
        r.compress(to_device(_field(dims, np.float32)).data_ptr(), 1e-3)
    assert ei.value.status == NO_SUCH_CODEC
    r.close()


def test_other_codecs_stay_refused():
    dims = (300, 1, 1)
    for codec in (1, 2, 4, cz.NullCodec):  # HuffmanRevisit, LC, RunLength, NullCodec
        r = cz.Resource(cz.F4, dims, codec=codec)
        with pytest.raises(cz.PszError) as ei:
            r.compress(to_device(_field(dims, np.float32)).data_ptr(), 1e-3)
        assert ei.value.status == NO_SUCH_CODEC
        r.close()


def test_cli_writes_the_c_api_archive_and_reads_the_codec_from_it(tmp_path):
    dims = (96, 64, 40)
    data = _field(dims, np.float32, 4)
    f = tmp_path / "field.f32"
    data.tofile(f)
    z = subprocess.run([cz.CLI_PATH, "-z", "-t", "f32", "-m", "abs", "-e", "1e-4", "-l", "96x64x40", "--codec", "fzgcodec",
                        "-R", "time,cr", "-i", str(f)], capture_output=True, text=True, timeout=120)
    assert z.returncode == 0, z.stderr
    arch = (tmp_path / "field.f32.cusza").read_bytes()
    r = cz.Resource(cz.F4, dims, codec=cz.FZCodec)
    assert _compress(r, to_device(data), 1e-4) == arch
    r.close()
    x = subprocess.run([cz.CLI_PATH, "-x", "-i", str(tmp_path / "field.f32.cusza"), "--origin", str(f), "-R", "time"],
                       capture_output=True, text=True, timeout=120)
    assert x.returncode == 0, x.stderr
    assert " bounded" in x.stdout and "NOT bounded" not in x.stdout, x.stdout
    out = np.fromfile(tmp_path / "field.f32.cuszx", dtype=np.float32)
    assert np.abs(out.astype(np.float64) - data).max() <= 1.001e-4 + 2.0 ** -23 * float(np.abs(data).max())
    # --region on an FZG archive: the fallback, the same values
    x = subprocess.run([cz.CLI_PATH, "-x", "-i", str(tmp_path / "field.f32.cusza"), "--region", "5,6,7:20,3,2"],
                       capture_output=True, text=True, timeout=120)
    assert x.returncode == 0 and "fallback" in x.stdout, x.stdout + x.stderr
    box = np.fromfile(tmp_path / "field.f32.cuszx", dtype=np.float32)
    np.testing.assert_array_equal(box, out.reshape(40, 64, 96)[7:9, 6:9, 5:25].reshape(-1))


class psz_len3(C.Structure):
    _fields_ = [("x", C.c_size_t), ("y", C.c_size_t), ("z", C.c_size_t)]


def test_legacy_psz_create_with_fzcodec():
    L = cz.lib()
    L.psz_create.restype = C.c_void_p
    L.psz_create.argtypes = [C.c_int, psz_len3, C.c_int, C.c_int, C.c_int]
    L.psz_compress.restype = C.c_int
    L.psz_compress.argtypes = [C.c_void_p, C.c_void_p, psz_len3, C.c_double, C.c_int, C.POINTER(C.c_void_p),
                               C.POINTER(C.c_size_t), C.c_void_p, C.c_void_p, C.c_void_p]
    L.psz_decompress.restype = C.c_int
    L.psz_decompress.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, psz_len3, C.c_void_p, C.c_void_p]
    L.psz_release.argtypes = [C.c_void_p]
    dims = (96, 64, 40)
    data = _field(dims, np.float32)
    d = to_device(data)
    comp = L.psz_create(cz.F4, psz_len3(*dims), cz.Lorenzo, 512, cz.FZCodec)
    assert comp
    out, nb = C.c_void_p(), C.c_size_t()
    st = L.psz_compress(comp, d.data_ptr(), psz_len3(*dims), 1e-4, cz.Abs, C.byref(out), C.byref(nb), None, None, None)
    assert st == cz.PSZ_SUCCESS
    r = cz.Resource(cz.F4, dims, codec=cz.FZCodec)
    a_leg, a_api = d2h(out.value, nb.value).tobytes(), _compress(r, d, 1e-4)
    r.close()
    assert a_leg[176:] == a_api[176:]
    assert cz.psz_header.from_buffer_copy(a_leg[:176]).pipeline.codec1 == cz.FZCodec
    o = _poisoned(data.size, np.float32)
    st = L.psz_decompress(comp, out.value, nb.value, o.data_ptr(), psz_len3(*dims), None, None)
    sync()
    assert st == cz.PSZ_SUCCESS
    assert np.abs(o.cpu().numpy().astype(np.float64) - data).max() <= 1.001e-4 + 2.0 ** -23 * float(np.abs(data).max())
    L.psz_release(comp)


@pytest.mark.parametrize("dims", [(256, 16, 16), (50_000, 1, 1)])
def test_no_state_leaks_between_codecs(dims):
    """A Huffman compress / decompress before and after an FZG one on managers of the same field
    gives the archive and the field it always gives."""
    data = _field(dims, np.float32)
    n = data.size
    d_in = to_device(data)
    rh, rf = cz.Resource(cz.F4, dims), cz.Resource(cz.F4, dims, codec=cz.FZCodec)
    before = _compress(rh, d_in, 2e-4)
    d_h = to_device(np.frombuffer(before, np.uint8).copy())
    field = full_decompress(rh, d_h, len(before), n, np.float32)
    fz = _compress(rf, d_in, 2e-4)
    d_f = to_device(np.frombuffer(fz, np.uint8).copy())
    np.testing.assert_array_equal(full_decompress(rf, d_f, len(fz), n, np.float32), field)
    # the Huffman manager reads the FZG archive (the codec comes from the header), then goes on
    rh.set_header(cz.psz_header.from_buffer_copy(fz[:176]))
    np.testing.assert_array_equal(full_decompress(rh, d_f, len(fz), n, np.float32), field)
    rh.set_header(cz.psz_header.from_buffer_copy(before[:176]))  # (the header carries the pipeline)
    assert _compress(rh, d_in, 2e-4) == before
    np.testing.assert_array_equal(full_decompress(rh, d_h, len(before), n, np.float32), field)
    # and the FZG manager a Huffman archive
    rf.set_header(cz.psz_header.from_buffer_copy(before[:176]))
    np.testing.assert_array_equal(full_decompress(rf, d_h, len(before), n, np.float32), field)
    rh.close()
    rf.close()
