"""One manager driven through every compress path, the pending-scan state machine, and the order
in which a compress refuses its arguments.

A manager carries state from call to call: which path the last scan chose, the layout it reports,
buffers sized by the chunking, epochs and flags of the host transfers.  None of it may leak: an
archive is a function of the field and the knobs, whatever the manager did before.  And a finish
runs only right after the scan it belongs to: anything that overwrites the code buffer in between
(a decompress, a decode, a region decode) makes it PSZ_AMD_ERR_STATE.
"""
import numpy as np
import pytest
import torch

import cusz_amd as cz
from cusz_amd import datagen
from gpu_util import d2h, empty_device, sync, to_device

pytestmark = pytest.mark.gpu

EB = 1e-3
NO_SUCH_PREDICTOR = cz.STATUS_NAMES.index("PSZ_ABORT_NO_SUCH_PREDICTOR")
NO_SUCH_CODEC = cz.STATUS_NAMES.index("PSZ_ABORT_NO_SUCH_CODEC")

D3 = (256, 13, 11)   # brick-eligible, partial bricks in y and z
D1 = (40000,)        # three 16,384-element bricks, the last short
D2 = (300, 70)       # reference layout by default, linear bricks when forced

_fields = {}


def field(dims, dtype=np.float32):
    key = (dims, np.dtype(dtype).name)
    if key not in _fields:
        if len(dims) == 1:  # a seeded random walk
            a = np.cumsum(0.01 * np.random.default_rng(7).standard_normal(dims[0])).astype(dtype)
        else:
            a = datagen.smooth3d_np((tuple(dims) + (1,))[:3], dtype=dtype)
        _fields[key] = a
    return _fields[key]


def dt_of(dtype):
    return cz.F4 if np.dtype(dtype) == np.float32 else cz.F8


# a step: (codebook, layout, predictor, codec1) -- the whole configuration, not a change to it
S_SAMPLED = (cz.CODEBOOK_SAMPLED, cz.LAYOUT_BRICK, cz.Lorenzo, cz.Huffman)
S_STREAM = (cz.CODEBOOK_STREAM, cz.LAYOUT_BRICK, cz.Lorenzo, cz.Huffman)
S_EXACT = (cz.CODEBOOK_EXACT, cz.LAYOUT_BRICK, cz.Lorenzo, cz.Huffman)
S_REFERENCE = (cz.CODEBOOK_EXACT, cz.LAYOUT_REFERENCE, cz.Lorenzo, cz.Huffman)
S_ZIGZAG = (cz.CODEBOOK_EXACT, cz.LAYOUT_BRICK, cz.LorenzoZigZag, cz.Huffman)
S_FZG = (cz.CODEBOOK_EXACT, cz.LAYOUT_BRICK, cz.Lorenzo, cz.FZCodec)
S_SPLINE = (cz.CODEBOOK_EXACT, cz.LAYOUT_BRICK, cz.Spline, cz.Huffman)
S_FORCE = (cz.CODEBOOK_SAMPLED, cz.LAYOUT_BRICK_FORCE, cz.Lorenzo, cz.Huffman)
S_FZG_DEFAULT = (cz.CODEBOOK_SAMPLED, cz.LAYOUT_BRICK, cz.Lorenzo, cz.FZCodec)


def configure(r, step):
    """Put manager r (which has compressed at least once, or was created for this predictor and
    codec) into the configuration `step`."""
    codebook, layout, pred, codec = step
    r.set_codebook(codebook)
    r.set_layout(layout)
    if r.header.entry[5]:  # the last archive's header, with the step's predictor and codec
        h = cz.psz_header.from_buffer_copy(bytes(r.header))
        h.pipeline.predictor, h.pipeline.codec1 = pred, codec
        r.set_header(h)


def run(r, d_in, dtype):
    """compress + decompress on r -> (archive bytes, layout reported, decompressed bits)."""
    ptr, nbytes, st = r.compress(d_in.data_ptr(), EB)
    assert st == cz.PSZ_SUCCESS
    arch = d2h(ptr, nbytes).tobytes()
    layout = r.internals().layout
    out = empty_device(d_in.numel(), d_in.dtype)
    out.fill_(float("nan"))
    r.decompress(ptr, nbytes, out.data_ptr())
    sync()
    return arch, layout, out.cpu().numpy().view(np.uint64 if dtype == np.float64 else np.uint32)


_fresh = {}


def fresh(dims, dtype, step):
    """What a new manager configured for `step` alone makes of the field (computed once)."""
    key = (dims, np.dtype(dtype).name, step)
    if key not in _fresh:
        r = cz.Resource(dt_of(dtype), dims, step[2], codec=step[3])
        configure(r, step)
        _fresh[key] = run(r, to_device(field(dims, dtype)), dtype)
        r.close()
    return _fresh[key]


SEQ3 = [S_SAMPLED, S_STREAM, S_EXACT, S_REFERENCE, S_ZIGZAG, S_FZG, S_SPLINE, S_SAMPLED]
SEQUENCES = [
    ("3d-f32", D3, np.float32, SEQ3),
    ("3d-f64", D3, np.float64, SEQ3),
    ("1d-f32", D1, np.float32, [S_SAMPLED, S_EXACT, S_REFERENCE, S_FZG]),
    ("2d-f32", D2, np.float32, [S_SAMPLED, S_FORCE, S_FZG_DEFAULT]),
]


@pytest.mark.parametrize("dims,dtype,steps", [s[1:] for s in SEQUENCES], ids=[s[0] for s in SEQUENCES])
def test_one_manager_through_every_path(dims, dtype, steps):
    """After each step the reused manager's archive, reported layout and decompressed field equal
    those of a fresh manager configured for that step alone; coming back to the first
    configuration gives the first archive again."""
    d_in = to_device(field(dims, dtype))
    r = cz.Resource(dt_of(dtype), dims, steps[0][2], codec=steps[0][3])
    seen = []
    for k, step in enumerate(steps):
        configure(r, step)
        arch, layout, bits = run(r, d_in, dtype)
        arch_f, layout_f, bits_f = fresh(dims, dtype, step)
        assert layout == layout_f, f"step {k + 1}: layout {layout}, a fresh manager reports {layout_f}"
        assert len(arch) == len(arch_f), f"step {k + 1}: {len(arch)} bytes, a fresh manager gives {len(arch_f)}"
        diff = np.flatnonzero(np.frombuffer(arch, np.uint8) != np.frombuffer(arch_f, np.uint8))
        assert diff.size == 0, f"step {k + 1}: {diff.size} bytes differ from a fresh manager's, first at {diff[:4]}"
        np.testing.assert_array_equal(bits, bits_f, err_msg=f"step {k + 1}: decompressed field")
        seen.append(arch)
    if steps[-1] == steps[0]:
        assert seen[-1] == seen[0], "the first configuration again does not give the first archive again"
    r.close()


def test_layouts_reported():
    """The paths the sequences are meant to drive are the ones taken."""
    brick, ref = cz.LAYOUT_BRICK, cz.LAYOUT_REFERENCE
    want3 = [brick, brick, brick, ref, brick, ref, ref, brick]
    assert [fresh(D3, np.float32, s)[1] for s in SEQ3] == want3
    assert [fresh(D1, np.float32, s)[1] for s in (S_SAMPLED, S_EXACT, S_REFERENCE, S_FZG)] == [brick, brick, ref, ref]
    assert [fresh(D2, np.float32, s)[1] for s in (S_SAMPLED, S_FORCE, S_FZG_DEFAULT)] == [ref, brick, ref]


# ---- the pending-scan state machine ---------------------------------------------------------

STATE_CASES = [
    ("3d-brick", D3, cz.Lorenzo, cz.LAYOUT_BRICK, (32, 3, 2), (100, 7, 5)),
    ("1d-reference", D1, cz.Lorenzo, cz.LAYOUT_REFERENCE, (100,), (5000,)),
    ("3d-spline", D3, cz.Spline, cz.LAYOUT_BRICK, (32, 3, 2), (100, 7, 5)),
]


def expect_status(status, fn, *args, **kw):
    with pytest.raises(cz.PszError) as e:
        fn(*args, **kw)
    assert e.value.status == status, e.value


@pytest.mark.parametrize("dims,pred,layout,origin,extent", [c[1:] for c in STATE_CASES], ids=[c[0] for c in STATE_CASES])
def test_pending_scan_state_machine(dims, pred, layout, origin, extent):
    data = field(dims)
    n = data.size
    d_in = to_device(data)
    d_hist = empty_device(1025, torch.int32)  # u32[2 radius + 1]
    out = empty_device(n, torch.float32)
    r = cz.Resource(cz.F4, dims, pred)
    r.set_layout(layout)

    def compress_bytes():
        ptr, nbytes, _ = r.compress(d_in.data_ptr(), EB)
        return d2h(ptr, nbytes).tobytes()

    def scan():
        assert r.compress_scan(d_in.data_ptr(), EB, d_hist.data_ptr()) == cz.PSZ_SUCCESS

    def finish_bytes():
        ptr, nbytes, _ = r.compress_finish()
        return d2h(ptr, nbytes).tobytes()

    expect_status(cz.PSZ_AMD_ERR_STATE, r.compress_finish)  # nothing scanned yet
    before = compress_bytes()
    earlier = to_device(np.frombuffer(before, np.uint8).copy())  # (a scan may write into the manager's archive)

    scan()
    single = finish_bytes()
    expect_status(cz.PSZ_AMD_ERR_STATE, r.compress_finish)  # the scan is consumed
    assert compress_bytes() == before

    middles = [lambda: r.decompress(earlier.data_ptr(), len(before), out.data_ptr()),
               lambda: r.decode_codes(earlier.data_ptr()),
               lambda: r.decompress_region(earlier.data_ptr(), len(before), origin, extent, out.data_ptr())]
    for middle in middles:
        scan()
        middle()  # overwrites the codes the finish would pack
        expect_status(cz.PSZ_AMD_ERR_STATE, r.compress_finish)
        assert compress_bytes() == before

    scan()
    scan()
    assert finish_bytes() == single
    sync()
    r.close()


# ---- the order of refusals ------------------------------------------------------------------

def compress_status(r, d_in, d_hist, via, mode, radius):
    """The status of a compress (via "compress") or of a scan (via "scan") with this radius."""
    try:
        if via == "compress":
            return r.compress(d_in.data_ptr(), EB, mode, radius)[2]
        return r.compress_scan(d_in.data_ptr(), EB, d_hist.data_ptr(), mode, radius)
    except cz.PszError as e:
        return e.status


PRECEDENCE = [
    # predictor, codec1, radius, expected status
    ("bad-predictor-bad-codec", cz.LorenzoProto, cz.NullCodec, 512, NO_SUCH_PREDICTOR),
    ("bad-predictor-radius-0", cz.LorenzoProto, cz.Huffman, 0, NO_SUCH_PREDICTOR),
    ("bad-codec", cz.Lorenzo, cz.NullCodec, 512, NO_SUCH_CODEC),
    ("bad-codec-radius-0", cz.Lorenzo, cz.NullCodec, 0, NO_SUCH_CODEC),
    ("spline-fzcodec", cz.Spline, cz.FZCodec, 512, NO_SUCH_CODEC),
    ("radius-0", cz.Lorenzo, cz.Huffman, 0, cz.PSZ_AMD_ERR_INVALID_ARG),
    ("radius-0-fzcodec", cz.Lorenzo, cz.FZCodec, 0, cz.PSZ_AMD_ERR_INVALID_ARG),
    ("radius-0-spline", cz.Spline, cz.Huffman, 0, cz.PSZ_AMD_ERR_INVALID_ARG),
    ("radius-600", cz.Lorenzo, cz.Huffman, 600, cz.PSZ_WARN_RADIUS_TOO_LARGE),
]


@pytest.mark.parametrize("mode", [cz.Abs, cz.Rel], ids=["abs", "rel"])
@pytest.mark.parametrize("via", ["compress", "scan"])
@pytest.mark.parametrize("pred,codec,radius,want", [c[1:] for c in PRECEDENCE], ids=[c[0] for c in PRECEDENCE])
def test_status_precedence(pred, codec, radius, want, via, mode):
    """Predictor, then codec, then radius; a radius above 512 is clamped with a warning."""
    d_in = to_device(field(D3))
    d_hist = empty_device(1025, torch.int32)
    r = cz.Resource(cz.F4, D3, pred, codec=codec)
    assert compress_status(r, d_in, d_hist, via, mode, radius) == want
    if want == cz.PSZ_WARN_RADIUS_TOO_LARGE:
        if via == "scan":
            r.compress_finish()
        assert r.header.rc.radius == 512
    elif via == "scan":
        expect_status(cz.PSZ_AMD_ERR_STATE, r.compress_finish)  # a refused scan leaves nothing pending
    r.close()


@pytest.mark.parametrize("mode", [cz.Abs, cz.Rel], ids=["abs", "rel"])
def test_bad_codec_in_stream_mode(mode):
    d_in = to_device(field(D3))
    r = cz.Resource(cz.F4, D3, cz.Lorenzo, codec=cz.NullCodec)
    r.set_codebook(cz.CODEBOOK_STREAM)
    assert compress_status(r, d_in, None, "compress", mode, 512) == NO_SUCH_CODEC
    assert compress_status(r, d_in, None, "compress", mode, 0) == NO_SUCH_CODEC
    r.close()


def test_decompress_refuses_unknown_predictor():
    """A valid archive whose header copy names a predictor this build does not have."""
    d_in = to_device(field(D3))
    out = empty_device(d_in.numel(), torch.float32)
    r = cz.Resource(cz.F4, D3)
    ptr, nbytes, _ = r.compress(d_in.data_ptr(), EB)
    h = cz.psz_header.from_buffer_copy(bytes(r.header))
    h.pipeline.predictor = cz.LorenzoProto
    r.set_header(h)
    expect_status(NO_SUCH_PREDICTOR, r.decompress, ptr, nbytes, out.data_ptr())
    expect_status(NO_SUCH_PREDICTOR, r.decompress_region, ptr, nbytes, (32, 3, 2), (100, 7, 5), out.data_ptr())
    r.close()
