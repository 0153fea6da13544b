"""Outlier bursts on the brick path: a y-step, a brick, or every brick of a field past its outlier
slot (edge_fields.burst_field; test_edge_fields.py checks that each field overflows what it is
meant to).  A slot that overflows sends cells to the shared spill list, the slots grow and the
compress repeats (pipeline.cc grow_slots, pipeline_compress.cc finish_compress); what the caller gets must be the
archive a manager with roomy slots writes: bit-exact parity with the oracle (codes, outlier set
and values, histogram, Huffman segment, every decoder), the same bytes from the grown manager
again and from a fresh one, cells in brick order (the fused region decoder reads them ranked).

Growth shows in internals().archive_capacity, which alloc_chunk_state recomputes from the slots.
"""
import numpy as np
import pytest
import torch

import cusz_amd as cz
import edge_fields as ef
from gpu_util import check_phf_against_oracle, d2h, parse_archive, sync, to_device
from test_gpu_parity import run_roundtrip
from test_gpu_region import full_decompress, region
from test_gpu_sampled import sampled_roundtrip

pytestmark = pytest.mark.gpu

MODES = {"sampled": cz.CODEBOOK_SAMPLED, "exact": cz.CODEBOOK_EXACT, "stream": cz.CODEBOOK_STREAM}

# kind, dtype, zigzag, codebook mode
CASES = [(k, np.float32, False, m) for k in ("ystep", "brick", "all") for m in MODES] + [
    ("brick", np.float64, False, "sampled"), ("ystep", np.float64, False, "stream"),
    ("brick", np.float32, True, "sampled"), ("ystep", np.float32, True, "stream"),
    ("brick2d", np.float32, False, "sampled"),
]

# a box across the saturated brick and its two neighbours in y (bricks by = 0, 1, 2 of one column)
REGION_BOX = {"ystep": ((300, 6, 9), (50, 13, 4)), "brick": ((100, 6, 9), (50, 13, 4)), "all": ((100, 6, 9), (50, 13, 4))}


def _manager(dtype, dims, zz, mode, layout):
    r = cz.Resource(cz.F4 if dtype == np.float32 else cz.F8, dims, cz.LorenzoZigZag if zz else cz.Lorenzo)
    if layout is not None:
        r.set_layout(layout)
    r.set_codebook(MODES[mode])
    return r


def _compress(r, d_in, eb, radius):
    ptr, nb, st = r.compress(d_in.data_ptr(), eb, cz.Abs, radius)
    assert st == cz.PSZ_SUCCESS
    return d2h(ptr, nb).tobytes()


@pytest.mark.parametrize("kind,dtype,zz,mode", CASES,
                         ids=[f"{k}-{np.dtype(d).name}-zz{int(z)}-{m}" for k, d, z, m in CASES])
def test_burst(oracle, kind, dtype, zz, mode):
    data, dims, eb, radius = ef.burst_field(kind, dtype)
    layout = cz.LAYOUT_BRICK_FORCE if kind == "brick2d" else None
    n = data.size

    # parity with the oracle, from a manager of its own
    if mode == "stream":
        arch_parity = sampled_roundtrip(oracle, data, dims, dtype, eb, zz, radius, MODES[mode])
    else:
        arch_parity, _ = run_roundtrip(oracle, data, dims, eb, dtype, zz, radius, layout=layout, codebook=MODES[mode])

    # growth, and the same bytes whatever the manager went through before
    r = _manager(dtype, dims, zz, mode, layout)
    d_in = to_device(data)
    cap0 = r.internals().archive_capacity
    first = _compress(r, d_in, eb, radius)
    assert r.internals().layout == cz.LAYOUT_BRICK
    cap1 = r.internals().archive_capacity
    print(f"burst {kind} {np.dtype(dtype).name} zz{int(zz)} {mode}: archive_capacity {cap0} -> {cap1}")
    if kind == "ystep" and mode != "stream":
        assert cap1 == cap0, "no brick is past its slot: nothing may grow"
    else:
        assert cap1 > cap0, "a slot overflowed: the slots must have grown"
    assert first == arch_parity, "the manager under test and the parity run's manager disagree"
    assert _compress(r, d_in, eb, radius) == first, "second compress on the grown manager"
    assert r.internals().archive_capacity == cap1
    fresh = _manager(dtype, dims, zz, mode, layout)
    assert _compress(fresh, d_in, eb, radius) == first, "fresh manager"
    fresh.close()

    # the whole field, by the manager itself and by one made from the header alone
    d_arch = to_device(np.frombuffer(first, np.uint8).copy())
    header = cz.psz_header.from_buffer_copy(first[:176])
    full = full_decompress(r, d_arch, len(first), n, dtype)
    codes_o, ov_o, oi_o = oracle.lorenzo_c(data, dims, eb, radius, zz)
    xo = oracle.lorenzo_x(codes_o, ov_o, oi_o, dims, eb, radius, zz, dtype)
    np.testing.assert_array_equal(full, xo.view(full.dtype))
    r2 = cz.Resource(None, None, header=header)
    np.testing.assert_array_equal(full_decompress(r2, d_arch, len(first), n, dtype), full)

    # a box across the saturated brick and two neighbours (the fused region decoder, plain Lorenzo
    # on 3-D bricks; ZigZag and 2-D take the fallback by design)
    if kind in REGION_BOX:
        o, e = REGION_BOX[kind]
        want = np.ascontiguousarray(full.reshape(dims[::-1])[o[2]:o[2] + e[2], o[1]:o[1] + e[1], o[0]:o[0] + e[0]])
        for mgr in (r, r2):
            got, guards = region(mgr, d_arch, len(first), o, e, dtype)
            np.testing.assert_array_equal(got, want.reshape(-1))
            assert guards, "written outside the box"
            info = mgr.last_region()
            assert info.path == (cz.REGION_FALLBACK if zz else cz.REGION_FUSED)
            if not zz:
                assert info.bricks == 3 and (info.brick_n.x, info.brick_n.y, info.brick_n.z) == (1, 3, 1)
    r2.close()

    # the grown manager on a field without bursts: what a fresh manager writes
    if kind != "brick2d":
        d_smooth = to_device(ef.smooth_field(dtype))
        fresh = _manager(dtype, dims, zz, mode, layout)
        assert _compress(r, d_smooth, eb, radius) == _compress(fresh, d_smooth, eb, radius)
        fresh.close()
    r.close()


@pytest.mark.parametrize("mode", ["sampled", "exact"])
def test_scan_finish_warns_once_then_matches_compress(oracle, mode):
    """The two-call form does not repeat by itself: the finish after a scan whose brick overflowed
    its slot returns PSZ_WARN_OUTLIER_TOO_MANY (the slots have grown), the repeated scan and finish
    succeed and give compress()'s archive.

    Byte for byte in the exact mode.  In the default mode the two differ by design in the codebook
    alone (compress() books pass 1's brick sample on the host, a finish books the whole histogram
    on the device: test_gpu_shard.test_sharded_default_mode_decodes_like_whole_field), so there the
    outlier segment must equal compress()'s byte for byte, the Huffman segment the oracle's
    encoding with the two-queue book of the whole histogram, and both decompress to the same bits."""
    data, dims, eb, radius = ef.burst_field("brick")
    d_in = to_device(data)
    r = _manager(np.float32, dims, False, mode, None)
    hist = torch.zeros(2 * radius + 1, dtype=torch.int32, device="cuda")
    cap0 = r.internals().archive_capacity
    r.compress_scan(d_in.data_ptr(), eb, hist.data_ptr(), cz.Abs, radius)
    with pytest.raises(cz.PszError) as ei:
        r.compress_finish(0)
    assert ei.value.status == cz.PSZ_WARN_OUTLIER_TOO_MANY
    assert r.internals().archive_capacity > cap0
    r.compress_scan(d_in.data_ptr(), eb, hist.data_ptr(), cz.Abs, radius)
    ptr, nb, st = r.compress_finish(0)
    assert st == cz.PSZ_SUCCESS
    two_call = d2h(ptr, nb).tobytes()
    sync()
    assert int(hist[:2 * radius].sum().item()) == data.size
    fresh = _manager(np.float32, dims, False, mode, None)
    single = _compress(fresh, d_in, eb, radius)
    if mode == "exact":
        assert two_call == single
    else:
        a, b = parse_archive(two_call), parse_archive(single)
        ha, hb = a["header"], b["header"]
        assert two_call[ha.entry[3]:ha.entry[4]] == single[hb.entry[3]:hb.entry[4]], "outlier segments differ"
        codes_o, _, _ = oracle.lorenzo_c(data, dims, eb, radius)
        books = oracle.book_twoqueue(oracle.histogram(codes_o, 2 * radius), 2 * radius, smooth=0)
        seg_o, info = oracle.phf_segment(codes_o, 2 * radius, sublen=a["sublen"], books=books)
        check_phf_against_oracle(a, info, seg_o, cz.LAYOUT_BRICK)
        outs = []
        for arch in (two_call, single):
            d_arch = to_device(np.frombuffer(arch, np.uint8).copy())
            rx = cz.Resource(None, None, header=cz.psz_header.from_buffer_copy(arch[:176]))
            outs.append(full_decompress(rx, d_arch, len(arch), data.size, np.float32))
            rx.close()
        np.testing.assert_array_equal(outs[0], outs[1])
    fresh.close()
    r.close()
