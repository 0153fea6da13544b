"""The codebook sample inside pass 1 (3-D bricks) is accepted by value: the wave that completes it
re-reads the sample histogram until its bins sum to the number of sample-brick elements inside
the field, which brick_configure works out from the shape (brick_scan.hip finish_brick).

What can go wrong, and what shows it:
  * a sample handed over early or incomplete, or a total that is too small: the host builds
    another (valid) book.  So the archive's revbook, every chunk's bit count and every chunk's
    cells are compared with the oracle encoder's output for the oracle-computed book of the
    complete sample (gpu_util.expected_books), the contract of test_gpu_sampled.py -- here on
    shapes whose bricks are ragged in y and z at every sample stride (1, 3, 5), which that file
    does not have and which are the cases of the host-side row count.
  * a total that is too large: the wave gives up after a bound of about 0.1 s of re-reads and hands
    over the complete sample, so no byte changes; it shows only as time.  A compress of these
    fields takes about a millisecond, so 20 ms separates the two whatever the machine's load.
"""
import time

import numpy as np
import pytest

import cusz_amd as cz
from cusz_amd import datagen
from gpu_util import chunk_cells, d2h, expected_books, parse_archive, to_device

pytestmark = pytest.mark.gpu

SHAPES = [
    (256, 13, 11),     # 4 bricks, every one sampled, ragged in y and z
    (256, 9, 203),     # 52 bricks, every one sampled, ragged in y and z
    (768, 133, 125),   # 816 bricks: every 3rd sampled, ragged in y and z
    (512, 203, 197),   # 1300 bricks: every 5th sampled, ragged in y and z
]
EB, RADIUS = 1e-4, 512


@pytest.mark.parametrize("dims", SHAPES, ids=["x".join(map(str, d)) for d in SHAPES])
def test_sample_complete_and_prompt(oracle, dims):
    n = int(np.prod(dims))
    data = datagen.smooth3d_np(dims, sum(dims))
    d_in = to_device(data)
    r = cz.Resource(cz.F4, dims)
    ptr, nbytes, _ = r.compress(d_in.data_ptr(), EB, cz.Abs, RADIUS)  # also the warm-up: first-use allocations
    first = d2h(ptr, nbytes).tobytes()
    layout = r.internals().layout
    assert layout == cz.LAYOUT_BRICK
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        ptr, nbytes, _ = r.compress(d_in.data_ptr(), EB, cz.Abs, RADIUS)
        times.append(time.perf_counter() - t0)
        assert d2h(ptr, nbytes).tobytes() == first

    # the book is the one of the complete sample: the oracle's encoding with it, chunk by chunk
    a = parse_archive(first)
    codes_o, _, _ = oracle.lorenzo_c(data, dims, EB, RADIUS, False)
    bklen = 2 * RADIUS
    book, rv = expected_books(oracle, r, codes_o, dims, bklen, layout)
    nbit_o, entry_o, bs_o, tot_o = oracle.hf_encode(codes_o, book, 256)
    np.testing.assert_array_equal(a["revbook"], rv)
    np.testing.assert_array_equal(a["par_nbit"], nbit_o)
    ours, _ = chunk_cells(a["par_nbit"], a["par_entry"], a["bitstream"])
    ref, _ = chunk_cells(nbit_o, entry_o, bs_o)
    np.testing.assert_array_equal(ours, ref)
    assert a["total_nbit"] == tot_o
    dec = oracle.hf_decode(a["bitstream"], a["revbook"], a["par_nbit"], a["par_entry"], 256, n, bklen)
    np.testing.assert_array_equal(dec, codes_o)
    r.close()

    print(f"{dims}: compress wall times {[round(t * 1e3, 3) for t in times]} ms")
    assert min(times) < 0.020, times
