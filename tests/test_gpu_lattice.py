"""Lattice values through every layout (edge_fields.lattice_field; test_edge_fields.py checks what
each flavour contains): deltas exactly on the outlier predicate |delta| < radius and on the code
extremes, rounding ties and their float neighbours, -0.0 and a denormal, and -- "order" --
magnitudes from 2^23 (f64: 2^52) up, where differences and partial sums round and only the
reference's operation order (z-, x-, y-difference in compress; the shuffle-scan order in
reconstruct) gives the oracle's bits.  All of them sit on the kernels' structural seams.

Every case is run_roundtrip's bit-exact contract.  "exact" and "ties" are also held against the
closed form -- the input itself, round-half-away of it -- so that a mistake the oracle shares with
the kernels cannot hide.
"""
import numpy as np
import pytest
import torch

import cusz_amd as cz
import edge_fields as ef
from gpu_util import empty_device, sync, to_device
from test_gpu_parity import run_roundtrip
from test_gpu_sampled import sampled_roundtrip

pytestmark = pytest.mark.gpu

# dims, layout
SHAPES = [
    ((512, 16, 9), None),                       # 2 x 2 x 2 bricks, ragged z
    ((256, 13, 11), None),                      # ragged y and z
    ((40, 24, 17), None),                       # reference layout
    ((300, 40, 1), cz.LAYOUT_BRICK_FORCE),      # 2-D linear bricks
    ((70, 45, 1), None),                        # 2-D reference layout
    ((33068, 1, 1), cz.LAYOUT_BRICK),           # 1-D, three linear bricks (the last ragged)
    ((33068, 1, 1), cz.LAYOUT_REFERENCE),
]
# flavour, radius
FLAVOURS = [("exact", 512), ("exact", 64), ("ties", 512), ("near_ties", 512), ("order", 512)]
# the layout each shape is here for (x a multiple of 256 in 3-D: bricks)
EXPECT_LAYOUT = [cz.LAYOUT_BRICK, cz.LAYOUT_BRICK, cz.LAYOUT_REFERENCE, cz.LAYOUT_BRICK, cz.LAYOUT_REFERENCE,
                 cz.LAYOUT_BRICK, cz.LAYOUT_REFERENCE]
SHAPE_IDS = ["x".join(map(str, d)) + {None: "", 0: "-brick", 1: "-reference", 2: "-forced"}[l] for d, l in SHAPES]


@pytest.mark.parametrize("shape,expect", zip(SHAPES, EXPECT_LAYOUT), ids=SHAPE_IDS)
def test_shapes_take_the_layout_they_are_here_for(shape, expect):
    dims, layout = shape
    r = cz.Resource(cz.F4, dims)
    if layout is not None:
        r.set_layout(layout)
    d_in = to_device(np.zeros(int(np.prod(dims)), np.float32))
    r.compress(d_in.data_ptr(), 0.5)
    assert r.internals().layout == expect
    r.close()


def _decompress(arch, n, dtype):
    """The archive through a manager made from its header alone -> the field."""
    d_arch = to_device(np.frombuffer(arch, np.uint8).copy())
    r = cz.Resource(None, None, header=cz.psz_header.from_buffer_copy(arch[:176]))
    out = empty_device(n, torch.float32 if dtype == np.float32 else torch.float64)
    out.fill_(float("nan"))
    r.decompress(d_arch.data_ptr(), len(arch), out.data_ptr())
    sync()
    r.close()
    return out.cpu().numpy()


def _closed_form(flavour, data, got):
    if flavour == "exact":  # integers at eb = 0.5, every operation exact: the input, bit for bit
        np.testing.assert_array_equal(got.view(np.uint8), data.view(np.uint8))
    elif flavour == "ties":  # (values: Lorenzo codes carry no sign of zero)
        np.testing.assert_array_equal(got, ef.round_half_away(data))


@pytest.mark.parametrize("zz", [False, True], ids=["plain", "zigzag"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("flavour,radius", FLAVOURS, ids=[f"{f}-r{r}" for f, r in FLAVOURS])
@pytest.mark.parametrize("dims,layout", SHAPES, ids=SHAPE_IDS)
def test_lattice(oracle, dims, layout, flavour, radius, dtype, zz):
    data = ef.lattice_field(dims, dtype, flavour, radius)
    arch, a = run_roundtrip(oracle, data, dims, ef.lattice_eb(flavour), dtype, zz, radius,
                            check_bound=flavour != "order", layout=layout)
    _closed_form(flavour, data, _decompress(arch, data.size, dtype))


@pytest.mark.parametrize("zz", [False, True], ids=["plain", "zigzag"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("flavour", ["exact", "order"])
def test_lattice_single_pass(oracle, flavour, dtype, zz):
    """The single-pass (CODEBOOK_STREAM) kernel predicts with code of its own."""
    dims = (512, 16, 9)
    data = ef.lattice_field(dims, dtype, flavour)
    arch = sampled_roundtrip(oracle, data, dims, dtype, 0.5, zz, 512, cz.CODEBOOK_STREAM)
    _closed_form(flavour, data, _decompress(arch, data.size, dtype))
