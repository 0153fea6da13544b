"""The delta fields (delta_fields.py) on the CPU: for every (shape, radius, dtype, predictor) that
test_gpu_lorenzo_matrix.py compresses one for, the oracle's codes, outlier cells and reconstruction
equal the closed form, and the field meets the conditions the GPU tests rely on."""
import numpy as np
import pytest

import delta_fields as df
from edge_fields import tile_of

CASES = df.delta_cases()


def _id(c):
    d, r, dt, zz = c
    return f"{'x'.join(map(str, d))}-r{r}-{np.dtype(dt).name}-{'zigzag' if zz else 'plain'}"


def test_vector_width_table():
    table = {  # (dtype, lx): V, written out from lorenzo.hip lorenzo_geom
        (np.float32, 260): 4, (np.float32, 130): 2, (np.float32, 65): 1, (np.float32, 66): 2, (np.float32, 33): 1,
        (np.float32, 35): 1, (np.float32, 45): 1, (np.float32, 4): 4, (np.float32, 2): 2, (np.float32, 1): 1,
        (np.float32, 256): 4, (np.float32, 40): 4, (np.float32, 7): 1, (np.float32, 6): 2,
        (np.float64, 260): 2, (np.float64, 130): 2, (np.float64, 65): 1, (np.float64, 66): 2, (np.float64, 33): 1,
        (np.float64, 35): 1, (np.float64, 45): 1, (np.float64, 4): 2, (np.float64, 2): 2, (np.float64, 1): 1,
        (np.float64, 256): 2, (np.float64, 40): 2, (np.float64, 7): 1, (np.float64, 6): 2,
    }
    for (dt, lx), v in table.items():
        assert df.vector_width(dt, lx) == v, (dt, lx)


def test_zigzag_is_the_int16_formula():
    d = np.arange(-600, 601)
    want = ((d.astype(np.int16) << 1) ^ (d.astype(np.int16) >> 15)).astype(np.uint16)
    np.testing.assert_array_equal(df.zigzag(d).astype(np.uint16), want)


def test_integrate_restarts_at_tile_borders():
    """Differencing inside the tile (edge_fields.lorenzo_deltas, plain numpy) gives the deltas back."""
    from edge_fields import lorenzo_deltas

    for dims, order in (((70, 1, 1), "x"), ((2100, 1, 1), "x"), ((70, 45, 1), "yx"), ((19, 11, 21), "zxy")):
        d = df.draw_deltas(dims, 512)
        f = df.integrate(d, dims).astype(np.float64)
        np.testing.assert_array_equal(lorenzo_deltas(f, dims, 0.5, order), d)
    assert tile_of((70, 1, 1)) == (1024, 1, 1)


@pytest.mark.parametrize("case", CASES, ids=map(_id, CASES))
def test_oracle_equals_closed_form(oracle, case):
    dims, radius, dtype, zz = case
    n = int(np.prod(dims))
    data, codes, idx, val = df.delta_field(dims, radius, dtype, zz)
    assert data.dtype == dtype and data.size == n
    # the conditions the GPU cases rely on
    if n >= df.OUTLIER_FROM:
        assert 0 < idx.size <= n // 20, "outliers present, and under 5 %: the growth path is not entered"
    else:
        assert idx.size == 0
    if n >= 40 * radius:
        ends = np.array([radius - 1, -(radius - 1)])  # the extreme in-range deltas
        present = np.delete(codes, idx)
        assert np.isin(df.zigzag(ends) if zz else ends + radius, present).all(), "both extreme in-range codes occur"
    # the oracle against the closed form
    codes_o, ov_o, oi_o = oracle.lorenzo_c(data, dims, 0.5, radius, zz)
    np.testing.assert_array_equal(codes_o, codes)
    np.testing.assert_array_equal(oi_o, idx)
    np.testing.assert_array_equal(ov_o.view(np.uint32), val.view(np.uint32))
    xo = oracle.lorenzo_x(codes_o, ov_o, oi_o, dims, 0.5, radius, zz, dtype)
    np.testing.assert_array_equal(xo.view(np.uint8), data.view(np.uint8))


def test_single_outlier_element(oracle):
    for zz in (False, True):
        data, codes, idx, val = df.delta_field((1, 1, 1), 512, np.float32, zz, planted={0: 3 * 512})
        assert data[0] == 1536 and codes[0] == 0 and idx.tolist() == [0] and val[0] == (1536 if zz else 2048)
        codes_o, ov_o, oi_o = oracle.lorenzo_c(data, (1, 1, 1), 0.5, 512, zz)
        assert codes_o.tolist() == [0] and oi_o.tolist() == [0] and ov_o[0] == val[0]
