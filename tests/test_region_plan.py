"""psz_amd_region_plan (host only, no GPU): the box is validated against the header's field, the
path is the header's verdict, and the covering bricks (256 x 8 x 8) are those a brute-force numpy
marking of the box's elements gives."""
import numpy as np
import pytest

import cusz_amd as cz

FIELDS = [(512, 24, 24), (256, 20, 13)]
BW, BH = 256, 8  # brick width (x), brick height and depth (y, z)


def _header(dims, dtype=cz.F4, predictor=cz.Lorenzo, sublen=256, radius=512):
    h = cz.psz_header()
    x, y, z = (tuple(dims) + (1, 1, 1))[:3]
    h.dtype = dtype
    h.pipeline.predictor = predictor
    h.rc.radius = radius
    h.vle_sublen = sublen
    h.vle_pardeg = (x * y * z + sublen - 1) // sublen
    h.len = cz.psz_len(x, y, z)
    return h


def _covering_bricks(dims, o, e):
    """(lo, n, count) of the bricks holding an element of the box, by marking every element."""
    x, y, z = dims
    hit = np.zeros((z, y, x), bool)
    hit[o[2]:o[2] + e[2], o[1]:o[1] + e[1], o[0]:o[0] + e[0]] = True
    nb = ((z + BH - 1) // BH, (y + BH - 1) // BH, x // BW)
    pad = np.zeros((nb[0] * BH, nb[1] * BH, nb[2] * BW), bool)
    pad[:z, :y, :x] = hit
    per = pad.reshape(nb[0], BH, nb[1], BH, nb[2], BW).any(axis=(1, 3, 5))  # [bz, by, bx]
    bz, by, bx = np.nonzero(per)
    lo = (bx.min(), by.min(), bz.min())
    n = (bx.max() - lo[0] + 1, by.max() - lo[1] + 1, bz.max() - lo[2] + 1)
    return lo, n, int(per.sum())


def _random_boxes(dims, count, rng):
    for _ in range(count):
        o = [int(rng.integers(0, d)) for d in dims]
        e = [int(rng.integers(1, d - a + 1)) for d, a in zip(dims, o)]
        if rng.random() < 0.3:  # small boxes near brick borders
            e = [min(x, int(rng.integers(1, 12))) for x in e]
        yield o, e


@pytest.mark.parametrize("dims", FIELDS, ids=["512x24x24", "256x20x13"])
def test_plan_matches_brute_force(dims):
    rng = np.random.default_rng(sum(dims))
    h = _header(dims)
    boxes = list(_random_boxes(dims, 100, rng))
    boxes += [([0, 0, 0], list(dims)), ([dims[0] - 1, dims[1] - 1, dims[2] - 1], [1, 1, 1]), ([max(dims[0] - 257, 0), 7, 7], [2, 2, 2])]  # (512: across the x brick border)
    for o, e in boxes:
        p = cz.region_plan(h, o, e)
        lo, n, count = _covering_bricks(dims, o, e)
        assert p.path == cz.REGION_FUSED, (o, e)
        assert (p.brick_lo.x, p.brick_lo.y, p.brick_lo.z) == lo, (o, e)
        assert (p.brick_n.x, p.brick_n.y, p.brick_n.z) == n, (o, e)
        assert p.bricks == count == n[0] * n[1] * n[2], (o, e)
        assert p.chunks == 64 * count, (o, e)
        assert p.elems == e[0] * e[1] * e[2], (o, e)


@pytest.mark.parametrize("origin,extent", [
    ((0, 0, 0), (0, 1, 1)), ((0, 0, 0), (1, 0, 1)), ((0, 0, 0), (1, 1, 0)),          # zero extent
    ((512, 0, 0), (1, 1, 1)), ((0, 24, 0), (1, 1, 1)), ((0, 0, 24), (1, 1, 1)),      # origin >= len
    ((500, 0, 0), (13, 1, 1)), ((0, 20, 0), (1, 5, 1)), ((0, 0, 1), (512, 24, 24)),  # crosses the far face
    ((1, 0, 0), (2**64 - 1, 1, 1)),                                                  # origin + extent wraps
])
def test_plan_rejects_boxes_outside_the_field(origin, extent):
    h = _header((512, 24, 24))
    o = cz.psz_amd_region_info()
    st = cz.lib().psz_amd_region_plan(h, cz.psz_len(*origin), cz.psz_len(*extent), o)
    assert st == cz.PSZ_AMD_ERR_INVALID_ARG
    with pytest.raises(cz.PszError):
        cz.region_plan(h, origin, (extent[0] % 2**64, extent[1], extent[2]))


@pytest.mark.parametrize("dims,kw", [
    ((512, 24, 24), dict(sublen=1024)),              # another chunk length
    ((512, 24, 1), {}),                              # 2-D
    ((50_000, 1, 1), {}),                            # 1-D
    ((96, 64, 40), {}),                              # x no multiple of the brick width
    ((512, 24, 24), dict(predictor=cz.LorenzoZigZag)),
    ((512, 24, 24), dict(predictor=cz.Spline)),
], ids=["sublen1024", "2d", "1d", "x96", "zigzag", "spline"])
def test_plan_reports_fallback(dims, kw):
    h = _header(dims, **kw)
    p = cz.region_plan(h, (0, 0, 0), (min(dims[0], 5), 1, 1))
    assert p.path == cz.REGION_FALLBACK
    assert (p.brick_lo.x, p.brick_lo.y, p.brick_lo.z, p.brick_n.x, p.brick_n.y, p.brick_n.z) == (0,) * 6
    assert p.bricks == 0 and p.chunks == h.vle_pardeg and p.elems == min(dims[0], 5)


def test_plan_f64_is_fused_too():
    p = cz.region_plan(_header((512, 16, 16), dtype=cz.F8, radius=64), (250, 7, 7), (13, 2, 2))
    assert p.path == cz.REGION_FUSED and p.bricks == 2 * 2 * 2
