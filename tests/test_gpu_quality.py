"""Quality assessment on the device (psz_amd_assess_quality_*, include/cusz_amd.h) against the model
(quality_model.py: two passes, sums in numpy.longdouble) and its derived tolerances: the edges of
the kernel's own units and of pointer alignment, planted extrema and ties, identical and constant
arrays, non-finite values, ill-conditioned fields, the autocorrelations, the region variant, a
compress round trip, the manager's state, indices past 2^32 and the CLI's report.

The lengths are named from the constants the launch uses (quality_reduce.hh through the CPU shim).
A model result is computed once per (field, length) and shared by the cases that need it."""
import ctypes as C
import math
import re
import subprocess

import numpy as np
import pytest
import torch

import cusz_amd as cz
import quality_model as qm
from gpu_util import d2h, sync, to_device
from test_quality_host import shim  # noqa: F401  (the fixture: the header's constants)

pytestmark = pytest.mark.gpu

DTYPES = {"f32": np.float32, "f64": np.float64}
EDGE_FIELD = {"f32": "ramp_f32", "f64": "offset_f64"}
UNITS = ("vec", "wave", "block", "cap", "trip2")
EDGE_LENGTHS = ["1", "2", "3"] + [f"{u}{d}" for u in UNITS for d in ("-1", "", "+1")]
OFFSETS = {"aligned": (0, 0), "o+1": (1, 0), "x+1": (0, 1), "both+1": (1, 1)}

_managers, _cache = {}, {}


def manager(dt):
    """One manager per element type; the assessed lengths have nothing to do with its field."""
    if dt not in _managers:
        _managers[dt] = cz.Resource(cz.F4 if dt == "f32" else cz.F8, (512, 1, 1))
    return _managers[dt]


def units(shim, dt):  # noqa: F811
    """Elements in one 16-byte vector, one wave's and one workgroup's trip, the shortest length at
    which the grid has reached its cap, and the shortest at which a lane makes a second trip."""
    k = (C.c_int * 5)()
    shim.qr_shim_constants(k)
    block, wave, vec_bytes, vecs, cap = list(k)
    es = np.dtype(DTYPES[dt]).itemsize
    item = vecs * vec_bytes // es
    u = {"vec": vec_bytes // es, "item": item, "wave": wave * item, "block": block * item,
         "cap": ((cap - 1) * block + 1) * item, "trip2": (cap * block + 1) * item}
    assert shim.qr_shim_grid(u["cap"] - 1, es) == cap - 1 and shim.qr_shim_grid(u["cap"], es) == cap
    return u


def length(shim, dt, name):  # noqa: F811
    m = re.fullmatch(r"([a-z0-9]+?)([+-]1)?", name)
    base = int(m.group(1)) if m.group(1).isdigit() else units(shim, dt)[m.group(1)]
    return base + int(m.group(2) or 0)


def field(name, n, nmax):
    """The first n elements of the seeded field of nmax elements, and the model's result for them."""
    if (name, nmax) not in _cache:
        o, x, eb = qm.field(name, nmax)
        o.setflags(write=False), x.setflags(write=False)
        _cache[name, nmax] = (o, x, eb)
    o, x, eb = _cache[name, nmax]
    if (name, nmax, n) not in _cache:
        _cache[name, nmax, n] = qm.assess(x[:n], o[:n], eb, autocor=True)
    return o[:n], x[:n], eb, _cache[name, nmax, n]


def device(a, shift=0):
    """(tensor, address): a on the device, `shift` elements past a 16-byte aligned address."""
    t = torch.empty(a.size + shift, dtype=torch.float32 if a.dtype == np.float32 else torch.float64, device="cuda")
    assert t.data_ptr() % 16 == 0
    t[shift:].copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return t, t.data_ptr() + shift * a.itemsize


def assess(x, o, eb, autocor=False, o_shift=0, x_shift=0):
    dt = "f32" if o.dtype == np.float32 else "f64"
    to, po = device(o, o_shift)
    tx, px = device(x, x_shift)
    sync()
    return manager(dt).assess_quality(px, po, o.size, eb, autocor)


def agree(q, x, o, eb, autocor=False):
    bad = qm.check(q, qm.assess(x, o, eb, autocor))
    assert bad == [], bad


# ---- 1. edges of the kernel's units, every alignment ------------------------------------------------
@pytest.mark.parametrize("align", list(OFFSETS))
@pytest.mark.parametrize("name", EDGE_LENGTHS)
@pytest.mark.parametrize("dt", list(DTYPES))
def test_unit_edges_and_alignment(shim, dt, name, align):  # noqa: F811
    n = length(shim, dt, name)
    o, x, eb, want = field(EDGE_FIELD[dt], n, units(shim, dt)["trip2"] + 1)
    o_shift, x_shift = OFFSETS[align]
    q = assess(x, o, eb, True, o_shift, x_shift)
    bad = qm.check(q, want)
    assert bad == [], bad


# ---- 2. planted extrema -----------------------------------------------------------------------------
def planted(shim, dt):  # noqa: F811
    """An exact copy over three workgroups' trips, one more item and a three-element tail."""
    u = units(shim, dt)
    n = 3 * u["block"] + u["item"] + 3
    o, _, eb, _ = field(EDGE_FIELD[dt], n, units(shim, dt)["trip2"] + 1)
    return u, n, o.copy(), o.copy(), eb


@pytest.mark.parametrize("where", ["first", "last", "tail", "last_workgroup"])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_largest_error_is_found_where_it_is_planted(shim, dt, where):  # noqa: F811
    u, n, o, x, eb = planted(shim, dt)
    i = {"first": 0, "last": n - 1, "tail": n - 2, "last_workgroup": 3 * u["block"] + 2}[where]
    x[i] = o[i] + o.dtype.type(3.0)
    x[n // 2] = o[n // 2] + o.dtype.type(1.0)  # a smaller one elsewhere
    q = assess(x, o, eb)
    assert q.stat.max_err_idx == i and q.first_diff_idx == min(i, n // 2) and q.n_unbounded == 2
    agree(q, x, o, eb)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_equal_errors_in_two_workgroups_lowest_index_wins(shim, dt):  # noqa: F811
    u, n, o, x, eb = planted(shim, dt)
    lo, hi = u["block"] + 3, 2 * u["block"] + u["item"] + 2  # workgroups 1 and 2
    for i in (hi, lo):
        o[i], x[i] = 1.0, 1.5
    q = assess(x, o, eb)
    assert (q.stat.max_err_idx, q.stat.max_err_abs, q.first_unbounded_idx, q.n_unbounded) == (lo, 0.5, lo, 2)
    agree(q, x, o, eb)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_planted_extrema_bound_breakers_and_no_bound(shim, dt):  # noqa: F811
    u, n, o, x, eb = planted(shim, dt)
    o[7], o[n - 1] = -1e6, 1e6
    x[7], x[n - 1] = -1e6, 1e6
    x[u["block"] + 1], x[n - 3] = -2e6, 3e6
    q = assess(x, o, eb)
    assert (q.stat.odata.min, q.stat.odata.max, q.stat.xdata.min, q.stat.xdata.max) == (-1e6, 1e6, -2e6, 3e6)
    agree(q, x, o, eb)
    u, n, o, x, eb = planted(shim, dt)
    idx = (2 * u["block"] + 9, u["wave"] + 1, n - 1)
    for i in idx:
        x[i] = o[i] + o.dtype.type(2 * eb)
    q = assess(x, o, eb)
    assert (q.n_unbounded, q.first_unbounded_idx, q.first_diff_idx) == (3, min(idx), min(idx))
    agree(q, x, o, eb)
    q = assess(x, o, 0.0)
    assert (q.n_unbounded, q.first_unbounded_idx, q.first_diff_idx) == (0, cz.SIZE_MAX, min(idx))
    agree(q, x, o, 0.0)


# ---- 3. identical arrays ----------------------------------------------------------------------------
@pytest.mark.parametrize("dt", list(DTYPES))
def test_identical_constant_and_one_flipped_bit(shim, dt):  # noqa: F811
    u, n, o, x, eb = planted(shim, dt)
    q = assess(x, o, eb)
    assert (q.stat.score_MSE, q.stat.score_PSNR, q.first_diff_idx, q.n_unbounded) == (0.0, math.inf, cz.SIZE_MAX, 0)
    agree(q, x, o, eb)
    c = np.full(n, 2.5, DTYPES[dt])
    q = assess(c, c, eb)
    assert math.isnan(q.stat.score_coeff) and q.stat.odata.std == 0 and q.stat.odata.rng == 0
    agree(q, c, c, eb)
    j = 2 * u["block"] + 77
    bits = x.view(np.uint32 if dt == "f32" else np.uint64)
    bits[j] ^= 1
    q = assess(x, o, eb)
    assert q.first_diff_idx == j and q.stat.max_err_idx == j and q.n_unbounded == 0
    agree(q, x, o, eb)


# ---- 4. non-finite values ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", list(DTYPES))
def test_non_finite_pairs_are_counted_and_left_out(shim, dt):  # noqa: F811
    u = units(shim, dt)
    n = 3 * u["block"] + u["item"] + 3
    o, x, eb, _ = field(EDGE_FIELD[dt], n, u["trip2"] + 1)
    o, x = o.copy(), x.copy()
    a, b, c = u["block"] + 2, 40, n - 2
    o[a], x[b] = np.nan, np.inf
    o[c] = x[c] = np.nan  # the same bits in both: not finite, not a difference
    q = assess(x, o, eb, True)
    want = qm.assess(x, o, eb, True)
    assert q.n_nonfinite == 3 and q.n_unbounded == want["n_unbounded"] and q.first_unbounded_idx <= b
    with np.errstate(invalid="ignore"):
        beyond = (np.abs(x.astype(np.float64) - o) > 1.001 * eb) & np.isfinite(x) & np.isfinite(o)
    assert want["n_unbounded"] == 2 + int(beyond.sum())  # the NaN in o and the Inf in x, not the shared NaN
    bad = qm.check(q, want)
    assert bad == [], bad
    nan = np.full(n, np.nan, DTYPES[dt])
    q = assess(nan, nan, eb, True)
    assert q.n_finite == 0 and q.n_nonfinite == n and q.n_unbounded == 0
    assert (q.stat.max_err_idx, q.first_unbounded_idx, q.first_diff_idx) == (cz.SIZE_MAX,) * 3
    for f in ("score_PSNR", "score_MSE", "score_NRMSE", "score_coeff", "max_err_abs", "autocor_lag_one"):
        assert math.isnan(getattr(q.stat, f))
    agree(q, nan, nan, eb, True)


# ---- 5. ill-conditioned fields: what sum v^2 / n - mean^2 cannot take -------------------------------
@pytest.mark.parametrize("name", ["offset_f32", "offset_f64"])
def test_ill_conditioned_fields(name):
    n = 2 ** 20 + 37
    o, x, eb, want = field(name, n, n)
    bad = qm.check(assess(x, o, eb, True), want)
    assert bad == [], bad


# ---- 6. autocorrelation ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ramp_f32", "white_f32", "white_f64"])
def test_autocorrelation(name):
    n = 70001
    if name == "ramp_f32":
        o, x, eb, want = field(name, n, n)
    else:
        o = np.random.default_rng(5).standard_normal(n).astype(DTYPES[name[-3:]])
        x, eb = o, 0.0
        want = qm.assess(x, o, eb, True)
    q = assess(x, o, eb, True)
    bad = qm.check(q, want)
    assert bad == [], bad
    assert abs(q.stat.autocor_lag_one) <= 1 and (name != "ramp_f32" or q.stat.autocor_lag_two > 0.99)
    plain = assess(x, o, eb, False)
    assert math.isnan(plain.stat.autocor_lag_one) and math.isnan(plain.stat.autocor_lag_two)
    plain.stat.autocor_lag_one, plain.stat.autocor_lag_two = q.stat.autocor_lag_one, q.stat.autocor_lag_two
    assert bytes(plain) == bytes(q)


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_autocorrelation_of_the_shortest_arrays(dt, n):
    o = np.array([1.0, 3.0, 2.0][:n], DTYPES[dt])
    q = assess(o, o, 0.0, True)
    assert math.isnan(q.stat.autocor_lag_one) == (n < 3)  # two elements: one pair, zero std
    assert math.isnan(q.stat.autocor_lag_two)
    agree(q, o, o, 0.0, True)


# ---- 7. region ----------------------------------------------------------------------------------------
REGION_FIELDS = {"3d": (70, 9, 5), "2d": (300, 7, 1), "1d": (1000, 1, 1)}


def boxes(dims):
    odd = tuple((max(d // 3, 1) | 1) if d > 2 else 0 for d in dims), tuple(max((d // 2 - 1) | 1, 1) if d > 2 else 1 for d in dims)
    far = tuple(max(d // 4, 1) for d in dims)
    return {"origin": ((0, 0, 0), tuple(max(d // 2, 1) for d in dims)),
            "far_corner": (tuple(d - e for d, e in zip(dims, far)), far),
            "element": (tuple(d // 2 for d in dims), (1, 1, 1)),
            "whole": ((0, 0, 0), dims),
            "interior_odd": odd}


@pytest.mark.parametrize("box", ["origin", "far_corner", "element", "whole", "interior_odd"])
@pytest.mark.parametrize("shape", list(REGION_FIELDS))
@pytest.mark.parametrize("dt", list(DTYPES))
def test_region_against_the_cropped_box(dt, shape, box):
    dims = REGION_FIELDS[shape]
    n = int(np.prod(dims))
    o, x, eb, _ = field(EDGE_FIELD[dt], n, n)
    (ox, oy, oz), (ex, ey, ez) = boxes(dims)[box]
    assert ox + ex <= dims[0] and oy + ey <= dims[1] and oz + ez <= dims[2]
    crop = lambda a: np.ascontiguousarray(a.reshape(dims[::-1])[oz:oz + ez, oy:oy + ey, ox:ox + ex]).ravel()  # noqa: E731
    ob, xb = crop(o), crop(x).copy()
    xb[xb.size // 2] += xb.dtype.type(0.5)  # the largest error, at a known index of the box
    to, po = device(o)
    tx, px = device(xb)
    sync()
    q = manager(dt).assess_quality_region(px, po, dims, (ox, oy, oz), (ex, ey, ez), eb, True)
    want = qm.assess(xb, ob, eb, True)
    assert q.stat.max_err_idx == xb.size // 2 == want["max_err_idx"] and q.stat.len == xb.size
    bad = qm.check(q, want)
    assert bad == [], bad


@pytest.mark.parametrize("dt", list(DTYPES))
def test_bad_arguments_leave_the_struct_untouched(dt):
    L, r = cz.lib(), manager(dt)
    o = np.arange(64, dtype=DTYPES[dt])
    to, po = device(o)
    sync()
    f = L.psz_amd_assess_quality_float if dt == "f32" else L.psz_amd_assess_quality_double
    g = L.psz_amd_assess_quality_region_float if dt == "f32" else L.psz_amd_assess_quality_region_double
    q = cz.psz_amd_quality()
    C.memset(C.byref(q), 0xA5, C.sizeof(q))
    before = bytes(q)
    P = C.c_void_p
    for args in ((None, P(po), P(po), 64, 0.0, 0), (r._h, None, P(po), 64, 0.0, 0), (r._h, P(po), None, 64, 0.0, 0),
                 (r._h, P(po), P(po), 0, 0.0, 0), (r._h, P(po), P(po), 64, -1e-3, 0),
                 (r._h, P(po), P(po), 64, math.nan, 0), (r._h, P(po), P(po), 64, 0.0, 2), (r._h, P(po), P(po), 64, 0.0, -1)):
        assert f(*args, C.byref(q)) == cz.PSZ_AMD_ERR_INVALID_ARG
    assert f(r._h, P(po), P(po), 64, 0.0, 0, None) == cz.PSZ_AMD_ERR_INVALID_ARG
    dims = cz.psz_len(8, 4, 2)
    for origin, extent in (((0, 0, 0), (0, 1, 1)), ((0, 0, 0), (9, 1, 1)), ((7, 0, 0), (2, 1, 1)), ((0, 4, 0), (1, 1, 1)),
                           ((0, 0, 1), (8, 4, 2)), ((8, 0, 0), (1, 1, 1))):
        assert g(r._h, P(po), P(po), dims, cz.psz_len(*origin), cz.psz_len(*extent), 0.0, 0, C.byref(q)) == cz.PSZ_AMD_ERR_INVALID_ARG
    assert bytes(q) == before
    assert g(r._h, P(po), P(po), dims, cz.psz_len(0, 0, 0), dims, 0.0, 0, C.byref(q)) == cz.PSZ_SUCCESS and q.stat.len == 64


def smooth(dims, dtype):
    """A compressible field of magnitude <= 1 (x fastest)."""
    z, y, xx = np.meshgrid(*(np.arange(d) for d in dims[::-1]), indexing="ij")
    data = (0.6 * np.sin(0.05 * xx + 0.3 * y) * np.cos(0.2 * z) + 0.3 * np.sin(0.011 * xx * y)).astype(dtype).ravel()
    assert np.abs(data).max() <= 1
    return data


# ---- 8. round trip -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,dt", [((256, 16, 16), "f32"), ((64, 24, 17), "f64")])
def test_compress_decompress_assess(oracle, dims, dt):
    eb, n = 1e-3, int(np.prod(dims))
    data = smooth(dims, DTYPES[dt])
    codes, ol_val, ol_idx = oracle.lorenzo_c(data, dims, eb)
    ref = oracle.lorenzo_x(codes, ol_val, ol_idx, dims, eb, dtype=DTYPES[dt])
    assert np.abs(ref.astype(np.float64) - data).max() <= 1.001 * eb  # the premise: the oracle keeps the bound
    r = cz.Resource(cz.F4 if dt == "f32" else cz.F8, dims)
    d_in = to_device(data)
    ptr, nbytes, _ = r.compress(d_in.data_ptr(), eb)
    d_arch = to_device(d2h(ptr, nbytes).copy())
    d_out = torch.zeros(n, dtype=d_in.dtype, device="cuda")
    r.decompress(d_arch.data_ptr(), nbytes, d_out.data_ptr())
    q = r.assess_quality(d_out.data_ptr(), d_in.data_ptr(), n, eb)
    out = d_out.cpu().numpy()
    assert q.n_unbounded == 0 and q.first_unbounded_idx == cz.SIZE_MAX and q.n_finite == n
    assert q.stat.max_err_abs == np.abs(out.astype(np.float64) - data).max() <= 1.001 * eb
    agree(q, out, data, eb)
    origin, extent = (dims[0] // 4 + 1, 3, 5), (dims[0] // 2 - 1, 7, 9)
    nb = int(np.prod(extent))
    d_box = torch.zeros(nb, dtype=d_in.dtype, device="cuda")
    r.decompress_region(d_arch.data_ptr(), nbytes, origin, extent, d_box.data_ptr())
    q = r.assess_quality_region(d_box.data_ptr(), d_in.data_ptr(), dims, origin, extent, eb)
    sl = tuple(slice(o, o + e) for o, e in zip(origin[::-1], extent[::-1]))
    ob, xb = data.reshape(dims[::-1])[sl].ravel(), out.reshape(dims[::-1])[sl].ravel()
    np.testing.assert_array_equal(d_box.cpu().numpy(), xb)
    assert q.n_unbounded == 0 and q.stat.len == nb and q.stat.max_err_abs == np.abs(xb.astype(np.float64) - ob).max()
    agree(q, xb, ob, eb)


# ---- 9. manager state ----------------------------------------------------------------------------------
def test_repeatable_no_allocation_and_a_pending_scan_survives():
    dims, eb = (256, 16, 16), 1e-3
    n = int(np.prod(dims))
    o = smooth(dims, np.float32)
    x = (o + np.random.default_rng(3).uniform(-eb, eb, n)).astype(np.float32)
    d_o, d_x = to_device(o), to_device(x)
    plain = cz.Resource(cz.F4, dims)
    plain.set_codebook(cz.CODEBOOK_EXACT)  # the book of the whole histogram, as a finish after a scan builds
    ptr, nbytes, _ = plain.compress(d_o.data_ptr(), eb)
    want = d2h(ptr, nbytes).tobytes()
    r = cz.Resource(cz.F4, dims)
    r.set_codebook(cz.CODEBOOK_EXACT)
    hist = torch.zeros(1025, dtype=torch.int32, device="cuda")
    r.compress_scan(d_o.data_ptr(), eb, hist.data_ptr())
    q1 = r.assess_quality(d_x.data_ptr(), d_o.data_ptr(), n, eb, True)  # the first call allocates the partials
    sync()
    free1, _ = torch.cuda.mem_get_info()
    q2 = r.assess_quality(d_x.data_ptr(), d_o.data_ptr(), n, eb, True)
    sync()
    free2, _ = torch.cuda.mem_get_info()
    assert bytes(q1) == bytes(q2) and free1 == free2
    ptr, nbytes, _ = r.compress_finish(0)
    assert d2h(ptr, nbytes).tobytes() == want


# ---- 10. past 32 bits ------------------------------------------------------------------------------------
def test_indices_past_32_bits():
    n = 2 ** 32 + 64
    need = 2 * 4 * n + (2 << 30)
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f"needs {need} bytes of device memory, {free} are free")
    o = torch.zeros(n, dtype=torch.float32, device="cuda")
    x = torch.zeros(n, dtype=torch.float32, device="cuda")
    big, small = 2 ** 32 + 5, 2 ** 31 + 1
    x[big], x[small] = 4.0, 2.0
    sync()
    q = manager("f32").assess_quality(x.data_ptr(), o.data_ptr(), n, 1.0)
    # every other pair is (0, 0): the sums are exact, so are the expected values
    assert (q.stat.max_err_idx, q.stat.max_err_abs, q.first_unbounded_idx, q.first_diff_idx) == (big, 4.0, small, small)
    assert (q.n_unbounded, q.n_finite, q.n_nonfinite, q.stat.len) == (2, n, 0, n)
    assert q.stat.score_MSE == 20.0 / n and q.stat.xdata.max == 4.0 and q.stat.xdata.min == 0.0
    assert q.stat.odata.std == 0 and math.isnan(q.stat.score_coeff) and math.isnan(q.stat.max_err_pwrrel)
    # the model's tolerances (quality_model.check) with kappa = avg / std < 1
    assert abs(q.stat.xdata.avg - 6.0 / n) <= 8 * n * qm.U * 4.0
    assert abs(q.stat.xdata.std / math.sqrt(20.0 / n - (6.0 / n) ** 2) - 1) <= 8 * (n + 1) * qm.U


# ---- 11. CLI ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("region", [None, "10,3,2:200,9,11"])
def test_cli_reports_from_the_device(tmp_path, region):
    dims = (256, 16, 16)
    z, y, xx = np.meshgrid(*(np.arange(d) for d in dims[::-1]), indexing="ij")
    data = (np.sin(0.05 * xx + 0.3 * y) * np.cos(0.2 * z)).astype(np.float32)
    f = tmp_path / "field.f32"
    data.tofile(f)
    zr = subprocess.run([cz.CLI_PATH, "-z", "-t", "f32", "-m", "abs", "-e", "1e-3", "-l", "256x16x16", "-i", str(f)],
                        capture_output=True, text=True, timeout=120)
    assert zr.returncode == 0, zr.stderr
    cmd = [cz.CLI_PATH, "-x", "-i", str(f) + ".cusza", "--origin", str(f)] + (["--region", region] if region else [])
    xr = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert xr.returncode == 0, xr.stderr
    lines = xr.stdout.splitlines()
    k = next(i for i, ln in enumerate(lines) if ln.startswith("max-error"))
    m = re.search(r"max-error ([0-9.e+-]+)", lines[k])
    assert m and 0 < float(m.group(1)) <= 1.001e-3 and ", bounded)" in lines[k] and "PSNR" in lines[k] and "NRMSE" in lines[k]
    assert "n_unbounded 0" in lines[k + 1] and "coeff" in lines[k + 1] and "n_nonfinite 0" in lines[k + 1]
    out = np.fromfile(str(f) + ".cuszx", np.float32)
    if region:
        ob = data[2:13, 3:12, 10:210].ravel()
    else:
        ob = data.ravel()
    assert float(m.group(1)) == float(f"{np.abs(out.astype(np.float64) - ob).max():.6e}")
