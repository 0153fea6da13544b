"""The quality assessment's host side, CPU-only: quality_reduce.hh compiled with g++ alone and walked
with the kernel's partition and combine order (tests/host/quality_reduce_shim.cc) against the model
(quality_model.py), psz_amd_quality_merge through the library, the exports and the struct's size."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import cusz_amd as cz
import quality_model as qm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = [1000, 70001, 2 ** 20 + 37]
NEW_SYMBOLS = ["psz_amd_assess_quality_float", "psz_amd_assess_quality_double",
               "psz_amd_assess_quality_region_float", "psz_amd_assess_quality_region_double",
               "psz_amd_quality_merge"]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("quality") / "libqrshim.so"
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "cusz_amd", "csrc"), "-o", str(out),
           os.path.join(ROOT, "tests", "host", "quality_reduce_shim.cc")]
    try:
        subprocess.run(cmd, check=True, capture_output=True, timeout=120)
    except OSError as e:
        pytest.skip(f"g++ unavailable: {e}")
    except subprocess.CalledProcessError as e:
        pytest.fail(f"quality_reduce.hh does not compile with g++ alone:\n{e.stderr.decode()}")
    lib = C.CDLL(str(out))
    lib.qr_shim_assess.restype = C.c_int
    lib.qr_shim_assess.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_int,
                                   C.POINTER(cz.psz_amd_quality)]
    lib.qr_shim_grid.restype = C.c_uint
    lib.qr_shim_grid.argtypes = [C.c_size_t, C.c_int]
    lib.qr_shim_sizeof.restype = C.c_size_t
    return lib


def shim_assess(shim, x, o, eb, autocor=False):
    q = cz.psz_amd_quality()
    st = shim.qr_shim_assess(x.ctypes.data, o.ctypes.data, o.size, int(o.dtype == np.float64), eb,
                             cz.QUALITY_AUTOCOR if autocor else 0, C.byref(q))
    assert st == 0
    return q


_fields = {}


def case(name, n):
    """(o, x, eb, the model's result): computed once, shared, never modified."""
    if (name, n) not in _fields:
        o, x, eb = qm.field(name, n)
        o.setflags(write=False), x.setflags(write=False)
        _fields[name, n] = (o, x, eb, qm.assess(x, o, eb, autocor=True))
    return _fields[name, n]


def test_partition_constants_come_from_the_header(shim):
    k = (C.c_int * 5)()
    shim.qr_shim_constants(k)
    block, wave, vec_bytes, vecs, cap = list(k)
    assert block % wave == 0 and wave == 64 and vec_bytes == 16 and vecs >= 2
    for es in (4, 8):
        item = vecs * vec_bytes // es
        assert shim.qr_shim_grid(1, es) == 1
        assert shim.qr_shim_grid(block * item, es) == 1 and shim.qr_shim_grid(block * item + item, es) == 2
        assert shim.qr_shim_grid(cap * block * item, es) == cap == shim.qr_shim_grid(2 ** 33, es)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", sorted(qm.FIELDS))
def test_scheme_agrees_with_the_model(shim, name, n):
    o, x, eb, want = case(name, n)
    got = shim_assess(shim, x, o, eb, autocor=True)
    assert qm.check(got, want) == []
    # without the flag: the autocorrelations NaN, every other byte the same
    plain = shim_assess(shim, x, o, eb)
    assert math.isnan(plain.stat.autocor_lag_one) and math.isnan(plain.stat.autocor_lag_two)
    plain.stat.autocor_lag_one, plain.stat.autocor_lag_two = got.stat.autocor_lag_one, got.stat.autocor_lag_two
    assert bytes(plain) == bytes(got)


def test_naive_variance_misses_the_tolerances():
    """What the tolerances are there to catch: sum v^2 / n - mean^2 in double on the offset fields."""
    for name in ("offset_f32", "offset_f64"):
        o, x, eb, want = case(name, NS[-1])
        v = o.astype(np.float64)
        std = math.sqrt(max((v * v).sum() / v.size - (v.sum() / v.size) ** 2, 0.0))
        got = dict(want)
        got["odata.std"] = std
        assert any(b.startswith("odata.std") for b in qm.check(got, want))


def test_degenerate_inputs(shim):
    o = np.array([1.0, 2.0, 3.0, 5.0], np.float32)
    q = shim_assess(shim, o, o, 1e-3)
    assert qm.check(q, qm.assess(o, o, 1e-3)) == []
    assert q.stat.score_MSE == 0 and q.stat.score_PSNR == math.inf and q.first_diff_idx == cz.SIZE_MAX
    c = np.full(9, 2.5, np.float64)
    q = shim_assess(shim, c, c, 0.0)
    assert math.isnan(q.stat.score_coeff) and q.stat.odata.std == 0
    assert qm.check(q, qm.assess(c, c, 0.0)) == []
    nan = np.full(5, np.nan, np.float32)
    q = shim_assess(shim, nan, nan, 1e-3)
    assert qm.check(q, qm.assess(nan, nan, 1e-3)) == []
    assert q.n_finite == 0 and q.n_nonfinite == 5 and q.n_unbounded == 0 and q.stat.max_err_idx == cz.SIZE_MAX
    assert math.isnan(q.stat.score_PSNR) and math.isnan(q.stat.odata.avg)
    # a NaN in o, an Inf in x, the same NaN bits in both: three non-finite pairs, two of them unbounded
    o, x, eb, _ = case("ramp_f32", 1000)
    o, x = o.copy(), x.copy()
    o[17], x[500], o[900], x[900] = np.nan, np.inf, np.nan, np.nan
    q = shim_assess(shim, x, o, eb, autocor=True)
    assert (q.n_nonfinite, q.first_unbounded_idx) == (3, 17)
    assert qm.check(q, qm.assess(x, o, eb, autocor=True)) == []


def _parts(n, k):
    """k uneven consecutive parts of n elements, one of them a single element (k > 1)."""
    if k == 1:
        return [0, n]
    cuts = sorted({1 + (n - 2) * (i * i + 1) // (k * k + 1) for i in range(1, k - 1)} | {n - 1})
    cuts = [0] + cuts + [n]
    assert len(cuts) == k + 1 and cuts[-1] - cuts[-2] == 1
    return cuts


@pytest.mark.parametrize("k", [1, 2, 3, 7])
@pytest.mark.parametrize("name", sorted(qm.FIELDS))
def test_merge_of_parts_equals_the_whole(shim, name, k):
    o, x, eb, want = case(name, 70001)
    cuts = _parts(o.size, k)
    parts = [shim_assess(shim, x[a:b], o[a:b], eb) for a, b in zip(cuts, cuts[1:])]
    got = cz.quality_merge(parts, cuts[:-1])
    want = dict(want, autocor_lag_one=math.nan, autocor_lag_two=math.nan)  # not mergeable: NaN
    assert qm.check(got, want) == []
    assert math.isnan(got.stat.autocor_lag_one) and math.isnan(got.stat.autocor_lag_two)


def test_merge_rebases_indices_and_breaks_ties_low(shim):
    n, eb = 3000, 1e-3
    o = ((np.arange(n) - 1500) / 1024).astype(np.float32)  # multiples of 2^-10: adding 0.25 is exact
    x = o.copy()
    for i in (700, 1800, 2900):  # the same largest error in three parts
        x[i] = o[i] + np.float32(0.25)
    x[2500] = np.nextafter(o[2500], np.float32(2))  # differs, within the bound
    cuts = [0, 1000, 1001, 2000, n]
    parts = [shim_assess(shim, x[a:b], o[a:b], eb) for a, b in zip(cuts, cuts[1:])]
    assert [p.stat.max_err_idx for p in parts] == [700, 0, 799, 900]
    got = cz.quality_merge(parts, cuts[:-1])
    want = qm.assess(x, o, eb)
    assert qm.check(got, want) == []
    # the three errors are equal: the lowest index wins
    assert (got.stat.max_err_idx, got.n_unbounded, got.first_unbounded_idx, got.first_diff_idx) == (700, 3, 700, 700)
    # parts whose first difference / first unbounded element lie in a later part
    got = cz.quality_merge(parts[1:3], [0, 1])
    assert (got.first_diff_idx, got.first_unbounded_idx, got.stat.max_err_idx, got.stat.len) == (800, 800, 800, 1000)
    got = cz.quality_merge(parts[1:2], [0])
    assert (got.first_diff_idx, got.first_unbounded_idx, got.n_unbounded) == (cz.SIZE_MAX, cz.SIZE_MAX, 0)


def test_merge_refuses_bad_arguments(shim):
    o, x, eb, _ = case("ramp_f32", 1000)
    a, b = shim_assess(shim, x[:400], o[:400], eb), shim_assess(shim, x[400:], o[400:], eb)
    L = cz.lib()
    arr, out = (cz.psz_amd_quality * 2)(a, b), cz.psz_amd_quality()
    before = bytes(out)
    offs = (C.c_size_t * 2)(0, 400)
    assert L.psz_amd_quality_merge(arr, offs, 2, C.byref(out)) == cz.PSZ_SUCCESS
    out = cz.psz_amd_quality()
    for args in ((None, offs, 2, C.byref(out)), (arr, None, 2, C.byref(out)), (arr, offs, 0, C.byref(out)),
                 (arr, offs, 2, None), (arr, (C.c_size_t * 2)(0, 399), 2, C.byref(out)),
                 (arr, (C.c_size_t * 2)(1, 401), 2, C.byref(out))):
        assert L.psz_amd_quality_merge(*args) == cz.PSZ_AMD_ERR_INVALID_ARG
    other = shim_assess(shim, x[400:], o[400:], 2 * eb)  # parts of different bounds
    assert L.psz_amd_quality_merge((cz.psz_amd_quality * 2)(a, other), offs, 2, C.byref(out)) == cz.PSZ_AMD_ERR_INVALID_ARG
    assert bytes(out) == before
    with pytest.raises(cz.PszError):
        cz.quality_merge([a, b], [0, 1])


def test_new_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", cz.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for s in NEW_SYMBOLS:
        assert s in cz.EXPORTS and s in exported, s
    for s in ("assess_quality", "assess_quality_region"):
        assert callable(getattr(cz.Resource, s))
    assert callable(cz.quality_merge)


def test_struct_size_matches_c(tmp_path, shim):
    src = r'''
#include <stddef.h>
#include <stdio.h>
#include "cusz_amd.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", sizeof(psz_data_summary), sizeof(psz_statistics), sizeof(psz_amd_quality),
         offsetof(psz_amd_quality, n_finite), offsetof(psz_statistics, max_err_idx));
  return 0;
}'''
    tmp = str(tmp_path / "quality_abi")
    with open(tmp + ".c", "w") as f:
        f.write(src)
    subprocess.run(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-o", tmp, tmp + ".c"], check=True)
    out = [int(v) for v in subprocess.run([tmp], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [C.sizeof(cz.psz_data_summary), C.sizeof(cz.psz_statistics), C.sizeof(cz.psz_amd_quality),
                   cz.psz_amd_quality.n_finite.offset, cz.psz_statistics.max_err_idx.offset]
    assert shim.qr_shim_sizeof() == C.sizeof(cz.psz_amd_quality)
