"""The yardstick of the quality assessment (include/cusz_amd.h psz_amd_assess_quality_*): the header's
definitions computed from the two arrays in two passes, sums in numpy.longdouble (64-bit mantissa,
pairwise), masks for the finite pairs.  What the header defines as one double operation (the error,
the range, the two ratios of the largest error) is one double operation here, so those compare
exactly.  The library is compared against this, never against itself.

Also here: the seeded test fields, the tolerances (derived below, not tuned) and the comparison.
"""
import math

import numpy as np

SIZE_MAX = 2 ** 64 - 1
U = 2.0 ** -53
L = np.longdouble

EXACT = ("odata.min", "odata.max", "odata.rng", "xdata.min", "xdata.max", "xdata.rng", "max_err_abs",
         "max_err_idx", "max_err_rel", "max_err_pwrrel", "user_eb", "len", "n_finite", "n_nonfinite",
         "n_unbounded", "first_unbounded_idx", "first_diff_idx")


def _first(mask):
    i = np.flatnonzero(mask)
    return int(i[0]) if i.size else SIZE_MAX


def _corr(a, b):
    """(sum (a - avg_a)(b - avg_b) / m) / (std_a std_b) of two longdouble arrays; NaN for a zero std."""
    m = a.size
    if m == 0:
        return math.nan
    da, db = a - a.sum() / m, b - b.sum() / m
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(((da * db).sum() / m) / (np.sqrt((da * da).sum() / m) * np.sqrt((db * db).sum() / m)))


def assess(x, o, eb=0.0, autocor=False):
    """dict of every field of psz_amd_quality ("odata.min" ... for the summaries) for the
    reconstruction x against the original o (1-D arrays of one float type)."""
    x, o = np.ascontiguousarray(x).ravel(), np.ascontiguousarray(o).ravel()
    assert x.dtype == o.dtype and x.size == o.size and x.size
    n = o.size
    bits = np.uint32 if o.dtype == np.float32 else np.uint64
    differ = x.view(bits) != o.view(bits)
    od, xd = o.astype(np.float64), x.astype(np.float64)
    fin = np.isfinite(od) & np.isfinite(xd)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.abs(xd - od)  # one double operation
    m = int(fin.sum())
    r = {"len": n, "user_eb": float(eb), "n_finite": m, "n_nonfinite": n - m,
         "first_diff_idx": _first(differ)}
    if eb > 0:
        with np.errstate(invalid="ignore"):
            unb = (fin & (e > 1.001 * eb)) | (~fin & differ)
        r["n_unbounded"], r["first_unbounded_idx"] = int(unb.sum()), _first(unb)
    else:
        r["n_unbounded"], r["first_unbounded_idx"] = 0, SIZE_MAX
    nan = math.nan
    r["autocor_lag_one"] = r["autocor_lag_two"] = nan
    if autocor:
        for k, name in ((1, "autocor_lag_one"), (2, "autocor_lag_two")):
            if n > k:
                a, b = od[:n - k], od[k:]
                f = np.isfinite(a) & np.isfinite(b)
                r[name] = _corr(a[f].astype(L), b[f].astype(L))
    if m == 0:
        for s in ("odata", "xdata"):
            for f in ("min", "max", "rng", "avg", "std"):
                r[f"{s}.{f}"] = nan
        for f in ("score_PSNR", "score_MSE", "score_NRMSE", "score_coeff", "max_err_abs", "max_err_rel",
                  "max_err_pwrrel"):
            r[f] = nan
        r["max_err_idx"] = SIZE_MAX
        return r
    of, xf, ef = od[fin], xd[fin], e[fin]
    for s, v in (("odata", of), ("xdata", xf)):
        lo, hi = float(v.min()), float(v.max())
        vl = v.astype(L)
        avg = vl.sum() / m
        r[f"{s}.min"], r[f"{s}.max"], r[f"{s}.rng"] = lo, hi, hi - lo
        r[f"{s}.avg"], r[f"{s}.std"] = float(avg), float(np.sqrt(((vl - avg) ** 2).sum() / m))
    rng = r["odata.rng"]
    emax = float(ef.max())
    r["max_err_abs"] = emax
    r["max_err_idx"] = _first(fin & (e == emax))
    with np.errstate(invalid="ignore", divide="ignore"):
        r["max_err_rel"] = float(np.float64(emax) / np.float64(rng))
        nz = of != 0
        r["max_err_pwrrel"] = float((ef[nz] / np.abs(of[nz])).max()) if nz.any() else nan
        mse = (ef.astype(L) ** 2).sum() / m
        r["score_MSE"] = float(mse)
        r["score_NRMSE"] = float(np.sqrt(mse) / L(rng))
        r["score_PSNR"] = float(20 * np.log10(L(rng)) - 10 * np.log10(mse))
    r["score_coeff"] = _corr(of.astype(L), xf.astype(L))
    return r


def as_dict(q):
    """The same dict from a cusz_amd.psz_amd_quality."""
    s = q.stat
    r = {f"{n}.{f}": getattr(getattr(s, n), f) for n in ("odata", "xdata") for f in ("min", "max", "rng", "avg", "std")}
    for f in ("score_PSNR", "score_MSE", "score_NRMSE", "score_coeff", "max_err_abs", "max_err_rel", "max_err_pwrrel",
              "max_err_idx", "autocor_lag_one", "autocor_lag_two", "user_eb", "len"):
        r[f] = getattr(s, f)
    for f in ("n_finite", "n_nonfinite", "n_unbounded", "first_unbounded_idx", "first_diff_idx"):
        r[f] = getattr(q, f)
    return r


def _same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def _ulps(a, b):
    if _same(a, b):
        return 0.0
    if not (math.isfinite(a) and math.isfinite(b)):
        return math.inf
    return abs(a - b) / float(np.spacing(np.float64(max(abs(a), abs(b)))))


def check(got, want, verbose=False):
    """Compare a result (dict, or the ctypes struct) against the model's dict.  With u = 2^-53, n the
    length and kappa = max(|avg_o|, |avg_x|) / min(std_o, std_x) of the model:
      exactly equal   min, max, rng, max_err_abs / _idx / _rel / _pwrrel, every count and index, len,
                      user_eb (one double operation each, or none)
      rel 8 (n + kappa) u   score_MSE, both std: a sum of n non-negative terms is within n u in any
                      order; a mean held as a double is off by u |avg|, which is kappa u of a std
      abs 8 (n + kappa) u   score_coeff, the autocorrelations: Cauchy-Schwarz bounds the cross sum
                      by the two sums of squares
      abs 8 n u max(|min|, |max|)   avg
      2 ulp           score_NRMSE and score_PSNR against the header's formulas applied, in double, to
                      the returned score_MSE and odata.rng
    Returns the list of violations (empty: passed)."""
    if not isinstance(got, dict):
        got = as_dict(got)
    bad = []
    for f in EXACT:
        if not _same(got[f], want[f]):
            bad.append(f"{f}: {got[f]!r} != {want[f]!r}")
    n = want["len"]
    if want["n_finite"] == 0 or want["n_finite"] != got["n_finite"]:
        for f in ("odata.avg", "odata.std", "xdata.avg", "xdata.std", "score_MSE", "score_NRMSE", "score_PSNR",
                  "score_coeff"):
            if not _same(got[f], want[f]):
                bad.append(f"{f}: {got[f]!r} != {want[f]!r}")
        return bad
    stds = min(want["odata.std"], want["xdata.std"])
    kappa = max(abs(want["odata.avg"]), abs(want["xdata.avg"])) / stds if stds > 0 else 0.0
    tol = 8 * (n + kappa) * U

    def near(f, bound, relative):
        g, w = got[f], want[f]
        if _same(g, w):
            return
        err = abs(g - w) / (abs(w) if relative and w != 0 else 1.0)
        if verbose:
            print(f"  {f}: err {err:.3e} bound {bound:.3e}")
        if not (err <= bound):
            bad.append(f"{f}: {g!r} vs {w!r}: {'rel' if relative else 'abs'} {err:.3e} > {bound:.3e}")

    near("score_MSE", tol, True)
    for s in ("odata", "xdata"):
        near(f"{s}.std", tol, True)
        near(f"{s}.avg", 8 * n * U * max(abs(want[f"{s}.min"]), abs(want[f"{s}.max"])), False)
    for f in ("score_coeff", "autocor_lag_one", "autocor_lag_two"):
        near(f, tol, False)
    mse, rng = np.float64(got["score_MSE"]), np.float64(got["odata.rng"])
    with np.errstate(invalid="ignore", divide="ignore"):
        nrmse = float(np.sqrt(mse) / rng)
        psnr = float(20 * np.log10(rng) - 10 * np.log10(mse))
    for f, w in (("score_NRMSE", nrmse), ("score_PSNR", psnr)):
        if _ulps(got[f], w) > 2:
            bad.append(f"{f}: {got[f]!r} is {_ulps(got[f], w):.1f} ulp from {w!r}")
    return bad


# ---- fields ------------------------------------------------------------------------------------
FIELDS = {  # name: (dtype, eb)
    "offset_f32": (np.float32, 2e-3),  # kappa about 1e5: kappa^2 >> n, what sum v^2 / n - mean^2 cannot take
    "offset_f64": (np.float64, 1e-4),
    "ramp_f32": (np.float32, 1e-3),
}


def field(name, n, seed=2024):
    """(o, x, eb): the seeded original, x = o + U(-eb, eb) rounded to the element type."""
    dtype, eb = FIELDS[name]
    rng = np.random.default_rng([seed, n, sorted(FIELDS).index(name)])
    g = rng.standard_normal(n)
    if name == "offset_f32":
        o = 4096 + 0.05 * g
    elif name == "offset_f64":
        o = 1e4 + 0.1 * g
    else:
        o = 0.01 * np.arange(n, dtype=np.float64) + g
    o = o.astype(dtype)
    x = (o.astype(np.float64) + rng.uniform(-eb, eb, n)).astype(dtype)
    return o, x, eb
