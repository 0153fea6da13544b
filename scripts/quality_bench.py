#!/usr/bin/env python3
"""Time the one-pass quality assessment (psz_amd_assess_quality_*) on 512^3 f32 and f64 fields: the
two arrays together are 1 and 2 GiB, well past the 256 MiB cache.  Reported, not gated.

In one process, taking turns: assess_quality without the autocorrelation flag, with it, and two
psz_amd_value_range calls, one per array (the project's one-stream min/max reduction: what reading
the two arrays costs here).  Times are HIP events on the manager's stream around each call, medians
and min..max of --reps repetitions after --warmup; assess_quality's interval includes its one host
wait (it returns the struct), value_range's none.  Bytes are counted from the shapes: each array
once.  One JSON line at the end; needs a GPU and never falls back.

    python scripts/quality_bench.py [--dims 512x512x512] [--reps 10] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cusz_amd as cz  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s (spec)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b)  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="512x512x512")
    ap.add_argument("--eb", type=float, default=1e-4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("quality_bench.py needs a GPU")
    dims = tuple(int(d) for d in args.dims.split("x"))
    n = int(np.prod(dims))
    res = {"workload": f"{args.dims}, x = o + U(-eb, eb), eb={args.eb}", "reps": args.reps, "warmup": args.warmup}
    for name, ctype, tdt in (("f32", cz.F4, torch.float32), ("f64", cz.F8, torch.float64)):
        g = torch.Generator(device="cuda").manual_seed(7)
        o = torch.randn(n, generator=g, device="cuda", dtype=tdt)
        x = o + (2 * torch.rand(n, generator=g, device="cuda", dtype=tdt) - 1) * args.eb
        r = cz.Resource(ctype, dims)
        mm = torch.zeros(4, dtype=torch.float64, device="cuda")
        calls = {
            "assess": lambda: r.assess_quality(x.data_ptr(), o.data_ptr(), n, args.eb),
            "assess_autocor": lambda: r.assess_quality(x.data_ptr(), o.data_ptr(), n, args.eb, True),
            "two_value_range": lambda: (r.value_range(o.data_ptr(), mm.data_ptr(), n),
                                        r.value_range(x.data_ptr(), mm.data_ptr() + 16, n)),
        }
        times = {k: [] for k in calls}
        for it in range(args.warmup + args.reps):
            for k, fn in calls.items():  # the three take turns
                t = timed(fn)
                if it >= args.warmup:
                    times[k].append(t)
        q = r.assess_quality(x.data_ptr(), o.data_ptr(), n, args.eb, True)
        lo, hi = mm.cpu().numpy()[:2]
        assert (q.stat.odata.min, q.stat.odata.max) == (lo, hi), "the two kernels disagree on the original's range"
        nbytes = 2 * n * o.element_size()
        out = {"bytes": nbytes, "psnr": q.stat.score_PSNR, "autocor_lag_one": q.stat.autocor_lag_one,
               "n_unbounded": q.n_unbounded}  # f32: x rounds half an ulp past the bound at |o| > 4
        for k, v in times.items():
            med = statistics.median(v)
            out[k] = {"median_us": round(med, 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1),
                      "TB_per_s": round(nbytes / med / 1e6, 3), "share_of_hbm_peak": round(nbytes / med / 1e6 / (HBM_PEAK / 1e12), 3)}
        for k in ("assess", "assess_autocor"):
            out[k]["ratio_to_two_value_range"] = round(out[k]["median_us"] / out["two_value_range"]["median_us"], 3)
        res[name] = out
        print(f"{name}: " + "  ".join(f"{k} {out[k]['median_us']:.1f} us ({out[k]['TB_per_s']:.2f} TB/s)" for k in calls),
              file=sys.stderr)
        del o, x
    print(json.dumps(res))


if __name__ == "__main__":
    main()
