#!/usr/bin/env python3
"""Region decode benchmark: one f32 field (512^3 by default; --dims takes one, two or three
extents) compressed at abs 1e-4, then the time of psz_amd_decompress_region_float for a few boxes
against the full psz_decompress_float of the same archive, in one process on one device.  --mode
whole|cover|both picks the manager's region mode (psz_amd_set_region_mode); `both` times every box
in either mode, taking turns, on the one manager.

Each call is bracketed by HIP events on the manager's stream (a region call's one 4-byte
read-back, when the archive has outlier cells, falls inside the bracket: it is part of the call).
The cases take turns inside every repetition, so drift hits them alike; the first WARMUP rounds are
dropped and the median of the rest is reported.  Every box is also compared, bit for bit, with the
same box of the full decompress.  usage: region_bench.py [--dims 512x512x512] [--eb 1e-4]
[--mode whole|cover|both] [--reps 30] [--warmup 5] [--json FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import cusz_amd as cz  # noqa: E402
from cusz_amd import datagen  # noqa: E402


def boxes_for(dims):
    x, y, z = dims
    q = lambda v, d: max(1, v // d)  # noqa: E731  (the issue's boxes, scaled to smaller test fields)
    if y == 1 and z == 1:  # 1-D: ranges of particles
        return [("range %d" % min(x, k), (min(x // 2 + 5, x - min(x, k)), 0, 0), (min(x, k), 1, 1))
                for k in (1 << 10, 1 << 20, 1 << 24)] + [("one element", (x // 2 + 1, 0, 0), (1, 1, 1))]
    if z == 1:  # 2-D: bands of rows
        return [("band %d rows" % min(y, k), (0, min(y // 2 + 3, y - min(y, k)), 0), (x, min(y, k), 1)) for k in (32, 256)] + [
            ("block %dx%d" % (q(x, 4), q(y, 8)), (x // 3, y // 3, 0), (q(x, 4), q(y, 8), 1)),
            ("one element", (x // 2 + 1, y // 2 + 1, 0), (1, 1, 1))]
    return [
        ("8 planes %dx%dx%d" % (x, y, min(z, 8)), (0, 0, min(z // 2 // 8 * 8, z - min(z, 8))), (x, y, min(z, 8))),
        ("plane slab %dx%dx%d" % (x, y, q(z, 64)), (0, 0, z // 2), (x, y, q(z, 64))),
        ("thick slab %dx%dx%d" % (x, y, q(z, 8)), (0, 0, z // 4), (x, y, q(z, 8))),
        ("block %dx%dx%d" % (q(x, 2), q(y, 8), q(z, 8)), (x // 2, y // 4, z // 4), (q(x, 2), q(y, 8), q(z, 8))),
        ("same, unaligned", (x // 4 + 3, y // 3 + 1, z // 3 + 2), (q(x, 2), q(y, 8), q(z, 8))),
        ("one element", (x // 2 + 1, y // 2 + 1, z // 2 + 1), (1, 1, 1)),
    ]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="512x512x512")
    ap.add_argument("--eb", type=float, default=1e-4)
    ap.add_argument("--mode", default="whole", choices=["whole", "cover", "both"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    dims = tuple(int(v) for v in a.dims.split("x"))
    if not 1 <= len(dims) <= 3 or a.reps < 20:
        ap.error("one to three dims and at least 20 repetitions")
    dims = (dims + (1, 1))[:3]
    modes = dict(whole=[cz.REGION_MODE_WHOLE], cover=[cz.REGION_MODE_COVER],
                 both=[cz.REGION_MODE_WHOLE, cz.REGION_MODE_COVER])[a.mode]
    mode_name = {cz.REGION_MODE_WHOLE: "whole", cz.REGION_MODE_COVER: "cover"}
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev)
    if dims[1] == 1 and dims[2] == 1:  # 1-D: the particle recipe of the benchmark's config 3
        field = datagen.hacc1d_torch(dims[0], device=dev)
    else:
        field = datagen.smooth3d_torch(dims, seed=2, device=dev)
    n = field.numel()
    r = cz.Resource(cz.F4, dims, stream=s.cuda_stream)
    ptr, nbytes, _ = r.compress(field.data_ptr(), a.eb, cz.Abs)
    torch.cuda.synchronize()
    arch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    cz.hip_memcpy(arch.data_ptr(), ptr, nbytes, 3)
    full = torch.empty(n, dtype=torch.float32, device=dev)
    r.decompress(arch.data_ptr(), nbytes, full.data_ptr())
    torch.cuda.synchronize()
    full3 = full.view(dims[2], dims[1], dims[0])
    print(f"dims={dims} eb={a.eb} archive={nbytes} B CR={4 * n / nbytes:.2f} outliers={r.header.splen}", flush=True)

    # (case, origin, extent, region mode): every box once per mode, the modes next to each other
    cases = [("full decompress", None, None, None)]
    cases += [(f"{name} [{mode_name[m]}]" if len(modes) > 1 else name, o, e, m) for name, o, e in boxes_for(dims) for m in modes]
    outs, infos = {}, {}
    for name, o, e, _ in cases[1:]:
        outs[name] = torch.full((e[0] * e[1] * e[2],), float("nan"), dtype=torch.float32, device=dev)

    def run(name, o, e):
        if o is None:
            r.decompress(arch.data_ptr(), nbytes, full.data_ptr())
        else:
            r.decompress_region(arch.data_ptr(), nbytes, o, e, outs[name].data_ptr())

    times = {c[0]: [] for c in cases}
    for it in range(a.warmup + a.reps):
        for name, o, e, m in cases:
            if m is not None:
                r.set_region_mode(m)  # (host only, outside the bracket)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            run(name, o, e)
            e1.record(s)
            torch.cuda.synchronize()
            if it >= a.warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
            if it == 0 and o is not None:
                infos[name] = r.last_region()
                want = full3[o[2]:o[2] + e[2], o[1]:o[1] + e[1], o[0]:o[0] + e[0]].reshape(-1)
                if not torch.equal(outs[name].view(torch.int32), want.contiguous().view(torch.int32)):
                    print(f"MISMATCH: {name}")
                    return 1

    def stats(ts):
        ts = sorted(ts)
        return ts[len(ts) // 2], ts[0], ts[(len(ts) * 9) // 10]

    base = stats(times["full decompress"])[0]
    rows = []
    paths = {cz.REGION_FUSED: "fused", cz.REGION_FALLBACK: "fallback", cz.REGION_SLAB: "slab"}
    print(f"{'case':<36} {'path':<8} {'bricks':>6} {'chunks':>8} {'median us':>10} {'min us':>8} {'p90 us':>8} {'of full':>8}")
    for name, o, e, m in cases:
        med, mn, p90 = stats(times[name])
        info = infos.get(name)
        path = "-" if info is None else paths[info.path]
        bricks = "-" if info is None else str(info.bricks)
        chunks = "-" if info is None else str(info.chunks)
        print(f"{name:<36} {path:<8} {bricks:>6} {chunks:>8} {med:10.1f} {mn:8.1f} {p90:8.1f} {med / base:8.2f}", flush=True)
        rows.append(dict(case=name, origin=o, extent=e, mode=None if m is None else mode_name[m], path=path, bricks=bricks,
                         chunks=chunks, median_us=med, min_us=mn, p90_us=p90, of_full=med / base))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(dims=dims, eb=a.eb, mode=a.mode, reps=a.reps, warmup=a.warmup, archive_bytes=nbytes, rows=rows), f,
                      indent=1)
    r.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
