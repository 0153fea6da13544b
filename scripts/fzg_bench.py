#!/usr/bin/env python3
"""Measure the FZG codec against the default Huffman path on bench.py's config-2 recipe (512^3 f32,
abs 1e-4, datagen.smooth3d, seed 2, Lorenzo).  Reported, not gated: bench.py stays the yardstick.

Both codecs run in one process and take turns (Huffman, FZG, Huffman, ...).  Times are the
managers' HIP-event stage times (psz_amd_enable_timing): medians and min..max of --reps repetitions
after --warmup.  One JSON line at the end; needs a GPU and never falls back.

    python scripts/fzg_bench.py [--dims 512x512x512] [--reps 5] [--warmup 2]
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
from cusz_amd import datagen  # noqa: E402

STAGES = {"predict": cz.T_PREDICT, "book": cz.T_BOOK, "encode": cz.T_ENCODE, "finalize": cz.T_FINALIZE,
          "compress": cz.T_COMPRESS, "scatter": cz.T_SCATTER, "decode": cz.T_DECODE, "recon": cz.T_RECON,
          "decompress": cz.T_DECOMPRESS}
COMPRESS_STAGES = ("predict", "book", "encode", "finalize", "compress")


def counted_bytes_per_element(n, words, splen):
    """HBM bytes per element the FZG kernels move, counted from the code: the sizing
    and packing passes each read the 2-byte codes; flags are written once and read twice (pack,
    decode); the payload is written once and read once."""
    units = (n + 255) // 256
    enc = (2 * n + 8 * units) + (2 * n + 8 * units + 8 * words)  # size: codes -> flags; pack: codes + flags -> words
    dec = 8 * units + 8 * words + 2 * n                          # flags + words -> codes
    return {"encode": enc / n, "decode": dec / n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="512x512x512")
    ap.add_argument("--eb", type=float, default=1e-4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fzg_bench.py needs a GPU")
    dims = tuple(int(d) for d in args.dims.split("x"))
    n = int(np.prod(dims))
    dev = torch.device("cuda:0")
    d_in = datagen.smooth3d_torch(dims, seed=args.seed, dtype=torch.float32, device=dev)
    out = torch.empty(n, dtype=torch.float32, device=dev)
    mgr = {"huffman": cz.Resource(cz.F4, dims), "fzg": cz.Resource(cz.F4, dims, codec=cz.FZCodec)}
    times = {k: {s: [] for s in STAGES} for k in mgr}
    size, splen, recon = {}, {}, {}
    for r in mgr.values():
        r.enable_timing()
    for it in range(args.warmup + args.reps):
        for name, r in mgr.items():  # the codecs take turns
            ptr, nb, _ = r.compress(d_in.data_ptr(), args.eb)
            t = r.stage_times()
            for s in COMPRESS_STAGES:
                if it >= args.warmup:
                    times[name][s].append(1e3 * t[STAGES[s]])
            r.decompress(ptr, nb, out.data_ptr())
            torch.cuda.synchronize()
            t = r.stage_times()
            for s in STAGES:
                if s not in COMPRESS_STAGES and it >= args.warmup:
                    times[name][s].append(1e3 * t[STAGES[s]])
            size[name], splen[name] = nb, r.header.splen
            if it == 0:
                recon[name] = out.clone()
    # both codecs carry the same codes: the same field comes back, within the bound
    assert torch.equal(recon["huffman"], recon["fzg"]), "the codecs decompress to different fields"
    err = float((recon["fzg"].double() - d_in.double()).abs().max())
    assert err <= 1.001 * args.eb + 2.0 ** -23 * float(d_in.abs().max()), err

    def summary(v):
        return {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}

    words = (size["fzg"] - 176 - 8 * splen["fzg"] - (32 + 8 * ((n + 255) // 256) + 4 * ((n + 4095) // 4096 + 1) + 7) // 8 * 8) // 8
    res = {"workload": f"{args.dims} f32 abs eb={args.eb} smooth3d seed {args.seed}, Lorenzo", "reps": args.reps,
           "warmup": args.warmup, "max_err": err, "outliers": splen["fzg"],
           "fzg_payload_words": words, "fzg_counted_bytes_per_element": counted_bytes_per_element(n, words, splen["fzg"])}
    for name in mgr:
        res[name] = {"archive_bytes": size[name], "ratio": round(4 * n / size[name], 3),
                     **{s: summary(times[name][s]) for s in STAGES}}
        c, d = res[name]["compress"]["median_us"], res[name]["decompress"]["median_us"]
        print(f"{name:8s} CR {res[name]['ratio']:7.3f}  compress {c:9.1f} us ({4 * n / c / 1e3:7.1f} GB/s)  "
              f"decompress {d:9.1f} us ({4 * n / d / 1e3:7.1f} GB/s)  encode {res[name]['encode']['median_us']:8.1f} us  "
              f"decode {res[name]['decode']['median_us']:8.1f} us", file=sys.stderr)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
