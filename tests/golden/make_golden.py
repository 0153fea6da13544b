#!/usr/bin/env python3
"""Regenerate the committed golden fixtures under tests/golden/.

Run in the development container (needs /root/reference and oracle/_ref built):

    make -C oracle ref && python tests/golden/make_golden.py

Fixtures written (data only -- inputs and expected outputs):

* kat_lorenzo.npz   -- the reference's own known-answer arrays, parsed as data from
                       test/src/detail/correctness.inl (t{1,2,3}_{in,eq,comp_out,decomp_out});
                       sizes 256 (1D), 16x16 (2D), 8x8x8 (3D); they fit inside one GPU tile,
                       so they pin the GPU semantics too.
* ref_lrz3d.npz     -- outputs of the compiled reference CPU Lorenzo-3D
                       (psz/src/kernel/lrz.seq.cc:35-55) on integer-valued inputs at eb=0.5
                       (ebx2_r = 1, so the CPU path's missing round() is the identity and its
                       8^3 tiling equals the GPU's: SURVEY.md §8c item 2).
* ref_codebook.npz  -- histograms and the compiled reference's canonical codebook
                       (codec/hf/src/hf_bk.seq.cc:72-145) for each: book u32[1024], revbook.
* ref_hist.npz      -- codes and the reference serial histogram (hist_generic.seq.cc:17-30).
* ref_ragged.npz    -- the compiled reference CPU Lorenzo-3D, plain and ZigZag, on a ragged
                       40x24x17 integer field at eb=0.5 where most points are outliers.
* ref_brick3d.npz, ref_brick3d_b.npz
                    -- the compiled reference on shapes that take the brick layout (256x16x16,
                       512x8x24; whole 8^3 tiles, see above): the "exact" lattice field of
                       tests/edge_fields.py (integers at eb=0.5 with deltas on the outlier
                       predicate and the code extremes, at the kernels' seams), its codes and
                       outlier cells for plain f32 and ZigZag f32 (zz_*), and for the first
                       shape the f64 instantiation on the same field as doubles (f64_*).
                       Written as .npz with LZMA members (np.load reads them as any other): the
                       walk's codes are dense, deflate would leave the files larger than the rest.
"""
import os
import re
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import edge_fields  # noqa: E402
import pyoracle  # noqa: E402

REF = os.environ.get("PSZ_REFERENCE", "/root/reference")


def parse_correctness_inl():
    txt = open(os.path.join(REF, "test/src/detail/correctness.inl")).read()
    out = {}
    for m in re.finditer(r"static const (float|uint16_t) (t\d_\w+)\[\] = \{(.*?)\};", txt, re.S):
        ty, name, body = m.groups()
        body = re.sub(r"//[^\n]*", "", body)
        vals = [float(v) for v in body.replace("\n", " ").split(",") if v.strip()]
        out[name] = np.array(vals, np.float32 if ty == "float" else np.uint16)
    return out


def skewed_hist(rng, n_sym, total, width):
    h = np.zeros(1024, np.uint32)
    c = rng.normal(512, width, total).round().astype(np.int64)
    c = np.clip(c, 1, 1023)
    np.add.at(h, c, 1)
    h[0] = rng.integers(0, 50)
    return h


def savez_lzma(path, **arrays):
    """np.savez_compressed with LZMA instead of deflate, and fixed member dates (same bytes each run)."""
    with zipfile.ZipFile(path, "w") as zf:
        for name, a in arrays.items():
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_LZMA
            with zf.open(info, "w", force_zip64=False) as f:
                np.lib.format.write_array(f, np.asanyarray(a), allow_pickle=False)


def main():
    kat = parse_correctness_inl()
    assert set(kat) >= {"t1_in", "t1_eq", "t1_comp_out", "t1_decomp_out", "t3_decomp_out"}, kat.keys()
    np.savez_compressed(os.path.join(HERE, "kat_lorenzo.npz"), **kat)

    rng = np.random.default_rng(20260313)
    # 3D integer-valued field, dims multiples of 8 (the CPU path carries stale tile
    # buffers across partial tiles, lrz.seq.inl:140-150, so only full tiles coincide).
    dims = (40, 24, 16)
    n = dims[0] * dims[1] * dims[2]
    walk = np.cumsum(rng.integers(-3, 4, n)).astype(np.float32)
    walk[rng.integers(0, n, 40)] += rng.integers(-5000, 5000, 40)
    codes, ov, oi = pyoracle.ref_lorenzo_c_f32(walk, dims, 0.5)
    np.savez_compressed(os.path.join(HERE, "ref_lrz3d.npz"), data=walk, dims=np.array(dims),
                        codes=codes, ol_val=ov, ol_idx=oi)

    hists, books, rvbks = [], [], []
    cases = []
    cases.append(skewed_hist(rng, 1024, 200000, 3.0))
    cases.append(skewed_hist(rng, 1024, 50000, 20.0))
    cases.append(skewed_hist(rng, 1024, 3000, 100.0))
    flat = np.zeros(1024, np.uint32)
    flat[100:900] = 7
    cases.append(flat)
    ties = np.zeros(1024, np.uint32)
    ties[rng.choice(1024, 300, replace=False)] = rng.integers(1, 4, 300)
    cases.append(ties)
    two = np.zeros(1024, np.uint32)
    two[[3, 700]] = [5, 9]
    cases.append(two)
    fib = np.zeros(1024, np.uint32)  # Fibonacci depth 25 (< 27): exact reference behaviour
    a, b = 1, 1
    for i in range(26):
        fib[400 + i] = a
        a, b = b, a + b
    cases.append(fib)
    for k in range(5):
        h = np.zeros(1024, np.uint32)
        m = rng.integers(2, 1024)
        idx = rng.choice(1024, m, replace=False)
        h[idx] = rng.integers(1, 1000, m)
        cases.append(h)
    for h in cases:
        book, rv = pyoracle.ref_codebook(h)
        hists.append(h)
        books.append(book)
        rvbks.append(rv)
    np.savez_compressed(os.path.join(HERE, "ref_codebook.npz"), hist=np.stack(hists),
                        book=np.stack(books), revbook=np.stack(rvbks))

    codes = rng.integers(0, 1024, 100000).astype(np.uint16)
    np.savez_compressed(os.path.join(HERE, "ref_hist.npz"), codes=codes,
                        hist=pyoracle.ref_histogram(codes))
    # (round 2; own generator so the fixtures above stay as they were)
    rng2 = np.random.default_rng(20261016)
    # ZigZag (the reference's own f4 instantiation, lrz.seq.cc:82) and f64 (the 3-D template
    # instantiated for double by oracle/ref_shim.cc) on the same kind of integer field
    codes, ov, oi = pyoracle.ref_lorenzo_c_zz_f32(walk, dims, 0.5)
    np.savez_compressed(os.path.join(HERE, "ref_lrz3d_zz.npz"), data=walk, dims=np.array(dims),
                        codes=codes, ol_val=ov, ol_idx=oi)
    walk64 = np.cumsum(rng2.integers(-3, 4, n)).astype(np.float64)
    walk64[rng2.integers(0, n, 40)] += rng2.integers(-5000, 5000, 40)
    codes, ov, oi = pyoracle.ref_lorenzo3d_f64(walk64, dims, 0.5)
    np.savez_compressed(os.path.join(HERE, "ref_lrz3d_f64.npz"), data=walk64, dims=np.array(dims),
                        codes=codes, ol_val=ov, ol_idx=oi)
    # ragged field (partial tiles on every axis) where almost every point is an outlier: the
    # reference's outputs as it wrote them (the outlier list runs past the field's end)
    rdims = (40, 24, 17)
    rdata = np.random.default_rng(11).integers(-4000, 4000, size=rdims[::-1]).astype(np.float32).ravel()
    out = {"data": rdata, "dims": np.array(rdims)}
    for tag, fn in (("", pyoracle.ref_lorenzo_c_f32), ("zz_", pyoracle.ref_lorenzo_c_zz_f32)):
        codes, ov, oi = fn(rdata, rdims, 0.5)
        out.update({tag + "codes": codes, tag + "ol_val": ov, tag + "ol_idx": oi})
    np.savez_compressed(os.path.join(HERE, "ref_ragged.npz"), **out)
    # brick-layout shapes (the field has its own generator, seeded from the shape: the fixtures
    # above stay as they were)
    for name, bdims, with_f64 in (("ref_brick3d.npz", (256, 16, 16), True), ("ref_brick3d_b.npz", (512, 8, 24), False)):
        bdata = edge_fields.lattice_field(bdims, np.float32, "exact")
        out = {"data": bdata, "dims": np.array(bdims)}
        runs = [("", pyoracle.ref_lorenzo_c_f32, bdata), ("zz_", pyoracle.ref_lorenzo_c_zz_f32, bdata)]
        if with_f64:
            bdata64 = edge_fields.lattice_field(bdims, np.float64, "exact")
            assert np.array_equal(bdata64, bdata)  # the same integers: stored once
            runs.append(("f64_", pyoracle.ref_lorenzo3d_f64, bdata64))
        for tag, fn, d in runs:
            codes, ov, oi = fn(d, bdims, 0.5)
            out.update({tag + "codes": codes, tag + "ol_val": ov, tag + "ol_idx": oi})
        savez_lzma(os.path.join(HERE, name), **out)
    print("fixtures written to", HERE)


if __name__ == "__main__":
    main()
