"""Fields past 2 GiB and 2^31 elements, with an expected result that costs a few small oracle runs
(a plain helper module, no tests).

A field is a seeded, non-periodic sequence of R blocks drawn from an alphabet of K small distinct
blocks, plus a ragged tail block.  Blocks are whole multiples of 8 planes (3-D), 32 rows (2-D) or
16384 elements (1-D), so the Lorenzo predictor (tiles of 8^3, 32^2, 1024; linear bricks of 16384)
never reads across a block border: the oracle's codes, outlier cells and reconstruction of the
whole field are those of the blocks, put together by the same sequence.  The spline predictor's
tile reads one plane past its own eight, so there the oracle runs on each (block, first plane of
the next block) pair.  test_huge_fields.py proves both at small R against the oracle on the whole
field.

Every block size has the factor 3, so 2^31, 2^32, 2^33 bytes and 2^31 elements are no whole
number of blocks: an offset that wraps or sign-extends lands on other in-block data, and on
another block id for most positions (shift_differs).

Each block is smooth data plus planted spikes, so every block has outliers, those of the last
blocks at indices >= 2^31.
"""
import dataclasses

import numpy as np

from cusz_amd import datagen

MARK_BYTES = (2 ** 31, 2 ** 32, 2 ** 33)
MARK_ELEMS = 2 ** 31
ABS, REL = 0, 1
REL_LO, REL_HI = -8.0, 8.0  # Rel mode: the planted extremes (beyond the smooth data and every spike)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    dtype: type
    row: tuple        # extents faster than the axis the blocks are stacked on: (x, y), (x,) or ()
    block: int        # a block's extent on the stacked axis: planes, rows or elements
    reps: int         # R
    tail: int         # the tail block's extent on the stacked axis
    k: int = 3        # blocks in the alphabet
    eb: float = 1e-3
    radius: int = 512
    noise: float = 1e-3
    mode: int = ABS
    spline: bool = False
    zigzag: bool = False
    seed: int = 1

    @property
    def unit(self):
        return int(np.prod(self.row, dtype=np.int64))

    @property
    def block_elems(self):
        return self.block * self.unit

    @property
    def tail_elems(self):
        return self.tail * self.unit

    @property
    def n(self):
        return self.reps * self.block_elems + self.tail_elems

    @property
    def itemsize(self):
        return np.dtype(self.dtype).itemsize

    def dims3(self, extent):
        """(x, y, z) of `extent` steps of the stacked axis."""
        return (tuple(self.row) + (extent,) + (1, 1))[:3]

    @property
    def dims(self):
        return self.dims3(self.reps * self.block + self.tail)

    def small(self, reps=5):
        """The same alphabet and tail in a field that the oracle takes whole."""
        return dataclasses.replace(self, reps=reps)

    def shifts(self):
        """What a truncated or sign-extended offset moves an access by, in elements."""
        return sorted({m // self.itemsize for m in MARK_BYTES} | {MARK_ELEMS})


P256 = (256, 256)
# the cases of test_gpu_huge.py: each the smallest shape that reaches its edge
CASES = {c.name: c for c in [
    # 3-D f64 on bricks, 2^29 + 1.4 M elements: input and output cross 2^31 and 2^32 bytes
    Case("f64_4g", np.float64, P256, 24, 342, 5, seed=11),
    # 3-D f32 on bricks just past 2^31 elements: bytes past 2^33, element and outlier indices >= 2^31
    Case("f32_2g", np.float32, P256, 24, 1366, 5, seed=12),
    # x no multiple of 256: reference layout, just past 2^31 bytes
    Case("ref3d", np.float32, (250, 256), 24, 350, 5, seed=13),
    Case("1d", np.float32, (), 3 * 16384, 43690, 5 * 16384 + 77, seed=14),   # n = 2^31 + 3 * 16384 + 77
    Case("2d_under", np.float32, (4096,), 96, 1365, 31, seed=15),            # 131071 rows: 2^31 - 16 KiB bytes
    Case("2d_over", np.float64, (4096,), 96, 683, 31, seed=16),              # 65599 rows: 2 GiB + 2 MB
    Case("spline_over", np.float32, P256, 24, 1366, 5, k=2, spline=True, seed=17),
    Case("spline_under", np.float32, P256, 24, 1365, 5, k=2, spline=True, seed=17),
    # codes of ~9.6 bits each: a Huffman bitstream between 2^31 and 2^32 bytes
    Case("noisy", np.float32, P256, 24, 1366, 5, noise=0.15, seed=18),
    Case("rel", np.float32, P256, 24, 1366, 5, eb=5e-5, mode=REL, seed=19),
]}


def sequence(case):
    """Block ids of the R blocks.  The first is block 0 (Rel mode: it holds the minimum), the last
    block 1: where only the field's last elements can wrap onto its first, the ids still differ."""
    seq = np.random.default_rng(1000 + case.seed).integers(0, case.k, case.reps)
    seq[0], seq[-1] = 0, 1
    return seq


def shift_differs(case, seq, shift):
    """Fraction of the elements e < n - shift whose block id differs from that of element e + shift
    (the tail counts as a block of its own; None when the shift is not inside the field).
    Computed on block ids: both ids are constant between the points where e or e + shift crosses a
    block border."""
    n, be, reps = case.n, case.block_elems, case.reps
    if shift >= n:
        return None
    m = n - shift
    edges = np.unique(np.concatenate((np.arange(0, m, be), np.arange(-shift % be, m, be), [m])))
    ids = np.concatenate((np.asarray(seq), [case.k]))
    e = edges[:-1]
    differ = ids[np.minimum(e // be, reps)] != ids[np.minimum((e + shift) // be, reps)]
    return float((np.diff(edges) * differ).sum() / m)


def _spikes(f, rng, count, height):
    pos = rng.choice(f.size, count, replace=False)
    f[pos] += np.where(rng.random(count) < 0.5, -height, height) * rng.uniform(1.0, 1.5, count)


def blocks(case):
    """-> (alphabet [K, block_elems], tail [tail_elems]) in the case's dtype.  Rel mode: block 0
    holds the field's minimum, the tail its maximum."""
    rng = np.random.default_rng(case.seed)
    # a delta well past the radius (Rel mode: of the bound times the range, REL_LO .. REL_HI)
    height = 3 * case.radius * 2 * case.eb * (REL_HI - REL_LO if case.mode == REL else 1.0)
    out = []
    for i in range(case.k + 1):
        ext = case.tail if i == case.k else case.block
        f = datagen.smooth3d_np(case.dims3(ext), 100 * case.seed + i, noise=case.noise, dtype=np.float64)
        if len(case.row) < 2:  # 1-D, 2-D: the formula's z term alone is constant
            f = f + 0.25 * np.sin(0.011 * np.arange(f.size) / max(1, case.unit) + i)
        _spikes(f, rng, 12 if i < case.k else 5, height)
        out.append(f)
    if case.mode == REL:
        out[0][out[0].size // 3] = REL_LO
        out[case.k][out[case.k].size - 7] = REL_HI
    return np.stack(out[:case.k]).astype(case.dtype), out[case.k].astype(case.dtype)


def value_range(case, alphabet, tail):
    used = np.unique(sequence(case))
    lo = min(float(alphabet[used].min()), float(tail.min()))
    hi = max(float(alphabet[used].max()), float(tail.max()))
    return lo, hi


def abs_eb(case, alphabet, tail):
    """The bound the kernels work with: Rel mode scales eb by the range, in double."""
    if case.mode == ABS:
        return case.eb
    lo, hi = value_range(case, alphabet, tail)
    return case.eb * (hi - lo)


@dataclasses.dataclass
class Expected:
    """Per block of the alphabet (Lorenzo: index k; spline: index k * K + id of the next block, the
    last block before the tail: K * K + k) and for the tail: codes, reconstruction, outlier cells
    (values f32, in-block indices) and, for spline, anchors."""
    case: Case
    eb: float
    alphabet: np.ndarray
    tail: np.ndarray
    codes: np.ndarray
    recon: np.ndarray
    cells: list
    anchors: np.ndarray
    codes_tail: np.ndarray
    recon_tail: np.ndarray
    cells_tail: tuple
    anchors_tail: np.ndarray

    def ids(self, seq):
        """The sequence as indices into codes / recon / cells."""
        seq = np.asarray(seq)
        if not self.case.spline:
            return seq
        k = self.case.k
        nxt = np.concatenate((seq[1:], [k]))
        return np.where(nxt == k, k * k + seq, seq * k + nxt)


def expected(case, oracle):
    """The oracle once per distinct block (spline: per pair)."""
    alphabet, tail = blocks(case)
    eb = abs_eb(case, alphabet, tail)
    bd, td = case.dims3(case.block), case.dims3(case.tail)
    if not case.spline:
        def run(data, dims):
            c, ov, oi = oracle.lorenzo_c(data, dims, eb, case.radius, case.zigzag)
            x = oracle.lorenzo_x(c, ov, oi, dims, eb, case.radius, case.zigzag, dtype=case.dtype)
            return c, x, (ov, oi), np.zeros(0, case.dtype)
        res = [run(alphabet[i], bd) for i in range(case.k)]
        rt = run(tail, td)
    else:
        u, be = case.unit, case.block_elems
        na = oracle.spline_anchor_len(bd)

        def run(data, dims, keep_elems, keep_anchors):
            c, a, ov, oi = oracle.spline3_c(data, dims, eb, case.radius)
            x = oracle.spline3_x(c, a, ov, oi, dims, eb, case.radius)
            m = oi < keep_elems
            return c[:keep_elems], x[:keep_elems], (ov[m], oi[m]), a[:keep_anchors]
        nd = case.dims3(case.block + 1)
        firsts = [alphabet[j][:u] for j in range(case.k)] + [tail[:u]]
        res = [run(np.concatenate((alphabet[i], firsts[j])), nd, be, na)
               for i in range(case.k) for j in range(case.k)]
        res += [run(np.concatenate((alphabet[i], firsts[case.k])), nd, be, na) for i in range(case.k)]
        rt = run(tail, td, tail.size, oracle.spline_anchor_len(td))
    return Expected(case, eb, alphabet, tail, np.stack([r[0] for r in res]), np.stack([r[1] for r in res]),
                    [r[2] for r in res], np.stack([r[3] for r in res]), rt[0], rt[1], rt[2], rt[3])


def assemble(per_block, tail, ids):
    """Host assembly (small fields)."""
    return np.concatenate([per_block[i] for i in ids] + [tail])


def assemble_cells(exp, seq):
    """-> (index i64[k] ascending, value bits u32[k]) of the whole field's outlier cells."""
    be = exp.case.block_elems
    ids = exp.ids(seq)
    idx, val = [], []
    for k in np.unique(ids):
        ov, oi = exp.cells[k]
        at = np.flatnonzero(ids == k).astype(np.int64)
        idx.append((at[:, None] * be + oi.astype(np.int64)[None, :]).ravel())
        val.append(np.broadcast_to(ov.view(np.uint32)[None, :], (at.size, ov.size)).ravel())
    ov, oi = exp.cells_tail
    idx.append(len(seq) * be + oi.astype(np.int64))
    val.append(ov.view(np.uint32))
    idx, val = np.concatenate(idx), np.concatenate(val)
    order = np.argsort(idx, kind="stable")
    return idx[order], val[order]


def sort_cells(ol_idx, ol_val):
    idx = np.asarray(ol_idx).astype(np.int64)
    order = np.argsort(idx, kind="stable")
    return idx[order], np.asarray(ol_val).view(np.uint32)[order]


def bit_cost(exp, seq, oracle):
    """Bits of the field's codes under the oracle's book of the field's histogram."""
    bklen = 2 * exp.case.radius
    times = np.bincount(exp.ids(seq), minlength=len(exp.codes))
    hists = np.stack([np.bincount(c, minlength=bklen) for c in exp.codes]).astype(np.int64)
    hist = (hists * times[:, None]).sum(0) + np.bincount(exp.codes_tail, minlength=bklen)
    lens = oracle.huffman_lengths(np.minimum(hist, 2 ** 32 - 1).astype(np.uint32), bklen).astype(np.int64)
    return int((hist * lens).sum()), hist


# ---- on the device -----------------------------------------------------------------------------
INT_VIEW = {np.dtype(np.float32): "int32", np.dtype(np.float64): "int64", np.dtype(np.uint16): "int16"}
CHUNK_ELEMS = 1 << 27  # elements a gather or a comparison handles at a time


def _bits(a):
    """A host array as a device tensor of same-sized integers: -0.0 and NaN count in comparisons."""
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(getattr(np, INT_VIEW[a.dtype]))).cuda()


def _chunks(case):
    per = max(1, CHUNK_ELEMS // case.block_elems)
    for i0 in range(0, case.reps, per):
        yield i0, min(case.reps, i0 + per)


def device_field(case, alphabet, tail, seq):
    """The field on the device (never on the host): an index copy of the alphabet per chunk of blocks."""
    import torch

    ab, tb = _bits(alphabet), _bits(tail)
    ids = torch.from_numpy(np.asarray(seq, np.int64)).cuda()
    out = torch.empty(case.n, dtype=ab.dtype, device="cuda")
    be = case.block_elems
    for i0, i1 in _chunks(case):
        torch.index_select(ab, 0, ids[i0:i1], out=out[i0 * be:i1 * be].view(i1 - i0, be))
    out[case.reps * be:] = tb
    return out.view(torch.float32 if case.dtype == np.float32 else torch.float64)


def mismatches(case, got, per_block, tail, ids):
    """Elements of `got` (a device tensor of n elements) whose bits differ from the assembly of the
    host arrays per_block[ids] + tail -> (count, index of the first or -1)."""
    import torch

    pb, tb = _bits(per_block), _bits(tail)
    got = got.view(pb.dtype)
    assert got.numel() == case.n and pb.shape[1] == case.block_elems and tb.numel() == case.tail_elems
    ids = torch.from_numpy(np.asarray(ids, np.int64)).cuda()
    be = case.block_elems
    count, first = 0, -1
    spans = [(i0 * be, i1 * be, (i0, i1)) for i0, i1 in _chunks(case)] + [(case.reps * be, case.n, None)]
    for e0, e1, blk in spans:
        want = tb if blk is None else pb[ids[blk[0]:blk[1]]].view(-1)
        bad = got[e0:e1] != want
        c = int(bad.sum().item())
        if c and first < 0:
            first = e0 + int(torch.nonzero(bad)[0].item())
        count += c
        del want, bad
    return count, first


def max_abs_err(case, a, b):
    """max |a - b| in double over two device tensors, a chunk at a time."""
    worst = 0.0
    for e0 in range(0, case.n, CHUNK_ELEMS):
        worst = max(worst, (a[e0:e0 + CHUNK_ELEMS].double() - b[e0:e0 + CHUNK_ELEMS].double()).abs().max().item())
    return worst


def code_histogram(codes, bklen):
    """bincount of a device int16 tensor of codes, a chunk at a time -> host i64[bklen]."""
    import torch

    h = torch.zeros(bklen, dtype=torch.int64, device="cuda")
    for e0 in range(0, codes.numel(), CHUNK_ELEMS):
        c = codes[e0:e0 + CHUNK_ELEMS].to(torch.int32) & 0xFFFF
        h += torch.bincount(c, minlength=bklen)[:bklen]
    return h.cpu().numpy()
