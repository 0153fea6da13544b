"""Crafted books and code streams for the Huffman ENCODERS (a plain helper module, no tests).

crafted_books.py lays code streams out for the decoders and hands them over as archives.  An
encoder takes a field, not codes, and builds its own book -- so two more steps are needed, both
closed forms that test_deep_books.py checks against the oracle on the CPU:

1. dyadic_hist(): psz_amd_compress_finish takes a caller's histogram, and the optimal code of the
   histogram hist[s] = 2^(27 - len[s]) is the profile's own length for every symbol (a dyadic
   distribution has one optimal code), so both codebook builders return the crafted book word for
   word and a test dictates the book an encoder packs with.
2. field_of_codes(): at eb = 0.5 a code c >= 1 is the Lorenzo delta c - radius and a code 0 an
   outlier delta; the field is the deltas' integral inside the Lorenzo tile (delta_fields.py), and
   the reconstruction is the field bit for bit.

encoder_census() says, on the CPU, what each stream does to the encoders' packers: per brick row
of 256 codes (k_brick3_pack, k_brick3_stream) the row's bits and how many of its 64 lanes -- a
lane holds four consecutive codes -- total more than, exactly, or less than 64 bits (more: the
general packer hfd::pack_words, else pack4_or_lj), in the order a brick's rows are packed in; per
round of 1024 codes of a reference-layout chunk (k_hf_pack at sublen >= 1024, 16 codes a lane)
whether the round takes the fast branch (every group of four <= 64 bits).

The single-process paths (the SAMPLED book on bricks, the STREAM single pass) take no histogram:
blind_codes() builds a field whose sampled bricks / units hold a Fibonacci-distributed handful of
symbols and whose rest uses symbols the sample never saw (weight 1 under sample + 1), which the
sampled book therefore gives codes of 23 bits (brick sample) and 19 bits (unit sample).
"""
import functools

import numpy as np

import crafted_books as cb
import delta_fields as df
from edge_fields import BRICK_ELEMS, BRICK_X

ROW = cb.ROW            # codes per brick row = per chunk of the brick layouts
LANE = 4                # codes per lane of a brick row; a lane round of k_hf_pack is 4 such groups
ROUND = 1024            # codes per wave round of k_hf_pack at sublen >= 1024 (64 lanes x 16)
FAST_BITS = 64          # a lane group of at most this many bits takes the fast packers


def dyadic_hist(book):
    """-> u32[bklen + 1]: 2^(27 - len) on the book's symbols, 0 elsewhere, overflow word 0."""
    lens = np.asarray(book.lens, np.int64)
    h = np.zeros(lens.size + 1, np.uint32)
    used = np.flatnonzero(lens)
    h[used] = (1 << (cb.LMAX - lens[used])).astype(np.uint32)
    return h


def field_of_codes(codes, dims, radius=512, dtype=np.float32):
    """-> (data, ol_idx u32[k] ascending, ol_val f32[k]): the field whose plain Lorenzo codes at
    eb = 0.5 are `codes`; a code 0 takes the outlier deltas of delta_fields.outlier_deltas in turn
    (the cell holds delta + radius)."""
    codes = np.asarray(codes, np.int64).reshape(-1)
    assert codes.size == int(np.prod(dims)) and codes.min() >= 0 and codes.max() < 2 * radius
    d = codes - radius
    idx = np.flatnonzero(codes == 0)
    d[idx] = np.resize(np.array(df.outlier_deltas(radius), np.int64), idx.size)
    f = df.integrate(d, dims)
    assert np.abs(f).max() < 2 ** 21, "partial differences and sums must stay exact in f32"
    return f.astype(dtype), idx.astype(np.uint32), (d[idx] + radius).astype(np.float32)


# ---- what a stream does to the packers ------------------------------------------------------------
def _rows(codes, lens):
    """Code lengths by row of ROW codes in index order, 0 past the end -> i64[nrow, ROW]."""
    wl = np.asarray(lens, np.int64)[np.asarray(codes).reshape(-1)]
    nrow = -(-wl.size // ROW)
    out = np.zeros(nrow * ROW, np.int64)
    out[:wl.size] = wl
    return out.reshape(nrow, ROW)


def brick_packing_order(dims):
    """-> [(rows i64[k], full)] per brick in brick order: the chunks (rows of ROW codes, index
    order) of the brick in the order k_brick3_pack packs them, and whether the brick is full.
    3-D: brick (bz, by, bx), rows y-major then z.  Linear bricks (y == 1 or z == 1): BRICK_ELEMS
    consecutive elements, position k holds row 4 (k mod 16) + k / 16."""
    x, y, z = dims
    out = []
    if z == 1:
        n = x * y
        nchunk = -(-n // ROW)
        k = np.arange(64)
        perm = 4 * (k % 16) + k // 16
        for b in range(-(-n // BRICK_ELEMS)):
            rows = 64 * b + perm
            rows = rows[rows < nchunk]
            out.append((rows, rows.size == 64 and n - b * BRICK_ELEMS >= BRICK_ELEMS))
        return out
    assert x % BRICK_X == 0
    nbx, nby, nbz = x // BRICK_X, (y + 7) // 8, (z + 7) // 8
    for bz in range(nbz):
        for by in range(nby):
            for bx in range(nbx):
                ys = np.arange(8 * by, min(8 * by + 8, y))
                zs = np.arange(8 * bz, min(8 * bz + 8, z))
                rows = ((zs[None, :] * y + ys[:, None]) * nbx + bx).reshape(-1)
                out.append((rows, rows.size == 64))
    return out


def encoder_census(codes, lens, dims, brick, sublen=ROW):
    """-> dict.  Always: row_bits i64[nrow]; group_bits, group_pos i64[nrow, 64] (a lane group's bits
    and the bit of its row it starts on); wide, exact, narrow i64[nrow]: the row's groups above, at
    and below FAST_BITS (groups without a code count as narrow).
    brick (a brick layout): bricks = brick_packing_order(dims).
    else (the reference layout, chunks of sublen codes): chunk_bits i64[pardeg], and for
    sublen a multiple of ROUND rounds = [bool[k]] per chunk: round r of the chunk takes
    k_hf_pack's fast branch (a full round, every group at most FAST_BITS)."""
    wl = _rows(codes, lens)
    n = np.asarray(codes).size
    gb = wl.reshape(wl.shape[0], ROW // LANE, LANE).sum(2)
    c = dict(row_bits=wl.sum(1), group_bits=gb, group_pos=np.cumsum(gb, 1) - gb,
             wide=(gb > FAST_BITS).sum(1), exact=(gb == FAST_BITS).sum(1), narrow=(gb < FAST_BITS).sum(1))
    if brick:
        assert sublen == ROW
        c["bricks"] = brick_packing_order(dims)
        return c
    flat = wl.reshape(-1)[:n]
    starts = np.arange(0, n, sublen)
    c["chunk_bits"] = np.add.reduceat(flat, starts)
    if sublen % ROUND == 0:   # (other chunk lengths end on a partial round: not modelled)
        ok =np.zeros(-(-n // ROUND) * ROUND // LANE, bool)   # a group: full and at most FAST_BITS
        g = flat[:n // LANE * LANE].reshape(-1, LANE).sum(1)
        ok[:g.size] = g <= FAST_BITS
        fast = ok.reshape(-1, ROUND // LANE).all(1)
        per = sublen // ROUND
        nround = -(-(np.minimum(starts + sublen, n) - starts) // ROUND)   # the last chunk may be short
        c["rounds"] = [fast[i * per:i * per + int(k)] for i, k in enumerate(nround)]
    return c


def census_line(c, row):
    """One row of the census as text (for a mismatch message)."""
    return (f"row {row}: {int(c['row_bits'][row])} bits, groups > 64: {int(c['wide'][row])}, == 64: "
            f"{int(c['exact'][row])}, < 64: {int(c['narrow'][row])}")


def switches(flags):
    """(a False directly followed by a True, a True directly followed by a False) in a sequence."""
    f = np.asarray(flags, bool)
    return bool(np.any(~f[:-1] & f[1:])), bool(np.any(f[:-1] & ~f[1:]))


# ---- a field the sampled books are blind to --------------------------------------------------------
BLIND_DIMS = (768, 128, 128)   # 768 bricks (every 3rd sampled), 6144 units of 32 x 8 x 8 (every 16th)
BLIND_SEEN = {"bricks": 17, "units": 14}   # symbols the sample sees (Fibonacci-distributed counts)
BLIND_UNSEEN = 3
BLIND_BASE = 400                # the seen symbols are BLIND_BASE + 7 i, the unseen ones follow


def sample_mask(oracle, dims, scheme):
    """bool[z, y, x]: the elements the codebook sample counts -- scheme "bricks": the bricks of
    oracle.sample_bricks (PSZ_AMD_CODEBOOK_SAMPLED); "units": the 32 x 8 x 8 units of the rule
    restated in oracle.sample_histogram (PSZ_AMD_CODEBOOK_STREAM)."""
    x, y, z = dims
    m = np.zeros((z, y, x), bool)
    if scheme == "bricks":
        nbx, nby, nbz = x // 256, (y + 7) // 8, (z + 7) // 8
        for b in oracle.sample_bricks(nbx * nby * nbz):
            bx, t = b % nbx, b // nbx
            by, bz = t % nby, t // nby
            m[bz * 8:bz * 8 + 8, by * 8:by * 8 + 8, bx * 256:bx * 256 + 256] = True
        return m
    nux, nuy, nuz = x // 32, (y + 7) // 8, (z + 7) // 8
    units = nux * nuy * nuz
    stride = 16 if units >= 256 * 16 else 1
    for i in range((units + stride - 1) // stride):
        u = i * stride + i % stride
        if u < units:
            ux, t = u % nux, u // nux
            uy, uz = t % nuy, t // nuy
            m[uz * 8:uz * 8 + 8, uy * 8:uy * 8 + 8, ux * 32:ux * 32 + 32] = True
    return m


def blind_symbols(scheme):
    seen = BLIND_BASE + 7 * np.arange(BLIND_SEEN[scheme])
    unseen = seen[-1] + 7 * np.arange(1, BLIND_UNSEEN + 1)
    return seen.astype(np.uint16), unseen.astype(np.uint16)


def blind_codes(oracle, scheme, dims=BLIND_DIMS, seed=3):
    """-> codes u16[n] (no code 0).  Sampled elements: the seen symbols with Fibonacci weights
    (symbol i about Fib(i + 1) times as often as the rarest).  The rest: the unseen symbols, iid --
    except that in bricks with by + bz odd the rows with (y + 2 z) % 5 == 0 hold seen symbols, so
    that a brick's rows switch between the packers."""
    x, y, z = dims
    rng = np.random.default_rng([seed, ("bricks", "units").index(scheme)])
    seen, unseen = blind_symbols(scheme)
    fib = np.ones(seen.size)
    for i in range(2, seen.size):
        fib[i] = fib[i - 1] + fib[i - 2]
    p = fib[::-1] / fib.sum()
    sampled = sample_mask(oracle, dims, scheme)
    gz, gy = np.arange(z)[:, None, None], np.arange(y)[None, :, None]
    mixed = ((gy // 8 + gz // 8) % 2 == 1) & ((gy + 2 * gz) % 5 == 0)
    from_seen = sampled | np.broadcast_to(mixed, sampled.shape)
    codes = unseen[rng.integers(0, unseen.size, (z, y, x))]
    k = int(np.count_nonzero(from_seen))
    codes[from_seen] = seen[rng.choice(seen.size, k, p=p)]
    return np.ascontiguousarray(codes.reshape(-1))


@functools.lru_cache(maxsize=None)
def blind_case(oracle, scheme):
    """-> (data f32, codes, book, revbook): the blind field of a scheme with the book the sampled
    compress builds for it (the two-queue book of the sample + 1)."""
    codes = blind_codes(oracle, scheme)
    hist = oracle.sample_histogram(codes, BLIND_DIMS, cb.BKLEN, scheme)
    book, rv = oracle.book_twoqueue(hist, cb.BKLEN, smooth=1)
    data, idx, _ = field_of_codes(codes, BLIND_DIMS)
    assert idx.size == 0
    for a in (data, codes, book, rv):
        a.setflags(write=False)
    return data, codes, book, rv


# ---- the streams and rows of test_gpu_deep_encode.py (test_deep_books.py checks each on the CPU) ----
SEED = 1
DIMS = {
    "b3": (512, 24, 17),             # 2 x 3 x 3 bricks, ragged z
    "b1": (16384 * 3 + 77, 1, 1),    # ragged last brick, short last chunk
    "b2": (300, 200, 1),             # 2-D linear bricks when forced: 3 full bricks and a ragged one
    "c2": (300, 200, 1),             # the reference layout
    "c3": (64, 48, 40),
}
BRICK_KEYS, REF_KEYS = ("b3", "b1", "b2"), ("c2", "c3")
REF_SUBLENS = (256, 512, 1024, 2048, 8192, None)   # None: the tuned default
STREAMS_EVERYWHERE = [(n, p) for n in cb.PROFILES for p in ("bands", "iid")] + [(n, "q75") for n in cb.Q75_PROFILES] + \
    [(n, "sparse16") for n in ("deep27", "long17")]   # (sparse16: rounds of k_hf_pack that alternate)
STREAMS_BRICKS = [(n, p) for n in ("deep27", "long17") for p in ("period3", "period5")]
SWITCHING = ("deep27", "bands")    # the stream whose rows switch packers in every full brick
EXACT_STREAM = ("every", "iid")    # the stream that also runs under CODEBOOK_EXACT on every row


def streams_of(dkey):
    return STREAMS_EVERYWHERE + (STREAMS_BRICKS if dkey in BRICK_KEYS else [])


@functools.lru_cache(maxsize=None)
def stream(name, pattern, dkey, dtype=np.float32):
    """-> (book, codes, data, ol_idx, ol_val), read-only: computed once per stream and dims."""
    dims = DIMS[dkey]
    b = cb.book_of(name)
    codes = cb.place(b, int(np.prod(dims)), pattern, SEED)
    data, oi, ov = field_of_codes(codes, dims, cb.BKLEN // 2, dtype)
    for a in (codes, data, oi, ov):
        a.setflags(write=False)
    return b, codes, data, oi, ov


@functools.lru_cache(maxsize=None)
def relabelled_stream(oracle):
    """The codes of edge_fields.burst_field("brick") (more than 128 outlier cells in one brick)
    under deep27's lengths dealt anti-optimally (crafted_books.relabel), as a field of its own."""
    import edge_fields as ef

    data0, dims, eb, radius = ef.burst_field("brick")
    assert dims == DIMS["b3"] and radius == cb.BKLEN // 2
    codes = oracle.lorenzo_c(data0, dims, eb, radius)[0]
    b = cb.relabel(codes, "deep27")
    data, oi, ov = field_of_codes(codes, dims, radius)
    for a in (codes, data, oi, ov):
        a.setflags(write=False)
    return b, codes, data, oi, ov
