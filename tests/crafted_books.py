"""Crafted canonical codebooks and code streams for the Huffman decoders (a plain helper module,
no tests).

The books that small test fields produce are shallow: an optimal code gives a symbol a length-L
code only if it is rarer than about 1 / Fib(L + 2), so a 200k-element field holds a 27-bit code
once at most and never a run of them.  Any complete prefix code is the optimal code of some
histogram, though, and a decompressor must decode whatever canonical book an archive carries.  So
the books here are canonised from chosen complete length profiles (PROFILES), and place() lays
their long codes out in the patterns that drive each decoder off its fast path: runs of the
longest code, one dense row among sparse ones, long codes at every step index of a quarter.
path_census() says, on the CPU, which decoder class (first table, second table, threshold search)
serves each code word of such a stream, so that test_crafted_books.py can check that a stream
reaches what it is meant to reach before test_gpu_deep_codes.py decodes it on the GPU.

Nothing here calls the oracle: canon() is checked against oracle.codebook, and the census's own
bit stream against oracle.hf_encode, in test_crafted_books.py.
"""
import functools

import numpy as np

BKLEN = 1024
LMAX = 27          # longest code a book word (code | len << 27) holds
ROW = 256          # place()'s patterns are laid out over rows of 256 codes (a brick row)
L1_BITS, L2_BITS = 12, 16
# usable second-table entries: kL2Cap4 (hf_device.hh) = kL2Cap (hf_decode.hip) = 2048, whose last slot
# stays 0; 4095 is the same edge of a 4096-entry table, which no decoder has: kept as a second cap
L2_CAPS = (2047, 4095)
KLASS_L1, KLASS_L2, KLASS_LONG = 0, 1, 2


def canon(lens):
    """lens u8[bklen] (0: unused) -> (book u32[bklen], revbook u8[256 + 2 bklen]), canonised as
    codebook.cc canonize / the reference do: first[max] = 0, first[l] = ceil((first[l + 1] +
    numl[l + 1]) / 2), first[0] = 0xff; entry[l] = codes shorter than l; keys ordered by (length,
    symbol); book word = code | len << 27, 0xFFFFFFFF for an unused symbol."""
    lens = np.asarray(lens, np.int64)
    bklen = lens.size
    assert lens.min() >= 0 and lens.max() <= LMAX
    numl = np.bincount(lens, minlength=32)[:32]
    numl[0] = 0
    entry = np.concatenate(([0], np.cumsum(numl)[:-1])).astype(np.int64)
    used = np.flatnonzero(lens)
    max_l = int(lens.max()) if used.size else 0
    first = np.zeros(32, np.int64)
    for l in range(max_l - 1, 0, -1):
        first[l] = (first[l + 1] + numl[l + 1] + 1) // 2
    first[0] = 0xFF
    keys = np.zeros(bklen, np.uint16)
    order = used[np.argsort(lens[used], kind="stable")]   # (length, symbol)
    keys[:order.size] = order
    book = np.full(bklen, 0xFFFFFFFF, np.uint32)
    l_of = lens[order]
    code = first[l_of] + np.arange(order.size) - entry[l_of]
    book[order] = ((code & 0x07FFFFFF) | (l_of << 27)).astype(np.uint32)
    rv = np.concatenate([first.astype(np.int32).view(np.uint8), entry.astype(np.int32).view(np.uint8),
                         keys.view(np.uint8)])
    assert rv.size == 256 + 2 * bklen
    return book, rv


def kraft_is_one(lengths):
    """Exactly complete, in integer arithmetic."""
    lengths = [int(l) for l in lengths]
    return bool(lengths) and min(lengths) >= 1 and max(lengths) <= LMAX and \
        sum(1 << (LMAX - l) for l in lengths) == 1 << LMAX


# name -> the multiset of code lengths (complete: Kraft sum exactly 1)
PROFILES = {
    # every length once: every threshold comparison of the long search, every L1 packing
    "every": list(range(1, 27)) + [27, 27],
    # runs at the maximum length: a 256-symbol row is 6912 bits
    "deep27": list(range(1, 19)) + [27] * 512,
    # the first length no table holds, just above the 3-D decoder's refill rate (16 bits a step)
    "long17": list(range(1, 9)) + [17] * 512,
    # runs of 16-bit codes out of the second table: exactly the refill rate
    "l2full": list(range(1, 8)) + [16] * 512,
    # first[12] = 256 and 256 << 4 = 4096 is past every second-table cap: the upper half of the
    # 13-bit codes falls through to the long search with l = 13
    "l2over": [1, 2, 3, 4] + [13] * 512,
    # control: first table only, never self-synchronising (the only profile that uses symbol 0)
    "flat10": [10] * 1024,
}
for _name, _lengths in PROFILES.items():
    assert kraft_is_one(_lengths), _name
PATTERNS = ("bands", "sparse16", "period3", "period5", "iid", "q75")
Q75_PROFILES = ("every", "deep27")   # the profiles that hold 16-bit codes and longer ones


class Book:
    """A canonical book over bklen symbols with its symbols grouped for place()."""

    def __init__(self, name, lens):
        self.name = name
        self.lens = np.asarray(lens, np.uint8)
        self.book, self.revbook = canon(self.lens)
        self.used = np.flatnonzero(self.lens).astype(np.uint16)
        ul = self.lens[self.used]
        self.longest = self.used[ul == ul.max()]
        self.shortest = self.used[ul == ul.min()]
        self.max_len, self.min_len = int(ul.max()), int(ul.min())


@functools.lru_cache(maxsize=None)
def book_of(name, seed=0):
    """The profile's lengths on symbols >= 1 by a seeded permutation (symbol 0, the outlier marker,
    stays unused; flat10 needs all 1024 symbols)."""
    lengths = np.array(PROFILES[name], np.uint8)
    rng = np.random.default_rng([seed, sorted(PROFILES).index(name)])
    lens = np.zeros(BKLEN, np.uint8)
    if lengths.size == BKLEN:
        lens[rng.permutation(BKLEN)] = lengths
    else:
        lens[1 + rng.permutation(BKLEN - 1)[:lengths.size]] = lengths
    return Book(name, lens)


def _as_book(profile):
    return profile if isinstance(profile, Book) else book_of(profile)


def place(profile, n, pattern, seed):
    """-> codes u16[n] of the profile's used symbols, patterned over rows of ROW codes:
    "bands":    rows cycle all-longest, all-shortest, iid over the used symbols -- neighbouring
                lanes (chunks) run at the longest, the shortest and a middling rate side by side;
    "sparse16": one all-longest row in 16 (row % 16 == 7), the rest all-shortest: one chunk far
                above the average;
    "period3", "period5": inside each row a longest code every 3rd / 5th symbol (the phase moves
                with the row), shortest ones between: the long code lands on every step index of a
                4-step quarter;
    "iid":      uniform over the used symbols;
    "q75":      every row three 16-bit codes, then a longest code, over and over: the densest
                quarter the compact decoder can take (quarter_load), for books that have both.
    A "longest" code is drawn from all symbols of the longest length, a "shortest" likewise."""
    b = _as_book(profile)
    rng = np.random.default_rng([seed, PATTERNS.index(pattern)])
    nrow = -(-n // ROW)


    def draw(pool, rows):
        if pool.size == 1:
            return np.full((rows, ROW), pool[0], np.uint16)
        return pool[rng.integers(0, pool.size, (rows, ROW))]

    row = np.arange(nrow)
    out = np.empty((nrow, ROW), np.uint16)
    if pattern == "bands":
        for k, pool in enumerate((b.longest, b.shortest, b.used)):
            out[row % 3 == k] = draw(pool, np.count_nonzero(row % 3 == k))
    elif pattern == "sparse16":
        dense = row % 16 == 7
        out[dense] = draw(b.longest, np.count_nonzero(dense))
        out[~dense] = draw(b.shortest, np.count_nonzero(~dense))
    elif pattern in ("period3", "period5"):
        p = int(pattern[-1])
        at = np.arange(ROW)[None, :] % p == row[:, None] % p
        out[:] = np.where(at, draw(b.longest, nrow), draw(b.shortest, nrow))
    elif pattern == "iid":
        out[:] = draw(b.used, nrow)
    elif pattern == "q75":
        ul = b.lens[b.used]
        assert b.max_len > L2_BITS and np.any(ul == L2_BITS), "q75 needs 16-bit codes and longer ones"
        out[:] = np.where(np.arange(ROW)[None, :] % 4 == 3, draw(b.longest, nrow), draw(b.used[ul == L2_BITS], nrow))
    else:
        raise ValueError(pattern)
    return np.ascontiguousarray(out.reshape(-1)[:n])


def relabel(codes, profile):
    """A Book that gives the profile's lengths to a real field's used symbols in anti-optimal order:
    the most frequent symbol takes the longest code (ties: the lower symbol first).  Lengths left
    over go to unused symbols >= 1, so the code stays complete.  The field's used symbols must fit
    the profile."""
    lengths = np.sort(np.array(PROFILES[profile], np.uint8))[::-1]
    hist = np.bincount(np.asarray(codes).reshape(-1), minlength=BKLEN)
    assert hist.size == BKLEN
    used = np.flatnonzero(hist)
    assert used.size <= lengths.size, f"{used.size} used symbols do not fit the {lengths.size} codes of {profile}"
    by_freq = used[np.argsort(-hist[used], kind="stable")]
    spare = np.setdiff1d(np.arange(1, BKLEN), used)[:lengths.size - used.size]
    lens = np.zeros(BKLEN, np.uint8)
    lens[np.concatenate([by_freq, spare])] = lengths
    return Book(profile + "/relabel", lens)


# ---- which decoder class serves each code word ---------------------------------------------------
def revbook_tables(revbook):
    """revbook -> (first i64[32], entry i64[32], keys u16[bklen], lens u8[bklen], code u32[bklen])."""
    rv = np.asarray(revbook, np.uint8)
    first = rv[:128].view(np.int32).astype(np.int64)
    entry = rv[128:256].view(np.int32).astype(np.int64)
    keys = rv[256:].view(np.uint16)
    bklen = keys.size
    lens = np.zeros(bklen, np.uint8)
    code = np.zeros(bklen, np.uint32)
    total = int(entry[31])  # (no code is 31 bits long)
    for l in range(1, 31):
        lo, hi = int(entry[l]), int(entry[l + 1])
        if hi > lo:
            syms = keys[lo:hi]
            lens[syms] = l
            code[syms] = first[l] + np.arange(hi - lo)
    assert total == int(np.count_nonzero(lens))
    return first, entry, keys, lens, code


def encode_bits(codes, revbook, sublen):
    """The reference-layout bit stream of `codes` in plain numpy -> (par_nbit u32[pardeg], par_entry
    u32[pardeg], bitstream u32[cells], word_len i64[n], word_bit i64[n], bits u8[32 cells + 64]):
    chunks of sublen codes, MSB first, each chunk from a fresh 32-bit cell; word_bit is a code
    word's first bit, counted from bit 0 of the stream; bits is the stream bit by bit (zeros
    after its end)."""
    codes = np.asarray(codes, np.uint16).reshape(-1)
    n = codes.size
    _, _, _, lens, code = revbook_tables(revbook)
    wl = lens[codes].astype(np.int64)
    assert wl.min() >= 1, "a code without a code word"
    pardeg = (n - 1) // sublen + 1
    starts = np.arange(pardeg) * sublen
    nbit = np.add.reduceat(wl, starts)
    ncell = (nbit + 31) >> 5
    entry = np.concatenate(([0], np.cumsum(ncell)[:-1]))
    cum = np.cumsum(wl) - wl                      # bits before the word, chunks packed tight
    chunk = np.arange(n) // sublen
    word_bit = cum - cum[starts][chunk] + 32 * entry[chunk]
    total_cells = int(ncell.sum())
    bits = np.zeros(32 * total_cells + 64, np.uint8)
    rep = np.repeat(np.arange(n), wl)
    k = np.arange(rep.size) - np.repeat(cum, wl)  # bit of the word, 0 = its most significant
    bits[word_bit[rep] + k] = (code[codes][rep] >> (wl[rep] - 1 - k).astype(np.uint32)) & 1
    stream = np.packbits(bits[:32 * total_cells]).view(">u4").astype(np.uint32)
    return nbit.astype(np.uint32), entry.astype(np.uint32), stream, wl, word_bit, bits


def path_census(codes, revbook, sublen=ROW):
    """For each code word of the stream (chunks of sublen, reference layout), the decoder class that
    serves it -> dict(len=i64[n], q16=i64[n], klass={cap: u8[n]}, par_nbit=u32[pardeg]):
    KLASS_L1 for a word of <= 12 bits; KLASS_L2 for one of 13..16 bits whose second-table index q16
    (the 16 stream bits from the word's first bit on: the word, then whatever follows it in the
    stream) is below the cap; KLASS_LONG (the threshold search) for a longer word or an index at or
    past the cap.  Caps: L2_CAPS."""
    nbit, _, _, wl, word_bit, bits = encode_bits(codes, revbook, sublen)
    q16 = np.zeros(wl.size, np.int64)
    for j in range(L2_BITS):
        q16 = (q16 << 1) | bits[word_bit + j]
    klass = {}
    for cap in L2_CAPS:
        k = np.full(wl.size, KLASS_LONG, np.uint8)
        k[(wl > L1_BITS) & (wl <= L2_BITS) & (q16 < cap)] = KLASS_L2
        k[wl <= L1_BITS] = KLASS_L1
        klass[cap] = k
    return dict(len=wl, q16=q16, klass=klass, par_nbit=nbit)


RING_START_BITS, REFILL_BITS_PER_QUARTER = 8 * 32, 4 * 32 // 2


def quarter_load(census, rows, cap=2047):
    """How hard the given rows of ROW code words (a lane's chunk at sublen 256) drive the compact
    decoder (brick_decode.hh decode_chunks4) -> (quarters i64[len(rows)], bits i64[len(rows)]).  A lane
    takes up to four table steps per quarter -- a step is one code word, or two first-table words
    of <= 12 bits together -- and a long-class word, found where a table step comes back empty,
    ends the quarter: at most 3 x 16 + 27 = 75 bits.  The lane starts with 8 words in its ring and
    gets 4 more per two quarters of its wave, so a wave all of whose rows hold
        bits > RING_START_BITS + REFILL_BITS_PER_QUARTER * quarters
    cannot decode them without its lanes waiting for words (the stall branch): must_stall()."""
    wl, klass = census["len"], census["klass"][cap]
    quarters, bits = [], []
    for r in rows:
        l, k = wl[r * ROW:(r + 1) * ROW], klass[r * ROW:(r + 1) * ROW]
        i = q = 0
        while i < l.size:
            q += 1
            for _ in range(4):
                if i >= l.size:
                    break
                if k[i] == KLASS_LONG:
                    i += 1
                    break
                i += 2 if k[i] == KLASS_L1 and i + 1 < l.size and l[i] + l[i + 1] <= L1_BITS else 1
        quarters.append(q)
        bits.append(int(l.sum()))
    return np.array(quarters), np.array(bits)


def must_stall(quarters, bits):
    return bits > RING_START_BITS + REFILL_BITS_PER_QUARTER * quarters


def longest_run(mask):
    """Length of the longest run of True."""
    m = np.concatenate(([0], np.asarray(mask, np.int8), [0]))
    d = np.flatnonzero(np.diff(m))
    return int((d[1::2] - d[0::2]).max()) if d.size else 0


def brick_order(ol_idx, dims):
    """Permutation that puts outlier cells in the order the fused 3-D decoders rank them in (the
    order this project's compressor writes): grouped by brick (bz, by, bx), inside a brick by
    row (y % 8) * 8 + z % 8, then x (brick3_decode.hip k_brick_cell_bounds)."""
    x, y, z = dims
    idx = np.asarray(ol_idx, np.int64)
    gx, gy, gz = idx % x, idx // x % y, idx // (x * y)
    nbx, nby = x // 256, (y + 7) // 8
    brick = (gz // 8 * nby + gy // 8) * nbx + gx // 256
    key = (brick << 14) | (((gy & 7) * 8 + (gz & 7)) << 8) | (gx & 255)
    return np.argsort(key, kind="stable")
