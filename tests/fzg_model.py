"""A numpy restatement of the FZG segment (codec1 = FZCodec), written from the format's description
(include/cusz_amd.h, DESIGN.md §4 "The FZG codec"), not from the kernels.

Symbols: the u16 codes as they are (LorenzoZigZag, transform 0) or zigzag(code - radius)
(Lorenzo, transform 1).  A unit is 256 symbols; lane l (0..63) holds symbols 4l..4l+3 as one
little-endian u64; word w (0..63) of the unit has bit l = bit w of lane l's u64 (a 64 x 64 bit
transpose).  flag bit w = word w is nonzero; the payload is the nonzero words in ascending w, unit
after unit.  Symbols past n in the last unit are 0.

segment = header 32 B: u32 magic "FZG1" | u32 256 | u32 transform | u32 units | u32 blocks | u32 0 | u64 words
        | u64 flags[units]
        | u32 block_off[blocks + 1] (payload words before each block of 16 units; [blocks] = total), padded to 8
        | u64 payload[words]
"""
import struct

import numpy as np

MAGIC = 0x31475A46
UNIT, BLOCK_UNITS = 256, 16
BLOCK = UNIT * BLOCK_UNITS
HEADER = struct.Struct("<6IQ")
PLAIN, ZIGZAG_DELTA = 0, 1


def symbols(codes, radius, zigzag):
    """codes -> symbols (u16).  zigzag: the predictor is LorenzoZigZag, whose codes are taken as they are."""
    codes = np.asarray(codes, np.uint16)
    if zigzag:
        return codes.copy()
    d = codes.astype(np.int32) - radius
    return (((d << 1) ^ (d >> 31)) & 0xFFFF).astype(np.uint16)


def codes_of(sym, radius, transform):
    sym = np.asarray(sym, np.uint16)
    if transform == PLAIN:
        return sym.copy()
    s = sym.astype(np.int32)
    d = (s >> 1) ^ -(s & 1)
    return ((d + radius) & 0xFFFF).astype(np.uint16)


def counts(n):
    return (n + UNIT - 1) // UNIT, (n + BLOCK - 1) // BLOCK


def offsets(n):
    """(flags, block_off, payload) byte offsets from the segment's start."""
    units, blocks = counts(n)
    off = HEADER.size + 8 * units
    return HEADER.size, off, (off + 4 * (blocks + 1) + 7) // 8 * 8


def _transpose(lanes):
    """(units, 64) u64 -> (units, 64) u64, bit l of out[u, w] = bit w of in[u, l]; its own inverse."""
    bits = np.unpackbits(np.ascontiguousarray(lanes).view(np.uint8).reshape(-1, 64, 8), axis=-1, bitorder="little")
    bits = bits.reshape(-1, 64, 64).transpose(0, 2, 1)
    return np.packbits(np.ascontiguousarray(bits), axis=-1, bitorder="little").reshape(-1, 64 * 8).view(np.uint64)


def encode(codes, radius, zigzag):
    sym = symbols(codes, radius, zigzag)
    n = sym.size
    units, blocks = counts(n)
    padded = np.zeros(units * UNIT, np.uint16)
    padded[:n] = sym
    words = _transpose(padded.view(np.uint64).reshape(units, 64))
    nz = words != 0
    flags = np.packbits(nz, axis=-1, bitorder="little").reshape(-1).view(np.uint64)
    per_unit = np.zeros(blocks * BLOCK_UNITS, np.int64)
    per_unit[:units] = nz.sum(axis=1)
    per_block = per_unit.reshape(blocks, BLOCK_UNITS).sum(axis=1)
    block_off = np.concatenate(([0], np.cumsum(per_block))).astype(np.uint32)
    payload = words[nz]
    _, off_rel, payload_rel = offsets(n)
    seg = bytearray(payload_rel + 8 * payload.size)
    HEADER.pack_into(seg, 0, MAGIC, UNIT, PLAIN if zigzag else ZIGZAG_DELTA, units, blocks, 0, payload.size)
    seg[HEADER.size:off_rel] = flags.tobytes()
    seg[off_rel:off_rel + 4 * (blocks + 1)] = block_off.tobytes()
    seg[payload_rel:] = payload.tobytes()
    return bytes(seg)


def parse(segment, n):
    magic, unit, transform, units, blocks, zero, total = HEADER.unpack_from(segment, 0)
    assert (magic, unit, zero) == (MAGIC, UNIT, 0) and (units, blocks) == counts(n)
    flags_rel, off_rel, payload_rel = offsets(n)
    assert len(segment) == payload_rel + 8 * total
    flags = np.frombuffer(segment, np.uint64, units, flags_rel)
    block_off = np.frombuffer(segment, np.uint32, blocks + 1, off_rel)
    payload = np.frombuffer(segment, np.uint64, total, payload_rel)
    return dict(transform=transform, units=units, blocks=blocks, total=total, flags=flags, block_off=block_off,
                payload=payload)


def decode(segment, n, radius=512):
    s = parse(segment, n)
    units = s["units"]
    nz = np.unpackbits(s["flags"].view(np.uint8).reshape(units, 8), axis=-1, bitorder="little").astype(bool)
    per_unit = nz.sum(axis=1)
    # a unit starts at its block's offset plus the words of the block's units before it
    starts = np.concatenate(([0], np.cumsum(per_unit)[:-1]))
    blk = np.arange(units) // BLOCK_UNITS
    first = np.concatenate(([0], np.cumsum(per_unit)))[blk * BLOCK_UNITS]
    assert np.array_equal(s["block_off"][blk] + (starts - first), starts) and s["block_off"][-1] == s["total"]
    words = np.zeros((units, 64), np.uint64)
    words[nz] = s["payload"]
    sym = _transpose(words).reshape(-1).view(np.uint16)
    assert not sym[n:].any()
    return codes_of(sym[:n], radius, s["transform"])
