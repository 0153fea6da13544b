// cusz_amd/csrc/archive_layout.hh -- where the Huffman (phf) segment's sections lie in an archive:
// the one host-side definition every writer (pipeline.cc's compress paths, merge.cc) and reader
// (the decode launches) takes its offsets from.  Host only, no HIP header: g++ alone compiles it
// (tests/host/layout_shim.cc).  archive_device.hh fills the size-dependent header fields on the
// device and relies on the same layout.  The FZG segment (codec1 = FZCodec), which takes the phf
// segment's place, is defined the same way at the end: FzgLayout to write, FzgView to read and check.
//
//   archive = [psz_header 176][anchors (spline)][phf segment][outlier cells]     (cusz/header.h)
//   phf     = [phf_header, padded to 128][revbook][par_nbit u32[pardeg]][par_entry u32[pardeg]]
//             [bitstream u32[total_ncell]]                            (hf.h, hf_buf.cc:199-211)
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

#include "cusz/header.h"
#include "hf.h"

namespace cusz_amd {

static_assert(sizeof(psz_header) == 176 && sizeof(phf_header) <= PHFHEADER_FORCED_ALIGN, "header sizes");

// reverse book: first i32[32] | entry i32[32] | keys u16[bklen]
inline size_t rvbk_bytes(int bklen) { return 4 * 64 + 2 * (size_t)bklen; }

struct PhfLayout {
  size_t phf_off;                                    // of the segment, from the archive's start
  size_t rvbk;                                       // reverse book bytes
  static constexpr size_t rvbk_rel = PHFHEADER_FORCED_ALIGN;
  size_t nbit_rel, entry_rel, bits_rel;              // sections, from the segment's start
  PhfLayout(size_t anchor_bytes, int bklen, size_t pardeg)  // anchors: spline only (compressor.inl:160)
      : phf_off(sizeof(psz_header) + anchor_bytes),
        rvbk(rvbk_bytes(bklen)),
        nbit_rel(rvbk_rel + rvbk),
        entry_rel(nbit_rel + 4 * pardeg),
        bits_rel(entry_rel + 4 * pardeg)
  {
  }
};

// The static fields of both headers: the psz header's chunking, extents and entries 0..2 (h keeps
// every other field), and a zeroed phf header's shape and entries 0..4.  The sizes -- splen, the
// later entries, total_nbit / total_ncell -- are known on the device (archive_device.hh) or to
// the merge.
inline void fill_header_templates(const PhfLayout& l, int bklen, int sublen, int pardeg, size_t n, psz_len len,
                                  psz_header* h, phf_header* ph)
{
  h->vle_sublen = sublen;
  h->vle_pardeg = pardeg;
  h->len = len;
  h->entry[PSZHEADER_HEADER] = 0;
  h->entry[PSZHEADER_ANCHOR] = (uint32_t)sizeof(psz_header);
  h->entry[PSZHEADER_ENCODED] = (uint32_t)l.phf_off;
  std::memset(ph, 0, sizeof(*ph));
  ph->bklen = bklen, ph->sublen = sublen, ph->pardeg = pardeg, ph->original_len = n;
  ph->entry[PHFHEADER_HEADER] = 0;
  ph->entry[PHFHEADER_RVBK] = (uint32_t)l.rvbk_rel;
  ph->entry[PHFHEADER_PAR_NBIT] = (uint32_t)l.nbit_rel;
  ph->entry[PHFHEADER_PAR_ENTRY] = (uint32_t)l.entry_rel;
  ph->entry[PHFHEADER_BITSTREAM] = (uint32_t)l.bits_rel;
}

// The decode side: the sections of an archive's phf segment, from the psz header alone (its
// segment entry, chunk count and radius -- not the phf header's own entries, which a decoder
// never reads).
struct PhfView {
  const uint32_t* bitstream;
  size_t bs_words;  // words from the bitstream's start to the archive's end (the range of the
                    // decoders' loads); 0 when entry[5] does not reach the bitstream
  size_t bits_words;  // the bitstream's own cells (to the outlier cells at entry[3]); 0 likewise
                      // (a chunks() view: its chunks' share, see there)
  const uint8_t* revbook;
  const uint32_t* par_nbit;
  const uint32_t* par_entry;
  int bklen, sublen, pardeg;
  size_t bits_rel;  // of the bitstream, from the segment's start

  PhfView(const psz_header* h, const uint8_t* archive)
      : bklen(2 * h->rc.radius), sublen(h->vle_sublen), pardeg(h->vle_pardeg)
  {
    const PhfLayout l(0, bklen, (size_t)pardeg);
    const size_t phf_off = h->entry[PSZHEADER_ENCODED];
    const uint8_t* phf = archive + phf_off;
    revbook = phf + l.rvbk_rel;
    par_nbit = reinterpret_cast<const uint32_t*>(phf + l.nbit_rel);
    par_entry = reinterpret_cast<const uint32_t*>(phf + l.entry_rel);
    bitstream = reinterpret_cast<const uint32_t*>(phf + l.bits_rel);
    bits_rel = l.bits_rel;
    const size_t bits_off = phf_off + l.bits_rel, total = h->entry[PSZHEADER_ENC_PASS2_END];
    bs_words = total > bits_off ? (total - bits_off) / 4 : 0;
    const size_t cells_off = h->entry[PSZHEADER_SPFMT];
    bits_words = cells_off > bits_off ? (cells_off - bits_off) / 4 : 0;
  }
  // Chunks [c0, c1) as a view of their own (0 <= c0 <= c1 <= pardeg): the decoders then write chunk
  // c0's codes at their output pointer.  The bitstream and its word counts stay, because
  // par_entry counts cells from the bitstream's start.  bits_words, which only sizes the WAVE
  // decoder's staging by the average chunk, becomes the range's share at the archive's average.
  PhfView chunks(size_t c0, size_t c1) const
  {
    PhfView v = *this;
    v.par_nbit += c0, v.par_entry += c0;
    v.bits_words = pardeg > 0 ? bits_words / (size_t)pardeg * (c1 - c0) : 0;
    v.pardeg = (int)(c1 - c0);
    return v;
  }
};

// ---- the FZG segment (codec1 = FZCodec; DESIGN.md §4, "The FZG codec") -----------------------
//   fzg = [FzgHeader 32][flags u64[units]][block_off u32[blocks + 1], padded to 8][payload u64[total_words]]
// It takes the phf segment's place at entry[PSZHEADER_ENCODED]; the outlier cells follow it.  A
// unit is 256 symbols (one wave64, 64 bit-plane words, flag bit w = word w is nonzero), a block is
// 16 units; block_off[b] counts the payload words before block b.
constexpr uint32_t kFzgMagic = 0x31475A46u;  // "FZG1"
constexpr uint32_t kFzgUnit = 256, kFzgBlockUnits = 16, kFzgBlock = kFzgUnit * kFzgBlockUnits;
enum : uint32_t { kFzgPlain = 0, kFzgZigzagDelta = 1 };  // symbol = code | zigzag(code - radius)

struct FzgHeader {
  uint32_t magic, unit, transform, units, blocks, reserved;
  uint64_t total_words;  // filled on the device
};
static_assert(sizeof(FzgHeader) == 32 && offsetof(FzgHeader, total_words) == 24, "FZG header");

struct FzgLayout {
  static constexpr size_t fzg_off = sizeof(psz_header);  // Lorenzo only: no anchors
  size_t units, blocks;
  static constexpr size_t flags_rel = sizeof(FzgHeader);
  size_t off_rel, payload_rel;  // sections, from the segment's start
  explicit FzgLayout(size_t n)
      : units((n + kFzgUnit - 1) / kFzgUnit),
        blocks((n + kFzgBlock - 1) / kFzgBlock),
        off_rel(flags_rel + 8 * units),
        payload_rel((off_rel + 4 * (blocks + 1) + 7) & ~(size_t)7)
  {
  }
  // every bit-plane word nonzero: 64 words a unit
  size_t worst_bytes() const { return payload_rel + 512 * units; }
};

// the psz header's static fields of an FZG archive and the segment header's (total_words: device)
inline void fill_fzg_templates(const FzgLayout& l, uint32_t transform, psz_len len, psz_header* h, FzgHeader* fh)
{
  h->vle_sublen = (int)kFzgBlock;
  h->vle_pardeg = (int)l.blocks;
  h->len = len;
  h->entry[PSZHEADER_HEADER] = 0;
  h->entry[PSZHEADER_ANCHOR] = (uint32_t)sizeof(psz_header);
  h->entry[PSZHEADER_ENCODED] = (uint32_t)l.fzg_off;
  *fh = FzgHeader{kFzgMagic, kFzgUnit, transform, (uint32_t)l.units, (uint32_t)l.blocks, 0u, 0ull};
}

// The decode side.  Before any launch the host checks the psz header's entries, the segment's own
// header and its last offset word (`fh` and `last_off`: the caller's copies of the segment's first
// 32 bytes and of block_off[blocks]; read them only after span_ok()).  ok() false: a bad archive.
struct FzgView {
  FzgLayout l;
  size_t seg_off, seg_bytes;  // the segment inside the archive (entry[ENCODED] .. entry[SPFMT])
  bool entries_ok;

  FzgView(const psz_header* h, size_t n) : l(n)
  {
    const uint32_t* e = h->entry;
    seg_off = e[PSZHEADER_ENCODED];
    entries_ok = e[PSZHEADER_SPFMT] >= e[PSZHEADER_ENCODED] && e[PSZHEADER_ENC_PASS2_END] >= e[PSZHEADER_SPFMT];
    seg_bytes = entries_ok ? e[PSZHEADER_SPFMT] - e[PSZHEADER_ENCODED] : 0;
  }
  // the header, flags and offsets lie inside the segment, 8-byte aligned in the archive
  bool span_ok() const { return entries_ok && seg_off % 8 == 0 && seg_off >= sizeof(psz_header) && seg_bytes >= l.payload_rel; }
  size_t last_off_rel() const { return l.off_rel + 4 * l.blocks; }
  bool ok(const FzgHeader& fh, uint32_t last_off) const
  {
    return span_ok() && fh.magic == kFzgMagic && fh.unit == kFzgUnit && fh.transform <= kFzgZigzagDelta &&
           fh.units == l.units && fh.blocks == l.blocks && fh.total_words == last_off &&
           fh.total_words <= 64 * l.units && seg_bytes == l.payload_rel + 8 * fh.total_words;
  }
};

}  // namespace cusz_amd
