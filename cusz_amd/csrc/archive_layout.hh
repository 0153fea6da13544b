// cusz_amd/csrc/archive_layout.hh -- where the Huffman (phf) segment's sections lie in an archive:
// the one host-side definition every writer (pipeline.cc's compress paths, merge.cc) and reader
// (the decode launches) takes its offsets from.  Host only, no HIP header: g++ alone compiles it
// (tests/host/layout_shim.cc).  archive_device.hh fills the size-dependent header fields on the
// device and relies on the same layout.
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
  }
};

}  // namespace cusz_amd
