// tests/host/layout_shim.cc -- C entry points over cusz_amd/csrc/archive_layout.hh, compiled by
// tests/test_archive_layout.py with plain g++ (the header is host-only) for a CPU-only check of
// the phf segment's offsets, the header templates and the decode-side view.
#include "archive_layout.hh"

using namespace cusz_amd;

// off[5]: phf_off, rvbk, nbit_rel, entry_rel, bits_rel
extern "C" void shim_layout(size_t anchor_bytes, int bklen, size_t pardeg, uint64_t* off)
{
  const PhfLayout l(anchor_bytes, bklen, pardeg);
  off[0] = l.phf_off, off[1] = l.rvbk, off[2] = l.nbit_rel, off[3] = l.entry_rel, off[4] = l.bits_rel;
}

// both templates start as 0xFF bytes: what the fill leaves alone in the psz header stays so, and
// the phf header comes back zeroed outside its static fields
extern "C" void shim_fill(size_t anchor_bytes, int bklen, int sublen, int pardeg, size_t n, psz_header* h,
                          phf_header* ph)
{
  std::memset(h, 0xFF, sizeof(*h));
  std::memset(ph, 0xFF, sizeof(*ph));
  fill_header_templates(PhfLayout(anchor_bytes, bklen, (size_t)pardeg), bklen, sublen, pardeg, n, psz_len{n, 1, 1}, h, ph);
}

// out[8]: bitstream, revbook, par_nbit, par_entry as byte offsets from `archive`; bs_words; bklen,
// sublen, pardeg
extern "C" void shim_view(const psz_header* h, const uint8_t* archive, int64_t* out)
{
  const PhfView v(h, archive);
  out[0] = reinterpret_cast<const uint8_t*>(v.bitstream) - archive;
  out[1] = v.revbook - archive;
  out[2] = reinterpret_cast<const uint8_t*>(v.par_nbit) - archive;
  out[3] = reinterpret_cast<const uint8_t*>(v.par_entry) - archive;
  out[4] = (int64_t)v.bs_words;
  out[5] = v.bklen, out[6] = v.sublen, out[7] = v.pardeg;
}
