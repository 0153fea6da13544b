// tests/host/fzg_layout_shim.cc -- C entry points over the FZG part of cusz_amd/csrc/archive_layout.hh,
// compiled by tests/test_fzg_layout.py with plain g++ (the header is host-only): the segment's
// offsets, the header templates and the decode side's checks.  With FZG_SHIM_MAIN it is a
// stand-alone program that runs the checks over good and corrupt headers (for a sanitizer build).
#include "archive_layout.hh"

using namespace cusz_amd;

// off[6]: fzg_off, units, blocks, off_rel, payload_rel, worst_bytes
extern "C" void fzg_shim_layout(size_t n, uint64_t* off)
{
  const FzgLayout l(n);
  off[0] = l.fzg_off, off[1] = l.units, off[2] = l.blocks, off[3] = l.off_rel, off[4] = l.payload_rel;
  off[5] = l.worst_bytes();
}

// h starts as 0xFF bytes: what the fill leaves alone stays so; fh: the 32 header bytes
extern "C" void fzg_shim_fill(size_t n, uint32_t transform, psz_header* h, uint8_t* fh)
{
  std::memset(h, 0xFF, sizeof(*h));
  FzgHeader f;
  fill_fzg_templates(FzgLayout(n), transform, psz_len{n, 1, 1}, h, &f);
  std::memcpy(fh, &f, sizeof(f));
}

// the decode side's verdict on an archive in host memory: 0 ok, 1 the entries / span, 2 the
// segment's header or last offset.  Reads the segment only after span_ok(), as the pipeline does.
extern "C" int fzg_shim_check(const psz_header* h, size_t n, const uint8_t* archive)
{
  const FzgView v(h, n);
  if (!v.span_ok()) return 1;
  FzgHeader fh;
  uint32_t last;
  std::memcpy(&fh, archive + v.seg_off, sizeof(fh));
  std::memcpy(&last, archive + v.seg_off + v.last_off_rel(), 4);
  return v.ok(fh, last) ? 0 : 2;
}

#ifdef FZG_SHIM_MAIN
#include <cstdio>
#include <vector>

int main()
{
  int bad = 0;
  for (size_t n : {1ul, 255ul, 256ul, 257ul, 4095ul, 4096ul, 4097ul, 65537ul}) {
    const FzgLayout l(n);
    psz_header h;
    uint8_t fhb[32];
    fzg_shim_fill(n, kFzgZigzagDelta, &h, fhb);
    std::vector<uint8_t> a(l.fzg_off + l.payload_rel, 0);  // an archive with an empty payload
    std::memcpy(a.data() + l.fzg_off, fhb, 32);
    h.entry[PSZHEADER_SPFMT] = h.entry[PSZHEADER_ENC_PASS1_END] = h.entry[PSZHEADER_ENC_PASS2_END] = (uint32_t)a.size();
    bad += fzg_shim_check(&h, n, a.data()) != 0;
    psz_header t = h;  // truncated: the span check refuses before anything is read
    t.entry[PSZHEADER_SPFMT] = t.entry[PSZHEADER_ENC_PASS1_END] = t.entry[PSZHEADER_ENC_PASS2_END] = (uint32_t)a.size() - 8;
    std::vector<uint8_t> cut(a.begin(), a.end() - 8);
    bad += fzg_shim_check(&t, n, cut.data()) != 1;
    a[l.fzg_off + 12] ^= 1;  // unit count
    bad += fzg_shim_check(&h, n, a.data()) != 2;
  }
  std::printf("fzg layout checks: %d failures\n", bad);
  return bad != 0;
}
#endif
