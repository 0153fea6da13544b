// cusz_amd/csrc/codebook.hh -- the host codebook builders (codebook.cc).  Host only, no HIP header.
#pragma once

#include <cstdint>

namespace cusz_amd {

// book: u32[bklen]; revbook: 4*64 + 2*bklen bytes.  Both return the revbook's bytes.
int build_codebook(const uint32_t* hist, int bklen, uint32_t* book, uint8_t* revbook);
// the two-queue book of hist + smooth: the device builder's output (book_device.hh)
int build_codebook_twoqueue(const uint32_t* hist, int bklen, uint32_t smooth, uint32_t* book, uint8_t* revbook);

}  // namespace cusz_amd
