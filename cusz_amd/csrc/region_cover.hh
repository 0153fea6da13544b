// cusz_amd/csrc/region_cover.hh -- what a region decode in PSZ_AMD_REGION_MODE_COVER touches: the
// tile-aligned slab of the slow axis that covers a box, and the chunks (Huffman) or blocks (FZG)
// that hold the slab's codes.  Host only, no HIP header: g++ alone compiles it
// (tests/host/region_plan_shim.cc).  The plan (pipeline_decode.cc region_plan) and the decode
// (Pipeline::decompress_slab) take their numbers from here and nowhere else.
//
// Lorenzo prediction restarts at every tile (1024 elements in 1-D, 64 V x 32 rows in 2-D,
// 64 V x 8 x 8 in 3-D), so the codes of whole tiles along the slow axis plus the outlier cells
// that fall among them reconstruct to the bits of the same elements of the whole field
// ("Region decode"; tests/test_region_slab_model.py).
//
// size_t throughout: a * P and b * P pass 2^32 on fields the project accepts.
#pragma once

#include <cstddef>

namespace cusz_amd {

struct RegionCover {
  size_t T;       // slab unit on the slow axis: 1024 elements (1-D), 32 rows (2-D), 8 planes (3-D)
  size_t P;       // elements per step of the slow axis: the product of the faster extents
  size_t a, b;    // the slab [a, b) on the slow axis: a = floor(o / T) T, b = min(len, ceil((o + e) / T) T)
  size_t c0, c1;  // the chunks (blocks) [c0, c1) that hold codes [a P, b P)
  size_t chunks() const { return c1 - c0; }
  size_t elems() const { return (b - a) * P; }
};

// nd: 1, 2 or 3 (pipeline.hh ndim_of); (lx, ly, lz) the field, o / e the box's origin and extent on
// the slow axis (x, y or z), which lies inside the field; sublen > 0: the chunk length (FZG: 4096),
// pardeg: the archive's chunk (block) count.
inline RegionCover region_cover(int nd, size_t lx, size_t ly, size_t lz, size_t o, size_t e, size_t sublen, size_t pardeg)
{
  RegionCover r{};
  r.T = nd == 3 ? 8 : nd == 2 ? 32 : 1024;
  r.P = nd == 3 ? lx * ly : nd == 2 ? lx : 1;
  const size_t len = nd == 3 ? lz : nd == 2 ? ly : lx;
  r.a = o / r.T * r.T;
  const size_t up = (o + e + r.T - 1) / r.T * r.T;
  r.b = up < len ? up : len;
  r.c1 = (r.b * r.P + sublen - 1) / sublen;
  if (r.c1 > pardeg) r.c1 = pardeg;
  r.c0 = r.a * r.P / sublen;
  if (r.c0 > r.c1) r.c0 = r.c1;  // (an archive with fewer chunks than its field needs)
  return r;
}

// The fused 1-D path (k_brick1_region): the tiles of 1024 elements [t0, t1) that cover the range
// [o, o + e), and the chunks of 256 they hold in a field of nchunks chunks.
struct Region1Tiles {
  size_t t0, t1;
  size_t chunks(size_t nchunks) const { return (4 * t1 < nchunks ? 4 * t1 : nchunks) - 4 * t0; }
};
inline Region1Tiles region_tiles1(size_t o, size_t e) { return Region1Tiles{o / 1024, (o + e + 1023) / 1024}; }

// the slow axis of a box: which of (x, y, z) region_cover's o and e are
template <class Len>
inline size_t slow_axis(int nd, const Len& v)
{
  return nd == 3 ? v.z : nd == 2 ? v.y : v.x;
}

}  // namespace cusz_amd
