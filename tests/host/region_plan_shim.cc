// tests/host/region_plan_shim.cc -- a C entry point over cusz_amd/csrc/region_cover.hh, compiled by
// tests/test_region_plan_cover.py with plain g++ (the header is host-only): the covering slab of a
// box and the chunks that hold its codes.  With REGION_SHIM_MAIN it is a stand-alone program that
// checks the cover of many boxes against a brute-force walk (for a sanitizer build).
#include <cstdint>

#include "region_cover.hh"

using namespace cusz_amd;

// out[6]: T, P, a, b, c0, c1
extern "C" void region_shim_cover(int nd, size_t lx, size_t ly, size_t lz, size_t o, size_t e, size_t sublen, size_t pardeg,
                                  uint64_t* out)
{
  const RegionCover c = region_cover(nd, lx, ly, lz, o, e, sublen, pardeg);
  out[0] = c.T, out[1] = c.P, out[2] = c.a, out[3] = c.b, out[4] = c.c0, out[5] = c.c1;
}

// out[2]: t0, t1 of the fused 1-D path; returns its chunk count
extern "C" size_t region_shim_tiles1(size_t o, size_t e, size_t nchunks, uint64_t* out)
{
  const Region1Tiles t = region_tiles1(o, e);
  out[0] = t.t0, out[1] = t.t1;
  return t.chunks(nchunks);
}

#ifdef REGION_SHIM_MAIN
#include <cstdio>
#include <initializer_list>

// every chunk that holds a code of the slab, found by walking the chunks
static int check(int nd, size_t lx, size_t ly, size_t lz, size_t sublen)
{
  const size_t n = lx * ly * lz, pardeg = (n + sublen - 1) / sublen;
  const size_t len = nd == 3 ? lz : nd == 2 ? ly : lx;
  int bad = 0;
  for (size_t o = 0; o < len; o += len > 4000 ? 997 : 1)
    for (size_t e = 1; o + e <= len; e += len > 4000 ? 1013 : 3) {
      const RegionCover c = region_cover(nd, lx, ly, lz, o, e, sublen, pardeg);
      bad += c.a > o || c.b < o + e || c.b > len || c.a % c.T || (c.b % c.T && c.b != len) || o - c.a >= c.T;
      size_t first = pardeg, last = 0;
      for (size_t k = 0; k < pardeg; k++) {
        const size_t k0 = k * sublen, k1 = k0 + sublen < n ? k0 + sublen : n;
        if (k0 < c.b * c.P && k1 > c.a * c.P) first = k < first ? k : first, last = k + 1;
      }
      bad += first != c.c0 || last != c.c1;
    }
  return bad;
}

int main()
{
  int bad = 0;
  bad += check(1, 50000, 1, 1, 256) + check(1, 200003, 1, 1, 256) + check(1, 200003, 1, 1, 4096);
  for (size_t s : {256ul, 2048ul, 8192ul}) bad += check(2, 300, 70, 1, s) + check(2, 301, 70, 1, s);
  bad += check(3, 96, 64, 40, 256) + check(3, 256, 20, 13, 256) + check(3, 96, 20, 13, 1024);
  // offsets past 2^32: a 2-D field of 2^31 + 2^24 rows of 4 elements
  const RegionCover c = region_cover(2, 4, ((size_t)1 << 31) + ((size_t)1 << 24), 1, ((size_t)1 << 31) + 5, 40, 256,
                                     (((size_t)1 << 33) + ((size_t)1 << 26)) / 256);
  bad += c.a != ((size_t)1 << 31) || c.b != ((size_t)1 << 31) + 64 || c.c0 != ((size_t)1 << 33) / 256 || c.c1 != c.c0 + 1;
  for (size_t n : {50000ul, 200003ul, ((size_t)1 << 32) - 5})  // tiles of the fused 1-D path, by walking the chunks
    for (size_t o = 0; o < n; o += n / 37 + 1)
      for (size_t e : {(size_t)1, (size_t)1024, (size_t)70001, n - o}) {
        if (o + e > n) continue;
        const size_t nchunks = (n + 255) / 256;
        const Region1Tiles t = region_tiles1(o, e);
        bad += t.t0 * 1024 > o || t.t1 * 1024 < o + e || o - t.t0 * 1024 >= 1024 || t.t1 * 1024 - (o + e) >= 1024;
        size_t cnt = 0;
        if (n < ((size_t)1 << 24))
          for (size_t k = 0; k < nchunks; k++) cnt += k * 256 < t.t1 * 1024 && k * 256 + 256 > t.t0 * 1024;
        else
          cnt = t.chunks(nchunks);
        bad += cnt != t.chunks(nchunks);
      }
  std::printf("region cover checks: %d failures\n", bad);
  return bad != 0;
}
#endif
