// cusz_amd/csrc/chunk_decode.hip -- the codes-only decoder on the fused decoders' chunk loop
// (brick_decode.hh): k_chunk_decode and its launcher, the default of launch_hf_decode.
#include "brick_decode.hh"

namespace cusz_amd {

BPROF_UNIT(chunk_profile)

namespace {

// ---- decode only: any layout -> codes in index order ------------------------------------------
// The fused decoders' chunk loop with the tile copied out instead of reconstructed: wave u
// decodes chunks [64 u, 64 u + 64) (lane = chunk), and after each block of 64 columns stores the
// tile as codes (two rows of 128 B per store instruction).  Used for every archive (chunk length
// a multiple of 64) the fused decoders do not take: 2-D, spline, the reference layout, a
// standalone decode of the codes.
__global__ void __launch_bounds__(64 * kDecWaves)
k_chunk_decode(const uint32_t* __restrict__ bitstream, uint32_t bs_words, const uint8_t* __restrict__ revbook,
               int bklen, const uint32_t* __restrict__ par_nbit, const uint32_t* __restrict__ par_entry,
               uint16_t* __restrict__ codes, size_t n, uint32_t nchunks, uint32_t sublen, uint32_t wpb)
{
  __shared__ hfd::Tab4 tb;
  extern __shared__ __attribute__((aligned(16))) uint8_t dsm[];
  BPROF(const unsigned long long tb0 = __builtin_readcyclecounter();)
  hfd::build_tab4(tb, revbook, bklen);
  const hfd::DecRegs4 rg = hfd::load_dec_regs4(tb);
  BPROF(const unsigned long long tb1 = __builtin_readcyclecounter();)
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint8_t* wbase = dsm + (size_t)wid * kD4Cells;  // ring + tile (no cell staging)
  uint16_t* tile = reinterpret_cast<uint16_t*>(wbase + kD4Tile);
  const DecWave4 dw = dec_wave4(bitstream, bs_words, wbase, tile, bklen, lane);
  // waves [wpb, 8) only help build the tables (launch_chunk_decode)
  const uint32_t nw = gridDim.x * wpb;
  const uint32_t nunits = (nchunks + 63) / 64;
  BPROF(unsigned long long pc[16] = {}; unsigned long long tk = __builtin_readcyclecounter(), tp = tk;)
  for (uint32_t u = blockIdx.x * wpb + wid; (uint32_t)wid < wpb && u < nunits; u += nw) {
    const size_t c = (size_t)u * 64u + (uint32_t)lane;
    const bool live = c < nchunks;
    const uint32_t nbit = live ? par_nbit[c] : 0u;
    const uint32_t vbase = (live ? par_entry[c] : 0u) * 4u;
    const uint32_t vlen = live ? (uint32_t)min((size_t)sublen, n - c * sublen) : 0u;
    auto recon = [&](int blk) {
      const uint32_t* t32 = reinterpret_cast<const uint32_t*>(tile);
      const uint32_t cp = (uint32_t)lane & 31u;  // column pair
#pragma unroll 4
      for (uint32_t it = 0; it < 32; it++) {
        const uint32_t row = 2u * it + ((uint32_t)lane >> 5);
        const uint32_t w = t32[row * (kTP4 / 2) + cp];
        const size_t e = ((size_t)u * 64u + row) * sublen + (uint32_t)blk * kBlk + 2u * cp;
        if ((uint32_t)blk * kBlk + 2u * cp >= sublen) continue;  // (sublen is a multiple of kBlk)
        if (e + 1 < n)
          *reinterpret_cast<uint32_t*>(codes + e) = w;
        else if (e < n)
          codes[e] = (uint16_t)w;
      }
    };
    BPROF(pc[0]++;)
    decode_chunks4(tb, rg, dw, live, vbase, nbit, vlen, [] {}, [](int) {}, recon BPROF_A4, sublen, nullptr);
  }
#ifdef CUSZ_AMD_DEC_PROFILE
  pc[11] += tb1 - tb0;  // table build (per wave)
  pc[12] += __builtin_readcyclecounter() - tb0;  // whole wave
  pc[13] += 1;
  prof_add(pc, lane);
#endif
}

}  // namespace

int launch_chunk_decode(uint32_t ncu, const PhfView& v, uint16_t* codes, size_t n, hipStream_t st)
{
  const uint32_t nchunks = (uint32_t)v.pardeg, sublen = (uint32_t)v.sublen;
  if (v.bs_words >= (1ull << 30) || v.bklen < 1 || v.bklen > kMaxBklen || sublen % kBlk != 0 || sublen == 0)
    return (int)hipErrorInvalidValue;
  if (!nchunks) return (int)hipSuccess;
  // Fewer units than 8 per CU (a 2-D field of a few million values): spread them over every CU,
  // ceil(units / nCU) decoding waves per workgroup, instead of 8 on a fifth of the chip; the
  // workgroup keeps 8 waves so the tables take no longer to build.
  const uint32_t units = (nchunks + 63) / 64;
  const uint32_t wpb = std::min<uint32_t>(kDecWaves, (units + ncu - 1) / ncu);
  const size_t lds = (size_t)wpb * kD4Cells;
  const uint32_t grid = std::max<uint32_t>(1, std::min<uint32_t>(ncu, (units + wpb - 1) / wpb));
  k_chunk_decode<<<grid, 64 * kDecWaves, lds, st>>>(v.bitstream, (uint32_t)v.bs_words, v.revbook, v.bklen, v.par_nbit,
                                                    v.par_entry, codes, n, nchunks, sublen, wpb);
  return (int)hipGetLastError();
}

}  // namespace cusz_amd
