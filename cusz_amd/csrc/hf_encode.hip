// cusz_amd/csrc/hf_encode.hip -- the reference-layout Huffman encoder for gfx950: quant codes in
// index order -> the phf segment's par_nbit, par_entry and bitstream.
//
// Output format = the reference phf segment (codec/hf/src/hf_kernels.cuhip.inl:76-170,
// hf_buf.cc:111-139,191-211): chunk c covers codes [c*sublen, (c+1)*sublen); its codewords
// are packed MSB-first into u32 cells starting on a fresh cell; par_nbit[c] bits,
// par_entry[c] = exclusive scan of per-chunk cell counts; bitstream = concatenated cells.
//
// Three launches, not the reference's four phases with a host scan round trip, and no look-back: a
// decoupled look-back serialises workgroups on their predecessors' prefixes, and on MI355X that
// latency, not bandwidth, bounds it (measured in round 1).  Here:
//  (1) k_hf_pack: persistent waves, one chunk per wave at a time, codes prefetched a round
//      ahead; the chunk's cells go to a scratch slot at a fixed worst-case stride;
//  (2) k_hf_tile_sums: cells and bits per tile of 64 chunks; its last workgroup scans the tile
//      totals into tile offsets and sums the bits (past kFusedTiles tiles the same scan runs as
//      k_hf_tile_scan, a launch of its own);
//  (3) k_hf_gather: per tile, par_entry from the tile offset + an in-tile scan, then the
//      chunks' cells copied to their final place (coalesced).
// The extra 2 x (compressed bytes) of traffic is far cheaper than the look-back chain.
// (The brick layout has encoders of its own: brick_pack.hip, brick_stream.hip.)
#include "common.hh"
#include "hf_device.hh"
#include "kernels.hh"
#include "pub_device.hh"

namespace cusz_amd {

namespace {

// codes are read 16 per lane per round (two 16-B loads, issued for the next round before the
// current one is packed)
constexpr int kRound = 16;  // codes per lane per round

__device__ __forceinline__ void load_codes16(const uint16_t* p, int mine, uint32_t (&v)[8], bool vec)
{
  if (vec) {
    const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1];
    v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
  }
  else {
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const uint32_t lo = 2 * i < mine ? p[2 * i] : 0u, hi = 2 * i + 1 < mine ? p[2 * i + 1] : 0u;
      v[i] = lo | (hi << 16);
    }
  }
}

static int enc_wave_cellcap(int sublen) { return ((sublen * kLmax / 32 + 2) + 3) / 4 * 4; }
static size_t hf_encode_tile_words(int pardeg) { return 2 * (((size_t)pardeg + 63) / 64) + 4; }
constexpr int kPackWaves = 4;
// per-tile cell totals (tile = kGatherTile consecutive chunks)
constexpr int kGatherTile = 64;
// k_hf_tile_sums' last workgroup scans up to kFusedTiles tiles (one pass of its 256 threads); more go
// to k_hf_tile_scan, whose launch costs less than further passes (2,049 tiles: encode 117 against 120 us)
constexpr int kScanPer = 8;
constexpr int kFusedTiles = 256 * kScanPer;

__global__ void __launch_bounds__(64 * kPackWaves) k_hf_pack(HfEncodeArgs a, int cellcap)
{
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  uint32_t* s_book = smem;                          // bklen words (rounded to 4)
  uint32_t* s_cells = smem + ((a.bklen + 3) & ~3);  // kPackWaves * cellcap words
  for (int i = threadIdx.x; i < a.bklen; i += blockDim.x) s_book[i] = a.book[i];
  for (int i = threadIdx.x; i < kPackWaves * cellcap / 4; i += blockDim.x)
    reinterpret_cast<uint4*>(s_cells)[i] = make_uint4(0, 0, 0, 0);
  __syncthreads();

  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int stride = gridDim.x * kPackWaves;
  const int per = a.sublen / 64 < kRound ? a.sublen / 64 : kRound;  // codes per lane per round
  const int span = per * 64;
  const bool vec_ok = per == kRound;
  uint32_t* cells = s_cells + wid * cellcap;
  auto chunk_len = [&](int c) -> int {
    const size_t start = (size_t)c * a.sublen;
    return (int)((a.n - start) < (size_t)a.sublen ? (a.n - start) : (size_t)a.sublen);
  };
  auto load_round = [&](int c, int r0, int cnt, uint32_t(&v)[8]) {
    const int lo = r0 + lane * per, mine = min(max(cnt - lo, 0), per);
    load_codes16(a.codes + (size_t)c * a.sublen + lo, mine, v, vec_ok && mine == per);
  };

  int c = blockIdx.x * kPackWaves + wid;
  uint32_t nxt[8];
  if (c < a.pardeg) load_round(c, 0, chunk_len(c), nxt);
  for (; c < a.pardeg; c += stride) {
    const int cnt = chunk_len(c);
    uint32_t nbits = 0;
    for (int r0 = 0; r0 < cnt; r0 += span) {
      const int lo = r0 + lane * per, mine = min(max(cnt - lo, 0), per);
      uint32_t cur[8];
#pragma unroll
      for (int i = 0; i < 8; i++) cur[i] = nxt[i];
      if (r0 + span < cnt)  // prefetch: next round of this chunk, or the first of the next chunk
        load_round(c, r0 + span, cnt, nxt);
      else if (c + stride < a.pardeg)
        load_round(c + stride, 0, chunk_len(c + stride), nxt);
      uint32_t w[kRound], bits = 0;
#pragma unroll
      for (int i = 0; i < kRound; i++) {
        const uint32_t code = (cur[i >> 1] >> ((i & 1) * 16)) & 0xFFFFu;
        w[i] = i < mine ? s_book[code] : 0u;
        bits += w[i] >> 27;
      }
      const uint32_t inc = hfd::wave_incl_scan(bits);
      // full rounds whose 4-code groups each fit 64 bits (every lane): Horner-pack each group and
      // OR it in (hf_device.hh pack4_or); otherwise the general word-by-word packer
      uint32_t lg[kRound / 4];
      bool fast = mine == kRound;
#pragma unroll
      for (int g = 0; g < kRound / 4; g++) {
        lg[g] = (w[4 * g] >> 27) + (w[4 * g + 1] >> 27) + (w[4 * g + 2] >> 27) + (w[4 * g + 3] >> 27);
        fast = fast && lg[g] <= 64u;
      }
      if (__builtin_expect(__ballot(!fast) == 0, 1)) {
        uint32_t p = nbits + inc - bits;
#pragma unroll
        for (int g = 0; g < kRound / 4; g++) {
          const uint32_t wg[4] = {w[4 * g], w[4 * g + 1], w[4 * g + 2], w[4 * g + 3]};
          hfd::pack4_or(cells, p, wg, lg[g]);
          p += lg[g];
        }
      }
      else if (mine)
        hfd::pack_words<kRound>(cells, nbits + inc - bits, w, mine);
      nbits += __shfl(inc, 63);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    const uint32_t nc = (nbits + 31) >> 5;
    uint32_t* dst = a.temp + (size_t)c * cellcap;
    for (uint32_t i = lane; i < nc; i += 64) {
      dst[i] = cells[i];
      cells[i] = 0u;  // ready for the next chunk
    }
    if (lane == 0) a.par_nbit[c] = nbits;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
  }
}

// The exclusive scan of the tile totals in place, and the bit total, by one workgroup of NW waves
// (every thread calls it): kScanPer consecutive tiles per thread and pass, a carry between passes.
// (Agent-scope loads: k_hf_tile_sums' last workgroup reads what workgroups on other XCDs wrote.)
template <int NW>
__device__ __forceinline__ void scan_tiles(uint32_t* tile_sum, const uint32_t* tile_bits, int ntiles,
                                           unsigned long long* total_nbit)
{
  __shared__ uint32_t s_wc[NW];
  __shared__ unsigned long long s_wb[NW];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  unsigned long long tb = 0;  // this thread's share of the bit total
  uint32_t carry = 0;
  for (int base = 0; base < ntiles; base += 64 * NW * kScanPer) {
    uint32_t v[kScanPer], sum = 0;
#pragma unroll
    for (int k = 0; k < kScanPer; k++) {
      const int i = base + (int)threadIdx.x * kScanPer + k;
      v[k] = i < ntiles ? __hip_atomic_load(tile_sum + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
      tb += i < ntiles ? __hip_atomic_load(tile_bits + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
      sum += v[k];
    }
    const uint32_t inc = hfd::wave_incl_scan(sum);
    if (lane == 63) s_wc[wid] = inc;
    __syncthreads();
    uint32_t run = carry, tot = carry;
    for (int w = 0; w < NW; w++) tot += s_wc[w], run += w < wid ? s_wc[w] : 0u;
    run += inc - sum;
#pragma unroll
    for (int k = 0; k < kScanPer; k++) {
      const int i = base + (int)threadIdx.x * kScanPer + k;
      if (i < ntiles) tile_sum[i] = run;
      run += v[k];
    }
    carry = tot;
    __syncthreads();
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) tb += __shfl_xor(tb, d);
  if (lane == 0) s_wb[wid] = tb;
  __syncthreads();
  if (threadIdx.x == 0 && total_nbit) {
    unsigned long long tot = 0;
    for (int w = 0; w < NW; w++) tot += s_wb[w];
    *total_nbit = tot;
  }
}

// per-tile cell totals, one wave per tile.  With a ticket (kPubTicketWords words zeroed per call)
// the last workgroup also scans them (launch_hf_encode: up to kFusedTiles tiles, one launch fewer).
// (Per-tile bit totals, not one atomic per tile on the single total_nbit word: those queued
// 2,048 waves at the L2 -- 27 us for config 5's 131,072 chunks.)
__global__ void __launch_bounds__(256) k_hf_tile_sums(const uint32_t* __restrict__ par_nbit, int pardeg,
                                                      uint32_t* __restrict__ tile_sum, uint32_t* __restrict__ tile_bits,
                                                      int ntiles, uint32_t* ticket, unsigned long long* total_nbit)
{
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int t = blockIdx.x * 4 + wid;
  if (t < ntiles) {
    uint32_t acc = 0, bits = 0;
    for (int i = t * kGatherTile + lane; i < min((t + 1) * kGatherTile, pardeg); i += 64) {
      const uint32_t nb = par_nbit[i];
      acc += (nb + 31) >> 5;
      bits += nb;  // a tile of 64 chunks of <= 8192 codes of <= 27 bits: < 2^32
    }
    acc = hfd::wave_sum(acc);
    bits = hfd::wave_sum(bits);
    if (lane == 0) {  // (agent scope: the last workgroup may read them from another XCD)
      __hip_atomic_store(tile_sum + t, acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(tile_bits + t, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (ticket && last_block(ticket)) scan_tiles<4>(tile_sum, tile_bits, ntiles, total_nbit);
}

// the scan in a launch of its own: one workgroup of 16 waves, a pass for up to 8,192 tiles
__global__ void __launch_bounds__(1024) k_hf_tile_scan(uint32_t* __restrict__ tile_sum,
                                                      const uint32_t* __restrict__ tile_bits, int ntiles,
                                                      unsigned long long* total_nbit)
{
  scan_tiles<16>(tile_sum, tile_bits, ntiles, total_nbit);
}

// one workgroup per tile: wave 0 turns the tile offset + in-tile exclusive scan into
// par_entry; then the 4 waves copy the tile's chunks scratch -> bitstream, two chunks per wave
// per iteration with all their loads issued before the stores.
__global__ void __launch_bounds__(256) k_hf_gather(HfEncodeArgs a, int cellcap, const uint32_t* __restrict__ tile_off)
{
  __shared__ uint32_t s_ent[kGatherTile], s_nc[kGatherTile];
  const int t = blockIdx.x, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int c0 = t * kGatherTile;
  if (wid == 0) {
    const int c = c0 + lane;
    const uint32_t nc = c < a.pardeg ? (a.par_nbit[c] + 31) >> 5 : 0u;
    const uint32_t inc = hfd::wave_incl_scan(nc);
    const uint32_t off = tile_off[t] + inc - nc;
    s_ent[lane] = off, s_nc[lane] = nc;
    if (c < a.pardeg) a.par_entry[c] = off;
  }
  __syncthreads();
  const int nch = min(kGatherTile, a.pardeg - c0);
  for (int j = 2 * wid; j < nch; j += 8) {  // chunk pairs (j, j + 1)
    const int j2 = j + 1;
    const uint32_t n1 = s_nc[j], e1 = s_ent[j];
    const uint32_t n2 = j2 < nch ? s_nc[j2] : 0u, e2 = j2 < nch ? s_ent[j2] : 0u;
    const uint32_t* src1 = a.temp + (size_t)(c0 + j) * cellcap;
    const uint32_t* src2 = a.temp + (size_t)(c0 + j2) * cellcap;
    for (uint32_t i = lane; i < max(n1, n2); i += 256) {
      uint32_t v1[4], v2[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t ii = i + 64 * k;
        v1[k] = ii < n1 ? src1[ii] : 0u;
        v2[k] = ii < n2 ? src2[ii] : 0u;
      }
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t ii = i + 64 * k;
        if (ii < n1) a.bitstream[e1 + ii] = v1[k];
        if (ii < n2) a.bitstream[e2 + ii] = v2[k];
      }
    }
  }
}

}  // namespace

static_assert(kGatherTile == 64, "hf_encode_tile_words");
size_t hf_encode_temp_words(int sublen, int pardeg)
{  // chunk slots at a worst-case stride, then the per-tile cell and bit totals
  return (size_t)enc_wave_cellcap(sublen) * (size_t)pardeg + hf_encode_tile_words(pardeg);
}
static size_t hf_encode_tile_offset(int sublen, int pardeg)
{
  return hf_encode_temp_words(sublen, pardeg) - hf_encode_tile_words(pardeg);
}

// sublen: a multiple of 256 (the pipeline rounds it), so every chunk is a whole number of
// 16-code lane rounds of its wave
int launch_hf_encode(const HfEncodeArgs& a, hipStream_t st)
{
  if (!a.temp || !a.ticket || a.sublen % 64 != 0 || a.sublen > 8192) return (int)hipErrorInvalidValue;
  const int cellcap = enc_wave_cellcap(a.sublen);
  const size_t lds = (size_t)(((a.bklen + 3) & ~3) + kPackWaves * cellcap) * 4;
  int dev = 0, ncu = 0, per_cu = 0;
  (void)hipGetDevice(&dev);
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu < 1) ncu = 256;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_hf_pack, 64 * kPackWaves, lds) != hipSuccess ||
      per_cu < 1)
    per_cu = 1;
  const int need = (a.pardeg + kPackWaves - 1) / kPackWaves;
  const int grid = need < per_cu * ncu ? need : per_cu * ncu;
  k_hf_pack<<<grid, 64 * kPackWaves, lds, st>>>(a, cellcap);
  const int ntiles = (a.pardeg + kGatherTile - 1) / kGatherTile;
  uint32_t* tile_sum = a.temp + hf_encode_tile_offset(a.sublen, a.pardeg);
  uint32_t* tile_bits = tile_sum + ntiles;
  uint32_t* const ticket = ntiles <= kFusedTiles ? a.ticket : nullptr;
  k_hf_tile_sums<<<(ntiles + 3) / 4, 256, 0, st>>>(a.par_nbit, a.pardeg, tile_sum, tile_bits, ntiles, ticket,
                                                   a.total_nbit);
  if (!ticket) k_hf_tile_scan<<<1, 1024, 0, st>>>(tile_sum, tile_bits, ntiles, a.total_nbit);
  k_hf_gather<<<ntiles, 256, 0, st>>>(a, cellcap, tile_sum);
  return (int)hipGetLastError();
}

}  // namespace cusz_amd
