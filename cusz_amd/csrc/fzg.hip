// cusz_amd/csrc/fzg.hip -- the FZG codec (codec1 = FZCodec): bit-plane shuffle + zero-word coder.
//
// No histogram, no codebook, nothing data-dependent is serial.  A unit is 256 consecutive symbols
// held by one wave64: lane l holds symbols 4l..4l+3 as one little-endian u64, and word w (0..63) of
// the unit is the ballot, over lanes, of bit w of that u64 -- a 64 x 64 bit transpose, its own
// inverse.  The unit's flag has bit w set iff word w is nonzero, its payload is the nonzero words
// in ascending w.  Small symbols leave the high planes of all four 16-bit fields zero, so a smooth
// field keeps a handful of the 64 words.  Segment layout: archive_layout.hh FzgLayout.
//
// Encode is three launches, and the archive is a pure function of the codes (placement comes from
// a prefix sum of popcounts, never from arrival order):
//   k_fzg_size  codes -> flags (a wave OR: bit w of the flag = some lane has bit w) and the words
//               of each block of 16 units, left in block_off[block]
//   k_fzg_scan  one workgroup: block_off -> its exclusive prefix, block_off[blocks] = total
//   k_fzg_pack  codes + flags + block_off -> the nonzero words at their offsets: one ballot per
//               SET flag bit (walked as scalar masks), so the work follows the output, not the 64 planes
// Decode (k_fzg_decode) is one launch: a wave takes its unit's words (rank r = the r-th set flag
// bit), rebuilds each lane's u64 from bit `lane` of every word, inverts the symbol transform and
// stores four codes per lane.  Every load and store of codes is checked against n; payload loads
// are checked against the segment's word count, so a corrupt flag or offset reads 0, never
// outside the archive.
//
// The reference ships a codec of this family (codec/fzg) that it never wires into its pipeline;
// the unit, the flag granularity, the transform and the deterministic placement here are this
// project's own.
#include "common.hh"
#include "hf_device.hh"
#include "kernels.hh"

namespace cusz_amd {

namespace {

constexpr int kUnitsPerWave = kFzgBlockUnits / 4;  // a workgroup of 4 waves takes one block

__device__ __forceinline__ uint32_t uniform32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t uniform64(uint64_t v)
{
  return (uint64_t)uniform32((uint32_t)v) | ((uint64_t)uniform32((uint32_t)(v >> 32)) << 32);
}

// t(c) = zigzag(c - radius): radius -> 0, radius -+ k -> 2k -+ 1 / 2k, the outlier code 0 -> 2 radius - 1
__device__ __forceinline__ uint32_t sym_of(uint32_t c, int radius, bool tr)
{
  if (!tr) return c;
  const int d = (int)c - radius;
  return ((uint32_t)(d << 1) ^ (uint32_t)(d >> 31)) & 0xFFFFu;
}
__device__ __forceinline__ uint32_t code_of(uint32_t s, int radius, bool tr)
{
  if (!tr) return s;
  const int d = (int)(s >> 1) ^ -(int)(s & 1u);
  return (uint32_t)(d + radius) & 0xFFFFu;
}

// symbols i..i+3 as one u64 (symbols at or past n: 0)
__device__ __forceinline__ uint64_t load_symbols(const uint16_t* __restrict__ codes, size_t n, size_t i, int radius, bool tr)
{
  uint64_t v = 0;
  if (i + 3 < n) {
    const uint64_t raw = *reinterpret_cast<const uint64_t*>(codes + i);
#pragma unroll
    for (int k = 0; k < 4; k++) v |= (uint64_t)sym_of((uint32_t)(raw >> (16 * k)) & 0xFFFFu, radius, tr) << (16 * k);
  }
  else {
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (i + k < n) v |= (uint64_t)sym_of(codes[i + k], radius, tr) << (16 * k);
  }
  return v;
}

__device__ __forceinline__ uint64_t wave_or(uint64_t v)
{
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v |= __shfl_xor(v, d);
  return v;
}

// Where the units of block b start: every wave loads the block's 16 flags (lanes 0..15) and scans
// their popcounts; unit q's flag and its first payload word come back wave-uniform.
struct BlockUnits {
  uint64_t flag;   // lane q < 16: unit q's flag
  uint32_t excl;   // lane q: words of the block before unit q
  __device__ __forceinline__ BlockUnits(const uint64_t* __restrict__ flags, size_t block, size_t units, int lane)
  {
    const size_t u = block * kFzgBlockUnits + (size_t)lane;
    flag = lane < (int)kFzgBlockUnits && u < units ? flags[u] : 0ull;
    const uint32_t pc = (uint32_t)__popcll(flag);
    excl = hfd::wave_incl_scan(pc) - pc;
  }
  __device__ __forceinline__ uint64_t flag_of(int q) const { return uniform64(__shfl(flag, q)); }
  __device__ __forceinline__ uint32_t start_of(int q) const { return uniform32(__shfl(excl, q)); }
};

__global__ void __launch_bounds__(256) k_fzg_size(const uint16_t* __restrict__ codes, size_t n, size_t units, int radius,
                                                  uint32_t transform, uint64_t* __restrict__ flags,
                                                  uint32_t* __restrict__ block_off)
{
  __shared__ uint32_t s_words[4];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const bool tr = transform == kFzgZigzagDelta;
  const size_t u0 = (size_t)blockIdx.x * kFzgBlockUnits + (size_t)wid * kUnitsPerWave;
  uint64_t v[kUnitsPerWave];
#pragma unroll
  for (int j = 0; j < kUnitsPerWave; j++) v[j] = load_symbols(codes, n, (u0 + j) * kFzgUnit + 4 * (size_t)lane, radius, tr);
  uint32_t words = 0;
#pragma unroll
  for (int j = 0; j < kUnitsPerWave; j++) {
    const uint64_t f = wave_or(v[j]);
    words += (uint32_t)__popcll(f);
    if (lane == 0 && u0 + j < units) flags[u0 + j] = f;
  }
  if (lane == 0) s_words[wid] = words;
  __syncthreads();
  if (threadIdx.x == 0) block_off[blockIdx.x] = s_words[0] + s_words[1] + s_words[2] + s_words[3];
}

// one workgroup: the words per block -> their exclusive prefix, in place; the total to
// block_off[blocks] and, in 4-byte cells, to the compress summary
__global__ void __launch_bounds__(1024) k_fzg_scan(uint32_t* __restrict__ block_off, uint32_t blocks, CompressInfo* info)
{
  __shared__ uint32_t s_wave[16];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < blocks; base += 4096) {
    const uint32_t i = base + 4 * (uint32_t)tid;
    uint32_t c[4];
#pragma unroll
    for (int k = 0; k < 4; k++) c[k] = i + k < blocks ? block_off[i + k] : 0u;
    const uint32_t own = c[0] + c[1] + c[2] + c[3];
    const uint32_t inc = hfd::wave_incl_scan(own);
    if (lane == 63) s_wave[wid] = inc;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 16; w++) {
      before += w < wid ? s_wave[w] : 0u;
      total += s_wave[w];
    }
    uint32_t r = carry + before + inc - own;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      if (i + k < blocks) block_off[i + k] = r;
      r += c[k];
    }
    carry += total;
    __syncthreads();
  }
  if (tid == 0) {
    block_off[blocks] = carry;
    if (!(blocks & 1u)) block_off[blocks + 1] = 0u;  // the pad word before the 8-byte aligned payload
    info->total_ncell = 2ull * carry;
  }
}

__global__ void __launch_bounds__(256) k_fzg_pack(const uint16_t* __restrict__ codes, size_t n, size_t units, int radius,
                                                  uint32_t transform, const uint64_t* __restrict__ flags,
                                                  const uint32_t* __restrict__ block_off, uint64_t* __restrict__ payload)
{
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const bool tr = transform == kFzgZigzagDelta;
  const size_t u0 = (size_t)blockIdx.x * kFzgBlockUnits + (size_t)wid * kUnitsPerWave;
  uint64_t v[kUnitsPerWave];
#pragma unroll
  for (int j = 0; j < kUnitsPerWave; j++) v[j] = load_symbols(codes, n, (u0 + j) * kFzgUnit + 4 * (size_t)lane, radius, tr);
  const BlockUnits bu(flags, blockIdx.x, units, lane);
  const size_t base = block_off[blockIdx.x];
#pragma unroll
  for (int j = 0; j < kUnitsPerWave; j++) {
    const int q = wid * kUnitsPerWave + j;
    const uint64_t fl = bu.flag_of(q);  // 0 past the last unit
    const size_t start = base + bu.start_of(q);
    // lane r keeps the r-th nonzero word: per set flag bit one AND with the bit's mask (f & -f,
    // scalar), the ballot, and two selects; the planes of the low and of the high 32 bits apart
    uint32_t mlo = 0, mhi = 0, r = 0;
#pragma unroll
    for (int half = 0; half < 2; half++) {
      const uint32_t vh = (uint32_t)(v[j] >> (32 * half));
      for (uint32_t f = (uint32_t)(fl >> (32 * half)); f; f &= f - 1, r++) {
        const uint64_t word = __ballot((vh & (f & (0u - f))) != 0u);
        if ((uint32_t)lane == r) mlo = (uint32_t)word, mhi = (uint32_t)(word >> 32);
      }
    }
    if ((uint32_t)lane < r) payload[start + (size_t)lane] = (uint64_t)mlo | ((uint64_t)mhi << 32);
  }
}

__global__ void __launch_bounds__(256) k_fzg_decode(FzgDecodeArgs a, size_t units)
{
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const bool tr = a.transform == kFzgZigzagDelta;
  const size_t u0 = (size_t)blockIdx.x * kFzgBlockUnits + (size_t)wid * kUnitsPerWave;
  const BlockUnits bu(a.flags, blockIdx.x, units, lane);
  const uint64_t base = a.block_off[blockIdx.x];
  uint64_t fl[kUnitsPerWave], mine[kUnitsPerWave];
#pragma unroll
  for (int j = 0; j < kUnitsPerWave; j++) {
    const int q = wid * kUnitsPerWave + j;
    fl[j] = bu.flag_of(q);
    const uint64_t idx = base + bu.start_of(q) + (uint64_t)lane;
    mine[j] = lane < __popcll(fl[j]) && idx < a.total_words ? a.payload[idx] : 0ull;
  }
#pragma unroll
  for (int j = 0; j < kUnitsPerWave; j++) {
    if (u0 + j >= units) break;  // wave-uniform
    // the r-th word, broadcast from lane r, carries this lane's bit of the r-th set plane
    uint32_t vh[2] = {0u, 0u}, r = 0;
#pragma unroll
    for (int half = 0; half < 2; half++)
      for (uint32_t f = (uint32_t)(fl[j] >> (32 * half)); f; f &= f - 1, r++) {
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)mine[j], (int)r);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(mine[j] >> 32), (int)r);
        const uint32_t mybit = (uint32_t)__builtin_amdgcn_sbfe((int)(lane < 32 ? lo : hi), (unsigned)(lane & 31), 1u);  // 0 or ~0
        vh[half] |= mybit & (f & (0u - f));
      }
    const uint64_t v = (uint64_t)vh[0] | ((uint64_t)vh[1] << 32);
    const size_t i = (u0 + j) * kFzgUnit + 4 * (size_t)lane;
    uint64_t out = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) out |= (uint64_t)code_of((uint32_t)(v >> (16 * k)) & 0xFFFFu, a.radius, tr) << (16 * k);
    if (i + 3 < a.n) *reinterpret_cast<uint64_t*>(a.codes + i) = out;
    else {
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (i + k < a.n) a.codes[i + k] = (uint16_t)(out >> (16 * k));
    }
  }
}

}  // namespace

int launch_fzg_encode(const FzgEncodeArgs& a, hipStream_t st)
{
  const FzgLayout l(a.n);
  if (!a.n || l.blocks > 0x7FFFFFFFu) return (int)hipErrorInvalidValue;
  const uint32_t blocks = (uint32_t)l.blocks;
  k_fzg_size<<<blocks, 256, 0, st>>>(a.codes, a.n, l.units, a.radius, a.transform, a.flags, a.block_off);
  k_fzg_scan<<<1, 1024, 0, st>>>(a.block_off, blocks, a.info);
  k_fzg_pack<<<blocks, 256, 0, st>>>(a.codes, a.n, l.units, a.radius, a.transform, a.flags, a.block_off, a.payload);
  return (int)hipGetLastError();
}

int launch_fzg_decode(const FzgDecodeArgs& a, hipStream_t st)
{
  const FzgLayout l(a.n);
  if (!a.n || l.blocks > 0x7FFFFFFFu) return (int)hipErrorInvalidValue;
  k_fzg_decode<<<(uint32_t)l.blocks, 256, 0, st>>>(a, l.units);
  return (int)hipGetLastError();
}

}  // namespace cusz_amd
