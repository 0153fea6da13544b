// cusz_amd/csrc/brick_device.hh -- what the fused brick kernels for gfx950 share across their
// translation units (brick_scan.hip, brick_pack.hip, brick_stream.hip and, with brick_decode.hh on
// top, brick3_decode.hip, brick1_decode.hip, chunk_decode.hip).  In the brick pipeline the Lorenzo predictor feeds the Huffman packer (compress) and the Huffman decoder
// feeds the Lorenzo reconstructor directly (decompress).
//
// Reference semantics (unchanged, bit-exact): predictor lrz_c.cuhip.inl:275-372 (3D 8^3 tiles),
// reconstruct lrz_x.cuhip.inl:271-360, histogram hist.cuhip.inl:55-89, chunked MSB-first
// Huffman cells hf_kernels.cuhip.inl:97-157, canonical decode hf_kernels.cuhip.inl:331-396.
//
// MI355X layout.  A wave owns a brick of W x 8 x 8 elements (W = 64 V, V = 4: kBrickW, kBrickV;
// lane l holds x in [l V, l V + V)), in both encode passes: one histogram record (u16 counts: a
// brick has 16384 elements), one outlier slot and one reserved bitstream region per brick.  The
// Huffman chunk length is W, so every brick ROW (fixed y, z) is exactly one reference chunk:
// chunk c covers codes [c W, c W + W) of the linear (x-fastest) order.
//   pass 1 (brick_scan.hip, k_brick3_scan):  predict -> codes in brick order (byte rows; u16 rows
//                            when a code leaves the byte window, one mask bit per row), per-brick
//                            histogram (u16, kept for the plan), global histogram, outlier slots.
//                            Reads the input once.
//   host:                    canonical codebook from the global histogram (exact reference heap).
//   plan (brick_pack.hip, k_brick_plan):  a brick's bits = sum(hist_b[s] * len[s]); its region in
//                            the bitstream is that many bits plus one partial cell per row -- an
//                            upper bound, known BEFORE encoding, so every brick writes at a fixed
//                            offset: no look-back, no scratch, no gather.  The last block writes
//                            the headers.
//   pass 2 (brick_pack.hip, k_brick3_pack):  bricks last to first; codes (read back, not
//                            re-predicted) -> codewords -> pack each row (= chunk) into LDS cells
//                            -> store at region + running offset; par_nbit / par_entry; the
//                            brick's outlier slot is copied out.
//   decompress (brick3_decode.hip, k_brick3_decode): one wave per brick, one chunk per lane decoded
//                            in x-blocks of 64 symbols (32 for an f32 field of at least 12 bricks
//                            per CU) into an LDS code tile; the block is reconstructed (reference
//                            scan order) and stored as whole rows.  1-D: brick1_decode.hip; the
//                            chunk loop they share, decode_chunks4: brick_decode.hh.
// Single-pass mode (brick_stream.hip: k_brick3_sample, k_brick3_stream, k_brick3_stream_finish):
// the book comes from a 1/16 sample of 32 x 8 x 8 units before the field is predicted, and one
// pass -- a workgroup per brick, a wave per y-step -- predicts, sizes (look-back over the bricks)
// and packs each brick.
// The archive is the reference phf format: par_entry[c] points at chunk c (the reference decoder
// reads chunk c from there, hf_kernels.cuhip.inl:386-391); chunks are laid out brick by brick,
// and the few cells between a brick's last chunk and the next region are zero.
//
// Everything here has internal linkage or is __forceinline__: each .hip file compiles its own copy.
#pragma once

#include <algorithm>
#include <type_traits>

#include "archive_device.hh"
#include "common.hh"
#include "hf_device.hh"
#include "kernels.hh"
#include "lrz_device.hh"
#include "pub_device.hh"

namespace cusz_amd {

using namespace lrzd;

namespace {

constexpr int kBrickWaves = 4;  // waves per workgroup in the encode passes
constexpr int kBrickV = 4, kBrickW = 64 * kBrickV;  // elements per lane and per brick row (BrickGeom::V, W)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
constexpr uint32_t kBufRsrcW3 = 0x00020000;  // raw buffer resource word 3 (gfx9)
constexpr uint32_t kOOB = 0x80000000u;       // buffer offset past any range: the load returns 0

__device__ __forceinline__ uint32_t readlane(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }

// cache-policy bits of the encoders' field loads: 2 = nontemporal
// (config 2 pass 1 189 -> 163 us: the streamed field no longer evicts the code rows pass 2 reads)
constexpr int kScanLoadAux = 2;

// a lane's four elements of a row at byte offset `off` of a raw buffer: one 16-B load (f64: two);
// an offset past the range reads 0 and touches no memory
template <typename T, int AUX>
__device__ __forceinline__ void buffer_load4(__amdgpu_buffer_rsrc_t rs, uint32_t off, T (&dst)[kBrickV])
{
#pragma unroll
  for (int h = 0; h < (int)(kBrickV * sizeof(T) / 16); h++) {
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(off + 16 * h), 0, AUX);
    __builtin_memcpy(reinterpret_cast<char*>(&dst[0]) + 16 * h, &v, 16);
  }
}

// The rows of a brick, for the encoders that stream the field brick by brick (pass 1 and the
// single-pass encoder): raw buffer loads from the brick's origin, issued ahead of their use and
// across brick boundaries.  The brick's address work is done once (rows_of: its coordinates, the
// 64-bit origin, the descriptor); a row takes its in-brick offset and two compares.  That saves
// work in pass 1, whose rolled row loop would redo the brick's part every y-step; the single-pass
// encoder issues its eight rows in one straight line, where the compiler shares that part anyway,
// and uses the same pair for the one code path, at no measured gain.  Straight-line code: no
// per-row branches, so the waitcnt pass can count the loads exactly.
template <typename T>
struct StepLoader {
  const T* in;
  size_t plane;
  uint32_t lx, ly, lz, nbx, nby, nbricks;
  uint32_t lane;
  struct BrickRows {
    __amdgpu_buffer_rsrc_t rs;  // at the brick's origin, 8 planes long
    uint32_t nyv, nzv;          // rows y < nyv, z < nzv lie in the field (0: past the last brick)
  };
  // past the last brick the loads still issue (at brick 0's origin, past the range: they read 0
  // and touch no memory): every path issues the same loads, so the compiler counts the waits
  // (vmcnt(7) for the row loaded 8 rows ago, not vmcnt(0): compress -3 us, 1-D -9 us)
  __device__ __forceinline__ BrickRows rows_of(uint32_t brick) const
  {
    const bool live = brick < nbricks;
    const uint32_t b = live ? brick : 0u, bx = b % nbx, t = b / nbx, by = t % nby, bz = t / nby;
    const T* origin = in + (size_t)bz * 8 * plane + (size_t)by * 8 * lx + (size_t)bx * kBrickW;
    const uint32_t span = (uint32_t)(8 * plane * sizeof(T));  // < 2^31 (brick_geom)
    return {__builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(origin), 0, (int)span, (int)kBufRsrcW3),
            live ? min(8u, ly - by * 8) : 0u, live ? min(8u, lz - bz * 8) : 0u};
  }
  // row (y, z) of the brick; rows outside the field get an offset past the range and read 0
  __device__ __forceinline__ void issue_row(const BrickRows& br, uint32_t y, uint32_t z, T (&dst)[kBrickV]) const
  {
    const uint32_t span = (uint32_t)(8 * plane * sizeof(T));
    const bool ok = y < br.nyv && z < br.nzv;
    const uint32_t off = ok ? (z * (uint32_t)plane + y * lx) * (uint32_t)sizeof(T) + lane * (kBrickV * sizeof(T)) : span;
    buffer_load4<T, kScanLoadAux>(br.rs, off, dst);
  }
};

// The same two steps for linear bricks (1-D and 2-D pass 1): brick b is elements [b 64 W,
// (b + 1) 64 W) of the field, row r its r-th W.  The descriptor ends with the field, so rows past
// its end, and every row past the last brick (brick 0 with an empty range), read 0.
template <typename T>
struct LinearLoader {
  static constexpr uint32_t kBrickElems = 64 * kBrickW;
  const T* in;
  size_t n;
  uint32_t nbricks, lane;
  __device__ __forceinline__ __amdgpu_buffer_rsrc_t rows_of(uint32_t brick) const
  {
    const bool live = brick < nbricks;
    const size_t o = live ? (size_t)brick * kBrickElems : 0;
    const uint32_t span = live ? (uint32_t)(min((size_t)kBrickElems, n - o) * sizeof(T)) : 0u;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(in + o), 0, (int)span, (int)kBufRsrcW3);
  }
  __device__ __forceinline__ void issue_row(__amdgpu_buffer_rsrc_t rs, int row, T (&dst)[kBrickV]) const
  {
    buffer_load4<T, kScanLoadAux>(rs, ((uint32_t)row * kBrickW + lane * kBrickV) * (uint32_t)sizeof(T), dst);
  }
};

// Row packing (hfd::pack4_or_lj / hfd::pack_words into a wave's LDS cells), pass 2 and the
// single-pass encoder:
constexpr int kPackRowMax = (kBrickW * kLmax + 31) / 32 + 2;  // words one row's packing may touch

// four consecutive elements (16 B for f32, 32 B for f64) to / from 16-B aligned LDS
template <typename T>
__device__ __forceinline__ void lds_store4(T* p, const T (&v)[4])
{
#pragma unroll
  for (int i = 0; i < (int)sizeof(T) / 4; i++) {
    u32x4 w;
    __builtin_memcpy(&w, reinterpret_cast<const char*>(&v[0]) + 16 * i, 16);
    reinterpret_cast<u32x4*>(p)[i] = w;
  }
}
template <typename T>
__device__ __forceinline__ void lds_load4(const T* p, T (&v)[4])
{
#pragma unroll
  for (int i = 0; i < (int)sizeof(T) / 4; i++) {
    const u32x4 w = reinterpret_cast<const u32x4*>(p)[i];
    __builtin_memcpy(reinterpret_cast<char*>(&v[0]) + 16 * i, &w, 16);
  }
}

}  // namespace

// blocks of pass 2 (k_brick3_pack, brick_pack.hip) resident per CU, 0 when the query fails: for
// brick_configure (brick_scan.hip), which sizes both encode grids
int brick_pack_blocks_per_cu();

// Diagnostic build (make prof, psz_amd_debug_brick_profile): the decoders and the single-pass
// encoder sum per-phase clocks and counts over their waves into 16 counters.  A __device__ array
// is private to its translation unit, so each unit that counts keeps one, by BPROF_UNIT(fn) at
// namespace scope: the array, prof_add for a wave to add its counters, and fn, which adds the
// unit's counters to host[0..15] and clears them when `reset`.  psz_amd_debug_brick_profile
// (brick3_decode.hip) returns the sum over the units.
#ifdef CUSZ_AMD_DEC_PROFILE
#define BPROF(...) __VA_ARGS__
#define BPROF_UNIT(fn)                                                                             \
  namespace {                                                                                      \
  __device__ unsigned long long g_prof[16];                                                        \
  __device__ __forceinline__ void prof_add(const unsigned long long (&pc)[16], int lane)           \
  {                                                                                                \
    if (lane == 0)                                                                                 \
      for (int i = 0; i < 16; i++) atomicAdd(&g_prof[i], pc[i]);                                   \
  }                                                                                                \
  }                                                                                                \
  int fn(unsigned long long* host, int reset)                                                      \
  {                                                                                                \
    unsigned long long c[16] = {};                                                                 \
    const hipError_t e = hipMemcpyFromSymbol(c, HIP_SYMBOL(g_prof), sizeof(c));                    \
    for (int i = 0; i < 16; i++) host[i] += c[i];                                                  \
    const unsigned long long z[16] = {};                                                           \
    if (reset) (void)hipMemcpyToSymbol(HIP_SYMBOL(g_prof), z, sizeof(z));                          \
    return (int)e;                                                                                 \
  }
int brick3_profile(unsigned long long* host, int reset);        // brick3_decode.hip
int brick1_profile(unsigned long long* host, int reset);        // brick1_decode.hip
int chunk_profile(unsigned long long* host, int reset);         // chunk_decode.hip
int brick_stream_profile(unsigned long long* host, int reset);  // brick_stream.hip
#else
#define BPROF(...)
#define BPROF_UNIT(fn)
#endif

}  // namespace cusz_amd
