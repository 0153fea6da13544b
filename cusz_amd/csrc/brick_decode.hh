// cusz_amd/csrc/brick_decode.hh -- what the fused decoders (overview: brick_device.hh) share: the
// chunk loop decode_chunks4 and its constants, the decoders' output stores.  Built on it:
// k_brick3_decode (brick3_decode.hip), k_brick1_decode (brick1_decode.hip) and k_chunk_decode
// (chunk_decode.hip).
#pragma once

#include "brick_device.hh"

namespace cusz_amd {

namespace {

// =========================================================================================
// decompress: chunk decode + reconstruct, one wave per brick
// =========================================================================================
// Lane l decodes chunk l of the brick (brick row (y, z) = (l / 8, l % 8)) in blocks of 64 (or 32)
// symbols into an LDS code tile [row][column]; after each block the wave reconstructs it with
// lane = column (y running sums and z Hillis-Steele in registers, x Hillis-Steele across lanes by
// DPP) and stores whole rows.  The chunk loop is decode_chunks4, shared by every decoder kernel.
//
// Decode step.  The lane's state is its bit position and its tile pointer.  The window is read
// from the lane's LDS ring each step (word k in slot k % 16, [slot][lane]: conflict-free): words
// J and J + 1 by one ds_read2st64 (slot 16 mirrors slot 0, so the pair never wraps), shifted by
// alignbit -- no window registers to rotate, no word-crossing test; `pos8` = 8 x (the bit position
// + 511) masked by 0xF00 is the slot's byte offset, `npos` (= -position) the shift.  A step reads
// one table entry (hfd::Tab4: L1, one or two codes of <= 12 bits, or L2, one code of <= 16 bits,
// chosen by the window: they are exclusive); the tile pointer's advance, the bits and the symbols
// come out of the entry with one or two instructions each.  The loop is bound by how fast one
// wave issues this dependent chain (~15 VALU + 4 LDS per step), not by LDS or HBM bandwidth.
//
// Steps are grouped in quarters of kF: a lane takes part in a whole quarter or sits it out --
// it steps while its pointer is below the block's limit and the ring holds every word the quarter
// can reach (4 x 16 + 27 bits on) -- so the steps carry no predicates and no branch: a code longer
// than 16 bits reads entry 0, "no symbol, no bits", so the lane stands still, and one extra step
// after the quarter decodes it by threshold counting (hfd::lookup_long4) for the lanes that need
// it.  A lane may thus run up to 2 kF + 1 symbols past the block end, into the tile's 10 spare
// columns, which move to the block's front after the reconstruction.  Tile stores: each step
// writes both symbol slots of its entry as two naturally aligned u16 stores (ds_write_b16 /
// _d16_hi of one register; a compiler barrier keeps them from merging into a 2-B aligned b32
// store, which stalls the LDS pipeline); a slot past the entry's symbols is overwritten by the
// next step.
//
// Ring refills are wave-uniform, one group per two quarters: each lane issues one 16-B load of its
// next four words (or an out-of-range load that returns nothing, when its ring is full or its
// chunk read) and writes the group it loaded four quarters earlier.  The ring is drained at the
// block's end, so no load is in flight across the reconstruction's stores.
//
// LDS: the tables (hfd::Tab4) and, per wave, ring + tile + outlier staging let 8 waves (64-column
// blocks) or 12 waves (32-column blocks, Dec3Cfg) share a CU.
constexpr int kF = 4;         // decode steps per quarter
constexpr int kDecWaves = 8;  // waves per workgroup of the 1-D and the chunk decoder
constexpr int kBlk = 64;      // columns reconstructed per block (= lanes)

struct Empty {};  // the region parameter of a kernel's full-field instantiations

// what both region launchers ask of the field and the archive before they look at the box
inline bool region_launch_ok(const BrickLaunch& L, const PhfView& v, int ndim)
{
  return L.g.ok && L.g.ndim == ndim && L.g.W == 256 && v.bs_words < (1ull << 30) && v.bklen >= 1 && v.bklen <= kMaxBklen;
}

template <typename T>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const T* base)
{
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(base), 0, (int)0xFFFFFFFF, (int)kBufRsrcW3);
}
// cache-policy bits of the decoders' output stores: 2 = nontemporal
// (config 2 858 -> 893 GB/s: the written field no longer evicts what the next step reads)
constexpr int kOutStoreAux = 2;
template <typename T>
__device__ __forceinline__ void buf_store(T v, __amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff);
template <>
__device__ __forceinline__ void buf_store<float>(float v, __amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff)
{
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v), r, (int)voff, (int)soff, kOutStoreAux);
}
template <>
__device__ __forceinline__ void buf_store<double>(double v, __amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff)
{
  typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), r, (int)voff, (int)soff, kOutStoreAux);
}

// four consecutive elements (16 B for f32, 32 B for f64) at byte offset voff
template <typename T>
__device__ __forceinline__ void buf_store4(const T* v, __amdgpu_buffer_rsrc_t r, uint32_t voff)
{
  u32x4 w[sizeof(T) / 4];
  __builtin_memcpy(&w[0], v, 4 * sizeof(T));
#pragma unroll
  for (int i = 0; i < (int)sizeof(T) / 4; i++) __builtin_amdgcn_raw_buffer_store_b128(w[i], r, (int)(voff + 16 * i), 0, kOutStoreAux);
}

// Diagnostic build (brick_device.hh BPROF): per-phase clocks and counts summed over waves:
// 0 bricks, 1 brick-start cycles (cells, loads and their wait), 2 decode-loop cycles, 3 drain
// cycles, 4 reconstruct cycles, 5 loop iterations, 6 quarters, 7 quarters with a long-code step,
// 8 lane-quarters sat out for want of data, 9 lane-quarters short of the block's end (the 1-D
// kernel adds its reconstruction's cycles to 8 and 9; the chunk decoder uses 11-13)
#ifdef CUSZ_AMD_DEC_PROFILE
// decode_chunks4's extra parameters and arguments: the wave's counters and clocks
#define BPROF_P4 , unsigned long long(&pc)[16], unsigned long long &tk, unsigned long long &tp0
#define BPROF_A4 , pc, tk, tp
#else
#define BPROF_P4
#define BPROF_A4
#endif

constexpr int kTP4 = kBlk + 10;
static_assert(((kTP4 / 2) & 1) == 1, "odd dword pitch");
static_assert(kBlk + 2 * kF + 1 <= kTP4, "overshoot columns");
constexpr uint32_t kRing4 = 16;                             // ring words per lane (+ mirror, junk)
constexpr size_t kD4Tile = (size_t)(kRing4 + 2) * 256;       // slots 0..15, mirror 16, junk 17
constexpr size_t kD4Cells = kD4Tile + (size_t)64 * kTP4 * 2;  // ring + tile of 64-column blocks

// pos8 limit for entering a quarter: every word the quarter reads (<= 4 x 16 + 27 bits on) is in
// the ring (the window pair: p + 122 < 32 ctop)
constexpr uint32_t kRdy4 = 8u * (511u - 123u);

struct DecWave4 {
  __amdgpu_buffer_rsrc_t rbits;
  uint32_t* ring_lane;  // slot s of this lane at ring_lane[64 s]
  uint16_t* tile;
  uint32_t ubk;
  int lane;
};
// a wave's ring at wbase (slot s of lane l at word 64 s + l) and its tile, over the bitstream
__device__ __forceinline__ DecWave4 dec_wave4(const uint32_t* bitstream, uint32_t bs_words, uint8_t* wbase, uint16_t* tile,
                                              int bklen, int lane)
{
  return DecWave4{__builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(bitstream), 0, (int)(bs_words * 4u), (int)kBufRsrcW3),
                  reinterpret_cast<uint32_t*>(wbase) + lane, tile, (uint32_t)bklen, lane};
}

// One chunk per lane (bits at byte vbase, nbit bits, vlen <= W symbols; a dead lane decodes
// nothing; its first 8 words in first[0..1]) in W / kBlk blocks into the tile; recon(blk) after
// each block, blk_start(blk) before it, pro() while the first words are written.
template <int BLK = kBlk, int TP = kTP4, class Pro, class BlkStart, class Recon>
__device__ __forceinline__ void decode_chunks4(const hfd::Tab4& tb, const hfd::DecRegs4& rg, const DecWave4& dw,
                                               bool live, uint32_t vbase, uint32_t nbit, uint32_t vlen, Pro&& pro,
                                               BlkStart&& blk_start, Recon&& recon BPROF_P4, uint32_t W,
                                               const u32x4* first)
{
  const int lane = dw.lane;
  uint32_t* const ring = dw.ring_lane;
  const uint32_t nwords = live ? (nbit + 31u) >> 5 : 0u;
  u32x4 a0, a1;  // words 0..7: loaded by the caller ahead of time (first[0..1]), or now
  if (first)
    a0 = first[0], a1 = first[1];
  else {
    a0 = __builtin_amdgcn_raw_buffer_load_b128(dw.rbits, (int)(live ? vbase : kOOB), 0, 0);
    a1 = __builtin_amdgcn_raw_buffer_load_b128(dw.rbits, (int)(live ? vbase + 16u : kOOB), 0, 0);
  }
  pro();
  ring[0] = a0.x, ring[64] = a0.y, ring[2 * 64] = a0.z, ring[3 * 64] = a0.w;
  ring[4 * 64] = a1.x, ring[5 * 64] = a1.y, ring[6 * 64] = a1.z, ring[7 * 64] = a1.w;
  ring[16 * 64] = a0.x;  // mirror of slot 0
  uint32_t A = 0, Bw = a0.x;  // words J, J + 1 of the window (J = -1 at bit 0: junk, shift 0)
  uint32_t pos8 = 8u * 511u, npos = 0;  // 8 x (chunk bit position + 511); -position (the shift)
  uint32_t ltop = 8, ctop = 8;   // words requested / written to the ring
  // a quarter reaches at most 4 x 16 + 27 bits: the lane steps only if their words are in
  // (pos8 < 8 (32 ctop + 388))
  uint32_t rdy = ctop >= nwords ? 0xFFFFFFFFu : 256u * ctop + kRdy4;
  uint16_t* tp = dw.tile + lane * TP;
  u32x4 pa, pb;  // groups in flight
  bool fa = false, fb = false;
  BPROF(hfd::wave_sync(); tk = __builtin_readcyclecounter(); pc[1] += tk - tp0; tp0 = tk;)

  // next four words of the chunk, once their slots are free (words before J are)
  auto issue = [&](u32x4& p, bool& f) {
    const bool ok = ltop < nwords && ltop + 4u <= (pos8 >> 8);
    p = __builtin_amdgcn_raw_buffer_load_b128(dw.rbits, (int)(ok ? vbase + ltop * 4u : kOOB), 0, 0);
    f = ok;
    ltop += ok ? 4u : 0u;
  };
  // a landed group into its slots (and the mirror)
  auto consume = [&](const u32x4& p, bool& f) {
    if (f) {
      uint32_t* sl = ring + (ctop & (kRing4 - 1u)) * 64;
      sl[0] = p.x, sl[64] = p.y, sl[128] = p.z, sl[192] = p.w;
      if ((ctop & (kRing4 - 1u)) == 0u) ring[16 * 64] = p.x;
      ctop += 4u;
      rdy = ctop >= nwords ? 0xFFFFFFFFu : 256u * ctop + kRdy4;
    }
    f = false;
  };
  // the entry's symbols into the tile, the position forward, the next window read
  auto advance = [&](uint32_t e) {
    const uint32_t sy = e & hfd::kEnt4SymMask;
    tp[0] = (uint16_t)sy;
    asm volatile("" ::: "memory");  // two u16 stores: merged they would be an unaligned b32
    tp[1] = (uint16_t)(sy >> 16);
    tp = reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(tp) + hfd::ent4_adv(e));
    const uint32_t b = hfd::ent4_bits(e);
    pos8 += b << 3;
    npos -= b;
    const uint32_t* rr = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(ring) + (pos8 & 0xF00u));
    A = rr[0];
    Bw = rr[64];
  };
  auto window = [&]() { return __builtin_amdgcn_alignbit(A, Bw, npos); };

  for (int blk = 0; blk < (int)(W / BLK); blk++) {
    blk_start(blk);
    const uint32_t done = (uint32_t)blk * BLK;
    const uint32_t target = live && vlen > done ? min((uint32_t)BLK, vlen - done) : 0u;
    uint16_t* const tlim = dw.tile + lane * TP + target;
    auto quarter = [&]() {
      BPROF(pc[8] += __builtin_popcountll(__builtin_amdgcn_ballot_w64(tp < tlim && !(pos8 < rdy)));
            pc[9] += __builtin_popcountll(__builtin_amdgcn_ballot_w64(tp < tlim));)
      if (tp < tlim && pos8 < rdy) {
        uint32_t e = 0;
#pragma unroll
        for (int st = 0; st < kF; st++) {
          e = tb.e[hfd::tab4_index(rg, window())];
          advance(e);
        }
        BPROF(pc[7] += __builtin_amdgcn_ballot_w64(e == 0) ? 1 : 0;)
        if (__builtin_amdgcn_ballot_w64(e == 0)) {  // a code longer than 16 bits stopped the lane
          if (e == 0) advance(hfd::lookup_long4(tb, rg, window(), dw.ubk));
        }
      }
      BPROF(pc[6]++;)
    };
    // one group per two quarters (a lane reads at most 2 x 91 bits in them, 6 words: the ring
    // buffers the difference), each in flight for four quarters
    issue(pa, fa);
    quarter();
    quarter();
    issue(pb, fb);
    quarter();
    quarter();
    bool odd = false;
    // the block ends after the first quarter that leaves no lane short of it
    for (;;) {
      consume(pa, fa);
      issue(pa, fa);
      quarter();
      BPROF(pc[5]++;)
      if (!__builtin_amdgcn_ballot_w64(tp < tlim)) {
        odd = true;
        break;
      }
      quarter();
      if (!__builtin_amdgcn_ballot_w64(tp < tlim)) {
        odd = true;
        break;
      }
      consume(pb, fb);
      issue(pb, fb);
      quarter();
      BPROF(pc[5]++;)
      if (!__builtin_amdgcn_ballot_w64(tp < tlim)) break;
      quarter();
      if (!__builtin_amdgcn_ballot_w64(tp < tlim)) break;
    }
    BPROF(hfd::wave_sync(); tk = __builtin_readcyclecounter(); pc[2] += tk - tp0; tp0 = tk;)
    if (odd) consume(pb, fb);  // drain in issue order: nothing stays in flight across the stores
    consume(pa, fa);
    consume(pb, fb);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // a group no lane consumed may be in flight
    hfd::wave_sync();
    BPROF(tk = __builtin_readcyclecounter(); pc[3] += tk - tp0; tp0 = tk;)
    // symbols decoded past the block end move to its front; they are held in registers across
    // the reconstruction, which may use the tile as scratch
    uint32_t* rw = reinterpret_cast<uint32_t*>(dw.tile + lane * TP);
    uint32_t ovs[kF + 1];
#pragma unroll
    for (int i = 0; i <= kF; i++) ovs[i] = rw[BLK / 2 + i];
    recon(blk);
    hfd::wave_sync();
#pragma unroll
    for (int i = 0; i <= kF; i++) rw[i] = ovs[i];
    hfd::wave_sync();
    // next block's columns; a lane that stopped short of the block (a dead or short chunk)
    // restarts at column 0, where its (zero) target keeps it out of the quarters
    uint16_t* const row = dw.tile + lane * TP;
    tp = tp >= row + BLK ? tp - BLK : row;
    BPROF(tk = __builtin_readcyclecounter(); pc[4] += tk - tp0; tp0 = tk;)
  }
}

}  // namespace

}  // namespace cusz_amd
