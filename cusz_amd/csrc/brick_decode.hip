// cusz_amd/csrc/brick_decode.hip -- the fused brick decoders (overview: brick_device.hh): the chunk
// loop decode_chunks4 and the kernels built on it -- k_brick3_decode, k_brick3_region (a box of the
// field), k_brick1_decode and, as its REGION instantiation, k_brick1_region (a range of a 1-D field),
// k_chunk_decode (codes only) -- with k_brick_cell_bounds and the launchers.
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
//
// Outliers.  When the archive's cells are grouped by brick and sorted by (row, x) -- this
// compressor writes them so, k_brick_cell_bounds checks -- the k-th zero code of a row takes the
// row's k-th cell (values staged in LDS per brick), and no scatter pass runs; otherwise the
// scatter pass has written the values into `out`, where the reconstruction reads them.
constexpr int kF = 4;              // decode steps per quarter
constexpr int kDecWaves = 8;       // waves per workgroup of the 1-D and the chunk decoder
constexpr int kBlk = 64;           // columns reconstructed per block (= lanes)
constexpr uint32_t kCellCap = 128;  // outlier values of a brick kept in LDS

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

// Outlier values of one brick for the reconstruction, without the scatter pass: the archive's
// cells of the brick are contiguous and sorted by (row, x) (this compressor writes them so; a
// bounds pass checks it), so the k-th zero code of a row, in x order, takes the row's k-th cell.
// `val` holds the brick's values in LDS (or points at the archive's cells, stride 2 words, when
// the brick has more than fit), row_start[64 + 1] the first cell of each row, carry[64] the cells
// of each row consumed by earlier blocks.
struct BrickCells {
  const uint32_t* val;   // value bits of cell j at val[j * vstride]
  uint32_t vstride;
  uint32_t* row_start;   // LDS, 65 entries
  uint32_t* carry;       // LDS, 64 entries
};

// Column of the block a lane reconstructs.  Each 16-lane DPP row holds two 8-wide x tiles
// interleaved -- even lanes the first, odd lanes the second -- so the x Hillis-Steele step d reads
// lane - 2 d (row_shr 2 d) and the lanes whose source lies in the previous tile read past the DPP
// row, which returns 0: no selects (lrz_x.cuhip.inl:311-353 order d = 1, 2, 4; t + 0 == t).
__device__ __forceinline__ uint32_t rcol(uint32_t l) { return (l & 48u) | ((l & 1u) << 3) | ((l & 15u) >> 1); }

template <int CTRL>
__device__ __forceinline__ float dpp0(float v)
{
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
template <int CTRL>
__device__ __forceinline__ double dpp0(double v)
{
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)u, CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(u >> 32), CTRL, 0xf, 0xf, false);
  return __builtin_bit_cast(double, (unsigned long long)(uint32_t)lo | ((unsigned long long)(uint32_t)hi << 32));
}
// Each step must stay one v_add_*_dpp: left alone, the SLP vectorizer pairs two z rows' steps
// into v_mov_b32_dpp x 2 (plus two movs of the 0 `old`) + v_pk_add_f32, 5 instructions for 2;
// the empty asm makes every step's result opaque to it.
template <typename T>
__device__ __forceinline__ void no_slp(T& t)
{
  if constexpr (sizeof(T) == 4) asm("" : "+v"(t));  // (not volatile: free to schedule)
}
template <typename T>
__device__ __forceinline__ T x_scan8i(T t)
{
  t = t + dpp0<0x112>(t);  // row_shr:2 = column x - 1
  no_slp(t);
  t = t + dpp0<0x114>(t);  // row_shr:4 = column x - 2
  no_slp(t);
  t = t + dpp0<0x118>(t);  // row_shr:8 = column x - 4
  no_slp(t);
  return t;
}

// Rank, in column order, of this lane's zero code among the row's zero codes (m: ballot of the
// row's zero codes over lanes; rcol's order: DPP rows in turn, even lanes before odd lanes).
__device__ __forceinline__ uint32_t col_rank(uint64_t m, uint32_t l)
{
  const uint32_t r0 = l & 48u;
  const uint32_t below = (uint32_t)__builtin_popcountll(m & ((1ull << r0) - 1ull));
  const uint32_t row = (uint32_t)(m >> r0) & 0xFFFFu, li = l & 15u;
  const uint32_t before = (1u << li) - 1u;
  return below + ((l & 1u) ? (uint32_t)__builtin_popcount(row & 0x5555u) + (uint32_t)__builtin_popcount(row & 0xAAAAu & before)
                           : (uint32_t)__builtin_popcount(row & 0x5555u & before));
}

// Reconstruct columns [x0, x0 + 64) of the brick from the code tile (lane l = column rcol(l),
// row pitch TP).  lrz_x.cuhip.inl:271-360 order: v = (outlier + code) - r; y running sum
// (sequential); x then z Hillis-Steele; times 2 eb.  Outlier values (code 0) come from the ranked
// cells (CELLS) or from `out`, where the scatter pass has put them.  Stores address the block's
// row (y, z) as a buffer at base + y lx with z plane as the scalar offset.
// REGION (k_brick3_region): `out` is a compact box, not the field.  The sums run as for the whole
// block (rows 0 .. nyv - 1, planes 0 .. nzv - 1, which the caller has clipped to the box's far
// faces); only the elements inside the box are stored, each by a guarded global store at its
// index in the box -- no address before or past the box is ever formed.
struct RegionClip {
  uint32_t x0, y0, z0;  // field coordinates of the block's first element
  uint32_t ox, oy, oz;  // box origin
  uint32_t ex, ey, ez;  // box extent
};
template <typename T, bool ZZ, bool BUF, int TP, bool CELLS, bool REGION = false>
__device__ __forceinline__ void recon_block(const uint16_t* tile, T* out, size_t plane, uint32_t lx, uint32_t nyv,
                                            uint32_t nzv, size_t base_elem, T r, T ebx2, int lane,
                                            const BrickCells* bc = nullptr, const RegionClip* rc = nullptr)
{
  static_assert(!REGION || (CELLS && !BUF && !ZZ), "the region decoder reads ranked cells only");
  T* base = out + base_elem;  // element (x0, y0, z0) of this block
  const uint32_t col = rcol((uint32_t)lane);
  const uint32_t voff = col * (uint32_t)sizeof(T);
  const bool full = nyv == 8u && nzv == 8u;  // wave-uniform
  T s[8];
#pragma unroll
  for (int y = 0; y < 8; y++) {
    if ((uint32_t)y >= nyv) break;
    uint32_t cd[8];
#pragma unroll
    for (int z = 0; z < 8; z++) cd[z] = tile[(y * 8 + z) * TP + col];
    T v[8];
#pragma unroll
    for (int z = 0; z < 8; z++) {
      if constexpr (ZZ)
        v[z] = (T)zz_dec((uint16_t)cd[z]);
      else
        v[z] = (T)cd[z] - r;
    }
    const uint32_t mn = min(min(min(cd[0], cd[1]), min(cd[2], cd[3])), min(min(cd[4], cd[5]), min(cd[6], cd[7])));
    if (__builtin_amdgcn_ballot_w64(mn == 0u)) {  // a zero code in this y step (rare)
      if constexpr (CELLS) {  // outliers: ranked cells of the brick
#pragma unroll
        for (int z = 0; z < 8; z++) {
          const uint64_t m = __builtin_amdgcn_ballot_w64(cd[z] == 0u);
          if (m && (uint32_t)z < nzv) {
            const uint32_t row = (uint32_t)y * 8u + (uint32_t)z;
            const uint32_t c0 = bc->row_start[row] + bc->carry[row], ce = bc->row_start[row + 1];
            const uint32_t j = c0 + col_rank(m, (uint32_t)lane);
            if (cd[z] == 0u) v[z] = (j < ce ? (T)__builtin_bit_cast(float, bc->val[j * bc->vstride]) : T(0)) - r;
            hfd::wave_sync();
            if (lane == 0) bc->carry[row] += (uint32_t)__builtin_popcountll(m);
          }
        }
      }
      else {  // outliers: their values were scattered into out
        T ov[8];
#pragma unroll
        for (int z = 0; z < 8; z++) {
          ov[z] = T(0);
          if (__builtin_amdgcn_ballot_w64(cd[z] == 0u) && (uint32_t)z < nzv) ov[z] = base[(size_t)z * plane + (size_t)y * lx + col];
        }
#pragma unroll
        for (int z = 0; z < 8; z++)
          if (cd[z] == 0u) v[z] = ZZ ? ov[z] + T(0) : ov[z] - r;
      }
    }
    T t[8];
    if constexpr (sizeof(T) == 4) {
      // the same IEEE operations, two z rows per packed instruction where the operands pair up
      // (v_pk_add_f32 / v_pk_mul_f32): the y sums, the z Hillis-Steele steps d = 2, 4, the scale
      typedef float f2 __attribute__((ext_vector_type(2)));
#pragma unroll
      for (int j = 0; j < 4; j++) {
        f2 sv = {s[2 * j], s[2 * j + 1]};
        const f2 vv = {v[2 * j], v[2 * j + 1]};
        sv = y > 0 ? sv + vv : vv;
        s[2 * j] = sv.x, s[2 * j + 1] = sv.y;
        t[2 * j] = x_scan8i<T>(sv.x), t[2 * j + 1] = x_scan8i<T>(sv.y);
      }
#pragma unroll
      for (int z = 7; z >= 1; z--) t[z] = t[z] + t[z - 1];
      f2 tp[4];
#pragma unroll
      for (int j = 0; j < 4; j++) tp[j] = f2{t[2 * j], t[2 * j + 1]};
      tp[3] = tp[3] + tp[2], tp[2] = tp[2] + tp[1], tp[1] = tp[1] + tp[0];  // d = 2 (descending)
      tp[3] = tp[3] + tp[1], tp[2] = tp[2] + tp[0];                          // d = 4
#pragma unroll
      for (int j = 0; j < 4; j++) tp[j] = tp[j] * f2{(float)ebx2, (float)ebx2};
#pragma unroll
      for (int j = 0; j < 4; j++) t[2 * j] = tp[j].x, t[2 * j + 1] = tp[j].y;
    }
    else {
#pragma unroll
      for (int z = 0; z < 8; z++) {
        s[z] = y > 0 ? s[z] + v[z] : v[z];
        t[z] = x_scan8i<T>(s[z]);
      }
#pragma unroll
      for (int d = 1; d < 8; d *= 2)
#pragma unroll
        for (int z = 7; z >= d; z--) t[z] = t[z] + t[z - d];
#pragma unroll
      for (int z = 0; z < 8; z++) t[z] = t[z] * ebx2;
    }
    if constexpr (REGION) {
      // unsigned differences: a coordinate before the origin wraps past the extent
      const uint32_t bx = rc->x0 + col - rc->ox, by = rc->y0 + (uint32_t)y - rc->oy;
      if (bx < rc->ex && by < rc->ey) {
#pragma unroll
        for (int z = 0; z < 8; z++) {
          const uint32_t bz = rc->z0 + (uint32_t)z - rc->oz;
          // (32-bit index: the box is part of a field of fewer than 2^32 elements)
          if ((uint32_t)z < nzv && bz < rc->ez) out[(size_t)((bz * rc->ey + by) * rc->ex + bx)] = t[z];
        }
      }
      continue;
    }
    T* rowb = base + (size_t)y * lx;
    if constexpr (BUF) {
      const __amdgpu_buffer_rsrc_t ro = rsrc(rowb);
      if (full) {
#pragma unroll
        for (int z = 0; z < 8; z++) buf_store<T>(t[z], ro, voff, (uint32_t)((size_t)z * plane * sizeof(T)));
      }
      else {
#pragma unroll
        for (int z = 0; z < 8; z++)
          if ((uint32_t)z < nzv) buf_store<T>(t[z], ro, voff, (uint32_t)((size_t)z * plane * sizeof(T)));
      }
    }
    else {
#pragma unroll
      for (int z = 0; z < 8; z++)
        if ((uint32_t)z < nzv) rowb[(size_t)z * plane + col] = t[z];
    }
  }
}

// lanes 32-63: lane - 32's x; lanes 0-31: -0.0 (v_permlane32_swap: lanes 32-63 of the first
// operand trade with lanes 0-31 of the second)
template <typename T>
__device__ __forceinline__ T from_lower_half(T x)
{
  if constexpr (sizeof(T) == 4) {
    const auto s = __builtin_amdgcn_permlane32_swap(0x80000000u, __builtin_bit_cast(uint32_t, x), false, false);
    return __builtin_bit_cast(T, (uint32_t)s[0]);
  }
  else {
    const uint64_t u = __builtin_bit_cast(uint64_t, x);
    const auto lo = __builtin_amdgcn_permlane32_swap(0u, (uint32_t)u, false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap(0x80000000u, (uint32_t)(u >> 32), false, false);
    return __builtin_bit_cast(T, (uint64_t)(uint32_t)lo[0] | ((uint64_t)(uint32_t)hi[0] << 32));
  }
}

// 32-column blocks (the 12-wave decoder, k_brick3_decode32): lane l reconstructs column
// rcol(l mod 32) of y-steps 4 h .. 4 h + 3, h = l / 32, so both halves' x and z scans run
// together.  The y running sum keeps the reference's order: every lane sums its four values
// from a start value, -0.0 in the lower half (-0.0 + v == v for every v, so s_0 = v_0 exactly)
// and, in the upper half, the lower half's s_3 of the same column (v_permlane32_swap).
// Outliers: as recon_block, each row's zero codes ranked among the 32 lanes of its half.
template <typename T, bool ZZ, bool BUF, int TP, bool CELLS>
__device__ __forceinline__ void recon_block32(const uint16_t* tile, T* out, size_t plane, uint32_t lx, uint32_t nyv,
                                              uint32_t nzv, size_t base_elem, T r, T ebx2, int lane,
                                              const BrickCells* bc = nullptr)
{
  T* base = out + base_elem;  // element (x0, y0, z0) of this block
  const uint32_t hl = (uint32_t)lane >> 5, l32 = (uint32_t)lane & 31u;
  const uint32_t col = rcol(l32);
  const uint32_t ybase = 4u * hl;
  T v[4][8];
#pragma unroll
  for (int yy = 0; yy < 4; yy++) {
    const uint32_t y = ybase + (uint32_t)yy;
    const bool yok = y < nyv;
    uint32_t cd[8];
#pragma unroll
    for (int z = 0; z < 8; z++) cd[z] = tile[(y * 8 + (uint32_t)z) * TP + col];
#pragma unroll
    for (int z = 0; z < 8; z++) {
      if constexpr (ZZ)
        v[yy][z] = (T)zz_dec((uint16_t)cd[z]);
      else
        v[yy][z] = (T)cd[z] - r;
    }
    const uint32_t mn = min(min(min(cd[0], cd[1]), min(cd[2], cd[3])), min(min(cd[4], cd[5]), min(cd[6], cd[7])));
    if (__builtin_amdgcn_ballot_w64(yok && mn == 0u)) {  // a zero code in this y step (rare)
      if constexpr (CELLS) {  // outliers: ranked cells of the brick
#pragma unroll
        for (int z = 0; z < 8; z++) {
          const uint64_t m = __builtin_amdgcn_ballot_w64(yok && cd[z] == 0u);
          if (m && (uint32_t)z < nzv) {
            const uint32_t mh = (uint32_t)(m >> (32u * hl));  // this half's row
            const uint32_t row = y * 8u + (uint32_t)z;
            if (mh) {
              const uint32_t c0 = bc->row_start[row] + bc->carry[row], ce = bc->row_start[row + 1];
              const uint32_t j = c0 + col_rank((uint64_t)mh, l32);
              if (cd[z] == 0u) v[yy][z] = (j < ce ? (T)__builtin_bit_cast(float, bc->val[j * bc->vstride]) : T(0)) - r;
            }
            hfd::wave_sync();
            if (l32 == 0 && mh) bc->carry[row] += (uint32_t)__builtin_popcount(mh);
          }
        }
      }
      else {  // outliers: their values were scattered into out
#pragma unroll
        for (int z = 0; z < 8; z++) {
          if (yok && cd[z] == 0u && (uint32_t)z < nzv) {
            const T o = base[(size_t)z * plane + (size_t)y * lx + col];
            v[yy][z] = ZZ ? o + T(0) : o - r;
          }
        }
      }
    }
  }
  // y running sums: the lower half's s_3 (computed by every lane, used by the upper half)
  T c[8];
#pragma unroll
  for (int z = 0; z < 8; z++) {
    T u = v[0][z];
#pragma unroll
    for (int yy = 1; yy < 4; yy++) u = u + v[yy][z];
    c[z] = from_lower_half<T>(u);
  }
#pragma unroll
  for (int yy = 0; yy < 4; yy++) {
    const uint32_t y = ybase + (uint32_t)yy;
    T t[8];
#pragma unroll
    for (int z = 0; z < 8; z++) {
      c[z] = c[z] + v[yy][z];
      t[z] = x_scan8i<T>(c[z]);
    }
#pragma unroll
    for (int d = 1; d < 8; d *= 2)
#pragma unroll
      for (int z = 7; z >= d; z--) t[z] = t[z] + t[z - d];
#pragma unroll
    for (int z = 0; z < 8; z++) t[z] = t[z] * ebx2;
    if (y < nyv) {
      if constexpr (BUF) {
        const __amdgpu_buffer_rsrc_t ro = rsrc(base + (size_t)yy * lx);
        const uint32_t voff = (col + hl * 4u * lx) * (uint32_t)sizeof(T);
#pragma unroll
        for (int z = 0; z < 8; z++)
          if ((uint32_t)z < nzv) buf_store<T>(t[z], ro, voff, (uint32_t)((size_t)z * plane * sizeof(T)));
      }
      else {
        T* rowb = base + (size_t)y * lx;
#pragma unroll
        for (int z = 0; z < 8; z++)
          if ((uint32_t)z < nzv) rowb[(size_t)z * plane + col] = t[z];
      }
    }
  }
}

#ifdef CUSZ_AMD_DEC_PROFILE
// diagnostic build (psz_amd_debug_brick_profile): per-phase clocks and counts summed over waves:
// 0 bricks, 1 brick-start cycles (cells, loads and their wait), 2 decode-loop cycles, 3 drain
// cycles, 4 reconstruct cycles, 5 loop iterations, 6 quarters, 7 quarters with a long-code step,
// 8 lane-quarters sat out for want of data, 9 lane-quarters short of the block's end (the 1-D
// kernel adds its reconstruction's cycles to 8 and 9; the chunk decoder uses 11-13)
__device__ unsigned long long g_brick_prof[16];
// decode_chunks4's extra parameters and arguments: the wave's counters and clocks
#define BPROF_P4 , unsigned long long(&pc)[16], unsigned long long &tk, unsigned long long &tp0
#define BPROF_A4 , pc, tk, tp
#else
#define BPROF_P4
#define BPROF_A4
#endif

// Cells of a brick-layout archive: bstart[b] = first cell of brick b (nbricks + 1 entries) and
// *unsorted != 0 unless the cells are grouped by brick and sorted by (row, x) inside each brick
// -- key (brick, row = (y % 8) * 8 + z % 8, x % 256) strictly increasing: then every bstart
// entry is written; otherwise *unsorted = epoch (the word is never reset: no memset launch).
__global__ void __launch_bounds__(256) k_brick_cell_bounds(const uint32_t* __restrict__ cells, size_t ncell,
                                                           uint32_t lx, uint32_t ly, uint32_t lz, uint32_t nbx,
                                                           uint32_t nby, uint32_t nbricks, uint32_t* bstart,
                                                           uint32_t* unsorted, uint32_t epoch)
{
  auto key = [&](uint32_t idx, uint32_t& brick) -> uint64_t {
    const uint32_t x = idx % lx, yz = idx / lx, y = yz % ly, z = yz / ly;
    brick = (z < lz) ? ((z / 8) * nby + y / 8) * nbx + x / 256 : nbricks;
    return ((uint64_t)brick << 14) | (((y & 7u) * 8u + (z & 7u)) << 8) | (x & 255u);
  };
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < ncell; i += (size_t)gridDim.x * 256) {
    uint32_t b, bp = 0;
    const uint64_t k = key(cells[2 * i + 1], b);
    int64_t prev = -1;
    if (i > 0) {
      const uint64_t kp = key(cells[2 * i - 1], bp);
      if (kp >= k) *unsorted = epoch;
      prev = bp;
    }
    if (b >= nbricks) *unsorted = epoch;
    for (int64_t u = prev + 1; u <= (int64_t)b && u <= (int64_t)nbricks; u++) bstart[u] = (uint32_t)i;
    if (i + 1 == ncell)
      for (int64_t u = (int64_t)b + 1; u <= (int64_t)nbricks; u++) bstart[u] = (uint32_t)ncell;
  }
}

constexpr int kTP4 = kBlk + 10;
static_assert(((kTP4 / 2) & 1) == 1, "odd dword pitch");
static_assert(kBlk + 2 * kF + 1 <= kTP4, "overshoot columns");
constexpr uint32_t kRing4 = 16;                                // ring words per lane (+ mirror, junk)
constexpr size_t kD4Tile = (size_t)(kRing4 + 2) * 256;          // slots 0..15, mirror 16, junk 17
constexpr size_t kD4Cells = kD4Tile + (size_t)64 * kTP4 * 2;
constexpr size_t kD4Rows = kD4Cells + (size_t)kCellCap * 4;
constexpr size_t kD4WaveBytes = kD4Rows + (size_t)(65 + 64) * 4;
// 8 waves per CU: a 512^3 field's 8192 bricks are 4 full rounds of the 2048 waves (9 waves left
// a partial fourth round: decode 285 -> 259 us)
constexpr int kDec4Waves = 8;
static_assert(sizeof(hfd::Tab4) + kDec4Waves * kD4WaveBytes <= 160 * 1024, "LDS");

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

// Per block width: 64 columns (8 waves per CU, a 15 KB ring + tile per wave) or 32 columns (12
// waves per CU in 11 KB each: 3 waves per SIMD on the same LDS, recon_block32).  The step's chain
// of two LDS round trips bounds the loop, so a third wave per SIMD pays although a 512^3 field's
// 8192 bricks then make 2.67 rounds: f32 decompress 255 -> 229 us (config 2).  f64 keeps 64
// columns (at 32 its reconstruction spills 29-37 VGPRs).
// launch_brick_decode takes 32 for f32 fields of >= 12 bricks per CU, else 64.
template <int BLK>
struct Dec3Cfg {
  static constexpr int TP = BLK + 10;  // 9 overshoot columns, odd dword pitch
  static constexpr size_t kCells = kD4Tile + (size_t)64 * TP * 2;
  static constexpr size_t kRows = kCells + (size_t)kCellCap * 4;
  static constexpr size_t kWaveBytes = kRows + (size_t)(65 + 64) * 4;
  static constexpr int kWaves = BLK == 64 ? kDec4Waves : 12;
  static_assert(((TP / 2) & 1) == 1 && BLK + 2 * kF + 1 <= TP, "tile pitch");
  static_assert(sizeof(hfd::Tab4) + kWaves * kWaveBytes <= 160 * 1024, "LDS");
};

// What k_brick3_decode and k_brick3_region share.
// Wave `wid`'s part of the dynamic LDS (C = Dec3Cfg<BLK>): ring | tile | cell values | row starts
// (65) | row carries (64).
template <class C>
__device__ __forceinline__ void dec3_lds(uint8_t* dsm, int wid, uint8_t*& wbase, uint16_t*& tile, uint32_t*& cval,
                                         BrickCells& bc)
{
  wbase = dsm + (size_t)wid * C::kWaveBytes;
  tile = reinterpret_cast<uint16_t*>(wbase + kD4Tile);
  cval = reinterpret_cast<uint32_t*>(wbase + C::kCells);
  bc = BrickCells{cval, 1, reinterpret_cast<uint32_t*>(wbase + C::kRows), reinterpret_cast<uint32_t*>(wbase + C::kRows) + 65};
}
__device__ __forceinline__ DecWave4 dec3_wave(const uint32_t* bitstream, uint32_t bs_words, uint8_t* wbase, uint16_t* tile,
                                              int bklen, int lane)
{
  return DecWave4{__builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(bitstream), 0, (int)(bs_words * 4u), (int)kBufRsrcW3),
                  reinterpret_cast<uint32_t*>(wbase) + lane, tile, (uint32_t)bklen, lane};
}
// A brick's first 8 bitstream words per lane (its chunk at word `entry`; a dead lane reads nothing)
// and, when `cells`, the brick's outlier cells cb + lane and cb + 64 + lane below ce: {value, index}.
__device__ __forceinline__ void dec3_prefetch(const DecWave4& dw, const BrickOutliers& ol, bool live, uint32_t entry,
                                              bool cells, uint32_t cb, uint32_t ce, u32x4 (&first)[2], uint2 (&pcell)[2])
{
  first[0] = __builtin_amdgcn_raw_buffer_load_b128(dw.rbits, (int)(live ? entry * 4u : kOOB), 0, 0);
  first[1] = __builtin_amdgcn_raw_buffer_load_b128(dw.rbits, (int)(live ? entry * 4u + 16u : kOOB), 0, 0);
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const uint32_t j = cb + (uint32_t)dw.lane + 64u * k;
    pcell[k] = cells && j < ce ? make_uint2(ol.cells[2 * (size_t)j], ol.cells[2 * (size_t)j + 1]) : make_uint2(0, 0);
  }
}
// The brick's outlier cells [cb, ce), the first 128 of them prefetched in cp: per-row counts -> row
// starts; values into LDS (cval) when they fit.
__device__ __forceinline__ void dec3_stage_cells(BrickCells& bc, uint32_t* cval, const BrickOutliers& ol, uint32_t cb,
                                                 uint32_t ce, const uint2 (&cp)[2], uint32_t lx, uint32_t ly, int lane)
{
  const uint32_t nc = ce - cb;
  bc.row_start[lane] = 0;
  hfd::wave_sync();
  for (uint32_t j = (uint32_t)lane; j < nc; j += 64) {
    const uint2 cell = j < 64u    ? cp[0]
                       : j < 128u ? cp[1]
                                  : make_uint2(ol.cells[2 * (size_t)(cb + j)], ol.cells[2 * (size_t)(cb + j) + 1]);
    const uint32_t yz = cell.y / lx;  // y + ly z
    atomicAdd(&bc.row_start[((yz % ly) & 7u) * 8u + ((yz / ly) & 7u)], 1u);
    if (nc <= kCellCap) cval[j] = cell.x;
  }
  hfd::wave_sync();
  const uint32_t cr = bc.row_start[lane];
  const uint32_t incl = hfd::wave_incl_scan(cr);
  bc.row_start[lane] = incl - cr;
  if (lane == 63) bc.row_start[64] = incl;
  bc.carry[lane] = 0;
  bc.val = nc <= kCellCap ? cval : ol.cells + 2 * (size_t)cb;
  bc.vstride = nc <= kCellCap ? 1u : 2u;
}

template <typename T, bool ZZ, bool BUF, int BLK>
__global__ void __launch_bounds__(64 * Dec3Cfg<BLK>::kWaves)
k_brick3_decode(const uint32_t* __restrict__ bitstream, uint32_t bs_words, const uint8_t* __restrict__ revbook,
                int bklen, const uint32_t* __restrict__ par_nbit, const uint32_t* __restrict__ par_entry, T* out,
                uint32_t lx, uint32_t ly, uint32_t lz, T ebx2, T r, uint32_t nbx, uint32_t nby, uint32_t nbricks,
                BrickOutliers ol)
{
  __shared__ hfd::Tab4 tb;  // static: table addresses fold into the ds offsets
  extern __shared__ __attribute__((aligned(16))) uint8_t dsm[];
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  typedef Dec3Cfg<BLK> C;
  uint8_t* wbase;
  uint16_t* tile;
  uint32_t* cval;
  BrickCells bc;
  dec3_lds<C>(dsm, wid, wbase, tile, cval, bc);
  const bool ranked = !ZZ && (ol.ncell == 0 || *ol.unsorted != ol.epoch);
  const DecWave4 dw = dec3_wave(bitstream, bs_words, wbase, tile, bklen, lane);
  const size_t plane = (size_t)lx * ly;
  constexpr uint32_t W = 256;
  const uint32_t nw = gridDim.x * (blockDim.x >> 6);
  const uint32_t ry = (uint32_t)lane >> 3, rz = (uint32_t)lane & 7u;

  BPROF(unsigned long long pc[16] = {}; unsigned long long tk = __builtin_readcyclecounter(), tp = tk;)
  // A brick's chunk sizes / offsets and cell range are loaded during the previous brick's last
  // block (they land while it decodes), so a brick starts with the bitstream loads only.
  // Its first bitstream words and first two outlier cells per lane are loaded at the start of
  // the previous brick's last reconstruction (they land under its stores).
  struct Next {
    uint32_t nbit, entry, cb, ce;
    bool live;
  };
  auto fetch = [&](uint32_t b) {
    Next x{0, 0, 0, 0, false};
    if (b >= nbricks) return x;
    const uint32_t bx = b % nbx, t = b / nbx, by = t % nby, bz = t / nby;
    x.live = by * 8 + ry < ly && bz * 8 + rz < lz;
    if (x.live) {
      const size_t c = ((size_t)(bz * 8 + rz) * ly + (by * 8 + ry)) * nbx + bx;
      x.nbit = par_nbit[c], x.entry = par_entry[c];
    }
    if (ranked && ol.ncell) x.cb = ol.bstart[b], x.ce = ol.bstart[b + 1];
    return x;
  };
  u32x4 first[2];
  uint2 pcell[2];  // cells cb + lane and cb + 64 + lane of the next brick: {value, index}
  auto prefetch = [&](const Next& x) { dec3_prefetch(dw, ol, x.live, x.entry, ranked, x.cb, x.ce, first, pcell); };
  // a wave's first brick: 8 consecutive bricks per workgroup (they share par_nbit / par_entry /
  // bitstream lines in one L2), unless the field has fewer bricks than waves (a small slab): then
  // wave w of every workgroup takes brick w * grid + block, spreading them over every CU (one per
  // SIMD for 1024 bricks) instead of filling half the CUs two waves per SIMD
  // (32-column blocks: always wave-major, so that the bricks' last, partial round is spread over
  // every CU instead of ending on the first 170)
  const uint32_t b0 = BLK == 32 || nbricks <= nw ? (uint32_t)wid * gridDim.x + blockIdx.x : blockIdx.x * (blockDim.x >> 6) + wid;
  Next nx = fetch(b0);  // (lands while the tables are built)
  hfd::build_tab4(tb, revbook, bklen);
  const hfd::DecRegs4 rg = hfd::load_dec_regs4(tb);
  prefetch(nx);
  for (uint32_t brick = b0; brick < nbricks; brick += nw) {
    BPROF(pc[0]++; tp = __builtin_readcyclecounter();)
    const uint32_t bx = brick % nbx, t = brick / nbx, by = t % nby, bz = t / nby;
    const uint32_t y0 = by * 8, z0 = bz * 8;
    const bool live = y0 + ry < ly && z0 + rz < lz;
    const Next cur = nx;
    const uint32_t nbit = live ? cur.nbit : 0u;
    const uint32_t vbase = (live ? cur.entry : 0u) * 4u;
    const u32x4 f2[2] = {first[0], first[1]};
    const uint2 cp[2] = {pcell[0], pcell[1]};
    // the brick's outlier cells [cb, ce): per-row counts -> row starts; values into LDS
    auto pro = [&]() {
      if (ranked) dec3_stage_cells(bc, cval, ol, cur.cb, cur.ce, cp, lx, ly, lane);
    };
    auto recon = [&](int blk) {
      if (blk == (int)(W / BLK) - 1) prefetch(nx);  // the next brick (fetched during this block)
      const uint32_t nyv = min(8u, ly - y0), nzv = min(8u, lz - z0);
      const size_t base_elem = (size_t)z0 * plane + (size_t)y0 * lx + (size_t)bx * W + (size_t)blk * BLK;
      if constexpr (BLK == 64) {
        if (ranked)
          recon_block<T, ZZ, BUF, C::TP, true>(tile, out, plane, lx, nyv, nzv, base_elem, r, ebx2, lane, &bc);
        else
          recon_block<T, ZZ, BUF, C::TP, false>(tile, out, plane, lx, nyv, nzv, base_elem, r, ebx2, lane);
      }
      else {
        if (ranked)
          recon_block32<T, ZZ, BUF, C::TP, true>(tile, out, plane, lx, nyv, nzv, base_elem, r, ebx2, lane, &bc);
        else
          recon_block32<T, ZZ, BUF, C::TP, false>(tile, out, plane, lx, nyv, nzv, base_elem, r, ebx2, lane);
      }
    };
    auto blk_start = [&](int blk) {
      if (blk == (int)(W / BLK) - 1) nx = fetch(brick + nw);
    };
    decode_chunks4<BLK, C::TP>(tb, rg, dw, live, vbase, nbit, W, pro, blk_start, recon BPROF_A4, W, f2);
  }
#ifdef CUSZ_AMD_DEC_PROFILE
  if (lane == 0)
    for (int i = 0; i < 16; i++) atomicAdd(&g_brick_prof[i], pc[i]);
#endif
}

// ---- 3-D: region decode ---------------------------------------------------------------------
// k_brick3_decode over the bricks that cover a box of the field, writing only the box, compactly
// (x fastest), to `out`.  A brick is decoded whole -- its 64 rows are one wave's 64 chunks, the y
// sums and the z scan need the rows before the box -- but no brick outside the covering box
// bn = (bnx, bny, bnz) at brick lo = (blx, bly, blz) is fetched: work item i is brick
// (blx + i % bnx, bly + i / bnx % bny, blz + i / (bnx bny)); par_nbit, par_entry and ol.bstart keep
// the field's indexing.  64-column blocks only (a region is a few bricks per wave at most: one
// brick's latency bounds it).  x: the chunk is read front to back, so the blocks left of the box
// are decoded (and reconstructed without stores when the brick has outlier cells: the rows'
// consumed-cell counts carry on), the blocks right of it are not.  The cells are ranked (the host
// has read the bounds pass's verdict), non-ZigZag.  Work items are wave-major over the grid
// (wave w of workgroup g starts at w grid + g): one brick per CU before any CU gets a second.
template <typename T>
__global__ void __launch_bounds__(64 * Dec3Cfg<64>::kWaves)
k_brick3_region(const uint32_t* __restrict__ bitstream, uint32_t bs_words, const uint8_t* __restrict__ revbook,
                int bklen, const uint32_t* __restrict__ par_nbit, const uint32_t* __restrict__ par_entry, T* out,
                uint32_t lx, uint32_t ly, uint32_t lz, T ebx2, T r, uint32_t nbx, uint32_t nby, BrickOutliers ol,
                RegionBox box)
{
  __shared__ hfd::Tab4 tb;
  extern __shared__ __attribute__((aligned(16))) uint8_t dsm[];
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  typedef Dec3Cfg<64> C;
  constexpr int BLK = 64;
  uint8_t* wbase;
  uint16_t* tile;
  uint32_t* cval;
  BrickCells bc;
  dec3_lds<C>(dsm, wid, wbase, tile, cval, bc);
  const DecWave4 dw = dec3_wave(bitstream, bs_words, wbase, tile, bklen, lane);
  constexpr uint32_t W = 256;
  const uint32_t nw = gridDim.x * (blockDim.x >> 6);
  const uint32_t nitems = box.bnx * box.bny * box.bnz;
  const uint32_t ry = (uint32_t)lane >> 3, rz = (uint32_t)lane & 7u;
  const uint32_t xend = box.ox + box.ex;  // one past the box's last column
  BPROF(unsigned long long pc[16] = {}; unsigned long long tk = __builtin_readcyclecounter(), tp = tk;)

  struct Next {
    uint32_t nbit, entry, cb, ce;
    bool live;
  };
  auto fetch = [&](uint32_t i) {
    Next x{0, 0, 0, 0, false};
    if (i >= nitems) return x;
    const uint32_t bx = box.blx + i % box.bnx, t = i / box.bnx, by = box.bly + t % box.bny, bz = box.blz + t / box.bny;
    x.live = by * 8 + ry < ly && bz * 8 + rz < lz;
    if (x.live) {
      const size_t c = ((size_t)(bz * 8 + rz) * ly + (by * 8 + ry)) * nbx + bx;
      x.nbit = par_nbit[c], x.entry = par_entry[c];
    }
    if (ol.ncell) {
      const uint32_t b = (bz * nby + by) * nbx + bx;
      x.cb = ol.bstart[b], x.ce = ol.bstart[b + 1];
    }
    return x;
  };
  u32x4 first[2];
  uint2 pcell[2];
  auto prefetch = [&](const Next& x) { dec3_prefetch(dw, ol, x.live, x.entry, true, x.cb, x.ce, first, pcell); };
  const uint32_t i0 = (uint32_t)wid * gridDim.x + blockIdx.x;
  Next nx = fetch(i0);  // (lands while the tables are built)
  hfd::build_tab4(tb, revbook, bklen);
  const hfd::DecRegs4 rg = hfd::load_dec_regs4(tb);
  prefetch(nx);
  for (uint32_t item = i0; item < nitems; item += nw) {
    const uint32_t bx = box.blx + item % box.bnx, t = item / box.bnx, by = box.bly + t % box.bny, bz = box.blz + t / box.bny;
    const uint32_t x0 = bx * W, y0 = by * 8, z0 = bz * 8;
    const bool live = y0 + ry < ly && z0 + rz < lz;
    const Next cur = nx;
    const uint32_t nbit = live ? cur.nbit : 0u;
    const uint32_t vbase = (live ? cur.entry : 0u) * 4u;
    const u32x4 f2[2] = {first[0], first[1]};
    const uint2 cp[2] = {pcell[0], pcell[1]};
    // blocks of this brick that reach into the box's columns or lie left of them: 1..4
    const uint32_t nblk = xend - x0 >= W ? W / BLK : (xend - x0 + BLK - 1) / BLK;
    const uint32_t nc = cur.ce - cur.cb;
    // the brick's outlier cells [cb, ce): per-row counts -> row starts; values into LDS
    auto pro = [&]() { dec3_stage_cells(bc, cval, ol, cur.cb, cur.ce, cp, lx, ly, lane); };
    auto recon = [&](int blk) {
      if (blk == (int)nblk - 1) prefetch(nx);  // the next brick (fetched during this block)
      const uint32_t xb = x0 + (uint32_t)blk * BLK;
      // a block left of the box stores nothing; its zero codes still consume the rows' cells
      if (xb + BLK <= box.ox && nc == 0) return;
      // rows and planes up to the box's (and the field's) far faces: the sums never look ahead
      const uint32_t nyv = min(min(8u, ly - y0), box.oy + box.ey - y0), nzv = min(min(8u, lz - z0), box.oz + box.ez - z0);
      const RegionClip rc{xb, y0, z0, box.ox, box.oy, box.oz, box.ex, box.ey, box.ez};
      recon_block<T, false, false, C::TP, true, true>(tile, out, 0, 0, nyv, nzv, 0, r, ebx2, lane, &bc, &rc);
    };
    auto blk_start = [&](int blk) {
      if (blk == (int)nblk - 1) nx = fetch(item + nw);
    };
    decode_chunks4<BLK, C::TP>(tb, rg, dw, live, vbase, nbit, nblk * BLK, pro, blk_start, recon BPROF_A4, nblk * BLK, f2);
  }
}
// ---- 1-D: fused decode + reconstruct -------------------------------------------------------
// A wave owns a unit of 64 tiles of 1024 (4 chunks of 256 each); lane l owns tile 64 u + l and
// decodes its four chunks in four phases (phase p: chunk 4 t + p).  After each block of 64
// columns the lane reconstructs its own row -- 16 reference threads of 4 elements -- in
// registers, in the reference's 1-D order (lrz_x.cuhip.inl:11-78, wave32.cuhip.inl:7-66): per
// thread 4 sequential sums; Hillis-Steele over the 32 thread totals of each 128-element segment
// (a block is half a segment: the first half's raw totals stay in registers for the second
// half, which runs the 32-wide scan); a serial sum of the segment totals, carried per tile
// across the phases.  No cross-lane traffic; the lane stores its 256-B row piece.
//
// Outliers (archive cells in index order, k_x1d_bounds with chunk granularity): each lane
// prefetches the next kCellPf cell values of its chunk at a block's start (they land while the
// block decodes, and go to LDS for the reconstruction); zero codes take them by rank, ranks past
// the prefetch read the cell directly.
constexpr uint32_t kCellPf = 8;
constexpr uint32_t kCvPitch = kCellPf + 1;  // odd word pitch: lane rows on distinct banks
constexpr size_t kD1Cv = kD4Tile + (size_t)64 * kTP4 * 2;  // values[64][kCvPitch]
constexpr size_t kD1WaveBytes = kD1Cv + (size_t)64 * kCvPitch * 4;
constexpr int kD1MaxWaves = (int)((160 * 1024 - sizeof(hfd::Tab4) - 512) / kD1WaveBytes);
static_assert(kD1MaxWaves >= 4, "LDS");
static_assert(64 * 144 <= 64 * kTP4 * 2, "store staging fits the code tile");

//
// REGION (k_brick1_region): the same walk over the tiles [t0, t1) that cover the range [o, o + e)
// of the field only, unit u of the launch taking tiles t0 + 64 u + lane, and `out` the compact
// range.  Chunks wholly past the range are skipped; chunks of the first tile before it are decoded
// and summed (the tile's carry needs them) and store nothing.  Every element is stored by a guarded
// global store at its index in the range: no buffer resource or base reaching outside the range's
// allocation is formed.  Non-ZigZag, ranked cells only (the caller has read the bounds pass's
// verdict).  Waves [wpb, 8) of a workgroup only help build the tables; a wave takes one unit
// (launch_brick1_region), units wave-major so that they spread over the CUs first.
struct Region1 {
  uint32_t t0, t1;  // covering tiles of 1024
  size_t o, e;      // the range, in elements
  uint32_t wpb;     // decoding waves per workgroup
};

struct NoRegion1 {};

// k_brick1_decode<T, ZZ> (the field) and k_brick1_decode<T, false, true> = k_brick1_region (a range
// of it): one body, the region's differences under `if constexpr (REGION)`.
template <typename T, bool ZZ, bool REGION = false>
__global__ void __launch_bounds__(64 * kDecWaves)
k_brick1_decode(const uint32_t* __restrict__ bitstream, uint32_t bs_words, const uint8_t* __restrict__ revbook,
                int bklen, const uint32_t* __restrict__ par_nbit, const uint32_t* __restrict__ par_entry, T* out,
                size_t n, T ebx2, T r, uint32_t nchunks, uint32_t nunits, BrickOutliers ol,
                std::conditional_t<REGION, Region1, NoRegion1> rg1)
{
  __shared__ hfd::Tab4 tb;
  extern __shared__ __attribute__((aligned(16))) uint8_t dsm[];
  hfd::build_tab4(tb, revbook, bklen);
  const hfd::DecRegs4 rg = hfd::load_dec_regs4(tb);
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if constexpr (REGION)
    if ((uint32_t)wid >= rg1.wpb) return;
  uint8_t* wbase = dsm + (size_t)wid * kD1WaveBytes;
  uint16_t* tile = reinterpret_cast<uint16_t*>(wbase + kD4Tile);
  uint32_t* cv = reinterpret_cast<uint32_t*>(wbase + kD1Cv) + lane * kCvPitch;  // this lane's values
  // else: values in `out` (scatter); REGION: the caller has checked
  const bool ranked = !ZZ && (REGION || ol.ncell == 0 || *ol.unsorted != ol.epoch);
  const uint32_t npf = ol.ncell < (1u << 28) ? kCellPf : 0u;  // prefetched ranks (32-bit buffer offsets)
  const DecWave4 dw{__builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(bitstream), 0, (int)(bs_words * 4u), (int)kBufRsrcW3),
                    reinterpret_cast<uint32_t*>(wbase) + lane, tile, (uint32_t)bklen, lane};
  const __amdgpu_buffer_rsrc_t rcells = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint32_t*>(ol.cells), 0, (int)min(ol.ncell * 8, (size_t)0x7FFFFFFF), (int)kBufRsrcW3);
  uint32_t nw_, u0_;  // REGION: units wave-major, so that they spread over the workgroups first
  if constexpr (REGION) nw_ = gridDim.x * rg1.wpb, u0_ = (uint32_t)wid * gridDim.x + blockIdx.x;
  else nw_ = gridDim.x * (blockDim.x >> 6), u0_ = blockIdx.x * (blockDim.x >> 6) + wid;
  const uint32_t nw = nw_, u0 = u0_;
  // chunk p of this lane's tile in unit u, and whether it is decoded
  auto chunk_of = [&](uint32_t u, uint32_t p) {
    if constexpr (REGION) return ((size_t)rg1.t0 + (size_t)u * 64u + (uint32_t)lane) * 4u + p;
    else return ((size_t)u * 64u + (uint32_t)lane) * 4u + p;
  };
  auto wanted = [&](size_t c) {
    if constexpr (REGION) return c / 4u < rg1.t1 && c < nchunks && c * 256u < rg1.o + rg1.e;
    else return c < nchunks;
  };
  BPROF(unsigned long long pc[16] = {}; unsigned long long tk = __builtin_readcyclecounter(), tp = tk;)
  // chunk size / offset and cell range of each phase's chunk, loaded during the previous phase's
  // last block (they land while it decodes)
  struct Next {
    uint32_t nbit, entry, cb, ce;
  };
  auto fetch = [&](uint32_t u, uint32_t p) {
    Next x{0, 0, 0, 0};
    const size_t c = chunk_of(u, p);
    if (u < nunits && wanted(c)) {
      x.nbit = par_nbit[c], x.entry = par_entry[c];
      if (ranked && ol.ncell) x.cb = ol.bstart[c], x.ce = ol.bstart[c + 1];
    }
    return x;
  };
  Next nxt = fetch(u0, 0);
  for (uint32_t u = u0; u < nunits; u += nw) {
    T carry = T(0);  // serial sum of this tile's segment totals (exclusive)
    T fh[16];        // raw thread totals of the current segment's first half
    const size_t ubase = (size_t)u * 65536u;
    const bool full = ubase + 65536u <= n;  // every element of the unit is in the field (uniform)
    // unit-relative stores: 32-bit offsets; past the field's end they are dropped
    // (REGION: an empty resource, never used; the stores are element stores below)
    const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(
        out + (REGION ? 0 : ubase), 0, REGION ? 0 : (int)(min((size_t)65536u, n - ubase) * sizeof(T)), (int)kBufRsrcW3);
    for (uint32_t p = 0; p < 4; p++) {
      BPROF(pc[0]++; tp = __builtin_readcyclecounter();)
      const size_t c = chunk_of(u, p);
      const bool live = wanted(c);
      const Next me = nxt;
      const uint32_t nbit = live ? me.nbit : 0u;
      const uint32_t vbase = (live ? me.entry : 0u) * 4u;
      const uint32_t vlen = live ? (uint32_t)min((size_t)256, n - c * 256u) : 0u;
      uint32_t cur = 0, cend = 0;  // this chunk's cells [cur, cend), cur advancing
      u32x4 pf[kCellPf / 2];
      auto pro = [&]() {
        if (ranked && live && ol.ncell) cur = me.cb, cend = me.ce;
      };
      auto blk_start = [&](int blk) {
        if (blk == (int)(256 / kBlk) - 1) nxt = p < 3 ? fetch(u, p + 1) : fetch(u + nw, 0);
        if (!ranked) return;
        // only pairs that start inside the chunk's cells: a chunk's cells are re-read by every
        // block, and a phase's blocks lie too far apart for the lines to stay in L2
#pragma unroll
        for (int h = 0; h < (int)kCellPf / 2; h++)
          pf[h] = __builtin_amdgcn_raw_buffer_load_b128(
              rcells, (int)(live && npf && cur + 2u * h < cend ? cur * 8u + 16u * h : kOOB), 0, 0);
      };
      auto recon = [&](int blk) {
        const uint32_t roff = ((uint32_t)lane * 1024u + p * 256u + (uint32_t)blk * kBlk) * (uint32_t)sizeof(T);
        const uint32_t* trow = reinterpret_cast<const uint32_t*>(tile + lane * kTP4);
        if (ranked) {  // the prefetched values; ranks at or past the chunk's last cell read 0
#pragma unroll
          for (int h = 0; h < (int)kCellPf / 2; h++) {
            cv[2 * h] = cur + 2u * h < cend ? pf[h].x : 0u;
            cv[2 * h + 1] = cur + 2u * h + 1u < cend ? pf[h].z : 0u;
          }
        }
        T v[64];
        uint32_t tw[32];  // the row's 64 codes, all read before use (one LDS wait)
#pragma unroll
        for (int q = 0; q < 32; q++) tw[q] = trow[q];
        uint32_t rk = 0;  // zero codes so far in this block
        // values of the codes: (o + c) - r, where a zero code's o is its cell by rank and any other
        // code's o is 0 -- one of the two is zero, so the sum is the other exactly and the value is
        // (z ? o : c) - r.  The rank's value is read for every code and selected bitwise, so no
        // code branches.
        // The value reads are issued 16 at a time (ranks first, then the reads, then the selects):
        // under the decode's LDS traffic their latency is long, and a wait per code would serialise.
        auto values = [&](auto rtag) {
          constexpr bool RK = decltype(rtag)::value;
#pragma unroll
          for (int s = 0; s < 4; s++) {
            uint32_t val[16];
            if constexpr (RK && !ZZ) {
              uint32_t rr = rk;
#pragma unroll
              for (int e = 0; e < 16; e++) {
                const uint32_t cd = (e & 1) ? tw[8 * s + e / 2] >> 16 : tw[8 * s + e / 2] & 0xFFFFu;
                val[e] = cv[rr];  // ranks past the prefetch: fixed below (reads stay in LDS)
                rr += cd == 0u ? 1u : 0u;
              }
            }
#pragma unroll
            for (int e = 0; e < 16; e++) {
              const int q = 8 * s + e / 2, h = e & 1;
              const uint32_t cd = h ? tw[q] >> 16 : tw[q] & 0xFFFFu;
              T x;
              if constexpr (ZZ)
                x = (T)zz_dec((uint16_t)cd);
              else if constexpr (RK) {
                const uint32_t zm = 0u - (uint32_t)(cd == 0u);  // all ones for a zero code
                const float cf = (float)cd;                      // exact (codes < 2^16)
                const uint32_t b = (val[e] & zm) | (__builtin_bit_cast(uint32_t, cf) & ~zm);
                x = (T)__builtin_bit_cast(float, b) - r;
                rk -= zm;  // + 1 for a zero code
              }
              else
                x = (T)cd - r;
              v[2 * q + h] = x;
            }
          }
        };
        if (ranked)
          values(std::true_type{});
        else
          values(std::false_type{});
        if (ranked && __builtin_amdgcn_ballot_w64(rk > npf)) {  // ranks past the prefetch (rare)
          uint32_t j = 0;
#pragma unroll
          for (int q = 0; q < 32; q++) {
            const uint32_t w = tw[q];
#pragma unroll
            for (int h = 0; h < 2; h++) {
              const bool z = (h ? w >> 16 : w & 0xFFFFu) == 0u;
              if (z && j >= npf)
                v[2 * q + h] = (cur + j < cend ? (T)__builtin_bit_cast(float, ol.cells[2 * (size_t)(cur + j)]) : T(0)) - r;
              j += z ? 1u : 0u;
            }
          }
        }
        if (ranked) cur += rk;
        BPROF(const unsigned long long tv = __builtin_readcyclecounter(); pc[8] += tv - tk;)
        if (!ranked) {  // values scattered into `out`: plane + zz_dec(0), or (plane + 0) - r
#pragma unroll
          for (int q = 0; q < 32; q++) {
            const uint32_t w = tw[q];
#pragma unroll
            for (int h = 0; h < 2; h++) {
              if ((h ? w >> 16 : w & 0xFFFFu) == 0u) {
                const uint32_t off = roff + (uint32_t)(2 * q + h) * (uint32_t)sizeof(T);
                T o;
                if constexpr (sizeof(T) == 4)
                  o = __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b32(ro, (int)off, 0, 0));
                else
                  o = __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b64(ro, (int)off, 0, 0));
                v[2 * q + h] = ZZ ? o + v[2 * q + h] : o - r;
              }
            }
          }
        }
        // per thread: 4 sequential elements (wave32.cuhip.inl:10); then the thread totals'
        // Hillis-Steele over the segment's 32 (wave32.cuhip.inl:14-17), descending in place (each
        // stage reads the previous stage's values): a[t] holds thread t's inclusive total and
        // thread t adds a[t - 1]; then the segment carry and the scale.  f32: the same IEEE
        // operations two at a time where the operands pair up (v_pk_add_f32 / v_pk_mul_f32).
        T tot = T(0);
        auto scan = [&](auto otag) {
          constexpr bool ODD = decltype(otag)::value;
          constexpr int t0 = ODD ? 16 : 0, nt = t0 + 16;  // this block's threads: t0 .. t0 + 15
          T a[32];
          if constexpr (sizeof(T) == 4) {
            typedef float f2 __attribute__((ext_vector_type(2)));
#pragma unroll
            for (int k = 1; k < 4; k++)
#pragma unroll
              for (int t = 0; t < 16; t += 2) {
                f2 x = {v[4 * t + k], v[4 * t + 4 + k]};
                x = x + f2{v[4 * t + k - 1], v[4 * t + 3 + k]};
                v[4 * t + k] = x.x, v[4 * t + 4 + k] = x.y;
              }
#pragma unroll
            for (int t = 0; t < 16; t++) {
              if constexpr (ODD) a[t] = fh[t];
              a[t0 + t] = v[4 * t + 3];
              if constexpr (!ODD) fh[t] = v[4 * t + 3];
            }
#pragma unroll
            for (int d = 1; d < 32; d *= 2) {
              if (d >= nt) break;
#pragma unroll
              for (int t = nt - 1; t >= d; t -= 2) {
                if (t - 1 >= d) {  // pair (t, t - 1): both sources still hold the previous stage
                  f2 x = {a[t], a[t - 1]};
                  x = x + f2{a[t - d], a[t - 1 - d]};
                  a[t] = x.x, a[t - 1] = x.y;
                }
                else
                  a[t] = a[t] + a[t - d];
              }
            }
          }
          else {
#pragma unroll
            for (int t = 0; t < 16; t++) {
              v[4 * t + 1] = v[4 * t + 1] + v[4 * t];
              v[4 * t + 2] = v[4 * t + 2] + v[4 * t + 1];
              v[4 * t + 3] = v[4 * t + 3] + v[4 * t + 2];
            }
#pragma unroll
            for (int t = 0; t < 16; t++) {
              if constexpr (ODD) a[t] = fh[t];
              a[t0 + t] = v[4 * t + 3];
              if constexpr (!ODD) fh[t] = v[4 * t + 3];
            }
#pragma unroll
            for (int d = 1; d < 32; d *= 2)
#pragma unroll
              for (int t = nt - 1; t >= d; t--) a[t] = a[t] + a[t - d];
          }
#pragma unroll
          for (int t = 0; t < 16; t++) {
            T o[4];
            if (t0 + t > 0) {
#pragma unroll
              for (int k = 0; k < 4; k++) v[4 * t + k] = v[4 * t + k] + a[t0 + t - 1];
            }
            if constexpr (sizeof(T) == 4) {
              typedef float f2 __attribute__((ext_vector_type(2)));
#pragma unroll
              for (int k = 0; k < 4; k += 2) {
                f2 x = {v[4 * t + k], v[4 * t + k + 1]};
                x = (x + f2{carry, carry}) * f2{ebx2, ebx2};
                o[k] = x.x, o[k + 1] = x.y;
              }
            }
            else {
#pragma unroll
              for (int k = 0; k < 4; k++) o[k] = (v[4 * t + k] + carry) * ebx2;
            }
            if constexpr (REGION) {
              const size_t g0 = c * 256u + (uint32_t)blk * kBlk + 4u * (uint32_t)t;
#pragma unroll
              for (int k = 0; k < 4; k++) {
                const size_t g = g0 + (uint32_t)k;
                if (live && g >= rg1.o && g - rg1.o < rg1.e) out[g - rg1.o] = o[k];
              }
            }
            else if (full) {
              // through the tile's space (the codes are in registers): RE elements of every row
              // per round (128 B), then each store instruction writes whole 128-B pieces of
              // 64 / (RE / 4) rows instead of 16-B pieces of 64 rows
              T* st = reinterpret_cast<T*>(tile);
              constexpr uint32_t RE = 128 / sizeof(T), RT = RE / 4, LPR = RE / 4;  // elements, threads, lanes per row
              constexpr uint32_t SP = RE + 16 / sizeof(T);  // row pitch (elements): 144 B
              lds_store4<T>(st + lane * SP + 4u * (t % RT), o);
              if (t % RT == RT - 1) {
#pragma unroll
                for (int m = 0; m < (int)(64 / (64 / LPR)); m++) {
                  const uint32_t row = (64u / LPR) * m + (uint32_t)lane / LPR, sub = (uint32_t)lane % LPR;
                  T w[4];
                  lds_load4<T>(st + row * SP + 4u * sub, w);
                  buf_store4<T>(w, ro, (row * 1024u + p * 256u + (uint32_t)blk * kBlk + RE * (t / RT) + 4u * sub) *
                                           (uint32_t)sizeof(T));
                }
              }
            }
            else {
              const uint32_t off = roff + (uint32_t)(4 * t) * (uint32_t)sizeof(T);
#pragma unroll
              for (int k = 0; k < 4; k++) buf_store<T>(o[k], ro, off + (uint32_t)k * (uint32_t)sizeof(T), 0);
            }
          }
          if constexpr (ODD) tot = v[63];  // the segment's total
        };
        if (blk & 1)
          scan(std::true_type{});
        else
          scan(std::false_type{});
        if (blk & 1) carry = carry + tot;
        BPROF(pc[9] += __builtin_readcyclecounter() - tv;)
      };
      decode_chunks4(tb, rg, dw, live, vbase, nbit, vlen, pro, blk_start, recon BPROF_A4, 256, nullptr);
    }
  }
#ifdef CUSZ_AMD_DEC_PROFILE
  if (lane == 0)
    for (int i = 0; i < 16; i++) atomicAdd(&g_brick_prof[i], pc[i]);
#endif
}

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
  const DecWave4 dw{__builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(bitstream), 0, (int)(bs_words * 4u), (int)kBufRsrcW3),
                    reinterpret_cast<uint32_t*>(wbase) + lane, tile, (uint32_t)bklen, lane};
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
  if (lane == 0)
    for (int i = 0; i < 16; i++) atomicAdd(&g_brick_prof[i], pc[i]);
#endif
}

}  // namespace

int launch_brick_cell_bounds(const BrickLaunch& L, const uint32_t* cells, size_t ncell, uint32_t* bstart,
                             uint32_t* unsorted, uint32_t epoch, hipStream_t st)
{
  if (!ncell) return (int)hipSuccess;
  const uint32_t grid = (uint32_t)std::min<size_t>((ncell + 255) / 256, 2048);
  k_brick_cell_bounds<<<grid, 256, 0, st>>>(cells, ncell, L.lx, L.ly, L.lz, L.g.nbx, L.g.nby, L.g.nbricks, bstart,
                                            unsorted, epoch);
  return (int)hipGetLastError();
}

template <typename T>
int launch_brick_decode(const BrickLaunch& L, const PhfView& v, T* out, double eb, int radius, bool zz,
                        const BrickOutliers& ol, hipStream_t st)
{
  const T ebx2 = (T)(eb * 2);  // lrz_x.cuhip.inl:432
  const T r = (T)radius;
  const BrickGeom& g = L.g;
  if (v.bs_words >= (1ull << 30)) return (int)hipErrorInvalidValue;
  if (g.ndim == 1) {
    const uint32_t ntiles = (uint32_t)((g.n + 1023) / 1024), nunits = (ntiles + 63) / 64;
    // waves per CU: the static unit assignment ends when the busiest wave's units are done, and
    // the CU is throughput-bound, so minimise rounds x waves (ties: more waves)
    int wpb = 4;
    size_t best = ~(size_t)0;
    for (int w = 4; w <= kD1MaxWaves && w <= kDecWaves; w++) {
      const size_t rounds = (nunits + (size_t)L.ncu * w - 1) / ((size_t)L.ncu * w);
      if (rounds * w <= best) best = rounds * w, wpb = w;
    }
    const uint32_t grid = (uint32_t)std::max<size_t>(1, std::min<size_t>(L.ncu, (nunits + wpb - 1) / wpb));
    const size_t lds1 = (size_t)wpb * kD1WaveBytes;
    if (zz)
      k_brick1_decode<T, true><<<grid, 64 * wpb, lds1, st>>>(v.bitstream, (uint32_t)v.bs_words, v.revbook, v.bklen, v.par_nbit,
                                                             v.par_entry, out, g.n, ebx2, r, g.nchunks, nunits, ol, NoRegion1{});
    else
      k_brick1_decode<T, false><<<grid, 64 * wpb, lds1, st>>>(v.bitstream, (uint32_t)v.bs_words, v.revbook, v.bklen, v.par_nbit,
                                                              v.par_entry, out, g.n, ebx2, r, g.nchunks, nunits, ol, NoRegion1{});
    return (int)hipGetLastError();
  }
  // buffer stores address a brick block with 32-bit offsets from its first element
  const size_t plane = (size_t)L.lx * L.ly;
  const bool buf = (7 * plane + 7 * (size_t)L.lx + (size_t)kBlk) * sizeof(T) < (1ull << 31);
  const uint32_t bw = (uint32_t)v.bs_words;
  // 32-column blocks pay once the bricks fill the 12-wave slots (a 512^3 field); a small slab,
  // one brick per wave, is bound by one brick's latency, which the 64-column blocks keep shorter
  // (512 x 512 x 64: 88 against 94 us)
  const bool b32 = sizeof(T) == 4 && g.nbricks >= (uint32_t)Dec3Cfg<32>::kWaves * (uint32_t)L.ncu;
  auto launch = [&](auto blk) {
    constexpr int B3 = decltype(blk)::value;
    const size_t lds = (size_t)Dec3Cfg<B3>::kWaves * Dec3Cfg<B3>::kWaveBytes;  // dynamic part
#define DEC_LAUNCH(ZZ, BUF)                                                                                     \
    k_brick3_decode<T, ZZ, BUF, B3><<<L.ncu, 64 * Dec3Cfg<B3>::kWaves, lds, st>>>(v.bitstream, bw, v.revbook, v.bklen, v.par_nbit, \
                                                                              v.par_entry, out, L.lx, L.ly, L.lz, ebx2, r, \
                                                                              g.nbx, g.nby, g.nbricks, ol)
    if (zz) {
      if (buf) DEC_LAUNCH(true, true); else DEC_LAUNCH(true, false);
    }
    else {
      if (buf) DEC_LAUNCH(false, true); else DEC_LAUNCH(false, false);
    }
#undef DEC_LAUNCH
  };
  if constexpr (sizeof(T) == 4) {
    if (b32) launch(std::integral_constant<int, 32>{});
    else launch(std::integral_constant<int, 64>{});
  }
  else
    launch(std::integral_constant<int, 64>{});
  return (int)hipGetLastError();
}

RegionBox region_box(uint32_t ox, uint32_t oy, uint32_t oz, uint32_t ex, uint32_t ey, uint32_t ez, uint32_t W)
{
  RegionBox b{ox, oy, oz, ex, ey, ez, ox / W, oy / 8, oz / 8, 0, 0, 0};
  b.bnx = (ox + ex - 1) / W - b.blx + 1;
  b.bny = (oy + ey - 1) / 8 - b.bly + 1;
  b.bnz = (oz + ez - 1) / 8 - b.blz + 1;
  return b;
}

template <typename T>
int launch_brick_region(const BrickLaunch& L, const PhfView& v, T* out_box, double eb, int radius,
                        const BrickOutliers& ol, const uint32_t (&o)[3], const uint32_t (&e)[3], hipStream_t st)
{
  const BrickGeom& g = L.g;
  // the box lies inside the field, so its covering bricks lie inside the brick grid
  if (!g.ok || g.ndim != 3 || g.W != 256 || v.bs_words >= (1ull << 30) || v.bklen < 1 || v.bklen > kMaxBklen || !e[0] ||
      !e[1] || !e[2] || o[0] >= L.lx || e[0] > L.lx - o[0] || o[1] >= L.ly || e[1] > L.ly - o[1] || o[2] >= L.lz ||
      e[2] > L.lz - o[2])
    return (int)hipErrorInvalidValue;
  const RegionBox box = region_box(o[0], o[1], o[2], e[0], e[1], e[2], (uint32_t)g.W);
  const T ebx2 = (T)(eb * 2);  // lrz_x.cuhip.inl:432
  const T r = (T)radius;
  typedef Dec3Cfg<64> C;
  const uint32_t items = box.bnx * box.bny * box.bnz;
  // one brick per CU while they last (wave 0 of each workgroup), then one per SIMD, ...: a
  // region is bound by one brick's serial walk, not by throughput
  const uint32_t grid = std::max(1u, std::min((uint32_t)L.ncu, items));
  const size_t lds = (size_t)C::kWaves * C::kWaveBytes;  // dynamic part
  k_brick3_region<T><<<grid, 64 * C::kWaves, lds, st>>>(v.bitstream, (uint32_t)v.bs_words, v.revbook, v.bklen, v.par_nbit,
                                                        v.par_entry, out_box, L.lx, L.ly, L.lz, ebx2, r, g.nbx, g.nby,
                                                        ol, box);
  return (int)hipGetLastError();
}

template <typename T>
int launch_brick1_region(const BrickLaunch& L, const PhfView& v, T* out_box, double eb, int radius,
                         const BrickOutliers& ol, size_t o, size_t e, hipStream_t st)
{
  const BrickGeom& g = L.g;
  if (!g.ok || g.ndim != 1 || g.W != 256 || v.bs_words >= (1ull << 30) || v.bklen < 1 || v.bklen > kMaxBklen || !e ||
      o >= g.n || e > g.n - o || (uint32_t)v.pardeg != g.nchunks || L.ncu < 1)
    return (int)hipErrorInvalidValue;
  const Region1Tiles t = region_tiles1(o, e);
  const uint32_t nunits = (uint32_t)((t.t1 - t.t0 + 63) / 64);
  // one unit per wave; one wave per workgroup while the units fit the CUs (a small range is bound
  // by one tile's serial walk), then more decoding waves per workgroup
  const uint32_t wmax = (uint32_t)std::min<int>(kDecWaves, kD1MaxWaves);
  const uint32_t wpb = std::max(1u, std::min(wmax, (nunits + (uint32_t)L.ncu - 1) / (uint32_t)L.ncu));
  const uint32_t grid = (nunits + wpb - 1) / wpb;
  const Region1 rg1{(uint32_t)t.t0, (uint32_t)t.t1, o, e, wpb};
  k_brick1_decode<T, false, true><<<grid, 64 * kDecWaves, (size_t)wpb * kD1WaveBytes, st>>>(
      v.bitstream, (uint32_t)v.bs_words, v.revbook, v.bklen, v.par_nbit, v.par_entry, out_box, g.n, (T)(eb * 2), (T)radius,
      g.nchunks, nunits, ol, rg1);
  return (int)hipGetLastError();
}

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

#ifdef CUSZ_AMD_DEC_PROFILE
extern "C" int psz_amd_debug_brick_profile(unsigned long long* host, int reset)
{
  hipError_t e = hipMemcpyFromSymbol(host, HIP_SYMBOL(g_brick_prof), sizeof(unsigned long long) * 16);
  if (reset) {
    unsigned long long z[16] = {};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_brick_prof), z, sizeof(z));
  }
  if (e == hipSuccess) return brick_stream_profile(host, reset);  // + the single-pass encoder's
  return (int)e;
}
#endif

#define INST(T)                                                                                                   \
  template int launch_brick_decode<T>(const BrickLaunch&, const PhfView&, T*, double, int, bool, const BrickOutliers&, \
                                      hipStream_t);                                                                \
  template int launch_brick_region<T>(const BrickLaunch&, const PhfView&, T*, double, int, const BrickOutliers&,   \
                                      const uint32_t(&)[3], const uint32_t(&)[3], hipStream_t);             \
  template int launch_brick1_region<T>(const BrickLaunch&, const PhfView&, T*, double, int, const BrickOutliers&, size_t, \
                                       size_t, hipStream_t);
INST(float)
INST(double)
#undef INST

}  // namespace cusz_amd
