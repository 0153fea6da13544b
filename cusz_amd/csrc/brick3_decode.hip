// cusz_amd/csrc/brick3_decode.hip -- the fused 3-D decoder (overview: brick_device.hh; the chunk
// loop: brick_decode.hh): the block reconstruction, k_brick_cell_bounds, and k_brick3_decode for the
// whole field and, as its REGION instantiation (k_brick3_region), for a box of it; the launchers.
#include "brick_decode.hh"

namespace cusz_amd {

BPROF_UNIT(brick3_profile)

namespace {

// Outliers.  When the archive's cells are grouped by brick and sorted by (row, x) -- this
// compressor writes them so, k_brick_cell_bounds checks -- the k-th zero code of a row takes the
// row's k-th cell (values staged in LDS per brick), and no scatter pass runs; otherwise the
// scatter pass has written the values into `out`, where the reconstruction reads them.
constexpr uint32_t kCellCap = 128;  // outlier values of a brick kept in LDS

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
// FULL (the caller's wave-uniform nyv == 8 && nzv == 8, every brick of a field whose y and z
// extents are multiples of 8): no row or plane test anywhere, the four row descriptors and the
// plane offsets formed once, and the sums, scans and 32 stores of the block in one straight
// line -- the same IEEE operations in the same order, two z rows per packed instruction where
// the operands pair up (as recon_block: the y sums, the z steps d = 2, 4, the scale).
template <typename T, bool ZZ, bool BUF, int TP, bool CELLS, bool FULL>
__device__ __forceinline__ void recon_block32(const uint16_t* tile, T* out, size_t plane, uint32_t lx, uint32_t nyv,
                                              uint32_t nzv, size_t base_elem, T r, T ebx2, int lane,
                                              const BrickCells* bc = nullptr)
{
  T* base = out + base_elem;  // element (x0, y0, z0) of this block
  const uint32_t hl = (uint32_t)lane >> 5, l32 = (uint32_t)lane & 31u;
  const uint32_t col = rcol(l32);
  const uint32_t ybase = 4u * hl;
  if constexpr (FULL) nzv = 8u;
  T v[4][8];
#pragma unroll
  for (int yy = 0; yy < 4; yy++) {
    const uint32_t y = ybase + (uint32_t)yy;
    const bool yok = FULL || y < nyv;
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
  if constexpr (FULL && sizeof(T) == 4) {
    typedef float f2 __attribute__((ext_vector_type(2)));
    // y running sums: the lower half's s_3 (computed by every lane, used by the upper half)
    f2 c[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      f2 u = {v[0][2 * j], v[0][2 * j + 1]};
#pragma unroll
      for (int yy = 1; yy < 4; yy++) u = u + f2{v[yy][2 * j], v[yy][2 * j + 1]};
      c[j] = f2{from_lower_half<T>(u.x), from_lower_half<T>(u.y)};
    }
    const uint32_t voff = (col + hl * 4u * lx) * (uint32_t)sizeof(T);
    f2 scale = {(float)ebx2, (float)ebx2};
    asm("" : "+s"(scale));  // one scalar pair for every v_pk_mul_f32, not one per use
    __amdgpu_buffer_rsrc_t ro[4];
    uint32_t soff[8];
    if constexpr (BUF) {
#pragma unroll
      for (int yy = 0; yy < 4; yy++) ro[yy] = rsrc(base + (size_t)yy * lx);
#pragma unroll
      for (int z = 0; z < 8; z++) soff[z] = (uint32_t)((size_t)z * plane * sizeof(T));
    }
#pragma unroll
    for (int yy = 0; yy < 4; yy++) {
      T t[8];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        c[j] = c[j] + f2{v[yy][2 * j], v[yy][2 * j + 1]};
        t[2 * j] = c[j].x, t[2 * j + 1] = c[j].y;
      }
      // x Hillis-Steele, step by step over the eight independent z rows (x_scan8i's steps)
#pragma unroll
      for (int z = 0; z < 8; z++) t[z] = t[z] + dpp0<0x112>(t[z]), no_slp(t[z]);  // column x - 1
#pragma unroll
      for (int z = 0; z < 8; z++) t[z] = t[z] + dpp0<0x114>(t[z]), no_slp(t[z]);  // column x - 2
#pragma unroll
      for (int z = 0; z < 8; z++) t[z] = t[z] + dpp0<0x118>(t[z]), no_slp(t[z]);  // column x - 4
#pragma unroll
      for (int z = 7; z >= 1; z--) t[z] = t[z] + t[z - 1];
      f2 tp[4];
#pragma unroll
      for (int j = 0; j < 4; j++) tp[j] = f2{t[2 * j], t[2 * j + 1]};
      tp[3] = tp[3] + tp[2], tp[2] = tp[2] + tp[1], tp[1] = tp[1] + tp[0];  // d = 2 (descending)
      tp[3] = tp[3] + tp[1], tp[2] = tp[2] + tp[0];                          // d = 4
#pragma unroll
      for (int j = 0; j < 4; j++) tp[j] = tp[j] * scale;
#pragma unroll
      for (int j = 0; j < 4; j++) t[2 * j] = tp[j].x, t[2 * j + 1] = tp[j].y;
      if constexpr (BUF) {
#pragma unroll
        for (int z = 0; z < 8; z++) buf_store<T>(t[z], ro[yy], voff, soff[z]);
      }
      else {
        // wave-uniform row address plus the lane's 32-bit byte offset (no 64-bit lane addresses)
#pragma unroll
        for (int z = 0; z < 8; z++)
          *reinterpret_cast<T*>(reinterpret_cast<char*>(base + (size_t)z * plane + (size_t)yy * lx) + (size_t)voff) = t[z];
      }
    }
    return;
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

// Per block width: 64 columns (8 waves per CU, a 15 KB ring + tile per wave) or 32 columns (12
// waves per CU in 11 KB each: 3 waves per SIMD on the same LDS, recon_block32).  The step's chain
// of two LDS round trips bounds the loop, so a third wave per SIMD pays although a 512^3 field's
// 8192 bricks then make 2.67 rounds: f32 decompress 255 -> 229 us (config 2).  f64 keeps 64
// columns (at 32 its reconstruction spills 29-37 VGPRs).
// launch_brick_decode takes 32 for f32 fields of >= 12 bricks per CU, else 64.
// 64 columns, 8 waves per CU: a 512^3 field's 8192 bricks are 4 full rounds of the 2048 waves (9
// waves left a partial fourth round: decode 285 -> 259 us)
template <int BLK>
struct Dec3Cfg {
  static constexpr int TP = BLK + 10;  // 9 overshoot columns, odd dword pitch
  static constexpr size_t kCells = kD4Tile + (size_t)64 * TP * 2;
  static constexpr size_t kRows = kCells + (size_t)kCellCap * 4;
  static constexpr size_t kWaveBytes = kRows + (size_t)(65 + 64) * 4;
  static constexpr int kWaves = BLK == 64 ? 8 : 12;
  static_assert(((TP / 2) & 1) == 1 && BLK + 2 * kF + 1 <= TP, "tile pitch");
  static_assert(sizeof(hfd::Tab4) + kWaves * kWaveBytes <= 160 * 1024, "LDS");
};

// One wave per brick: the field's bricks or, REGION (k_brick3_region = <T, false, false, 64, true>),
// the bricks that cover a box of the field, writing only the box, compactly (x fastest), to `out`.
// One body, the region's differences under `if constexpr (REGION)`:
//  * A brick is decoded whole -- its 64 rows are one wave's 64 chunks, the y sums and the z scan
//    need the rows before the box -- but no brick outside the covering box bn = (bnx, bny, bnz) at
//    brick lo = (blx, bly, blz) is fetched: work item i is brick (blx + i % bnx, bly + i / bnx % bny,
//    blz + i / (bnx bny)); par_nbit, par_entry and ol.bstart keep the field's indexing.
//  * x: the chunk is read front to back, so the blocks left of the box are decoded (and
//    reconstructed without stores when the brick has outlier cells: the rows' consumed-cell counts
//    carry on), the blocks right of it are not.
//  * The cells are ranked (the host has read the bounds pass's verdict), non-ZigZag; 64-column
//    blocks only (a region is a few bricks per wave at most: one brick's latency bounds it).
//  * Work items are always wave-major over the grid (wave w of workgroup g starts at w grid + g):
//    one brick per CU before any CU gets a second.
template <typename T, bool ZZ, bool BUF, int BLK, bool REGION = false>
__global__ void __launch_bounds__(64 * Dec3Cfg<BLK>::kWaves)
k_brick3_decode(const uint32_t* __restrict__ bitstream, uint32_t bs_words, const uint8_t* __restrict__ revbook,
                int bklen, const uint32_t* __restrict__ par_nbit, const uint32_t* __restrict__ par_entry, T* out,
                uint32_t lx, uint32_t ly, uint32_t lz, T ebx2, T r, uint32_t nbx, uint32_t nby, uint32_t nbricks,
                BrickOutliers ol, std::conditional_t<REGION, RegionBox, Empty> box)
{
  static_assert(!REGION || (!ZZ && !BUF && BLK == 64), "the region decoder: ranked cells, 64-column blocks");
  __shared__ hfd::Tab4 tb;  // static: table addresses fold into the ds offsets
  extern __shared__ __attribute__((aligned(16))) uint8_t dsm[];
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  typedef Dec3Cfg<BLK> C;
  // this wave's part of the dynamic LDS: ring | tile | cell values | row starts (65) | row carries (64)
  uint8_t* wbase = dsm + (size_t)wid * C::kWaveBytes;
  uint16_t* tile = reinterpret_cast<uint16_t*>(wbase + kD4Tile);
  uint32_t* cval = reinterpret_cast<uint32_t*>(wbase + C::kCells);
  BrickCells bc{cval, 1, reinterpret_cast<uint32_t*>(wbase + C::kRows), reinterpret_cast<uint32_t*>(wbase + C::kRows) + 65};
  const bool ranked = REGION || (!ZZ && (ol.ncell == 0 || *ol.unsorted != ol.epoch));
  const DecWave4 dw = dec_wave4(bitstream, bs_words, wbase, tile, bklen, lane);
  const size_t plane = (size_t)lx * ly;
  constexpr uint32_t W = 256;
  const uint32_t nw = gridDim.x * (blockDim.x >> 6);
  const uint32_t ry = (uint32_t)lane >> 3, rz = (uint32_t)lane & 7u;
  // work items: the field's bricks, or the box's covering bricks
  struct Brick {
    uint32_t bx, by, bz;
  };
  auto brick_of = [&](uint32_t i) {
    if constexpr (REGION) {
      const uint32_t t = i / box.bnx;
      return Brick{box.blx + i % box.bnx, box.bly + t % box.bny, box.blz + t / box.bny};
    }
    else {
      const uint32_t t = i / nbx;
      return Brick{i % nbx, t % nby, t / nby};
    }
  };
  const uint32_t nitems = [&] {
    if constexpr (REGION) return box.bnx * box.bny * box.bnz;
    else return nbricks;
  }();

  BPROF(unsigned long long pc[16] = {}; unsigned long long tk = __builtin_readcyclecounter(), tp = tk;)
  // A brick's chunk sizes / offsets and cell range are loaded during the previous brick's last
  // block (they land while it decodes), so a brick starts with the bitstream loads only.
  // Its first bitstream words and first two outlier cells per lane are loaded at the start of
  // the previous brick's last reconstruction (they land under its stores).
  struct Next {
    uint32_t nbit, entry, cb, ce;
    bool live;
  };
  auto fetch = [&](uint32_t i) {
    Next x{0, 0, 0, 0, false};
    if (i >= nitems) return x;
    const Brick k = brick_of(i);
    x.live = k.by * 8 + ry < ly && k.bz * 8 + rz < lz;
    if (x.live) {
      const size_t c = ((size_t)(k.bz * 8 + rz) * ly + (k.by * 8 + ry)) * nbx + k.bx;
      x.nbit = par_nbit[c], x.entry = par_entry[c];
    }
    if (ranked && ol.ncell) {
      const uint32_t b = REGION ? (k.bz * nby + k.by) * nbx + k.bx : i;  // the brick's index in the field
      x.cb = ol.bstart[b], x.ce = ol.bstart[b + 1];
    }
    return x;
  };
  u32x4 first[2];
  uint2 pcell[2];  // cells cb + lane and cb + 64 + lane of the next brick: {value, index}
  auto prefetch = [&](const Next& x) {
    first[0] = __builtin_amdgcn_raw_buffer_load_b128(dw.rbits, (int)(x.live ? x.entry * 4u : kOOB), 0, 0);
    first[1] = __builtin_amdgcn_raw_buffer_load_b128(dw.rbits, (int)(x.live ? x.entry * 4u + 16u : kOOB), 0, 0);
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const uint32_t j = x.cb + (uint32_t)lane + 64u * k;
      pcell[k] = ranked && j < x.ce ? make_uint2(ol.cells[2 * (size_t)j], ol.cells[2 * (size_t)j + 1]) : make_uint2(0, 0);
    }
  };
  // a wave's first brick: 8 consecutive bricks per workgroup (they share par_nbit / par_entry /
  // bitstream lines in one L2), unless the field has fewer bricks than waves (a small slab): then
  // wave w of every workgroup takes brick w * grid + block, spreading them over every CU (one per
  // SIMD for 1024 bricks) instead of filling half the CUs two waves per SIMD
  // (32-column blocks: always wave-major, so that the bricks' last, partial round is spread over
  // every CU instead of ending on the first 170)
  const uint32_t b0 = REGION || BLK == 32 || nitems <= nw ? (uint32_t)wid * gridDim.x + blockIdx.x : blockIdx.x * (blockDim.x >> 6) + wid;
  Next nx = fetch(b0);  // (lands while the tables are built)
  hfd::build_tab4(tb, revbook, bklen);
  const hfd::DecRegs4 rg = hfd::load_dec_regs4(tb);
  prefetch(nx);
  for (uint32_t item = b0; item < nitems; item += nw) {
    BPROF(pc[0]++; tp = __builtin_readcyclecounter();)
    const Brick k = brick_of(item);
    const uint32_t bx = k.bx, y0 = k.by * 8, z0 = k.bz * 8;
    const bool live = y0 + ry < ly && z0 + rz < lz;
    const Next cur = nx;
    const uint32_t nbit = live ? cur.nbit : 0u;
    const uint32_t vbase = (live ? cur.entry : 0u) * 4u;
    const u32x4 f2[2] = {first[0], first[1]};
    const uint2 cp[2] = {pcell[0], pcell[1]};
    const uint32_t nc = cur.ce - cur.cb;
    // blocks of this brick: all, or those that reach into the box's columns or lie left of them (1..4)
    const uint32_t nblk = [&] {
      if constexpr (REGION) {
        const uint32_t xr = box.ox + box.ex - bx * W;  // columns from the brick's first to the box's last
        return xr >= W ? W / BLK : (xr + BLK - 1) / BLK;
      }
      else
        return W / BLK;
    }();
    // the brick's outlier cells [cb, ce), the first 128 of them prefetched in cp: per-row counts ->
    // row starts; values into LDS when they fit
    auto pro = [&]() {
      if (!ranked) return;
      bc.row_start[lane] = 0;
      hfd::wave_sync();
      for (uint32_t j = (uint32_t)lane; j < nc; j += 64) {
        const uint2 cell = j < 64u    ? cp[0]
                           : j < 128u ? cp[1]
                                      : make_uint2(ol.cells[2 * (size_t)(cur.cb + j)], ol.cells[2 * (size_t)(cur.cb + j) + 1]);
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
      bc.val = nc <= kCellCap ? cval : ol.cells + 2 * (size_t)cur.cb;
      bc.vstride = nc <= kCellCap ? 1u : 2u;
    };
    auto recon = [&](int blk) {
      if (blk == (int)nblk - 1) prefetch(nx);  // the next brick (fetched during this block)
      if constexpr (REGION) {
        const uint32_t xb = bx * W + (uint32_t)blk * BLK;
        // a block left of the box stores nothing; its zero codes still consume the rows' cells
        if (xb + BLK <= box.ox && nc == 0) return;
        // rows and planes up to the box's (and the field's) far faces: the sums never look ahead
        const uint32_t nyv = min(min(8u, ly - y0), box.oy + box.ey - y0), nzv = min(min(8u, lz - z0), box.oz + box.ez - z0);
        const RegionClip rc{xb, y0, z0, box.ox, box.oy, box.oz, box.ex, box.ey, box.ez};
        recon_block<T, false, false, C::TP, true, true>(tile, out, 0, 0, nyv, nzv, 0, r, ebx2, lane, &bc, &rc);
      }
      else {
        const uint32_t nyv = min(8u, ly - y0), nzv = min(8u, lz - z0);
        const size_t base_elem = (size_t)z0 * plane + (size_t)y0 * lx + (size_t)bx * W + (size_t)blk * BLK;
        if constexpr (BLK == 64) {
          if (ranked)
            recon_block<T, ZZ, BUF, C::TP, true>(tile, out, plane, lx, nyv, nzv, base_elem, r, ebx2, lane, &bc);
          else
            recon_block<T, ZZ, BUF, C::TP, false>(tile, out, plane, lx, nyv, nzv, base_elem, r, ebx2, lane);
        }
        else {
          // full bricks (every one of a field with y and z extents in multiples of 8) take the
          // straight-line body: one wave-uniform choice per block
          auto go = [&](auto cells, auto full) {
            recon_block32<T, ZZ, BUF, C::TP, decltype(cells)::value, decltype(full)::value>(tile, out, plane, lx, nyv, nzv, base_elem, r,
                                                                                          ebx2, lane, &bc);
          };
          const bool full = nyv == 8u && nzv == 8u;
          if (ranked) {
            if (full) go(std::true_type{}, std::true_type{});
            else go(std::true_type{}, std::false_type{});
          }
          else {
            if (full) go(std::false_type{}, std::true_type{});
            else go(std::false_type{}, std::false_type{});
          }
        }
      }
    };
    auto blk_start = [&](int blk) {
      if (blk == (int)nblk - 1) nx = fetch(item + nw);
    };
    decode_chunks4<BLK, C::TP>(tb, rg, dw, live, vbase, nbit, nblk * BLK, pro, blk_start, recon BPROF_A4, nblk * BLK, f2);
  }
  BPROF(prof_add(pc, lane);)
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
  const BrickGeom& g = L.g;
  if (v.bs_words >= (1ull << 30)) return (int)hipErrorInvalidValue;
  if (g.ndim == 1) return launch_brick1_decode<T>(L, v, out, eb, radius, zz, ol, st);
  const T ebx2 = (T)(eb * 2);  // lrz_x.cuhip.inl:432
  const T r = (T)radius;
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
                                                                              g.nbx, g.nby, g.nbricks, ol, Empty{})
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
  if (!region_launch_ok(L, v, 3) || !e[0] || !e[1] || !e[2] || o[0] >= L.lx || e[0] > L.lx - o[0] || o[1] >= L.ly ||
      e[1] > L.ly - o[1] || o[2] >= L.lz || e[2] > L.lz - o[2])
    return (int)hipErrorInvalidValue;
  const RegionBox box = region_box(o[0], o[1], o[2], e[0], e[1], e[2], (uint32_t)g.W);
  typedef Dec3Cfg<64> C;
  const uint32_t items = box.bnx * box.bny * box.bnz;
  // one brick per CU while they last (wave 0 of each workgroup), then one per SIMD, ...: a
  // region is bound by one brick's serial walk, not by throughput
  const uint32_t grid = std::max(1u, std::min((uint32_t)L.ncu, items));
  const size_t lds = (size_t)C::kWaves * C::kWaveBytes;  // dynamic part
  k_brick3_decode<T, false, false, 64, true><<<grid, 64 * C::kWaves, lds, st>>>(
      v.bitstream, (uint32_t)v.bs_words, v.revbook, v.bklen, v.par_nbit, v.par_entry, out_box, L.lx, L.ly, L.lz,
      (T)(eb * 2) /* lrz_x.cuhip.inl:432 */, (T)radius, g.nbx, g.nby, g.nbricks, ol, box);
  return (int)hipGetLastError();
}

#ifdef CUSZ_AMD_DEC_PROFILE
extern "C" int psz_amd_debug_brick_profile(unsigned long long* host, int reset)
{
  std::fill(host, host + 16, 0ull);
  for (auto unit : {brick3_profile, brick1_profile, chunk_profile, brick_stream_profile})
    if (const int e = unit(host, reset)) return e;
  return 0;
}
#endif

#define INST(T)                                                                                                   \
  template int launch_brick_decode<T>(const BrickLaunch&, const PhfView&, T*, double, int, bool, const BrickOutliers&, \
                                      hipStream_t);                                                                \
  template int launch_brick_region<T>(const BrickLaunch&, const PhfView&, T*, double, int, const BrickOutliers&,   \
                                      const uint32_t(&)[3], const uint32_t(&)[3], hipStream_t);
INST(float)
INST(double)
#undef INST

}  // namespace cusz_amd
