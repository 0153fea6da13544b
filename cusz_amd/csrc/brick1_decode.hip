// cusz_amd/csrc/brick1_decode.hip -- the fused 1-D decoder (overview: brick_device.hh; the chunk
// loop: brick_decode.hh): k_brick1_decode for the whole field and, as its REGION instantiation
// (k_brick1_region), for a range of it; their launchers.
#include "brick_decode.hh"

namespace cusz_amd {

BPROF_UNIT(brick1_profile)

namespace {

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
constexpr size_t kD1Cv = kD4Cells;          // values[64][kCvPitch], behind ring + tile
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

// k_brick1_decode<T, ZZ> (the field) and k_brick1_decode<T, false, true> = k_brick1_region (a range
// of it): one body, the region's differences under `if constexpr (REGION)`.
template <typename T, bool ZZ, bool REGION = false>
__global__ void __launch_bounds__(64 * kDecWaves)
k_brick1_decode(const uint32_t* __restrict__ bitstream, uint32_t bs_words, const uint8_t* __restrict__ revbook,
                int bklen, const uint32_t* __restrict__ par_nbit, const uint32_t* __restrict__ par_entry, T* out,
                size_t n, T ebx2, T r, uint32_t nchunks, uint32_t nunits, BrickOutliers ol,
                std::conditional_t<REGION, Region1, Empty> rg1)
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
  const DecWave4 dw = dec_wave4(bitstream, bs_words, wbase, tile, bklen, lane);
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
  BPROF(prof_add(pc, lane);)
}

}  // namespace

// the 1-D half of launch_brick_decode (brick3_decode.hip), which has checked the bitstream's size
template <typename T>
int launch_brick1_decode(const BrickLaunch& L, const PhfView& v, T* out, double eb, int radius, bool zz,
                         const BrickOutliers& ol, hipStream_t st)
{
  const T ebx2 = (T)(eb * 2);  // lrz_x.cuhip.inl:432
  const T r = (T)radius;
  const BrickGeom& g = L.g;
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
                                                           v.par_entry, out, g.n, ebx2, r, g.nchunks, nunits, ol, Empty{});
  else
    k_brick1_decode<T, false><<<grid, 64 * wpb, lds1, st>>>(v.bitstream, (uint32_t)v.bs_words, v.revbook, v.bklen, v.par_nbit,
                                                            v.par_entry, out, g.n, ebx2, r, g.nchunks, nunits, ol, Empty{});
  return (int)hipGetLastError();
}

template <typename T>
int launch_brick1_region(const BrickLaunch& L, const PhfView& v, T* out_box, double eb, int radius,
                         const BrickOutliers& ol, size_t o, size_t e, hipStream_t st)
{
  const BrickGeom& g = L.g;
  if (!region_launch_ok(L, v, 1) || !e || o >= g.n || e > g.n - o || (uint32_t)v.pardeg != g.nchunks || L.ncu < 1)
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

#define INST(T)                                                                                                         \
  template int launch_brick1_decode<T>(const BrickLaunch&, const PhfView&, T*, double, int, bool, const BrickOutliers&, \
                                       hipStream_t);                                                                    \
  template int launch_brick1_region<T>(const BrickLaunch&, const PhfView&, T*, double, int, const BrickOutliers&, size_t, \
                                       size_t, hipStream_t);
INST(float)
INST(double)
#undef INST

}  // namespace cusz_amd
