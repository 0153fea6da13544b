// cusz_amd/csrc/brick_pack.hip -- plan and pass 2 of the fused brick compressor (overview:
// brick_device.hh): k_brick_plan sizes every brick's bitstream region from its histogram and writes
// the headers; k_brick3_pack packs the codes pass 1 left into chunks at those regions.
#include "brick_device.hh"

namespace cusz_amd {

namespace {

// =========================================================================================
// plan: per-brick region sizes and outlier offsets, archive totals and headers
// =========================================================================================
// One launch after the codebook upload plans the whole archive:
//  * per brick: region upper bound ub = (sum_s hist_b[s] len[s] + 31 rows) / 32 cells and its
//    outlier count; block-local exclusive prefixes of both (kPlanBricks bricks per block);
//  * block totals by agent-scope atomics; the block that finishes last scans them (every brick's
//    base = local prefix + block prefix), fills the size fields and writes both headers.
// Replaces the reference's host-side scans (hf_kernels.cuhip.inl:449-473, compressor.inl:398-418).
constexpr int kPlanBricks = 64;  // bricks per plan block: 4 per wave (one per wave, 512 blocks: 15 -> 20 us)
constexpr int kPlanThreads = 1024;
constexpr int kPlanWaves = kPlanThreads / 64;
static_assert(kPlanBricks % kPlanWaves == 0 && kPlanBricks <= 64, "wave 0 scans the block's bricks");

__device__ __forceinline__ uint32_t brick_rows3(uint32_t brick, uint32_t nbx, uint32_t nby, uint32_t ly, uint32_t lz)
{
  const uint32_t t = brick / nbx, by = t % nby, bz = t / nby;
  return min(8u, ly - by * 8) * min(8u, lz - bz * 8);
}

__global__ void __launch_bounds__(kPlanThreads) k_brick_plan(BrickPlanArgs a, HeaderTpl tpl)
{
  __shared__ uint32_t s_len[kMaxBklen];
  __shared__ uint32_t s_ub[kPlanBricks], s_oc[kPlanBricks];
  __shared__ unsigned long long s_bits[kPlanWaves];
  __shared__ uint32_t s_last;
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int i = tid; i < a.bhs; i += kPlanThreads) s_len[i] = i < a.bklen ? a.book[i] >> 27 : 0u;
  __syncthreads();
  const uint32_t nblk = gridDim.x, b0 = blockIdx.x * kPlanBricks;
  unsigned long long wbits = 0;
  // every histogram of the wave's bricks is requested before the first is used: bhs <= 1024, two
  // 16-B loads (8 bins each) per lane and brick, bins past bhs (and bricks past the end) read 0
  constexpr int kPer = kPlanBricks / kPlanWaves;
  const int i0 = lane * 8, i1 = lane * 8 + 512;
  const __amdgpu_buffer_rsrc_t rh = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint16_t*>(a.bhist), 0, (int)min((size_t)a.nbricks * a.bhs * 2u, (size_t)0x7FFFFFFF), (int)kBufRsrcW3);
  u32x4 hv[kPer][2];
#pragma unroll
  for (int j = 0; j < kPer; j++) {
    const uint32_t brick = b0 + wid * kPer + j;
    const uint32_t hb = brick * (uint32_t)a.bhs * 2u;
    hv[j][0] = __builtin_amdgcn_raw_buffer_load_b128(rh, (int)(brick < a.nbricks && i0 < a.bhs ? hb + i0 * 2u : kOOB), 0, 0);
    hv[j][1] = __builtin_amdgcn_raw_buffer_load_b128(rh, (int)(brick < a.nbricks && i1 < a.bhs ? hb + i1 * 2u : kOOB), 0, 0);
  }
#pragma unroll
  for (int j = 0; j < kPer; j++) {
    const uint32_t slot = wid * kPer + j, brick = b0 + slot;
    uint32_t ub = 0, oc = 0;
    if (brick < a.nbricks) {
      uint32_t bits = 0;
      const uint32_t w[8] = {hv[j][0].x, hv[j][0].y, hv[j][0].z, hv[j][0].w, hv[j][1].x, hv[j][1].y, hv[j][1].z, hv[j][1].w};
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const int i = (k < 4 ? i0 : i1) + 2 * (k & 3);
        if (i < a.bhs) bits += (w[k] & 0xFFFFu) * s_len[i] + (w[k] >> 16) * s_len[i + 1];
      }
      bits = readlane(hfd::wave_incl_scan(bits), 63);  // DPP, no LDS round trips
      wbits += bits;
      // chunks of the brick: each may end with a partial cell
      const uint32_t rows = a.nd == 1 ? min(64u, a.nchunks - 64u * brick) : brick_rows3(brick, a.nbx, a.nby, a.ly, a.lz);
      ub = (bits + 31u * rows) >> 5;
      const uint32_t bc = a.brick_cnt[brick];
      oc = min(bc, a.cap_per_brick);
      if (bc > a.cap_per_brick && lane == 0) atomicMax(&a.info->max_brick_cnt, bc);  // slot growth
    }
    if (lane == 0) s_ub[slot] = ub, s_oc[slot] = oc;
  }
  if (lane == 0) s_bits[wid] = wbits;
  __syncthreads();
  if (wid == 0) {  // one brick per lane (lanes < kPlanBricks)
    const bool in = lane < kPlanBricks;
    const uint32_t ub = in ? s_ub[lane] : 0u, oc = in ? s_oc[lane] : 0u;
    const uint32_t iu = hfd::wave_incl_scan(ub), io = hfd::wave_incl_scan(oc);
    const uint32_t brick = b0 + lane;
    if (in && brick < a.nbricks) a.ub[brick] = ub, a.cell_local[brick] = iu - ub, a.ol_local[brick] = io - oc;
    if (lane == 63) {
      atomicExch(a.cell_pre + blockIdx.x, iu);
      atomicExch(a.ol_pre + blockIdx.x, io);
      unsigned long long tb = 0;
      for (int w = 0; w < kPlanWaves; w++) tb += s_bits[w];
      atomicAdd(&a.info->total_nbit, tb);
      // two-level ticket (pub_device.hh): blocks by blockIdx % 8, then the groups' last ones
      const uint32_t g = blockIdx.x % kPubGroups;
      const uint32_t in_group = nblk / kPubGroups + (g < nblk % kPubGroups ? 1u : 0u);
      const uint32_t groups = nblk < kPubGroups ? nblk : kPubGroups;
      bool last = false;
      if (__hip_atomic_fetch_add(a.ticket + g, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == in_group - 1)
        last = __hip_atomic_fetch_add(a.ticket + kPubGroups, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == groups - 1;
      s_last = last;
    }
  }
  __syncthreads();
  if (!s_last) return;
  // last block: exclusive scans of the block totals (read back by atomics: other XCDs' L2s)
  __shared__ uint32_t s_wsum[2][kPlanWaves];
  __shared__ uint32_t s_carry[2];
  if (tid < 2) s_carry[tid] = 0;
  __syncthreads();
  for (uint32_t c0 = 0; c0 < nblk; c0 += kPlanThreads) {
    const uint32_t i = c0 + tid;
    const uint32_t vc = i < nblk ? atomicAdd(a.cell_pre + i, 0u) : 0u;
    const uint32_t vo = i < nblk ? atomicAdd(a.ol_pre + i, 0u) : 0u;
    const uint32_t ic = hfd::wave_incl_scan(vc), io = hfd::wave_incl_scan(vo);
    if (lane == 63) s_wsum[0][wid] = ic, s_wsum[1][wid] = io;
    __syncthreads();
    uint32_t oc = s_carry[0], oo = s_carry[1];
    for (int w = 0; w < wid; w++) oc += s_wsum[0][w], oo += s_wsum[1][w];
    if (i < nblk) a.cell_pre[i] = oc + ic - vc, a.ol_pre[i] = oo + io - vo;
    __syncthreads();
    if (tid == kPlanThreads - 1) s_carry[0] = oc + ic, s_carry[1] = oo + io;
    __syncthreads();
  }
  if (tid == 0) {
    const unsigned long long ncell = s_carry[0], slot_total = s_carry[1];
    a.cell_pre[nblk] = (uint32_t)ncell;
    a.ol_pre[nblk] = (uint32_t)slot_total;
    const uint32_t sp = *a.spill_cnt;
    const uint32_t sp_kept = sp < a.spill_cap ? sp : a.spill_cap;
    const unsigned long long nbit = __hip_atomic_load(&a.info->total_nbit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    a.info->total_ncell = ncell;
    a.info->splen = slot_total + sp_kept;
    a.info->outlier_lost = sp > a.spill_cap ? sp - a.spill_cap : 0u;
    a.info->spilled = sp;
    write_headers_dev(a.archive, tpl, nbit, ncell, slot_total + sp_kept, a.phf_offset, a.bitstream_rel);
  }
}

// =========================================================================================
// pass 2: predict -> codewords -> one chunk per brick row, written at the brick's region
// =========================================================================================
constexpr int kPackCells = 768;  // per-wave LDS cell buffer (words): rows accumulate until a flush
static_assert(kPackCells >= 2 * kPackRowMax, "a flush every row or two at worst");

// Pass 2 packs the brick's rows from the codes pass 1 left in brick order (row r of brick b at
// (b * 64 + r) * W): per row, codewords (byte rows through a 256-entry table of the byte window)
// -> wave scan of their lengths -> MSB-first packing into the wave's LDS cell buffer (each row
// starts a new cell, hf_kernels.cuhip.inl:97-157).  Rows accumulate back to back in the buffer;
// it is copied to the brick's region in coalesced 256-B stores when the next row might not fit
// and at the brick's end.  Each row's load is issued when the same z of the previous y-step is
// consumed (8 rows in flight).  The loop is VALU-issue-bound (SQ counters: VALU busy ~75 % of
// the kernel), so a row is kept to ~40 VALU: LDS tables at static addresses (their offsets fold
// into the ds immediates), bricks inside the field take a path with no row checks, lanes pack
// left-justified words with no exec masking, one lane records the row's size and entry in LDS.  ~60 VGPRs:
// 8 waves per SIMD.  Bricks are walked last to first: pass 1 wrote the last bricks' code rows
// last, so pass 2 starts on what is still in the cache.
template <int ND>
__global__ void __launch_bounds__(64 * kBrickWaves) __attribute__((amdgpu_waves_per_eu(8)))
k_brick3_pack(BrickCodes bcs, uint32_t ly, uint32_t lz, const uint32_t* __restrict__ book,
              int bklen, BrickPlanArgs pl, uint32_t* __restrict__ par_nbit, uint32_t* __restrict__ par_entry,
              uint32_t* __restrict__ bitstream, uint32_t nbx, uint32_t nby, uint32_t nbricks,
              unsigned int* overflow, HostPub pub)
{
  constexpr int V = kBrickV, W = kBrickW;  // 8-B code loads
  __shared__ uint32_t s_book[kMaxBklen];  // book word by code
  __shared__ uint32_t s_b8[256];          // book word by byte code (255: code 0)
  __shared__ uint32_t s_cells[kBrickWaves][kPackCells];
  __shared__ uint2 s_rowinfo[kBrickWaves][64];  // per row of the wave's brick: bits, first cell
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wid: uniform (SGPR)
  uint32_t* const cells = s_cells[wid];
  const uint32_t nw = gridDim.x * kBrickWaves;  // (read before the divergent fill loops)
  for (int i = threadIdx.x; i < bklen; i += 64 * kBrickWaves) s_book[i] = book[i];
  for (int i = threadIdx.x; i < 256; i += 64 * kBrickWaves) {
    const uint32_t c = i == 255 ? 0u : (uint32_t)i + bcs.c0;
    s_b8[i] = c < (uint32_t)bklen ? book[c] : 0u;
  }
  for (int i = lane; i < kPackCells; i += 64) cells[i] = 0;
  __syncthreads();
  const uint32_t ncell = pl.cell_pre[pl.nblk];
  uint2* ol_dst = reinterpret_cast<uint2*>(bitstream + ncell);  // outlier cells follow the bitstream
  {  // spill list (bricks past their slot; not expected below 10 % outliers) after every slot
    const uint32_t slot_total = pl.ol_pre[pl.nblk], sp = min(*pl.spill_cnt, pl.spill_cap);
    for (uint32_t i = (blockIdx.x * kBrickWaves + wid) * 64 + lane; i < sp; i += nw * 64) {
      const uint64_t c = pl.spill[i];
      ol_dst[slot_total + i] = make_uint2((uint32_t)c, (uint32_t)(c >> 32));
    }
  }
  const uint32_t lo8 = (uint32_t)lane * 8u, lo4 = (uint32_t)lane * 4u;
  for (uint32_t it = blockIdx.x * kBrickWaves + wid; it < nbricks; it += nw) {
    const uint32_t brick = nbricks - 1 - it;
    const uint32_t pb = brick / kPlanBricks;
    // (uniform values loaded per lane: read back as scalars)
    const uint32_t base = (uint32_t)__builtin_amdgcn_readfirstlane((int)(pl.cell_local[brick] + pl.cell_pre[pb]));
    const uint32_t lim = (uint32_t)__builtin_amdgcn_readfirstlane((int)pl.ub[brick]);
    {  // this brick's outlier slot -> the archive's outlier segment (brick order)
      const uint32_t cnt = min(pl.brick_cnt[brick], pl.cap_per_brick);
      const uint64_t* slot = pl.slots + (size_t)brick * pl.cap_per_brick;
      uint2* d = ol_dst + pl.ol_local[brick] + pl.ol_pre[pb];
      for (uint32_t i = lane; i < cnt; i += 64) {
        const uint64_t c = slot[i];
        d[i] = make_uint2((uint32_t)c, (uint32_t)(c >> 32));
      }
    }
    uint32_t* dst = bitstream + base;
    uint32_t off = 0;    // region words packed (buffered or copied)
    uint32_t fbase = 0;  // region word at the buffer's start
    // buffered words [fbase, off) -> the region (never past lim: the region is an upper bound, so
    // the clamp only guards a corrupt plan), buffer cleared
    auto flush = [&]() {
      hfd::wave_sync();
      const uint32_t n = off - fbase, nst = fbase >= lim ? 0u : min(n, lim - fbase);
      for (uint32_t i0 = 0; i0 < n; i0 += 64) {  // uniform trip count
        const uint32_t i = i0 + (uint32_t)lane;
        if (i < n) {
          const uint32_t v = cells[i];
          cells[i] = 0;
          if (i < nst) dst[fbase + i] = v;
        }
      }
      fbase = off;
      hfd::wave_sync();
    };
    const uint32_t bx = brick % nbx, t = brick / nbx, by = t % nby, bz = t / nby;
    const uint32_t y0 = by * 8, z0 = bz * 8;
    // 1-D: rows [0, nrow) of the brick are chunks 64 brick + row (row = 8 y + z)
    const uint32_t nrow = ND == 1 ? min(64u, pl.nchunks - 64u * brick) : 64u;
    const uint32_t nyv = ND == 1 ? (nrow + 7u) / 8u : min(8u, ly - y0), nzv = ND == 1 ? 8u : min(8u, lz - z0);
    const uint8_t* src16 = reinterpret_cast<const uint8_t*>(bcs.c16 + (size_t)brick * 64 * W);
    const uint8_t* src8 = bcs.c8 + (size_t)brick * 64 * W;
    const uint64_t rm = ((uint64_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)bcs.rowmask[brick]) & 0xFFFFFFFFull) |
                        ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(bcs.rowmask[brick] >> 32)) << 32);
    // row r: 8 u16 bytes per lane when bit r of rm is set, else 4 code bytes (.x); one 8-B load
    // either way (a byte row's lane reads its neighbour's 4 bytes too: no branch around loads);
    // the row's base is uniform, the lane's offset one of two registers
    auto load_row = [&](uint32_t row) -> uint2 {
      const bool wide = (rm >> row) & 1ull;
      const uint8_t* a = (wide ? src16 + (size_t)row * (2 * W) : src8 + (size_t)row * W) + (wide ? lo8 : lo4);
      uint2 v;
      __builtin_memcpy(&v, a, 8);
      return v;
    };
    // full: every row of the brick lies in the field (no row checks, no short chunk)
    const bool full = ND == 1 ? nrow == 64u && pl.n - (size_t)brick * 64u * W >= 64u * W
                              : nyv == 8u && nzv == 8u;
    // Packing order: 3-D, the rows in order.  1-D, position k holds row 4 (k mod 16) + k / 16:
    // the brick's 16 tiles' chunks of one phase are adjacent, as the 1-D decoder's lanes read
    // them (lane = tile, phase p = the tile's chunk p: k_brick1_decode), so neighbouring lanes
    // share cache lines instead of reading chunks 4 apart.  par_entry records the placement.
    auto prow = [](uint32_t k) -> uint32_t { return ND == 1 ? 4u * (k & 15u) + (k >> 4) : k; };
    auto row_ok = [&](uint32_t row) { return ND == 1 ? row < nrow : (row & 7u) < nzv; };
    // Straight-line row loop (no branch around a load: the compiler then waits for each row's
    // own load, not for all of them): every row's load is issued, rows outside the field read
    // a row of the brick's own code block and pack nothing.
    uint2 qv[8];
#pragma unroll
    for (int z = 0; z < 8; z++) qv[z] = load_row(prow(z));
    for (uint32_t y = 0; y < (ND == 1 ? 8u : nyv); y++) {
#pragma unroll
      for (int z = 0; z < 8; z++) {
        const uint32_t k = y * 8 + z, row = prow(k);
        if (off - fbase + kPackRowMax > kPackCells) flush();
        uint32_t w[V];
        if ((rm >> row) & 1ull) {
          w[0] = s_book[qv[z].x & 0xFFFFu], w[1] = s_book[qv[z].x >> 16];
          w[2] = s_book[qv[z].y & 0xFFFFu], w[3] = s_book[qv[z].y >> 16];
        }
        else {
#pragma unroll
          for (int k = 0; k < V; k++) w[k] = s_b8[(qv[z].x >> (8 * k)) & 255u];
        }
        qv[z] = load_row(prow((k + 8) & 63u));
        if (__builtin_expect(!full, 0)) {
          asm volatile("" ::: "memory");  // a real branch: full bricks run no selects here
          if (!row_ok(row)) {
#pragma unroll
            for (int k = 0; k < V; k++) w[k] = 0;
          }
          // 1-D: the field's last chunk may be short; codes past its end get no codeword
          if (ND == 1) {
            const size_t cfirst = ((size_t)brick * 64u + row) * W;
            if (pl.n - cfirst < (size_t)W)
#pragma unroll
              for (int k = 0; k < V; k++)
                if (cfirst + (uint32_t)lane * V + k >= pl.n) w[k] = 0;
          }
        }
        uint32_t bits = 0;
#pragma unroll
        for (int k = 0; k < V; k++) bits += w[k] >> 27;
        const uint32_t inc = hfd::wave_incl_scan(bits);
        const uint32_t tot = readlane(inc, 63);
        const uint32_t pos = ((off - fbase) << 5) + inc - bits;
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(bits > 64u) == 0, 1))
          hfd::pack4_or_lj(cells, pos, w, bits);
        else
          hfd::pack_words<V>(cells, pos, w, V);
        if (lane == 0) s_rowinfo[wid][row] = make_uint2(tot, base + off);  // the row's bits and first cell
        off += (tot + 31) >> 5;
      }
    }
    flush();  // (ends with a wave sync: every row's info is in)
    const uint32_t ry = lane >> 3, rz = lane & 7;
    const bool lane_ok = ND == 1 ? (uint32_t)lane < nrow : ry < nyv && rz < nzv;
    if (lane_ok) {
      const uint2 ri = s_rowinfo[wid][lane];
      const size_t c = ND == 1 ? (size_t)brick * 64u + (uint32_t)lane : ((size_t)(z0 + rz) * ly + (y0 + ry)) * nbx + bx;
      par_nbit[c] = ri.x;
      par_entry[c] = ri.y;
    }
    if (off > lim && lane == 0) atomicOr(overflow, 1u);  // cannot happen (region is an upper bound)
    for (uint32_t i = off + lane; i < lim; i += 64) dst[i] = 0u;
  }
  // the workgroup that finishes last publishes the compress summary (header, totals, status)
  publish_last(pub);
}

}  // namespace

int launch_brick_plan(const BrickLaunch& L, const BrickPlanArgs& a, const void* psz_tpl, const void* phf_tpl,
                      hipStream_t st)
{
  HeaderTpl t;
  __builtin_memcpy(t.psz, psz_tpl, 176);
  __builtin_memcpy(t.phf, phf_tpl, 64);
  k_brick_plan<<<a.nblk, kPlanThreads, 0, st>>>(a, t);
  return (int)hipGetLastError();
}

uint32_t brick_plan_blocks(uint32_t nbricks) { return (nbricks + kPlanBricks - 1) / kPlanBricks; }

int launch_brick_pack(const BrickLaunch& L, const BrickCodes& bcodes, const uint32_t* book, int bklen,
                      const BrickPlanArgs& plan, uint32_t* par_nbit, uint32_t* par_entry, uint32_t* bitstream,
                      unsigned int* overflow, hipStream_t st, const HostPub& pub)
{
  const BrickGeom& g = L.g;
  const size_t lds = 0;  // static LDS only
  if (g.ndim != 3)
    k_brick3_pack<1><<<L.grid_pack, 64 * kBrickWaves, lds, st>>>(bcodes, L.ly, L.lz, book, bklen, plan, par_nbit, par_entry,
                                                                 bitstream, g.nbx, g.nby, g.nbricks, overflow, pub);
  else
    k_brick3_pack<3><<<L.grid_pack, 64 * kBrickWaves, lds, st>>>(bcodes, L.ly, L.lz, book, bklen, plan, par_nbit, par_entry,
                                                                 bitstream, g.nbx, g.nby, g.nbricks, overflow, pub);
  return (int)hipGetLastError();
}

int brick_pack_blocks_per_cu()
{
  int per_cu = 0;  // static LDS only
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_brick3_pack<3>, 64 * kBrickWaves, 0) != hipSuccess) return 0;
  return per_cu;
}

}  // namespace cusz_amd
