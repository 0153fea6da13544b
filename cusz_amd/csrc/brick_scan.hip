// cusz_amd/csrc/brick_scan.hip -- pass 1 of the fused brick compressor (overview: brick_device.hh):
// k_brick3_scan (3-D) and k_brick1_scan (1-D, 2-D) predict the field once and leave the codes in
// brick order, the per-brick and global histograms, the outlier slots and the codebook sample; and
// the host side of the brick layout: brick_geom, brick_configure, brick_sample_plan.
#include "brick_device.hh"

namespace cusz_amd {

namespace {

// per-brick u16 histograms are stored at a stride of whole 16-B groups (the plan kernel's loads)
__host__ __device__ constexpr int bhist_stride(int bklen) { return (bklen + 7) & ~7; }

// one 8-B store per lane and row
__device__ __forceinline__ void store_codes_row(uint16_t* p, const uint16_t (&q)[kBrickV])
{
  uint2 w;
  w.x = (uint32_t)q[0] | ((uint32_t)q[1] << 16);
  w.y = (uint32_t)q[2] | ((uint32_t)q[3] << 16);
  *reinterpret_cast<uint2*>(p) = w;
}

// One brick row of codes between the encode passes: bytes (code - c0, and 255 for the outlier
// code 0) when every code of the row fits [c0, c0 + 254] or is 0, else u16 with the row's bit set
// in the brick's row mask (BrickCodes).  Code 0 is always stored as 255 (never code - c0).
__device__ __forceinline__ void store_brick_row(const BrickCodes& bcs, uint16_t* cbrick, uint8_t* cbrick8, int row,
                                                const uint16_t (&qc)[kBrickV], uint64_t& rowmask)
{
  bool wide = false;
#pragma unroll
  for (int k = 0; k < kBrickV; k++) wide |= (uint32_t)qc[k] - bcs.c0 > 254u && qc[k] != 0;
  if (__builtin_amdgcn_ballot_w64(wide)) {
    store_codes_row(cbrick + (size_t)row * kBrickW, qc);
    rowmask |= 1ull << row;
  }
  else {  // one 4-B byte-code store per lane and row
    uint32_t w = 0;
#pragma unroll
    for (int k = 0; k < kBrickV; k++) w |= (qc[k] == 0 ? 255u : (uint32_t)qc[k] - bcs.c0) << (8 * k);
    *reinterpret_cast<uint32_t*>(cbrick8 + (size_t)row * kBrickW) = w;
  }
}

// Pass-1 visiting order (BrickSample): iteration j < count takes sample brick j stride + stride / 2,
// then the other bricks in index order (the k-th of them: group k / (stride - 1), skipping the
// group's sample position; stride - 1 is a power of two).  stride 1: index order.
__device__ __forceinline__ uint32_t pass1_brick(uint32_t j, const BrickSample& sp)
{
  if (sp.stride <= 1) return j;
  const uint32_t o = sp.stride / 2;
  if (j < sp.count) return j * sp.stride + o;
  const uint32_t k = j - sp.count, m = sp.stride - 2, g = k >> (31 - __builtin_clz(sp.stride - 1)), p = k & m;
  return g * sp.stride + (p < o ? p : p + 1);
}

// What only the wave completing the codebook sample needs of BrickSample.  The 3-D kernel keeps it
// in LDS, not in scalar registers live across the row loop (pass 1 spills scalars as it is).
struct SamplePub {
  uint32_t* dst;
  uint32_t* flag;
  uint32_t epoch, total;
};

// Pass 1's dynamic LDS: the workgroup histogram, then a brick histogram per wave (3-D: then SamplePub)
constexpr size_t scan_lds_bytes(int ndim)
{
  return (size_t)(1 + kBrickWaves) * kMaxBklen * 4 + (ndim == 3 ? sizeof(SamplePub) : 0);
}

// Start of a pass-1 kernel: the workgroup histogram (smem) and this wave's brick histogram
// (returned) are zeroed.
__device__ __forceinline__ uint32_t* scan_hist_begin(uint32_t* smem, int wid, int lane, int bklen)
{
  uint32_t* s_hist = smem + (1 + wid) * kMaxBklen;
  for (int i = threadIdx.x; i < bklen; i += blockDim.x) smem[i] = 0;
  for (int i = lane; i < bhist_stride(bklen); i += 64) s_hist[i] = 0;
  __syncthreads();
  return s_hist;
}

// End of a pass-1 kernel: the workgroup histogram -> the global one (once per workgroup); the
// workgroup that finishes last publishes it.
__device__ __forceinline__ void scan_hist_end(const uint32_t* s_wg, uint32_t* g_hist, int bklen, const HostPub& pub)
{
  __syncthreads();
  for (int i = threadIdx.x; i < bklen; i += blockDim.x) {
    const uint32_t c = s_wg[i];
    if (c) atomicAdd(&g_hist[i], c);
  }
  publish_last(pub);
}

// what finish_brick needs of its kernel, the same for every brick
struct ScanEnd {
  const OutlierSink& ol;
  const BrickCodes& bcs;
  uint32_t* s_hist;  // this wave's brick histogram
  uint32_t* s_wg;    // the workgroup's
  uint16_t* bhist;
  int hs, bklen, lane;
  const BrickSample& sp;
  const SamplePub& sb;
};

// End of a pass-1 brick: outlier count, row mask, the brick's histogram as a u16 record (16-B
// stores, 8 bins per lane; the wave's LDS copy is cleared) and into the workgroup histogram; a
// sample brick also adds it to the codebook sample (global atomics) and then counts itself done.
template <bool BY_VALUE>
__device__ __forceinline__ void finish_brick(const ScanEnd& e, uint32_t brick, uint32_t cnt, uint64_t rowmask, bool sample)
{
  if (e.lane == 0) e.ol.brick_cnt[brick] = cnt;
  if (e.lane == 0) e.bcs.rowmask[brick] = rowmask;
  hfd::wave_sync();
  uint16_t* bh = e.bhist + (size_t)brick * e.hs;
  for (int i0 = e.lane * 8; i0 < e.hs; i0 += 512) {
    uint32_t c[8];
#pragma unroll
    for (int k = 0; k < 8; k++) c[k] = e.s_hist[i0 + k];
#pragma unroll
    for (int k = 0; k < 8; k++) e.s_hist[i0 + k] = 0;
    *reinterpret_cast<uint4*>(bh + i0) =
        make_uint4(c[0] | c[1] << 16, c[2] | c[3] << 16, c[4] | c[5] << 16, c[6] | c[7] << 16);
#pragma unroll
    for (int k = 0; k < 8; k++)
      if (c[k]) atomicAdd(&e.s_wg[i0 + k], c[k]);
    if (sample)
#pragma unroll
      for (int k = 0; k < 8; k++)
        if (c[k]) atomicAdd(&e.sp.hist[(i0 + k) * kSampleBinStride], c[k]);
  }
  hfd::wave_sync();
  if (sample) {
    __builtin_amdgcn_s_waitcnt(0);  // this wave's sample atomics have completed
    uint32_t prev = 0;
    // 3-D bricks (BY_VALUE; sb.total: the sample's element count, known from the shape): the count
    // is relaxed, and the completing wave validates the sample by value.  Every bin only grows, by
    // whole atomic adds, and the sample is complete exactly when its bins sum to sb.total -- so a
    // read whose sum is sb.total has seen every sample brick's counts, by the atomicity and the
    // coherence of each bin alone; nothing rests on the order in which another XCD's atomics become
    // visible.  (A release per sample brick wrote back the XCD's L2, megabytes of dirty code rows,
    // 248 times a pass: +27 us of pass 1.)  The wave re-reads until the sum matches; the bound
    // (~0.1 s) only keeps a broken device from hanging the host.
    // Linear bricks: release / acquire at agent scope per sample brick, so that the completing
    // wave sees every sample brick's atomics by the memory model.
    if (e.lane == 0)
      prev = __hip_atomic_fetch_add(e.sp.hist + kMaxBklen * kSampleBinStride, 1u, BY_VALUE ? __ATOMIC_RELAXED : __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if ((uint32_t)__builtin_amdgcn_readfirstlane((int)prev) == e.sp.count - 1 && e.sb.flag) {
      // the sample is complete: this wave hands it to the host (agent-scope reads).  The host
      // pointers come out of LDS, so their address space is stated: as flat stores they would
      // turn the row loop's counted vmcnt waits into waits for everything (measured: +40 us)
      typedef __attribute__((address_space(1))) uint32_t global_u32;
      global_u32* const pub_dst = (global_u32*)e.sb.dst;
      global_u32* const pub_flag = (global_u32*)e.sb.flag;
      for (uint32_t tries = 0; tries < (1u << 16); tries++) {
        uint32_t sum = 0;
        for (int i = e.lane; i < e.bklen; i += 64) {
          const uint32_t v = __hip_atomic_load(e.sp.hist + i * kSampleBinStride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          pub_dst[i] = v;
          sum += v;
        }
        if (!BY_VALUE || readlane(hfd::wave_incl_scan(sum), 63) == e.sb.total) break;
        __builtin_amdgcn_s_sleep(32);
      }
      __threadfence_system();
      hfd::wave_sync();
      if (e.lane == 0) __hip_atomic_store(pub_flag, e.sb.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// =========================================================================================
// pass 1: predict -> histograms + outliers
// =========================================================================================
// Rows are streamed: one brick row (y, z) at a time, in (y, z) order, with the z-diff against
// the previous row of the same y-step and the y-diff against row (y - 1, z) kept in registers
// (bprev).  kScanAhead rows (one y-step) are in flight per wave, loaded into a register queue
// whose slot is the row's position modulo kScanAhead (the row loop is unrolled by kScanAhead, so
// the queue needs no copies); the loads run across brick boundaries.  f32: capped at 128 VGPRs
// (4 waves per SIMD: a 512^3 field's 8192 bricks are exactly two rounds of the 4096 waves).
constexpr int kScanAhead = 8;

template <typename T, bool ZZ>
__global__ void __launch_bounds__(64 * kBrickWaves)
__attribute__((amdgpu_waves_per_eu(sizeof(T) == 4 ? 3 : 1)))  // f32: <= 168 VGPRs, 3 waves per SIMD
k_brick3_scan(const T* __restrict__ in, uint32_t lx, uint32_t ly, uint32_t lz, T ebx2_r, T r, OutlierSink ol,
              uint32_t* __restrict__ g_hist, uint16_t* __restrict__ bhist, BrickCodes bcs, int bklen,
              uint32_t nbx, uint32_t nby, uint32_t nbricks, HostPub pub, BrickSample sp)
{
  constexpr int V = kBrickV, W = kBrickW;
  extern __shared__ uint32_t smem[];
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wid: uniform (SGPR)
  SamplePub& sb = *reinterpret_cast<SamplePub*>(smem + (1 + kBrickWaves) * kMaxBklen);  // after the histograms
  if (threadIdx.x == 0) sb = SamplePub{sp.pub_dst, sp.pub_flag, sp.pub_epoch, sp.total};
  uint32_t* s_hist = scan_hist_begin(smem, wid, lane, bklen);
  const uint32_t nw = gridDim.x * kBrickWaves;
  const StepLoader<T> ld{in, (size_t)lx * ly, lx, ly, lz, nbx, nby, nbricks, (uint32_t)lane};
  const size_t plane = ld.plane;
  const ScanEnd end{ol, bcs, s_hist, smem, bhist, bhist_stride(bklen), bklen, lane, sp, sb};
  constexpr int D = kScanAhead;
  static_assert(D == 8, "one y-step in flight: the rows ahead are one y-step of one brick");
  uint32_t it = blockIdx.x * kBrickWaves + wid;  // iteration; its brick in the pass-1 order (BrickSample)
  const T bias = r - (T)bcs.c0;  // the byte-first path (below)
  T q[D][V];
  {
    const auto b0 = ld.rows_of(it < nbricks ? pass1_brick(it, sp) : nbricks);
#pragma unroll
    for (int j = 0; j < D; j++) ld.issue_row(b0, (uint32_t)j >> 3, (uint32_t)j & 7u, q[j]);
  }
  for (; it < nbricks; it += nw) {
    uint32_t cnt = 0;
    uint64_t rowmask = 0;  // rows of the brick stored as u16 (uniform)
    const uint32_t brick = pass1_brick(it, sp);
    const uint32_t bnext = it + nw < nbricks ? pass1_brick(it + nw, sp) : nbricks;  // next brick of the stream
    const auto rc = ld.rows_of(brick), rn = ld.rows_of(bnext);
    const uint32_t bx = brick % nbx, t = brick / nbx, by = t % nby, bz = t / nby;
    const uint32_t x0 = bx * W + lane * V, y0 = by * 8, z0 = bz * 8;
    uint16_t* cbrick = bcs.c16 + (size_t)brick * 64 * W + (size_t)lane * V;
    uint8_t* cbrick8 = bcs.c8 + (size_t)brick * 64 * W + (size_t)lane * V;
    T bprev[8][V], pprev[V];
#pragma unroll
    for (int z = 0; z < 8; z++)
#pragma unroll
      for (int k = 0; k < V; k++) bprev[z][k] = (T)0;
#pragma unroll 1
    for (int r0 = 0; r0 < 64; r0 += D) {  // not unrolled: instruction cache
      const bool last = r0 + D >= 64;  // the rows ahead are the next brick's first y-step
      const auto ahead = last ? rn : rc;
      const uint32_t ya = last ? 0u : (uint32_t)(r0 + D) >> 3;
#pragma unroll
      for (int j = 0; j < D; j++) {
        const int row = r0 + j, z = j & 7, y = row >> 3;
        // lrz_c.cuhip.inl:341-352 order: z, then x inside the 8-wide tile, then y
        T a[V], d[V];
        residual_zx(q[j], ebx2_r, z == 0, x0 % 8 == 0, pprev, a);
        ld.issue_row(ahead, ya, (uint32_t)j & 7u, q[j]);  // row + D: y-step ya of `ahead`, z = j
        const uint32_t gy = y0 + (uint32_t)y;
#pragma unroll
        for (int k = 0; k < V; k++) {
          d[k] = a[k] - bprev[z][k];  // bprev = 0 on the brick's first y-step: a - 0 == a
          bprev[z][k] = a[k];
        }
        if (gy >= ly || z0 + (uint32_t)z >= lz) continue;  // outside the field (wave-uniform)
        float olv[V];
        uint16_t qc[V];
        uint64_t anyol = 0;  // SALU: OR of the per-element outlier lane masks
        if constexpr (!ZZ && sizeof(T) == 4) {
          // Byte-first quantization.  d is integer-valued, so for |d| < r the reference code
          // (int)(d + r) equals (int)(d + bias) + c0 (bias = r - c0, i.e. 127 unless r < 127) and
          // the byte is (int)(d + bias).
          // A row is clean when every element has |d| < r and a byte in [0, 254]: then the
          // bytes pack by shifts, the histogram bin is byte + c0, and nothing else is computed.
          // Any other row (an outlier, a NaN, a code outside the byte window) takes the exact path.
          int cib[V];
          bool q[V];
          uint64_t suspect = 0;
#pragma unroll
          for (int k = 0; k < V; k++) {
            cib[k] = (int)(d[k] + bias);
            q[k] = dabs(d[k]) < r;
            anyol |= __ballot(!q[k]);
            suspect |= __ballot((uint32_t)cib[k] > 254u);
          }
          if ((suspect | anyol) == 0) {
            uint32_t* s_hc0 = s_hist + bcs.c0;
#pragma unroll
            for (int k = 0; k < V; k++) atomicAdd(&s_hc0[cib[k]], 1u);
            *reinterpret_cast<uint32_t*>(cbrick8 + (size_t)row * W) =  // one 4-B byte store per lane and row
                (uint32_t)cib[0] | (uint32_t)cib[1] << 8 | (uint32_t)cib[2] << 16 | (uint32_t)cib[3] << 24;
            continue;
          }
#pragma unroll
          for (int k = 0; k < V; k++) {
            qc[k] = q[k] ? (uint16_t)(cib[k] + (int)bcs.c0) : uint16_t(0);
            olv[k] = (float)(d[k] + r);  // quantize(): the outlier value is d + r
            atomicAdd(&s_hist[qc[k]], 1u);
          }
        }
        else {
#pragma unroll
          for (int k = 0; k < V; k++) {
            bool is_ol;
            qc[k] = quantize<T, ZZ>(d[k], r, is_ol, olv[k]);
            anyol |= __ballot(is_ol);
            atomicAdd(&s_hist[qc[k]], 1u);
          }
        }
        store_brick_row(bcs, cbrick, cbrick8, row, qc, rowmask);
        if (anyol) {
          uint32_t mask = 0;
          size_t idx[V];
          const size_t base = (size_t)(z0 + z) * plane + (size_t)gy * lx;
#pragma unroll
          for (int k = 0; k < V; k++) {
            mask |= (uint32_t)(qc[k] == 0 && (ZZ ? !(dabs(d[k]) < r) : true)) << k;
            idx[k] = base + x0 + k;
          }
          emit_outliers<V>(ol, brick, cnt, mask, olv, idx);  // one slot per brick
        }
      }
    }
    finish_brick<true>(end, brick, cnt, rowmask, sp.hist && it < sp.count);
  }
  scan_hist_end(smem, g_hist, bklen, pub);
}

// 1-D pass 1 (lrz_c.cuhip.inl:23-109): a brick is 64 consecutive chunks of W = 256 (16 tiles
// of 1024), brick row r = chunk 64 b + r, so brick order is index order.  Lane l holds x in
// [4 l, 4 l + 4) of each row; the prequant of the element before the row's first comes from lane
// 63 of the previous row, 0 at a tile start.  Rows are loaded kScanAhead ahead (register queue,
// raw buffer loads from the brick's origin, past the field's end they read 0); codes, histograms,
// outlier slots and row masks as in the 3-D pass.
//
// 2-D fields use the same linear bricks (ND = 2, lx % 4 == 0, lx >= 256): the predictor is the
// reference's 2-D one (lrz_c.cuhip.inl:187-273, 32 x 32 tiles: a = p - p(north) unless y % 32 == 0,
// then d = a - a(west) unless x % 32 == 0), the north row coming from a second load queue.
template <typename T, bool ZZ, int ND>
__global__ void __launch_bounds__(64 * kBrickWaves)
k_brick1_scan(const T* __restrict__ in, size_t n, T ebx2_r, T r, OutlierSink ol, uint32_t* __restrict__ g_hist,
              uint16_t* __restrict__ bhist, BrickCodes bcs, int bklen, uint32_t nbricks, HostPub pub, uint32_t lx,
              BrickSample sp)
{
  constexpr int V = kBrickV, W = kBrickW;
  extern __shared__ uint32_t smem[];
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const SamplePub sb{sp.pub_dst, sp.pub_flag, sp.pub_epoch, 0u};
  uint32_t* s_hist = scan_hist_begin(smem, wid, lane, bklen);
  const uint32_t nw = gridDim.x * kBrickWaves;
  const ScanEnd end{ol, bcs, s_hist, smem, bhist, bhist_stride(bklen), bklen, lane, sp, sb};
  constexpr int D = kScanAhead;
  const LinearLoader<T> ld{in, n, nbricks, (uint32_t)lane};
  constexpr uint32_t kBE = LinearLoader<T>::kBrickElems;
  const uint32_t x0 = (uint32_t)lane * V;
  // 2-D: the north row (element i - lx) of the row issued, by a whole-field resource (the field is
  // < 2^31 bytes, brick_geom); rows on a tile's first line (y % 32 == 0) read 0 past its range.
  // (xi, yi) is the issue cursor of this lane's first element, (xl, yl) the compute cursor.
  const __amdgpu_buffer_rsrc_t rsall =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(in), 0, (int)(ND == 2 ? n * sizeof(T) : 0), (int)kBufRsrcW3);
  uint32_t xi = 0, yi = 0;
  auto cursor_at = [&](uint32_t b, uint32_t& x, uint32_t& y) {
    const size_t i = (size_t)b * kBE + x0;
    x = (uint32_t)(i % lx), y = (uint32_t)(i / lx);
  };
  auto advance = [&](uint32_t& x, uint32_t& y) {  // next row: + W elements (lx >= W)
    x += W;
    if (x >= lx) x -= lx, y++;
  };
  auto issue_north = [&](uint32_t b, uint32_t x, uint32_t y, T (&dst)[V]) {
    const size_t i = (size_t)y * lx + x;
    buffer_load4<T, 0>(rsall, (b < nbricks && y % 32u != 0u) ? (uint32_t)((i - lx) * sizeof(T)) : kOOB, dst);
  };
  uint32_t it = blockIdx.x * kBrickWaves + wid;  // iteration; its brick in the pass-1 order (BrickSample)
  T q[D][V];
  T qn[ND == 2 ? D : 1][V];
  {
    const uint32_t b0 = it < nbricks ? pass1_brick(it, sp) : nbricks;
    if constexpr (ND == 2) cursor_at(b0, xi, yi);
    const __amdgpu_buffer_rsrc_t r0s = ld.rows_of(b0);
#pragma unroll
    for (int j = 0; j < D; j++) {
      ld.issue_row(r0s, j, q[j]);
      if constexpr (ND == 2) {
        issue_north(b0, xi, yi, qn[j]);
        advance(xi, yi);
      }
    }
  }
  for (; it < nbricks; it += nw) {
    const uint32_t brick = pass1_brick(it, sp), bnext = it + nw < nbricks ? pass1_brick(it + nw, sp) : nbricks;
    uint32_t cnt = 0;
    uint64_t rowmask = 0;
    const size_t bbase = (size_t)brick * kBE;
    const bool full = n - bbase >= kBE;  // no element past the field's end (uniform)
    uint16_t* cbrick = bcs.c16 + bbase + x0;
    uint8_t* cbrick8 = bcs.c8 + bbase + x0;
    T carry = 0;  // 1-D: prequant, 2-D: y-difference, of the previous row's last element
    uint32_t xl = 0, yl = 0;
    if constexpr (ND == 2) {
      cursor_at(brick, xl, yl);
      // a brick starts on a 1-D tile boundary, not on a 2-D one: the element before it belongs
      // to the previous brick (a is needed when it lies in the same 32-wide tile row)
      if (bbase > 0) {
        const size_t i = bbase - 1;
        const uint32_t y = (uint32_t)(i / lx);
        T a = dround(in[i] * ebx2_r);
        if (y % 32u != 0u) a = a - dround(in[i - lx] * ebx2_r);
        carry = a;
      }
    }
    const __amdgpu_buffer_rsrc_t rc = ld.rows_of(brick), rn = ld.rows_of(bnext);
    static_assert(64 % D == 0, "the rows ahead of a D-row block lie in one brick");
#pragma unroll 1
    for (int r0 = 0; r0 < 64; r0 += D) {
      const bool tail = r0 + D >= 64;  // the rows ahead are the next brick's first rows
      const __amdgpu_buffer_rsrc_t ahead = tail ? rn : rc;
      const int ra = tail ? r0 + D - 64 : r0 + D;
#pragma unroll
      for (int j = 0; j < D; j++) {
        const int row = r0 + j;
        T p[V];
#pragma unroll
        for (int k = 0; k < V; k++) p[k] = dround(q[j][k] * ebx2_r);
        if constexpr (ND == 2) {  // a = p - p(north): 0 past the field / on a tile's first line
#pragma unroll
          for (int k = 0; k < V; k++) p[k] = p[k] - dround(qn[j][k] * ebx2_r);
        }
        const uint32_t bahead = row + D < 64 ? brick : bnext;
        ld.issue_row(ahead, ra + j, q[j]);
        if constexpr (ND == 2) {
          if (row + D == 64) cursor_at(bnext, xi, yi);  // the queue moves on to the next brick
          issue_north(bahead, xi, yi, qn[j]);
          advance(xi, yi);
        }
        const size_t base = bbase + (size_t)row * W;
        T west = __shfl_up(p[V - 1], 1);
        const T last = __shfl(p[V - 1], 63);
        if (lane == 0) west = (ND == 2 || (row & 3)) ? carry : T(0);
        carry = last;
        const uint32_t xcur = xl;
        if constexpr (ND == 2) advance(xl, yl);
        if (!full && base >= n) continue;  // past the field's end (uniform)
        T d[V];
#pragma unroll
        for (int k = V - 1; k > 0; k--) d[k] = p[k] - p[k - 1];
        if constexpr (ND == 2)
          d[0] = (xcur % 32u != 0u) ? p[0] - west : p[0];  // x % 32 == 0: a tile's first column
        else
          d[0] = p[0] - west;
        float olv[V];
        uint16_t qc[V];
        uint32_t mask = 0;
#pragma unroll
        for (int k = 0; k < V; k++) {
          bool is_ol;
          qc[k] = quantize<T, ZZ>(d[k], r, is_ol, olv[k]);
          const bool inr = full || base + x0 + k < n;
          if (inr) atomicAdd(&s_hist[qc[k]], 1u);
          mask |= (uint32_t)(inr && is_ol) << k;
        }
        store_brick_row(bcs, cbrick, cbrick8, row, qc, rowmask);
        if (__builtin_amdgcn_ballot_w64(mask != 0)) {
          size_t idx[V];
#pragma unroll
          for (int k = 0; k < V; k++) idx[k] = base + x0 + k;
          emit_outliers<V>(ol, brick, cnt, mask, olv, idx);
        }
      }
    }
    finish_brick<false>(end, brick, cnt, rowmask, sp.hist && it < sp.count);
  }
  scan_hist_end(smem, g_hist, bklen, pub);
}

}  // namespace

BrickSample brick_sample_plan(const BrickLaunch& L, uint32_t* hist)
{
  const uint32_t nbricks = L.g.nbricks;
  BrickSample s;
  s.hist = hist, s.total = L.sample_total;
  // stride - 1 a power of two (the order's arithmetic); ~256 sample bricks where possible (a
  // 512^3 field: every 33rd brick, 4 M codes -- the book's bits +0.001 % against every 17th, and
  // pass 1 adds half the sample atomics: -6 us)
  s.stride = nbricks >= 8192 ? 33u : nbricks >= 4352 ? 17u : nbricks >= 2304 ? 9u : nbricks >= 1280 ? 5u : nbricks >= 768 ? 3u : 1u;
  const uint32_t o = s.stride / 2;
  s.count = s.stride == 1 ? nbricks : (nbricks > o ? (nbricks - o + s.stride - 1) / s.stride : 0u);
  return s;
}

// =========================================================================================
// host launchers
// =========================================================================================

BrickGeom brick_geom(int ndim, size_t lx, size_t ly, size_t lz, int elem_bytes)
{
  BrickGeom g{};
  g.V = kBrickV, g.W = kBrickW;  // W = 256: f32 16-B loads, f64 32-B loads per lane
  g.ndim = ndim;
  g.n = lx * ly * lz;
  if (ndim == 1 || ndim == 2) {  // linear bricks (2-D: x extent a multiple of 4, >= 256; < 2 GiB)
    g.ok = g.n < (1ull << 32) && (elem_bytes == 4 || elem_bytes == 8) &&
           (ndim == 1 || (lx % 4 == 0 && lx >= (size_t)g.W && g.n * elem_bytes < (1ull << 31)));
    if (!g.ok) return g;
    g.brick_elems = (uint32_t)g.W * 64;
    g.nbricks = (uint32_t)((g.n + g.brick_elems - 1) / g.brick_elems);
    g.nbx = g.nbricks, g.nby = 1, g.nbz = 1;
    g.nchunks = (uint32_t)((g.n + g.W - 1) / g.W);
    return g;
  }
  g.ok = ndim == 3 && lx % (size_t)g.W == 0 && lx * ly * lz < (1ull << 32) && (elem_bytes == 4 || elem_bytes == 8) &&
         8 * lx * ly * (size_t)elem_bytes < (1ull << 31);  // 32-bit buffer offsets within 8 planes
  if (!g.ok) return g;
  g.nbx = (uint32_t)(lx / g.W);
  g.nby = (uint32_t)((ly + 7) / 8);
  g.nbz = (uint32_t)((lz + 7) / 8);
  g.nbricks = g.nbx * g.nby * g.nbz;
  g.brick_elems = (uint32_t)g.W * 64;
  g.nchunks = (uint32_t)(lx / g.W * ly * lz);
  return g;
}

int brick_configure(BrickLaunch& L, int elem_bytes, int device)
{
  int ncu = 0;
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || ncu < 1) ncu = 256;
  L.ncu = ncu;
  int per_scan = 0, per_pack = brick_pack_blocks_per_cu();
  const size_t lds_scan = scan_lds_bytes(3);  // (the 3-D kernel sizes the grid of the linear ones too)
  hipError_t e1;
  if (elem_bytes == 8)
    e1 = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_scan, k_brick3_scan<double, false>, 64 * kBrickWaves, lds_scan);
  else
    e1 = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_scan, k_brick3_scan<float, false>, 64 * kBrickWaves, lds_scan);
  if (e1 != hipSuccess || per_scan < 1) per_scan = 1;
  if (per_pack < 1) per_pack = 1;
  const int need = (int)((L.g.nbricks + kBrickWaves - 1) / kBrickWaves);
  L.grid_scan = need < per_scan * ncu ? need : per_scan * ncu;
  L.grid_pack = need < per_pack * ncu ? need : per_pack * ncu;
  if (L.grid_scan < 1) L.grid_scan = 1;
  if (L.grid_pack < 1) L.grid_pack = 1;
  // the codebook sample's element count (finish_brick validates the completed sample against it):
  // pass 1 counts the rows of a brick that lie inside the field, whole in x
  L.sample_total = 0;
  if (L.g.ndim == 3) {
    const BrickGeom& g = L.g;
    const BrickSample s = brick_sample_plan(L, nullptr);
    uint64_t rows = 0;
    for (uint32_t j = 0; j < s.count; j++) {
      const uint32_t t = (s.stride <= 1 ? j : j * s.stride + s.stride / 2) / g.nbx, by = t % g.nby, bz = t / g.nby;
      rows += (uint64_t)std::min(8u, L.ly - by * 8) * std::min(8u, L.lz - bz * 8);
    }
    L.sample_total = (uint32_t)(rows * (uint64_t)g.W);  // < 2^32: the field is
  }
  return (int)hipSuccess;
}

template <typename T>
int launch_brick_scan(const BrickLaunch& L, const T* in, double eb, int radius, bool zz, const BrickSample& sample,
                      const OutlierSink& ol, uint32_t* hist, uint16_t* bhist, const BrickCodes& bcodes, int bklen,
                      hipStream_t st, const HostPub& pub)
{
  const T ebx2_r = (T)(1.0 / (eb * 2));  // lrz_c.cuhip.inl:489
  const T r = (T)radius;
  const BrickGeom& g = L.g;
  const size_t lds = scan_lds_bytes(g.ndim);
  const int grid = L.grid_scan;
  if (g.ndim == 1 || g.ndim == 2) {
#define SCAN1(ZZ, ND)                                                                                           \
  k_brick1_scan<T, ZZ, ND><<<grid, 64 * kBrickWaves, lds, st>>>(in, g.n, ebx2_r, r, ol, hist, bhist, bcodes, bklen, \
                                                                g.nbricks, pub, L.lx, sample)
    if (g.ndim == 1) {
      if (zz) SCAN1(true, 1); else SCAN1(false, 1);
    }
    else {
      if (zz) SCAN1(true, 2); else SCAN1(false, 2);
    }
#undef SCAN1
    return (int)hipGetLastError();
  }
  if (zz)
    k_brick3_scan<T, true><<<grid, 64 * kBrickWaves, lds, st>>>(in, L.lx, L.ly, L.lz, ebx2_r, r, ol, hist, bhist, bcodes,
                                                                bklen, g.nbx, g.nby, g.nbricks, pub, sample);
  else
    k_brick3_scan<T, false><<<grid, 64 * kBrickWaves, lds, st>>>(in, L.lx, L.ly, L.lz, ebx2_r, r, ol, hist, bhist, bcodes,
                                                                 bklen, g.nbx, g.nby, g.nbricks, pub, sample);
  return (int)hipGetLastError();
}

int brick_hist_stride(int bklen) { return bhist_stride(bklen); }

#define INST(T)                                                                                                   \
  template int launch_brick_scan<T>(const BrickLaunch&, const T*, double, int, bool, const BrickSample&,            \
                                    const OutlierSink&, uint32_t*, uint16_t*, const BrickCodes&, int, hipStream_t,   \
                                    const HostPub&);
INST(float)
INST(double)
#undef INST

}  // namespace cusz_amd
